"""``--module=bcgru`` plugin: conv-emotion's bc-GRU baseline (reference: GRUModel, track_mm/dgcnv2_models.py:350-386, and
MaskedNLLLoss :13-33).  The reference has no plugin file of its own for it; the defaults are those of ``--module=bclstm``
(track_mm/dgcnv2.py:22-48)."""
from functools import partial

from erc_amd.bcrnn import BcGruTrainer, GRUModule  # noqa: F401
from erc_amd.trainer import run
from track_mm.bclstm import BcRnnParams

ParamsType = BcRnnParams
main = partial(run, BcGruTrainer, ParamsType)
