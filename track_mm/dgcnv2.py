"""``--module=dgcnv2`` plugin: the conv-emotion DialogueGCN (reference: track_mm/dgcnv2.py:22-48,184-219)."""
from functools import partial

from erc_amd.dgcnv2 import DGCNModule, DGCNv2Trainer  # noqa: F401
from erc_amd.params import ERCParams, Group
from erc_amd.trainer import run


class DGCNParams(ERCParams):
    def __init__(self):
        super().__init__()
        self.train.batch_size = self.val.batch_size = self.test.batch_size = 32   # dgcnv2.py:28-30
        self.base_model = "LSTM"                                                  # dgcnv2.py:32 (first of the choice)
        self.dataset = "iemocap-cogmen-6"
        self.epoch = 55
        self.optim = Group(name="Adam", lr=0.0003, weight_decay=0)                # dgcnv2.py:37
        self.loss_weights = True                                                  # dgcnv2.py:42
        self.speaker_onehot, self.batch_first = True, False                       # dgcnv2.py:43-44
        self.dropout = 0.4                                                        # DGCNModule's default (dgcnv2.py:62)
        # capacity buckets (one captured graph per padded (B, T, N) bucket instead of per exact shape) are opt-in here:
        # --capacity_buckets=True, or --resident (with --device_collate), which implies them; --resident_eval with --resident
        self.capacity_buckets = False


ParamsType = DGCNParams
main = partial(run, DGCNv2Trainer, ParamsType)
