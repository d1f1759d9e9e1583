"""``--module=dialogrnn`` plugin: the DialogueRNN model (reference: DialogRNNModel, track_mm/dgcnv2_models.py:428-487, and
MaskedNLLLoss :13-33).  The reference has no plugin file of its own for it; the defaults are those of its sibling
track_mm/dgcnv2.py:22-48."""
from functools import partial

from erc_amd.dialogrnn import DialogRNNModule, DialogRNNTrainer  # noqa: F401
from erc_amd.params import ERCParams, Group
from erc_amd.trainer import run


class DialogRNNParams(ERCParams):
    def __init__(self):
        super().__init__()
        self.train.batch_size = self.val.batch_size = self.test.batch_size = 32   # dgcnv2.py:28-30
        self.dataset = "iemocap-cogmen-6"
        self.epoch = 55
        self.optim = Group(name="Adam", lr=0.0003, weight_decay=0)                # dgcnv2.py:37
        self.loss_weights = True                                                  # dgcnv2.py:42
        self.speaker_onehot, self.batch_first = True, False                       # dgcnv2.py:43-44
        self.dropout_rec, self.dropout = 0.5, 0.5                                 # dgcnv2_models.py:430-431
        # capacity buckets (one captured graph per padded (B, T, N) bucket instead of per exact shape) are opt-in here:
        # --capacity_buckets=True, or --resident (with --device_collate), which implies them; --resident_eval with --resident
        self.capacity_buckets = False


ParamsType = DialogRNNParams
main = partial(run, DialogRNNTrainer, ParamsType)
