"""``--module=cim`` plugin (reference: track_mm/cim.py:28-57,180-227)."""
from functools import partial

from erc_amd.cim import CIMModule, CIMTrainer  # noqa: F401
from erc_amd.params import ERCParams, Group
from erc_amd.trainer import run


class CIMParams(ERCParams):
    def __init__(self):
        super().__init__()
        self.seed = 1
        self.train.batch_size = 16                                                # cim.py:35-37
        self.val.batch_size = self.test.batch_size = 32
        self.num_heads = 17                                                       # cim.py:39 (unused by the model)
        self.dataset = "iemocap-cogmen-6"
        self.epoch = 55
        self.optim = Group(name="Adam", lr=0.001, weight_decay=0)                 # cim.py:42
        self.apply_multi = True
        self.apply_bin = True
        # capacity buckets (one captured graph per (B_cap, T_cap, N_cap) instead of per exact shape) are opt-in here:
        # --capacity_buckets=True, or --resident (with --device_collate), which implies them; --resident_eval with --resident
        # (not on CMU-MOSEI with its multi-label metrics)
        self.capacity_buckets = False

    def iparams(self):
        super().iparams()
        if "mosei" not in self.dataset:                                           # cim.py:52-53
            self.apply_multi = False
        if self.n_classes != 2:                                                   # cim.py:57-58
            self.mosei_metric = ""
        return self


ParamsType = CIMParams
main = partial(run, CIMTrainer, ParamsType)
