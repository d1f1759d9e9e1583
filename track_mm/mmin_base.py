"""``--module=mmin_base`` plugin: MMIN's full-modality base model, the utterance classifier the missing-modality plugins start
from (reference: track_mm/mmin_base.py, track_mm/mmin_models.py:202-240)."""
from functools import partial

from erc_amd.mmin import MMINBaseModule, MMINBaseTrainer, run  # noqa: F401
from erc_amd.params import ERCParams, Group


class MMINBaseParams(ERCParams):
    def __init__(self):
        super().__init__()
        self.train.batch_size = self.val.batch_size = self.test.batch_size = 32       # mmin_base.py:32-34
        self.num_heads, self.gnn_heads = 10, 1                                          # :36-37 (declared, never read)
        self.confuse_matrix = True                                                      # :38
        self.dataset = "iemocap-mmin-4"                                                 # :39
        self.epoch = 55                                                                 # :40
        self.optim = Group(name="Adam", lr=0.0002, weight_decay=0)                     # :41
        self.split_params = False
        self.ema = True                                                                 # :45
        self.sche_type, self.warmup_epochs = "cos", 0                                   # :47-48 (declared, never read)
        self.pretrain_path = None                                                       # :49
        # build-specific: the two baselines of the missing-modality model (the reference has neither flag).  eval_missing: the
        # validation and test epochs are also scored under the six missing-modality patterns; train_missing: every training
        # sample is masked at random as --module=mmin_miss masks it.  The defaults keep every launch and printed line as they are
        self.eval_missing = False
        self.train_missing = False
        # build-specific: the synthetic splits (no .h5 features and no h5py here) and the assumed ComParE frame-count range
        self.n_train, self.n_val, self.n_test = 256, 64, 64
        self.mmin_frames = (50, 400)
        self.save_dir = None

    def iparams(self):
        super().iparams()
        if self.debug:                                                                  # :53-57
            self.train.batch_size = self.test.batch_size = 2
        return self


ParamsType = MMINBaseParams
main = partial(run, MMINBaseTrainer, ParamsType)
