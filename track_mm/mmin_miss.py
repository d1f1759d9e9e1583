"""``--module=mmin_miss`` plugin: MMIN's missing-modality model -- the residual autoencoders that imagine the features of the
modalities an utterance lacks, trained against a pretrained ``--module=mmin_base`` model (reference: track_mm/mmin_miss.py,
track_mm/mmin_models.py:133-199)."""
from functools import partial

from erc_amd.mmin import run
from erc_amd.mmin_miss import Missing, MMINMissCollate, MMINMissModule, MMINMissTrainer  # noqa: F401
from erc_amd.params import ERCParams, Group


class MMINMissParams(ERCParams):
    def __init__(self):
        super().__init__()
        self.train.batch_size = self.val.batch_size = self.test.batch_size = 32       # mmin_miss.py:36-38
        self.num_heads, self.gnn_heads = 10, 1                                          # :40-41 (declared, never read)
        self.confuse_matrix = True                                                      # :42
        self.dataset = "iemocap-mmin-4"                                                 # :43
        self.epoch = 55                                                                 # :44
        self.optim = Group(name="Adam", lr=0.0002, weight_decay=0)                     # :45
        self.split_params = False
        self.ema = True                                                                 # :49
        self.sche_type, self.warmup_epochs = "cos", 0                                   # :51-52 (declared, never read)
        # :53 is a path on the authors' machine; here the flag names a checkpoint written by --module=mmin_base (this library's or
        # the reference's), and without it the pretrained model keeps its initialisation
        self.pretrain_path = None
        self.finetune = False                                                           # :54 (accepted; it has no effect, :149-154)
        # build-specific: keep the loaded pretrained weights instead of re-initialising them as the reference does (:157-158)
        self.pretrain_reinit = True
        # build-specific: score the validation and test epochs under the six missing-modality patterns as well (the reference
        # evaluates full-modality only, :368); the default keeps every launch and every printed line as they are
        self.eval_missing = False
        self.n_train, self.n_val, self.n_test = 256, 64, 64
        self.mmin_frames = (50, 400)
        self.save_dir = None

    def iparams(self):
        super().iparams()
        if self.debug:                                                                  # :58-62
            self.train.batch_size = self.test.batch_size = 2
        return self


ParamsType = MMINMissParams
main = partial(run, MMINMissTrainer, ParamsType)
