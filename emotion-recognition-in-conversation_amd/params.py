"""Run parameters of the ERC plugins: same flag names and derived values as the
reference's ``MMBaseParams`` (track_mm/mmbase.py:22-126), ``DataParams``
(mmdatasets/dataset_utils.py:16-31) and ``n_classes`` rule
(mmdatasets/const.py:35-37), with the ``fire``-style command line of
lumo/core/params.py:248-270 (``--key=value``, dotted keys for nested groups,
bare ``--flag`` -> True).  No lumo / fire / omegaconf dependency.

Datasets: the IEMOCAP / MELD feature releases of the conversation-graph track and ``mosei-cim-2`` (CIM's CMU-MOSEI
release: text 300, audio 74, visual 35, two sentiment classes, and 7-way multi-hot emotion labels that CIM trains on
as a second task).  ``mosei_metric`` is ``'multiemo'`` on MOSEI -- the test pass then also reports per-emotion metrics
of the multi-label head -- and ``''`` elsewhere (mmbase.py:49,62-63; CIM also clears it when n_classes != 2).
"""
import ast
import sys

MODALITIES = ("atv", "av", "at", "tv", "t", "a", "v")


def _names(stem, texts, visuals, ks):
    out = []
    for k in ks:
        for t in texts:
            for v in visuals:
                out.append("-".join([stem] + [p for p in (t, v) if p] + [str(k)]))
    return out


# the conversation-graph (IEMOCAP / MELD feature) subset of regist_data,
# mmdatasets/datas/__init__.py:33-68.
DATASETS = tuple(
    _names("iemocap-cogmen", ("", "sbert", "robert"), ("", "tsn", "tsn-v+"), (6,))
    + _names("iemocap-cogmen", ("", "sbert", "robert"), ("", "tsn", "tsn-v+", "tsnss", "tsnss-v+"), (4,))
    + ["meld-mmgcn-7", "meld-mmgcn-sbert-7"])
# CIM's CMU-MOSEI release (:81): videos of CIM/{text,audio,video}.npz with binary sentiment and 7-way multi-hot emotion
# labels, trained by --module=cim only.  The MOSEI.adpated.pkl names (sbert / fbank / is10) and the raw-audio tracks
# are out of scope.
MOSEI_DATASETS = ("mosei-cim-2",)
# MMIN's IEMOCAP utterance features (:31: ComParE audio frames, DenseFace visual frames, BERT token rows; four classes), read by
# --module=mmin_base and --module=mmin_miss only
MMIN_DATASETS = ("iemocap-mmin-4",)
ALL_DATASETS = DATASETS + MOSEI_DATASETS + MMIN_DATASETS


class Group(dict):
    """Attribute dict for nested groups (train/test/optim)."""
    __getattr__ = dict.get

    def __setattr__(self, k, v):
        self[k] = v


class ERCParams:
    """Defaults of MMBaseParams + DataloaderParams; plugins override in
    ``__init__`` exactly as the reference's XParams classes do."""

    def __init__(self):
        self.seed = 1
        self.module = None
        self.method = None
        self.dataset = "iemocap-cogmen-6"
        self.modality = "atv"
        self.n_speakers = 2
        self.n_classes = 6
        self.class_names = []
        self.batch_first = True
        self.speaker_onehot = False
        self.hidden_text = 100
        self.hidden_audio = 100
        self.hidden_visual = 100
        self.hidden_all = 300
        self.reimplement = False
        self.mosei_metric = "multiemo"  # mmbase.py:49; '' for every non-MOSEI dataset (:62-63)
        self.confusion_matrix = True
        self.epoch = 10
        self.device = None
        self.debug = False
        self.train = Group(batch_size=100, num_workers=0, shuffle=True)
        self.val = Group(batch_size=100, num_workers=0, shuffle=False)
        self.test = Group(batch_size=100, num_workers=0, shuffle=False)
        self.optim = Group(name="Adam", lr=1e-3, weight_decay=0.0)
        # build-specific switches (not in the reference)
        self.synthetic = True          # no dataset pickles exist offline
        self.n_train = 120             # IEMOCAP train dialogues
        self.n_test = 31
        self.compute = "f32"           # 'f32' (parity) | 'bf16' (input GEMM operands in bf16)
        self.graph_replay = True       # capture the step in a HIP graph per shape bucket
        self.log_every = 1
        self.faithful_dead_encoder = False   # COGMEN: also run the reference's dead encoder (cost parity, result discarded)
        self.chained_encoder = False         # COGMEN: rnn.1(rnn.0(x, padding mask)) -- trains the encoder

    # ------------------------------------------------------------------ CLI
    def from_args(self, argv=None):
        argv = sys.argv[1:] if argv is None else argv
        for tok in argv:
            if not tok.startswith("--"):
                raise SystemExit("unexpected argument %r (expected --key=value)" % tok)
            key, eq, val = tok[2:].partition("=")
            value = True if not eq else _literal(val)
            self._set(key, value)
        self.iparams()
        return self

    def _set(self, dotted, value):
        parts = dotted.split(".")
        obj = self
        for p in parts[:-1]:
            nxt = getattr(obj, p, None) if not isinstance(obj, dict) else obj.get(p)
            if nxt is None:
                nxt = Group()
                setattr(obj, p, nxt)
            obj = nxt
        if isinstance(obj, dict):
            obj[parts[-1]] = value
        else:
            setattr(obj, parts[-1], value)

    def get(self, key, default=None):
        return getattr(self, key, default)

    # -------------------------------------------------------------- derived
    def iparams(self):
        if self.modality not in MODALITIES:
            raise ValueError("modality %r not in %s" % (self.modality, MODALITIES))
        if self.dataset not in ALL_DATASETS:
            raise ValueError("dataset %r not in %s" % (self.dataset, ALL_DATASETS))
        ds = self.dataset
        self.n_classes = round(float(ds.split("-")[-1]))            # const.py:35-37
        if self.debug:                                              # mmbase.py:56-60
            self.train.batch_size = self.test.batch_size = 2
        if "mosei" not in ds:                                       # mmbase.py:62-63
            self.mosei_metric = ""
        if "iemocap" in ds:                                         # mmbase.py:65-78
            self.class_names = ["hap", "sad", "neu", "ang"] if self.n_classes == 4 else \
                ["hap", "sad", "neu", "ang", "exc", "fru"]
            if "cogmen" in ds:
                self.hidden_audio, self.hidden_text, self.hidden_visual = 100, 100, 512
        elif "meld" in ds:                                          # mmbase.py:80-88
            self.class_names = ["neutral", "sad", "mad", "scared", "powerful", "peaceful", "joyful"]
            self.n_speakers = 9
            if "mmgcn" in ds:
                self.hidden_audio, self.hidden_text, self.hidden_visual = 300, 600, 342
        elif "mosei" in ds:                                         # mmbase.py:89-93
            self.class_names = ["hap", "sad", "disgust", "fear", "surprise", "ang"]
            self.hidden_text, self.hidden_audio, self.hidden_visual = 300, 74, 35
        if "sbert" in ds or "robert" in ds:                         # mmbase.py:103-104
            self.hidden_text = 768
        if "tsn" in ds:                                             # mmbase.py:107-115
            self.hidden_visual = self.hidden_visual + 2048 if "v+" in ds else 2048
        self.hidden_all = sum(d for m, d in (("t", self.hidden_text), ("a", self.hidden_audio),
                                             ("v", self.hidden_visual)) if m in self.modality)
        return self

    def dims(self):
        return {"a": self.hidden_audio, "t": self.hidden_text, "v": self.hidden_visual}


def _literal(text):
    try:
        return ast.literal_eval(text)
    except (ValueError, SyntaxError):
        return text
