"""bc-LSTM and bc-GRU on the MI355X hot path (drop-ins for LSTMModel, track_mm/dgcnv2_models.py:389-425, and GRUModel
:350-386, with MaskedNLLLoss :13-33): conv-emotion's context-only baselines, a 2-layer bidirectional RNN over the utterance
features followed by the 'general2' matching attention and the classifier.

``LSTMModule`` / ``GRUModule`` keep the reference's constructor signature, its ``state_dict`` key for key and shape for shape
(``lstm.*`` or ``gru.*`` -- 16 tensors --, ``matchatt.transform.{weight,bias}``, ``linear.*``, ``smax_fc.*``; all 22 are live)
and ``forward(**batch) -> (log_prob [N, C], emotions [N, 200])`` on the valid rows, dialogue-major.  Built: D_e = D_h = 100,
fp32, att2=True, up to 110 utterances (the matching attention's limit); anything else raises ``ErcGraftError`` naming the
argument.

Batches are time-major (batch_first=False): padded row t*B + b.  Chain: the unpacked 2-layer bidirectional RNN over all B*T
padded rows (rnn.py: both directions run all T steps, so the reverse direction of a short dialogue starts inside its zero
padding, as the reference's nn.LSTM / nn.GRU on the padded tensor does; csrc/lstm.hip, csrc/gru100.hip) -> gather of the N
valid rows -> Q = E W^T + b (GEMM) -> matching attention 'general2' per dialogue over its valid rows (200 wide) ->
ReLU(Linear(200, 100)) + dropout in the GEMM epilogue -> smax_fc + class-weighted NLL in one launch.  The backward mirrors
it; every weight gradient joins the step's batched weight-gradient launch (erc_wgrad_table).  One ``dropout`` value drives the
RNN's inter-layer dropout and the classifier's (:357-358, :396-397).
"""
import torch
from torch import nn

from . import capi
from .engine import WorkspaceCache, FlatParams, FusedAdam, GemmPlanner, all_reduce_grads, linear_fwd, linear_wgrad
from .dgcnv2 import IEMOCAP6_WEIGHTS
from .rnn import BiGRU2, BiLSTM2, gru_groups, lstm_groups

D_E, D_HID, EW, MAX_T = 100, 100, 200, 110


class _Transform(nn.Module):          # MatchingAttention('general2'): its one parameterised layer
    def __init__(self, d):
        super().__init__()
        self.transform = nn.Linear(d, d, bias=True)


class _BcRnnModule(nn.Module):
    CELL = None                       # "lstm" | "gru": the attribute / state_dict prefix of the RNN

    def __init__(self, D_m, D_e, D_h, n_classes=7, dropout=0.5, compute="f32", seed=1):
        super().__init__()
        tag = "bc" + self.CELL
        for name, got, want in (("D_e", D_e, D_E), ("D_h", D_h, D_HID)):
            if got != want:
                raise capi.ErcGraftError("%s: the kernels are built for %s=%d, got %r" % (tag, name, want, got))
        if int(D_m) < 1:
            raise capi.ErcGraftError("%s: D_m=%r" % (tag, D_m))
        if compute != "f32":
            raise capi.ErcGraftError("%s runs in fp32 only (the reference is fp32); --compute=%s is not supported" % (tag, compute))
        if not 0.0 <= dropout < 1.0:
            raise capi.ErcGraftError("%s: dropout=%r out of range" % (tag, dropout))
        self.D_m, self.n_classes, self.compute, self.drop_p = int(D_m), n_classes, compute, float(dropout)
        rnn = (nn.LSTM if self.CELL == "lstm" else nn.GRU)(input_size=D_m, hidden_size=D_e, num_layers=2, bidirectional=True,
                                                           dropout=dropout)
        setattr(self, self.CELL, rnn)
        self.matchatt = _Transform(2 * D_e)
        self.linear = nn.Linear(2 * D_e, D_h)
        self.smax_fc = nn.Linear(D_h, n_classes)
        self.flat, self._ws, self._seed = None, WorkspaceCache(), seed

    def live_groups(self):
        groups = (lstm_groups if self.CELL == "lstm" else gru_groups)(self.CELL + ".", getattr(self, self.CELL))
        return groups + [[("matchatt.transform.weight", self.matchatt.transform.weight)],
                         [("matchatt.transform.bias", self.matchatt.transform.bias)],
                         [("linear.weight", self.linear.weight)], [("linear.bias", self.linear.bias)],
                         [("smax_fc.weight", self.smax_fc.weight)], [("smax_fc.bias", self.smax_fc.bias)]]

    def finalize(self, device):
        self.to(device)
        self.flat = FlatParams(self.live_groups(), device)
        self.enc = (BiLSTM2 if self.CELL == "lstm" else BiGRU2)(self.flat, self.CELL + ".", self.D_m, drop_p=self.drop_p)
        self.rng_state = torch.tensor([0, self._seed], dtype=torch.int64, device=device)
        return self

    @property
    def _last_ws(self):
        """workspace of the most recent forward (tests / bench read results out of it)"""
        return self._ws.last

    def _workspace(self, B, T, N, device):
        return self._ws.get((B, T, N), lambda: self._make_workspace(B, T, N, device))

    def _make_workspace(self, B, T, N, device):
        # zeros, not empty: a stale NaN must never reach a weight-gradient GEMM through a row the step did not touch
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)
        C, BT, D = self.n_classes, B * T, self.D_m
        ws = dict(node_off=i32(B + 1), node_row=i32(N), node_spk=i32(N), M=f32(BT, EW), E=f32(N, EW), Q=f32(N, EW), A=f32(N, EW),
                  P=f32(B * T * T), TH=f32(B * T * T), Zc=f32(N, D_HID), logits=f32(N, C), logp=f32(N, C),
                  stats=f32(max(256, capi.head_ce_stats_floats(N))), dlogits=f32(N, C), dZc=f32(N, D_HID), dA=f32(N, EW),
                  DZ=f32(B * T * T), dQ=f32(N, EW), dE=f32(N, EW), dM=f32(BT, EW))
        ws["planner"] = GemmPlanner(device, 4 * BT * 800 + 10 * (800 * D + 800 * 200) + (1 << 21), grad=self.flat.grad)
        ws["jobs"] = None
        return ws

    def _shape(self, x, lens, label, n_nodes=None):
        T, B = int(x.shape[0]), int(x.shape[1])
        N = int(label.shape[0]) if label is not None else (int(n_nodes) if n_nodes is not None else int(lens.sum().item()))
        return B, T, N

    def _check(self, x, onehot, T):
        if T > MAX_T:
            raise capi.ErcGraftError("bc%s: the 200-wide matching attention (erc_match_att_fwd) is built for dialogues of up to %d "
                                     "utterances (batch T=%d)" % (self.CELL, MAX_T, T))
        if int(x.shape[-1]) != self.D_m:
            raise capi.ErcGraftError("bc%s: input_tensor has %d features, D_m=%d" % (self.CELL, int(x.shape[-1]), self.D_m))
        if x.dtype != torch.float32 or onehot.dtype != torch.float32:
            raise capi.ErcGraftError("bc%s: input_tensor and speaker_tensor must be fp32 (one-hot speakers)" % self.CELL)

    def _forward_impl(self, x, onehot, lens, B, T, N, training, with_logits=True, att2=True):
        if not att2:
            raise capi.ErcGraftError("bc%s: att2=False is not built (the reference default, True, is)" % self.CELL)
        self._check(x, onehot, T)
        fp = self.flat
        ws = self._workspace(B, T, N, x.device)
        pl = ws["planner"]
        pl.reset()
        D, C, BT = self.D_m, self.n_classes, B * T
        x, onehot = x.contiguous(), onehot.contiguous()
        # node_off / node_row (= t*B + b) of the valid rows; the speakers do not enter these models
        capi.dialogrnn_meta(onehot, int(onehot.shape[-1]), lens, B, T, N, ws["node_off"], ws["node_row"], ws["node_spk"])
        # unpacked: lengths=None runs every dialogue over all T padded steps, row t*B + b (sb = 1, st = B)
        self.enc.forward(pl, x, D, BT, B, T, 1, B, None, training, self.rng_state, ws["M"], EW, store=ws)
        E = ws["E"]
        capi.gather_rows(ws["M"], EW, ws["node_row"], N, EW, E, EW)
        linear_fwd(pl, E, EW, None, fp.w("matchatt.transform.weight"), fp.w("matchatt.transform.bias"), ws["Q"], EW, N, EW, EW)
        capi.match_att_fwd(E, EW, ws["Q"], EW, ws["node_off"], B, T, EW, ws["A"], EW, ws["P"], ws["TH"])
        p = self.drop_p if training else 0.0
        linear_fwd(pl, ws["A"], EW, None, fp.w("linear.weight"), fp.w("linear.bias"), ws["Zc"], D_HID, N, D_HID, EW,
                   act=3 if p > 0 else 1, drop_p=p, rng=self.rng_state)
        if with_logits:
            linear_fwd(pl, ws["Zc"], D_HID, None, fp.w("smax_fc.weight"), fp.w("smax_fc.bias"), ws["logits"], C, N, C, D_HID)
        ws["x"] = x
        return ws

    def forward(self, input_tensor, speaker_tensor, attention_mask=None, text_length=None, label=None, att2=True, **kwargs):
        if self.flat is None:
            raise capi.ErcGraftError("call %s.finalize(device) before forward" % type(self).__name__)
        B, T, N = self._shape(input_tensor, text_length, label, kwargs.get("n_nodes"))
        ws = self._forward_impl(input_tensor, speaker_tensor, text_length, B, T, N, self.training, att2=att2)
        capi.log_softmax_rows(ws["logits"], self.n_classes, self.n_classes, N, ws["logp"], self.n_classes)
        return ws["logp"], ws["E"]

    def loss_and_grads(self, batch, class_weight=None):
        """MaskedNLLLoss(weight) of the log-probabilities (= class-weighted cross entropy of the valid rows' logits) and every
        gradient into flat.grad"""
        x, onehot, lens, ys = batch["input_tensor"], batch["speaker_tensor"], batch["text_length"], batch["label"]
        B, T, N = self._shape(x, lens, ys)
        head = self.n_classes <= 8
        ws = self._forward_impl(x, onehot, lens, B, T, N, self.training, with_logits=not head)
        fp, pl, off = self.flat, ws["planner"], self.flat.offsets
        C = self.n_classes
        E, dE = ws["E"], ws["dE"]
        p = self.drop_p if self.training else 0.0
        # smax_fc + NLL of the log-softmax + their backward through the dropout / ReLU mask
        if head:
            capi.head_ce(ws["Zc"], D_HID, D_HID, C, N, fp.w("smax_fc.weight"), fp.w("smax_fc.bias"), ys, class_weight,
                         1.0 / (1.0 - p), ws["logits"], C, ws["dlogits"], C, ws["dZc"], D_HID, ws["stats"])
        else:
            capi.cross_entropy(ws["logits"], C, C, N, None, ys, class_weight, 1.0, ws["dlogits"], C, ws["stats"])
            capi.gemm_f32(ws["dlogits"], C, 0, None, fp.w("smax_fc.weight"), D_HID, 1, None, ws["dZc"], D_HID, N, D_HID, C,
                          act=2, aux=ws["Zc"], ldaux=D_HID, act_scale=1.0 / (1.0 - p))
        linear_wgrad(pl, ws["dlogits"], C, ws["Zc"], D_HID, None, C, D_HID, N, off["smax_fc.weight"], off["smax_fc.bias"], defer=True)
        capi.gemm_f32(ws["dZc"], D_HID, 0, None, fp.w("linear.weight"), EW, 1, None, ws["dA"], EW, N, EW, D_HID)
        linear_wgrad(pl, ws["dZc"], D_HID, ws["A"], EW, None, D_HID, EW, N, off["linear.weight"], off["linear.bias"], defer=True)
        # matching attention: dQ and dE (key side + score side); E is also the query transform's input
        capi.match_att_bwd(E, EW, ws["Q"], EW, ws["dA"], EW, ws["node_off"], B, T, EW, ws["P"], ws["TH"], ws["DZ"], ws["dQ"], EW, dE, EW)
        linear_wgrad(pl, ws["dQ"], EW, E, EW, None, EW, EW, N, off["matchatt.transform.weight"], off["matchatt.transform.bias"],
                     defer=True)
        capi.gemm_f32(ws["dQ"], EW, 0, None, fp.w("matchatt.transform.weight"), EW, 1, None, dE, EW, N, EW, EW, accumulate=1)
        # back to the padded rows (zero on the padding: nothing downstream reads the RNN's output there), then the RNN
        dM = ws["dM"]
        dM.zero_()
        capi.gather_rows(dE, EW, ws["node_row"], N, EW, dM, EW, scatter=1)
        self.enc.backward(pl, dM, EW)
        pl.reduce_into(ws, fp.grad)
        return ws["stats"]


class LSTMModule(_BcRnnModule):
    """bc-LSTM: LSTMModel (track_mm/dgcnv2_models.py:389-425)"""
    CELL = "lstm"


class GRUModule(_BcRnnModule):
    """bc-GRU: GRUModel (track_mm/dgcnv2_models.py:350-386)"""
    CELL = "gru"


class BcRnnTrainer:
    """train_step / to_logits for ``--module=bclstm`` and ``--module=bcgru``: class-weighted MaskedNLLLoss, Adam lr 3e-4, no
    weight decay (the defaults of the sibling plugin, track_mm/dgcnv2.py:22-48,184-219).  ``MODULE`` picks the cell."""
    MODULE, NAME = None, None

    def __init__(self, params, device):
        self.params, self.device = params, torch.device(device)
        compute = params.get("compute", "f32")
        if compute != "f32":
            raise capi.ErcGraftError("--module=%s runs in fp32 (the reference is fp32); --compute=%s is not supported"
                                     % (self.NAME, compute))
        self.class_weight = None
        if params.get("loss_weights", True):
            if params.n_classes != 6:
                raise capi.ErcGraftError("--loss_weights uses the six hard-coded IEMOCAP-6 inverse frequencies "
                                         "(dgcnv2.py:213-214); run %d-class datasets with --loss_weights=False" % params.n_classes)
            self.class_weight = torch.tensor(IEMOCAP6_WEIGHTS, dtype=torch.float32, device=self.device)
        torch.manual_seed(params.seed)
        self.model = self.MODULE(params.hidden_all, D_E, D_HID, n_classes=params.n_classes, dropout=params.get("dropout", 0.5),
                                 compute=compute, seed=params.seed).finalize(self.device)
        o = params.optim
        self.optim = FusedAdam(self.model.flat, lr=o.lr, weight_decay=o.get("weight_decay", 0.0),
                               decoupled=(o.name == "AdamW"), seed=params.seed)
        self.model.rng_state = self.optim.rng_state

    def to_logits(self, batch):
        return self.model(**batch)[0]

    def prepare_batch(self, batch):
        out = {k: (v.to(self.device) if torch.is_tensor(v) else v) for k, v in batch.items()}
        tl = batch.get("text_length")
        if "n_nodes" not in out and torch.is_tensor(tl) and not tl.is_cuda:
            out["n_nodes"] = int(tl.sum())      # host tensor: no device sync when a batch carries no labels
        return out

    def train_step(self, batch):
        self.model.train()
        stats = self.model.loss_and_grads(batch, self.class_weight)
        scale = all_reduce_grads(self.model.flat)
        self.optim.step(grad_scale=scale)
        return stats


class BcLstmTrainer(BcRnnTrainer):
    MODULE, NAME = LSTMModule, "bclstm"


class BcGruTrainer(BcRnnTrainer):
    MODULE, NAME = GRUModule, "bcgru"
