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

Capacity mode (``--capacity_buckets=True``, ``--resident``; off by default): the same chain with every launch sized for a
bucket (B_cap, T_cap, N_cap) and the batch's node count and longest dialogue read from the device -- ``_forward_cap``,
``BcRnnTrainer.capacity_bucket`` / ``all_capacity_buckets`` / ``resident_batch``; DESIGN.md section 8e.
"""
import torch
from torch import nn

from . import capi
from .capacity import CapacityBuckets, ConvEmotionTrainer, ZeroRowStores
from .engine import WorkspaceCache, FlatParams, GemmPlanner
from .matchhead import ConvEmotionModule, MatchAttHead, Transform
from .rnn import BiGRU2, BiLSTM2, gru_groups, lstm_groups

D_E, D_HID, EW, MAX_T = 100, 100, 200, 110


class _BcRnnModule(ConvEmotionModule):
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
        self.matchatt = Transform(2 * D_e)
        self.linear = nn.Linear(2 * D_e, D_h)
        self.smax_fc = nn.Linear(D_h, n_classes)
        # CAPACITY MODE (trainer.StepGraphs buckets, trainer.ResidentEpochs): the batch tensors are capacity-sized static
        # buffers -- B dialogue slots of which some may have length 0, T the longest dialogue of the split, label [N_cap] -- and
        # every launch is sized for the capacities.  erc_bcrnn_meta_cap writes the batch's node count and its longest dialogue
        # to the device (ws["counts"]): the scans run that many steps, the loss covers that many rows, and the kernels that own
        # a gradient buffer zero its rows past them, so ONE captured HIP graph serves every batch that fits.
        self.dynamic_n = False
        self.flat, self._ws, self._seed = None, WorkspaceCache(), seed

    def live_groups(self):
        groups = (lstm_groups if self.CELL == "lstm" else gru_groups)(self.CELL + ".", getattr(self, self.CELL))
        return groups + MatchAttHead.groups("", self)

    def finalize(self, device):
        self.to(device)
        self.flat = FlatParams(self.live_groups(), device)
        self.enc = (BiLSTM2 if self.CELL == "lstm" else BiGRU2)(self.flat, self.CELL + ".", self.D_m, drop_p=self.drop_p)
        self.head = MatchAttHead(self.flat, "", EW, D_HID, self.n_classes, self.drop_p)
        self.rng_state = torch.tensor([0, self._seed], dtype=torch.int64, device=device)
        return self

    def _workspace(self, B, T, N, device, cap=False):
        if cap:
            return self._ws.get((B, T, N, "capacity"), lambda: self._make_workspace(B, T, N, device, cap=True))
        return self._ws.get((B, T, N), lambda: self._make_workspace(B, T, N, device))

    def _make_workspace(self, B, T, N, device, cap=False):
        # zeros, not empty: a stale NaN must never reach a weight-gradient GEMM through a row the step did not touch
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)
        BT, D = B * T, self.D_m
        # capacity mode: one more row behind the padded RNN output (M) and behind the node gradient (dE), never written by
        # anything: the zero row that node_row (capacity nodes) and pad_node (padded positions) point at
        zrow = 1 if cap else 0
        ws = dict(node_off=i32(B + 1), node_row=i32(N), node_spk=i32(N), M=f32(BT + zrow, EW), E=f32(N, EW), dM=f32(BT, EW),
                  **self.head.buffers(B, T, N, device, dE_rows=N + zrow))
        if cap:
            ws.update(pad_node=i32(BT), x_row=i32(BT), counts=i32(2), label=torch.zeros(N, dtype=torch.int64, device=device))
        ws["planner"] = GemmPlanner(device, 4 * BT * 800 + 10 * (800 * D + 800 * 200) + (1 << 21), grad=self.flat.grad)
        ws["jobs"] = None
        return ws

    def _check(self, x, onehot, T):
        if T > MAX_T:
            raise capi.ErcGraftError("bc%s: the 200-wide matching attention (erc_match_att_fwd) is built for dialogues of up to %d "
                                     "utterances (batch T=%d)" % (self.CELL, MAX_T, T))
        if int(x.shape[-1]) != self.D_m:
            raise capi.ErcGraftError("bc%s: input_tensor has %d features, D_m=%d" % (self.CELL, int(x.shape[-1]), self.D_m))
        if x.dtype != torch.float32 or onehot.dtype != torch.float32:
            raise capi.ErcGraftError("bc%s: input_tensor and speaker_tensor must be fp32 (one-hot speakers)" % self.CELL)

    def _forward_cap(self, x, lens, B, T, N, training, desc=None, store_label=None):
        """The forward in CAPACITY mode: B, T, N are capacities, the batch's own node count and longest dialogue are on the
        device (ws["counts"] = [n_dev, t_dev]).  ``desc`` (int32 [2 B]: lengths | first store rows): RESIDENT batch -- x is the
        feature store [U + 1, D] whose last row is zero, read through ws["x_row"]; labels are gathered into ws["label"].

        Rows past the batch: the RNN's rows t >= *t_dev are not run (outputs written 0, gate gradients written 0 by the
        backward scans); node rows i >= N gather the zero row of M, so E is 0 there; A / Zc of those rows are whatever an
        earlier batch left (finite) and meet a zero gradient row in every weight-gradient product (dZc, dlogits: head_ce_cap;
        dQ, dE: match_att_bwd_cap; dA = dZc W).  Dialogue slots the batch does not fill (length 0) run the RNN over zero
        input; no valid node reads their rows, so the gradient wrt their outputs (pad_node -> the zero row of dE) and with it
        every gate gradient of theirs is exactly 0."""
        if T > MAX_T:
            raise capi.ErcGraftError("bc%s: the 200-wide matching attention (erc_match_att_fwd) is built for dialogues of up to %d "
                                     "utterances (T_cap=%d)" % (self.CELL, MAX_T, T))
        if x.dtype != torch.float32 or int(x.shape[-1]) != self.D_m:
            raise capi.ErcGraftError("bc%s: capacity mode needs fp32 features of width D_m=%d" % (self.CELL, self.D_m))
        if desc is None and lens.dtype != torch.int64:
            raise capi.ErcGraftError("bc%s: capacity mode needs int64 text_length" % self.CELL)
        ws = self._workspace(B, T, N, x.device, cap=True)
        pl = ws["planner"]
        pl.reset()
        D, BT = self.D_m, B * T
        x = x.contiguous()
        if desc is not None:
            capi.bcrnn_meta_cap(None, desc, store_label, int(x.shape[0]) - 1, B, T, N, ws["node_off"], ws["node_row"], ws["pad_node"],
                                ws["x_row"], ws["label"], ws["counts"])
        else:
            capi.bcrnn_meta_cap(lens, None, None, 0, B, T, N, ws["node_off"], ws["node_row"], ws["pad_node"], None, None,
                                ws["counts"])
        self.enc.forward(pl, x, D, BT, B, T, 1, B, None, training, self.rng_state, ws["M"], EW, store=ws,
                         node_row=ws["x_row"] if desc is not None else None, t_dev=ws["counts"][1:])
        capi.gather_rows(ws["M"], EW, ws["node_row"], N, EW, ws["E"], EW)
        self.head.forward(pl, ws, ws["E"], ws["node_off"], B, T, N, training, self.rng_state, with_logits=False)
        ws["x"] = x
        return ws

    def _forward_impl(self, x, onehot, lens, B, T, N, training, with_logits=True, att2=True):
        if not att2:
            raise capi.ErcGraftError("bc%s: att2=False is not built (the reference default, True, is)" % self.CELL)
        if self.dynamic_n:
            raise capi.ErcGraftError("bc%s: capacity mode (dynamic_n) is the training step's (loss_and_grads)" % self.CELL)
        self._check(x, onehot, T)
        ws = self._workspace(B, T, N, x.device)
        pl = ws["planner"]
        pl.reset()
        D, BT = self.D_m, B * T
        x, onehot = x.contiguous(), onehot.contiguous()
        # node_off / node_row (= t*B + b) of the valid rows; the speakers do not enter these models
        capi.dialogrnn_meta(onehot, int(onehot.shape[-1]), lens, B, T, N, ws["node_off"], ws["node_row"], ws["node_spk"])
        # unpacked: lengths=None runs every dialogue over all T padded steps, row t*B + b (sb = 1, st = B)
        self.enc.forward(pl, x, D, BT, B, T, 1, B, None, training, self.rng_state, ws["M"], EW, store=ws)
        capi.gather_rows(ws["M"], EW, ws["node_row"], N, EW, ws["E"], EW)
        self.head.forward(pl, ws, ws["E"], ws["node_off"], B, T, N, training, self.rng_state, with_logits)
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
        desc = batch.get("desc")          # resident batch (trainer.ResidentEpochs): the store + 2 B int32 of batch description
        cap = self.dynamic_n or desc is not None
        head = self.n_classes <= 8
        if cap:
            if not (self.dynamic_n and head):
                raise capi.ErcGraftError("bc%s: capacity mode needs dynamic_n and at most 8 classes (erc_head_ce_cap)" % self.CELL)
            B, T, N = batch["caps"] if desc is not None else self._shape(x, lens, ys)
            ws = self._forward_cap(x, lens, B, T, N, self.training, desc=desc, store_label=ys if desc is not None else None)
            if desc is not None:
                ys = ws["label"]
        else:
            B, T, N = self._shape(x, lens, ys)
            ws = self._forward_impl(x, onehot, lens, B, T, N, self.training, with_logits=not head)
        pl, dE = ws["planner"], ws["dE"]
        self.head.backward(pl, ws, ws["E"], ws["node_off"], B, T, N, ys, class_weight, self.training,
                           n_dev=ws["counts"] if cap else None, n_cap=N if cap else 0)
        # back to the padded rows (zero on the padding: nothing downstream reads the RNN's output there), then the RNN
        dM = ws["dM"]
        if cap:
            # every padded row fetches its node's gradient, or the zero row behind dE: no whole-buffer zero_() per step
            capi.gather_rows(dE, EW, ws["pad_node"], B * T, EW, dM, EW)
        else:
            dM.zero_()
            capi.gather_rows(dE, EW, ws["node_row"], N, EW, dM, EW, scatter=1)
        self.enc.backward(pl, dM, EW)
        pl.reduce_into(ws, self.flat.grad)
        return ws["stats"]


class LSTMModule(_BcRnnModule):
    """bc-LSTM: LSTMModel (track_mm/dgcnv2_models.py:389-425)"""
    CELL = "lstm"


class GRUModule(_BcRnnModule):
    """bc-GRU: GRUModel (track_mm/dgcnv2_models.py:350-386)"""
    CELL = "gru"


class BcRnnTrainer(CapacityBuckets, ConvEmotionTrainer):
    """train_step / to_logits for ``--module=bclstm`` and ``--module=bcgru``: class-weighted MaskedNLLLoss, Adam lr 3e-4, no
    weight decay (the defaults of the sibling plugin, track_mm/dgcnv2.py:22-48,184-219).  ``MODULE`` picks the cell."""
    MODULE = None

    def __init__(self, params, device):
        # capacity buckets are opt-in: the default stays the exact-shape step, whose dropout masks (keyed by the element
        # index, so by B) a captured exact-shape graph must reproduce
        super().__init__(params, device, opt_in=True)
        self._store_ext = ZeroRowStores()

    def _build_model(self, params, compute):
        return self.MODULE(params.hidden_all, D_E, D_HID, n_classes=params.n_classes, dropout=params.get("dropout", 0.5),
                           compute=compute, seed=params.seed)

    # -- capacity mode: the policy (the implementation is capacity.CapacityBuckets).  N_BUCKET 128 and "a batch of exactly its
    #    bucket's shape stays exact" are the mixin's defaults, and so is the precapture list, built from train.batch_size
    #    and T_cap alone; ``opt_in=True`` (above) makes the buckets opt-in
    TIME_MAJOR = True          # [T, B, D] features, [T, B, S] one-hot speakers
    CLEAR_STALE = True         # the RNN is unpacked: it READS the padded rows t < T_eff of every dialogue slot, so they must
    #                            be zero, not stale

    def _capacity_ok(self, B_cap, T_cap, N_cap, batch=None):
        """no bucket with the flag off, with the peer-to-peer exchange, above the matching attention's T or the head's classes,
        or for a batch of other dtypes / ranks (the gate is on T_cap: the node launches take any N_cap)"""
        ok = self.capacity and not self._p2p() and 0 < T_cap <= MAX_T and self.model.n_classes <= 8
        if ok and batch is not None:
            x, spk = batch["input_tensor"], batch["speaker_tensor"]
            ok = (x.dtype == torch.float32 and x.dim() == 3 and int(x.shape[2]) == self.model.D_m and spk.dim() == 3 and
                  batch["text_length"].dtype == torch.int64)
        return bool(ok)

    def _resident_ok(self, store, B_cap, T_cap, N_cap):
        return store.fused.dtype == torch.float32 and int(store.fused.shape[1]) == self.model.D_m and self._capacity_ok(B_cap, T_cap, N_cap)

    def _resident_inputs(self, store):
        """The layer-0 projection reads the store's rows through the step's row map; padded positions read a zero row, which
        the store does not have, so the features are kept once per store with one appended.  No speakers: the model reads none."""
        return self._store_ext(store, store.fused), None


class BcLstmTrainer(BcRnnTrainer):
    MODULE, NAME = LSTMModule, "bclstm"


class BcGruTrainer(BcRnnTrainer):
    MODULE, NAME = GRUModule, "bcgru"
