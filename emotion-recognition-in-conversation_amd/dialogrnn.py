"""DialogueRNN on the MI355X hot path (drop-in for DialogRNNModel, track_mm/dgcnv2_models.py:428-487 over :235-347, with
MaskedNLLLoss :13-33).

``DialogRNNModule`` keeps the reference's constructor signature, its ``state_dict`` key for key and shape for shape
(``dialog_rnn_{f,r}.dialogue_cell.{g_cell,p_cell,e_cell}.*``, ``...attention.transform.weight``, ``matchatt.transform.*``,
``linear.*``, ``smax_fc.*``; all 32 parameters are live) and ``forward(**batch) -> (log_prob [N, C], emotions [N, 2 D_e])``
on the valid rows, dialogue-major.  Built: context_attention='general', listener_state=False, D_g = D_p = 150,
D_e = D_h = 100, fp32, up to 9 speakers and 110 utterances; anything else raises ``ErcGraftError`` naming the argument.

Batches are time-major (batch_first=False, one-hot speakers): padded row t*B + b.  Chain: batch tables (node_off, node_row,
speaker per node) -> the u-side products W_ih^g[:, :D] u, W_ih^p[:, :D] u (one GEMM per direction: the two weights are
neighbours in the flat buffer) and W_a u over the N valid rows, gathered straight from the padded batch -> the two scans of
all dialogues in one launch (csrc/dialogrnn.hip: padded steps are not run, only the speaker's party cell is evaluated,
dropout_rec' on the emotions in the same launch) -> Q = E W^T + b (GEMM) -> matching attention 'general2' per dialogue
(200 wide) -> ReLU(Linear(200, 100)) + dropout in the GEMM epilogue -> smax_fc + class-weighted NLL in one launch.  The
backward mirrors it; every weight gradient (hoisted products, head, and the recurrent blocks as GEMMs over the per-step gate
gradients and saved states the backward scan writes) joins the step's batched weight-gradient launch (erc_wgrad_table).

Capacity mode (``--capacity_buckets=True``, ``--resident``, ``--resident_eval``; off by default): the same chain with every
launch sized for a bucket (B_cap, T_cap, N_cap) and the batch's node count read from the device -- ``_forward_cap``,
``eval_scores``, ``DialogRNNTrainer``'s policy; DESIGN.md section 8d.
"""
import torch
from torch import nn

from . import capi
from .capacity import CapacityBuckets, ConvEmotionTrainer, ResidentEvalSteps, ZeroRowStores
from .engine import WorkspaceCache, FlatParams, GemmPlanner, linear_fwd, linear_wgrad
from .matchhead import ConvEmotionModule, MatchAttHead, Transform

D_G, D_E, D_HID, EW, MAX_T, MAX_S = 150, 100, 100, 200, 110, 9
GXW = capi.DIALOGRNN_GXW
DIRS = ("dialog_rnn_f", "dialog_rnn_r")
RNG_STREAM = 0x5d10


class _Attention(nn.Module):          # MatchingAttention(D_g, D_m, att_type='general'): Linear(D_m, D_g, bias=False)
    def __init__(self, d_m, d_g):
        super().__init__()
        self.transform = nn.Linear(d_m, d_g, bias=False)


class _Cell(nn.Module):
    def __init__(self, D_m, D_g, D_p, D_e):
        super().__init__()
        self.g_cell = nn.GRUCell(D_m + D_p, D_g)
        self.p_cell = nn.GRUCell(D_m + D_g, D_p)
        self.e_cell = nn.GRUCell(D_p, D_e)
        self.attention = _Attention(D_m, D_g)


class _DialogueRNN(nn.Module):
    def __init__(self, D_m, D_g, D_p, D_e):
        super().__init__()
        self.dialogue_cell = _Cell(D_m, D_g, D_p, D_e)


class DialogRNNModule(ConvEmotionModule):
    def __init__(self, D_m, D_g, D_p, D_e, D_h, D_a=100, n_classes=7, listener_state=False, context_attention="simple",
                 dropout_rec=0.5, dropout=0.5, compute="f32", seed=1):
        super().__init__()
        if listener_state:
            raise capi.ErcGraftError("dialogrnn: listener_state=True is not built (the reference default, False, is)")
        if context_attention != "general":
            raise capi.ErcGraftError("dialogrnn: context_attention=%r is not built ('general' is)" % (context_attention,))
        for name, got, want in (("D_g", D_g, D_G), ("D_p", D_p, D_G), ("D_e", D_e, D_E), ("D_h", D_h, D_HID)):
            if got != want:
                raise capi.ErcGraftError("dialogrnn: the kernels are built for %s=%d (dgcnv2.py:71-77), got %r" % (name, want, got))
        if int(D_m) < 1:
            raise capi.ErcGraftError("dialogrnn: D_m=%r" % (D_m,))
        if compute != "f32":
            raise capi.ErcGraftError("dialogrnn runs in fp32 only (the reference is fp32); --compute=%s is not supported" % compute)
        for name, p in (("dropout_rec", dropout_rec), ("dropout", dropout)):
            if not 0.0 <= p + (0.15 if name == "dropout" else 0.0) < 1.0:
                raise capi.ErcGraftError("dialogrnn: %s=%r out of range" % (name, p))
        self.D_m, self.n_classes, self.compute = int(D_m), n_classes, compute
        self.drop_cell, self.drop_emo, self.drop_p = float(dropout_rec), float(dropout) + 0.15, float(dropout)   # :436-438
        self.dialog_rnn_f = _DialogueRNN(D_m, D_g, D_p, D_e)
        self.dialog_rnn_r = _DialogueRNN(D_m, D_g, D_p, D_e)
        self.matchatt = Transform(2 * D_e)
        self.linear = nn.Linear(2 * D_e, D_h)
        self.smax_fc = nn.Linear(D_h, n_classes)
        # CAPACITY MODE (trainer.StepGraphs buckets, trainer.ResidentEpochs / ResidentEval): the batch tensors are
        # capacity-sized static buffers -- B dialogue slots of which some may have length 0, T the longest dialogue of the
        # split, label [N_cap] -- and every launch is sized for the capacities.  erc_dialogrnn_meta_cap writes the batch's node
        # count to the device (ws["counts"]): the scans take every dialogue's extent from node_off, the loss covers that many
        # rows, and the kernels that own a gradient buffer zero its rows past them, so ONE captured HIP graph serves every
        # batch that fits.
        self.dynamic_n = False
        self.n_speakers = MAX_S                # a resident batch carries speaker ids, not one-hot rows: the trainer names S
        self.flat, self._ws, self._seed = None, WorkspaceCache(), seed
        self._eval_ws = WorkspaceCache()      # eval_scores' own buffers: never those of a (captured) training step

    def live_groups(self):
        groups = []
        for d in DIRS:
            c = getattr(self, d).dialogue_cell
            n = d + ".dialogue_cell."
            # the two input-side weights (and their biases) are neighbours: [900, D_m + 150], one hoisted GEMM per direction
            groups += [[(n + "g_cell.weight_ih", c.g_cell.weight_ih), (n + "p_cell.weight_ih", c.p_cell.weight_ih)],
                       [(n + "g_cell.bias_ih", c.g_cell.bias_ih), (n + "p_cell.bias_ih", c.p_cell.bias_ih)]]
            groups += [[(n + "%s.%s" % (cell, k), getattr(getattr(c, cell), k))]
                       for cell, k in (("g_cell", "weight_hh"), ("g_cell", "bias_hh"), ("p_cell", "weight_hh"), ("p_cell", "bias_hh"),
                                       ("e_cell", "weight_ih"), ("e_cell", "weight_hh"), ("e_cell", "bias_ih"), ("e_cell", "bias_hh"))]
            groups.append([(n + "attention.transform.weight", c.attention.transform.weight)])
        return groups + MatchAttHead.groups("", self)

    def finalize(self, device):
        self.to(device)
        self.flat = FlatParams(self.live_groups(), device)
        self.head = MatchAttHead(self.flat, "", EW, D_HID, self.n_classes, self.drop_p)
        off = self.flat.offsets
        self.offs = capi.dialogrnn_offsets([off[d + ".dialogue_cell." + k] for d in DIRS for k in (
            "g_cell.weight_ih", "g_cell.weight_hh", "g_cell.bias_hh", "p_cell.weight_ih", "p_cell.weight_hh", "p_cell.bias_hh",
            "e_cell.weight_ih", "e_cell.weight_hh", "e_cell.bias_ih", "e_cell.bias_hh")])
        if self.flat.device.type == "cuda":
            self.WT = torch.zeros(capi.dialogrnn_wt_floats(), dtype=torch.float32, device=device)
        self.rng_state = torch.tensor([0, self._seed], dtype=torch.int64, device=device)
        return self

    def _workspace(self, B, T, N, device, cap=False):
        if cap:
            return self._ws.get((B, T, N, "capacity"), lambda: self._make_workspace(B, T, N, device, cap=True))
        return self._ws.get((B, T, N), lambda: self._make_workspace(B, T, N, device))

    def _make_workspace(self, B, T, N, device, cap=False, grads=True):
        """``cap``: capacity mode -- the counts of erc_dialogrnn_meta_cap and the labels a resident step gathers.  ``grads=False``
        (eval_scores): no gradient buffer."""
        # zeros, not empty: a stale NaN must never reach a weight-gradient GEMM through a row the step did not touch
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)
        ws = dict(node_off=i32(B + 1), node_row=i32(N), node_spk=i32(N), GX=f32(N, 2 * GXW), E=f32(N, EW),
                  save=f32(capi.dialogrnn_save_floats(N, B, T)))
        if cap:
            ws.update(counts=i32(2), label=torch.zeros(N, dtype=torch.int64, device=device))
        if grads:
            ws.update(dGX=f32(N, 2 * GXW), dREC=f32(2 * N * capi.DIALOGRNN_DREC_ROW), **self.head.buffers(B, T, N, device))
            ws["dr"] = capi.dialogrnn_planes(ws["dREC"], N, capi.DIALOGRNN_DREC)
        else:
            # what MatchAttHead.forward writes, and nothing of its backward
            ws.update(Q=f32(N, EW), A=f32(N, EW), P=f32(B * T * T), TH=f32(B * T * T), Zc=f32(N, D_HID), logits=f32(N, self.n_classes))
        ws["sv"] = capi.dialogrnn_planes(ws["save"], N, capi.DIALOGRNN_SAVE)
        ws["alpha"] = capi.dialogrnn_alpha(ws["save"], N, B, T)
        ws["planner"] = GemmPlanner(device, 1 << 21, grad=self.flat.grad)
        ws["jobs"] = None
        return ws

    def _check(self, x, onehot, T):
        if T > MAX_T:
            raise capi.ErcGraftError("dialogrnn: the scan keeps the history of the global state in LDS, dialogues of up to %d "
                                     "utterances are supported (batch T=%d)" % (MAX_T, T))
        if int(onehot.shape[-1]) > MAX_S:
            raise capi.ErcGraftError("dialogrnn: n_speakers=%d (up to %d party states are built)" % (int(onehot.shape[-1]), MAX_S))
        if int(x.shape[-1]) != self.D_m:
            raise capi.ErcGraftError("dialogrnn: input_tensor has %d features, D_m=%d" % (int(x.shape[-1]), self.D_m))
        if x.dtype != torch.float32 or onehot.dtype != torch.float32:
            raise capi.ErcGraftError("dialogrnn: input_tensor and speaker_tensor must be fp32 (one-hot speakers)")

    def _drops(self, training):
        return (self.drop_cell, self.drop_emo) if training else (0.0, 0.0)

    def _forward_impl(self, x, onehot, lens, B, T, N, training, with_logits=True):
        self._check(x, onehot, T)
        fp = self.flat
        ws = self._workspace(B, T, N, x.device)
        pl = ws["planner"]
        pl.reset()
        D, S = self.D_m, int(onehot.shape[-1])
        x, onehot = x.contiguous(), onehot.contiguous()
        capi.dialogrnn_meta(onehot, S, lens, B, T, N, ws["node_off"], ws["node_row"], ws["node_spk"])
        capi.dialogrnn_pack(fp.data, self.offs, D, self.WT)
        GX = ws["GX"]
        for d, name in enumerate(DIRS):
            c = name + ".dialogue_cell."
            # [g_cell.weight_ih ; p_cell.weight_ih][:, :D] u + [b_ih^g ; b_ih^p], and W_a u, over the gathered valid rows
            linear_fwd(pl, x, D, ws["node_row"], fp.w(c + "g_cell.weight_ih"), fp.w(c + "g_cell.bias_ih"), GX[:, d * GXW:], 2 * GXW,
                       N, 900, D, ldw=D + D_G)
            linear_fwd(pl, x, D, ws["node_row"], fp.w(c + "attention.transform.weight"), None, GX[:, d * GXW + 900:], 2 * GXW,
                       N, D_G, D)
        p_cell, p_emo = self._drops(training)
        capi.dialogrnn_scan_fwd(GX, 2 * GXW, self.WT, fp.data, self.offs, D, ws["node_off"], ws["node_spk"], B, T, S, N, p_cell, p_emo,
                                self.rng_state, RNG_STREAM, ws["E"], EW, ws["save"])
        self.head.forward(pl, ws, ws["E"], ws["node_off"], B, T, N, training, self.rng_state, with_logits)
        ws["x"], ws["S"] = x, S
        return ws

    def _forward_cap(self, x, onehot, lens, B, T, N, training, desc=None, store_label=None, ws=None, with_logits=False):
        """The forward in CAPACITY mode: B, T, N are capacities, the batch's own node count and longest dialogue are on the
        device (ws["counts"] = [n_dev, t_dev]).  ``desc`` (int32 [2 B]: lengths | first store rows): RESIDENT batch -- x is the
        feature store [U + 1, D] whose last row is zero, read through ws["node_row"], ``onehot`` the store's speaker ids [U]
        (int64), labels are gathered into ws["label"].  ``ws``: the caller's own workspace (eval_scores).

        The rows are compact (node_off[b] + t), so no padded position is ever read: both scans and the matching attention walk
        every dialogue slot through node_off on the device, and a slot of length 0 runs no step.  What is left are the rows
        past the batch, i in [n_dev, N), buffer by buffer (every weight-gradient product runs over all N capacity rows and
        must meet a +0 gradient row wherever the other operand is stale):
          x     gathered through node_row: row 0 of the static block (bucket form) or the appended zero row of the store
                (resident form), both finite; it meets dGX in d W_ih[:, :D] and d W_a, whose capacity rows are +0
                (erc_dialogrnn_scan_bwd_cap).
          GX    capacity rows hold the projection of that row (finite); no scan reads them (their extents end at n_dev) and GX
                enters no weight gradient.
          save  (g'_{s-1}, q[p] before, c, q', e'_{s-1}: the other operands of the recurrent weight gradients), E, A, Zc hold
                what an earlier batch left; finite, because the workspace starts as zeros and only finite values are written.
                save meets the capacity rows of dGX and of the dREC planes dgh_g, dgh_p, dgi_e, dgh_e: +0, both directions
                (erc_dialogrnn_scan_bwd_cap).  E meets dQ in dW_transform; A meets dZc; Zc meets dlogits.
          Q, Zc are GEMMs over all N rows of finite operands: finite.
          dZc, dlogits   +0 past n_dev (erc_head_ce_cap); dA = dZc W is 0 there.
          dQ, dE         +0 past n_dev (erc_match_att_bwd_cap); dE += dQ W adds 0.  The backward scan reads dE below n_dev only.
        The dropout masks inside the scans are keyed by the compact row and the classifier's by (row, column) of Zc (gemm.hip),
        so a bucket step draws the masks of the exact-shape step from the same rng_state."""
        if T > MAX_T:
            raise capi.ErcGraftError("dialogrnn: the scan keeps the history of the global state in LDS, dialogues of up to %d "
                                     "utterances are supported (T_cap=%d)" % (MAX_T, T))
        if x.dtype != torch.float32 or int(x.shape[-1]) != self.D_m:
            raise capi.ErcGraftError("dialogrnn: capacity mode needs fp32 features of width D_m=%d" % self.D_m)
        if desc is None and (lens.dtype != torch.int64 or onehot.dtype != torch.float32 or onehot.dim() != 3):
            raise capi.ErcGraftError("dialogrnn: capacity mode needs int64 text_length and fp32 one-hot speakers [T, B, S]")
        if desc is not None and onehot.dtype != torch.int64:
            raise capi.ErcGraftError("dialogrnn: a resident batch carries the store's int64 speaker ids")
        S = int(onehot.shape[-1]) if desc is None else int(self.n_speakers)
        if not 1 <= S <= MAX_S:
            raise capi.ErcGraftError("dialogrnn: n_speakers=%d (up to %d party states are built)" % (S, MAX_S))
        fp = self.flat
        if ws is None:
            ws = self._workspace(B, T, N, x.device, cap=True)
        pl = ws["planner"]
        pl.reset()
        D = self.D_m
        x = x.contiguous()
        if desc is not None:
            capi.dialogrnn_meta_cap(None, S, None, desc, onehot, store_label, int(x.shape[0]) - 1, B, T, N, ws["node_off"],
                                    ws["node_row"], ws["node_spk"], ws["label"] if store_label is not None else None, ws["counts"])
        else:
            capi.dialogrnn_meta_cap(onehot.contiguous(), S, lens, None, None, None, 0, B, T, N, ws["node_off"], ws["node_row"],
                                    ws["node_spk"], None, ws["counts"])
        capi.dialogrnn_pack(fp.data, self.offs, D, self.WT)
        GX = ws["GX"]
        for d, name in enumerate(DIRS):
            c = name + ".dialogue_cell."
            linear_fwd(pl, x, D, ws["node_row"], fp.w(c + "g_cell.weight_ih"), fp.w(c + "g_cell.bias_ih"), GX[:, d * GXW:], 2 * GXW,
                       N, 900, D, ldw=D + D_G)
            linear_fwd(pl, x, D, ws["node_row"], fp.w(c + "attention.transform.weight"), None, GX[:, d * GXW + 900:], 2 * GXW,
                       N, D_G, D)
        p_cell, p_emo = self._drops(training)
        # B dialogue slots, their extents from node_off: T and N are only the strides of alpha and of the planes (ercgraft.h)
        capi.dialogrnn_scan_fwd(GX, 2 * GXW, self.WT, fp.data, self.offs, D, ws["node_off"], ws["node_spk"], B, T, S, N, p_cell, p_emo,
                                self.rng_state, RNG_STREAM, ws["E"], EW, ws["save"])
        self.head.forward(pl, ws, ws["E"], ws["node_off"], B, T, N, training, self.rng_state, with_logits)
        ws["x"], ws["S"] = x, S
        return ws

    def eval_scores(self, batch, cm):
        """Forward-only step in capacity form, scored on the device: the capacity forward in eval mode (no dropout: the counter
        is not read) on a workspace of its own, smax_fc, and erc_rows_score, which reads the batch's node count from the device
        and ADDS its confusion matrix to ``cm`` (int64 [C, C], true x predicted).  No host synchronisation, capturable.
        ``batch``: a resident batch (``desc`` + ``caps``, as loss_and_grads takes) or a capacity-sized static one.  Returns the
        step's own workspace (``logits`` [N_cap, C]: rows below the device count are valid).  Reads neither ``training`` nor
        ``dynamic_n`` and touches no training state."""
        if self.flat is None:
            raise capi.ErcGraftError("call DialogRNNModule.finalize(device) before eval_scores")
        C = self.n_classes
        if C > capi.rows_score_max_classes():
            raise capi.ErcGraftError("dialogrnn eval_scores: at most %d classes (erc_rows_score)" % capi.rows_score_max_classes())
        x, onehot, lens, ys = batch["input_tensor"], batch["speaker_tensor"], batch["text_length"], batch["label"]
        desc = batch.get("desc")
        B, T, N = batch["caps"] if desc is not None else self._shape(x, lens, ys)
        ws = self._eval_ws.get(("eval", B, T, N), lambda: self._make_workspace(B, T, N, x.device, cap=True, grads=False))
        self._forward_cap(x, onehot, lens, B, T, N, False, desc=desc, store_label=ys if desc is not None else None, ws=ws,
                          with_logits=True)
        capi.rows_score(ws["logits"], C, N, C, N, ws["counts"], None, ws["label"] if desc is not None else ys, cm)
        return ws

    def forward(self, input_tensor, speaker_tensor, attention_mask=None, text_length=None, label=None, **kwargs):
        if self.flat is None:
            raise capi.ErcGraftError("call DialogRNNModule.finalize(device) before forward")
        if self.dynamic_n:
            raise capi.ErcGraftError("dialogrnn: capacity mode (dynamic_n) is the training step's (loss_and_grads) and eval_scores'")
        B, T, N = self._shape(input_tensor, text_length, label, kwargs.get("n_nodes"))
        ws = self._forward_impl(input_tensor, speaker_tensor, text_length, B, T, N, self.training)
        capi.log_softmax_rows(ws["logits"], self.n_classes, self.n_classes, N, ws["logp"], self.n_classes)
        return ws["logp"], ws["E"]

    def loss_and_grads(self, batch, class_weight=None):
        """MaskedNLLLoss(weight) of the log-probabilities (= class-weighted cross entropy of the valid rows' logits) and every
        gradient into flat.grad"""
        x, onehot, lens, ys = batch["input_tensor"], batch["speaker_tensor"], batch["text_length"], batch["label"]
        desc = batch.get("desc")          # resident batch (trainer.ResidentEpochs): the store + 2 B int32 of batch description
        cap = self.dynamic_n or desc is not None
        if cap:
            if not (self.dynamic_n and self.n_classes <= 8):
                raise capi.ErcGraftError("dialogrnn: capacity mode needs dynamic_n and at most 8 classes (erc_head_ce_cap)")
            B, T, N = batch["caps"] if desc is not None else self._shape(x, lens, ys)
            ws = self._forward_cap(x, onehot, lens, B, T, N, self.training, desc=desc, store_label=ys if desc is not None else None)
            if desc is not None:
                ys = ws["label"]
        else:
            B, T, N = self._shape(x, lens, ys)
            ws = self._forward_impl(x, onehot, lens, B, T, N, self.training, with_logits=self.n_classes > 8)
        fp, pl, off = self.flat, ws["planner"], self.flat.offsets
        D, S = self.D_m, ws["S"]
        dE, sv, dr = ws["dE"], ws["sv"], ws["dr"]
        p_cell, p_emo = self._drops(self.training)
        self.head.backward(pl, ws, ws["E"], ws["node_off"], B, T, N, ys, class_weight, self.training,
                           n_dev=ws["counts"] if cap else None, n_cap=N if cap else 0)
        # both scans backwards in one launch (capacity mode: the same launch writes +0 to the rows past the batch of dGX / dREC)
        GX, dGX = ws["GX"], ws["dGX"]
        capi.dialogrnn_scan_bwd(GX, 2 * GXW, self.WT, fp.data, self.offs, D, ws["node_off"], ws["node_spk"], B, T, S, N, p_cell, p_emo,
                                self.rng_state, RNG_STREAM, ws["save"], dE, EW, dGX, 2 * GXW, ws["dREC"],
                                n_dev=ws["counts"] if cap else None)
        ldi = D + D_G
        for d, name in enumerate(DIRS):
            c = name + ".dialogue_cell."
            g0 = d * GXW
            # hoisted products: [d W_ih^g ; d W_ih^p][:, :D] and both input biases in one record, then d W_a
            linear_wgrad(pl, dGX[:, g0:], 2 * GXW, ws["x"], D, ws["node_row"], 900, D, N, off[c + "g_cell.weight_ih"],
                         off[c + "g_cell.bias_ih"], ld_w=ldi, defer=True)
            linear_wgrad(pl, dGX[:, g0 + 900:], 2 * GXW, ws["x"], D, ws["node_row"], D_G, D, N, off[c + "attention.transform.weight"],
                         None, defer=True)
            # recurrent blocks: the state columns of the input-side weights, then the hidden-side weights
            linear_wgrad(pl, dGX[:, g0:], 2 * GXW, sv["q_prev"][d], D_G, None, 450, D_G, N, off[c + "g_cell.weight_ih"], None,
                         ld_w=ldi, col_off=D, defer=True)
            linear_wgrad(pl, dGX[:, g0 + 450:], 2 * GXW, sv["c"][d], D_G, None, 450, D_G, N, off[c + "p_cell.weight_ih"], None,
                         ld_w=ldi, col_off=D, defer=True)
            linear_wgrad(pl, dr["dgh_g"][d], 450, sv["g_prev"][d], D_G, None, 450, D_G, N, off[c + "g_cell.weight_hh"],
                         off[c + "g_cell.bias_hh"], defer=True)
            linear_wgrad(pl, dr["dgh_p"][d], 450, sv["q_prev"][d], D_G, None, 450, D_G, N, off[c + "p_cell.weight_hh"],
                         off[c + "p_cell.bias_hh"], defer=True)
            linear_wgrad(pl, dr["dgi_e"][d], 300, sv["q_drop"][d], D_G, None, 300, D_G, N, off[c + "e_cell.weight_ih"],
                         off[c + "e_cell.bias_ih"], defer=True)
            linear_wgrad(pl, dr["dgh_e"][d], 300, sv["e_prev"][d], D_E, None, 300, D_E, N, off[c + "e_cell.weight_hh"],
                         off[c + "e_cell.bias_hh"], defer=True)
        pl.reduce_into(ws, fp.grad)
        return ws["stats"]


class DialogRNNTrainer(CapacityBuckets, ResidentEvalSteps, ConvEmotionTrainer):
    """train_step / to_logits for ``--module=dialogrnn``: class-weighted MaskedNLLLoss, Adam lr 3e-4, no weight decay (the
    defaults of the sibling plugin, track_mm/dgcnv2.py:22-48,184-219)."""
    NAME = "dialogrnn"

    def __init__(self, params, device):
        # capacity buckets are opt-in: the default stays the exact-shape loop (one graph per batch shape, on its second
        # occurrence)
        super().__init__(params, device, opt_in=True)
        self._store_ext = ZeroRowStores()

    def _build_model(self, params, compute):
        model = DialogRNNModule(params.hidden_all, D_G, D_G, D_E, D_HID, n_classes=params.n_classes, context_attention="general",
                                dropout_rec=params.get("dropout_rec", 0.5), dropout=params.get("dropout", 0.5),
                                compute=compute, seed=params.seed)
        model.n_speakers = min(int(params.n_speakers), MAX_S)      # what a resident step clamps the store's speaker ids to
        return model

    # -- capacity mode: the policy (the implementation is capacity.CapacityBuckets).  N_BUCKET 128 and "a batch of exactly its
    #    bucket's shape stays exact" are the mixin's defaults, and so is the precapture list, built from train.batch_size
    #    and T_cap alone; ``opt_in=True`` (above) makes the buckets opt-in
    TIME_MAJOR = True          # [T, B, D] features, [T, B, S] one-hot speakers
    CLEAR_STALE = False        # the rows are compact and both scans take every dialogue's extent from node_off: no launch
    #                            reads a padded position, so what an earlier batch left there may stay

    def _capacity_ok(self, B_cap, T_cap, N_cap, batch=None):
        """no bucket with the flag off, with the peer-to-peer exchange, above the scans' T, the head's classes or the party
        states' speakers, or for a batch of other dtypes / widths / ranks (the gate is on T_cap: the node launches take any
        N_cap)"""
        ok = (self.capacity and not self._p2p() and 0 < T_cap <= MAX_T and self.model.n_classes <= 8 and
              int(self.params.n_speakers) <= MAX_S)
        if ok and batch is not None:
            x, spk = batch["input_tensor"], batch["speaker_tensor"]
            ok = (x.dtype == torch.float32 and x.dim() == 3 and int(x.shape[2]) == self.model.D_m and spk.dim() == 3 and
                  spk.dtype == torch.float32 and int(spk.shape[2]) <= MAX_S and batch["text_length"].dtype == torch.int64)
        return bool(ok)

    def _resident_ok(self, store, B_cap, T_cap, N_cap):
        return (store.fused.dtype == torch.float32 and int(store.fused.shape[1]) == self.model.D_m and
                store.speaker.dtype == torch.int64 and self._capacity_ok(B_cap, T_cap, N_cap))

    def _resident_inputs(self, store):
        """The hoisted products gather the store's rows through node_row; the capacity rows read a zero row, which the store
        does not have, so the features are kept once per store with one appended.  The speakers are the store's ids:
        erc_dialogrnn_meta_cap reads them at the nodes' store rows."""
        return self._store_ext(store, store.fused), store.speaker
