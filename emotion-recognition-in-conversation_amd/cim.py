"""CIM on the MI355X hot path (drop-in for track_mm/cim.py:64-227).

``CIMModule`` keeps the reference's constructor, ``state_dict`` keys and shapes (``rnn_adapter.*`` included, which is
constructed but never receives a gradient) and ``forward(**batch) -> (logits2 [N, C], logits7 [N, 7])``.  ``cls7.*``
trains only with ``multitask=True`` (apply_multi on CMU-MOSEI, cim.py:206-213); otherwise it stays dead as in the
reference.

Chain, on compact rows (the N = sum(lengths) valid positions, row = node_off[b] + t; csrc/cim_attn.hip erc_cim_meta):
input projections of the three GRUs (one GEMM per modality, both directions: 1200 columns) -> one GRU scan launch for
3 modalities x 2 directions x B dialogues (csrc/gru.hip), drop0 applied by the scan -> adapters Linear(400, 100) + ReLU +
drop1 in the GEMM epilogue, written straight into the dense block (columns 600..900) of the [N, 900] merged buffer -> the
six cross-modal attention ops in one launch into columns 0..600 (csrc/cim_attn.hip) -> cls2 -> cross entropy.  The
backward mirrors it; every weight gradient joins the step's one batched weight-gradient launch (erc_wgrad_table).

Multi-task (``multitask=True``): cls2 and cls7 lie back to back in the flat buffer, one [C + 7, 900] head.  One GEMM
writes both logit blocks, erc_ce_bce_multitask computes cross entropy + 7-way BCE and their gradient in one launch, one
GEMM gives dmerged and one deferred weight-gradient record covers both heads: the same launch count as the single task.
"""
import torch
from torch import nn

from . import capi
from .capacity import CapacityBuckets, ResidentEvalSteps, TrainerBase, ZeroRowStores
from .engine import WorkspaceCache, FlatParams, GemmPlanner, linear_fwd, linear_wgrad

H = 200
MODS = ("a", "v", "t")          # order of the dense block of merged (cim.py:165-172): dense_a, dense_v, dense_t
FEATURE = {"a": "audio_feature", "v": "visual_feature", "t": "text_feature"}
GRU_STREAM = 0xC1A0           # counter-RNG stream of drop0 (+ modality index)
MERGED = 900


class CIMModule(nn.Module):
    def __init__(self, text_dim, audio_dim, visual_dim, hidden_size, n_classes, drop0=0.3, drop1=0.3, compute="f32", seed=1,
                 multitask=False):
        super().__init__()
        if hidden_size != H:
            raise capi.ErcGraftError("CIM: the GRU scan kernels are built for hidden_size 200 (cim.py:183-184), got %d"
                                     % hidden_size)
        if compute != "f32":
            raise capi.ErcGraftError("CIM runs in fp32 only (the reference is fp32); --compute=%s is not supported" % compute)
        self.dims = {"t": text_dim, "a": audio_dim, "v": visual_dim}
        self.n_classes, self.compute, self.multitask = n_classes, compute, bool(multitask)
        self.p0, self.p1 = float(drop0), float(drop1)
        self.rnn = nn.ModuleDict({m: nn.GRU(self.dims[m], hidden_size=H, bidirectional=True, batch_first=True) for m in "tav"})
        self.rnn_adapter = nn.ModuleDict({m: nn.Linear(self.dims[m], 2 * H) for m in "tav"})
        self.drop0 = nn.ModuleDict({m: nn.Dropout(drop0) for m in "tav"})
        self.adapter = nn.ModuleDict({m: nn.Sequential(nn.Linear(2 * H, 100), nn.ReLU()) for m in "tav"})
        self.drop1 = nn.ModuleDict({m: nn.Dropout(drop1) for m in "tav"})
        self.cls2 = nn.Linear(100 * 9, n_classes)
        self.cls7 = nn.Linear(100 * 9, 7)
        self.flat, self._ws, self._seed = None, WorkspaceCache(), seed
        # CAPACITY MODE (trainer.StepGraphs buckets, trainer.ResidentEpochs / ResidentEval): the batch tensors are capacity-sized
        # static buffers -- B_cap dialogue slots of which some may have length 0, T_cap utterances, label [N_cap] -- or the
        # HBM-resident store itself, and every launch is sized for (B_cap, T_cap, N_cap).  The step runs on compact rows anyway
        # and never reads a padded position; erc_cim_meta_cap writes the batch's own row count to the device (ws["counts"]), the
        # scans and the attention walk the dialogues through node_off / lengths and so never touch the TAIL rows [n, N_cap), and
        # the loss reads the count: ONE captured HIP graph serves every batch that fits.  The tail invariant is stated with
        # _forward_impl and loss_and_grads.
        self.dynamic_n = False
        self._eval_ws = WorkspaceCache()      # eval_scores' own buffers: never those of a (captured) training step

    def live_groups(self):
        """FlatParams groups: forward|reverse members adjacent (one [1200, d] W_ih per modality), and the six W_hh / b_hh in one
        group each, in (a, v, t) x (forward, reverse) order -- the [6][600][200] block the scan kernels index by 2 m + d."""
        g = []
        for m in MODS:
            r = self.rnn[m]
            g.append([("rnn.%s.weight_ih_l0" % m, r.weight_ih_l0), ("rnn.%s.weight_ih_l0_reverse" % m, r.weight_ih_l0_reverse)])
            g.append([("rnn.%s.bias_ih_l0" % m, r.bias_ih_l0), ("rnn.%s.bias_ih_l0_reverse" % m, r.bias_ih_l0_reverse)])
        for kind in ("weight", "bias"):
            g.append([("rnn.%s.%s_hh_l0%s" % (m, kind, sfx), getattr(self.rnn[m], "%s_hh_l0%s" % (kind, sfx)))
                      for m in MODS for sfx in ("", "_reverse")])
        for m in MODS:
            g.append([("adapter.%s.0.weight" % m, self.adapter[m][0].weight)])
            g.append([("adapter.%s.0.bias" % m, self.adapter[m][0].bias)])
        if self.multitask:      # one [C + 7, 900] head: cls2 rows, then cls7 rows
            g += [[("cls2.weight", self.cls2.weight), ("cls7.weight", self.cls7.weight)],
                  [("cls2.bias", self.cls2.bias), ("cls7.bias", self.cls7.bias)]]
        else:
            g += [[("cls2.weight", self.cls2.weight)], [("cls2.bias", self.cls2.bias)]]
        return g

    def finalize(self, device):
        self.to(device)
        self.flat = FlatParams(self.live_groups(), device)
        self.rng_state = torch.tensor([0, self._seed], dtype=torch.int64, device=device)
        # drop1 of the three adapters: the GEMM epilogue keys its mask by (rng_state, row * 100 + col), so each modality gets a
        # seed of its own (rng_state + salt, one device add per step: no host synchronisation)
        self._salt = torch.tensor([[0, 0], [0, 0xA1 << 32], [0, 0xA2 << 32]], dtype=torch.int64, device=device)
        self.rng3 = torch.zeros(3, 2, dtype=torch.int64, device=device)
        return self

    @property
    def _last_ws(self):
        return self._ws.last

    # ------------------------------------------------------------------ flat views
    def _span(self, first, rows, cols, grad=False):
        off = self.flat.offsets[first]
        buf = self.flat.grad if grad else self.flat.data
        return buf[off:off + rows * cols].view(rows, cols)

    def _w_ih(self, m):
        return self._span("rnn.%s.weight_ih_l0" % m, 2 * 3 * H, self.dims[m])

    def _b_ih(self, m):
        return self._span("rnn.%s.bias_ih_l0" % m, 1, 2 * 3 * H).view(-1)

    def _w_hh6(self):
        return self._span("rnn.a.weight_hh_l0", 6 * 3 * H, H)

    def _b_hh6(self):
        return self._span("rnn.a.bias_hh_l0", 1, 6 * 3 * H).view(-1)

    def _head(self):
        """(weight [C + 7, 900], bias [C + 7]) of cls2 | cls7 (multitask layout)"""
        C7 = self.n_classes + 7
        return self._span("cls2.weight", C7, MERGED), self._span("cls2.bias", 1, C7).view(-1)

    # ------------------------------------------------------------------ workspace
    def _workspace(self, B, T, N, device, cap=False):
        if cap:
            return self._ws.get((B, T, N, "capacity"), lambda: self._make_workspace(B, T, N, device, cap=True))
        return self._ws.get((B, T, N), lambda: self._make_workspace(B, T, N, device))

    def _make_workspace(self, B, T, N, device, cap=False, grads=True):
        """``cap``: a capacity step's workspace -- plus what erc_cim_meta_cap writes (the clamped lengths the scans read, the
        batch's counts, the labels gathered from a resident store).  ``grads`` False (eval_scores): the forward's buffers alone."""
        # zeros, not empty: every buffer is fully written before it is read, but a stale NaN must never reach a
        # weight-gradient GEMM through a row the step did not touch
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
        g32 = f32 if grads else (lambda *s: None)      # the backward's buffers
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)
        C = self.n_classes + (7 if self.multitask else 0)     # multitask: logits / dlogits hold cls2 | cls7
        ws = dict(node_off=i32(B + 1), node_row=i32(max(N, 1)), GX=f32(3, N, 6 * H), gates=f32(3, N, 6 * H), ghn=f32(3, N, 2 * H),
                  Hprev=f32(3, N, 2 * H), Hout=f32(3, N, 2 * H), Hdrop=f32(3, N, 2 * H), merged=f32(N, MERGED),
                  P=f32(6 * B * T * T), logits=f32(N, C), logits7=f32(N, 7), dlogits=g32(N, C), dmerged=g32(N, MERGED),
                  dH=g32(3, N, 2 * H), dGX=g32(3, N, 6 * H), dGH=g32(3, N, 6 * H), WT=f32(6, H, 3 * H),
                  stats=f32(max(256, capi.head_ce_stats_floats(N))))
        if cap:
            i64 = lambda *s: torch.zeros(*s, dtype=torch.int64, device=device)
            ws.update(lens=i64(B), counts=i32(2), label=i64(N), emo_label=i64(N, 7))
        dmax = max(self.dims.values())
        ws["planner"] = GemmPlanner(device, 16 * N * 6 * H + 8 * 6 * H * dmax + (1 << 20), grad=self.flat.grad)
        return ws

    def _shape(self, batch, label=None):
        x = batch["text_feature"]
        B, T = int(x.shape[0]), int(x.shape[1])
        if label is not None:
            N = int(label.shape[0])
        elif batch.get("n_nodes") is not None:
            N = int(batch["n_nodes"])
        else:
            N = int(batch["text_length"].sum().item())
        return B, T, N

    def _check_batch(self, batch, T):
        for m in MODS:
            if batch.get(FEATURE[m]) is None:
                raise capi.ErcGraftError("CIM needs all three modalities (--modality=atv): %s is missing" % FEATURE[m])
        if T > capi.cim_max_t():
            raise capi.ErcGraftError("CIM: dialogues of up to %d utterances are supported (batch T=%d)" % (capi.cim_max_t(), T))

    # ------------------------------------------------------------------ forward
    def _meta_cap(self, ws, batch, B, T, N, desc):
        """erc_cim_meta_cap into ``ws`` in the bucket form (int64 lengths + the padded [B_cap, T_cap, d_m] blocks) or the resident
        form (``desc``: int32 [2 B] lengths | first store rows; the features are the per-modality stores [U + 1, d_m] with a
        zero row appended, label / emo_label the store's).  Returns the features the GEMMs gather from through node_row."""
        if not 0 < N <= B * T:
            raise capi.ErcGraftError("CIM capacity mode: N_cap = %d outside [1, B_cap * T_cap = %d]" % (N, B * T))
        feats = {m: batch[FEATURE[m]] for m in MODS}
        out = (ws["node_off"], ws["node_row"], ws["lens"])
        if desc is not None:
            U = int(feats["t"].shape[0]) - 1
            label, emo = batch["label"], batch.get("emo_label") if self.multitask else None
            if desc.dtype != torch.int32 or int(desc.numel()) != 2 * B or label.dtype != torch.int64 or int(label.numel()) != U or \
                    any(x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous() or tuple(x.shape) != (U + 1, self.dims[m])
                        for m, x in feats.items()) or \
                    (emo is not None and (emo.dtype != torch.int64 or tuple(emo.shape) != (U, 7) or not emo.is_contiguous())):
                raise capi.ErcGraftError("CIM resident batch: per-modality fp32 features [U + 1, d_m] (a zero row appended), int64 "
                                         "labels [U] (emo_label [U, 7]), desc int32 [2 B]")
            capi.cim_meta_cap(None, desc, label, emo, U, B, T, N, *out, ws["label"], ws["emo_label"] if emo is not None else None,
                              ws["counts"])
            return feats
        lens = batch["text_length"]
        # tail nodes gather row ``tail_row`` of every block: the zero row a trainer's bucket keeps behind it (row B_cap * T_cap),
        # else row 0 -- in bounds, and finite like all features
        tail_row = int(batch.get("tail_row") or 0)
        for m, x in feats.items():
            rows = (int(x.untyped_storage().nbytes()) // 4 - x.storage_offset()) // self.dims[m]      # readable from x's first
            if x.dtype != torch.float32 or tuple(x.shape) != (B, T, self.dims[m]) or not x.is_contiguous() or tail_row >= rows:
                raise capi.ErcGraftError("CIM capacity mode needs contiguous fp32 %s [B_cap, T_cap, %d] (and the row tail_row = %d "
                                         "inside its storage)" % (FEATURE[m], self.dims[m], tail_row))
        if lens.dtype != torch.int64 or int(lens.numel()) != B:
            raise capi.ErcGraftError("CIM capacity mode needs int64 text_length [B_cap]")
        capi.cim_meta_cap(lens, None, None, None, tail_row, B, T, N, *out, None, None, ws["counts"])
        return feats

    def _forward_impl(self, batch, B, T, N, training, logits7=False, capacity=None, desc=None, ws=None):
        """``capacity`` (None = the module's ``dynamic_n``): B / T / N are the capacities (B_cap, T_cap, N_cap) every launch is
        sized for, and the batch's own row count is on the device (ws["counts"][0], written by erc_cim_meta_cap).  ``desc``
        (int32 [2 B]: lengths | first store rows): RESIDENT batch -- the three input GEMMs gather the store rows of the nodes
        through node_row.  ``ws``: the caller's own workspace (eval_scores).

        The tail invariant, forward half (rows [n, N_cap)): GX's tail is Linear(the features of tail_row), and
        Hout, Hdrop, merged and the logits hold there what an earlier batch left (zeros at first), all of it finite; the scans and
        the attention walk node_off / lengths and neither read nor write a tail row, the adapter and head GEMMs map rows to rows."""
        capacity = self.dynamic_n if capacity is None else capacity
        if desc is not None and not capacity:
            raise capi.ErcGraftError("CIM: a resident batch (desc) runs in capacity mode (dynamic_n)")
        self._check_batch(batch, T)
        fp = self.flat
        dev = batch["text_feature"].device
        if ws is None:
            ws = self._workspace(B, T, N, dev, cap=capacity)
        pl = ws["planner"]
        pl.reset()
        p0, p1 = (self.p0, self.p1) if training else (0.0, 0.0)
        if capacity:
            feats, lens = self._meta_cap(ws, batch, B, T, N, desc), ws["lens"]
        else:
            lens = batch["text_length"]
            capi.cim_meta(lens, B, T, N, ws["node_off"], ws["node_row"])
            feats = {m: batch[FEATURE[m]].contiguous() for m in MODS}
        ws["feats"], ws["lens_used"] = feats, lens
        for i, m in enumerate(MODS):
            linear_fwd(pl, feats[m], self.dims[m], ws["node_row"], self._w_ih(m), self._b_ih(m), ws["GX"][i], 6 * H, N, 6 * H,
                       self.dims[m])
        capi.transpose_batched(self._w_hh6(), 6, 3 * H, H, ws["WT"])
        hsrc = ws["Hdrop"] if p0 > 0 else ws["Hout"]
        capi.gru_scan_fwd(ws["GX"], ws["WT"], self._b_hh6(), lens, ws["node_off"], B, T, N, ws["Hout"],
                          ws["Hdrop"] if p0 > 0 else None, p0, self.rng_state, GRU_STREAM, ws["gates"], ws["ghn"], ws["Hprev"])
        if p1 > 0:
            torch.add(self.rng_state.unsqueeze(0), self._salt, out=self.rng3)
        merged = ws["merged"]
        for i, m in enumerate(MODS):
            linear_fwd(pl, hsrc[i], 2 * H, None, fp.w("adapter.%s.0.weight" % m), fp.w("adapter.%s.0.bias" % m),
                       merged[:, 600 + 100 * i:], MERGED, N, 100, 2 * H, act=3 if p1 > 0 else 1, drop_p=p1,
                       rng=self.rng3[i] if p1 > 0 else None)
        capi.cim_attn_fwd(merged, ws["node_off"], B, T, ws["P"])
        if self.multitask:
            C7 = self.n_classes + 7
            w, b = self._head()
            linear_fwd(pl, merged, MERGED, None, w, b, ws["logits"], C7, N, C7, MERGED)
        else:
            linear_fwd(pl, merged, MERGED, None, fp.w("cls2.weight"), fp.w("cls2.bias"), ws["logits"], self.n_classes, N,
                       self.n_classes, MERGED)
        if logits7 and not self.multitask:
            linear_fwd(pl, merged, MERGED, None, self.cls7.weight, self.cls7.bias, ws["logits7"], 7, N, 7, MERGED)
        ws["hsrc"], ws["p"] = hsrc, (p0, p1)
        return ws

    def forward(self, text_feature=None, audio_feature=None, visual_feature=None, text_length=None, attention_mask=None,
                *args, **kwargs):
        if self.flat is None:
            raise capi.ErcGraftError("call CIMModule.finalize(device) before forward")
        batch = dict(text_feature=text_feature, audio_feature=audio_feature, visual_feature=visual_feature,
                     text_length=text_length, n_nodes=kwargs.get("n_nodes"))
        if text_feature is None:
            raise capi.ErcGraftError("CIM needs all three modalities (--modality=atv): text_feature is missing")
        B, T, N = self._shape(batch, kwargs.get("label"))
        ws = self._forward_impl(batch, B, T, N, self.training, logits7=True, capacity=False)
        if self.multitask:
            C = self.n_classes
            return ws["logits"][:, :C], ws["logits"][:, C:]
        return ws["logits"], ws["logits7"]

    def supports_capacity(self, B_cap, T_cap):
        """Can a step of B_cap dialogue slots of up to T_cap utterances run in capacity mode?  The attention keeps a dialogue in
        LDS (T_cap <= erc_cim_max_t()), erc_cim_meta_cap prefixes up to 1024 slots, and the scoring kernel has a class limit."""
        return 0 < B_cap <= 1024 and 0 < T_cap <= capi.cim_max_t() and self.n_classes <= capi.rows_score_max_classes()

    def eval_scores(self, batch, cm):
        """Forward-only step in capacity form, scored on the device: erc_cim_meta_cap, the forward in eval mode (no dropout: the
        counter is not read) and erc_rows_score on the cls2 logits, which reads the batch's row count from the device and ADDS its
        confusion matrix to ``cm`` (int64 [C, C], true x predicted).  No host synchronisation, capturable.  ``batch``: a resident
        batch (``desc`` + ``caps``, as loss_and_grads takes) or a capacity-sized static one.  Returns the step's own workspace
        (``logits`` [N_cap, C (+ 7)]: rows below the device count are valid).  Reads neither ``training`` nor ``dynamic_n`` and
        touches no training state."""
        if self.flat is None:
            raise capi.ErcGraftError("call CIMModule.finalize(device) before eval_scores")
        if self.n_classes > capi.rows_score_max_classes():
            raise capi.ErcGraftError("CIM eval_scores: at most %d classes (erc_rows_score)" % capi.rows_score_max_classes())
        desc, ys = batch.get("desc"), batch["label"]
        B, T, N = batch["caps"] if desc is not None else self._shape(batch, ys)
        dev = batch["text_feature"].device
        ws = self._eval_ws.get(("eval", B, T, N), lambda: self._make_workspace(B, T, N, dev, cap=True, grads=False))
        self._forward_impl(batch, B, T, N, False, capacity=True, desc=desc, ws=ws)
        C = self.n_classes
        capi.rows_score(ws["logits"], int(ws["logits"].shape[1]), N, C, N, ws["counts"], None, ws["label"] if desc is not None else ys,
                        cm)
        return ws

    # ------------------------------------------------------------------ training step
    def loss_and_grads(self, batch):
        """F.cross_entropy(logits2, label) (unweighted mean, cim.py:204) -- plus, multitask,
        F.binary_cross_entropy_with_logits(logits7, emo_label.float()) (cim.py:206-213) -- and every live gradient into
        flat.grad.  Returns the stats buffer: [0] Lall, [1] #correct, multitask also [2] Lce, [3] Lmulti.

        ``batch``: the collated batch; in capacity mode (``dynamic_n``) capacity-sized static buffers or a RESIDENT batch
        (``desc`` + ``caps``: trainer.ResidentEpochs).  The tail invariant, backward half (rows [n, N_cap)): every
        gradient buffer that enters a weight-gradient product is exactly 0 there, so those products run over all N_cap rows.
        dlogits: written 0 by erc_ce_bce_multitask_cap (single task: erc_mm_zero_tail behind erc_cross_entropy_cap); dmerged =
        dlogits W and dH = dpre W_adapter: GEMMs over N_cap rows, zero rows in, zero rows out (the attention backward touches
        the rows of a dialogue only); dGX / dGH: written 0 by erc_gru_scan_bwd_cap."""
        ys = batch["label"]
        desc = batch.get("desc")          # resident batch (trainer.ResidentEpochs): the stores + 2 B int32 of batch description
        cap = self.dynamic_n
        if desc is not None and not cap:
            raise capi.ErcGraftError("CIM: a resident batch (desc) runs in capacity mode (dynamic_n)")
        if desc is not None:
            B, T, N = batch["caps"]
        else:
            B, T, N = self._shape(batch, ys)
        if self.multitask and batch.get("emo_label") is None:
            raise capi.ErcGraftError("CIM multitask (apply_multi) needs emo_label in the batch (a CMU-MOSEI dataset)")
        ws = self._forward_impl(batch, B, T, N, self.training, capacity=cap, desc=desc)
        nd = ws["counts"] if cap else None      # capacity mode: N above is the capacity, the batch's count is here
        emo = batch.get("emo_label")
        if desc is not None:
            ys, emo = ws["label"], ws["emo_label"]
        fp, pl, off = self.flat, ws["planner"], self.flat.offsets
        C, (p0, p1) = self.n_classes, ws["p"]
        merged, dmerged = ws["merged"], ws["dmerged"]
        if self.multitask:
            C7 = C + 7
            if cap:
                capi.ce_bce_multitask_cap(ws["logits"], C7, C, N, nd, ys, emo, emo.stride(0), 1.0, 1.0, 1.0, ws["dlogits"], C7,
                                          ws["stats"])
            else:
                capi.ce_bce_multitask(ws["logits"], C7, C, N, ys, emo, emo.stride(0), 1.0, 1.0, 1.0, ws["dlogits"], C7, ws["stats"])
            capi.gemm_f32(ws["dlogits"], C7, 0, None, self._head()[0], MERGED, 1, None, dmerged, MERGED, N, MERGED, C7)
            linear_wgrad(pl, ws["dlogits"], C7, merged, MERGED, None, C7, MERGED, N, off["cls2.weight"], off["cls2.bias"],
                         defer=True)
        else:
            if cap:      # the loss writes the batch's rows: the tail still holds those of an earlier, larger batch
                capi.cross_entropy_cap(ws["logits"], C, C, N, nd, None, ys, None, 1.0, ws["dlogits"], C, ws["stats"])
                capi.mm_zero_tail(ws["dlogits"], C, C, 1, N, nd)
            else:
                capi.cross_entropy(ws["logits"], C, C, N, None, ys, None, 1.0, ws["dlogits"], C, ws["stats"])
            capi.gemm_f32(ws["dlogits"], C, 0, None, fp.w("cls2.weight"), MERGED, 1, None, dmerged, MERGED, N, MERGED, C)
            linear_wgrad(pl, ws["dlogits"], C, merged, MERGED, None, C, MERGED, N, off["cls2.weight"], off["cls2.bias"],
                         defer=True)
        # attention backward: + d dense_m into columns 600..900, then through drop1 / ReLU
        capi.cim_attn_bwd(merged, dmerged, ws["node_off"], B, T, ws["P"], 1.0 / (1.0 - p1))
        hsrc = ws["hsrc"]
        for i, m in enumerate(MODS):
            dpre = dmerged[:, 600 + 100 * i:]
            linear_wgrad(pl, dpre, MERGED, hsrc[i], 2 * H, None, 100, 2 * H, N, off["adapter.%s.0.weight" % m],
                         off["adapter.%s.0.bias" % m], defer=True)
            capi.gemm_f32(dpre, MERGED, 0, None, fp.w("adapter.%s.0.weight" % m), 2 * H, 1, None, ws["dH"][i], 2 * H, N, 2 * H, 100)
        scan = (self._w_hh6(), ws["lens_used"], ws["node_off"], B, T, N, ws["gates"], ws["ghn"], ws["Hprev"], ws["dH"], p0,
                self.rng_state, GRU_STREAM, ws["dGX"], ws["dGH"])
        if cap:
            capi.gru_scan_bwd_cap(*scan, N)
        else:
            capi.gru_scan_bwd(*scan)
        for i, m in enumerate(MODS):
            d_m = self.dims[m]
            linear_wgrad(pl, ws["dGX"][i], 6 * H, ws["feats"][m], d_m, ws["node_row"], 6 * H, d_m, N,
                         off["rnn.%s.weight_ih_l0" % m], off["rnn.%s.bias_ih_l0" % m], defer=True)
            for d, sfx in enumerate(("", "_reverse")):
                linear_wgrad(pl, ws["dGH"][i][:, 3 * H * d:], 6 * H, ws["Hprev"][i][:, H * d:], 2 * H, None, 3 * H, H, N,
                             off["rnn.%s.weight_hh_l0%s" % (m, sfx)], off["rnn.%s.bias_hh_l0%s" % (m, sfx)], defer=True)
        pl.reduce_into(ws, fp.grad)
        return ws["stats"]


class CIMTrainer(CapacityBuckets, ResidentEvalSteps, TrainerBase):
    """train_step / to_logits / to_mosei_multitask_logits of track_mm/cim.py:180-227: unweighted cross entropy on logits2
    (apply_bin), plus the 7-way BCE on logits7 when apply_multi (CMU-MOSEI only, cim.py:52-53); torch.optim.Adam(lr)
    without clipping or weight decay.  apply_bin=False is refused: the reference's cls2 would then get neither a gradient
    nor Adam state, a layout this port does not build."""
    # -- capacity mode: the policy (the implementation is capacity.CapacityBuckets; the table in DESIGN.md).  Opt-in
    #    (--capacity_buckets=True; --resident implies it): the default stays the exact-shape step.  The GEMMs and the scans'
    #    buffers scale with N_cap: N_BUCKET 128, as elsewhere.
    CLASS_WEIGHTED = False
    TIME_MAJOR = False         # [B, T, d_m] feature blocks per modality
    CLEAR_STALE = False        # the step runs on compact rows gathered through node_row: a padded position (t >= length, or any
    #                            t of an empty slot) is never read, so what an earlier batch left there cannot matter

    def __init__(self, params, device):
        self.params, self.device = params, torch.device(device)
        if not params.get("apply_bin", True):
            raise capi.ErcGraftError("--module=cim: --apply_bin=False is not supported (the cross-entropy term on cls2 is "
                                     "always trained here)")
        if params.modality != "atv":
            raise ValueError("--module=cim needs all three modalities: the GRUs of cim.py:136-146 run on text, audio and visual "
                             "features (--modality=atv), got --modality=%s" % params.modality)
        compute = params.get("compute", "f32")
        if compute != "f32":
            raise ValueError("--module=cim runs in fp32 (the reference is fp32); --compute=%s is not supported" % compute)
        torch.manual_seed(params.seed)
        self.multitask = bool(params.get("apply_multi", False))
        self.model = CIMModule(text_dim=params.hidden_text, audio_dim=params.hidden_audio, visual_dim=params.hidden_visual,
                               hidden_size=H, n_classes=params.n_classes, seed=params.seed,
                               multitask=self.multitask).finalize(self.device)
        self._make_optim(opt_in=True)
        self._store_ext = ZeroRowStores()

    def to_mosei_multitask_logits(self, batch):
        """(logits2 [N, C], logits7 [N, 7]) (mmbase.py:144, cim.py:190-191)"""
        return self.model(**batch)

    # ------------------------------------------------------------------ capacity mode
    def _feature_keys(self):
        return tuple(FEATURE[m] for m in MODS)

    def _capacity_ok(self, B_cap, T_cap, N_cap, batch=None):
        """no bucket with the flag off; with the peer-to-peer exchange; beyond what the attention's LDS, the prefix kernel or the
        scoring kernel take (``supports_capacity``); or for a batch of other dtypes / ranks / widths than the plugin's (on
        CMU-MOSEI: without its int64 emo_label [N, 7]).  The exact-shape path runs then."""
        ok = self.capacity and not self._p2p() and 0 < N_cap <= B_cap * T_cap and self.model.supports_capacity(B_cap, T_cap)
        if ok and batch is not None:
            spk, lens, emo = batch.get("speaker_tensor"), batch.get("text_length"), batch.get("emo_label")
            ok = torch.is_tensor(spk) and spk.dim() >= 2 and torch.is_tensor(lens) and lens.dtype == torch.int64 and \
                all(torch.is_tensor(batch.get(FEATURE[m])) and batch[FEATURE[m]].dim() == 3 and
                    batch[FEATURE[m]].dtype == torch.float32 and int(batch[FEATURE[m]].shape[2]) == self.model.dims[m]
                    for m in MODS) and \
                (not self.multitask or (torch.is_tensor(emo) and emo.dtype == torch.int64 and emo.dim() == 2 and
                                        int(emo.shape[1]) == 7))
        return bool(ok)

    def _caps(self, batch):
        if not all(torch.is_tensor(batch.get(k)) and batch[k].dim() >= 2 for k in self._feature_keys()):
            return 0, 0      # a batch the gate refuses (a modality is missing)
        return super()._caps(batch)

    def _bucket(self, like, B_cap, T_cap, N_cap):
        """The mixin's bucket, plus what CIM's step wants of it: a zero row behind every feature block (static["tail_row"] =
        B_cap * T_cap: the row the tail nodes gather, so that GX's tail rows are Linear(0)) and, on CMU-MOSEI, the multi-hot
        emo_label [N_cap, 7] of the multi-task loss: the batch's rows are copied in as label's are, and the rows a larger earlier
        batch left behind them are cleared.  (The mixin, with CLEAR_STALE off, leaves label's tail stale; the loss stops at the
        device count and reads neither tail.)"""
        key, make0, fill0 = super()._bucket(like, B_cap, T_cap, N_cap)
        multi, dev, rows = self.multitask, self.device, B_cap * T_cap

        def make():
            static = make0()
            for k in self._feature_keys():
                block = torch.zeros(rows + 1, int(like[k].shape[2]), dtype=like[k].dtype, device=dev)
                static[k] = block[:rows].view(B_cap, T_cap, -1)
            static["tail_row"] = rows
            if multi:
                static["emo_label"] = torch.zeros(N_cap, 7, dtype=torch.int64, device=dev)
                static["emo_rows"] = 0          # host side: the rows the last batch filled
            return static

        def fill(static, b):
            fill0(static, b)
            if multi:
                Nb = int(b["emo_label"].shape[0])
                static["emo_label"][:Nb].copy_(b["emo_label"], non_blocking=True)
                if static["emo_rows"] > Nb:
                    static["emo_label"][Nb:static["emo_rows"]].zero_()
                static["emo_rows"] = Nb

        return key, make, fill

    def _resident_ok(self, store, B_cap, T_cap, N_cap):
        emo = getattr(store, "extra", {}).get("emo_label")
        return all(m in store.feats and store.feats[m].dtype == torch.float32 and store.feats[m].dim() == 2 and
                   int(store.feats[m].shape[1]) == self.model.dims[m] for m in MODS) and \
            (not self.multitask or (torch.is_tensor(emo) and emo.dtype == torch.int64 and emo.dim() == 2 and
                                    int(emo.shape[1]) == 7)) and \
            self._capacity_ok(B_cap, T_cap, N_cap)

    def resident_batch(self, store, cur_desc, B_cap, T_cap, N_cap):
        """trainer.ResidentEpochs: the "batch" of a step whose dialogues stay in the HBM-resident store -- the per-modality
        stores, each kept once per store with a zero row appended (the row the tail nodes gather), the flat labels (on
        CMU-MOSEI also ``store.extra["emo_label"]``), the 2 B_cap int32 the host rewrites per step and the capacities the
        launches are sized for.  None when the step cannot run that way (``_resident_ok``)."""
        if not self._resident_ok(store, B_cap, T_cap, N_cap):
            return None
        feats = self._store_ext(store, {m: store.feats[m] for m in MODS})
        batch = {FEATURE[m]: feats[m] for m in MODS}
        batch.update(speaker_tensor=store.speaker, text_length=None, label=store.label, desc=cur_desc,
                     caps=(B_cap, T_cap, N_cap))
        if self.multitask:
            batch["emo_label"] = store.extra["emo_label"]
        return batch
