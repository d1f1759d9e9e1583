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
from .capacity import TrainerBase
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
    def _workspace(self, B, T, N, device):
        return self._ws.get((B, T, N), lambda: self._make_workspace(B, T, N, device))

    def _make_workspace(self, B, T, N, device):
        # zeros, not empty: every buffer is fully written before it is read, but a stale NaN must never reach a
        # weight-gradient GEMM through a row the step did not touch
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)
        C = self.n_classes + (7 if self.multitask else 0)     # multitask: logits / dlogits hold cls2 | cls7
        ws = dict(node_off=i32(B + 1), node_row=i32(max(N, 1)), GX=f32(3, N, 6 * H), gates=f32(3, N, 6 * H), ghn=f32(3, N, 2 * H),
                  Hprev=f32(3, N, 2 * H), Hout=f32(3, N, 2 * H), Hdrop=f32(3, N, 2 * H), merged=f32(N, MERGED),
                  P=f32(6 * B * T * T), logits=f32(N, C), logits7=f32(N, 7), dlogits=f32(N, C), dmerged=f32(N, MERGED),
                  dH=f32(3, N, 2 * H), dGX=f32(3, N, 6 * H), dGH=f32(3, N, 6 * H), WT=f32(6, H, 3 * H),
                  stats=f32(max(256, capi.head_ce_stats_floats(N))))
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
    def _forward_impl(self, batch, B, T, N, training, logits7=False):
        self._check_batch(batch, T)
        fp, lens = self.flat, batch["text_length"]
        dev = lens.device
        ws = self._workspace(B, T, N, dev)
        pl = ws["planner"]
        pl.reset()
        p0, p1 = (self.p0, self.p1) if training else (0.0, 0.0)
        capi.cim_meta(lens, B, T, N, ws["node_off"], ws["node_row"])
        feats = {m: batch[FEATURE[m]].contiguous() for m in MODS}
        ws["feats"] = feats
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
        ws = self._forward_impl(batch, B, T, N, self.training, logits7=True)
        if self.multitask:
            C = self.n_classes
            return ws["logits"][:, :C], ws["logits"][:, C:]
        return ws["logits"], ws["logits7"]

    # ------------------------------------------------------------------ training step
    def loss_and_grads(self, batch):
        """F.cross_entropy(logits2, label) (unweighted mean, cim.py:204) -- plus, multitask,
        F.binary_cross_entropy_with_logits(logits7, emo_label.float()) (cim.py:206-213) -- and every live gradient into
        flat.grad.  Returns the stats buffer: [0] Lall, [1] #correct, multitask also [2] Lce, [3] Lmulti."""
        ys = batch["label"]
        B, T, N = self._shape(batch, ys)
        if self.multitask and batch.get("emo_label") is None:
            raise capi.ErcGraftError("CIM multitask (apply_multi) needs emo_label in the batch (a CMU-MOSEI dataset)")
        ws = self._forward_impl(batch, B, T, N, self.training)
        fp, pl, off = self.flat, ws["planner"], self.flat.offsets
        C, (p0, p1) = self.n_classes, ws["p"]
        merged, dmerged = ws["merged"], ws["dmerged"]
        if self.multitask:
            emo = batch["emo_label"]
            C7 = C + 7
            capi.ce_bce_multitask(ws["logits"], C7, C, N, ys, emo, emo.stride(0), 1.0, 1.0, 1.0, ws["dlogits"], C7, ws["stats"])
            capi.gemm_f32(ws["dlogits"], C7, 0, None, self._head()[0], MERGED, 1, None, dmerged, MERGED, N, MERGED, C7)
            linear_wgrad(pl, ws["dlogits"], C7, merged, MERGED, None, C7, MERGED, N, off["cls2.weight"], off["cls2.bias"],
                         defer=True)
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
        capi.gru_scan_bwd(self._w_hh6(), batch["text_length"], ws["node_off"], B, T, N, ws["gates"], ws["ghn"], ws["Hprev"],
                          ws["dH"], p0, self.rng_state, GRU_STREAM, ws["dGX"], ws["dGH"])
        for i, m in enumerate(MODS):
            d_m = self.dims[m]
            linear_wgrad(pl, ws["dGX"][i], 6 * H, ws["feats"][m], d_m, ws["node_row"], 6 * H, d_m, N,
                         off["rnn.%s.weight_ih_l0" % m], off["rnn.%s.bias_ih_l0" % m], defer=True)
            for d, sfx in enumerate(("", "_reverse")):
                linear_wgrad(pl, ws["dGH"][i][:, 3 * H * d:], 6 * H, ws["Hprev"][i][:, H * d:], 2 * H, None, 3 * H, H, N,
                             off["rnn.%s.weight_hh_l0%s" % (m, sfx)], off["rnn.%s.bias_hh_l0%s" % (m, sfx)], defer=True)
        pl.reduce_into(ws, fp.grad)
        return ws["stats"]


class CIMTrainer(TrainerBase):
    """train_step / to_logits / to_mosei_multitask_logits of track_mm/cim.py:180-227: unweighted cross entropy on logits2
    (apply_bin), plus the 7-way BCE on logits7 when apply_multi (CMU-MOSEI only, cim.py:52-53); torch.optim.Adam(lr)
    without clipping or weight decay.  apply_bin=False is refused: the reference's cls2 would then get neither a gradient
    nor Adam state, a layout this port does not build."""
    CLASS_WEIGHTED = False

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
        self._make_optim()

    def to_mosei_multitask_logits(self, batch):
        """(logits2 [N, C], logits7 [N, 7]) (mmbase.py:144, cim.py:190-191)"""
        return self.model(**batch)
