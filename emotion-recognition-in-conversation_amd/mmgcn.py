"""MMGCN on the MI355X hot path (drop-in for track_mm/mmgcn.py:56-157).

``MMGCNModule`` keeps the reference's constructor signature, ``state_dict`` keys (the
constructed-but-unused ``att_model.*``, ``gatedatt.*`` and ``graph_model.{a_fc,...}`` parameters included) and
``forward(**batch) -> (logits [N,C], None)`` on the time-major batch layout (batch_first=False, one-hot speakers).

Chain: per-modality Linear(d_m,200) on the padded [T,B,.] blocks (+ unpacked BiLSTM on text, rnn.py) -> valid
rows, modality-major node order [a | v | l(+speaker embedding)] -> block-structured adjacency (cosine blocks by a
grouped MFMA GEMM, arccos similarity, cross-modal same-utterance entries, symmetric degree normalisation) ->
64 GCNII layers, each: grouped block product A*h + cross terms, [hi | h0] W_l as two accumulating GEMMs,
fused theta/alpha combine + ReLU + dropout -> regroup + dropout + ReLU -> Linear -> CE; hand-written backward
including the gradient THROUGH the adjacency into the features (the reference's adjacency is built with autograd
on, mmgcn_models.py:582-646).
"""
import math

import torch
from torch import nn

from . import capi
from .capacity import CapacityBuckets, ResidentEvalSteps, TrainerBase, ZeroRowStores
from .engine import WorkspaceCache, FlatParams, GemmPlanner, SideStream, linear_fwd, linear_wgrad, \
    matmul_wgrad_io
from .rnn import BiLSTM2, lstm_groups

FD, NLAYERS, LAMDA, ALPHA, DROP = 200, 64, 0.5, 0.1, 0.4
KSPLIT = 16      # parts of the layer-plane sums in the backward (adjacency / h0 gradients); 8 .. 32 measured alike
_KEY = {"a": "audio_feature", "v": "visual_feature", "t": "text_feature"}
_LIN = {"a": "linear_a", "v": "linear_v", "t": "linear_l"}


class _Holder(nn.Module):
    """Registers parameters by dotted name: sub-modules the reference constructs but never uses."""

    def __init__(self, table=()):
        super().__init__()
        for name, shape in table:
            self._add(name, shape)

    def _add(self, name, shape):
        head, _, rest = name.partition(".")
        if rest:
            if not hasattr(self, head):
                setattr(self, head, _Holder())
            getattr(self, head)._add(rest, shape)
        else:
            self.register_parameter(name, nn.Parameter(torch.zeros(*shape).uniform_(-0.05, 0.05)))


class _Conv(nn.Module):
    def __init__(self):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(2 * FD, FD).uniform_(-1.0 / math.sqrt(FD), 1.0 / math.sqrt(FD)))


class _GraphNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.convs = nn.ModuleList([_Conv() for _ in range(NLAYERS)])
        self.fcs = nn.ModuleList([nn.Linear(FD, FD)])


class _GraphModel(_Holder):
    def __init__(self, n_classes, n_speakers):
        super().__init__([("a_fc.weight", (FD, FD)), ("a_fc.bias", (FD,)), ("v_fc.weight", (FD, FD)), ("v_fc.bias", (FD,)),
                          ("l_fc.weight", (FD, FD)), ("l_fc.bias", (FD,)), ("feature_fc.weight", (FD, 6 * FD)),
                          ("feature_fc.bias", (FD,)), ("final_fc.weight", (n_classes, FD)), ("final_fc.bias", (n_classes,)),
                          ("modal_embeddings.weight", (3, FD)), ("a_spk_embs.weight", (n_speakers, FD)),
                          ("v_spk_embs.weight", (n_speakers, FD)), ("l_spk_embs.weight", (n_speakers, FD))])
        self.graph_net = _GraphNet()
        self.speaker_embeddings = nn.Embedding(n_speakers, FD)


def _unused_tables():
    att = [("scalar.weight", (200, 200)), ("matchatt.transform.weight", (200, 200)), ("matchatt.transform.bias", (200,)),
           ("simpleatt.scalar.weight", (1, 200)), ("att.weight", (400,)), ("att.w_k.weight", (200, 200)),
           ("att.w_k.bias", (200,)), ("att.w_q.weight", (200, 200)), ("att.w_q.bias", (200,)),
           ("att.proj.weight", (200, 200)), ("att.proj.bias", (200,))]
    gated = []
    for n in ("l", "v", "a"):
        gated += [("transform_%s.weight" % n, (200, 400)), ("transform_%s.bias" % n, (200,))]
    for n in ("av", "al", "vl"):
        gated += [("transform_%s.weight" % n, (1, 1200)), ("transform_%s.bias" % n, (1,))]
    return att, gated


class MMGCNModule(nn.Module):
    X3_SPLIT = 10      # K splits of dh0 = DG U^T on erc_gemm_x3 (K = 12 800: 50 output tiles x 10 = 500 workgroups)

    def __init__(self, hidden_text=100, D_e=100, graph_hidden_size=200, n_speakers=2, max_seq_len=200, window_past=10,
                 window_future=10, n_classes=7, nodal_attention=True, hidden_visual=512, hidden_audio=100, modals="atv",
                 seed=1):
        super().__init__()
        if len(modals) < 2:
            raise NotImplementedError("MMGCN needs at least two modalities (mmgcn_models.py:594-595)")
        self.modals, self.n_speakers, self.n_classes = modals, n_speakers, n_classes
        self.dims = {"a": hidden_audio, "v": hidden_visual, "t": hidden_text}
        self.order = [m for m in "avt" if m in modals]            # [a, v, l] order of create_big_adj
        self.linear_l = nn.Linear(hidden_text, FD)
        self.lstm_l = nn.LSTM(FD, 100, 2, bidirectional=True, dropout=DROP)
        self.linear_a = nn.Linear(hidden_audio, FD)
        self.linear_v = nn.Linear(hidden_visual, FD)
        att, gated = _unused_tables()
        self.att_model = _Holder(att)
        self.graph_model = _GraphModel(n_classes, n_speakers)
        self.gatedatt = _Holder(gated)
        self.smax_fc = nn.Linear(2 * FD * len(modals), n_classes)
        self.drop_p = DROP
        self.flat, self._ws, self._seed = None, WorkspaceCache(), seed
        # CAPACITY MODE (trainer.StepGraphs buckets, trainer.ResidentEpochs / ResidentEval): the batch tensors are capacity-sized
        # static buffers -- B_cap dialogue slots of which some may have length 0, T_cap the longest dialogue of the split, label
        # [N_cap] -- and every launch is sized for (B_cap, T_cap, N_cap).  Modality m's node rows start at m * N_cap; the batch's
        # own node count and longest dialogue are written to the device by erc_mm_meta_cap (ws["counts"] = [n_dev, t_dev]).  The
        # adjacency kernels, the grouped products and the GCNII chain walk the dialogues through node_off (a slot of length 0 has
        # no block and no workgroup) and so never touch the TAIL rows [m * N_cap + n, (m + 1) * N_cap); the row operators run their
        # capacity instances (erc_*_cap) and the BiLSTM *t_dev steps, so ONE captured HIP graph serves every batch that fits.
        # The tail invariant is stated with _forward_impl.
        self.dynamic_n = False
        self._eval_ws = WorkspaceCache()      # eval_scores' own buffers: never those of a (captured) training step
        self._chain_fits = {}                 # (B_cap, T_cap) -> does the one-launch chain take it (chain_fits)

    def live_groups(self):
        groups = []
        for m in self.order:
            lin = getattr(self, _LIN[m])
            groups += [[(_LIN[m] + ".weight", lin.weight)], [(_LIN[m] + ".bias", lin.bias)]]
        if "t" in self.order:
            groups += lstm_groups("lstm_l.", self.lstm_l)
            groups += [[("graph_model.speaker_embeddings.weight", self.graph_model.speaker_embeddings.weight)]]
        gn = self.graph_model.graph_net
        groups += [[("graph_model.graph_net.fcs.0.weight", gn.fcs[0].weight)],
                   [("graph_model.graph_net.fcs.0.bias", gn.fcs[0].bias)]]
        groups += [[("graph_model.graph_net.convs.%d.weight" % i, gn.convs[i].weight)] for i in range(NLAYERS)]
        groups += [[("smax_fc.weight", self.smax_fc.weight)], [("smax_fc.bias", self.smax_fc.bias)]]
        return groups

    def finalize(self, device):
        self.to(device)
        self.flat = FlatParams(self.live_groups(), device)
        self.lstm = BiLSTM2(self.flat, "lstm_l.", FD, drop_p=DROP) if "t" in self.order else None
        self.rng_state = torch.tensor([0, self._seed], dtype=torch.int64, device=device)
        self.side = SideStream()
        return self

    @property
    def _last_ws(self):
        """workspace of the most recent forward (tests / bench read results out of it)"""
        return self._ws.last

    def _workspace(self, B, T, N, device, cap=False):
        if cap:
            return self._ws.get((B, T, N, "capacity"), lambda: self._make_workspace(B, T, N, device, cap=True))
        return self._ws.get((B, T, N), lambda: self._make_workspace(B, T, N, device))

    def chain_fits(self, B, T):
        """Does the one-launch GCNII chain (csrc/gcnii_chain.hip) take B dialogue slots of up to T utterances?  ``parts`` is
        what erc_gcnii_chain_config can know without the lengths: whether the chain form is on at this T and whether the
        B * modalities worst-case parts can be resident, a launch's share at a time."""
        import os
        if os.environ.get("ERC_MM_CHAIN", "1") == "0" or not 0 < T <= 128 or B < 1:
            return False
        fits = self._chain_fits.get((B, T))
        if fits is None:      # asked per step by the trainer's gate: the device is queried once per (B, T)
            Mo, P = len(self.order), (T + 3) // 4 * 4
            try:
                parts, grid_cap, per_launch = capi.gcnii_chain_config(B, T, Mo, P)
                fits = per_launch >= 1 and grid_cap >= per_launch * Mo * ((T + 31) // 32)
            except capi.ErcGraftError:
                fits = False
            self._chain_fits[(B, T)] = fits
        return fits

    def _make_workspace(self, B, T, N, device, cap=False, grads=True):
        """``cap``: a capacity step's workspace -- plus the tables of erc_mm_meta_cap, one zero row behind the node gradient dX,
        and without the per-layer planes only the launch-per-layer form (ERC_MM_CHAIN=0, which capacity mode refuses) uses.
        ``grads`` False (eval_scores): the forward's buffers alone."""
        ws = self._make_workspace_exact(B, T, N, device, planes=1 if cap else NLAYERS + 1, tail_row=1 if cap else 0, grads=grads)
        if cap:
            if not ws["chain"]:
                raise capi.ErcGraftError("MMGCN capacity mode runs the one-launch GCNII chain (ERC_MM_CHAIN != 0, T_cap <= 128)")
            i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)
            ws.update(node_pad=i32(N), pad_node=i32(T * B), x_row=i32(T * B), counts=i32(2),
                      label=torch.zeros(N, dtype=torch.int64, device=device))
        return ws

    def _make_workspace_exact(self, B, T, N, device, planes=NLAYERS + 1, tail_row=0, grads=True):
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
        g32 = f32 if grads else (lambda *s: None)      # the backward's buffers
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)
        Mo, C = len(self.order), self.n_classes
        R3, TB, P = Mo * N, T * B, (T + 3) // 4 * 4
        ws = dict(P=P, node_off=i32(B + 1), node_row=i32(N), node_dlg=i32(N), node_spk=i32(N),
                  LIN={m: f32(TB, FD) for m in self.order}, LO=f32(TB, FD), X=f32(R3, FD), XD=f32(R3, FD),
                  XH=f32(R3, FD), INV=f32(R3), COS=f32(B * Mo, P, P), ADJ=f32(B * Mo, P, P), CR=f32(B, Mo * Mo, P),
                  CCOS=f32(B, Mo * Mo, P), DEG=f32(R3), DDEG=f32(R3), H0=f32(R3, FD), Gt=f32(R3, FD),
                  HI=f32(planes, R3, 2 * FD), HD=f32(NLAYERS + 2, R3, FD), FE=f32(N, Mo * 2 * FD), logits=f32(N, C),
                  stats=torch.zeros(256, dtype=torch.float32, device=device), dlogits=g32(N, C), dFE=g32(N, Mo * 2 * FD), dXD=g32(R3, FD), DH=g32(R3, FD),
                  dG=g32(planes, R3, FD), dHIa=g32(planes, R3, FD), dH0=g32(R3, FD),
                  dADJs=g32(KSPLIT, B * Mo, P, P), dH0s=g32(KSPLIT + 1 if planes > 1 else 1, R3, FD),
                  emb_ws=g32(capi.mm_emb_grad_ws_floats(self.n_speakers)), dADJ=g32(B * Mo, P, P), dCR=g32(B, Mo * Mo, P),
                  Gb=g32(B * Mo, P, P), GC=g32(B, Mo * Mo, P), dXH=g32(R3, FD), dX=g32(R3 + tail_row, FD),
                  dLIN={m: g32(TB, FD) for m in self.order}, dLL=g32(TB, FD))
        import os
        ws["chain"] = os.environ.get("ERC_MM_CHAIN", "1") != "0" and T <= 128 and NLAYERS == 64 and FD == 200
        if ws["chain"]:
            # K8 (csrc/gcnii_chain.hip): the 64 layers in one persistent launch per direction
            LDS = NLAYERS * FD
            ws["chain_cfg"] = capi.gcnii_chain_config(B, T, Mo, P)
            ws["VT"], ws["V"] = f32(NLAYERS + 1, FD, 208), f32(NLAYERS + 1, FD, 208)
            ws["U"], ws["Call"] = f32(FD, LDS), f32(R3, LDS)
            # the two 16 GFLOP products around the chain (Call = h0 U, dh0 = DG U^T) as three-term bf16 splits on the bf16 matrix
            # cores (csrc/gemm_x3.hip: fp32-class, 2.4 x the exact-fp32 tiles); ERC_MM_GEMM_X3=0 keeps erc_gemm_f32
            ws["gemm_x3"] = os.environ.get("ERC_MM_GEMM_X3", "1") != "0"
            if ws["gemm_x3"]:
                ws["UT"], ws["dH0s3"] = f32(LDS, FD), g32(self.X3_SPLIT * R3 * FD)
            ws["ZS"], ws["DGl"], ws["DZl"] = f32(R3, LDS), g32(R3, LDS), g32(R3, LDS)
            ws["ZX"], ws["DH1"] = f32(2, R3, FD), g32(R3, FD)
            ws["chain_state"] = i32(1 + B + B * Mo * ws["chain_cfg"][0])
        dmax = max(self.dims[m] for m in self.order)
        slab = 4 * TB * 800 + 8 * (800 * FD + 2 * 400 * 100 * 2) + 8 * FD * dmax * 3 + NLAYERS * 2 * 8 * FD * FD + \
            8 * FD * FD + 8 * self.n_classes * Mo * 2 * FD + 8 * R3 * FD + (1 << 21)
        ws["planner"] = GemmPlanner(device, slab, grad=self.flat.grad)
        ws["planner"].MAX_SPLIT = 8      # 128 weight-gradient GEMMs per step: keep their slab sets small
        # ERC_MM_X3=1: weight gradients as three-term bf16 splits (csrc/wgrad.hip MB == 2: fp32-class products on the bf16
        # matrix cores).  Measured: 3.456 -> 3.421 ms per step -- the operand split on the VALU (two truncations, two
        # subtractions, three packs per value) eats most of what the matrix cores give back.  On by default with the other
        # fp32-class products (erc_gemm_x3); ERC_MM_X3=0 ERC_MM_GEMM_X3=0 is the exact-fp32 step.
        ws["planner"].mma_bf16 = 2 if os.environ.get("ERC_MM_X3", "1") == "1" else 0
        ws["jobs"] = None
        return ws

    def check_cluster(self):
        """Raise if a GCNII chain kernel (csrc/gcnii_chain.hip) flagged a per-layer exchange wait that ran into its bound.
        The affected optimizer steps were skipped ON THE DEVICE, on every rank (FusedAdam.skip_flag = the health word the
        chain kernels raise, summed over the ranks by the gradient all-reduce); the trainer calls this once per epoch
        after the training loop and after the evaluation loop, as for DAG-ERC."""
        self.flat.check_health("MMGCN GCNII chain")

    def _shape(self, batch_feat, lens, label, n_nodes=None):
        T, B = batch_feat.shape[0], batch_feat.shape[1]
        N = int(label.shape[0]) if label is not None else (int(n_nodes) if n_nodes is not None else int(lens.sum().item()))
        return B, T, N

    @staticmethod
    def theta(l):
        return math.log(LAMDA / l + 1)

    # ---------------------------------------------------------------- forward
    def _meta_cap(self, ws, qmask, lens, B, T, N, desc, store_label, n_store):
        """erc_mm_meta_cap into ``ws`` in the bucket form (lengths + padded one-hot qmask) or the resident form (``desc``:
        int32 [2 B] lengths | first store rows; qmask = the store's flat speaker ids)"""
        if not 0 < N <= B * T:
            raise capi.ErcGraftError("MMGCN capacity mode: N_cap = %d outside [1, B_cap * T_cap = %d]" % (N, B * T))
        out = (ws["node_off"], ws["node_row"], ws["node_pad"], ws["node_dlg"], ws["node_spk"], ws["pad_node"])
        if desc is not None:
            if qmask.dim() != 1 or qmask.dtype != torch.int64 or desc.dtype != torch.int32 or int(desc.numel()) != 2 * B or \
                    int(qmask.shape[0]) != n_store or (store_label is not None and store_label.dtype != torch.int64):
                raise capi.ErcGraftError("MMGCN resident batch: per-modality features [U + 1, d] (a zero row appended), flat int64 "
                                         "speaker ids and labels [U], desc int32 [2 B]")
            capi.mm_meta_cap(None, None, 0, 0, self.n_speakers, desc, qmask, store_label, n_store, B, T, N, *out, ws["x_row"],
                             ws["label"] if store_label is not None else None, ws["counts"])
            return
        if lens.dtype != torch.int64 or qmask.dim() != 3 or qmask.dtype != torch.float32 or qmask.stride(2) != 1 or \
                tuple(qmask.shape[:2]) != (T, B):
            raise capi.ErcGraftError("MMGCN capacity mode needs int64 text_length and fp32 one-hot speakers [T_cap, B_cap, S]")
        capi.mm_meta_cap(lens, qmask, qmask.stride(0), qmask.stride(1), qmask.shape[2], None, None, None, 0, B, T, N, *out, None, None,
                         ws["counts"])

    def _forward_impl(self, feats, qmask, lens, B, T, N, training, capacity=None, desc=None, store_label=None, ws=None):
        """``capacity`` (None = the module's ``dynamic_n``): B / T / N are the capacities (B_cap, T_cap, N_cap) every launch is
        sized for, and the batch's own node count and longest dialogue are on the device (ws["cap"] = (B_cap, T_cap, N_cap, n_dev,
        t_dev), written by erc_mm_meta_cap).  ``desc`` (int32 [2 B]: lengths | first store rows): RESIDENT batch -- feats[m] is
        modality m's feature store [U + 1, d_m] with a zero row appended, qmask the store's flat speaker ids, ``store_label`` its
        labels; the audio / visual Linear gathers the store rows of the nodes (node_row), the text Linear those of the padded rows
        (x_row: the zero row where t >= length, which is what the reference's zero padding is).  ``ws``: the caller's own
        workspace (eval_scores).

        The tail invariant (rows [m * N_cap + n, (m + 1) * N_cap) of a node buffer): a tail row's content is finite,
        and no tail row contributes to the loss, to a weight, bias, embedding or adjacency gradient, or to the confusion matrix.
        Forward: X's tail is Linear(a readable sentinel row) for audio / visual and 0 for text; XH, INV, XD (dropout on) and FE
        are written 0 there; H0, Call and the logits are finite functions of those; nothing that walks node_off reads a tail row.
        The BiLSTM runs *t_dev steps (its reverse direction starts at the batch's own T) and writes 0 at t >= *t_dev."""
        capacity = self.dynamic_n if capacity is None else capacity
        if desc is not None and not capacity:
            raise capi.ErcGraftError("MMGCN: a resident batch (desc) runs in capacity mode (dynamic_n)")
        fp = self.flat
        dev = qmask.device
        if ws is None:
            ws = self._workspace(B, T, N, dev, cap=capacity)
        pl = ws["planner"]
        pl.reset()
        Mo, C, TB, P = len(self.order), self.n_classes, T * B, ws["P"]
        R3 = Mo * N
        p = self.drop_p if training else 0.0
        rng = self.rng_state
        nd = x_row = td = None
        if capacity:
            n_store = int(feats[self.order[0]].shape[0]) - 1 if desc is not None else 0
            self._meta_cap(ws, qmask, lens, B, T, N, desc, store_label, n_store)
            nd, td = ws["counts"], ws["counts"][1:]
            x_row = ws["x_row"] if desc is not None else None
            ws["cap"] = (B, T, N, nd, td)
        else:
            if qmask.stride(2) != 1:
                qmask = qmask.contiguous()
            capi.mm_meta(lens, qmask, qmask.stride(0), qmask.stride(1), qmask.shape[2], B, ws["node_off"], ws["node_row"],
                         ws["node_dlg"], ws["node_spk"])
        X = ws["X"]
        for mi, m in enumerate(self.order):
            x = feats[m].reshape(-1, self.dims[m])       # the padded [T,B,.] block as TB rows (resident: the store's rows)
            if m != "t":
                # audio / visual: Linear only -- computed for the N valid utterances straight into node order (the padded rows
                # and the gather behind them are not needed; the text branch keeps them for its unpacked LSTM)
                linear_fwd(pl, x, self.dims[m], ws["node_row"], fp.w(_LIN[m] + ".weight"), fp.w(_LIN[m] + ".bias"),
                           X[mi * N:], FD, N, FD, self.dims[m])
                continue
            linear_fwd(pl, x, self.dims[m], x_row, fp.w(_LIN[m] + ".weight"), fp.w(_LIN[m] + ".bias"), ws["LIN"][m], FD, TB,
                       FD, self.dims[m])
            src = ws["LIN"][m]
            emb = spk = None
            if m == "t":
                # unpacked BiLSTM over the padded [T,B,200] block (row(b,t) = t*B + b): mmgcn.py:113-114
                self.lstm.forward(pl, ws["LIN"][m], FD, TB, B, T, 1, B, None, training, rng, ws["LO"], FD, store=ws, t_dev=td)
                src, emb, spk = ws["LO"], fp.w("graph_model.speaker_embeddings.weight"), ws["node_spk"]
            if capacity:
                capi.mm_flatten_cap(src, FD, ws["node_pad"], emb, spk, N, nd, X[mi * N:], FD)
            else:
                capi.mm_flatten(src, FD, ws["node_row"], emb, spk, N, X[mi * N:], FD)
        # adjacency (mmgcn_models.py:582-646)
        if capacity:
            capi.mm_row_normalize_cap(X, Mo, N, nd, ws["XH"], ws["INV"])
        else:
            capi.mm_row_normalize(X, R3, ws["XH"], ws["INV"])
        capi.gemm_grouped(1, ws["XH"], FD, ws["XH"], FD, ws["COS"], P, FD, ws["node_off"], B, Mo, N, T, P)
        capi.mm_adj_finish(ws["COS"], ws["XH"], ws["node_off"], B, Mo, N, P, ws["ADJ"], ws["CR"], ws["CCOS"], ws["DEG"])
        # GCNII input layer (mmgcn_models.py:382-384)
        n_el = R3 * FD
        XD = ws["XD"] if p > 0 else X

        def dropout(x, stream_id, y):
            if capacity:
                capi.dropout_fwd_cap(x, Mo, N, nd, FD, p, rng, stream_id, y)
            else:
                capi.dropout_fwd(x, n_el, p, rng, stream_id, y)
        if p > 0:
            dropout(X, 1000, XD)
        gn = "graph_model.graph_net."
        HD, HI = ws["HD"], ws["HI"]
        # h0 = relu(fc0 x); the chain's first plane is dropout(h0): without dropout the product writes it in place
        H0 = ws["H0"] if p > 0 else HD[1]
        linear_fwd(pl, XD, FD, None, fp.w(gn + "fcs.0.weight"), fp.w(gn + "fcs.0.bias"), H0, FD, R3, FD, FD, act=1)
        if p > 0:
            dropout(H0, 1001, HD[1])
        ws["_H0"] = H0
        if ws["chain"]:
            # K8: V_l / U_l from the layer weights, c_l = h0 U_l for all 64 layers as ONE product, then the whole chain in one
            # persistent launch (adjacency rows resident in LDS; csrc/gcnii_chain.hip)
            Wn0 = gn + "convs.0.weight"
            w_stride = fp.offsets[gn + "convs.1.weight"] - fp.offsets[Wn0]
            LDS = NLAYERS * FD
            capi.gcnii_chain_prep(fp.w(Wn0), w_stride, LAMDA, ALPHA, ws["VT"], ws["V"], ws["U"], ws.get("UT"))
            if ws["gemm_x3"]:
                capi.gemm_x3(H0, FD, ws["UT"], FD, ws["Call"], LDS, R3, LDS, FD)
            else:
                capi.gemm_f32(H0, FD, 0, None, ws["U"], LDS, 1, None, ws["Call"], LDS, R3, LDS, FD)
            capi.gcnii_chain_fwd(ws["ADJ"], P, ws["CR"], ws["node_off"], N, Mo, B, T, ws["chain_cfg"], ws["VT"], ws["Call"], LDS,
                                 HD, R3 * FD, ws["ZS"], LDS, ws["ZX"], ws["chain_state"], p, rng, 2000, health=fp.health)
        else:
            # every layer's input rows are [hi_l | h0] (pitch 2 FD): h0 is copied next to the 64 hi slots once per step, so that
            # [hi | h0] W is ONE product per layer, with the GCNII tail (residual mix, relu, dropout) in its epilogue
            HI[1:, :, FD:] = H0
            for l in range(1, NLAYERS + 1):
                W = fp.w(gn + "convs.%d.weight" % (l - 1))
                capi.gemm_grouped(0, ws["ADJ"], P, HD[l], FD, HI[l], 2 * FD, FD, ws["node_off"], B, Mo, N, T, P, cross=ws["CR"])
                capi.gcnii_layer_fwd(HI[l], 2 * FD, W, FD, self.theta(l), ALPHA, p, rng, 2000 + l, HD[l + 1], FD, R3, FD)
        if capacity:
            capi.mm_regroup_fwd_cap(XD, HD[NLAYERS + 1], Mo, N, nd, p, rng, 3000, ws["FE"])
        else:
            capi.mm_regroup_fwd(XD, HD[NLAYERS + 1], Mo, N, p, rng, 3000, ws["FE"])
        linear_fwd(pl, ws["FE"], Mo * 2 * FD, None, fp.w("smax_fc.weight"), fp.w("smax_fc.bias"), ws["logits"], C, N, C,
                   Mo * 2 * FD)
        ws["_p"], ws["_XD"] = p, XD
        return ws

    def _feats(self, kw):
        return {m: kw[_KEY[m]] for m in self.order}

    def forward(self, text_feature=None, audio_feature=None, visual_feature=None, speaker_tensor=None,
                text_length=None, label=None, **kwargs):
        if self.flat is None:
            raise capi.ErcGraftError("call MMGCNModule.finalize(device) before forward")
        feats = self._feats(dict(text_feature=text_feature, audio_feature=audio_feature, visual_feature=visual_feature))
        B, T, N = self._shape(feats[self.order[0]], text_length, label, kwargs.get("n_nodes"))
        ws = self._forward_impl(feats, speaker_tensor, text_length, B, T, N, self.training, capacity=False)
        return ws["logits"], None

    def supports_capacity(self, B_cap, T_cap):
        """Can a step of B_cap dialogue slots of up to T_cap utterances run in capacity mode?  It needs the one-launch chain
        (``chain_fits``) and a class count the scoring kernel takes."""
        return self.n_classes <= capi.rows_score_max_classes() and self.chain_fits(B_cap, T_cap)

    def eval_scores(self, batch, cm):
        """Forward-only step in capacity form, scored on the device: erc_mm_meta_cap, the forward in eval mode (p = 0: no
        dropout launch, the counter is not read) and erc_rows_score, which reads the batch's node count from the device and ADDS
        its confusion matrix to ``cm`` (int64 [C, C], true x predicted).  No host synchronisation, capturable.  ``batch``: a
        resident batch (``desc`` + ``caps``, as loss_and_grads takes) or a capacity-sized static one.  Returns the step's own
        workspace (``logits`` [N_cap, C]: rows below the device count are valid).  Reads neither ``training`` nor ``dynamic_n``
        and touches no training state."""
        if self.flat is None:
            raise capi.ErcGraftError("call MMGCNModule.finalize(device) before eval_scores")
        feats, qmask, lens, ys = self._feats(batch), batch["speaker_tensor"], batch["text_length"], batch["label"]
        desc = batch.get("desc")
        B, T, N = batch["caps"] if desc is not None else (qmask.shape[1], qmask.shape[0], int(ys.shape[0]))
        if self.n_classes > capi.rows_score_max_classes():
            raise capi.ErcGraftError("MMGCN eval_scores: at most %d classes (erc_rows_score)" % capi.rows_score_max_classes())
        ws = self._eval_ws.get(("eval", B, T, N), lambda: self._make_workspace(B, T, N, qmask.device, cap=True, grads=False))
        self._forward_impl(feats, qmask, lens, B, T, N, False, capacity=True, desc=desc, store_label=ys if desc is not None else None,
                           ws=ws)
        C = self.n_classes
        capi.rows_score(ws["logits"], C, N, C, N, ws["counts"], None, ws["label"] if desc is not None else ys, cm)
        return ws

    def _legacy_chain_backward(self, ws, pl, DH, B, T, N, p, ks):
        """Round-1 form of the chain's backward (ERC_MM_CHAIN=0): launches per layer."""
        fp, off = self.flat, self.flat.offsets
        Mo, P = len(self.order), ws["P"]
        R3, n_el = Mo * N, Mo * N * FD
        HD, HI = ws["HD"], ws["HI"]
        gn = "graph_model.graph_net."
        # Per layer only what the NEXT layer's gradient needs stays on the dependency chain: dG_l, dhi_l = its residual
        # part + dG_l W_l[:FD]^T, and DH = A^T dhi_l.  Everything that only meets in a sum over the layers -- the
        # adjacency gradient sum_l dhi_l h_l^T, its cross-modal entries, the h0 gradient sum_l dG_l W_l[FD:]^T and the
        # weight gradients -- is computed after the loop, one launch each over all 64 layer planes.
        dHIa, dH0 = ws["dHIa"], ws["dH0"]
        dH0e = ws["dH0s"][KSPLIT]          # elementwise residual contributions to dh0: the last slab of the dh0 sum
        dH0e.zero_(), ws["dCR"].zero_()
        for l in range(NLAYERS, 0, -1):
            Wn = gn + "convs.%d.weight" % (l - 1)
            W = fp.w(Wn)
            dG, dhi = ws["dG"][l], dHIa[l]
            capi.gcnii_combine_bwd(DH, HD[l + 1], n_el, self.theta(l), ALPHA, ks, 0, dG, dhi, dH0e, F=FD, ld_d=FD)
            capi.gemm_f32(dG, FD, 0, None, W, FD, 0, None, dhi, FD, R3, FD, FD, accumulate=1)          # dhi += dG W[:FD]^T
            matmul_wgrad_io(pl, HI[l], 2 * FD, dG, FD, 2 * FD, FD, R3, off[Wn], None, defer=True)        # dW = [hi|h0]^T dG
            capi.gemm_grouped(0, ws["ADJ"], P, dhi, FD, DH, FD, FD, ws["node_off"], B, Mo, N, T, P, cross=ws["CR"])
        # the sums over the layer planes, cut into KSPLIT parts each (slabs, reduced in order)
        plane, n_adj = R3 * FD, B * Mo * P * P
        capi.gemm_grouped(1, dHIa[1], FD, HD[1], FD, ws["dADJs"], P, FD, ws["node_off"], B, Mo, N, T, P, planes=NLAYERS,
                          a_plane=plane, b_plane=plane, split=KSPLIT, c_slab=n_adj)
        capi.slab_reduce(ws["dADJs"], KSPLIT, n_adj, None, P, 0, ws["dADJ"], n_adj)
        capi.mm_cross_grad(dHIa[1], FD, HD[1], FD, ws["node_dlg"], ws["node_off"], Mo, N, P, ws["dCR"], planes=NLAYERS,
                           d_plane=plane, h_plane=plane)
        w_stride = off[gn + "convs.1.weight"] - off[gn + "convs.0.weight"]
        assert all(off[gn + "convs.%d.weight" % i] == off[gn + "convs.0.weight"] + i * w_stride for i in range(NLAYERS))
        W_bot = fp.data[off[gn + "convs.0.weight"] + FD * FD:]                                        # rows FD.. of layer 1's weight
        capi.gemm_f32_planes(ws["dG"][1], FD, plane, W_bot, FD, w_stride, ws["dH0s"], FD, R3, FD, FD, NLAYERS,
                             split_k=KSPLIT, c_slab=n_el)
        capi.slab_reduce(ws["dH0s"], KSPLIT + 1, n_el, None, FD, 0, dH0, n_el)
        return DH, dH0

    # --------------------------------------------------------------- training
    def loss_and_grads(self, batch):
        """``batch``: the collated batch; in capacity mode (``dynamic_n``) capacity-sized static buffers or a RESIDENT batch
        (``desc`` + ``caps``: trainer.ResidentEpochs).  Backward half of the tail invariant (_forward_impl): the gradient-side tail
        rows -- dlogits, dFE, DH, DGl, DZl, dH0, dG0, dX (dXD) and dXH -- are exactly zero, so the weight-gradient products may run
        over all Mo * N_cap (T_cap * B_cap) rows.  dlogits is cleared and erc_cross_entropy_cap writes the batch's rows; dFE, dG0's
        and dXD's products carry zero rows through; the row operators' capacity instances write 0; the buffers whose valid rows
        the chain or a grouped product writes (DGl, DZl, dXH) get their tail rows cleared by erc_mm_zero_tail."""
        feats = self._feats(batch)
        qmask, lens, ys = batch["speaker_tensor"], batch["text_length"], batch["label"]
        desc = batch.get("desc")          # resident batch (trainer.ResidentEpochs): the stores + 2 B int32 of batch description
        cap = self.dynamic_n
        if desc is not None and not cap:
            raise capi.ErcGraftError("MMGCN: a resident batch (desc) runs in capacity mode (dynamic_n)")
        if cap:
            B, T, N = batch["caps"] if desc is not None else (qmask.shape[1], qmask.shape[0], int(ys.shape[0]))
        else:
            B, T, N = self._shape(feats[self.order[0]], lens, ys)
        self.flat.roll_health()      # a timeout of the previous step: counted, cleared -- this step runs normally
        ws = self._forward_impl(feats, qmask, lens, B, T, N, self.training, capacity=cap, desc=desc,
                                store_label=ys if desc is not None else None)
        nd = ws["counts"] if cap else None      # capacity mode: N above is the capacity, the batch's count is here
        x_row = ws["x_row"] if desc is not None else None
        if desc is not None:
            ys = ws["label"]
        fp, pl, off = self.flat, ws["planner"], self.flat.offsets
        Mo, C, TB, P = len(self.order), self.n_classes, T * B, ws["P"]
        R3, n_el = Mo * N, Mo * N * FD
        p, XD = ws["_p"], ws["_XD"]
        ks = 1.0 / (1.0 - p)
        HD, HI = ws["HD"], ws["HI"]
        gn = "graph_model.graph_net."
        if cap:
            ws["dlogits"].zero_()
            capi.cross_entropy_cap(ws["logits"], C, C, N, nd, None, ys, None, 1.0, ws["dlogits"], C, ws["stats"])
        else:
            capi.cross_entropy(ws["logits"], C, C, N, None, ys, None, 1.0, ws["dlogits"], C, ws["stats"])
        FW = Mo * 2 * FD
        capi.gemm_f32(ws["dlogits"], C, 0, None, fp.w("smax_fc.weight"), FW, 1, None, ws["dFE"], FW, N, FW, C)
        linear_wgrad(pl, ws["dlogits"], C, ws["FE"], FW, None, C, FW, N, off["smax_fc.weight"], off["smax_fc.bias"],
                     defer=True)
        DH = ws["DH"]
        if cap:
            capi.mm_regroup_bwd_cap(ws["dFE"], ws["FE"], Mo, N, nd, ks, ws["dXD"], DH)
        else:
            capi.mm_regroup_bwd(ws["dFE"], ws["FE"], Mo, N, ks, ws["dXD"], DH)
        if ws["chain"]:
            # K8 backward: one persistent launch leaves dg_l (= d out_l) and dz_l (= A dg_l) of every layer and the gradient wrt
            # the chain's input; what only meets in sums over the layers follows as batched products
            LDS = NLAYERS * FD
            plane, n_adj = R3 * FD, B * Mo * P * P
            dH0 = ws["dH0"]
            ws["dCR"].zero_()
            capi.gcnii_chain_bwd(ws["ADJ"], P, ws["CR"], ws["node_off"], N, Mo, B, T, ws["chain_cfg"], ws["V"], HD, plane, DH,
                                 ws["DH1"], ws["DGl"], ws["DZl"], LDS, ws["ZX"], ws["chain_state"], p, health=fp.health)
            if cap:      # the chain writes the batch's rows: the tail still holds those of an earlier, larger batch
                capi.mm_zero_tail(ws["DGl"], LDS, LDS, Mo, N, nd)
                capi.mm_zero_tail(ws["DZl"], LDS, LDS, Mo, N, nd)
            for l in range(1, NLAYERS + 1):
                Wn = gn + "convs.%d.weight" % (l - 1)
                th = self.theta(l)
                # dW_l[:200] = theta_l h_l^T dz_l ; dW_l[200:] = theta_l h0^T dg_l  (V_l, U_l are theta_l W + multiples of I)
                matmul_wgrad_io(pl, HD[l], FD, ws["DZl"][:, (l - 1) * FD:], LDS, FD, FD, R3, off[Wn], None, defer=True, scale=th)
                matmul_wgrad_io(pl, ws["_H0"], FD, ws["DGl"][:, (l - 1) * FD:], LDS, FD, FD, R3, off[Wn] + FD * FD, None,
                                defer=True, scale=th)
            if self.side.enabled:
                # nothing but the optimizer waits for the 128 weight gradients of the chain: second stream (ERC_SIDE_STREAM=1),
                # next to the rest of the backward, whose BiLSTM scans occupy 2 B of the 256 CUs
                with self.side.fork():
                    pl.flush_wgrads(ws, tag="_early")
            # dA = sum_l dg_l z_l^T on the block structure (and its cross-modal entries)
            if ws["gemm_x3"]:     # the planes of a row are contiguous: one K = 64 * 200 contraction per block
                capi.gemm_x3_grouped(ws["DGl"], LDS, ws["ZS"], LDS, ws["dADJs"], P, ws["node_off"], B, Mo, N, T, LDS,
                                     split_k=KSPLIT, c_slab=n_adj)
            else:
                capi.gemm_grouped(1, ws["DGl"], LDS, ws["ZS"], LDS, ws["dADJs"], P, FD, ws["node_off"], B, Mo, N, T, P, planes=NLAYERS,
                                  a_plane=FD, b_plane=FD, split=KSPLIT, c_slab=n_adj)
            capi.slab_reduce(ws["dADJs"], KSPLIT, n_adj, None, P, 0, ws["dADJ"], n_adj)
            if cap:
                capi.mm_cross_grad_cap(ws["DGl"], LDS, ws["ZS"], LDS, ws["node_dlg"], ws["node_off"], Mo, N, nd, P, ws["dCR"],
                                       planes=NLAYERS, d_plane=FD, h_plane=FD)
            else:
                capi.mm_cross_grad(ws["DGl"], LDS, ws["ZS"], LDS, ws["node_dlg"], ws["node_off"], Mo, N, P, ws["dCR"], planes=NLAYERS,
                                   d_plane=FD, h_plane=FD)
            # dh0 = sum_l dg_l U_l^T = DG U^T: one product with K = 64 * 200
            if ws["gemm_x3"]:
                capi.gemm_x3(ws["DGl"], LDS, ws["U"], LDS, ws["dH0s3"], FD, R3, FD, LDS, split_k=self.X3_SPLIT, c_slab=R3 * FD)
                capi.slab_reduce(ws["dH0s3"], self.X3_SPLIT, R3 * FD, None, FD, 0, dH0, R3 * FD)
            else:
                linear_fwd(pl, ws["DGl"], LDS, None, ws["U"], None, dH0, FD, R3, FD, LDS)
            DH = ws["DH1"]
        else:
            DH, dH0 = self._legacy_chain_backward(ws, pl, DH, B, T, N, p, ks)
        # input layer: HD[1] = dropout(H0), H0 = relu(fc0(XD))
        dG0 = ws["dG"][0]
        if cap:
            capi.axpy_mask_cap(DH, HD[1] if p > 0 else None, Mo, N, nd, FD, ks, 1, dH0)
            capi.gcnii_combine_bwd_cap(dH0, ws["_H0"], Mo, N, nd, 0.0, 0.0, 1.0, 1, dG0, None, None, FD)
        else:
            capi.axpy_mask(DH, HD[1] if p > 0 else None, n_el, ks, 1, dH0)
            capi.gcnii_combine_bwd(dH0, ws["_H0"], n_el, 0.0, 0.0, 1.0, 1, dG0, None, None)
        capi.gemm_f32(dG0, FD, 0, None, fp.w(gn + "fcs.0.weight"), FD, 1, None, ws["dXD"], FD, R3, FD, FD, accumulate=1)
        linear_wgrad(pl, dG0, FD, XD, FD, None, FD, FD, R3, off[gn + "fcs.0.weight"], off[gn + "fcs.0.bias"], defer=True)
        dX = ws["dX"]
        if cap:
            capi.axpy_mask_cap(ws["dXD"], XD if p > 0 else None, Mo, N, nd, FD, ks, 0, dX)
        else:
            capi.axpy_mask(ws["dXD"], XD if p > 0 else None, n_el, ks, 0, dX)
        # through the adjacency into the features
        capi.mm_adj_finish_bwd(ws["COS"], ws["CCOS"], ws["DEG"], ws["dADJ"], ws["dCR"], ws["node_off"], B, Mo, N, P,
                               ws["Gb"], ws["GC"], ws["DDEG"])
        capi.gemm_grouped(0, ws["Gb"], P, ws["XH"], FD, ws["dXH"], FD, FD, ws["node_off"], B, Mo, N, T, P)
        if cap:
            capi.mm_cross_apply_cap(ws["GC"], ws["XH"], FD, ws["node_dlg"], ws["node_off"], Mo, N, nd, P, ws["dXH"], FD)
            capi.mm_zero_tail(ws["dXH"], FD, FD, Mo, N, nd)
            capi.mm_row_normalize_bwd_cap(ws["XH"], ws["INV"], ws["dXH"], Mo, N, nd, dX)
        else:
            capi.mm_cross_apply(ws["GC"], ws["XH"], FD, ws["node_dlg"], ws["node_off"], Mo, N, P, ws["dXH"], FD)
            capi.mm_row_normalize_bwd(ws["XH"], ws["INV"], ws["dXH"], R3, dX)
        # per modality: back to the padded [T,B] rows, (speaker embedding, BiLSTM,) Linear
        for mi, m in enumerate(self.order):
            dm = dX[mi * N:]
            x = feats[m].reshape(-1, self.dims[m])
            if m != "t":
                linear_wgrad(pl, dm, FD, x, self.dims[m], ws["node_row"], FD, self.dims[m], N, off[_LIN[m] + ".weight"],
                             off[_LIN[m] + ".bias"])
                continue
            dpad = ws["dLIN"][m]
            if cap:
                # every padded row fetches its node's gradient, or the zero row behind dX (row N of the last modality's block,
                # which no launch writes): no whole-buffer zero_() per step, and no tail row scattered onto a valid one
                assert mi == Mo - 1
                capi.gather_rows(dm, FD, ws["pad_node"], TB, FD, dpad, FD)
            else:
                dpad.zero_()
                capi.gather_rows(dm, FD, ws["node_row"], N, FD, dpad, FD, scatter=1)
            dlin = dpad
            if m == "t":
                demb = fp.g("graph_model.speaker_embeddings.weight")
                if cap:
                    capi.mm_emb_grad_cap(dm, FD, ws["node_spk"], N, nd, self.n_speakers, demb, ws["emb_ws"])
                else:
                    capi.mm_emb_grad(dm, FD, ws["node_spk"], N, self.n_speakers, demb, ws["emb_ws"])
                self.lstm.backward(pl, dpad, FD, dx=ws["dLL"], lddx=FD)
                dlin = ws["dLL"]
            linear_wgrad(pl, dlin, FD, x, self.dims[m], x_row, FD, self.dims[m], TB, off[_LIN[m] + ".weight"],
                         off[_LIN[m] + ".bias"])
        pl.reduce_into(ws, fp.grad)
        self.side.join()
        return ws["stats"]


class MMGCNTrainer(CapacityBuckets, ResidentEvalSteps, TrainerBase):
    """train_step / to_logits of track_mm/mmgcn.py:126-157 (CE, Adam lr 3e-4 wd 3e-5)."""
    # -- capacity mode: the policy (the implementation is capacity.CapacityBuckets; the table in DESIGN.md).  Opt-in
    #    (--capacity_buckets=True; --resident implies it): the default stays the exact-shape step.  The node launches (the
    #    Linear / GCNII products over Mo * N rows, Call = h0 U at 12 800 columns) scale with N_cap: N_BUCKET 128, as elsewhere.
    CLASS_WEIGHTED = False
    TIME_MAJOR = True          # [T, B, d_m] feature blocks per modality, [T, B, S] one-hot speakers
    CLEAR_STALE = True         # the text branch's BiLSTM is unpacked: it READS the padded rows t < T_eff of every dialogue
    #                            slot, which the reference pads with zeros

    def __init__(self, params, device):
        self.params, self.device = params, torch.device(device)
        torch.manual_seed(params.seed)
        self.model = MMGCNModule(hidden_text=params.hidden_text, hidden_visual=params.hidden_visual,
                                 hidden_audio=params.hidden_audio, n_speakers=params.n_speakers,
                                 n_classes=params.n_classes, modals=params.modality, seed=params.seed).finalize(self.device)
        self._make_optim(health_gates=True, opt_in=True)      # a chain exchange timed out (on any rank) -> the update is skipped
        self._store_ext = ZeroRowStores()

    def _feature_keys(self):
        return tuple(_KEY[m] for m in self.model.order)

    def _absent_keys(self):
        return tuple(k for k in _KEY.values() if k not in self._feature_keys())

    def _capacity_ok(self, B_cap, T_cap, N_cap, batch=None):
        """no bucket with the flag off; where the one-launch chain is off (ERC_MM_CHAIN=0, T_cap > 128) or B_cap * modalities
        worst-case parts cannot be resident a launch's share at a time (erc_gcnii_chain_config); with the peer-to-peer
        exchange; or for a batch of other dtypes / ranks than the plugin's.  The exact-shape path runs then."""
        ok = self.capacity and not self._p2p() and 0 < N_cap <= B_cap * T_cap and self.model.supports_capacity(B_cap, T_cap)
        if ok and batch is not None:
            spk = batch["speaker_tensor"]
            ok = spk.dim() == 3 and spk.dtype == torch.float32 and batch["text_length"].dtype == torch.int64 and \
                all(batch[_KEY[m]].dim() == 3 and batch[_KEY[m]].dtype == torch.float32 and
                    int(batch[_KEY[m]].shape[2]) == self.model.dims[m] for m in self.model.order)
        return bool(ok)

    def _resident_ok(self, store, B_cap, T_cap, N_cap):
        return all(m in store.feats and store.feats[m].dtype == torch.float32 and
                   int(store.feats[m].shape[1]) == self.model.dims[m] for m in self.model.order) and \
            self._capacity_ok(B_cap, T_cap, N_cap)

    def _resident_inputs(self, store):
        """The Linear layers read the store's rows through the step's row maps; tail nodes and padded positions read a zero
        row, which the stores do not have, so each modality's features are kept once per store with one appended."""
        return self._store_ext(store, {m: store.feats[m] for m in self.model.order}), store.speaker

    def resident_batch(self, store, cur_desc, B_cap, T_cap, N_cap):
        """trainer.ResidentEpochs: the "batch" of a step whose dialogues stay in the HBM-resident store -- the per-modality
        stores, the flat speaker ids and labels, the 2 B_cap int32 the host rewrites per step and the capacities the launches
        are sized for.  None when the step cannot run that way (``_resident_ok``)."""
        if not self._resident_ok(store, B_cap, T_cap, N_cap):
            return None
        feats, spk = self._resident_inputs(store)
        batch = {k: None for k in _KEY.values()}
        batch.update({_KEY[m]: feats[m] for m in self.model.order})
        batch.update(speaker_tensor=spk, text_length=None, label=store.label, desc=cur_desc, caps=(B_cap, T_cap, N_cap))
        return batch
