"""conv-emotion DialogueGCN on the MI355X hot path (drop-in for track_mm/dgcnv2.py:51-219, base_model LSTM or None).

``DGCNModule`` keeps the reference's constructor signature, ``state_dict`` keys and shapes (``att_model.matchatt.*``,
``att_model.simpleatt.*`` and ``att_model.att.*`` included: constructed, never given a gradient, so they stay outside the
flat buffer and never change) and ``forward(**batch) -> (logits [N, C], features [N, 200])``.

Batches are time-major (batch_first=False): padded row t*B + b.  Chain:
unpacked 2-layer BiLSTM over all B*T padded rows (rnn.py; both directions run all T steps, so the reverse direction of a
short dialogue starts inside its padding) or Linear(D, 200) -> S = M Wscalar^T over the padded rows (GEMM) -> positional
edge attention (csrc/dgcnv2_att.hip) on the window graph (w = 10/10) -> RGCNConv(200, 100, 2 S^2, 30 bases) as the
basis-space tile kernels of DialogueGCN (csrc/dgcn_ops.hip) -> GraphConv (neighbour sum + two GEMMs) written next to the
gathered features in one [N, 300] buffer E -> Q = E W^T + b (GEMM) -> nodal matching attention (csrc/dgcnv2_att.hip) ->
ReLU(Linear(300, 100)) + dropout in the GEMM epilogue -> smax_fc + class-weighted cross entropy in one launch.  The
backward mirrors it; every weight gradient joins the step's batched weight-gradient launch (erc_wgrad_table).
"""
import torch
from torch import nn

from . import capi
from .capacity import ConvEmotionTrainer
from .engine import WorkspaceCache, FlatParams, GemmPlanner, linear_fwd, linear_wgrad, matmul_wgrad_io
from .matchhead import ConvEmotionModule, MatchAttHead, Transform
from .rnn import BiLSTM2, lstm_groups

G_DIM, H1, NB, NSCAL = 200, 100, 30, 110
EW = G_DIM + H1            # row width of E = [features | conv2 output]
DEAD = ("att_model.matchatt.", "att_model.simpleatt.", "att_model.att.")


class _SimpleAttention(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.scalar = nn.Linear(d, 1, bias=False)


class _MlpAttention(nn.Module):       # Attention(d, score_function='mlp'), parameters only
    def __init__(self, d):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(2 * d).uniform_(-1.0 / d ** 0.5, 1.0 / d ** 0.5))
        self.w_k, self.w_q, self.proj = nn.Linear(d, d), nn.Linear(d, d), nn.Linear(d, d)


class _EdgeAttention(nn.Module):
    """MaskedEdgeAttention (dgcnv2_models.py:517-531): only ``scalar`` is used (attn1)"""

    def __init__(self, d, max_seq_len):
        super().__init__()
        self.scalar = nn.Linear(d, max_seq_len, bias=False)
        self.matchatt = Transform(d)
        self.simpleatt = _SimpleAttention(d)
        self.att = _MlpAttention(d)


class _RGCNBasis(nn.Module):
    def __init__(self, cin, cout, R, nb):
        super().__init__()
        self.basis = nn.Parameter(torch.empty(nb, cin, cout))
        self.att = nn.Parameter(torch.empty(R, nb))
        self.root = nn.Parameter(torch.empty(cin, cout))
        self.bias = nn.Parameter(torch.empty(cout))
        bound = 1.0 / (nb * cin) ** 0.5                              # models/rgcn.py:317-322
        for p in (self.basis, self.att, self.root, self.bias):
            nn.init.uniform_(p, -bound, bound)


class _GraphConv(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.lin_rel = nn.Linear(cin, cout, bias=True)
        self.lin_root = nn.Linear(cin, cout, bias=False)


class _GraphNetwork(nn.Module):
    def __init__(self, d, n_classes, R, hidden, dropout):
        super().__init__()
        self.conv1 = _RGCNBasis(d, hidden, R, NB)
        self.conv2 = _GraphConv(hidden, hidden)
        self.matchatt = Transform(d + hidden)
        self.linear = nn.Linear(d + hidden, hidden)
        self.dropout = nn.Dropout(dropout)
        self.smax_fc = nn.Linear(hidden, n_classes)


class DGCNModule(ConvEmotionModule):
    def __init__(self, base_model, input_size=100, hidden_size=100, n_speakers=2, window_past=10, window_future=10, n_classes=7,
                 listener_state=False, context_attention="general", dropout_rec=0.5, dropout=0.4, nodal_attention=True, avec=False,
                 compute="f32", seed=1):
        super().__init__()
        if base_model not in ("LSTM", "None"):
            raise capi.ErcGraftError("dgcnv2: base_model=%r is not built (LSTM and None are; the serial party-state "
                                     "DialogueRNN and the GRU base are out of scope)" % (base_model,))
        if hidden_size != H1:
            raise capi.ErcGraftError("dgcnv2: the kernels are built for hidden_size 100 (dgcnv2.py:162), got %d" % hidden_size)
        if not nodal_attention or avec:
            raise capi.ErcGraftError("dgcnv2: only nodal_attention=True, avec=False (the defaults) are built")
        if compute != "f32":
            raise capi.ErcGraftError("dgcnv2 runs in fp32 only (the reference is fp32); --compute=%s is not supported" % compute)
        self.base_model, self.n_speakers, self.n_classes, self.compute = base_model, n_speakers, n_classes, compute
        self.input_size, self.wp, self.wf = input_size, window_past, window_future
        self.R = 2 * n_speakers ** 2
        self.drop_p = float(dropout)
        if base_model == "LSTM":
            self.lstm = nn.LSTM(input_size=input_size, hidden_size=hidden_size, num_layers=2, bidirectional=True, dropout=dropout)
        else:
            self.base_linear = nn.Linear(input_size, 2 * hidden_size)
        self.att_model = _EdgeAttention(2 * hidden_size, NSCAL)
        self.graph_net = _GraphNetwork(2 * hidden_size, n_classes, self.R, H1, dropout)
        self.flat, self._ws, self._seed = None, WorkspaceCache(), seed

    def live_groups(self):
        gn = self.graph_net
        if self.base_model == "LSTM":
            enc = lstm_groups("lstm.", self.lstm)
        else:
            enc = [[("base_linear.weight", self.base_linear.weight)], [("base_linear.bias", self.base_linear.bias)]]
        return enc + [
            [("att_model.scalar.weight", self.att_model.scalar.weight)],
            [("graph_net.conv1.basis", gn.conv1.basis)], [("graph_net.conv1.att", gn.conv1.att)],
            [("graph_net.conv1.root", gn.conv1.root)], [("graph_net.conv1.bias", gn.conv1.bias)],
            [("graph_net.conv2.lin_rel.weight", gn.conv2.lin_rel.weight)], [("graph_net.conv2.lin_rel.bias", gn.conv2.lin_rel.bias)],
            [("graph_net.conv2.lin_root.weight", gn.conv2.lin_root.weight)],
        ] + MatchAttHead.groups("graph_net.", gn)

    def finalize(self, device):
        self.to(device)
        self.flat = FlatParams(self.live_groups(), device)
        if self.base_model == "LSTM":
            self.enc = BiLSTM2(self.flat, "lstm.", self.input_size, drop_p=self.drop_p)
        self.head = MatchAttHead(self.flat, "graph_net.", EW, H1, self.n_classes, self.drop_p)
        self.rng_state = torch.tensor([0, self._seed], dtype=torch.int64, device=device)
        return self

    def _workspace(self, B, T, N, device):
        return self._ws.get((B, T, N), lambda: self._make_workspace(B, T, N, device))

    def _make_workspace(self, B, T, N, device):
        # zeros, not empty: a stale NaN must never reach a weight-gradient GEMM through a row the step did not touch
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)
        w = (self.wp if self.wp >= 0 else T) + (self.wf if self.wf >= 0 else T) + 1
        E = max(1, N * min(w, T))
        BT, n_sl = B * T, capi.brgcn_fwd_tile_slabs()
        g = dict(node_off=i32(B + 1), node_row=i32(N), node_spk=i32(N), in_ptr=i32(N + 1), in_src=i32(E),
                 in_typ=i32(E), out_ptr=i32(N + 1), out_dst=i32(E), out_typ=i32(E), out_eid=i32(E), counts=i32(2))
        ws = dict(g=g, E_cap=E, spk=torch.zeros(BT, dtype=torch.int64, device=device), node_row=i32(N),
                  M=f32(BT, G_DIM), S=f32(BT, NSCAL), norm=f32(E), Z=f32(N, NB * G_DIM), rgcn_slabs=f32(capi.brgcn_fwd_tile_slab_floats(N)),
                  Hc=f32(N, H1), AGG=f32(N, H1), E=f32(N, EW),
                  dAGG=f32(N, H1), dHc=f32(N, H1), TT=f32(E, NB), dn_slabs=f32(n_sl * E), rgcn_dslabs=f32(n_sl * N * G_DIM),
                  dS=f32(BT, NSCAL), dM=f32(BT, G_DIM), **self.head.buffers(B, T, N, device))
        D = self.input_size
        slab = 12 * N * H1 + 4 * BT * 800 + 10 * (800 * D + 800 * 200 + 2 * 400 * 100 * 2) + 4 * NB * G_DIM * H1 + \
            8 * (EW * EW + EW * H1 + NSCAL * G_DIM) + 4 * N * EW + (1 << 21)
        ws["planner"] = GemmPlanner(device, slab, grad=self.flat.grad)
        ws["jobs"] = None
        return ws

    def _check(self, T):
        if T > NSCAL:
            raise capi.ErcGraftError("dgcnv2: MaskedEdgeAttention.scalar has %d rows, so dialogues of up to %d utterances are "
                                     "supported (batch T=%d)" % (NSCAL, NSCAL, T))

    def _forward_impl(self, x, onehot, lens, B, T, N, training, with_logits=True):
        self._check(T)
        fp = self.flat
        ws = self._workspace(B, T, N, x.device)
        g, pl = ws["g"], ws["planner"]
        pl.reset()
        D, BT = self.input_size, B * T
        x, onehot = x.contiguous(), onehot.contiguous()
        capi.dgcnv2_meta(onehot, int(onehot.shape[-1]), lens, B, T, N, ws["spk"], ws["node_row"])
        capi.window_graph_build(lens, ws["spk"], 1, B, B, T, self.wp, self.wf, self.n_speakers, N, ws["E_cap"], g)
        M = ws["M"]
        if self.base_model == "LSTM":
            # unpacked: lengths=None runs every dialogue over all T padded steps, row t*B + b (sb = 1, st = B)
            self.enc.forward(pl, x, D, BT, B, T, 1, B, None, training, self.rng_state, M, G_DIM, store=ws)
        else:
            linear_fwd(pl, x, D, None, fp.w("base_linear.weight"), fp.w("base_linear.bias"), M, G_DIM, BT, G_DIM, D)
        E = ws["E"]
        capi.gather_rows(M, G_DIM, ws["node_row"], N, G_DIM, E, EW)
        # positional edge attention: scores of every padded row, softmax per source over its window (+ the 1e-10 leak)
        capi.gemm_f32(M, G_DIM, 0, None, fp.w("att_model.scalar.weight"), G_DIM, 0, None, ws["S"], NSCAL, BT, NSCAL, G_DIM)
        capi.dgcnv2_edge_att_fwd(ws["S"], NSCAL, g, B, T, self.wp, self.wf, ws["norm"])
        # RGCNConv(basis): aggregate + basis product + root product in one tile launch, then the slab sum + bias
        n_sl = capi.brgcn_fwd_tile_slabs()
        capi.brgcn_fwd_tile(E, EW, G_DIM, H1, N, g, ws["norm"], fp.w("graph_net.conv1.att"), NB, fp.w("graph_net.conv1.basis"),
                            fp.w("graph_net.conv1.root"), ws["Z"], ws["rgcn_slabs"])
        capi.slab_reduce(ws["rgcn_slabs"], n_sl, N * H1, fp.w("graph_net.conv1.bias"), H1, 0, ws["Hc"], N * H1)
        # GraphConv: lin_rel(sum_{j->i} h_j) + lin_root(h_i), written next to the features
        capi.csr_sum(ws["Hc"], H1, H1, N, g["in_ptr"], g["in_src"], ws["AGG"], H1)
        gout = E[:, G_DIM:]
        capi.gemm_f32(ws["AGG"], H1, 0, None, fp.w("graph_net.conv2.lin_rel.weight"), H1, 0, None, gout, EW, N, H1, H1,
                      bias=fp.w("graph_net.conv2.lin_rel.bias"))
        capi.gemm_f32(ws["Hc"], H1, 0, None, fp.w("graph_net.conv2.lin_root.weight"), H1, 0, None, gout, EW, N, H1, H1,
                      accumulate=1)
        # nodal attention over E, then the classifier
        self.head.forward(pl, ws, E, g["node_off"], B, T, N, training, self.rng_state, with_logits)
        ws["x"] = x
        return ws

    def forward(self, input_tensor, speaker_tensor, attention_mask=None, text_length=None, label=None, **kwargs):
        if self.flat is None:
            raise capi.ErcGraftError("call DGCNModule.finalize(device) before forward")
        B, T, N = self._shape(input_tensor, text_length, label, kwargs.get("n_nodes"))
        ws = self._forward_impl(input_tensor, speaker_tensor, text_length, B, T, N, self.training)
        return ws["logits"], ws["E"][:, :G_DIM]

    def loss_and_grads(self, batch, class_weight=None):
        """F.cross_entropy(logits, label, weight) (dgcnv2.py:206) and every live gradient into flat.grad"""
        x, onehot, lens, ys = batch["input_tensor"], batch["speaker_tensor"], batch["text_length"], batch["label"]
        B, T, N = self._shape(x, lens, ys)
        ws = self._forward_impl(x, onehot, lens, B, T, N, self.training, with_logits=self.n_classes > 8)
        fp, g, pl, off = self.flat, ws["g"], ws["planner"], self.flat.offsets
        BT = B * T
        E, dE = ws["E"], ws["dE"]
        self.head.backward(pl, ws, E, g["node_off"], B, T, N, ys, class_weight, self.training)
        # GraphConv
        dG = dE[:, G_DIM:]
        capi.gemm_f32(dG, EW, 0, None, fp.w("graph_net.conv2.lin_rel.weight"), H1, 1, None, ws["dAGG"], H1, N, H1, H1)
        linear_wgrad(pl, dG, EW, ws["AGG"], H1, None, H1, H1, N, off["graph_net.conv2.lin_rel.weight"],
                     off["graph_net.conv2.lin_rel.bias"], defer=True)
        linear_wgrad(pl, dG, EW, ws["Hc"], H1, None, H1, H1, N, off["graph_net.conv2.lin_root.weight"], None, defer=True)
        capi.gemm_f32(dG, EW, 0, None, fp.w("graph_net.conv2.lin_root.weight"), H1, 1, None, ws["dHc"], H1, N, H1, H1)
        capi.csr_sum(ws["dAGG"], H1, H1, N, g["out_ptr"], g["out_dst"], ws["dHc"], H1, accumulate=1)
        # RGCNConv(basis): d norm as partial vectors per basis group, d att from the per-edge basis sums
        n_sl, E_cap = capi.brgcn_fwd_tile_slabs(), ws["E_cap"]
        capi.brgcn_bwd_edges_tile(E, EW, G_DIM, H1, N, self.R, g, ws["norm"], fp.w("graph_net.conv1.att"), NB,
                                  fp.w("graph_net.conv1.basis"), ws["dHc"], H1, ws["TT"], ws["dn_slabs"], E_cap,
                                  fp.g("graph_net.conv1.att"))
        matmul_wgrad_io(pl, ws["Z"], NB * G_DIM, ws["dHc"], H1, NB * G_DIM, H1, N, off["graph_net.conv1.basis"],
                        off["graph_net.conv1.bias"], defer=True)
        matmul_wgrad_io(pl, E, EW, ws["dHc"], H1, G_DIM, H1, N, off["graph_net.conv1.root"], None, defer=True)
        capi.brgcn_bwd_source_tile(ws["dHc"], H1, G_DIM, H1, N, g, ws["norm"], fp.w("graph_net.conv1.att"), NB,
                                   fp.w("graph_net.conv1.basis"), fp.w("graph_net.conv1.root"), ws["rgcn_dslabs"])
        capi.slab_reduce(ws["rgcn_dslabs"], n_sl, N * G_DIM, None, G_DIM, 4, dE, N * G_DIM, ld_out=EW)
        # positional edge attention: dS [B*T, 110], then dWscalar = dS^T M and dM = scatter(dE features) + dS Wscalar
        capi.dgcnv2_edge_att_bwd(ws["S"], NSCAL, g, B, T, self.wp, self.wf, ws["dn_slabs"], ws["dS"], dn_parts=n_sl,
                                 dn_stride=E_cap)
        M, dM = ws["M"], ws["dM"]
        linear_wgrad(pl, ws["dS"], NSCAL, M, G_DIM, None, NSCAL, G_DIM, BT, off["att_model.scalar.weight"], None, defer=True)
        dM.zero_()
        capi.gather_rows(dE, EW, ws["node_row"], N, G_DIM, dM, G_DIM, scatter=1)
        capi.gemm_f32(ws["dS"], NSCAL, 0, None, fp.w("att_model.scalar.weight"), G_DIM, 1, None, dM, G_DIM, BT, G_DIM, NSCAL,
                      accumulate=1)
        if self.base_model == "LSTM":
            self.enc.backward(pl, dM, G_DIM)
        else:
            linear_wgrad(pl, dM, G_DIM, ws["x"], self.input_size, None, G_DIM, self.input_size, BT, off["base_linear.weight"],
                         off["base_linear.bias"], defer=True)
        pl.reduce_into(ws, fp.grad)
        return ws["stats"]


class DGCNv2Trainer(ConvEmotionTrainer):
    """train_step / to_logits of track_mm/dgcnv2.py:184-219 (class-weighted CE, Adam lr 3e-4, no weight decay)."""
    NAME = "dgcnv2"

    def _build_model(self, params, compute):
        base = params.get("base_model", "LSTM")
        base = "None" if base is None else base          # --base_model=None parses as the Python literal
        return DGCNModule(base_model=base, input_size=params.hidden_all, hidden_size=100, n_speakers=params.n_speakers,
                          n_classes=params.n_classes, context_attention="general", compute=compute, seed=params.seed)
