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

Capacity mode (``--capacity_buckets=True``, ``--resident``, ``--resident_eval``; off by default): the same chain with every
launch sized for a bucket (B_cap, T_cap, N_cap) and the batch's node count and longest dialogue read from the device --
``_forward_cap``, ``eval_scores``, ``DGCNv2Trainer``'s policy; DESIGN.md section 8c.
"""
import torch
from torch import nn

from . import capi
from .capacity import CapacityBuckets, ConvEmotionTrainer, ResidentEvalSteps, ZeroRowStores
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
        # CAPACITY MODE (trainer.StepGraphs buckets, trainer.ResidentEpochs): the batch tensors are capacity-sized static
        # buffers -- B dialogue slots of which some may have length 0, T the longest dialogue of the split, label [N_cap] -- and
        # every launch is sized for the capacities.  erc_bcrnn_meta_cap writes the batch's node count and its longest dialogue
        # to the device (ws["counts"]): the LSTM scans and the edge attention run over that many steps, the loss covers that
        # many rows, and the kernels that own a gradient buffer zero its rows past them, so ONE captured HIP graph serves
        # every batch that fits.
        self.dynamic_n = False
        self.flat, self._ws, self._seed = None, WorkspaceCache(), seed
        self._eval_ws = WorkspaceCache()      # eval_scores' own buffers: never those of a (captured) training step

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

    def _workspace(self, B, T, N, device, cap=False):
        if cap:
            return self._ws.get((B, T, N, "capacity"), lambda: self._make_workspace(B, T, N, device, cap=True))
        return self._ws.get((B, T, N), lambda: self._make_workspace(B, T, N, device))

    def _make_workspace(self, B, T, N, device, cap=False, grads=True):
        """``cap``: capacity mode -- the tables of erc_bcrnn_meta_cap, one zero row behind M and behind dE (what node_row of the
        capacity nodes and pad_node of the padded positions point at; nothing writes them), dQ | dE as one buffer (MatchAttHead
        ``tail_pair``).  ``grads=False`` (eval_scores): no gradient buffer."""
        # zeros, not empty: a stale NaN must never reach a weight-gradient GEMM through a row the step did not touch
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)
        w = (self.wp if self.wp >= 0 else T) + (self.wf if self.wf >= 0 else T) + 1
        E = max(1, N * min(w, T))
        BT, n_sl = B * T, capi.brgcn_fwd_tile_slabs()
        zrow = 1 if cap else 0
        g = dict(node_off=i32(B + 1), node_row=i32(N), node_spk=i32(N), in_ptr=i32(N + 1), in_src=i32(E),
                 in_typ=i32(E), out_ptr=i32(N + 1), out_dst=i32(E), out_typ=i32(E), out_eid=i32(E), counts=i32(2))
        ws = dict(g=g, E_cap=E, spk=torch.zeros(BT, dtype=torch.int64, device=device), node_row=i32(N),
                  M=f32(BT + zrow, G_DIM), S=f32(BT, NSCAL), norm=f32(E), Z=f32(N, NB * G_DIM), rgcn_slabs=f32(capi.brgcn_fwd_tile_slab_floats(N)),
                  Hc=f32(N, H1), AGG=f32(N, H1), E=f32(N, EW))
        if cap:
            ws.update(node_off=i32(B + 1), pad_node=i32(BT), x_row=i32(BT), counts=i32(2),
                      label=torch.zeros(N, dtype=torch.int64, device=device))
        if grads:
            ws.update(dAGG=f32(N, H1), dHc=f32(N, H1), TT=f32(E, NB), dn_slabs=f32(n_sl * E), rgcn_dslabs=f32(n_sl * N * G_DIM),
                      dS=f32(BT, NSCAL), dM=f32(BT, G_DIM), **self.head.buffers(B, T, N, device, dE_rows=N + zrow, tail_pair=cap))
        else:
            hb = self.head.buffers(B, T, N, device)
            ws.update({k: hb[k] for k in ("Q", "A", "P", "TH", "Zc", "logits")})
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
        self._graph_and_head(ws, B, T, N, training, with_logits)
        ws["x"] = x
        return ws

    def _graph_and_head(self, ws, B, T, N, training, with_logits, t_dev=None):
        """from the encoder's output ws["M"] (padded rows) to ws["Zc"] / ws["logits"]: the chain both forms of the forward
        share.  ``t_dev``: capacity mode, the edge attention reads the batch's longest dialogue from the device."""
        fp, g, pl, M, E, BT = self.flat, ws["g"], ws["planner"], ws["M"], ws["E"], B * T
        capi.gather_rows(M, G_DIM, ws["node_row"], N, G_DIM, E, EW)
        # positional edge attention: scores of every padded row, softmax per source over its window (+ the 1e-10 leak)
        capi.gemm_f32(M, G_DIM, 0, None, fp.w("att_model.scalar.weight"), G_DIM, 0, None, ws["S"], NSCAL, BT, NSCAL, G_DIM)
        capi.dgcnv2_edge_att_fwd(ws["S"], NSCAL, g, B, T, self.wp, self.wf, ws["norm"], t_dev=t_dev)
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

    def _forward_cap(self, x, onehot, lens, B, T, N, training, desc=None, store_label=None, ws=None, with_logits=False):
        """The forward in CAPACITY mode: B, T, N are capacities, the batch's own node count and longest dialogue are on the
        device (ws["counts"] = [n_dev, t_dev]).  ``desc`` (int32 [2 B]: lengths | first store rows): RESIDENT batch -- x is the
        feature store [U + 1, D] whose last row is zero, read through ws["x_row"], ``onehot`` the store's speaker ids [U]
        (int64), labels are gathered into ws["label"].  ``ws``: the caller's own workspace (eval_scores).

        Rows past the batch, buffer by buffer (every weight-gradient product runs over all capacity rows and must meet a
        zero gradient row wherever the other operand is stale):
          M     rows t >= *t_dev: 0 (LSTM: erc_lstm_scan_fwd_tcap writes them) or the bias (base None); the edge attention
                reads S = M Wscalar^T only at t < T_eff, and dS is +0 there (erc_dgcnv2_edge_att_bwd_cap), so dWscalar =
                dS^T M meets zero rows.  Slots of length 0 hold the LSTM's response to zero input (or the bias): all 110
                columns of their dS rows are +0 (same kernel) and pad_node points them at the zero row of dE, so dM and with
                it every gate gradient (or the row of base_linear's gradient product) of theirs is exactly 0.
          E     capacity rows i >= n_dev: features 0 (node_row -> the zero row behind M); the conv2 columns hold
                lin_rel.bias + Hc W_root (finite).  E enters dW_transform = dQ^T E and d root = E^T dHc: dQ rows are +0
                (erc_mm_zero_tail), dHc rows are 0 (below).
          Z, Hc capacity rows hold what the tile launch / erc_slab_reduce write for a node without in-edges (0, the bias):
                they meet dHc = dG W_root + the out-edge sum of dAGG, where dG (the conv2 columns of dE) is +0 on those
                rows (erc_mm_zero_tail; dE += dQ W adds 0) and the capacity rows' CSR ranges are empty.
          AGG   0 on capacity rows (erc_csr_sum over an empty range); meets dG, 0 there.
          Q, A, Zc  capacity rows: Q = transform(E) is finite, A / Zc are whatever an earlier batch left (finite; the
                matching attention walks the dialogues through node_off).  They meet dQ (erc_mm_zero_tail), dZc and
                dlogits (erc_head_ce_cap writes both 0 past n_dev) and dA = dZc W (0).
          dM    every padded row fetches its node's feature gradient or the zero row behind dE (pad_node), plus dS Wscalar:
                written whole, no zero_() and no scatter."""
        if T > NSCAL:
            raise capi.ErcGraftError("dgcnv2: MaskedEdgeAttention.scalar has %d rows, so dialogues of up to %d utterances are "
                                     "supported (T_cap=%d)" % (NSCAL, NSCAL, T))
        if x.dtype != torch.float32 or int(x.shape[-1]) != self.input_size:
            raise capi.ErcGraftError("dgcnv2: capacity mode needs fp32 features of width %d" % self.input_size)
        if desc is None and (lens.dtype != torch.int64 or onehot.dtype != torch.float32 or onehot.dim() != 3):
            raise capi.ErcGraftError("dgcnv2: capacity mode needs int64 text_length and fp32 one-hot speakers [T, B, S]")
        if desc is not None and onehot.dtype != torch.int64:
            raise capi.ErcGraftError("dgcnv2: a resident batch carries the store's int64 speaker ids")
        fp = self.flat
        if ws is None:
            ws = self._workspace(B, T, N, x.device, cap=True)
        g, pl = ws["g"], ws["planner"]
        pl.reset()
        D, BT = self.input_size, B * T
        x = x.contiguous()
        if desc is not None:
            capi.bcrnn_meta_cap(None, desc, store_label, int(x.shape[0]) - 1, B, T, N, ws["node_off"], ws["node_row"], ws["pad_node"],
                                ws["x_row"], ws["label"], ws["counts"])
            capi.window_graph_build(None, onehot, 0, 1, B, T, self.wp, self.wf, self.n_speakers, N, ws["E_cap"], g, desc=desc)
        else:
            onehot = onehot.contiguous()
            # the padded speaker ids; its node_row (valid nodes only) is rewritten whole by the next launch
            capi.dgcnv2_meta(onehot, int(onehot.shape[-1]), lens, B, T, N, ws["spk"], ws["node_row"])
            capi.bcrnn_meta_cap(lens, None, None, 0, B, T, N, ws["node_off"], ws["node_row"], ws["pad_node"], None, None,
                                ws["counts"])
            capi.window_graph_build(lens, ws["spk"], 1, B, B, T, self.wp, self.wf, self.n_speakers, N, ws["E_cap"], g)
        t_dev, x_row = ws["counts"][1:], ws["x_row"] if desc is not None else None
        M = ws["M"]
        if self.base_model == "LSTM":
            self.enc.forward(pl, x, D, BT, B, T, 1, B, None, training, self.rng_state, M, G_DIM, store=ws, node_row=x_row,
                             t_dev=t_dev)
        else:
            linear_fwd(pl, x, D, x_row, fp.w("base_linear.weight"), fp.w("base_linear.bias"), M, G_DIM, BT, G_DIM, D)
        self._graph_and_head(ws, B, T, N, training, with_logits, t_dev=t_dev)
        ws["x"], ws["x_gather"] = x, x_row
        return ws

    def eval_scores(self, batch, cm):
        """Forward-only step in capacity form, scored on the device: the capacity forward in eval mode (no dropout: the counter
        is not read) on a workspace of its own, smax_fc, and erc_rows_score, which reads the batch's node count from the device
        and ADDS its confusion matrix to ``cm`` (int64 [C, C], true x predicted).  No host synchronisation, capturable.
        ``batch``: a resident batch (``desc`` + ``caps``, as loss_and_grads takes) or a capacity-sized static one.  Returns the
        step's own workspace (``logits`` [N_cap, C]: rows below the device count are valid).  Reads neither ``training`` nor
        ``dynamic_n`` and touches no training state."""
        if self.flat is None:
            raise capi.ErcGraftError("call DGCNModule.finalize(device) before eval_scores")
        C = self.n_classes
        if C > capi.rows_score_max_classes():
            raise capi.ErcGraftError("dgcnv2 eval_scores: at most %d classes (erc_rows_score)" % capi.rows_score_max_classes())
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
            raise capi.ErcGraftError("call DGCNModule.finalize(device) before forward")
        if self.dynamic_n:
            raise capi.ErcGraftError("dgcnv2: capacity mode (dynamic_n) is the training step's (loss_and_grads) and eval_scores'")
        B, T, N = self._shape(input_tensor, text_length, label, kwargs.get("n_nodes"))
        ws = self._forward_impl(input_tensor, speaker_tensor, text_length, B, T, N, self.training)
        return ws["logits"], ws["E"][:, :G_DIM]

    def loss_and_grads(self, batch, class_weight=None):
        """F.cross_entropy(logits, label, weight) (dgcnv2.py:206) and every live gradient into flat.grad"""
        x, onehot, lens, ys = batch["input_tensor"], batch["speaker_tensor"], batch["text_length"], batch["label"]
        desc = batch.get("desc")          # resident batch (trainer.ResidentEpochs): the store + 2 B int32 of batch description
        cap = self.dynamic_n or desc is not None
        if cap:
            if not (self.dynamic_n and self.n_classes <= 8):
                raise capi.ErcGraftError("dgcnv2: capacity mode needs dynamic_n and at most 8 classes (erc_head_ce_cap)")
            B, T, N = batch["caps"] if desc is not None else self._shape(x, lens, ys)
            ws = self._forward_cap(x, onehot, lens, B, T, N, self.training, desc=desc, store_label=ys if desc is not None else None)
            if desc is not None:
                ys = ws["label"]
        else:
            B, T, N = self._shape(x, lens, ys)
            ws = self._forward_impl(x, onehot, lens, B, T, N, self.training, with_logits=self.n_classes > 8)
        nd, t_dev = (ws["counts"], ws["counts"][1:]) if cap else (None, None)
        fp, g, pl, off = self.flat, ws["g"], ws["planner"], self.flat.offsets
        BT = B * T
        E, dE = ws["E"], ws["dE"]
        self.head.backward(pl, ws, E, g["node_off"], B, T, N, ys, class_weight, self.training, n_dev=nd, n_cap=N if cap else 0)
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
                                 dn_stride=E_cap, t_dev=t_dev)
        M, dM = ws["M"], ws["dM"]
        linear_wgrad(pl, ws["dS"], NSCAL, M, G_DIM, None, NSCAL, G_DIM, BT, off["att_model.scalar.weight"], None, defer=True)
        if cap:
            # every padded row fetches its node's gradient, or the zero row behind dE: no whole-buffer zero_() per step
            capi.gather_rows(dE, EW, ws["pad_node"], BT, G_DIM, dM, G_DIM)
        else:
            dM.zero_()
            capi.gather_rows(dE, EW, ws["node_row"], N, G_DIM, dM, G_DIM, scatter=1)
        capi.gemm_f32(ws["dS"], NSCAL, 0, None, fp.w("att_model.scalar.weight"), G_DIM, 1, None, dM, G_DIM, BT, G_DIM, NSCAL,
                      accumulate=1)
        if self.base_model == "LSTM":
            self.enc.backward(pl, dM, G_DIM)
        else:
            linear_wgrad(pl, dM, G_DIM, ws["x"], self.input_size, ws["x_gather"] if cap else None, G_DIM, self.input_size, BT,
                         off["base_linear.weight"], off["base_linear.bias"], defer=True)
        pl.reduce_into(ws, fp.grad)
        return ws["stats"]


class DGCNv2Trainer(CapacityBuckets, ResidentEvalSteps, ConvEmotionTrainer):
    """train_step / to_logits of track_mm/dgcnv2.py:184-219 (class-weighted CE, Adam lr 3e-4, no weight decay)."""
    NAME = "dgcnv2"

    def __init__(self, params, device):
        # capacity buckets are opt-in: the default stays the exact-shape step, whose dropout masks (keyed by the padded element
        # index, so by B and T) a capacity-sized step does not reproduce
        super().__init__(params, device, opt_in=True)
        self._store_ext = ZeroRowStores()

    def _build_model(self, params, compute):
        base = params.get("base_model", "LSTM")
        base = "None" if base is None else base          # --base_model=None parses as the Python literal
        return DGCNModule(base_model=base, input_size=params.hidden_all, hidden_size=100, n_speakers=params.n_speakers,
                          n_classes=params.n_classes, context_attention="general", dropout=params.get("dropout", 0.4), compute=compute,
                          seed=params.seed)

    # -- capacity mode: the policy (the implementation is capacity.CapacityBuckets).  N_BUCKET 128 and "a batch of exactly its
    #    bucket's shape stays exact" are the mixin's defaults, and so is the precapture list, built from train.batch_size
    #    and T_cap alone; ``opt_in=True`` (above) makes the buckets opt-in
    TIME_MAJOR = True          # [T, B, D] features, [T, B, S] one-hot speakers
    CLEAR_STALE = True         # both bases READ the padded rows t < T_eff of every dialogue slot (the unpacked LSTM; the edge
    #                            attention softmaxes over them), so they must be zero, not stale

    def _capacity_ok(self, B_cap, T_cap, N_cap, batch=None):
        """no bucket with the flag off, with the peer-to-peer exchange, above the edge attention's T or the head's classes, or
        for a batch of other dtypes / widths / ranks (the gate is on T_cap: the node launches take any N_cap)"""
        ok = self.capacity and not self._p2p() and 0 < T_cap <= NSCAL and self.model.n_classes <= 8
        if ok and batch is not None:
            x, spk = batch["input_tensor"], batch["speaker_tensor"]
            ok = (x.dtype == torch.float32 and x.dim() == 3 and int(x.shape[2]) == self.model.input_size and spk.dim() == 3 and
                  spk.dtype == torch.float32 and batch["text_length"].dtype == torch.int64)
        return bool(ok)

    def _resident_ok(self, store, B_cap, T_cap, N_cap):
        return (store.fused.dtype == torch.float32 and int(store.fused.shape[1]) == self.model.input_size and
                store.speaker.dtype == torch.int64 and self._capacity_ok(B_cap, T_cap, N_cap))

    def _resident_inputs(self, store):
        """The encoder's input product reads the store's rows through the step's row map; padded positions read a zero row,
        which the store does not have, so the features are kept once per store with one appended.  The speakers are the
        store's ids: erc_window_graph_build_desc reads them at the nodes' store rows."""
        return self._store_ext(store, store.fused), store.speaker
