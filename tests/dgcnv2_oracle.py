"""CPU restatement of the conv-emotion DialogueGCN (track_mm/dgcnv2.py:51-181, dgcnv2_models.py:109-148,517-566,612-771),
written from the math rather than from the reference's loops.  Parameters come as a dict keyed by the reference's
state_dict names.  ``masks`` (training mode) gives the applied dropout masks, already scaled by 1 / (1 - p):
``lstm`` [T, B, 200] between the two LSTM layers and ``clf`` [N, 100] after the classifier's ReLU."""
import torch
import torch.nn.functional as F

MAX_T = 110
DEAD = ("att_model.matchatt.", "att_model.simpleatt.", "att_model.att.")


def lstm_layer(P, k, x):
    """one unpacked bidirectional LSTM layer over the padded [T, B, d] input (both directions run all T steps)"""
    outs = []
    for sfx, rev in (("", False), ("_reverse", True)):
        W_ih, W_hh = P["lstm.weight_ih_l%d%s" % (k, sfx)], P["lstm.weight_hh_l%d%s" % (k, sfx)]
        b = P["lstm.bias_ih_l%d%s" % (k, sfx)] + P["lstm.bias_hh_l%d%s" % (k, sfx)]
        T, B = x.shape[0], x.shape[1]
        h = x.new_zeros(B, 100)
        c = x.new_zeros(B, 100)
        gx = x @ W_ih.t() + b
        hs = [None] * T
        for t in (range(T - 1, -1, -1) if rev else range(T)):
            i, f, g, o = (gx[t] + h @ W_hh.t()).chunk(4, -1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            hs[t] = h
        outs.append(torch.stack(hs))
    return torch.cat(outs, -1)


def window_edges(L, wp=10, wf=10):
    """(src, dst) of one dialogue: src j -> dst i for i in [j - wp, j + wf] (edge_perms, dgcnv2_models.py:584-609)"""
    out = []
    for j in range(L):
        for i in range(max(0, j - wp), min(L, j + wf + 1)):
            out.append((j, i))
    return out


def relation(sj, si, j, i, S):
    """edge_type_mapping[str(s_src) + str(s_dst) + ('0' if src < dst else '1')] (dgcnv2.py:111-116, models:668-677)"""
    return 2 * (sj * S + si) + (0 if j < i else 1)


def forward(P, batch, base="LSTM", masks=None, wp=10, wf=10):
    """-> (logits [N, C], features [N, 200]) in dialogue-major node order"""
    x, onehot, lens = batch["input_tensor"], batch["speaker_tensor"], [int(v) for v in batch["text_length"]]
    T, B = x.shape[0], x.shape[1]
    S = onehot.shape[-1]
    if base == "LSTM":
        h0 = lstm_layer(P, 0, x)
        if masks is not None:
            h0 = h0 * masks["lstm"]
        M = lstm_layer(P, 1, h0)
    else:
        M = x @ P["base_linear.weight"].t() + P["base_linear.bias"]
    spk = onehot.argmax(-1)                              # first index of the maximum: the 1 of a one-hot row
    # positional edge attention: row j of Wscalar scores every position of the dialogue (padded ones included)
    scale = torch.einsum("tbd,kd->btk", M, P["att_model.scalar.weight"])           # [B, T, 110]
    feats, src, dst, typ, norm, off = [], [], [], [], [], 0
    for b, L in enumerate(lens):
        feats.append(M[:L, b])
        ex = torch.exp(scale[b] - scale[b].max(0, keepdim=True).values)            # [T(i), 110(j)]
        for j in range(L):
            lo, hi = max(0, j - wp), min(L, j + wf + 1)
            col = ex[:, j]
            den = col[lo:hi].sum() + 1e-10 * (col[:lo].sum() + col[hi:].sum())
            for i in range(lo, hi):
                src.append(off + j)
                dst.append(off + i)
                typ.append(relation(int(spk[j, b]), int(spk[i, b]), j, i, S))
                norm.append(col[i] / den)
        off += L
    X = torch.cat(feats)
    src, dst, typ = torch.tensor(src), torch.tensor(dst), torch.tensor(typ)
    norm = torch.stack(norm)
    # RGCNConv(200, 100, R, num_bases=30) with edge_norm (models/rgcn.py:300-355)
    nb, cin, cout = P["graph_net.conv1.basis"].shape
    W = (P["graph_net.conv1.att"] @ P["graph_net.conv1.basis"].reshape(nb, -1)).view(-1, cin, cout)
    msg = torch.bmm(X[src].unsqueeze(1), W[typ]).squeeze(1) * norm[:, None]
    H = torch.zeros(X.shape[0], cout).index_add(0, dst, msg) + X @ P["graph_net.conv1.root"] + P["graph_net.conv1.bias"]
    # GraphConv(100, 100): lin_rel(sum_{j -> i} h_j) + lin_root(h_i)
    agg = torch.zeros_like(H).index_add(0, dst, H[src])
    G = agg @ P["graph_net.conv2.lin_rel.weight"].t() + P["graph_net.conv2.lin_rel.bias"] + H @ P["graph_net.conv2.lin_root.weight"].t()
    E = torch.cat([X, G], -1)
    # nodal attention, MatchingAttention 'general2' per dialogue over its valid rows
    Q = E @ P["graph_net.matchatt.transform.weight"].t() + P["graph_net.matchatt.transform.bias"]
    A, off = [], 0
    for L in lens:
        e, q = E[off:off + L], Q[off:off + L]
        A.append(torch.softmax(torch.tanh(q @ e.t()), -1) @ e)
        off += L
    A = torch.cat(A)
    Z = F.relu(A @ P["graph_net.linear.weight"].t() + P["graph_net.linear.bias"])
    if masks is not None:
        Z = Z * masks["clf"]
    return Z @ P["graph_net.smax_fc.weight"].t() + P["graph_net.smax_fc.bias"], X


def loss_and_grads(P, batch, base="LSTM", class_weight=None, masks=None):
    """weighted CE (dgcnv2.py:206) and the gradient of every parameter; the dead ones (DEAD prefixes) get None"""
    Pg = {k: (v.detach().clone().requires_grad_(not k.startswith(DEAD))) for k, v in P.items()}
    logits, feats = forward(Pg, batch, base, masks)
    loss = F.cross_entropy(logits, batch["label"], weight=class_weight)
    loss.backward()
    return loss.detach(), logits.detach(), feats.detach(), {k: v.grad for k, v in Pg.items()}


def adam_step(P, grads, lr=3e-4, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam's first step (weight decay 0): parameters without a gradient stay as they are"""
    out = {}
    for k, v in P.items():
        g = grads.get(k)
        if g is None:
            out[k] = v.clone()
            continue
        m = (1 - betas[0]) * g
        s = (1 - betas[1]) * g * g
        out[k] = v - lr * (m / (1 - betas[0])) / ((s / (1 - betas[1])).sqrt() + eps)
    return out
