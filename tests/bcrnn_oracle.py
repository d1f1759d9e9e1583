"""CPU restatement of conv-emotion's bc-LSTM / bc-GRU baselines (track_mm/dgcnv2_models.py:389-425 LSTMModel, :350-386
GRUModel, att2=True), written from the math in plain torch: a 2-layer bidirectional RNN run UNPACKED over all T padded
steps of the time-major batch (the reverse direction of a short dialogue starts inside its zero padding), then on the valid
rows the 'general2' matching attention (with mask=umask the reference's masked renormalisation :127-138 is a softmax over
the valid keys), ReLU(Linear) and log-softmax.  Parameters come as a dict keyed by the reference's state_dict names
(``lstm.*`` / ``gru.*``, nn.LSTM / nn.GRU layout).  ``masks`` (training mode) gives the applied dropout masks, already scaled
by 1 / (1 - p): ``rnn`` [T*B, 200] on the layer-0 output (padded rows, row t*B + b) and ``clf`` [N, D_h] after the
classifier's ReLU.  ``gru_scan`` is also the float64 chain of the scan kernel's test."""
import torch
import torch.nn.functional as F

MAX_T = 110


def gru_scan(gx, W_hh, b_hh, eps=None, ops=torch):
    """dialogues in scan order: gx [L, 300] or [L, n, 300] (n dialogues of the same length) = x W_ih^T + b_ih -> h [L, (n,) 100];
    torch.nn.GRU, gate order r|z|n, h0 = 0.  ``eps`` (zeros, shaped as gx) is added to the recurrent pre-activations
    W_hh h + b_hh: its gradient is what the backward kernel calls dGH.  ``ops`` supplies matmul, sigmoid and tanh
    (tests/rnn_scan_ref.py passes ones whose float32 results do not depend on the machine's math libraries)."""
    h, out = gx.new_zeros(gx.shape[1:-1] + (W_hh.shape[1],)), []
    for s in range(gx.shape[0]):
        gh = ops.matmul(h, W_hh.t()) + b_hh
        if eps is not None:
            gh = gh + eps[s]
        ir, iz, inn = gx[s].chunk(3, -1)
        hr, hz, hn = gh.chunk(3, -1)
        r, z = ops.sigmoid(ir + hr), ops.sigmoid(iz + hz)
        n = ops.tanh(inn + r * hn)
        h = (1 - z) * n + z * h
        out.append(h)
    return torch.stack(out)


def gru_layer(x, W_ih, b_ih, W_hh, b_hh, reverse=False):
    """x [T, B, d] -> [T, B, 100]: every column runs all T steps"""
    gx = x @ W_ih.t() + b_ih
    T = x.shape[0]
    order = torch.arange(T - 1, -1, -1) if reverse else torch.arange(T)
    return gru_scan(gx[order], W_hh, b_hh)[order]       # order is its own inverse


def lstm_layer(x, W_ih, b_ih, W_hh, b_hh, reverse=False):
    """torch.nn.LSTM, gate order i|f|g|o, h0 = c0 = 0, batched over the columns"""
    gx = x @ W_ih.t() + b_ih
    T, B = x.shape[0], x.shape[1]
    h, c, out = gx.new_zeros(B, W_hh.shape[1]), gx.new_zeros(B, W_hh.shape[1]), [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        i, f, g, o = (gx[t] + h @ W_hh.t() + b_hh).chunk(4, -1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        out[t] = h
    return torch.stack(out)


def gru_layer_batched(x, W_ih, b_ih, W_hh, b_hh, reverse=False):
    """gru_layer over all columns at once (the whole-model paths; gru_scan stays the per-dialogue chain)"""
    gx = x @ W_ih.t() + b_ih
    T, B = x.shape[0], x.shape[1]
    h, out = gx.new_zeros(B, W_hh.shape[1]), [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        ir, iz, inn = gx[t].chunk(3, -1)
        hr, hz, hn = (h @ W_hh.t() + b_hh).chunk(3, -1)
        r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
        n = torch.tanh(inn + r * hn)
        h = (1 - z) * n + z * h
        out[t] = h
    return torch.stack(out)


def rnn2(P, cell, x, mask=None):
    """2 layers x 2 directions over the padded batch x [T, B, D] -> [T, B, 200]; ``mask`` [T*B, 200] on the layer-0 output"""
    layer = lstm_layer if cell == "lstm" else gru_layer_batched
    for k in (0, 1):
        halves = []
        for suffix, rev in (("", False), ("_reverse", True)):
            w = [P["%s.%s_l%d%s" % (cell, n, k, suffix)] for n in ("weight_ih", "bias_ih", "weight_hh", "bias_hh")]
            halves.append(layer(x, *w, reverse=rev))
        x = torch.cat(halves, -1)
        if k == 0 and mask is not None:
            x = x * mask.view(x.shape)
    return x


def forward(P, batch, cell, masks=None, double=False):
    """-> (log_prob [N, C], emotions [N, 200]) on the valid rows, dialogue-major"""
    if double:
        P = {k: v.double() for k, v in P.items()}
        masks = None if masks is None else {k: v.double() for k, v in masks.items()}
    x = batch["input_tensor"].to(next(iter(P.values())).dtype)
    lens = [int(v) for v in batch["text_length"]]
    M = rnn2(P, cell, x, None if masks is None else masks["rnn"])
    E = torch.cat([M[:L, b] for b, L in enumerate(lens)])
    Q = E @ P["matchatt.transform.weight"].t() + P["matchatt.transform.bias"]
    A, off = [], 0
    for L in lens:
        e, q = E[off:off + L], Q[off:off + L]
        A.append(torch.softmax(torch.tanh(q @ e.t()), -1) @ e)
        off += L
    Z = F.relu(torch.cat(A) @ P["linear.weight"].t() + P["linear.bias"])
    if masks is not None:
        Z = Z * masks["clf"]
    return F.log_softmax(Z @ P["smax_fc.weight"].t() + P["smax_fc.bias"], -1), E


def loss_and_grads(P, batch, cell, class_weight=None, masks=None, double=False):
    """MaskedNLLLoss (dgcnv2_models.py:13-33) = F.nll_loss over the valid rows, and the gradient of every parameter"""
    Pg = {k: (v.double() if double else v).detach().clone().requires_grad_() for k, v in P.items()}
    log_prob, E = forward(Pg, batch, cell, masks, double)
    w = class_weight.to(log_prob.dtype) if class_weight is not None else None
    loss = F.nll_loss(log_prob, batch["label"], weight=w)
    loss.backward()
    return loss.detach(), log_prob.detach(), E.detach(), {k: v.grad for k, v in Pg.items()}


def adam_steps(P, batch, cell, class_weight, steps, lr=3e-4):
    """``steps`` torch.optim.Adam steps (weight decay 0) on the restatement, eval-mode (no dropout)"""
    Pp = {k: torch.nn.Parameter(v.detach().clone()) for k, v in P.items()}
    opt = torch.optim.Adam(list(Pp.values()), lr=lr)
    losses = []
    for _ in range(steps):
        log_prob, _ = forward(Pp, batch, cell)
        loss = F.nll_loss(log_prob, batch["label"], weight=class_weight)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return {k: v.detach() for k, v in Pp.items()}, losses
