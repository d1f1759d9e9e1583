"""CPU restatement of the DialogueRNN model (track_mm/dgcnv2_models.py:235-347 DialogueRNNCell / DialogueRNN, :428-487
DialogRNNModel with context_attention='general', listener_state=False), written from the math rather than from the
reference's loops: one scan per (dialogue, direction) over its valid utterances only, only the speaker's party cell.
Parameters come as a dict keyed by the reference's state_dict names.  ``masks`` (training mode) gives the applied dropout
masks, already scaled by 1 / (1 - p), on compact rows (dialogue-major): ``g`` / ``q`` [2, N, 150], ``e`` [2, N, 100] per
direction, ``emo`` [N, 200] after the two scans and ``clf`` [N, D_h] after the classifier's ReLU."""
import torch
import torch.nn.functional as F

MAX_T = 110
DIRS = ("dialog_rnn_f", "dialog_rnn_r")
GXW = 1050


def gru_gates(gi, gh, h):
    """torch.nn.GRUCell from its two pre-activation halves (gate order r | z | n)"""
    ir, iz, inn = gi.chunk(3, -1)
    hr, hz, hn = gh.chunk(3, -1)
    r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
    n = torch.tanh(inn + r * hn)
    return (1 - z) * n + z * h


def hoist(P, d, U):
    """[L, 1050] u-side products of direction d: W_ih^g[:, :D] u + b_ih^g | W_ih^p[:, :D] u + b_ih^p | W_a u"""
    c = DIRS[d] + ".dialogue_cell."
    D = U.shape[-1]
    return torch.cat([U @ P[c + "g_cell.weight_ih"][:, :D].t() + P[c + "g_cell.bias_ih"],
                      U @ P[c + "p_cell.weight_ih"][:, :D].t() + P[c + "p_cell.bias_ih"],
                      U @ P[c + "attention.transform.weight"].t()], -1)


def scan_gx(P, d, gx, spk, D, n_speakers, masks=None):
    """one dialogue in scan order: gx [L, 1050] hoisted products, spk [L] speaker ids -> e' [L, 100].  ``masks`` = (g, q, e)
    rows in the same order, or None."""
    c = DIRS[d] + ".dialogue_cell."
    Wg, Wgh, bgh = P[c + "g_cell.weight_ih"][:, D:], P[c + "g_cell.weight_hh"], P[c + "g_cell.bias_hh"]
    Wp, Wph, bph = P[c + "p_cell.weight_ih"][:, D:], P[c + "p_cell.weight_hh"], P[c + "p_cell.bias_hh"]
    Wei, Weh, bei, beh = (P[c + "e_cell." + k] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
    L = gx.shape[0]
    q = [gx.new_zeros(150) for _ in range(n_speakers)]
    g_prev, e_prev, hist, out = gx.new_zeros(150), gx.new_zeros(100), [], []
    for s in range(L):
        p = int(spk[s])
        g = gru_gates(gx[s, :450] + q[p] @ Wg.t(), g_prev @ Wgh.t() + bgh, g_prev)
        if masks is not None:
            g = g * masks[0][s]
        if hist:
            H = torch.stack(hist)
            ctx = torch.softmax(H @ gx[s, 900:], 0) @ H
        else:
            ctx = gx.new_zeros(150)
        qn = gru_gates(gx[s, 450:900] + ctx @ Wp.t(), q[p] @ Wph.t() + bph, q[p])
        if masks is not None:
            qn = qn * masks[1][s]
        q[p] = qn
        e = gru_gates(qn @ Wei.t() + bei, e_prev @ Weh.t() + beh, e_prev)
        if masks is not None:
            e = e * masks[2][s]
        hist.append(g)
        g_prev, e_prev = g, e
        out.append(e)
    return torch.stack(out)


def emotions(P, batch, masks=None):
    """[N, 200] in dialogue-major node order: forward scan | reverse scan flipped back (before dropout_rec)"""
    x, onehot, lens = batch["input_tensor"], batch["speaker_tensor"], [int(v) for v in batch["text_length"]]
    x = x.to(next(iter(P.values())).dtype)
    S, D = onehot.shape[-1], x.shape[-1]
    spk = onehot.argmax(-1)
    rows, off = [], 0
    for b, L in enumerate(lens):
        U, sp = x[:L, b], spk[:L, b]
        halves = []
        for d in (0, 1):
            order = torch.arange(L) if d == 0 else torch.arange(L - 1, -1, -1)
            m = None if masks is None else tuple(masks[k][d, off:off + L][order] for k in ("g", "q", "e"))
            e = scan_gx(P, d, hoist(P, d, U[order]), sp[order], D, S, m)
            halves.append(e[order])                # order is its own inverse
        rows.append(torch.cat(halves, -1))
        off += L
    return torch.cat(rows)


def forward(P, batch, masks=None, double=False):
    """-> (log_prob [N, C], emotions [N, 200]) on the valid rows, dialogue-major"""
    if double:
        P = {k: v.double() for k, v in P.items()}
        masks = None if masks is None else {k: v.double() for k, v in masks.items()}
    lens = [int(v) for v in batch["text_length"]]
    E = emotions(P, batch, masks)
    if masks is not None:
        E = E * masks["emo"]
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


def loss_and_grads(P, batch, class_weight=None, masks=None, double=False):
    """MaskedNLLLoss (dgcnv2_models.py:13-33) = F.nll_loss over the valid rows, and the gradient of every parameter"""
    Pg = {k: (v.double() if double else v).detach().clone().requires_grad_() for k, v in P.items()}
    log_prob, E = forward(Pg, batch, masks, double)
    w = class_weight.to(log_prob.dtype) if class_weight is not None else None
    loss = F.nll_loss(log_prob, batch["label"], weight=w)
    loss.backward()
    return loss.detach(), log_prob.detach(), E.detach(), {k: v.grad for k, v in Pg.items()}


def adam_step(P, grads, lr=3e-4, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam's first step (weight decay 0)"""
    out = {}
    for k, v in P.items():
        g = grads.get(k)
        if g is None:
            out[k] = v.clone()
            continue
        g = g.to(v.dtype)
        m = (1 - betas[0]) * g
        s = (1 - betas[1]) * g * g
        out[k] = v - lr * (m / (1 - betas[0])) / ((s / (1 - betas[1])).sqrt() + eps)
    return out
