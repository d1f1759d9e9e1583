"""CPU restatement of CIM's forward (track_mm/cim.py:64-173) in fp32, written from the math, for the tests.

Parameters come as a ``{state_dict name: tensor}`` mapping; gradients follow from autograd.  Rows are compact (the valid
utterances of each dialogue in order, as ``label`` is), so padded positions cannot influence anything.  ``masks`` (optional)
gives the dropout multipliers, already scaled by 1 / (1 - p): ``drop0_<m>`` [N, 400] on the GRU output and ``drop1_<m>``
[N, 100] on the adapter output of modality m; without masks the step runs as in eval mode.
"""
import torch

H = 200
FEATURE = {"a": "audio_feature", "v": "visual_feature", "t": "text_feature"}
PAIRS = (("a", "v"), ("v", "a"), ("t", "a"), ("t", "v"), ("a", "t"), ("v", "t"))


def gru_direction(x, w_ih, w_hh, b_ih, b_hh):
    """one direction over x [L, d] from h0 = 0; gate order r | z | n"""
    gx = x @ w_ih.t() + b_ih
    h = x.new_zeros(H)
    out = []
    for t in range(x.shape[0]):
        gh = w_hh @ h + b_hh
        r = torch.sigmoid(gx[t, :H] + gh[:H])
        z = torch.sigmoid(gx[t, H:2 * H] + gh[H:2 * H])
        n = torch.tanh(gx[t, 2 * H:] + r * gh[2 * H:])
        h = (1 - z) * n + z * h
        out.append(h)
    return torch.stack(out)


def bigru_compact(x, lengths, P, prefix):
    """x [B, T, d] -> [N, 400]: forward | reverse outputs of the valid positions, dialogue-major"""
    rows = []
    for b, L in enumerate(lengths):
        xb = x[b, :L]
        f = gru_direction(xb, P[prefix + "weight_ih_l0"], P[prefix + "weight_hh_l0"], P[prefix + "bias_ih_l0"],
                          P[prefix + "bias_hh_l0"])
        r = gru_direction(xb.flip(0), P[prefix + "weight_ih_l0_reverse"], P[prefix + "weight_hh_l0_reverse"],
                          P[prefix + "bias_ih_l0_reverse"], P[prefix + "bias_hh_l0_reverse"]).flip(0)
        rows.append(torch.cat([f, r], -1))
    return torch.cat(rows)


def cross_attention(x, y, lengths):
    """softmax over each dialogue's valid keys of x y^T, times y, times x elementwise; x, y [N, 100] compact"""
    out, o = [], 0
    for L in lengths:
        xb, yb = x[o:o + L], y[o:o + L]
        out.append(torch.softmax(xb @ yb.t(), -1) @ yb * xb)
        o += L
    return torch.cat(out)


def cim_forward(P, batch, masks=None):
    """-> (logits2 [N, C], logits7 [N, 7], intermediates)"""
    lengths = [int(v) for v in batch["text_length"]]
    dense, hid = {}, {}
    for m in "avt":
        h = bigru_compact(batch[FEATURE[m]].float(), lengths, P, "rnn.%s." % m)
        if masks is not None:
            h = h * masks["drop0_" + m]
        hid[m] = h
        d = torch.relu(h @ P["adapter.%s.0.weight" % m].t() + P["adapter.%s.0.bias" % m])
        if masks is not None:
            d = d * masks["drop1_" + m]
        dense[m] = d
    merged = torch.cat([cross_attention(dense[x], dense[y], lengths) for x, y in PAIRS] + [dense[m] for m in "avt"], -1)
    logits2 = merged @ P["cls2.weight"].t() + P["cls2.bias"]
    logits7 = merged @ P["cls7.weight"].t() + P["cls7.bias"]
    return logits2, logits7, dict(merged=merged, dense=dense, hidden=hid)


def cim_loss_and_grads(P, batch, masks=None):
    """unweighted mean cross entropy on logits2 (cim.py:204) and the gradient of every parameter (None = untouched)"""
    Q = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    logits2, logits7, inter = cim_forward(Q, batch, masks)
    loss = torch.nn.functional.cross_entropy(logits2, batch["label"])
    loss.backward()
    return loss.detach(), logits2.detach(), logits7.detach(), {k: (v.grad if v.grad is None else v.grad.detach()) for k, v in Q.items()}, inter


def adam_step(P, grads, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    """one torch.optim.Adam step from fresh state; parameters without a gradient are skipped (grad None)"""
    Q = {k: torch.nn.Parameter(v.detach().clone()) for k, v in P.items()}
    for k, g in grads.items():
        Q[k].grad = None if g is None else g.clone()
    opt = torch.optim.Adam(list(Q.values()), lr=lr, betas=betas, eps=eps)
    opt.step()
    return {k: v.detach() for k, v in Q.items()}, opt
