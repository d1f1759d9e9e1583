"""Float64 restatement of MMGCN's 64-layer GCNII chain on the inputs of the chain kernels (csrc/gcnii_chain.hip), for the tests.

Reference formula per layer l = 1..64 (track_mm/mmgcn_models.py:27-39,385-388), NOT the kernels' re-association:
    hi = A h ;  out_l = theta_l [hi | h0] W_l + (1 - theta_l) ((1 - alpha) hi + alpha h0) ;  h <- keep_l . relu(out_l) . ks
with theta_l = ln(lambda / l + 1), lambda = 0.5, alpha = 0.1.  A is the block-structured adjacency of the kernels: per
dialogue b and modality m the block ADJ[b Mo + m][:L, :L], and between modalities m != n of the same utterance t the entry
CR[b][m Mo + n][t].  Rows are in node order (row m N + node_off[b] + t), as the kernels keep them; A is applied block by
block (batched over the dialogues), the dense (Mo N)^2 matrix is never built.

The backward runs with autograd one layer at a time (each layer recomputed from its saved input plane), so memory holds the
planes and saves only.  Gradients wrt the ADJ blocks and the CR entries accumulate over the layers; dz_l = A^T dg_l (equal to
A dg_l: the adjacency MMGCN builds is symmetric, which the kernels rely on).
"""
import math

import torch

FD, NL, LAMDA, ALPHA = 200, 64, 0.5, 0.1
MAXRW = 32       # rows of a part in the kernels' 32-row form


def theta(l):
    return math.log(LAMDA / l + 1)


def v_matrix(W, l):
    """V_l = theta W_l[:FD] + (1 - theta)(1 - alpha) I: z_l = h_l V_l is what the chain exchanges (l 1-based)"""
    th = theta(l)
    return th * W[l - 1, :FD] + (1 - th) * (1 - ALPHA) * torch.eye(FD, dtype=W.dtype)


def u_matrix(W, l):
    """U_l = theta W_l[FD:] + (1 - theta) alpha I: c_l = h0 U_l"""
    th = theta(l)
    return th * W[l - 1, FD:] + (1 - th) * ALPHA * torch.eye(FD, dtype=W.dtype)


class _Blocks:
    """the adjacency of a batch as blocks: index maps between node rows and padded [B Mo, T] positions"""

    def __init__(self, node_off, Mo, P):
        off = [int(v) for v in node_off]
        self.B, self.Mo, self.P = len(off) - 1, Mo, P
        self.lens = [off[b + 1] - off[b] for b in range(self.B)]
        self.N, self.T = off[-1], max(self.lens)
        B, T, N = self.B, self.T, self.N
        gather = torch.full((B * Mo, T), Mo * N, dtype=torch.long)        # padded position -> node row (Mo N: a zero row)
        pos = torch.empty(Mo * N, dtype=torch.long)                       # node row -> padded position (b Mo + m) T + t
        dlg, tpos = torch.empty(N, dtype=torch.long), torch.empty(N, dtype=torch.long)
        valid = torch.zeros(B * Mo, T, dtype=torch.float64)
        for b, L in enumerate(self.lens):
            t = torch.arange(L)
            dlg[off[b]:off[b + 1]], tpos[off[b]:off[b + 1]] = b, t
            for m in range(Mo):
                rows = m * N + off[b] + t
                gather[b * Mo + m, :L] = rows
                pos[rows] = (b * Mo + m) * T + t
                valid[b * Mo + m, :L] = 1
        self.gather, self.pos, self.dlg, self.tpos = gather, pos, dlg, tpos
        self.vmask = valid[:, :, None] * valid[:, None, :]
        self.offdiag = (1 - torch.eye(Mo, dtype=torch.float64))[:, :, None]

    def operands(self, ADJ, CR):
        """ADJ [B Mo, P, P] -> the padded blocks [B Mo, T, T] (zero outside the dialogue); CR [B, Mo Mo, P] -> per node
        the cross coefficients cw [Mo (row modality), Mo (column modality), N], zero on the diagonal"""
        A = ADJ.reshape(self.B * self.Mo, self.P, self.P)[:, :self.T, :self.T] * self.vmask
        cw = CR.reshape(self.B, self.Mo, self.Mo, self.P)[self.dlg, :, :, self.tpos].permute(1, 2, 0) * self.offdiag
        return A, cw

    def apply(self, A, cw, h):
        """A h on node rows h [Mo N, FD]"""
        hp = torch.cat([h, h.new_zeros(1, h.shape[1])])[self.gather]      # [B Mo, T, FD]
        out = (A @ hp).reshape(-1, h.shape[1])[self.pos]
        hv = h.reshape(self.Mo, self.N, -1)
        cross = torch.einsum("mnj,njc->mjc", cw, hv).reshape(self.Mo * self.N, -1)
        return out + cross

    def apply_t(self, A, cw, g):
        """A^T g"""
        return self.apply(A.transpose(1, 2), cw.transpose(0, 1), g)


def _layer(blk, A, cw, h, h0, Wl, l):
    th = theta(l)
    hi = blk.apply(A, cw, h)
    return th * (hi @ Wl[:FD] + h0 @ Wl[FD:]) + (1 - th) * ((1 - ALPHA) * hi + ALPHA * h0)


def _post(out, l, keep, ks, act):
    h = out * act[l - 1] if act is not None else torch.relu(out)
    if keep is not None:
        h = h * keep[l - 1] * ks
    return h


def chain_ref(ADJ, CR, node_off, h0, h1, W, Mo, dHin=None, keep=None, ks=1.0, act=None):
    """The chain in float64 on the kernels' inputs (any dtype / device; computed on the CPU).

    ADJ [B Mo, P, P], CR [B, Mo Mo, P], node_off [B + 1], h0 [Mo N, FD] (the residual input), h1 [Mo N, FD] (plane 1, the
    chain's input), W [NL, 2 FD, FD] (layer l at index l - 1).  keep (optional) [NL, Mo N, FD]: the 0/1 dropout keep mask of
    each layer, applied with the scale ks = 1 / (1 - p).  act (optional) [NL, Mo N, FD]: 0/1 patterns used in place of relu's
    (out > 0) -- kink-aware comparison with an fp32 chain, whose outputs within rounding of zero may take the other sign;
    the forward then keeps out . act.  dHin [Mo N, FD]: gradient wrt the last plane; without it only the forward runs.

    Returns float64 tensors: planes [NL + 1, Mo N, FD] (plane l at index l - 1), z [NL, Mo N, FD] (z_l = h_l V_l), and with
    dHin: dg [NL, Mo N, FD] (gradient wrt out_l), dz [NL, Mo N, FD] (A^T dg_l), dh1, dh0 [Mo N, FD], dW [NL, 2 FD, FD],
    dADJ [B Mo, P, P], dCR [B, Mo Mo, P] (diagonal entries m == n zero: the chain does not read them).  With act: "kinks",
    the number of (kept) entries where act differs from out > 0, and "kink_max", the largest |out| among them."""
    f64 = lambda t: None if t is None else torch.as_tensor(t).detach().to("cpu", torch.float64)
    ADJ, CR, h0, h1, W = f64(ADJ), f64(CR), f64(h0), f64(h1), f64(W)
    keep, act = f64(keep), f64(act)
    blk = _Blocks(torch.as_tensor(node_off).cpu(), Mo, ADJ.shape[-1])
    A, cw = blk.operands(ADJ, CR)
    res = {"kinks": 0, "kink_max": 0.0}
    planes, z = [h1], []
    with torch.no_grad():
        h = h1
        for l in range(1, NL + 1):
            z.append(h @ v_matrix(W, l))
            out = _layer(blk, A, cw, h, h0, W[l - 1], l)
            if act is not None:      # where the given pattern differs from the float64 sign: count, largest |out| there
                flip = (act[l - 1] != (out > 0).double()) & (keep[l - 1] != 0 if keep is not None else True)
                res["kinks"] += int(flip.sum())
                res["kink_max"] = max(res["kink_max"], float(out[flip].abs().max()) if flip.any() else 0.0)
            h = _post(out, l, keep, ks, act)
            planes.append(h)
    res["planes"], res["z"] = torch.stack(planes), torch.stack(z)
    if dHin is None:
        return res
    ADJg, CRg, h0g = ADJ.clone().requires_grad_(), CR.clone().requires_grad_(), h0.clone().requires_grad_()
    g = f64(dHin)
    dg, dz, dW = [None] * NL, [None] * NL, torch.zeros_like(W)
    for l in range(NL, 0, -1):
        hl = planes[l - 1].clone().requires_grad_()
        Wl = W[l - 1].clone().requires_grad_()
        Ag, cwg = blk.operands(ADJg, CRg)
        out = _layer(blk, Ag, cwg, hl, h0g, Wl, l)
        out.retain_grad()
        _post(out, l, keep, ks, act).backward(g)
        dg[l - 1], dW[l - 1], g = out.grad, Wl.grad, hl.grad
        with torch.no_grad():
            dz[l - 1] = blk.apply_t(A, cw, out.grad)
    res.update(dg=torch.stack(dg), dz=torch.stack(dz), dh1=g, dh0=h0g.grad, dW=dW, dADJ=ADJg.grad, dCR=CRg.grad)
    return res


def pre_activations(ADJ, CR, node_off, h0, planes, W, Mo):
    """out_l [NL, Mo N, FD] in float64 from given input planes [NL, Mo N, FD] (plane l at index l - 1), e.g. a kernel's own"""
    f64 = lambda t: torch.as_tensor(t).detach().to("cpu", torch.float64)
    ADJ, CR, h0, W = f64(ADJ), f64(CR), f64(h0), f64(W)
    blk = _Blocks(torch.as_tensor(node_off).cpu(), Mo, ADJ.shape[-1])
    A, cw = blk.operands(ADJ, CR)
    with torch.no_grad():
        return torch.stack([_layer(blk, A, cw, f64(planes[l - 1]), h0, W[l - 1], l) for l in range(1, NL + 1)])


def launches(lens, Mo, T, cfg):
    """[(b0, nb, grid, RW)]: the launches chain_launch makes for ``cfg`` and the part width gcnii_chain_kernel takes in each
    (tot16 <= grid -> 16), with the fit of the table asserted"""
    parts, cap, dpl = cfg
    out = []
    for b0 in range(0, len(lens), dpl):
        ls = lens[b0:b0 + dpl]
        grid = min(Mo * len(ls) * ((T + 15) // 16), cap)
        tot16 = sum(Mo * ((L + 15) // 16) for L in ls)
        rw = 16 if tot16 <= grid else MAXRW
        assert sum(Mo * ((L + rw - 1) // rw) for L in ls) <= grid
        out.append((b0, len(ls), grid, rw))
    return out


def build_adjacency(feats, node_off, P):
    """The kernels' adjacency inputs from per-modality features [Mo][N, d] (node order within a modality), dialogue by
    dialogue through oracle.mmgcn.big_adjacency (cosine blocks, cross-modal same-utterance entries, symmetric degree
    normalisation): ADJ [B Mo, P, P] and CR [B, Mo Mo, P] in the features' dtype, zero outside the dialogues (diagonal
    entries of CR too)."""
    from oracle.mmgcn import big_adjacency
    off = [int(v) for v in node_off]
    B, Mo = len(off) - 1, len(feats)
    ADJ = torch.zeros(B * Mo, P, P, dtype=feats[0].dtype)
    CR = torch.zeros(B, Mo * Mo, P, dtype=feats[0].dtype)
    for b in range(B):
        L = off[b + 1] - off[b]
        a = big_adjacency([f[off[b]:off[b + 1]] for f in feats], [L])
        idx = torch.arange(L)
        for m in range(Mo):
            ADJ[b * Mo + m, :L, :L] = a[m * L:(m + 1) * L, m * L:(m + 1) * L]
            for n in range(Mo):
                if n != m:
                    CR[b, m * Mo + n, :L] = a[m * L + idx, n * L + idx]
    return ADJ, CR


def oracle_per_dialogue(ref, batch):
    """oracle.mmgcn.MMGCNOracle ``ref`` (eval mode, in its own dtype) run dialogue by dialogue on a time-major ``batch``: each
    dialogue is sliced at the full T, so the unpacked text BiLSTM sees the same padding as in the whole batch.  The batch's
    mean cross entropy over its N nodes is sum_b (L_b / N) loss_b, and so are its gradients.
    Returns (logits [N, C], loss, {parameter name: gradient}) in the oracle's dtype; ``ref``'s own grads are left cleared."""
    from torch.nn import functional as F
    dt = next(ref.parameters()).dtype
    lens = [int(v) for v in batch["text_length"]]
    N = sum(lens)
    logits, grads, loss, off = [], {}, 0.0, 0
    for b, L in enumerate(lens):
        sub = {k: (batch[k][:, b:b + 1].to(dt) if batch.get(k) is not None else None)
               for k in ("text_feature", "audio_feature", "visual_feature", "speaker_tensor")}
        sub["text_length"] = batch["text_length"][b:b + 1]
        ref.zero_grad(set_to_none=True)
        lg, _ = ref(**sub)
        lb = F.cross_entropy(lg, batch["label"][off:off + L])
        lb.backward()
        w = L / N
        loss = loss + w * lb.detach()
        for n, p in ref.named_parameters():
            if p.grad is not None:
                grads[n] = grads[n] + w * p.grad if n in grads else w * p.grad
        logits.append(lg.detach())
        off += L
    ref.zero_grad(set_to_none=True)
    return torch.cat(logits), loss, grads
