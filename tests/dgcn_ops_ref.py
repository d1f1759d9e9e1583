"""DialogueGCN's graph operators (csrc/dgcn_ops.hip) restated in plain torch on the CPU, ``dtype`` a parameter: float64 is the
reference of tests/test_gpu_dgcn_ops.py, float32 the yardstick that says what an fp32 implementation can deliver.

    ATT = x W^T;  score(j -> k) = ATT[k] . x[j];  norm = softmax over each SOURCE's out-edges
    out = sum_r ( sum_{e -> i, type r} norm_e x_src ) W_r + x root + bias,   W_r = sum_b comp[r, b] basis[b]

Edges are the explicit ``edge_index [2, E]`` (row 0 = source j, row 1 = target k) / ``edge_type [E]`` of
``build_graph_tensors(..., explicit=True)``: canonical (target, then source) order, which is the order of the in-CSR, so
position e of every per-edge vector here is edge e of the kernels.  Nothing of size [E, F, O] or [E, 30, F] is formed: the layer
loops over the occupied relations with ``index_add``.  tests/test_dgcn_ops_ref.py pins this file to oracle.dgcn and the fixtures.
"""
import numpy as np
import torch

from oracle import graph as og

NB = 30          # num_bases (dgcn_models.py:41)


def host_graph(lengths, speakers, wp, wf, n_speakers):
    """edge_index [2, E], edge_type [E] (int64) built on the host, in the device builder's order"""
    ei, et = og.window_graph_closed_form(np.asarray(lengths), np.asarray(speakers), wp, wf, n_speakers)
    return torch.from_numpy(ei.astype(np.int64)), torch.from_numpy(et.astype(np.int64))


def segment_softmax(score, seg, n):
    """softmax of ``score`` within the groups ``seg`` (the maximum is subtracted as a constant: softmax is shift invariant)"""
    mx = torch.full((n,), -float("inf"), dtype=score.dtype).scatter_reduce(0, seg, score.detach(), "amax", include_self=True)
    p = torch.exp(score - mx[seg])
    return p / torch.zeros(n, dtype=score.dtype).index_add(0, seg, p)[seg]


def edge_att_backward(edge_index, x, ATT, norm, dnorm):
    """EdgeAtt's backward from given operands, in their dtype: dscore, DATT = d / dATT, and the source side's share of dx"""
    src, dst = edge_index
    N = x.shape[0]
    t = torch.zeros(N, dtype=x.dtype).index_add(0, src, norm * dnorm)
    dscore = norm * (dnorm - t[src])
    DATT = torch.zeros_like(x).index_add(0, dst, dscore[:, None] * x[src])
    dx_src = torch.zeros_like(x).index_add(0, src, dscore[:, None] * ATT[dst])
    return dscore, DATT, dx_src


def relation_sums(TT, edge_type, R):
    """datt[r, :] = sum of the rows of TT whose edge has type r, in TT's dtype"""
    return torch.zeros(R, TT.shape[1], dtype=TT.dtype).index_add(0, edge_type, TT)


def restate(edge_index, edge_type, R, x, W, comp, basis, root, bias, gout, dtype=torch.float64):
    """Forward, autograd backward of (out * gout).sum(), and the kernels' intermediates in their own layouts; every value detached."""
    src, dst = edge_index
    N, F = x.shape
    O = basis.shape[2]
    x, W, comp, basis, root, bias = (t.detach().to(dtype).clone().requires_grad_() for t in (x, W, comp, basis, root, bias))
    gout = gout.detach().to(dtype)
    ATT = x @ W.t()
    score = (ATT[dst] * x[src]).sum(1)
    norm = segment_softmax(score, src, N)
    Wr = torch.einsum("rb,bfo->rfo", comp, basis)
    for t in (ATT, score, norm, Wr):
        t.retain_grad()
    out = x @ root + bias
    for r in torch.unique(edge_type).tolist():
        e = torch.nonzero(edge_type == r).flatten()
        out = out + torch.zeros(N, F, dtype=dtype).index_add(0, dst[e], norm[e, None] * x[src[e]]) @ Wr[r]
    (out * gout).sum().backward()
    res = dict(ATT=ATT, score=score, norm=norm, out=out, Wr=Wr, WrT=Wr.transpose(1, 2).contiguous(), dx=x.grad, dW=W.grad,
               dbasis=basis.grad, dcomp=comp.grad, droot=root.grad, dbias=bias.grad, dnorm=norm.grad, dscore=score.grad,
               DATT=ATT.grad, dWr=Wr.grad)
    with torch.no_grad():
        xd, nd, cd, bd = x.detach(), norm.detach(), comp.detach(), basis.detach()
        flat = dst * R + edge_type
        Z_rel = torch.zeros(N * R, F, dtype=dtype).index_add(0, flat, nd[:, None] * xd[src]).view(N, R, F)
        Z = torch.einsum("nrf,rb->nbf", Z_rel, cd)
        dZ = torch.einsum("bfo,no->nbf", bd, gout)
        dZ_rel = torch.einsum("rfo,no->nrf", Wr.detach(), gout)
        T = torch.stack([(xd[src] * dZ[dst, b]).sum(1) for b in range(NB)], 1)          # T_e[b] = x_src . dZ[dst, b, :]
        U_rel = torch.zeros(N * R, O, dtype=dtype).index_add(0, src * R + edge_type, nd[:, None] * gout[dst]).view(N, R, O)
        U = torch.einsum("nro,rb->nbo", U_rel, cd)
        dscore, DATT, dx_att = edge_att_backward(edge_index, xd, ATT.detach(), nd, norm.grad)
        res.update(Z=Z.reshape(N, NB * F), Z_rel=Z_rel.reshape(N, R * F), dZ=dZ.reshape(N, NB * F), dZ_rel=dZ_rel.reshape(N, R * F),
                   TT=nd[:, None] * T, U=U.reshape(N, NB * O), U_rel=U_rel.reshape(N, R * O), dx_att=dx_att,
                   dx_rgcn=torch.einsum("nbo,bfo->nf", U, bd) + gout @ root.detach().t(), dscore_closed=dscore, DATT_closed=DATT)
    return {k: v.detach() for k, v in res.items()}
