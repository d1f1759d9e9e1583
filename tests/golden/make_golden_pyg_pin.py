#!/usr/bin/env python3
"""Golden vectors that pin the two graph operators the reference takes from PyG -- COGMEN's ``RGCNConv(aggr='mean')`` and
DialogueGCN's ``GraphConv(aggr='add')`` -- to an operator the reference ships: the vendored PyG 1.4.2 ``RGCNConv``
(models/rgcn.py:264-355).  It computes ``out_i = sum_{e: dst(e) = i} edge_norm_e x_src(e) W_type(e) + x_i root + bias`` with
``W_r = sum_b att[r, b] basis[b]``, the message taken from ``edge_index[0]`` and summed at ``edge_index[1]``.  Two settings of it
are the operators of the model:

  * ``num_bases = R``, ``att = I_R``, ``edge_norm_e = 1 / |N_type(e)(dst(e))|`` (the per-relation in-degree): RGCNConv-mean
    (``weight = basis``);
  * ``R = 1``, ``att = [[1]]``, no edge_norm: GraphConv-add (``basis[0] = lin_rel.weight^T``, ``root = lin_root.weight^T``,
    ``bias = lin_rel.bias``).

What this cannot pin: that PyG 2's RGCNConv(aggr='mean') takes the mean PER RELATION (and not over all in-edges) is PyG's
documented definition; here it is encoded in how edge_norm is built.

The graphs come from the reference's own COGMEN window builder (track_mm/cogmen_utils.py batch_graphify), the parameters from
the shared deterministic filler (the fixture carries the seed).  Run here, never on the GPU box (the reference tree is not there):

    python tests/golden/make_golden_pyg_pin.py [--ref /root/reference] [--check]

``--check`` regenerates every fixture in memory and compares it with the committed file: integers bit for bit, floats to 1e-6 of
the array's scale (exit 1 on any mismatch).
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

F = 100
R_COGMEN = 8
# (name, speakers, window past / future, dialogue lengths, graph seed, parameter seed)
RGCN_CASES = (("rgcn_mean_s2", 2, 5, 5, (1, 4, 9, 13, 22, 7), 71, 81),
              ("rgcn_mean_s3", 3, 5, 5, (1, 3, 11, 17, 8), 72, 82))
GCONV_CASES = (("graphconv_add", 9, 10, 10, (1, 6, 15, 24, 12), 73, 83),
               ("graphconv_add_w2_4", 2, 2, 4, (1, 5, 14, 9), 74, 84))    # asymmetric window: the message direction shows


def make_graph(cu, S, wp, wf, lens, seed):
    """node features and the reference's window graph in canonical (target, source) order"""
    from oracle.graph import relation_table, canonical_edges
    g = torch.Generator().manual_seed(seed)
    B, T = len(lens), max(lens)
    spk = torch.randint(0, S, (B, T), generator=g)
    feats = torch.randn(B, T, F, generator=g)
    for b, L in enumerate(lens):
        spk[b, L:] = 0
        feats[b, L:] = 0.0
    x, ei, et, _ = cu.batch_graphify(feats, torch.tensor(lens), spk, wp, wf, relation_table(S))
    ei_s, et_s = canonical_edges(ei.numpy(), et.numpy())
    return spk, x.detach().clone(), torch.from_numpy(ei_s).long(), torch.from_numpy(et_s).long()


def gen_rgcn_mean(rg, cu, name, S, wp, wf, lens, gseed, pseed):
    from oracle.pyg import RGCNConvMean
    spk, x, ei, et = make_graph(cu, S, wp, wf, lens, gseed)
    N, R = x.shape[0], R_COGMEN
    holder = RGCNConvMean(F, F, R)          # parameter holder only: names / shapes of COGMEN's gcn.conv1
    mg.fill_params(holder, pseed)
    # relation ids >= R: COGMEN's RGCNConv has R = 8 relations and PyG loops over range(num_relations) -- not in the call
    keep = et < R
    src, dst, typ = ei[0, keep], ei[1, keep], et[keep]
    cnt = torch.zeros(N, R).index_put_((dst, typ), torch.ones(src.numel()), accumulate=True)
    norm = 1.0 / cnt[dst, typ]
    conv = rg.RGCNConv(F, F, R, num_bases=R)
    with torch.no_grad():
        conv.basis.copy_(holder.weight)
        conv.att.copy_(torch.eye(R))
        conv.root.copy_(holder.root)
        conv.bias.copy_(holder.bias)
    xg = x.clone().requires_grad_(True)
    out = conv(xg, torch.stack([src, dst]), typ, edge_norm=norm)
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(pseed + 1000))
    out.backward(gout)
    edge_norm = torch.zeros(ei.shape[1])
    edge_norm[keep] = norm
    return dict(lengths=np.array(lens, dtype=np.int64), speakers=spk.numpy(), n_speakers=S, wp=wp, wf=wf, num_relations=R,
                param_seed=pseed, edge_index=ei.numpy(), edge_type=et.numpy(), in_reference_call=keep.numpy(),
                edge_norm=edge_norm.numpy(), x=x.numpy(), out=out.detach().numpy(), gout=gout.numpy(), dx=xg.grad.numpy(),
                dweight=conv.basis.grad.numpy(), droot=conv.root.grad.numpy(), dbias=conv.bias.grad.numpy())


def gen_graphconv_add(rg, cu, name, S, wp, wf, lens, gseed, pseed):
    from oracle.pyg import GraphConvAdd
    spk, x, ei, et = make_graph(cu, S, wp, wf, lens, gseed)
    holder = GraphConvAdd(F, F)             # parameter holder only: names / shapes of DialogueGCN's gcn.conv2
    mg.fill_params(holder, pseed)
    conv = rg.RGCNConv(F, F, 1, num_bases=1)
    with torch.no_grad():
        conv.basis.copy_(holder.lin_rel.weight.t()[None])
        conv.att.fill_(1.0)
        conv.root.copy_(holder.lin_root.weight.t())
        conv.bias.copy_(holder.lin_rel.bias)
    xg = x.clone().requires_grad_(True)
    out = conv(xg, ei, torch.zeros_like(et))
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(pseed + 1000))
    out.backward(gout)
    return dict(lengths=np.array(lens, dtype=np.int64), speakers=spk.numpy(), n_speakers=S, wp=wp, wf=wf, param_seed=pseed,
                edge_index=ei.numpy(), x=x.numpy(), out=out.detach().numpy(), gout=gout.numpy(), dx=xg.grad.numpy(),
                # in GraphConv's layout: lin_rel.weight = basis[0]^T, lin_root.weight = root^T
                dlin_rel_weight=conv.basis.grad[0].t().numpy(), dlin_rel_bias=conv.bias.grad.numpy(),
                dlin_root_weight=conv.root.grad.t().numpy())


def same(old, new):
    if old.shape != new.shape or old.dtype != new.dtype:
        return False
    if not np.issubdtype(new.dtype, np.floating):
        return bool(np.array_equal(old, new))
    return float(np.abs(old.astype(np.float64) - new).max(initial=0.0)) <= 1e-6 * float(np.abs(new).max(initial=0.0)) + 1e-30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(1)      # the scatter-adds of the backward sum in a thread-dependent order otherwise
    mg.install_stubs(args.ref)
    for pkg in ("track_mm", "contrib", "models"):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(args.ref, pkg)]
        sys.modules[pkg] = m
    rg = importlib.import_module("models.rgcn")
    cu = importlib.import_module("track_mm.cogmen_utils")
    bad = 0
    for gen, cases in ((gen_rgcn_mean, RGCN_CASES), (gen_graphconv_add, GCONV_CASES)):
        for name, *case in cases:
            arrays = {k: np.asarray(v) for k, v in gen(rg, cu, name, *case).items()}
            if not args.check:
                mg.save(name, **arrays)
                continue
            old = np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)
            for k, v in arrays.items():
                if k not in old.files or not same(old[k], v):
                    print("mismatch %s:%s" % (name, k))
                    bad += 1
            bad += len(set(old.files) - set(arrays))
    if args.check:
        print("%d mismatches" % bad)
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
