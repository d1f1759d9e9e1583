#!/usr/bin/env python3
"""Golden vectors of the conv-emotion DialogueGCN (track_mm/dgcnv2.py:51-181) from the REFERENCE's own DGCNModule on CPU
fp32, with the stubs and helpers of make_golden.py.  Run here, never on the GPU box (the reference tree is not there):

    python tests/golden/make_golden_dgcnv2.py [--ref /root/reference] [--check]

``--check`` regenerates every fixture in memory and compares it with the committed file (exit 1 on any mismatch).

Two deviations from running the reference as it stands, both in memory only:
  * dgcnv2_models.py's ``mask[edge_ind_] = 1`` and ``mask_copy[edge_ind_] = 1`` relied on legacy numpy-array-as-tuple
    indexing (torch 1.11); they are read as ``mask[tuple(edge_ind_)] = 1`` / ``mask_copy[tuple(edge_ind_)] = 1``.
  * PyG's ``GraphConv`` is absent here.  ``_GraphConv`` below restates it (add aggregation of the source features at
    each target, ``lin_rel(sum) + lin_root(x)``, PyG's parameter names).  GraphConv is therefore pinned only against
    this restatement, not against PyG itself.

Eval mode (dropout off): the logits selected by the attention mask, the returned node features, the (class-weighted)
cross entropy of dgcnv2.py:206, the gradient digest of every parameter, the names of the parameters whose grad stays
None (att_model.matchatt / simpleatt / att) and the state_dict key list with shapes.
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

IEMOCAP6_WEIGHTS = [1 / 0.086747, 1 / 0.144406, 1 / 0.227883, 1 / 0.160585, 1 / 0.127711, 1 / 0.252668]

# (name, param seed, base model, feature dim, speakers, classes, loss weights, dialogue lengths)
CASES = (("dgcnv2_s2", 41, "LSTM", 48, 2, 6, True, (9, 1, 23, 14)),
         ("dgcnv2_s9", 42, "LSTM", 40, 9, 7, False, (17, 6, 30)),
         ("dgcnv2_none", 43, "None", 36, 2, 6, True, (5, 12, 1)))


class _GraphConv(torch.nn.Module):
    """PyG GraphConv(in, out), aggr='add': out_i = lin_rel(sum_{j->i} x_j) + lin_root(x_i)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.lin_rel = torch.nn.Linear(cin, cout, bias=True)
        self.lin_root = torch.nn.Linear(cin, cout, bias=False)

    def forward(self, x, edge_index):
        agg = torch.zeros_like(x).index_add_(0, edge_index[1], x[edge_index[0]])
        return self.lin_rel(agg) + self.lin_root(x)


def load_models(ref):
    """track_mm.dgcnv2_models with the two indexing statements rewritten (module docstring)"""
    path = os.path.join(ref, "track_mm/dgcnv2_models.py")
    with open(path) as fh:
        text = fh.read()
    for old in ("mask[edge_ind_] = 1", "mask_copy[edge_ind_] = 1"):
        assert text.count(old) == 1, old
        text = text.replace(old, old.replace("[edge_ind_]", "[tuple(edge_ind_)]"))
    mod = types.ModuleType("track_mm.dgcnv2_models")
    mod.__file__ = path
    mod.__package__ = "track_mm"
    sys.modules[mod.__name__] = mod
    exec(compile(text, path, "exec"), mod.__dict__)
    return mod


def make_batch(D, S, C, lens, seed):
    g = torch.Generator().manual_seed(seed + 1000)
    B, T = len(lens), max(lens)
    x = torch.randn(T, B, D, generator=g) * 0.5
    spk = torch.randint(0, S, (T, B), generator=g)
    onehot = torch.nn.functional.one_hot(spk, S).float()
    for b, L in enumerate(lens):
        x[L:, b] = 0.0
        onehot[L:, b] = 0.0
    return {"input_tensor": x, "speaker_tensor": onehot, "text_length": torch.tensor(lens, dtype=torch.int64),
            "attention_mask": (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float(),
            "label": torch.randint(0, C, (sum(lens),), generator=g)}


def make_case(dg, seed, base, D, S, C, weighted, lens):
    import torch.nn.functional as F
    batch = make_batch(D, S, C, lens, seed)
    model = dg.DGCNModule(base_model=base, input_size=D, hidden_size=100, n_speakers=S, n_classes=C,
                          context_attention="general")
    mg.fill_params(model, seed)
    model.eval()
    logits, features = model(**batch)
    w = torch.tensor(IEMOCAP6_WEIGHTS) if weighted else None
    loss = F.cross_entropy(logits, batch["label"], weight=w)
    loss.backward()
    sd = model.state_dict()
    shapes = np.full((len(sd), 3), -1, dtype=np.int64)
    for i, v in enumerate(sd.values()):
        shapes[i, :v.dim()] = v.shape
    none = [n for n, q in model.named_parameters() if q.grad is None]
    return dict(param_seed=seed, base_model=np.array(base), n_speakers=S, n_classes=C, loss_weights=np.array(weighted),
                **{"in_" + k: v.numpy() for k, v in batch.items()},
                logits=logits.detach().numpy(), features=features.detach().numpy(), loss=np.array(float(loss.detach())),
                grad_none=np.array(none), sd_keys=np.array(list(sd)), sd_shapes=shapes,
                **mg.grad_digest([(n, q.grad) for n, q in model.named_parameters()]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(1)      # the scatter-adds of the backward sum in a thread-dependent order otherwise
    mg.install_stubs(args.ref)
    sys.modules["torch_geometric.nn"].GraphConv = _GraphConv
    for pkg in ("track_mm", "contrib", "models"):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(args.ref, pkg)]
        sys.modules[pkg] = m
    load_models(args.ref)
    dg = importlib.import_module("track_mm.dgcnv2")
    bad = 0
    for name, *case in CASES:
        arrays = make_case(dg, *case)
        if not args.check:
            mg.save(name, **arrays)
            continue
        old = np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)
        for k, v in arrays.items():
            v = np.asarray(v)
            if k not in old.files or old[k].shape != v.shape or not np.array_equal(old[k], v):
                print("mismatch %s:%s" % (name, k))
                bad += 1
        bad += len(set(old.files) - set(arrays))
    if args.check:
        print("%d mismatches" % bad)
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
