#!/usr/bin/env python3
"""Golden vectors of CIM (track_mm/cim.py:64-173) from the REFERENCE's own CIMModule on CPU fp32, with the stubs and
helpers of make_golden.py.  Run here, never on the GPU box (the reference tree is not there):

    python tests/golden/make_golden_cim.py [--ref /root/reference] [--check]

``--check`` regenerates every fixture in memory and compares it with the committed file (exit 1 on any mismatch).
Eval mode (dropout off): logits2 / logits7 selected by the attention mask, the unweighted cross entropy of cim.py:204,
the gradient digest of every parameter, the names of the parameters whose grad stays None (rnn_adapter.*, cls7.*),
and the state_dict key list with shapes.
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

# (name, param seed, dims a/t/v, n_classes, dialogue lengths): ragged, with a length-1 dialogue; IEMOCAP feature sizes
CASES = (("cim_tiny", 31, dict(a=12, t=16, v=20), 6, (4, 1, 9)),
         ("cim_iemocap_c4", 32, dict(a=100, t=100, v=512), 4, (7, 13, 1, 5)),
         ("cim_iemocap_c6", 33, dict(a=100, t=100, v=512), 6, (11, 3, 6)))


def make_case(cim, name, seed, dims, C, lens):
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed + 1000)
    B, T = len(lens), max(lens)
    batch = {"text_length": torch.tensor(lens, dtype=torch.int64),
             "attention_mask": (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float()}
    for m, key in (("a", "audio_feature"), ("t", "text_feature"), ("v", "visual_feature")):
        x = torch.randn(B, T, dims[m], generator=g) * 0.5
        for b, L in enumerate(lens):
            x[b, L:] = 0.0
        batch[key] = x
    batch["label"] = torch.randint(0, C, (sum(lens),), generator=g)
    model = cim.CIMModule(text_dim=dims["t"], audio_dim=dims["a"], visual_dim=dims["v"], hidden_size=200, n_classes=C)
    mg.fill_params(model, seed)
    model.eval()
    logits2, logits7 = model(**batch)
    loss = F.cross_entropy(logits2, batch["label"])
    loss.backward()
    sd = model.state_dict()
    shapes = np.full((len(sd), 2), -1, dtype=np.int64)
    for i, v in enumerate(sd.values()):
        shapes[i, :v.dim()] = v.shape
    none = [n for n, q in model.named_parameters() if q.grad is None]
    return dict(param_seed=seed, n_classes=C, dims=np.array([dims["a"], dims["t"], dims["v"]]),
                **{"in_" + k: v.numpy() for k, v in batch.items()},
                logits2=logits2.detach().numpy(), logits7=logits7.detach().numpy(), loss=np.array(float(loss)),
                grad_none=np.array(none), sd_keys=np.array(list(sd)), sd_shapes=shapes,
                **mg.grad_digest([(n, q.grad) for n, q in model.named_parameters()]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(4)
    mg.install_stubs(args.ref)
    for pkg in ("track_mm", "contrib", "models"):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(args.ref, pkg)]
        sys.modules[pkg] = m
    cim = importlib.import_module("track_mm.cim")
    bad = 0
    for name, seed, dims, C, lens in CASES:
        arrays = make_case(cim, name, seed, dims, C, lens)
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
