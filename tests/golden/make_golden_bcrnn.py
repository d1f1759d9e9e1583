#!/usr/bin/env python3
"""Golden vectors of the bc-LSTM and bc-GRU baselines (track_mm/dgcnv2_models.py:389-425 LSTMModel, :350-386 GRUModel, with
the loss MaskedNLLLoss :13-33) from the REFERENCE's own classes on CPU fp32, with the stubs and loaders of make_golden.py and
make_golden_dgcnv2.py.  Run here, never on the GPU box (the reference tree is not there):

    python tests/golden/make_golden_bcrnn.py [--ref /root/reference] [--check]

``--check`` regenerates every fixture in memory and compares it with the committed file (exit 1 on any mismatch).

The reference runs as it stands (no patch beyond those make_golden_dgcnv2.py applies to load its module).  Eval mode
(dropout off): LSTMModel / GRUModel(D, 100, 100) on a time-major batch, att2=True, mask = the attention mask; the valid rows
of its log-probabilities and of ``emotions`` in dialogue-major order, the MaskedNLLLoss over the padded rows, the gradient
digest of every parameter, the names of parameters whose grad stays None (there are none) and the state_dict key list with
shapes.
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
import make_golden_dgcnv2 as mg2  # noqa: E402

# (name, model class, param seed, feature dim, speakers, classes, loss weights, dialogue lengths)
CASES = (("bclstm_s2", "LSTMModel", 71, 48, 2, 6, True, (9, 1, 23, 14)),
         ("bclstm_s9", "LSTMModel", 72, 40, 9, 7, False, (17, 6, 30)),
         ("bcgru_s2", "GRUModel", 73, 48, 2, 6, True, (9, 1, 23, 14)),
         ("bcgru_s9", "GRUModel", 74, 40, 9, 7, False, (17, 6, 30)))


def make_case(dm, cls, seed, D, S, C, weighted, lens):
    batch = mg2.make_batch(D, S, C, lens, seed)
    model = getattr(dm, cls)(D, 100, 100, n_classes=C)
    mg.fill_params(model, seed)
    model.eval()
    umask = batch["attention_mask"]                                   # [B, T]
    log_prob, _, _, _, emotions = model(batch["input_tensor"], batch["speaker_tensor"], umask)
    T, B = log_prob.shape[0], log_prob.shape[1]
    valid = umask.bool()
    # padded rows in the batch-major order MaskedNLLLoss expects (pred: batch*seq_len rows)
    pred = log_prob.transpose(0, 1).contiguous().view(B * T, C)
    target = torch.zeros(B, T, dtype=torch.int64)
    target[valid] = batch["label"]
    w = torch.tensor(mg2.IEMOCAP6_WEIGHTS) if weighted else None
    loss = dm.MaskedNLLLoss(w)(pred, target.view(-1), umask)
    loss.backward()
    sd = model.state_dict()
    shapes = np.full((len(sd), 3), -1, dtype=np.int64)
    for i, v in enumerate(sd.values()):
        shapes[i, :v.dim()] = v.shape
    none = [n for n, q in model.named_parameters() if q.grad is None]
    return dict(param_seed=seed, n_speakers=S, n_classes=C, loss_weights=np.array(weighted),
                **{"in_" + k: v.numpy() for k, v in batch.items()},
                log_prob=log_prob.detach().transpose(0, 1)[valid].numpy(),
                emotions=emotions.detach().transpose(0, 1)[valid].numpy(), loss=np.array(float(loss.detach())),
                grad_none=np.array(none, dtype="U1"), sd_keys=np.array(list(sd)), sd_shapes=shapes,
                **mg.grad_digest([(n, q.grad) for n, q in model.named_parameters()]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(1)
    mg.install_stubs(args.ref)
    sys.modules["torch_geometric.nn"].GraphConv = mg2._GraphConv
    for pkg in ("track_mm", "contrib", "models"):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(args.ref, pkg)]
        sys.modules[pkg] = m
    dm = mg2.load_models(args.ref)
    importlib.import_module("track_mm.dgcnv2_models")
    bad = 0
    for name, *case in CASES:
        arrays = make_case(dm, *case)
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
