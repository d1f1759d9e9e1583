#!/usr/bin/env python3
"""Golden vectors of MMIN's full-modality base model (track_mm/mmin_models.py:202-240 MMINBaseModule, with the mean cross
entropy of track_mm/mmin_base.py:131) from the REFERENCE's own class on CPU fp32.  Run here, never on the GPU box (the reference
tree is not there):

    python tests/golden/make_golden_mmin.py [--ref /root/reference] [--check]

``--check`` regenerates every fixture in memory and compares it with the committed file (exit 1 on any mismatch).

The reference's model file imports only torch and runs as it stands.  Eval mode (dropout off): MMINBaseModule(342, 1024, 130, 4)
with ``make_golden.fill_params(model, seed)`` (the 2 M parameters are not stored) on a batch-first batch whose audio is
zero-padded as MMINBaseCollate pads it: logits, ``feat``, the three encoder outputs, the loss, the gradient digest of every
parameter, the names of parameters whose grad stays None (there are none) and the state_dict key list with shapes.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402
from tests.mmin_ref import make_batch  # noqa: E402

# (name, parameter seed, batch seed): shapes in tests/mmin_ref.py model_case
CASES = (("mmin_base_a", 81, 181),       # B = 5, audio T 13 padded from 13/4/1/9/13, visual T 6, text T 7
         ("mmin_base_b2", 82, 182))      # B = 2 (--debug), audio T 9, visual T 50, text T 22: the real visual / text shapes


def load_models(ref):
    spec = importlib.util.spec_from_file_location("mmin_models_ref", os.path.join(ref, "track_mm", "mmin_models.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_case(mm, name, seed, batch_seed):
    batch = make_batch(name, batch_seed)
    model = mm.MMINBaseModule(visual_dim=342, text_dim=1024, audio_dim=130, n_classes=4)
    mg.fill_params(model, seed)
    model.eval()
    inputs = {k: batch[k] for k in ("audio_feature", "visual_feature", "text_feature")}
    audio, visual, text = model.encode(**inputs)
    logits, feat = model(**inputs, audio_feature_length=batch["audio_feature_length"])
    loss = torch.nn.functional.cross_entropy(logits, batch["label"])
    loss.backward()
    sd = model.state_dict()
    shapes = np.full((len(sd), 4), -1, dtype=np.int64)
    for i, v in enumerate(sd.values()):
        shapes[i, :v.dim()] = v.shape
    none = [n for n, q in model.named_parameters() if q.grad is None]
    return dict(param_seed=seed, n_params=np.array(sum(p.numel() for p in model.parameters())),
                **{"in_" + k: v.numpy() for k, v in batch.items()},
                logits=logits.detach().numpy(), feat=feat.detach().numpy(), audio=audio.detach().numpy(),
                visual=visual.detach().numpy(), text=text.detach().numpy(), loss=np.array(float(loss.detach())),
                grad_none=np.array(none, dtype="U1"), sd_keys=np.array(list(sd)), sd_shapes=shapes,
                **mg.grad_digest([(n, q.grad) for n, q in model.named_parameters()]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(1)
    mm = load_models(args.ref)
    bad = 0
    for name, *case in CASES:
        arrays = make_case(mm, name, *case)
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
