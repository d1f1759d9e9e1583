#!/usr/bin/env python3
"""Golden vectors of MMIN's missing-modality model from the REFERENCE's own classes on CPU fp32.  Run where the reference tree
is, never on the GPU box:

    python tests/golden/make_golden_mmin_miss.py --ref <reference checkout> [--check]

``--check`` regenerates every fixture in memory and compares it with the committed file (exit 1 on any mismatch).

track_mm/mmin_miss.py itself imports lumo (which needs ``fire``), so track_mm/mmin_models.py is loaded alone, as
make_golden_mmin.py does, and its TextCNN, LSTMEncoder, ResidualAE, Classifier and MMINBaseModule are arranged here the way
mmin_miss.py:68-107 (the module) and :196-210 (the training step's losses) arrange them.  Eval mode (dropout off) for both
models; parameters by seed through ``make_golden.fill_params`` (not stored); a ``missing_type`` per sample that covers all six
patterns; inputs masked as MMINMissCollate masks them (:328-337).  Recorded: the full-modality inputs and missing_type, logits,
fusion, fusion_cycle, features, the pretrained model's features of the reverse inputs, Lce / Lmse / Lcycle / Lall, the gradient
digest (tests/mmin_miss_ref.py ``digest``) and norm of every parameter of ``model``, and its state_dict keys and shapes.
"""
import argparse
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402
from make_golden_mmin import load_models  # noqa: E402
from tests import mmin_miss_ref as MR  # noqa: E402


def miss_module(mm, n_classes=4):
    """MMINMissModule (mmin_miss.py:68-107) from the reference's building blocks, same attribute names and creation order"""
    class MMINMissModule(nn.Module):
        def __init__(self):
            super().__init__()
            self.netL = mm.TextCNN(1024, 128)
            self.netA = mm.LSTMEncoder(130, 128, embd_method="maxpool")
            self.netV = mm.LSTMEncoder(342, 128, embd_method="maxpool")
            self.netAE = mm.ResidualAE([256, 128, 64], 5, 384, dropout=0, use_bn=False)
            self.netAE_cycle = mm.ResidualAE([256, 128, 64], 5, 384, dropout=0, use_bn=False)
            self.netC = mm.Classifier(64 * 5, [128, 128], n_classes, dropout=0.3, use_bn=False)

        def forward(self, audio_feature, visual_feature, text_feature):
            features = torch.cat([self.netA(audio_feature), self.netV(visual_feature), self.netL(text_feature)], dim=-1)
            fusion, latent = self.netAE(features)
            fusion_cycle, _ = self.netAE_cycle(features)
            logits, _ = self.netC(latent)
            return logits, fusion, fusion_cycle, features
    return MMINMissModule()


def make_case(mm, name):
    seed, seed_pre, _ = MR.MODEL_SEEDS[name]
    full, missing_type = MR.make_batch(name)
    batch = MR.apply_missing(full, missing_type)
    model = miss_module(mm)
    mg.fill_params(model, seed)
    pre = mm.MMINBaseModule(visual_dim=342, text_dim=1024, audio_dim=130, n_classes=4)
    mg.fill_params(pre, seed_pre)
    model.eval(), pre.eval()
    logits, fusion, fusion_cycle, features = model(batch["audio_feature"], batch["visual_feature"], batch["text_feature"])
    reverse = torch.cat(pre.encode(audio_feature=batch["audio_feature_reverse"], visual_feature=batch["visual_feature_reverse"],
                                   text_feature=batch["text_feature_reverse"]), dim=-1)
    F = torch.nn.functional
    Lce, Lmse, Lcycle = F.cross_entropy(logits, full["label"]), F.mse_loss(reverse, fusion), F.mse_loss(features, fusion_cycle)
    Lall = Lce + Lmse * 4 + Lcycle * 2
    Lall.backward()
    sd = model.state_dict()
    shapes = np.full((len(sd), 4), -1, dtype=np.int64)
    for i, v in enumerate(sd.values()):
        shapes[i, :v.dim()] = v.shape
    none = [n for n, q in model.named_parameters() if q.grad is None]
    t = lambda v: v.detach().numpy()
    return dict(param_seed=seed, pretrained_seed=seed_pre, n_params=np.array(sum(p.numel() for p in model.parameters())),
                **{"in_" + k: v.numpy() for k, v in full.items()}, missing_type=missing_type.numpy(),
                logits=t(logits), fusion=t(fusion), fusion_cycle=t(fusion_cycle), features=t(features), reverse_features=t(reverse),
                Lce=t(Lce), Lmse=t(Lmse), Lcycle=t(Lcycle), Lall=t(Lall),
                grad_none=np.array(none, dtype="U1"), sd_keys=np.array(list(sd)), sd_shapes=shapes,
                **{"gd__" + n.replace(".", "__"): MR.digest(q.grad).numpy() for n, q in model.named_parameters()},
                **{"gnorm__" + n.replace(".", "__"): np.array(float(q.grad.double().norm())) for n, q in model.named_parameters()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(1)
    mm = load_models(args.ref)
    bad = 0
    for name in MR.MODEL_CASES:
        arrays = make_case(mm, name)
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
