#!/usr/bin/env python3
"""Golden vectors of CIM on CMU-MOSEI (``--dataset=mosei-cim-2``) from the REFERENCE's own code on CPU, with the stubs and
helpers of make_golden.py.  Run here, never on the GPU box (the reference tree is not there):

    python tests/golden/make_golden_cim_mosei.py [--ref /root/reference] [--check]

(a) a tiny CIM release under tests/golden/mosei_cim/CIM/{text,audio,video}.npz (videos padded to 98; lengths 1 and 98,
    rows without emotion, sentiment exactly 0 and on every bin edge) and, in mosei_cim_reader.npz, what the reference's
    mosei_feature.mosei_cim returns for 'train' and 'test' (key ``<split>_<video>_<sample key>``);
(b) cim_mosei_c2.npz: the reference's CIMModule at MOSEI dims (a 74, t 300, v 35), C = 2, eval mode, on ragged lengths
    including 1 -- logits2 / logits7, Lce, Lmulti, Lall = Lce + Lmulti (cim.py:202-213 with apply_multi and apply_bin), the
    gradient digest of every parameter and the names of those without one (rnn_adapter.* only).

``--check`` regenerates everything in memory and compares it with the committed files (exit 1 on any mismatch).
"""
import argparse
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

DATA = os.path.join(HERE, "mosei_cim")
PAD = 98
DIMS = dict(t=300, a=74, v=35)
# sentiment values on every bin edge of cmumosei_7 / cmumosei_2, exactly 0 (and -0), and inside every bin
EDGES = np.array([-3.0, -2.0, -1.0, 0.0, -0.0, 1.0, 2.0, 3.0, -2.5, -1.5, -0.4, 0.6, 1.4, 2.7], dtype=np.float64)
SPLITS = {"train": (1, 98, 6), "valid": (4, ), "test": (14, 3)}


def release_arrays(seed=5):
    """{file: {key: array}} of the tiny release"""
    rng = np.random.RandomState(seed)
    text, audio, video = {}, {}, {}
    for split, lens in SPLITS.items():
        n = len(lens)
        emo = np.zeros((n, PAD, 6), dtype=np.float64)
        sent = np.zeros((n, PAD, 1), dtype=np.float64)
        for i, L in enumerate(lens):
            e = rng.choice([0.0, 0.0, 0.0, 1 / 3, 2 / 3, 1.0], size=(L, 6))
            e[::3] = 0.0                                              # rows with no emotion -> column 6
            emo[i, :L] = e
            sent[i, :L, 0] = np.resize(np.roll(EDGES, i), L) if L > 1 else EDGES[3]
        for store, key, d in ((text, "t", DIMS["t"]), (audio, "a", DIMS["a"]), (video, "v", DIMS["v"])):
            x = np.zeros((n, PAD, d), dtype=np.float64)
            for i, L in enumerate(lens):
                x[i, :L] = np.round(rng.standard_normal((L, d)), 3)
            store[split + "_data"] = x
        text[split + "_length"] = np.array(lens, dtype=np.int64)
        text[split + "EmoLabel"] = emo
        text[split + "SentiLabel"] = sent
        text[split + "_idName"] = np.array(["%s_video%d" % (split, i) for i in range(n)])
    return {"text": text, "audio": audio, "video": video}


def reader_arrays(mosei_feature):
    out = {}
    for split in ("train", "test"):
        for i, s in enumerate(mosei_feature.mosei_cim(HERE + "/mosei_cim", split)):
            for k, v in s.items():
                out["%s_%d_%s" % (split, i, k)] = np.asarray(v)
    return out


def model_case(cim, seed=41, lens=(6, 1, 13, 4)):
    import torch.nn.functional as F
    C = 2
    g = torch.Generator().manual_seed(seed + 1000)
    B, T, N = len(lens), max(lens), sum(lens)
    batch = {"text_length": torch.tensor(lens, dtype=torch.int64),
             "attention_mask": (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float()}
    for m, key in (("a", "audio_feature"), ("t", "text_feature"), ("v", "visual_feature")):
        x = torch.randn(B, T, DIMS[m], generator=g) * 0.5
        for b, L in enumerate(lens):
            x[b, L:] = 0.0
        batch[key] = x
    batch["label"] = torch.randint(0, C, (N,), generator=g)
    emo = (torch.rand(N, 7, generator=g) < 0.25).long()
    emo[:, 6] = 0
    emo[::4] = 0
    emo[(emo.sum(1) == 0), 6] = 1
    batch["emo_label"] = emo
    model = cim.CIMModule(text_dim=DIMS["t"], audio_dim=DIMS["a"], visual_dim=DIMS["v"], hidden_size=200, n_classes=C)
    mg.fill_params(model, seed)
    model.eval()
    logits2, logits7 = model(**batch)
    lce = F.cross_entropy(logits2, batch["label"])
    lmulti = F.binary_cross_entropy_with_logits(logits7, batch["emo_label"].float())
    lall = lce + lmulti
    lall.backward()
    none = [n for n, q in model.named_parameters() if q.grad is None]
    return dict(param_seed=seed, n_classes=C, dims=np.array([DIMS["a"], DIMS["t"], DIMS["v"]]),
                **{"in_" + k: v.numpy() for k, v in batch.items()},
                logits2=logits2.detach().numpy(), logits7=logits7.detach().numpy(), Lce=np.array(lce.item()),
                Lmulti=np.array(lmulti.item()), Lall=np.array(lall.item()), grad_none=np.array(none),
                **mg.grad_digest([(n, q.grad) for n, q in model.named_parameters()]))


def compare(name, old, arrays):
    bad = 0
    for k, v in arrays.items():
        v = np.asarray(v)
        if k not in old.files or old[k].dtype != v.dtype or old[k].shape != v.shape or not np.array_equal(old[k], v):
            print("mismatch %s:%s" % (name, k))
            bad += 1
    extra = set(old.files) - set(arrays)
    for k in sorted(extra):
        print("stale %s:%s" % (name, k))
    return bad + len(extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(4)
    mg.install_stubs(args.ref)
    utils = types.ModuleType("lumo.utils")
    utils.safe_io = types.ModuleType("lumo.utils.safe_io")
    sys.modules["lumo.utils"], sys.modules["lumo.utils.safe_io"] = utils, utils.safe_io
    spec = importlib.util.spec_from_file_location("ref_mosei_feature",
                                                  os.path.join(args.ref, "mmdatasets/datas/mm/mosei_feature.py"))
    mosei_feature = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mosei_feature)
    for pkg in ("track_mm", "contrib", "models"):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(args.ref, pkg)]
        sys.modules[pkg] = m
    cim = importlib.import_module("track_mm.cim")

    bad = 0
    release = release_arrays()
    for f, arrays in release.items():
        path = os.path.join(DATA, "CIM", f + ".npz")
        if args.check:
            with np.load(path, allow_pickle=False) as old:
                bad += compare("mosei_cim/CIM/" + f, old, arrays)
        else:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            np.savez_compressed(path, **arrays)
            print("wrote mosei_cim/CIM/%s.npz %7.1f KB" % (f, os.path.getsize(path) / 1024))
    for name, arrays in (("mosei_cim_reader", reader_arrays(mosei_feature)), ("cim_mosei_c2", model_case(cim))):
        if args.check:
            bad += compare(name, np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False), arrays)
        else:
            mg.save(name, **arrays)
    if args.check:
        print("%d mismatches" % bad)
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
