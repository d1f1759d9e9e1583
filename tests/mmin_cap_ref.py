"""Restatements behind tests/test_mmin_cap_ref.py and tests/test_gpu_mmin_capacity.py: the device collate of an MMIN batch
(csrc/mmin_collate.hip) written in plain torch from its contract in include/ercgraft.h, the small stores and descriptors the
tests share, and the bound of the resident evaluation's accumulated loss.

Collate.  ``desc`` is int32 [3 B_cap]: frames | first frame row | sample index of every slot.  For slot b,
f = clamp(frames_b, 0, T_cap): audio[b, t] = store.audio[first_b + t] for t < f and 0 beyond; a slot with f > 0 copies the
sample's visual and text blocks and its label, an empty one gets zeros and label 0; counts = {#slots with f > 0, max f}.  What
only the device knows is clamped as the header says: first_b to [0, n_frames - f], the sample index to [0, n).

Lall.  The resident evaluation adds each batch's mean cross entropy, a float32 figure, into a float64 accumulator: Lall =
sum over batches of mean_b CE(logits_b, y_b).  Its float64 value comes from the same logits; the float32 twin evaluates each
batch mean in float32 (torch.nn.functional.cross_entropy on the CPU) and adds the batch means in float64.  The bound is
MARGIN = 4 times the twin's own deviation (tests/mmin_ref.py's rule: factor 2 for the order of the sum over the batch, factor 2
for the exponential and logarithm of the device), with one float32 rounding of the result, 2^-24 |Lall|, standing in for the
twin's deviation where the twin happens to land closer than that to the float64 value: every batch mean is rounded to float32
once, by the twin and by the kernel alike, and the batch means are positive, so their roundings add up to at most that.
The figure measured on an MI355X is recorded in FIGURES.
"""
import torch

from erc_amd.datasets import MMINDeviceStore
from erc_amd.synthetic import make_mmin_samples

AUDIO_D, VISUAL_D, TEXT_D = 130, 342, 1024
TV, TT = 50, 22
MARGIN = 4.0

# quantity -> (float32 twin's deviation from float64, bound, measured on an MI355X); tests/test_gpu_mmin_capacity.py prints them
FIGURES = {
    # test_resident_eval_equals_the_host_path: 7 samples in two batches, Lall = 2.75226422; the twin lands within 4e-8, so the
    # rounding unit 2^-24 |Lall| = 1.64e-7 stands in for it
    ("resident_eval", "Lall"): (4e-08, 6.56e-07, 1.95e-07),
}


def small_samples(n, frames, seed=3, split="train", tv=TV, tt=TT):
    """``n`` samples at the real feature widths with ``frames`` = (lo, hi) audio frames, and, to keep a test small, ``tv`` /
    ``tt`` visual / text rows"""
    out = make_mmin_samples(n, split, seed=seed, frames=frames)
    for s in out:
        s["visual_feature"], s["text_feature"] = s["visual_feature"][:tv].copy(), s["text_feature"][:tt].copy()
    return out


def samples_with_frames(frames, seed=3, tv=TV, tt=TT):
    """one sample per entry of ``frames`` (each >= 1), with exactly that many audio frames"""
    out = []
    for i, f in enumerate(frames):
        s = small_samples(1, (f, f), seed=seed + 17 * i, tv=tv, tt=tt)[0]
        s["name"] = "s%03d" % i
        out.append(s)
    return out


def collate_ref(store, desc, B_cap, T_cap):
    """(audio [B_cap, T_cap, 130], visual [B_cap, Tv, 342], text [B_cap, Tt, 1024], label [B_cap] int64, counts [2] int32) on
    the CPU"""
    desc = torch.as_tensor(desc).cpu().to(torch.int64).reshape(3, B_cap)
    sa, sv, st, sl = (t.cpu() for t in (store.audio, store.visual, store.text, store.label))
    n, n_frames = int(sv.shape[0]), int(sa.shape[0])
    audio = torch.zeros(B_cap, T_cap, sa.shape[1])
    visual = torch.zeros((B_cap, ) + tuple(sv.shape[1:]))
    text = torch.zeros((B_cap, ) + tuple(st.shape[1:]))
    label = torch.zeros(B_cap, dtype=torch.int64)
    nb = ta = 0
    for b in range(B_cap):
        f = min(max(int(desc[0, b]), 0), T_cap)
        if f == 0:
            continue
        f_rows = min(f, n_frames)
        first = min(max(int(desc[1, b]), 0), n_frames - f_rows)
        idx = min(max(int(desc[2, b]), 0), n - 1)
        audio[b, :f_rows] = sa[first:first + f_rows]
        visual[b], text[b], label[b] = sv[idx], st[idx], sl[idx]
        nb, ta = nb + 1, max(ta, f)
    return audio, visual, text, label, torch.tensor([nb, ta], dtype=torch.int32)


def host_store(samples):
    return MMINDeviceStore(samples, None)


def lall_reference(logits_per_batch, labels_per_batch):
    """(float64 Lall, float32 twin's Lall, bound) of a list of per-batch logits / labels (CPU tensors)"""
    F = torch.nn.functional
    l64 = sum(float(F.cross_entropy(lg.double(), y)) for lg, y in zip(logits_per_batch, labels_per_batch))
    l32 = sum(float(F.cross_entropy(lg.float(), y)) for lg, y in zip(logits_per_batch, labels_per_batch))
    twin = abs(l32 - l64)
    return l64, l32, MARGIN * max(twin, abs(l64) * 2.0 ** -24)
