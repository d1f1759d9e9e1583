"""Seeded synthetic IEMOCAP-/MELD-shaped dialogues.

There are no dataset pickles in the build or bench environment, so every test
and benchmark runs on dialogues drawn here.  A sample has the schema the
reference's readers produce (mmdatasets/datas/mm/iemocap_feature.py:401 and
meld_feature.py:12-40): per-utterance ``audio``/``text``/``visual`` float32
rows, ``speakers`` as one-hot lists, ``label`` as a list of ints.
"""
import numpy as np


def make_dialogues(n, dims, n_speakers=2, n_classes=6, min_len=20, max_len=110, seed=1,
                   force_max=False, p_switch=0.7):
    """``dims`` = dict(a=, t=, v=).  Lengths uniform in [min_len, max_len];
    speakers switch with probability ``p_switch`` (two-party) or are uniform
    (multi-party); labels uniform.  ``force_max`` pins dialogue 0 at max_len so
    that a bench batch always has T = max_len."""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        L = int(rng.randint(min_len, max_len + 1))
        if force_max and i == 0:
            L = max_len
        if n_speakers == 2:
            flips = rng.rand(L) < p_switch
            spk = np.cumsum(flips) % 2
        else:
            spk = rng.randint(0, n_speakers, size=L)
        onehot = np.eye(n_speakers, dtype=np.int64)[spk]
        out.append({
            "speakers": onehot.tolist(),
            "audio": rng.standard_normal((L, dims["a"])).astype(np.float32),
            "text": rng.standard_normal((L, dims["t"])).astype(np.float32),
            "visual": rng.standard_normal((L, dims["v"])).astype(np.float32),
            "label": rng.randint(0, n_classes, size=L).tolist(),
            "sentence": ["utt %d.%d" % (i, k) for k in range(L)],
        })
    return out


def make_mosei_dialogues(n, dims, min_len=1, max_len=98, seed=1, force_max=False):
    """CMU-MOSEI-shaped videos (the CIM release, datasets.read_mosei_cim): one speaker (``speakers: [0]``), lengths uniform
    in [min_len, max_len] (the release pads to 98), binary sentiment ``label`` = ``senti2_label``, and a 7-column
    multi-hot ``emo_label`` built like the reader's: six emotion columns, and column 6 for a row with none (about one row
    in five here)."""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        L = int(rng.randint(min_len, max_len + 1))
        if force_max and i == 0:
            L = max_len
        emo = np.zeros((L, 7), dtype=np.int64)
        emo[:, :6] = rng.rand(L, 6) < 0.2
        emo[~emo.any(1), 6] = 1
        senti = rng.randint(0, 2, size=L).astype(np.int64)
        out.append({
            "speakers": [0],
            "audio": rng.standard_normal((L, dims["a"])).astype(np.float32),
            "text": rng.standard_normal((L, dims["t"])).astype(np.float32),
            "visual": rng.standard_normal((L, dims["v"])).astype(np.float32),
            "label": senti,
            "emo_label": emo,
            "senti2_label": senti,
        })
    return out


MMIN_SPLIT_SALT = {"train": 0, "val": 1, "test": 2}


def make_mmin_samples(n, split="train", seed=1, frames=(50, 400), n_classes=4, dims=None):
    """Utterance samples in the shapes of the reference's MMIN readers (mmdatasets/datas/mm/iemocap_feature.py:304-357): visual
    [50, 342] (DenseFace frames), text [22, 1024] (BERT token rows), audio [t, 130] (ComParE frames), ``label`` in
    [0, n_classes), ``name``.  The real ComParE frame counts are not known here: ``t`` is drawn uniformly from ``frames``
    (inclusive) -- an ASSUMPTION behind the flag --mmin_frames.  ``split`` (train / val / test) salts the seed, so the three
    splits are disjoint draws; the same (n, split, seed, frames) gives the same samples."""
    dims = dims or dict(a=130, t=1024, v=342)
    rng = np.random.RandomState((seed * 3 + MMIN_SPLIT_SALT[split]) % (1 << 31))
    lo, hi = int(frames[0]), int(frames[1])
    out = []
    for i in range(n):
        t = int(rng.randint(lo, hi + 1))
        out.append({
            "audio_feature": rng.standard_normal((t, dims["a"])).astype(np.float32),
            "visual_feature": rng.standard_normal((50, dims["v"])).astype(np.float32),
            "text_feature": rng.standard_normal((22, dims["t"])).astype(np.float32),
            "label": int(rng.randint(0, n_classes)),
            "name": "%s_%05d" % (split, i),
        })
    return out
