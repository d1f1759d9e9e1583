"""Readers for the feature pickles the reference trains on: per-dialogue sample dicts with the keys
``ERCCollate`` consumes (``speakers, visual, audio, text, label, sentence[, ids]``).

File formats and name table follow the reference (behaviour, not code):
  * IEMOCAP (COGMEN release): a 9-tuple ``(ids, speakers, labels, text, audio, visual, sentence, train_ids, test_ids)`` of
    dicts keyed by dialogue id, ``cogmen/iemocap/IEMOCAP_features.pkl`` (6 classes) or
    ``cogmen/iemocap_4/IEMOCAP_features_4.pkl`` (4 classes); speakers are 'M' / 'F' strings, turned into 2-way one-hots
    (mmdatasets/datas/mm/iemocap_feature.py:360-458).
  * MELD (MMGCN release): the same tuple plus a tenth unused entry, ``MMGCN/MELD_features_raw.pkl``; speakers already
    9-way one-hot lists, features cast to float32 (mmdatasets/datas/mm/meld_feature.py:12-40).
  * optional per-dialogue override maps in the same directory: ``sbert_map.pkl`` / ``robert_map.pkl`` replace the text
    features, ``tsn_vfeat.pkl`` replaces the visual ones or, for the ``v+`` names, is concatenated to them.
  * dataset names ``{corpus}-{release}[-{text}][-{visual}[-v+]]-{n_classes}`` (mmdatasets/datas/__init__.py:33-69); the
    corpus prefix selects the data root (mmdatasets/const.py:9-10, config.py).

  * CMU-MOSEI (CIM release, ``mosei-cim-2``): ``CIM/{text,audio,video}.npz`` with videos padded to a common length;
    every video becomes one "dialogue" of a single speaker (``read_mosei_cim``, after
    mmdatasets/datas/mm/mosei_feature.py:9-126).

Reference quirk kept on purpose: the ``tsnss`` names resolve to ``tsn_vfeat.pkl`` there as well (the 'tsn' substring
test comes first, iemocap_feature.py:383-386), so they do here.

The pickles are the USER's data files (none ship with either repository); they are read with ``pickle`` as the reference
does.  A dialogue store can then be kept resident on the GPU (``DeviceDialogueStore``) so that batches are padded and
concatenated on the device instead of in DataLoader workers.
"""
import os
import pickle

import numpy as np
import torch

from .params import ALL_DATASETS

ROOT_ENV = {"iemocap": "ERC_IEMOCAP_ROOT", "meld": "ERC_MELD_ROOT", "mosei": "ERC_MOSEI_ROOT"}


def data_root(dataset, roots=None):
    """Root directory of a corpus: ``roots[corpus]`` (the reference's config.py mapping) or $ERC_<CORPUS>_ROOT."""
    corpus = dataset.split("-")[0]
    if isinstance(roots, dict) and roots.get(corpus):
        return roots[corpus]
    if isinstance(roots, str) and roots:
        return roots
    env = os.environ.get(ROOT_ENV.get(corpus, ""), "")
    if not env:
        raise FileNotFoundError("no data root for %r: pass --data_root=... or set $%s" % (corpus, ROOT_ENV.get(corpus)))
    return env


def parse_name(dataset):
    """-> dict(corpus, n_classes, text override or '', visual override or '', concat_visual)."""
    if dataset not in ALL_DATASETS:
        raise ValueError("dataset %r not in %s" % (dataset, ALL_DATASETS))
    parts = dataset.split("-")
    mid = parts[2:-1]
    text = next((t for t in ("sbert", "robert") if t in mid), "")
    visual = next((v for v in ("tsnss", "tsn") if v in mid), "")
    return dict(corpus=parts[0], n_classes=int(parts[-1]), text=text, visual=visual, concat_visual="v+" in mid)


def _load(path):
    with open(path, "rb") as fh:
        return pickle.load(fh)


def senti2(a):
    """binary sentiment of mosei_feature.cmumosei_2: 0 below zero, 1 otherwise (NaN included)"""
    return np.where(np.asarray(a) < 0, 0, 1).astype(np.int64)


def senti7(a):
    """7 sentiment bins of mosei_feature.cmumosei_7: [-3,-2) (-2 bin edges closed below) ... 0 alone ... (2, 3]"""
    a = np.asarray(a)
    out = np.select([a < -2, a < -1, a < 0, a == 0, a <= 1, a <= 2, a > 2], [0, 1, 2, 3, 4, 5, 6], -1).astype(np.int64)
    if (out < 0).any():
        raise ValueError("sentiment label %r cannot be binned" % a[out < 0][0])
    return out


def emotion_multi_hot(emo):
    """mosei_feature.create_emotion_label: [L, 7] int64 with a 1 wherever an emotion intensity is nonzero; a row with no
    emotion gets column 6"""
    emo = np.asarray(emo)
    out = np.zeros((emo.shape[0], 7), dtype=np.int64)
    out[:, :emo.shape[1]] = emo != 0
    out[~out.any(1), 6] = 1
    return out


def read_mosei_cim(root, split="train"):
    """Videos of CIM's CMU-MOSEI release as sample dicts: ``ids, length, speakers ([0]), visual, audio, text`` (cut to the
    video's length, float32), ``label`` (= ``senti2_label``), ``emo_label`` [L, 7], ``senti2_label``, ``senti7_label``
    (the binnings of ``*SentiLabel[..., 0]``).  Only 'train' and 'test' exist here: the reference's 'valid' branch takes
    its ids from ``train_idName`` (mosei_feature.py:84-92), so on the real release it indexes past the validation
    arrays; that split is refused rather than reproduced."""
    if split not in ("train", "test"):
        raise ValueError("mosei-cim-2: split %r is not supported (only 'train' and 'test'; the reference's 'val' split "
                         "pairs the validation arrays with the training ids)" % (split, ))
    folder = os.path.join(root, "CIM")
    text, video, audio = (np.load(os.path.join(folder, f + ".npz")) for f in ("text", "video", "audio"))
    lengths, emo, sent = text[split + "_length"], text[split + "EmoLabel"], text[split + "SentiLabel"]
    tdata, vdata, adata, ids = text[split + "_data"], video[split + "_data"], audio[split + "_data"], text[split + "_idName"]
    out = []
    for i in range(len(ids)):
        L = lengths[i]
        s = sent[i][:L, 0]
        s2 = senti2(s)
        out.append({"ids": ids[i], "length": lengths[i], "speakers": [0],
                    "visual": vdata[i][:L].astype(np.float32), "audio": adata[i][:L].astype(np.float32),
                    "text": tdata[i][:L].astype(np.float32), "label": s2, "emo_label": emotion_multi_hot(emo[i][:L]),
                    "senti2_label": s2, "senti7_label": senti7(s)})
    return out


def read_dialogues(dataset, split="train", roots=None):
    """List of per-dialogue sample dicts of ``split`` ('train' | anything else = the test ids; MOSEI: 'train' | 'test'),
    reference order."""
    spec = parse_name(dataset)
    root = data_root(dataset, roots)
    if spec["corpus"] == "mosei":
        return read_mosei_cim(root, split)
    if spec["corpus"] == "iemocap":
        sub = "cogmen/iemocap" if spec["n_classes"] == 6 else "cogmen/iemocap_4"
        main = "IEMOCAP_features.pkl" if spec["n_classes"] == 6 else "IEMOCAP_features_4.pkl"
    else:
        sub, main = "MMGCN", "MELD_features_raw.pkl"
    folder = os.path.join(root, sub)
    tup = _load(os.path.join(folder, main))
    ids, speakers, labels, text, audio, visual, sentence, train_ids, test_ids = tup[:9]
    if spec["text"]:
        text = _load(os.path.join(folder, spec["text"] + "_map.pkl"))
    if spec["visual"] and spec["corpus"] == "iemocap":
        extra = _load(os.path.join(folder, "tsn_vfeat.pkl"))      # also for the tsnss names (see module docstring)
        visual = {k: np.concatenate([visual[k], extra[k]], axis=1) for k in extra} if spec["concat_visual"] else extra
    out = []
    for k in (train_ids if split == "train" else test_ids):
        if spec["corpus"] == "iemocap":
            sample = {"speakers": [[1, 0] if s == "M" else [0, 1] for s in speakers[k]], "visual": visual[k],
                      "audio": audio[k], "text": text[k], "label": labels[k], "sentence": sentence[k]}
            if spec["n_classes"] == 6:
                sample["ids"] = ids[k]
        else:
            sample = {"ids": ids[k], "speakers": speakers[k], "visual": np.asarray(visual[k], dtype=np.float32),
                      "audio": np.asarray(audio[k], dtype=np.float32), "text": np.asarray(text[k], dtype=np.float32),
                      "label": labels[k], "sentence": sentence[k]}
        out.append(sample)
    return out


class DeviceDialogueStore:
    """All dialogues of a split resident in HBM as flat per-modality row stores; ``batch(indices)`` builds the same
    padded batch dict as ``ERCCollate`` with a handful of device gathers (no DataLoader worker, no host copy per step).
    Layout switches follow the params like ERCCollate's (mmbase.py:344-455)."""

    DESC_INTS = 2      # int32 per batch slot of a resident step's descriptor (trainer.batch_table: length | first row)

    def __init__(self, dialogues, params, device, dtype=torch.float32):
        self.params, self.device = params, device
        lens = [len(d["label"]) for d in dialogues]
        self.lengths = torch.tensor(lens, dtype=torch.int64)
        self.t_max = max(lens)      # the longest dialogue
        self.offsets = torch.zeros(len(lens) + 1, dtype=torch.int64)
        self.offsets[1:] = torch.cumsum(self.lengths, 0)
        order = {"t": "text", "a": "audio", "v": "visual"}
        cat = lambda key: torch.from_numpy(np.concatenate([np.asarray(d[key], dtype=np.float32) for d in dialogues], 0))
        self.feats = {m: cat(order[m]).to(device=device, dtype=dtype) for m in params.modality}
        self.fused = torch.cat([self.feats[m] for m in params.modality], dim=1)           # column order = --modality
        # a per-dialogue speakers list of one entry ([0], CMU-MOSEI) broadcasts over the utterances, as in the reference collate
        spk = np.concatenate([np.broadcast_to(np.asarray(d["speakers"], dtype=np.int64).argmax(-1), (n, ))
                              for d, n in zip(dialogues, lens)], 0)
        self.speaker = torch.from_numpy(spk).to(device)
        self.label = torch.from_numpy(np.concatenate([np.asarray(d["label"], dtype=np.int64) for d in dialogues], 0)).to(device)
        # CMU-MOSEI extras (mmbase.py:382-383, 422-425, 450-453): carried only when the samples have them
        self.extra = {}
        for key in ("emo_label", "senti2_label"):
            if dialogues and all(d.get(key) is not None for d in dialogues):
                self.extra[key] = torch.from_numpy(np.concatenate([np.asarray(d[key], dtype=np.int64) for d in dialogues],
                                                                  0)).to(device)
        self.lengths_dev, self.offsets_dev = self.lengths.to(device), self.offsets.to(device)

    def __len__(self):
        return int(self.lengths.numel())

    def batch(self, indices):
        p, dev = self.params, self.device
        idx = torch.as_tensor(indices, dtype=torch.int64)
        lens = self.lengths[idx]
        B, T, N = int(idx.numel()), int(lens.max()), int(lens.sum())
        idx_d = idx.to(dev)
        lens_d = self.lengths_dev[idx_d]
        t = torch.arange(T, device=dev)
        mask = t[None, :] < lens_d[:, None]                                           # [B, T]
        rows = (self.offsets_dev[idx_d][:, None] + t[None, :]).clamp_(max=self.offsets_dev[-1] - 1)
        pad = lambda src: torch.where(mask[..., None], src[rows], torch.zeros((), dtype=src.dtype, device=dev))
        sel = rows[mask]
        out = {"attention_mask": mask.float(), "text_length": lens_d, "label": self.label[sel]}
        for key, v in self.extra.items():
            out[key] = v[sel]
        spk = torch.where(mask, self.speaker[rows], torch.zeros((), dtype=torch.int64, device=dev))
        if p.speaker_onehot:
            spk = torch.nn.functional.one_hot(spk, p.n_speakers).float()   # padded slots: speaker 0, as ERCCollate
        seq = {"input_tensor": pad(self.fused), "speaker_tensor": spk}
        for m, key in (("t", "text_feature"), ("a", "audio_feature"), ("v", "visual_feature")):
            seq[key] = pad(self.feats[m]) if m in p.modality else None
        if not p.batch_first:
            seq = {k: (v.transpose(0, 1).contiguous() if v is not None else None) for k, v in seq.items()}
        out.update(seq)
        assert out["label"].shape[0] == N
        return out


# --------------------------------------------------------------------------------------------- MMIN utterances in HBM
MMIN_T_BUCKET = 64      # audio frame capacities are multiples of this


def mmin_t_cap(ta, t_max):
    """T capacity of a batch whose longest utterance has ``ta`` audio frames: ``ta`` rounded up to a multiple of MMIN_T_BUCKET,
    at most ``t_max`` (the split's longest utterance; 0 or None: no limit)"""
    cap = -(-int(ta) // MMIN_T_BUCKET) * MMIN_T_BUCKET
    return min(cap, int(t_max)) if t_max else cap


class MMINDeviceStore:
    """One split of MMIN utterance samples (synthetic.make_mmin_samples, or the reference readers' dicts) on ``device``: the
    audio frames of all utterances as one ragged matrix ``audio`` [sum t_i, 130] with ``lengths`` / ``offsets`` (host int64, as
    DeviceDialogueStore's), ``visual`` [n, 50, 342], ``text`` [n, 22, 1024], ``label`` [n] int64.  A batch is never
    materialised on the host: ``desc`` gives the 3 B_cap int32 erc_mmin_collate reads (frames | first frame row | sample index,
    empty slots last).  ``device=None`` keeps everything on the host (tests of the tables)."""

    DESC_INTS = 3      # int32 per batch slot of a resident step's descriptor (``desc``)

    def __init__(self, samples, device=None):
        f32 = lambda key: [np.asarray(s[key], dtype=np.float32) for s in samples]
        audio = f32("audio_feature")
        self.device = torch.device("cpu") if device is None else torch.device(device)
        self.lengths = torch.tensor([a.shape[0] for a in audio], dtype=torch.int64)
        self.offsets = torch.zeros(len(audio) + 1, dtype=torch.int64)
        self.offsets[1:] = torch.cumsum(self.lengths, 0)
        self.t_max = int(self.lengths.max()) if len(audio) else 0
        self.audio = torch.from_numpy(np.concatenate(audio, 0)).to(self.device)
        self.visual = torch.from_numpy(np.stack(f32("visual_feature"))).to(self.device)
        self.text = torch.from_numpy(np.stack(f32("text_feature"))).to(self.device)
        self.label = torch.tensor([int(s["label"]) for s in samples], dtype=torch.int64).to(self.device)
        self._lens32, self._offs32 = self.lengths.to(torch.int32).numpy(), self.offsets[:-1].to(torch.int32).numpy()

    def __len__(self):
        return int(self.lengths.numel())

    def desc(self, indices, B_cap):
        """host int32 [3 B_cap] of the batch ``indices`` (at most B_cap of them)"""
        return self.table([list(indices)], B_cap)[0][0]

    def table(self, batches, B_cap):
        """(int32 array [len(batches), 3 B_cap], the batches' T capacities) of an epoch's batches (lists of sample indices)"""
        tab = np.zeros((len(batches), 3, B_cap), dtype=np.int32)
        caps = []
        for row, idx in zip(tab, batches):
            idx = np.asarray(idx, dtype=np.int64)
            if idx.size > B_cap:
                raise ValueError("a batch of %d samples does not fit B_cap=%d" % (idx.size, B_cap))
            row[0, :idx.size], row[1, :idx.size], row[2, :idx.size] = self._lens32[idx], self._offs32[idx], idx
            caps.append(mmin_t_cap(row[0].max(), self.t_max))
        return tab.reshape(len(batches), 3 * B_cap), caps


class MMINMaskedDeviceStore(MMINDeviceStore):
    """the training split of ``--module=mmin_base --train_missing``: the descriptor has a fourth block, the slots' keep bits
    (bit 0 visual, bit 1 text, bit 2 audio: the columns of a MISSING_TYPES row), which erc_mmin_collate_masked reads"""

    DESC_INTS = 4

    def table(self, batches, B_cap, keep=None):
        """(int32 array [len(batches), 4 B_cap], the batches' T capacities); ``keep``: per batch the samples' keep bits (default:
        7, everything kept).  The T capacity follows the frames of all samples, kept or not, as the host path pads first"""
        tab3, caps = super().table(batches, B_cap)
        tab = np.zeros((len(batches), 4, B_cap), dtype=np.int32)
        tab[:, :3] = tab3.reshape(len(batches), 3, B_cap)
        for row, idx, bits in zip(tab, batches, keep if keep is not None else [[7] * len(b) for b in batches]):
            if len(bits) != len(idx):
                raise ValueError("%d keep-bit entries for a batch of %d samples" % (len(bits), len(idx)))
            row[3, :len(idx)] = np.asarray(bits, dtype=np.int32) & 7
        return tab.reshape(len(batches), 4 * B_cap), caps


def index_batches(n, batch_size, shuffle, generator=None):
    """the sample indices of one epoch's batches exactly as ``DataLoader(data, batch_size, shuffle, generator=generator)``
    visits them (it IS a DataLoader, over the indices: same sampler, same draws from ``generator``, a short last batch)"""
    from torch.utils.data import DataLoader
    return [list(b) for b in DataLoader(range(n), batch_size=batch_size, shuffle=shuffle, generator=generator, collate_fn=list)]
