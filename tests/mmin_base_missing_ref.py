"""Float64 restatement (and float32 twin) of ``--module=mmin_base --eval_missing`` and the torch restatement of the masked device
collate of ``--train_missing`` (erc_amd/mmin.py; csrc/resae_eval.hip, csrc/lstm128.hip, csrc/mmin_collate.hip).  Written from the
math on top of tests/mmin_ref.py, tests/mmin_eval_missing_ref.py and tests/mmin_cap_ref.py; nothing of the kernels' tiles.

Fused route.  MMINMissCollate masks a sample's modality x to x m, m in {0, 1}, and the encoders run on the zeros; an encoder's
output for a sample does not depend on the rest of its batch.  Under a pattern the 128 feature columns of a masked modality are
therefore those of an all-zero sample, and the base model's classifier reads the 384 features directly (no autoencoder):

    logits[c] = netC(where(keep_c, features(batch), zfeat(Ta)))          c over the six patterns

Prefix-maximum table.  The audio encoder on zero frames is one trajectory h_0, h_1, .. that depends on the weights alone, and the
feature at a padded length of Ta frames is max(h_0 .. h_{Ta-1}).  One scan over t_max + 1 zero frames saves Hprev[t] = h_{t-1};
table[Ta] = max over rows 1 .. Ta of Hprev, table[0] unused (zero).

Logits bound.  LOGITS_MARGIN = 4 times the float32 twin's worst deviation from float64 over the cases (relative to the largest
float64 logit of the case; at least one float32 rounding): the factor covers the GEMMs' other summation order.  The figure is
recorded in FIGURES.

Masked collate.  tests/mmin_cap_ref.collate_ref with a fourth descriptor block of keep bits (bit 0 visual, bit 1 text, bit 2
audio): a modality whose bit is clear is zeros; label and counts do not look at the bits.
"""
import torch

from tests import mmin_cap_ref as CR
from tests import mmin_eval_missing_ref as ER
from tests import mmin_miss_ref as MR
from tests import mmin_ref as R

H = 128
TV, TT = 5, 6                                    # visual / text rows of the small stores (the feature widths are the real ones)
KEYS = ER.KEYS
MIN_MARGIN = ER.MIN_MARGIN                       # 1e-4: the project's top-two margin
LOGITS_MARGIN = 4.0
PARAM_SEEDS = (731, 733)                         # the whole-path test's model weights and EMA weights (MR.named_filled)
# the default-loop test: 5 utterances in batches of 2, 2, 1 -> padded audio lengths 7, 16, 2
WHOLE_FRAMES, WHOLE_SEED, WHOLE_BATCH = (7, 4, 16, 9, 2), 5, 2
T_MAX_TABLE, TABLE_TA = 16, (1, 2, 7, 16)

# quantity -> (float32 twin's worst deviation from float64, bound, measured on an MI355X)
FIGURES = {
    ("eval_missing", "logits"): (1.86e-07, 7.44e-07, 3.11e-07),
}


def whole_samples():
    return CR.samples_with_frames(WHOLE_FRAMES, seed=WHOLE_SEED, tv=TV, tt=TT)


def whole_batches():
    """the collated batches of the default-loop test (host tensors)"""
    from torch.utils.data import DataLoader
    from erc_amd.mmin import mmin_collate
    return list(DataLoader(whole_samples(), batch_size=WHOLE_BATCH, shuffle=False, collate_fn=mmin_collate))


def whole_weights(k):
    """state_dict of pass k (0: the model, 1: the EMA copy)"""
    return MR.named_filled(R.SD_SHAPES, PARAM_SEEDS[k])


def prefix_table(P, t_max, dtype=torch.float64):
    """[t_max + 1, 128]: row Ta = the audio encoder's max-pool over Ta zero frames, from ONE scan over t_max + 1 zero frames"""
    names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    f = R.lstm_pool_fwd(torch.zeros(1, t_max + 1, R.AUDIO_D), *(P["netA.rnn." + n] for n in names), dtype=dtype)
    hp = f["Hprev"][0]                                   # row t = h_{t-1}
    return torch.cat([torch.zeros(1, H, dtype=dtype), torch.cummax(hp[1:], 0).values])


def zero_vt(P, Tv, Tt, dtype=torch.float64):
    """[256]: the visual | text features of an all-zero sample"""
    return ER.zero_features(P, 1, Tv, Tt, dtype)[H:]


def fused_logits(P, batch, dtype=torch.float64, table=None, zvt=None):
    """logits [6, B, C] of a FULL-modality batch under the six patterns by the fused route of ``mmin_base``: expand, classifier"""
    a, v, t = (batch[k] for k in ("audio_feature", "visual_feature", "text_feature"))
    feat = MR.encode(P, a, v, t, dtype)["features"]
    Ta = int(a.shape[1])
    if table is None:
        zfeat = ER.zero_features(P, Ta, int(v.shape[1]), int(t.shape[1]), dtype)
    else:
        zfeat = torch.cat([table[Ta], zvt]).to(dtype)
    lg = ER.classifier(P, ER.expand(feat, zfeat), dtype)
    return lg.reshape(len(MR.MISSING_TYPES), feat.shape[0], -1)


def naive_logits(P, batch, dtype=torch.float64):
    """the same by the whole-model restatement (tests/mmin_ref.py) on host-masked inputs: six forwards"""
    return torch.stack([R.model_forward(P, ER.mask_batch(batch, p), dtype)["logits"] for p in MR.MISSING_TYPES])


_WHOLE = {}


def whole_reference(k):
    """per batch of the default-loop test under weights k: (float64 logits [6, B, C], the float32 twin's), both through the
    prefix-maximum table; computed once, never modified"""
    if k not in _WHOLE:
        P, out = whole_weights(k), []
        with R.one_thread():
            tabs = [(prefix_table(P, max(WHOLE_FRAMES), dt), zero_vt(P, TV, TT, dt)) for dt in (torch.float64, torch.float32)]
            for b in whole_batches():
                out.append(tuple(fused_logits(P, b, dt, *tab) for dt, tab in zip((torch.float64, torch.float32), tabs)))
        _WHOLE[k] = out
    return _WHOLE[k]


def twin_deviation():
    """the float32 twin's worst deviation from float64 over the cases, relative to the case's largest float64 logit"""
    return max(R.rel(f32, f64) for k in (0, 1) for f64, f32 in whole_reference(k))


def logits_bound():
    return LOGITS_MARGIN * max(twin_deviation(), R.FLOOR)


def top_two_margin(logits):
    """the smallest gap between the largest and the second largest logit over all rows"""
    top = logits.reshape(-1, logits.shape[-1]).topk(2, -1).values
    return float((top[:, 0] - top[:, 1]).min())


# ------------------------------------------------------------------------------------------------------------ masked collate
def keep_bits(pattern):
    """a MISSING_TYPES row (visual, text, audio) as the descriptor's keep bits"""
    v, t, a = pattern
    return int(v) | int(t) << 1 | int(a) << 2


def collate_masked_ref(store, desc, B_cap, T_cap):
    """tests/mmin_cap_ref.collate_ref of the first three descriptor blocks, then every slot's modalities whose keep bit (fourth
    block, masked to 3 bits) is clear set to zero; label and counts as they were"""
    desc = torch.as_tensor(desc).cpu().to(torch.int64).reshape(4, B_cap)
    audio, visual, text, label, counts = CR.collate_ref(store, desc[:3].reshape(-1), B_cap, T_cap)
    for b in range(B_cap):
        bits = int(desc[3, b]) & 7
        for x, bit in ((visual, 0), (text, 1), (audio, 2)):
            if not (bits >> bit) & 1:
                x[b] = 0.0
    return audio, visual, text, label, counts


def masked_rows(desc, B_cap):
    """bool [B_cap] per modality (audio, visual, text): the slots whose rows the kernel writes as zeros without reading the store"""
    bits = torch.as_tensor(desc).cpu().to(torch.int64).reshape(4, B_cap)[3] & 7
    return ((bits >> 2) & 1) == 0, (bits & 1) == 0, ((bits >> 1) & 1) == 0
