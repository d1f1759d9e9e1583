"""Float64 restatement (and float32 twin) of ``--module=mmin_miss --eval_missing`` (erc_amd/mmin_miss.py; csrc/resae_eval.hip):
a batch's full-modality features expanded into the six missing-modality patterns against the zero-input feature row, netAE's
encoder-only chain, the classifier, the per-pattern scoring.  Written from the math on top of tests/mmin_miss_ref.py; nothing of
the kernels' tiles or buffers.

Math.  MMINMissCollate masks a sample's modality x to x m, m in {0, 1} (mmin_miss.py:328-337), and the encoders run on the zeros.
A sample's encoder output does not depend on the other samples of its batch, so under a pattern the 128 feature columns of a
masked modality are those of an all-zero sample: one row ``zfeat`` per (weights, audio length).  The classifier reads netAE's
latents only, and block i's latent needs the decoders of the blocks before it but not its own, nor the transition.
"""
import torch

from tests import mmin_miss_ref as MR
from tests import mmin_ref as R
from tests.rnn_scan_ref import mm

H, D = 128, 384
KEYS = ("v", "t", "a", "tv", "av", "at")       # the modalities that remain, in MR.MISSING_TYPES' order
WHOLE_PATH_ARGS = ("--n_train=4", "--n_val=5", "--n_test=5", "--train.batch_size=2", "--val.batch_size=2", "--test.batch_size=2",
                   "--mmin_frames=(3,20)")
PARAM_SEEDS = (611, 612)                        # the whole-path test's model weights and EMA weights (MR.named_filled)
MIN_MARGIN = 1e-4                               # top-two logit margin below which a float32 argmax may differ from float64's


def keep_columns(pattern):
    """bool [384]: the feature columns (audio | visual | text) a pattern (visual, text, audio) keeps"""
    v, t, a = (bool(x) for x in pattern)
    return torch.tensor([a] * H + [v] * H + [t] * H)


def zero_features(P, Ta, Tv, Tt, dtype=torch.float64):
    """[384]: the encoders' features of one all-zero sample with Ta audio frames"""
    z = lambda T, d: torch.zeros(1, T, d)
    return MR.encode(P, z(Ta, R.AUDIO_D), z(Tv, R.VISUAL_D), z(Tt, R.TEXT_D), dtype)["features"][0]


def expand(feat, zfeat, patterns=MR.MISSING_TYPES):
    """[len(patterns) B, 384]: row c B + b = feat[b] where pattern c keeps the column's modality, zfeat elsewhere"""
    return torch.cat([torch.where(keep_columns(p), feat, zfeat.expand_as(feat)) for p in patterns])


def latents_chain(P_ae, x, n_blocks, dtype=torch.float64):
    """the latents [B, 64 n_blocks] of MR.resae_fwd without the last block's decoder and the transition"""
    P_ae = [(W.to(dtype), b.to(dtype)) for W, b in P_ae]
    x_in, x_out, latents = x.to(dtype), torch.zeros_like(x, dtype=dtype), []
    for i in range(n_blocks):
        x_in = x_in + x_out
        h = x_in
        for l in range(6 * i, 6 * i + 6):
            y = mm(h, P_ae[l][0].t()) + P_ae[l][1]
            if l % 6 == 2:
                latents.append(y)
                if i == n_blocks - 1:
                    break
            h = MR._act(y, MR.activation_of(l, n_blocks))
        x_out = h
    return torch.cat(latents, -1)


def classifier(P, latents, dtype=torch.float64):
    lin = lambda x, n: mm(x, P[n + ".weight"].to(dtype).t()) + P[n + ".bias"].to(dtype)
    z0 = torch.clamp(lin(latents.to(dtype), "netC.module.0"), min=0)
    return lin(torch.clamp(lin(z0, "netC.module.3"), min=0), "netC.fc_out")


def score(logits, labels, n_cond):
    """(cm int64 [n_cond, C, C] true x predicted, loss float64 [n_cond]) of logits [n_cond B, C]: the first index of the maximum;
    a row with a label outside [0, C) or nothing but NaN is counted nowhere; loss = the mean over the counted rows of
    logsumexp - the label's logit, in float64"""
    C = logits.shape[1]
    B = logits.shape[0] // n_cond
    cm, loss = torch.zeros(n_cond, C, C, dtype=torch.int64), torch.zeros(n_cond, dtype=torch.float64)
    for c in range(n_cond):
        total, n = 0.0, 0
        for b in range(B):
            z, y = logits[c * B + b].double(), int(labels[b])
            if bool(torch.isnan(z).all()) or not 0 <= y < C:
                continue
            mx = z[~torch.isnan(z)].max()
            pred = int((z == mx).nonzero()[0])
            cm[c, y, pred] += 1
            total, n = total + float(torch.logsumexp(z, 0) - z[y]), n + 1
        loss[c] = total / n if n else 0.0
    return cm, loss


def fused_logits(P, batch, dtype=torch.float64, zfeat=None):
    """logits [6, B, C] of a FULL-modality batch under the six patterns by the fused route"""
    feat = MR.encode(P, batch["audio_feature"], batch["visual_feature"], batch["text_feature"], dtype)["features"]
    if zfeat is None:
        zfeat = zero_features(P, *(int(batch[k].shape[1]) for k in ("audio_feature", "visual_feature", "text_feature")), dtype)
    x = expand(feat, zfeat.to(dtype))
    lg = classifier(P, latents_chain(MR._ae_of(P, "netAE"), x, MR.N_BLOCKS, dtype), dtype)
    return lg.reshape(len(MR.MISSING_TYPES), feat.shape[0], -1)


def mask_batch(batch, pattern):
    """the batch as MMINMissCollate hands it over when every sample has ``pattern`` (visual, text, audio)"""
    B = int(batch["label"].shape[0])
    return MR.apply_missing(batch, torch.tensor([list(pattern)] * B, dtype=torch.long))


def whole_path_params():
    from track_mm.mmin_miss import MMINMissParams
    return MMINMissParams().from_args(list(WHOLE_PATH_ARGS))


def whole_path_batches(split):
    """the collated val / test batches of the whole-path test: 5 synthetic utterances in batches of 2, 2, 1"""
    from erc_amd.mmin_miss import MMINMissTrainer
    loaders = MMINMissTrainer.make_loaders(whole_path_params())
    return list(loaders[{"val": 1, "test": 2}[split]])


def whole_path_weights(k):
    """state_dict of pass k (0: the model, 1: the EMA copy)"""
    return MR.named_filled(MR.sd_shapes(), PARAM_SEEDS[k])


_WHOLE = {}


def whole_path_reference(split, k):
    """per batch of ``split`` under weights k: (float64 logits [6, B, C], the float32 twin's); computed once, never modified"""
    if (split, k) not in _WHOLE:
        P, out, zf = whole_path_weights(k), [], {}
        with R.one_thread():
            for b in whole_path_batches(split):
                Ta = int(b["audio_feature"].shape[1])
                if Ta not in zf:
                    zf[Ta] = tuple(zero_features(P, Ta, int(b["visual_feature"].shape[1]), int(b["text_feature"].shape[1]), dt)
                                   for dt in (torch.float64, torch.float32))
                out.append((fused_logits(P, b, torch.float64, zf[Ta][0]), fused_logits(P, b, torch.float32, zf[Ta][1])))
        _WHOLE[split, k] = out
    return _WHOLE[split, k]
