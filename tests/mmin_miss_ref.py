"""Float64 restatements of MMIN's missing-modality model (erc_amd/mmin_miss.py; csrc/resae.hip), their float32 twins, the case
table and the bounds of tests/test_mmin_miss_ref.py and tests/test_gpu_mmin_miss.py.  Written from the math, in plain torch on the
CPU; nothing of the kernels' tiles, buffers or scratch layout.

Math.  A residual autoencoder of n blocks over x [B, 384] is the chain of 6 n + 2 affine layers y_l = a_l W_l^T + b_l
(``chain order``: per block the encoder 384 -> 256 -> 128 -> 64 and the decoder 64 -> 128 -> 256 -> 384, then the transition
384 -> 384 -> 384) with
    x_in_0 = x,  x_in_i = x_in_{i-1} + x_out_{i-1},  x_out_i = decoder_i(encoder_i(x_in_i)),
    LeakyReLU(0.01) behind the encoder's first two layers, ReLU behind the decoder's first two, nothing behind the third of
    either (the encoder's third output is the block's latent), recon = T_2 relu(T_0 (x_in_{n-1} + x_out_{n-1})).
Backward in closed form: with G the gradient wrt x_in of the block at hand (G = dY_{T0} T_0 behind the transition),
    dY_{d2} = G;  every other dY_l = mask_l (dY_{l+1} W_{l+1}) (+ d_latents behind the encoder's third layer);
    G <- G + dY_{e0} W_{e0} (x_in_i feeds the encoder AND, through the sum, everything behind the block);  dx = G after block 0;
    dW_l = dY_l^T a_l,  db_l = column sums of dY_l.
The masks are an INPUT of the backward: a pre-activation within rounding of 0 may fall on either side in two correct float32
evaluations, so a backward is compared on the masks the kernel itself saved (as ``arg`` for the scans, tests/mmin_ref.py).

Float32 twins: the same functions with dtype=float32 on tests/rnn_scan_ref.py's ``ops`` (products from elementwise float32
multiplies and adds in a fixed tree), so a twin's figure does not depend on the machine's math libraries.

Bounds: round_up_1(MARGIN x max(the twin's deviation from float64, FLOOR)), MARGIN = 4, FLOOR = 2^-24, errors relative to the
quantity's largest float64 magnitude (mmin_ref.twin_bound: the rule and its reasons are stated there).  A kernel's measured
figure never enters a bound; the figures measured on an MI355X are recorded in FIGURES next to the twin's.
"""
import math
import zlib

import torch

from tests import mmin_ref as R
from tests.mmin_ref import FLOOR, MARGIN, twin_bound  # noqa: F401
from tests.rnn_scan_ref import mm, one_thread, ops, rel  # noqa: F401

D, LAYERS, LAT1 = 384, (256, 128, 64), 64
SLOPE = 0.01
N_BLOCKS = 5
W_MSE, W_CYCLE = 4.0, 2.0
MISSING_TYPES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1))      # columns visual, text, audio
MODAL_KEYS = ("visual_feature", "text_feature", "audio_feature")

# name -> (B list, n_blocks, jobs, decoder bias override); R = erc_resae_rows_per_group() is filled in by the GPU test
AE_CASES = {
    "a": (("1", ), 1, 1, None),                    # first block's x_out = 0, a single row
    "b": (("R-1", "R", "R+1"), 2, 1, None),        # the row guard on both sides of a group; residual gradient across blocks
    "c": (("5", ), 5, 2, None),                    # the model's own form: two jobs, wide pitches, d_latents = NULL on job 1
    "d": (("33", ), 5, 2, None),                   # more than 32 rows
    "e": (("4", ), 2, 1, -10.0),                   # every decoder bias -10: ReLU-dead
}

# Figures: max error relative to the quantity's largest float64 magnitude, per (family, case, quantity): (the float32 twin
# against float64 -- this file, any machine; the bound derived from it; the kernel against float64, measured on an MI355X --
# tests/test_gpu_mmin_miss.py prints the live values).  Per-layer quantities are recorded by their worst layer.  A record: the
# tests derive every bound from the twin at run time and never read the third column.
FIGURES = {
    ("resae", "a/B1/job0", "recon"): (1.651e-07, 7e-07, 1.93e-07),
    ("resae", "a/B1/job0", "latents"): (1.748e-07, 7e-07, 1.48e-07),
    ("resae", "a/B1/job0", "acts"): (1.748e-07, 7e-07, 1.48e-07),
    ("resae", "a/B1/job0", "dx"): (1.377e-07, 6e-07, 2.40e-07),
    ("resae", "a/B1/job0", "dY"): (3.048e-07, 2e-06, 5.72e-07),
    ("resae", "a/B1/job0", "dW"): (3.150e-07, 2e-06, 6.24e-07),
    ("resae", "a/B1/job0", "db"): (3.048e-07, 2e-06, 5.72e-07),
    ("resae", "b/B15/job0", "recon"): (1.787e-07, 8e-07, 1.71e-07),
    ("resae", "b/B15/job0", "latents"): (1.516e-07, 7e-07, 2.21e-07),
    ("resae", "b/B15/job0", "acts"): (2.215e-07, 9e-07, 2.45e-07),
    ("resae", "b/B15/job0", "dx"): (1.961e-07, 8e-07, 3.00e-07),
    ("resae", "b/B15/job0", "dY"): (2.380e-07, 1e-06, 3.41e-07),
    ("resae", "b/B15/job0", "dW"): (3.162e-07, 2e-06, 4.30e-07),
    ("resae", "b/B15/job0", "db"): (2.320e-07, 1e-06, 3.59e-07),
    ("resae", "b/B16/job0", "recon"): (1.547e-07, 7e-07, 1.72e-07),
    ("resae", "b/B16/job0", "latents"): (1.580e-07, 7e-07, 1.83e-07),
    ("resae", "b/B16/job0", "acts"): (1.973e-07, 8e-07, 2.26e-07),
    ("resae", "b/B16/job0", "dx"): (1.410e-07, 6e-07, 2.12e-07),
    ("resae", "b/B16/job0", "dY"): (2.012e-07, 9e-07, 3.74e-07),
    ("resae", "b/B16/job0", "dW"): (3.241e-07, 2e-06, 4.19e-07),
    ("resae", "b/B16/job0", "db"): (2.019e-07, 9e-07, 3.93e-07),
    ("resae", "b/B17/job0", "recon"): (1.352e-07, 6e-07, 1.62e-07),
    ("resae", "b/B17/job0", "latents"): (1.449e-07, 6e-07, 1.89e-07),
    ("resae", "b/B17/job0", "acts"): (1.609e-07, 7e-07, 1.99e-07),
    ("resae", "b/B17/job0", "dx"): (1.459e-07, 6e-07, 2.19e-07),
    ("resae", "b/B17/job0", "dY"): (1.917e-07, 8e-07, 2.96e-07),
    ("resae", "b/B17/job0", "dW"): (3.182e-07, 2e-06, 3.67e-07),
    ("resae", "b/B17/job0", "db"): (2.492e-07, 1e-06, 4.18e-07),
    ("resae", "c/B5/job0", "recon"): (1.165e-07, 5e-07, 1.75e-07),
    ("resae", "c/B5/job0", "latents"): (1.909e-07, 8e-07, 1.79e-07),
    ("resae", "c/B5/job0", "acts"): (2.030e-07, 9e-07, 2.09e-07),
    ("resae", "c/B5/job0", "dx"): (2.006e-07, 9e-07, 3.01e-07),
    ("resae", "c/B5/job0", "dY"): (2.073e-07, 9e-07, 3.89e-07),
    ("resae", "c/B5/job0", "dW"): (2.605e-07, 2e-06, 4.26e-07),
    ("resae", "c/B5/job0", "db"): (2.267e-07, 1e-06, 4.13e-07),
    ("resae", "c/B5/job1", "recon"): (1.974e-07, 8e-07, 1.96e-07),
    ("resae", "c/B5/job1", "latents"): (1.636e-07, 7e-07, 1.61e-07),
    ("resae", "c/B5/job1", "acts"): (2.079e-07, 9e-07, 2.29e-07),
    ("resae", "c/B5/job1", "dx"): (1.652e-07, 7e-07, 2.79e-07),
    ("resae", "c/B5/job1", "dY"): (3.244e-07, 2e-06, 5.57e-07),
    ("resae", "c/B5/job1", "dW"): (3.277e-07, 2e-06, 4.99e-07),
    ("resae", "c/B5/job1", "db"): (3.770e-07, 2e-06, 4.96e-07),
    ("resae", "d/B33/job0", "recon"): (1.584e-07, 7e-07, 2.26e-07),
    ("resae", "d/B33/job0", "latents"): (1.978e-07, 8e-07, 2.48e-07),
    ("resae", "d/B33/job0", "acts"): (2.021e-07, 9e-07, 2.51e-07),
    ("resae", "d/B33/job0", "dx"): (2.120e-07, 9e-07, 2.71e-07),
    ("resae", "d/B33/job0", "dY"): (2.053e-07, 9e-07, 3.85e-07),
    ("resae", "d/B33/job0", "dW"): (3.219e-07, 2e-06, 4.97e-07),
    ("resae", "d/B33/job0", "db"): (2.394e-07, 1e-06, 4.92e-07),
    ("resae", "d/B33/job1", "recon"): (1.540e-07, 7e-07, 1.95e-07),
    ("resae", "d/B33/job1", "latents"): (1.903e-07, 8e-07, 1.85e-07),
    ("resae", "d/B33/job1", "acts"): (2.459e-07, 1e-06, 2.38e-07),
    ("resae", "d/B33/job1", "dx"): (1.766e-07, 8e-07, 2.60e-07),
    ("resae", "d/B33/job1", "dY"): (3.100e-07, 2e-06, 4.42e-07),
    ("resae", "d/B33/job1", "dW"): (3.825e-07, 2e-06, 4.78e-07),
    ("resae", "d/B33/job1", "db"): (3.427e-07, 2e-06, 5.32e-07),
    ("resae", "e/B4/job0", "recon"): (1.579e-07, 7e-07, 2.03e-07),
    ("resae", "e/B4/job0", "latents"): (1.729e-07, 7e-07, 2.63e-07),
    ("resae", "e/B4/job0", "acts"): (1.729e-07, 7e-07, 2.63e-07),
    ("resae", "e/B4/job0", "dx"): (1.701e-07, 7e-07, 2.35e-07),
    ("resae", "e/B4/job0", "dY"): (1.721e-07, 7e-07, 2.47e-07),
    ("resae", "e/B4/job0", "dW"): (2.574e-07, 2e-06, 2.55e-07),
    ("resae", "e/B4/job0", "db"): (1.895e-07, 8e-07, 3.27e-07),
}


# erc_mse_grad and the whole model on the fixtures, same kind of record: (the bound the GPU test derived from the twin, the
# kernel's error against float64 measured on an MI355X); gradients by the parameter closest to its bound
OTHER_FIGURES = {
    ("mse", "B1", "loss"): (3e-07, 1.15e-08), ("mse", "B1", "d"): (5e-07, 1.09e-07),
    ("mse", "B33", "loss"): (3e-07, 8.08e-09), ("mse", "B33", "d"): (4e-07, 7.79e-08),
    ("model", "mmin_miss_a", "reverse"): (6e-07, 2.70e-07), ("model", "mmin_miss_a", "logits"): (3e-07, 6.20e-08),
    ("model", "mmin_miss_a", "fusion"): (9e-07, 2.43e-07), ("model", "mmin_miss_a", "fusion_cycle"): (8e-07, 2.58e-07),
    ("model", "mmin_miss_a", "features"): (5e-07, 2.05e-07), ("model", "mmin_miss_a", "Lall"): (4e-07, 1.76e-08),
    ("model", "mmin_miss_a", "Lmse"): (3e-07, 2.27e-08), ("model", "mmin_miss_a", "Lcycle"): (3e-07, 2.36e-08),
    ("model", "mmin_miss_a", "Lce"): (4e-07, 4.71e-09), ("model", "mmin_miss_a", "grads"): (5e-07, 3.71e-07),
    ("model", "mmin_miss_b2", "reverse"): (5e-07, 1.47e-07), ("model", "mmin_miss_b2", "logits"): (5e-07, 1.14e-07),
    ("model", "mmin_miss_b2", "fusion"): (8e-07, 2.88e-07), ("model", "mmin_miss_b2", "fusion_cycle"): (7e-07, 1.79e-07),
    ("model", "mmin_miss_b2", "features"): (8e-07, 2.30e-07), ("model", "mmin_miss_b2", "Lall"): (4e-07, 1.71e-08),
    ("model", "mmin_miss_b2", "Lmse"): (3e-07, 5.36e-08), ("model", "mmin_miss_b2", "Lcycle"): (3e-07, 1.05e-07),
    ("model", "mmin_miss_b2", "Lce"): (3e-07, 1.08e-08), ("model", "mmin_miss_b2", "grads"): (9e-07, 5.57e-07),
}

def _gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()))


def layer_dims(n_blocks):
    """(out, in) of every layer in chain order"""
    return [(256, 384), (128, 256), (64, 128), (128, 64), (256, 128), (384, 256)] * n_blocks + [(384, 384), (384, 384)]


def layer_names(n_blocks):
    """state_dict prefixes of a ResidualAE's layers in chain order"""
    out = []
    for i in range(n_blocks):
        out += ["encoder_%d.%d" % (i, k) for k in (0, 2, 4)] + ["decoder_%d.%d" % (i, k) for k in (0, 2, 4)]
    return out + ["transition.0", "transition.2"]


def activation_of(l, n_blocks):
    """'leaky' / 'relu' / None behind layer l of the chain"""
    if l >= 6 * n_blocks:
        return "relu" if l == 6 * n_blocks else None
    return ("leaky", "leaky", None, "relu", "relu", None)[l % 6]


def ae_params(n_blocks, g, decoder_bias=None):
    """[(W [out, in], b [out])] in chain order, nn.Linear's own range U(-1 / sqrt(in), 1 / sqrt(in))"""
    out = []
    for l, (n_out, n_in) in enumerate(layer_dims(n_blocks)):
        k = 1.0 / math.sqrt(n_in)
        W = (torch.rand(n_out, n_in, generator=g) * 2 - 1) * k
        b = (torch.rand(n_out, generator=g) * 2 - 1) * k
        if decoder_bias is not None and l < 6 * n_blocks and l % 6 >= 3:
            b = torch.full((n_out, ), float(decoder_bias))
        out.append((W, b))
    return out


def ae_case(name, B, job=0):
    """seeded inputs of one job of a case at batch size B"""
    _, nb, _, dec_bias = AE_CASES[name]
    g = _gen("mmin-miss-ae-%s-%d-%d" % (name, B, job))
    return dict(name=name, B=B, nb=nb, P=ae_params(nb, g, dec_bias), x=torch.randn(B, D, generator=g),
                d_recon=torch.randn(B, D, generator=g), d_latents=torch.randn(B, LAT1 * nb, generator=g))


def _act(y, kind):
    if kind == "leaky":
        return torch.where(y > 0, y, SLOPE * y)
    if kind == "relu":
        return torch.clamp(y, min=0)
    return y


def resae_fwd(P, x, n_blocks, dtype=torch.float64):
    """-> dict(recon [B,384], latents [B, 64 n], acts: every layer's INPUT rows, pre: every layer's pre-activation output)"""
    P = [(W.to(dtype), b.to(dtype)) for W, b in P]
    x_in, x_out = x.to(dtype), torch.zeros_like(x, dtype=dtype)
    acts, pre, latents = [], [], []
    for i in range(n_blocks):
        x_in = x_in + x_out
        h = x_in
        for l in range(6 * i, 6 * i + 6):
            acts.append(h)
            y = mm(h, P[l][0].t()) + P[l][1]
            pre.append(y)
            h = _act(y, activation_of(l, n_blocks))
            if l % 6 == 2:
                latents.append(y)
        x_out = h
    h = x_in + x_out
    for l in (6 * n_blocks, 6 * n_blocks + 1):
        acts.append(h)
        y = mm(h, P[l][0].t()) + P[l][1]
        pre.append(y)
        h = _act(y, activation_of(l, n_blocks))
    return dict(recon=h, latents=torch.cat(latents, -1), acts=acts, pre=pre)


def masks_of(pre, n_blocks):
    """{layer: pre-activation > 0} for the layers that have an activation"""
    return {l: y > 0 for l, y in enumerate(pre) if activation_of(l, n_blocks)}


def resae_bwd(P, acts, masks, d_recon, d_latents, n_blocks, dtype=torch.float64):
    """the closed form above on ``masks`` {layer: bool [B, out]}.  -> dict(dx, dY [layers], dW [layers], db [layers])"""
    Ws = [W.to(dtype) for W, _ in P]
    acts = [a.to(dtype) for a in acts]
    nL = 6 * n_blocks + 2
    dY = [None] * nL

    def through(l, d):
        kind = activation_of(l, n_blocks)
        if kind == "relu":
            return torch.where(masks[l], d, torch.zeros_like(d))
        if kind == "leaky":
            return torch.where(masks[l], d, SLOPE * d)
        return d
    dY[nL - 1] = d_recon.to(dtype)
    dY[nL - 2] = through(nL - 2, mm(dY[nL - 1], Ws[nL - 1]))
    G = mm(dY[nL - 2], Ws[nL - 2])
    for i in range(n_blocks - 1, -1, -1):
        dY[6 * i + 5] = G
        for l in range(6 * i + 4, 6 * i - 1, -1):
            d = mm(dY[l + 1], Ws[l + 1])
            if l % 6 == 2 and d_latents is not None:
                d = d + d_latents.to(dtype)[:, LAT1 * i:LAT1 * (i + 1)]
            dY[l] = through(l, d)
        G = G + mm(dY[6 * i], Ws[6 * i])
    return dict(dx=G, dY=dY, dW=[mm(dY[l].t(), acts[l]) for l in range(nL)], db=[ops.colsum(dY[l]) for l in range(nL)])


def mse_pair(a, b, weight, dtype=torch.float64):
    """F.mse_loss(a, b) and d(weight loss) / da (its negative is the gradient wrt b)"""
    a, b = a.to(dtype), b.to(dtype)
    diff = a - b
    n = diff.numel()
    return ops.colsum((diff * diff).reshape(-1)) / n, diff * (weight * 2.0 / n)


def ae_reference(c, with_latents=True):
    """float64 forward and backward (own masks), the twin's forward, the twin's backward on float64's masks: (f64, b64, f32, b32)"""
    dl = c["d_latents"] if with_latents else None
    with one_thread():
        f64 = resae_fwd(c["P"], c["x"], c["nb"])
        m64 = masks_of(f64["pre"], c["nb"])
        b64 = resae_bwd(c["P"], f64["acts"], m64, c["d_recon"], dl, c["nb"])
        f32 = resae_fwd(c["P"], c["x"], c["nb"], dtype=torch.float32)
        b32 = resae_bwd(c["P"], f32["acts"], m64, c["d_recon"], dl, c["nb"], dtype=torch.float32)
    return f64, b64, f32, b32


# ---------------------------------------------------------------------------------------------------------- whole model
def sd_shapes(n_classes=4):
    """the reference's MMINMissModule.state_dict(): 150 (key, shape) pairs"""
    out = [kv for kv in R.SD_SHAPES if not kv[0].startswith("netC.")]
    for net in ("netAE", "netAE_cycle"):
        names, dims = layer_names(N_BLOCKS), layer_dims(N_BLOCKS)
        order = names[-2:] + names[:-2]          # the transition is registered first
        shape = dict(zip(names, dims))
        for n in order:
            out += [("%s.%s.weight" % (net, n), shape[n]), ("%s.%s.bias" % (net, n), (shape[n][0], ))]
    return tuple(out) + (("netC.fc_out.weight", (n_classes, 128)), ("netC.fc_out.bias", (n_classes, )),
                         ("netC.module.0.weight", (128, LAT1 * N_BLOCKS)), ("netC.module.0.bias", (128, )),
                         ("netC.module.3.weight", (128, 128)), ("netC.module.3.bias", (128, )))


N_PARAMS = 5444228


def apply_missing(batch, missing_type):
    """MMINMissCollate's masking (mmin_miss.py:328-337): x m and x_reverse = x (1 - m); mask columns visual, text, audio"""
    out = dict(batch)
    mt = torch.as_tensor(missing_type, dtype=torch.long)
    for i, key in enumerate(MODAL_KEYS):
        m = mt[:, i][:, None, None]
        out[key] = batch[key] * m
        out[key + "_reverse"] = batch[key] * -1 * (m - 1)
    out["missing_type"] = mt
    return out


def encode(P, audio, visual, text, dtype=torch.float64):
    """the three encoders of the base model in eval mode -> dict(A, V, L (their forward records), text, features [B, 384])"""
    P = {k: v.to(dtype) for k, v in P.items()}
    lstm = lambda net, x: R.lstm_pool_fwd(x, *(P[net + ".rnn." + n] for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")),
                                          dtype=dtype)
    A, V = lstm("netA", audio), lstm("netV", visual)
    Ws = [P["netL.conv%d.weight" % (n + 1)].reshape(R.CH, k, -1) for n, k in enumerate(R.KS)]
    L = R.textcnn_fwd(text, Ws, [P["netL.conv%d.bias" % (n + 1)] for n in range(3)], dtype=dtype)
    text_f = torch.clamp(mm(L["pooled"], P["netL.embd.0.weight"].t()) + P["netL.embd.0.bias"], min=0)
    return dict(A=A, V=V, L=L, text=text_f, features=torch.cat([A["pool"], V["pool"], text_f], -1))


def _ae_of(P, net):
    return [(P["%s.%s.weight" % (net, n)], P["%s.%s.bias" % (net, n)]) for n in layer_names(N_BLOCKS)]


def model_loss_grads(P, batch, reverse_features, dtype=torch.float64, masks=None, args=None):
    """eval mode (no dropout).  P: MMINMissModule state_dict; batch: the MASKED batch; reverse_features [B, 384] a constant.
    masks: None (each network's own) or dict(netAE={layer: bool}, netAE_cycle=...); args: None or the encoders' routing
    (dict(audio, visual, text)).  -> dict(logits, fusion, fusion_cycle, features, latents, Lce, Lmse, Lcycle, Lall, grads, ...)"""
    P = {k: v.to(dtype) for k, v in P.items()}
    e = encode(P, batch["audio_feature"], batch["visual_feature"], batch["text_feature"], dtype)
    feats = e["features"]
    ae = {net: resae_fwd(_ae_of(P, net), feats, N_BLOCKS, dtype) for net in ("netAE", "netAE_cycle")}
    masks = masks or {net: masks_of(ae[net]["pre"], N_BLOCKS) for net in ae}
    args = args or dict(audio=e["A"]["arg"], visual=e["V"]["arg"], text=e["L"]["arg"])
    fusion, fusion_cycle, latents = ae["netAE"]["recon"], ae["netAE_cycle"]["recon"], ae["netAE"]["latents"]
    lin = lambda x, n: mm(x, P[n + ".weight"].t()) + P[n + ".bias"]
    z0 = torch.clamp(lin(latents, "netC.module.0"), min=0)
    feat = torch.clamp(lin(z0, "netC.module.3"), min=0)
    logits = lin(feat, "netC.fc_out")
    y = batch["label"].long()
    B = logits.shape[0]
    Lce = (torch.logsumexp(logits, -1) - logits.gather(1, y[:, None]).squeeze(1)).sum() / B
    Lmse, d_fusion = mse_pair(fusion, reverse_features, W_MSE, dtype)
    Lcycle, d_cycle = mse_pair(fusion_cycle, feats, W_CYCLE, dtype)
    G = {}

    def lin_bwd(name, dy, xin):
        G[name + ".weight"], G[name + ".bias"] = mm(dy.t(), xin), ops.colsum(dy)
        return mm(dy, P[name + ".weight"])
    dlog = (torch.softmax(logits, -1) - torch.nn.functional.one_hot(y, logits.shape[1]).to(dtype)) / B
    dfeat = lin_bwd("netC.fc_out", dlog, feat)
    dz1 = torch.where(feat > 0, dfeat, torch.zeros_like(dfeat))
    dz0 = lin_bwd("netC.module.3", dz1, z0)
    dz0 = torch.where(z0 > 0, dz0, torch.zeros_like(dz0))
    dlat = lin_bwd("netC.module.0", dz0, latents)
    bw = {"netAE": resae_bwd(_ae_of(P, "netAE"), ae["netAE"]["acts"], masks["netAE"], d_fusion, dlat, N_BLOCKS, dtype),
          "netAE_cycle": resae_bwd(_ae_of(P, "netAE_cycle"), ae["netAE_cycle"]["acts"], masks["netAE_cycle"], d_cycle, None, N_BLOCKS, dtype)}
    for net, r in bw.items():
        for l, n in enumerate(layer_names(N_BLOCKS)):
            G["%s.%s.weight" % (net, n)], G["%s.%s.bias" % (net, n)] = r["dW"][l], r["db"][l]
    # netAE_cycle reads features and Lcycle reads them again (mmin_miss.py:104, :208)
    dfeatures = bw["netAE"]["dx"] + bw["netAE_cycle"]["dx"] - d_cycle
    H = R.H
    dtext = torch.where(e["text"] > 0, dfeatures[:, 2 * H:], torch.zeros_like(e["text"]))
    dpooled = lin_bwd("netL.embd.0", dtext, e["L"]["pooled"])
    tb = R.textcnn_bwd(batch["text_feature"], e["L"]["pooled"], args["text"], dpooled, dtype)
    for n, k in enumerate(R.KS):
        G["netL.conv%d.weight" % (n + 1)] = tb[k][0].reshape(R.CH, 1, k, -1)
        G["netL.conv%d.bias" % (n + 1)] = tb[k][1]
    for net, key, xk, lo in (("netA", "A", "audio_feature", 0), ("netV", "V", "visual_feature", H)):
        r = R.lstm_pool_bwd(e[key], batch[xk], P[net + ".rnn.weight_hh_l0"], dfeatures[:, lo:lo + H], args["audio" if net == "netA" else "visual"],
                            dtype)
        G[net + ".rnn.weight_ih_l0"], G[net + ".rnn.weight_hh_l0"] = r["dW_ih"], r["dW_hh"]
        G[net + ".rnn.bias_ih_l0"] = G[net + ".rnn.bias_hh_l0"] = r["db"]
    return dict(logits=logits, fusion=fusion, fusion_cycle=fusion_cycle, features=feats, latents=latents, Lce=Lce, Lmse=Lmse,
                Lcycle=Lcycle, Lall=Lce + W_MSE * Lmse + W_CYCLE * Lcycle, grads=G, masks=masks, args=args, ae=ae, enc=e,
                dfeatures=dfeatures)


# name -> (B, Ta, Tv, Tt, audio zero-from, missing_type per sample)
MODEL_CASES = {
    "mmin_miss_a": (6, 13, 6, 7, (13, 4, 1, 9, 13, 7), MISSING_TYPES),                         # all six patterns
    "mmin_miss_b2": (2, 9, 50, 22, (9, 3), (MISSING_TYPES[4], MISSING_TYPES[1])),             # --debug: the real visual / text shapes
}
# (parameter seed of the model, of the pretrained model, batch seed)
MODEL_SEEDS = {"mmin_miss_a": (91, 92, 191), "mmin_miss_b2": (93, 94, 192)}


def make_batch(name):
    """seeded FULL-modality batch of a model case (audio zero-padded as the collate pads) and its missing_type"""
    B, Ta, Tv, Tt, zf, mt = MODEL_CASES[name]
    g = torch.Generator().manual_seed(MODEL_SEEDS[name][2])
    a = torch.randn(B, Ta, R.AUDIO_D, generator=g)
    for b, z in enumerate(zf):
        a[b, z:] = 0.0
    return dict(audio_feature=a, visual_feature=torch.randn(B, Tv, R.VISUAL_D, generator=g),
                text_feature=torch.randn(B, Tt, R.TEXT_D, generator=g), label=torch.randint(0, 4, (B, ), generator=g)), \
        torch.tensor(mt, dtype=torch.long)


def named_filled(shapes, seed):
    """{key: tensor} filled as make_golden.fill_params fills a model with these parameter names (sorted, seeded)"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in sorted(shapes):
        bound = 1.0 / (shape[-1] ** 0.5) if len(shape) > 1 else 0.1
        out[name] = (torch.rand(shape, generator=g) * 2 - 1) * bound
    return {k: out[k] for k, _ in shapes}


def digest(flat, seed=0, keep=512, whole=2048):
    """the entries of a gradient that the fixtures store (make_golden.grad_digest's scheme with a lower threshold: 128 of the
    150 tensors are Linear weights of 8 192 .. 147 456 elements): all of a tensor of at most ``whole`` elements, ``keep`` seeded
    positions of a larger one"""
    flat = flat.detach().flatten()
    if flat.numel() <= whole:
        return flat
    g = torch.Generator().manual_seed(seed + flat.numel())
    return flat[torch.randint(0, flat.numel(), (keep, ), generator=g)]
