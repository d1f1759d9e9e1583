"""Float64 restatements of the MMIN full-modality base model (erc_amd/mmin.py; csrc/lstm128.hip, textcnn.hip, ema.hip), their
float32 twins, the case tables and the bounds of tests/test_mmin_ref.py and tests/test_gpu_mmin.py.  Written from the math, in
plain torch on the CPU; nothing of the kernels' thread layout or chunking.

Math.  LSTM-128 + max-pool: GX = x W_ih^T + b_ih; per step (i, f, g, o) = GX_t + h_{t-1} W_hh^T + b_hh, i, f, o through the
sigmoid and g through tanh, c_t = f c_{t-1} + i g, h_t = o tanh(c_t), h_0 = c_0 = 0; pool[b, u] = max over ALL t < T of
h_t[b, u] (padded steps are steps like any other), arg the first t attaining it.  Text CNN + pool: for k = 3, 4, 5
conv_k[b, t, ch] = bias_k[ch] + sum_{j < k} <x[b, t + j, :], W_k[ch, j, :]>, t <= T - k; pooled = max_t relu(conv), arg the
first t; a channel whose windows are all <= 0 pools to 0 with gradient 0.

Every backward takes the ``arg`` routing as an INPUT: near-ties inside the audio padding are real (two steps of a unit can
differ by 8e-8), so two correct float32 evaluations may pick different steps, and a backward is compared on the routing the
kernel itself used.

Float32 twins: the same functions with dtype=float32, built on tests/rnn_scan_ref.py's ``ops`` (products from elementwise float32
multiplies and adds in a fixed order, activations evaluated in float64 and rounded), so a twin's figure does not depend on the
machine's math libraries.

Bounds.  A quantity's bound is MARGIN x (the twin's own deviation from float64 on that case and quantity), rounded up to one
significant digit, errors measured relative to the largest reference magnitude of the quantity (rnn_scan_ref.rel).  MARGIN = 4:
  * summation order, factor 2.  Twin and kernel sum the same K products in different orders (twin: radix-8 tree; scan: the
    quad splits K = 128 into 4 x 32, each as two chains of 16, then two DPP adds; text CNN: K = 3072 .. 5120 in MFMA blocks of 4
    split over wavefronts; weight gradients: K = B T rows split over work items).  With |w| <= 1 / sqrt(128) = 0.088 and
    |h| < 1, |x| ~ 1 every order's error is a sum of K - 1 roundings of partial sums of the same magnitude (<= K 0.088 u), i.e.
    a draw from the same distribution; the maxima of two such draws over the 10^3 .. 10^5 elements of a quantity differ by
    well under a factor 2.  That holds while the chains are short.  It does NOT hold for one chain over the text CNN's whole
    K: a chain of n adds loses ~sqrt(n) roundings where the twin's tree loses ~sqrt(log n), and the first form of
    erc_textcnn_pool_fwd (one accumulation over K per output) measured 6.09e-7 on `pooled` of case (a) against this bound
    of 6e-7.  The bound stayed; the kernel now cuts K into 8 pieces summed in index order (csrc/textcnn.hip) and measures
    2.2e-7.
  * activations, factor 2.  The twin's sigmoid / tanh are correctly rounded (0.5 ulp); the scans use the hardware exponential
    and reciprocal (1 ulp each; csrc/rnn100_dev.h), 2 ulp per activation against 0.5, diluted by the product error that
    both share.
This is the rule of tests/rnn_scan_ref.py (``bound``) for the hidden-100 scans.  A kernel's measured figure never enters a
bound; the figures measured on an MI355X are recorded in FIGURES below, next to the twin's.

``arg`` is a condition, not an equality: for every (b, u), ref64[b, arg_kernel[b, u], u] >= max64[b, u] - bound_fwd, where
bound_fwd is the pool's bound as an absolute figure.  For the text CNN the committed seeds have no live channel whose two
best windows are closer than 1e-5, float32 twin and float64 agree on every live channel (test_mmin_ref.py asserts both), and
the kernel's indices must equal float64's there.
"""
import math
import zlib

import numpy as np
import torch

from tests.rnn_scan_ref import _sum0, bound, mm, one_thread, ops, rel, round_up_1  # noqa: F401

H, G4, CH = 128, 512, 128
KS = (3, 4, 5)
MARGIN = 4.0
AUDIO_D, VISUAL_D, TEXT_D = 130, 342, 1024

# name -> (B, T, D, first zero row of each sample (None: no padding))
SCAN_CASES = {
    "a": (5, 13, AUDIO_D, (13, 4, 1, 9, 13)),      # the padding case: audio rows zero from step 13/4/1/9/13 on
    "b": (1, 1, AUDIO_D, None),
    "c": (3, 50, VISUAL_D, None),
    "d": (33, 70, AUDIO_D, None),                   # more workgroups than 32, T over every chunk boundary
}
# name -> (B, T, bias override)
CNN_CASES = {
    "a": (5, 7, None),       # k = 5 has 3 windows, k = 3 has 5
    "b": (1, 5, None),       # k = 5 has one window
    "c": (32, 22, None),     # the real shape
    "d": (4, 9, -10.0),      # every channel ReLU-dead: pooled 0, gradients exactly 0
}

# Figures: max error relative to the quantity's largest float64 magnitude, per (kernel family, case, quantity):
# (the float32 twin against float64 -- this file, any machine; the bound = round_up_1(MARGIN x max(twin, FLOOR));
#  the kernel against float64, measured on an MI355X -- tests/test_gpu_mmin.py prints the live values).  The table is a record:
# the tests derive every bound from the twin at run time and never read the third column.
FIGURES = {
    ("scan", "a", "pool"): (1.61e-07, 7e-07, 3.16e-07),
    ("scan", "a", "gates"): (2.00e-07, 8e-07, 3.20e-07),
    ("scan", "a", "Cst"): (1.17e-07, 5e-07, 2.15e-07),
    ("scan", "a", "Hprev"): (1.58e-07, 7e-07, 3.11e-07),
    ("scan", "a", "dGX"): (1.28e-07, 6e-07, 2.48e-07),
    ("scan", "a", "dW_ih"): (1.65e-07, 7e-07, 2.60e-07),
    ("scan", "a", "dW_hh"): (1.67e-07, 7e-07, 2.87e-07),
    ("scan", "a", "db_ih"): (1.69e-07, 7e-07, 5.10e-07),
    ("scan", "a", "db_hh"): (1.69e-07, 7e-07, 5.10e-07),
    ("scan", "b", "pool"): (1.60e-07, 7e-07, 2.40e-07),
    ("scan", "b", "gates"): (2.49e-07, 1e-06, 2.11e-07),
    ("scan", "b", "Cst"): (1.54e-07, 7e-07, 2.11e-07),
    ("scan", "b", "Hprev"): (0.00e+00, 3e-07, 0.00e+00),
    ("scan", "b", "dGX"): (1.29e-07, 6e-07, 1.84e-07),
    ("scan", "b", "dW_ih"): (1.42e-07, 6e-07, 1.87e-07),
    ("scan", "b", "dW_hh"): (0.00e+00, 3e-07, 0.00e+00),
    ("scan", "b", "db_ih"): (1.29e-07, 6e-07, 1.84e-07),
    ("scan", "b", "db_hh"): (1.29e-07, 6e-07, 1.84e-07),
    ("scan", "c", "pool"): (1.42e-07, 6e-07, 3.00e-07),
    ("scan", "c", "gates"): (2.93e-07, 2e-06, 8.14e-07),
    ("scan", "c", "Cst"): (1.52e-07, 7e-07, 2.96e-07),
    ("scan", "c", "Hprev"): (2.00e-07, 9e-07, 3.94e-07),
    ("scan", "c", "dGX"): (3.00e-07, 2e-06, 5.79e-07),
    ("scan", "c", "dW_ih"): (3.14e-07, 2e-06, 5.63e-07),
    ("scan", "c", "dW_hh"): (2.53e-07, 2e-06, 5.02e-07),
    ("scan", "c", "db_ih"): (2.14e-07, 9e-07, 3.88e-07),
    ("scan", "c", "db_hh"): (2.14e-07, 9e-07, 3.88e-07),
    ("scan", "d", "pool"): (1.63e-07, 7e-07, 3.23e-07),
    ("scan", "d", "gates"): (2.86e-07, 2e-06, 4.11e-07),
    ("scan", "d", "Cst"): (1.56e-07, 7e-07, 2.22e-07),
    ("scan", "d", "Hprev"): (1.79e-07, 8e-07, 3.84e-07),
    ("scan", "d", "dGX"): (1.52e-07, 7e-07, 3.14e-07),
    ("scan", "d", "dW_ih"): (3.61e-07, 2e-06, 4.96e-07),
    ("scan", "d", "dW_hh"): (3.69e-07, 2e-06, 6.10e-07),
    ("scan", "d", "db_ih"): (1.76e-07, 8e-07, 5.76e-07),
    ("scan", "d", "db_hh"): (1.76e-07, 8e-07, 5.76e-07),
    ("textcnn", "a", "pooled"): (1.44e-07, 6e-07, 2.23e-07),
    ("textcnn", "a", "dW3"): (8.18e-08, 4e-07, 8.18e-08),
    ("textcnn", "a", "db3"): (5.21e-08, 3e-07, 5.21e-08),
    ("textcnn", "a", "dW4"): (9.35e-08, 4e-07, 8.81e-08),
    ("textcnn", "a", "db4"): (5.38e-08, 3e-07, 5.38e-08),
    ("textcnn", "a", "dW5"): (1.13e-07, 5e-07, 1.13e-07),
    ("textcnn", "a", "db5"): (5.21e-08, 3e-07, 5.21e-08),
    ("textcnn", "b", "pooled"): (1.17e-07, 5e-07, 1.57e-07),
    ("textcnn", "b", "dW3"): (4.42e-08, 3e-07, 4.42e-08),
    ("textcnn", "b", "db3"): (0.00e+00, 3e-07, 0.00e+00),
    ("textcnn", "b", "dW4"): (4.03e-08, 3e-07, 4.03e-08),
    ("textcnn", "b", "db4"): (0.00e+00, 3e-07, 0.00e+00),
    ("textcnn", "b", "dW5"): (3.62e-08, 3e-07, 3.62e-08),
    ("textcnn", "b", "db5"): (0.00e+00, 3e-07, 0.00e+00),
    ("textcnn", "c", "pooled"): (5.12e-07, 3e-06, 2.21e-07),
    ("textcnn", "c", "dW3"): (2.54e-07, 2e-06, 2.54e-07),
    ("textcnn", "c", "db3"): (1.22e-07, 5e-07, 1.22e-07),
    ("textcnn", "c", "dW4"): (2.54e-07, 2e-06, 2.30e-07),
    ("textcnn", "c", "db4"): (1.18e-07, 5e-07, 1.18e-07),
    ("textcnn", "c", "dW5"): (2.39e-07, 1e-06, 2.39e-07),
    ("textcnn", "c", "db5"): (1.63e-07, 7e-07, 1.63e-07),
    ("textcnn", "d", "pooled"): (0.00e+00, 3e-07, 0.00e+00),
    ("textcnn", "d", "dW3"): (0.00e+00, 3e-07, 0.00e+00),
    ("textcnn", "d", "db3"): (0.00e+00, 3e-07, 0.00e+00),
    ("textcnn", "d", "dW4"): (0.00e+00, 3e-07, 0.00e+00),
    ("textcnn", "d", "db4"): (0.00e+00, 3e-07, 0.00e+00),
    ("textcnn", "d", "dW5"): (0.00e+00, 3e-07, 0.00e+00),
    ("textcnn", "d", "db5"): (0.00e+00, 3e-07, 0.00e+00),
}


def _gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()))


def lstm_params(D, g):
    """nn.LSTM's own initialisation range, U(-1 / sqrt(128), 1 / sqrt(128))"""
    k = 1.0 / math.sqrt(H)
    r = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k
    return dict(W_ih=r(G4, D), W_hh=r(G4, H), b_ih=r(G4), b_hh=r(G4))


def scan_case(name):
    B, T, D, zero_from = SCAN_CASES[name]
    g = _gen("mmin-scan-" + name)
    c = dict(name=name, B=B, T=T, D=D, **lstm_params(D, g))
    x = torch.randn(B, T, D, generator=g)
    if zero_from is not None:
        for b, z in enumerate(zero_from):
            x[b, z:] = 0.0
    c["x"], c["dpool"] = x, torch.randn(B, H, generator=g)
    return c


def cnn_case(name):
    B, T, bias = CNN_CASES[name]
    g = _gen("mmin-cnn-" + name)
    c = dict(name=name, B=B, T=T, D=TEXT_D, x=torch.randn(B, T, TEXT_D, generator=g), dpooled=torch.randn(B, 3 * CH, generator=g))
    for k in KS:
        s = 1.0 / math.sqrt(k * TEXT_D)      # nn.Conv2d's own range
        c["W%d" % k] = (torch.rand(CH, k, TEXT_D, generator=g) * 2 - 1) * s
        c["b%d" % k] = (torch.rand(CH, generator=g) * 2 - 1) * s if bias is None else torch.full((CH, ), float(bias))
    return c


def first_argmax(v, dim):
    """(max, the first index attaining it) along ``dim``"""
    mx = v.max(dim, keepdim=True).values
    n = v.shape[dim]
    shape = [1] * v.dim()
    shape[dim] = n
    idx = torch.arange(n).view(shape).expand_as(v)
    return mx.squeeze(dim), torch.where(v == mx, idx, torch.full_like(idx, n)).min(dim).values


# ------------------------------------------------------------------------------------------------ LSTM-128 + max-pool
def lstm_pool_fwd(x, W_ih, W_hh, b_ih, b_hh, dtype=torch.float64):
    """-> dict(GX [B,T,512], hs [B,T,128], pool, arg, gates [B,T,512], Cst, Hprev [B,T,128])"""
    x, W_ih, W_hh, b_ih, b_hh = (t.to(dtype) for t in (x, W_ih, W_hh, b_ih, b_hh))
    B, T, _ = x.shape
    GX = mm(x.reshape(B * T, -1), W_ih.t()).reshape(B, T, G4) + b_ih
    h = c = x.new_zeros(B, H)
    hs, cs, gs, hp = [], [], [], []
    for t in range(T):
        i, f, g, o = (GX[:, t] + mm(h, W_hh.t()) + b_hh).chunk(4, -1)
        i, f, g, o = ops.sigmoid(i), ops.sigmoid(f), ops.tanh(g), ops.sigmoid(o)
        hp.append(h)
        c = f * c + i * g
        h = o * ops.tanh(c)
        hs.append(h), cs.append(c), gs.append(torch.cat([i, f, g, o], -1))
    hs = torch.stack(hs, 1)
    pool, arg = first_argmax(hs, 1)
    return dict(GX=GX, hs=hs, pool=pool, arg=arg, gates=torch.stack(gs, 1), Cst=torch.stack(cs, 1), Hprev=torch.stack(hp, 1))


def lstm_pool_bwd(fwd, x, W_hh, dpool, arg, dtype=torch.float64):
    """the backward on routing ``arg`` [B,128]: dGX [B,T,512] and the caller's products dW_ih, dW_hh, db (= db_ih = db_hh)"""
    gates, Cst, Hprev = (fwd[k].to(dtype) for k in ("gates", "Cst", "Hprev"))
    x, W_hh, dpool = x.to(dtype), W_hh.to(dtype), dpool.to(dtype)
    B, T, _ = gates.shape
    dh_rec = dc = gates.new_zeros(B, H)
    out = [None] * T
    for t in range(T - 1, -1, -1):
        i, f, g, o = gates[:, t].chunk(4, -1)
        cprev = Cst[:, t - 1] if t > 0 else torch.zeros_like(dc)
        tc = ops.tanh(Cst[:, t])
        dh = torch.where(arg == t, dpool, torch.zeros_like(dpool)) + dh_rec
        dc = dc + dh * o * (1 - tc * tc)
        dpre = torch.cat([dc * g * i * (1 - i), dc * cprev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], -1)
        out[t] = dpre
        dh_rec = mm(dpre, W_hh)
        dc = dc * f
    dGX = torch.stack(out, 1)
    flat = dGX.reshape(B * T, G4)
    return dict(dGX=dGX, dW_ih=mm(flat.t(), x.reshape(B * T, -1)), dW_hh=mm(flat.t(), Hprev.reshape(B * T, H)), db=ops.colsum(flat))


def arg_condition(hs64, arg_kernel, tol):
    """number of (b, u) whose routed step is not within ``tol`` of the float64 maximum"""
    picked = hs64.gather(1, arg_kernel.long().unsqueeze(1)).squeeze(1)
    return int((picked < hs64.max(1).values - tol).sum())


# ------------------------------------------------------------------------------------------------------ text CNN + pool
def textcnn_fwd(x, Ws, bs, dtype=torch.float64):
    """Ws / bs: per k the weight [128, k, D] and bias [128].  -> dict(conv {k: [B, T-k+1, 128]}, pooled [B,384], arg [B,384])"""
    x = x.to(dtype)
    B, T, D = x.shape
    conv, pooled, arg = {}, [], []
    for k, W, b in zip(KS, Ws, bs):
        win = torch.stack([x[:, j:T - k + 1 + j] for j in range(k)], 2).reshape(B * (T - k + 1), k * D)
        c = (mm(win, W.to(dtype).reshape(CH, k * D).t()) + b.to(dtype)).reshape(B, T - k + 1, CH)
        conv[k] = c
        r = torch.clamp(c, min=0)
        p, a = first_argmax(r, 1)
        pooled.append(p), arg.append(a)
    return dict(conv=conv, pooled=torch.cat(pooled, -1), arg=torch.cat(arg, -1))


def textcnn_bwd(x, pooled, arg, dpooled, dtype=torch.float64):
    """on routing ``arg``: {k: (dW [128,k,D], db [128])}; the samples are summed in index order"""
    x, dpooled = x.to(dtype), dpooled.to(dtype)
    B, T, D = x.shape
    g = torch.where(pooled > 0, dpooled, torch.zeros_like(dpooled))
    out = {}
    for n, k in enumerate(KS):
        gk, ak = g[:, n * CH:(n + 1) * CH], arg[:, n * CH:(n + 1) * CH].long()
        dW = x.new_zeros(CH, k, D)
        for b in range(B):
            rows = ak[b][:, None] + torch.arange(k)[None, :]            # [128, k]
            dW = dW + gk[b][:, None, None] * x[b][rows]
        db = x.new_zeros(CH)
        for b in range(B):
            db = db + gk[b]
        out[k] = (dW, db)
    return out


def min_live_gap(conv, pooled):
    """smallest gap between the best and the second-best window of a live channel (inf when no channel has two windows)"""
    gap = float("inf")
    for n, k in enumerate(KS):
        r = torch.clamp(conv[k], min=0)
        if r.shape[1] < 2:
            continue
        top = r.topk(2, dim=1).values
        live = pooled[:, n * CH:(n + 1) * CH] > 0
        d = (top[:, 0] - top[:, 1])[live]
        if d.numel():
            gap = min(gap, float(d.min()))
    return gap


# ---------------------------------------------------------------------------------------------------------- whole model
SD_SHAPES = (("netL.conv1.weight", (128, 1, 3, 1024)), ("netL.conv1.bias", (128, )), ("netL.conv2.weight", (128, 1, 4, 1024)),
             ("netL.conv2.bias", (128, )), ("netL.conv3.weight", (128, 1, 5, 1024)), ("netL.conv3.bias", (128, )),
             ("netL.embd.0.weight", (128, 384)), ("netL.embd.0.bias", (128, )),
             ("netA.rnn.weight_ih_l0", (512, 130)), ("netA.rnn.weight_hh_l0", (512, 128)), ("netA.rnn.bias_ih_l0", (512, )),
             ("netA.rnn.bias_hh_l0", (512, )),
             ("netV.rnn.weight_ih_l0", (512, 342)), ("netV.rnn.weight_hh_l0", (512, 128)), ("netV.rnn.bias_ih_l0", (512, )),
             ("netV.rnn.bias_hh_l0", (512, )),
             ("netC.fc_out.weight", (4, 128)), ("netC.fc_out.bias", (4, )), ("netC.module.0.weight", (128, 384)),
             ("netC.module.0.bias", (128, )), ("netC.module.3.weight", (128, 128)), ("netC.module.3.bias", (128, )))
N_PARAMS = 2063620


def _lin(x, W, b):
    return mm(x, W.t()) + b


def model_forward(P, batch, dtype=torch.float64, masks=None):
    """P: state_dict (any dtype).  masks: None (eval) or dict(text [B,384], c0 [B,128], c1 [B,128]) of inverted-dropout
    multipliers.  -> dict with logits, feat, the three encoder outputs and everything the backward needs"""
    P = {k: v.to(dtype) for k, v in P.items()}
    m = masks or {}
    one = lambda k: m[k].to(dtype) if k in m else 1.0
    A = lstm_pool_fwd(batch["audio_feature"], *(P["netA.rnn." + n] for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")), dtype=dtype)
    V = lstm_pool_fwd(batch["visual_feature"], *(P["netV.rnn." + n] for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")), dtype=dtype)
    Ws = [P["netL.conv%d.weight" % (n + 1)].reshape(CH, k, -1) for n, k in enumerate(KS)]
    bs = [P["netL.conv%d.bias" % (n + 1)] for n in range(3)]
    L = textcnn_fwd(batch["text_feature"], Ws, bs, dtype=dtype)
    pd = L["pooled"] * one("text")
    text = torch.clamp(_lin(pd, P["netL.embd.0.weight"], P["netL.embd.0.bias"]), min=0)
    fused = torch.cat([A["pool"], V["pool"], text], -1)
    z0 = torch.clamp(_lin(fused, P["netC.module.0.weight"], P["netC.module.0.bias"]), min=0) * one("c0")
    feat = torch.clamp(_lin(z0, P["netC.module.3.weight"], P["netC.module.3.bias"]), min=0) * one("c1")
    logits = _lin(feat, P["netC.fc_out.weight"], P["netC.fc_out.bias"])
    return dict(P=P, A=A, V=V, L=L, pd=pd, text=text, fused=fused, z0=z0, feat=feat, logits=logits, audio=A["pool"], visual=V["pool"])


def model_loss_grads(P, batch, dtype=torch.float64, masks=None, args=None):
    """mean cross entropy and the gradient of every parameter.  args: None (each encoder's own first maximum) or
    dict(audio [B,128], visual [B,128], text [B,384]) -- the routing the backward runs on"""
    f = model_forward(P, batch, dtype, masks)
    P, m = f["P"], masks or {}
    one = lambda k: m[k].to(dtype) if k in m else 1.0
    args = args or dict(audio=f["A"]["arg"], visual=f["V"]["arg"], text=f["L"]["arg"])
    y, logits = batch["label"].long(), f["logits"]
    B = logits.shape[0]
    lse = torch.logsumexp(logits, -1)
    loss = (lse - logits.gather(1, y[:, None]).squeeze(1)).sum() / B
    dlog = (torch.softmax(logits, -1) - torch.nn.functional.one_hot(y, logits.shape[1]).to(dtype)) / B
    G = {}

    def lin_bwd(name, dy, xin):
        G[name + ".weight"], G[name + ".bias"] = mm(dy.t(), xin), ops.colsum(dy)
        return mm(dy, P[name + ".weight"])
    dfeat = lin_bwd("netC.fc_out", dlog, f["feat"])
    dz1 = torch.where(f["feat"] > 0, dfeat * one("c1"), torch.zeros_like(dfeat))
    dz0 = lin_bwd("netC.module.3", dz1, f["z0"])
    dz0 = torch.where(f["z0"] > 0, dz0 * one("c0"), torch.zeros_like(dz0))
    dfused = lin_bwd("netC.module.0", dz0, f["fused"])
    dtext = torch.where(f["text"] > 0, dfused[:, 2 * H:], torch.zeros_like(f["text"]))
    dpd = lin_bwd("netL.embd.0", dtext, f["pd"])
    dpooled = dpd * one("text")
    tb = textcnn_bwd(batch["text_feature"], f["L"]["pooled"], args["text"], dpooled, dtype)
    for n, k in enumerate(KS):
        G["netL.conv%d.weight" % (n + 1)] = tb[k][0].reshape(CH, 1, k, -1)
        G["netL.conv%d.bias" % (n + 1)] = tb[k][1]
    for net, key, xk, lo in (("netA", "A", "audio_feature", 0), ("netV", "V", "visual_feature", H)):
        r = lstm_pool_bwd(f[key], batch[xk], P[net + ".rnn.weight_hh_l0"], dfused[:, lo:lo + H], args[net == "netA" and "audio" or "visual"], dtype)
        G[net + ".rnn.weight_ih_l0"], G[net + ".rnn.weight_hh_l0"] = r["dW_ih"], r["dW_hh"]
        G[net + ".rnn.bias_ih_l0"] = G[net + ".rnn.bias_hh_l0"] = r["db"]
    f.update(loss=loss, grads=G, args=args)
    return f


def model_case(name):
    """the golden cases' shapes (tests/golden/make_golden_mmin.py builds the same batches): -> (B, Ta, Tv, Tt, audio zero-from)"""
    return {"mmin_base_a": (5, 13, 6, 7, (13, 4, 1, 9, 13)), "mmin_base_b2": (2, 9, 50, 22, (9, 3))}[name]


def make_batch(name, seed):
    """seeded batch of a model case, batch-first, fp32; audio zero-padded as MMINBaseCollate pads"""
    B, Ta, Tv, Tt, zf = model_case(name)
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, Ta, AUDIO_D, generator=g)
    for b, z in enumerate(zf):
        a[b, z:] = 0.0
    return dict(audio_feature=a, visual_feature=torch.randn(B, Tv, VISUAL_D, generator=g),
                text_feature=torch.randn(B, Tt, TEXT_D, generator=g), label=torch.randint(0, 4, (B, ), generator=g),
                audio_feature_length=torch.tensor(list(zf)))


def ema_step32(ema, p, alpha):
    """csrc/ema.hip in numpy float32: alpha as a float, 1 - alpha from that float in double and rounded, two rounded products and
    a rounded sum"""
    a = np.float32(alpha)
    one_minus = np.float32(1.0 - float(a))
    return torch.from_numpy(a * ema.numpy() + one_minus * p.numpy())


FLOOR = 2.0 ** -24     # one float32 rounding of the quantity itself: a twin cannot deviate less unless it is exact by luck


def twin_bound(q32, q64):
    """bound of a quantity from the twin's deviation: MARGIN x max(rel(twin, float64), one rounding), one significant digit up"""
    return round_up_1(MARGIN * max(rel(q32, q64), FLOOR))


def scan_reference(c):
    """float64 forward, the twin's forward, and the twin's backward on float64's routing: (f64, f32, b32)"""
    keys = ("x", "W_ih", "W_hh", "b_ih", "b_hh")
    with one_thread():
        f64 = lstm_pool_fwd(*(c[k] for k in keys))
        f32 = lstm_pool_fwd(*(c[k] for k in keys), dtype=torch.float32)
        b32 = lstm_pool_bwd(f32, c["x"], c["W_hh"], c["dpool"], f64["arg"], dtype=torch.float32)
    return f64, f32, b32


def cnn_reference(c):
    """float64 forward, the twin's forward, and the twin's backward on float64's routing: (f64, f32, b32)"""
    Ws, bs = [c["W%d" % k] for k in KS], [c["b%d" % k] for k in KS]
    with one_thread():
        f64 = textcnn_fwd(c["x"], Ws, bs)
        f32 = textcnn_fwd(c["x"], Ws, bs, dtype=torch.float32)
        b32 = textcnn_bwd(c["x"], f32["pooled"], f64["arg"], c["dpooled"], dtype=torch.float32)
    return f64, f32, b32
