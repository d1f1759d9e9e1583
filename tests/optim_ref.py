"""Float64 restatements of the shared optimizer tail (csrc/optim.hip, csrc/optim_dev.h, csrc/ema.hip): the Adam / AdamW step,
the gradient norm and the closed-form allowance for bias corrections computed in float; their float32 twins, the case tables
and the bounds of tests/test_optim_ref.py and tests/test_gpu_optim.py.  Written from torch/optim/adam.py's single-tensor path,
in plain torch on the CPU; nothing of the kernel's quads, passes or grid.

Math.  With g' = g * grad_scale * min(1, clip_norm / (gnorm + 1e-6)) (the min only when clip_norm > 0; gnorm is an INPUT):
  Adam:  g' += wd p          AdamW:  p *= 1 - lr wd
  m = b1 m + (1 - b1) g',  v = b2 v + (1 - b2) g'^2
  u = lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps),  p -= u
lr, b1, b2, eps, wd and grad_scale are rounded to float32 first: the C ABI takes floats, so 0.999 arrives as 0.999f and a
reference that used the double 0.999 would differ by 1.7e-5 in 1 - b2^t without any kernel being wrong.  The bias corrections
1 - b^t themselves are evaluated in double, in float64 and in the twin alike (torch computes them in Python floats).

Bounds.  tests/mmin_ref.py's rule: a quantity's bound is twin_bound = MARGIN x max(rel(twin, float64), 2^-24) rounded up to one
digit, errors relative to the quantity's largest float64 magnitude.  The update additionally gets bc_term (below), because the
kernel evaluates b^t with powf in float and the twin does not.  A kernel's measured figure never enters a bound;
tests/test_gpu_optim.py prints the live figures next to the twin's.
"""
import math
import zlib

import numpy as np
import torch

from tests.mmin_ref import FLOOR, MARGIN, ema_step32, one_thread, rel, round_up_1, twin_bound  # noqa: F401

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8

# ---------------------------------------------------------------------------------------------------------- case tables
# block 1: one step at every launch shape (the grid is min(512, ceil(n / 4 / 256)) workgroups of 256 quads)
SIZES = (1, 2, 3, 4, 5, 7, 1027, 524288, 524292, 524295, 1049607)
# block 2: name -> (decoupled, wd, grad_scale, clip_norm as a multiple of the true norm (0: no clipping))
OPTIONS = {
    "adam":          (False, 0.0, 1.0, 0.0),
    "adam_l2":       (False, 3e-5, 1.0, 0.0),
    "adamw":         (True, 1e-2, 1.0, 0.0),
    "adam_scale":    (False, 0.0, 0.25, 0.0),
    "adam_l2_clip":  (False, 3e-5, 1.0, 0.5),       # clipping bites: coefficient ~0.5
    "adamw_noclip":  (True, 1e-2, 0.25, 2.0),       # it does not: coefficient ~2, the gradient stays as it is
    "adamw_clip":    (True, 1e-2, 0.25, 0.5),
}
OPTION_SIZES = (1027, 524295)
# block 3: step counts reached without running the steps
STEP_COUNTS = (1, 2, 10, 1000, 100000)
STEP_N = (4099, 1027)         # the launch under test, and the follow-up launch with another grid
CHAIN_N, CHAIN_STEPS = 4099, 5
# grad norm: the grid is min(512, ceil(n / 256)) workgroups: one thread, one short and one over a workgroup, exactly one pass of
# the full grid, one element and a ragged piece of a second pass
NORM_SIZES = (1, 255, 257, 131072, 131073, 200003)
NORM_SCALES = (1.0, 1.0 / 3.0)
# name -> (n, log10 of the smallest and largest magnitude): squares of the first overflow float32 when summed, squares of the
# second underflow to 0 in float32
NORM_WIDE = {"wide": (200003, -25.0, 18.0), "tiny": (4099, -25.0, -23.5)}
EMA_SIZES = (1, 3, 5, 1027, 524295)


def _gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()))


def f32(x):
    """a Python float rounded to float32, as the C ABI receives it"""
    return float(np.float32(x))


def group(n):
    """element i belongs to group i % 3: 0: p = 0 exactly, 1: |p| ~ lr, 2: |p| ~ 1.  Interleaved, so that every group falls into
    every pass of the grid and into the scalar tail"""
    return torch.arange(n) % 3


def adam_case(tag, n, with_moments=False):
    """p in three interleaved groups; g = +-10^U(-6, 2) with one element in eight exactly 0; moments 0, or (with_moments) of the
    size a running optimizer holds: m ~ g, v ~ g^2, non-zero where g is 0 too"""
    gen = _gen("optim-" + tag)
    grp = group(n)
    p = torch.randn(n, generator=gen)
    p = torch.where(grp == 0, torch.zeros(n), torch.where(grp == 1, p * LR, p))
    mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 8.0 - 6.0)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    g = (mag * sign).float()
    g[torch.rand(n, generator=gen) < 0.125] = 0.0
    m, v = torch.zeros(n), torch.zeros(n)
    if with_moments:
        m = (g.double() * (0.5 + torch.rand(n, generator=gen).double()) + 1e-4 * torch.randn(n, generator=gen).double()).float()
        v = (g.double() ** 2 * (0.5 + torch.rand(n, generator=gen).double()) + 1e-10).float()
    return dict(p=p, g=g, m=m, v=v, grp=grp)


# ------------------------------------------------------------------------------------------------------------ Adam / AdamW
def _adam(p, g, m, v, t, lr, b1, b2, eps, wd, decoupled, grad_scale, clip_norm, gnorm, dtype):
    lr, b1, b2, eps, wd, gs = (f32(x) for x in (lr, b1, b2, eps, wd, grad_scale))
    if clip_norm > 0:
        if dtype == torch.float64:
            coef = f32(clip_norm) / (f32(gnorm) + 1e-6)
        else:
            coef = float(np.float32(clip_norm) / (np.float32(gnorm) + np.float32(1e-6)))
        if coef < 1.0:
            gs = gs * coef if dtype == torch.float64 else float(np.float32(gs) * np.float32(coef))
    P, G, M, V = (x.to(dtype) for x in (p, g, m, v))
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t              # in double, twin included
    step_size, bc2_sqrt = lr / bc1, math.sqrt(bc2)
    if decoupled:
        P = P * (1.0 - lr * wd)
    G = G * gs
    if wd != 0 and not decoupled:
        G = G + wd * P
    M = b1 * M + (1.0 - b1) * G
    V = b2 * V + (1.0 - b2) * G * G
    denom = V.sqrt() / bc2_sqrt + eps
    U = step_size * M / denom
    return P - U, M, V, U


def adam_step64(p, g, m, v, t, lr, b1, b2, eps, wd, decoupled, grad_scale, clip_norm, gnorm):
    """one step of torch's single-tensor Adam (decoupled: AdamW) in float64 on the fp32 inputs -> (p, m, v, u), u the update
    that was subtracted.  Clipping is the kernel's contract: g is multiplied by clip_norm / (gnorm + 1e-6) only when that is
    below 1, and gnorm is an input (the device's, in the GPU tests)"""
    return _adam(p, g, m, v, t, lr, b1, b2, eps, wd, decoupled, grad_scale, clip_norm, gnorm, torch.float64)


def adam_step32(p, g, m, v, t, lr, b1, b2, eps, wd, decoupled, grad_scale, clip_norm, gnorm):
    """the twin: the same expression on float32 tensors, the clip coefficient in float32, the bias corrections in double"""
    return _adam(p, g, m, v, t, lr, b1, b2, eps, wd, decoupled, grad_scale, clip_norm, gnorm, torch.float32)


def bc_term(b1, b2, t):
    """What computing the two bias corrections in float (powf, csrc/optim_dev.h AdamCoef::init) may add to the update's
    relative error, on top of the twin's deviation: 2^-23 (b1^t / (1 - b1^t) + 1/2 b2^t / (1 - b2^t)).

    q = b^t from powf is good to one unit in the last place of a value <= 1, |dq| <= 2^-23 q (the exponent t < 2^24 converts
    exactly).  bc = 1 - q: exact for q >= 1/2 (Sterbenz); below that it costs one rounding, 2^-24 bc, which is one of the
    roundings MARGIN already covers.  So |d bc| / bc <= 2^-23 q / (1 - q).  The update holds lr / bc1, which carries bc1's
    relative error, and 1 / sqrt(bc2), which carries half of bc2's (the +eps only shrinks it).  Nothing here is measured on a
    kernel.  The term is largest at t = 1 (6.1e-5 for 0.9 / 0.999), although powf(b, 1) = b is exact there: the allowance is for
    any powf within its specification, not for this one."""
    q1, q2 = f32(b1) ** t, f32(b2) ** t
    return 2.0 ** -23 * (q1 / (1.0 - q1) + 0.5 * q2 / (1.0 - q2))


def update_bound(u32, u64, b1, b2, t):
    """bound of the update on the p = 0 group (where p_out = -u): the twin's, plus the float bias corrections'"""
    return twin_bound(u32, u64) + bc_term(b1, b2, t)


def others_allowance(p64_out, u64, bound0):
    """elementwise allowance for |p_out - p64_out| where p != 0: MARGIN roundings of the result itself (the decay product and
    the final subtraction are two) plus the element's own update |u64| times the bound of the p = 0 group"""
    return MARGIN * FLOOR * p64_out.abs() + u64.abs() * bound0


# ------------------------------------------------------------------------------------------------------------- grad norm
def norm_case(tag, n, lo=None, hi=None):
    gen = _gen("norm-" + tag)
    if lo is None:
        return torch.randn(n, generator=gen)
    mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * (hi - lo) + lo)
    return (mag * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()).float()


def grad_norm64(g, scale):
    """sqrt(sum fl32(g * scale)^2) in float64: the product is the kernel's contract (one float32 rounding), the rest exact"""
    x = (g.float() * torch.tensor(scale, dtype=torch.float32)).double()
    return float(x.pow(2).sum().sqrt())


def grad_norm32(g, scale):
    """the twin: torch's float32 norm of the same products.  The products are first scaled by a power of two that brings the
    largest to [1, 2) -- exact, and without it the twin of NORM_WIDE's cases is inf or 0 and bounds nothing"""
    x = g.float() * torch.tensor(scale, dtype=torch.float32)
    top = float(x.abs().max())
    if top == 0.0:
        return 0.0
    e = math.floor(math.log2(top))
    lo, hi = e // 2, e - e // 2                     # two steps: 2^e itself may lie outside float32's range
    y = (x.double() * 2.0 ** -lo * 2.0 ** -hi).float()       # exact unless the element drops below 2^-149 of the largest
    with one_thread():                              # torch sums per thread: one thread, one figure
        return float(y.norm().double() * 2.0 ** lo * 2.0 ** hi)


def norm_bound(g, scale):
    want = grad_norm64(g, scale)
    return twin_bound(torch.tensor(grad_norm32(g, scale)), torch.tensor(want))
