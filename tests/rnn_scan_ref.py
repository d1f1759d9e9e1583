"""Float64 references of the recurrent scans csrc/lstm.hip (erc_lstm_scan_*, hidden 100) and csrc/gru.hip (erc_gru_scan_*,
CIM, hidden 200, three modalities per launch): plain torch on the CPU, nothing of the kernels' chunking or thread layout.

A case holds its data per (dialogue, step) -- every tensor is [B, T, .] -- and a launch form only decides which buffer row
holds position (b, t) (``layout``).  ``reference`` returns every tensor of the contract of include/ercgraft.h in that
[B, T, .] layout, zero where a dialogue does not run: the outputs and the saved state (Hout, Cst | ghn, gates, Hprev, with a
mask also Hdrop), the gate gradients (dGX, for the GRU also dGH) and the products the callers form from them
(dW_ih = dGX^T X, db_ih, dW_hh[d] = dG^T Hprev[d], db_hh[d]; dG = dGX for the LSTM, dGH for the GRU)."""
import contextlib
import math
import zlib

import numpy as np
import torch

from tests.bcrnn_oracle import gru_scan
from tests.gemm_forms_ref import erc_uniform_np

DX = 16
CLASSES = {"fwd": ("Hout", "Cst", "ghn", "gates", "Hprev", "Hdrop"), "dgate": ("dGX", "dGH"),
           "wgrad": ("dW_ih", "db_ih", "dW_hh0", "dW_hh1", "db_hh0", "db_hh1")}
SPARE = 5            # rows behind node_off[B] in the compact forms: nothing may touch them


def _lens(B, T):
    """ragged lengths, first and last = T, second = 1 (tests/test_gpu_gru100.py)"""
    if B == 1:
        return [T]
    g = torch.Generator().manual_seed(7 + B)
    lens = [int(v) for v in torch.randint(2, T + 1, (B,), generator=g)]
    lens[0], lens[1], lens[B - 1] = T, 1, T
    return lens


EDGES = [1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 40]
UNPACKED_T = (1, 8, 9, 16, 17, 33)
# name -> (cell, lengths, T of the launch)
_SPECS = {
    "edges": ("lstm", EDGES, 40),
    "edges0": ("lstm", EDGES[:7] + [0] + EDGES[7:], 40),         # a slot of length 0 in the middle: node_off repeats
    "b1": ("lstm", [25], 25),
    "workload": ("lstm", _lens(33, 110), 110),
    "long": ("lstm", _lens(5, 300), 300),
    "cap5": ("lstm", [1, 9, 17, 8, 25], 25),                     # erc_lstm_scan_bwd_cap alone: compared bit for bit, no bound
    "gru_ragged": ("gru", [1, 110, 37, 5], 110),
    "gru_empty": ("gru", [3, 0, 8, 1], 8),
    "gru_b33": ("gru", [1 + b % 12 for b in range(33)], 12),
    "gru_clamp": ("gru", [12, 9], 9),                            # T < length: the first dialogue runs 9 of its 12 rows
}
_SPECS.update({"unpacked%d" % T: ("lstm", [T] * 3, T) for T in UNPACKED_T})
LSTM_CASES = ("edges", "edges0", "b1", "workload", "long") + tuple("unpacked%d" % T for T in UNPACKED_T)
GRU_CASES = ("gru_ragged", "gru_empty", "gru_b33", "gru_clamp")
CASES = LSTM_CASES + GRU_CASES


def make_case(name):
    """deterministic inputs at the scale of the existing scan tests: W_hh, b_hh uniform +-0.1, GX = 0.5 randn, a random
    upstream gradient on every position (padded ones included) and X [., 16] to form dW_ih.  The GRU has three modalities:
    a leading dimension of 3 on every tensor.  ``Tc`` is the time extent of the [B, Tc, .] layout (> T only where the launch
    is shorter than a dialogue), ``run`` the steps every dialogue runs."""
    cell, lens, T = _SPECS[name]
    Hh, G = (100, 400) if cell == "lstm" else (200, 600)
    B, Tc = len(lens), max(max(lens), T)
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    lead = () if cell == "lstm" else (3, )
    c = dict(name=name, cell=cell, lens=list(lens), B=B, T=T, Tc=Tc, H=Hh, G=G, run=[min(L, T) for L in lens],
             W_hh=(torch.rand(*lead, 2, G, Hh, generator=g) * 2 - 1) * 0.1, b_hh=(torch.rand(*lead, 2, G, generator=g) * 2 - 1) * 0.1,
             GX=torch.randn(*lead, B, Tc, 2 * G, generator=g) * 0.5, up=torch.randn(*lead, B, Tc, 2 * Hh, generator=g),
             X=torch.randn(*lead, B, Tc, DX, generator=g))
    return c


def layout(form, B, T, lens):
    """-> (rows of every buffer, steps each dialogue runs, row [B, T] of position (b, t), sb, st, lengths, node_off).
    Forms: unpacked padded rows ``time_major`` (row t B + b) and ``batch_major`` (row b T + t), every dialogue runs T steps;
    ``packed_tm`` / ``packed_bm``: the same rows with lengths; ``compact``: row node_off[b] + t, lengths = None;
    ``compact_len``: the same with lengths passed too.  The compact forms have SPARE rows behind node_off[B]; positions
    t >= length have no row there (-1)."""
    bb, tt = torch.arange(B)[:, None], torch.arange(T)[None, :]
    if form in ("compact", "compact_len"):
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        rows = torch.from_numpy(off[:-1])[:, None] + tt
        rows = torch.where(tt < torch.tensor(lens)[:, None], rows, torch.full_like(rows, -1))
        lengths = torch.tensor(lens, dtype=torch.int64) if form == "compact_len" else None
        return int(off[-1]) + SPARE, list(lens), rows, 0, 0, lengths, torch.tensor(off, dtype=torch.int32)
    sb, st = (T, 1) if form in ("batch_major", "packed_bm") else (1, B)
    packed = form.startswith("packed")
    return (B * T, list(lens) if packed else [T] * B, bb * sb + tt * st, sb, st,
            torch.tensor(lens, dtype=torch.int64) if packed else None, None)


# ---------------------------------------------------------------------------------------------------------------- chains
def _sum0(x, radix=8):
    """sum over the leading dimension by elementwise adds alone, in a fixed tree: groups of ``radix`` neighbours summed in
    order, then the group sums likewise (torch's own sum picks its order by instruction set and by how the other dimensions
    divide into vectors)"""
    while x.shape[0] > 1:
        n = x.shape[0]
        if n % radix:
            x = torch.cat([x, x.new_zeros((radix - n % radix, ) + x.shape[1:])])
        x = x.reshape((-1, radix) + x.shape[1:])
        acc = x[:, 0]
        for j in range(1, radix):
            acc = acc + x[:, j]
        x = acc
    return x[0]


def _mm32(a, b):
    """float32 [n, K] @ [K, G] from elementwise arithmetic alone: every product rounded to float32, summed over k by _sum0
    in blocks of k, the blocks in order"""
    n, K = a.shape
    at, block = a.t(), max(8, (1 << 21) // max(1, n * b.shape[1]) // 8 * 8)
    out = a.new_zeros(n, b.shape[1])
    for k0 in range(0, K, block):
        part = _sum0(at[k0:k0 + block, :, None] * b[k0:k0 + block, None, :])
        out = part if k0 == 0 else out + part
    return out


class _MM32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return _mm32(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return (_mm32(g, b.t()) if ctx.needs_input_grad[0] else None, _mm32(a.t(), g) if ctx.needs_input_grad[1] else None)


class ops:
    """matmul, sigmoid and tanh of the chains.  float64: torch's.  float32 (the yardstick): torch hands these three to the
    machine's math libraries, which pick their kernels -- the order of a float32 sum, the polynomial of tanh -- by CPU model,
    and the yardstick of one and the same case then differs from machine to machine (forward class of `gru_ragged`: 7.3e-7
    on one, 4.2e-7 on another); the bounds derived from it must not.  So a float32 product is formed from elementwise
    float32 multiplies and adds in a fixed order (a blocked sum, as inexact as a float32 BLAS), and an activation is evaluated
    in float64 and rounded to float32.  Everything else in the chains is elementwise IEEE arithmetic already."""

    @staticmethod
    def matmul(a, b):
        if a.dtype == torch.float64:
            return a @ b
        return _MM32.apply(a.reshape(-1, a.shape[-1]), b).reshape(a.shape[:-1] + b.shape[-1:])

    @staticmethod
    def colsum(x):
        return x.sum(0) if x.dtype == torch.float64 else _sum0(x)

    @staticmethod
    def sigmoid(x):
        return torch.sigmoid(x) if x.dtype == torch.float64 else torch.sigmoid(x.double()).to(x.dtype)

    @staticmethod
    def tanh(x):
        return torch.tanh(x) if x.dtype == torch.float64 else torch.tanh(x.double()).to(x.dtype)


mm = ops.matmul


def lstm_scan(gx, W_hh, b_hh, mutate=None):
    """scan order: gx [L, n, 400] -> (h [L, n, 100], c [L, n, 100], gates [L, n, 400] post-activation i|f|g|o);
    torch.nn.LSTM, gate order i|f|g|o, h0 = c0 = 0.  ``mutate`` (sensitivity study only): "c0_at_8" takes c_{t-1} as 0 at
    steps s % 8 == 0, s > 0; "swap_fo" exchanges gates f and o."""
    h = c = gx.new_zeros(gx.shape[1], W_hh.shape[1])
    hs, cs, gs = [], [], []
    for s in range(gx.shape[0]):
        i, f, g, o = (gx[s] + mm(h, W_hh.t()) + b_hh).chunk(4, -1)
        if mutate == "swap_fo":
            f, o = o, f
        if mutate == "c0_at_8" and s > 0 and s % 8 == 0:
            c = torch.zeros_like(c)
        i, f, g, o = ops.sigmoid(i), ops.sigmoid(f), ops.tanh(g), ops.sigmoid(o)
        c = f * c + i * g
        h = o * ops.tanh(c)
        hs.append(h), cs.append(c), gs.append(torch.cat([i, f, g, o], -1))
    return torch.stack(hs), torch.stack(cs), torch.stack(gs)


def contract_products(dGX, dGrec, Hprev, X, G, Hh):
    """the weight-gradient products as include/ercgraft.h states them, over all rows given (rows that do not run hold 0)"""
    dGX, dGrec, Hprev, X = (t.reshape(-1, t.shape[-1]) for t in (dGX, dGrec, Hprev, X))
    out = {"dW_ih": mm(dGX.t(), X), "db_ih": ops.colsum(dGX)}
    for d in (0, 1):
        out["dW_hh%d" % d] = mm(dGrec[:, d * G:(d + 1) * G].t(), Hprev[:, d * Hh:(d + 1) * Hh])
        out["db_hh%d" % d] = ops.colsum(dGrec[:, d * G:(d + 1) * G])
    return out


def _reference_one(cell, c, GX, W_hh, b_hh, up, X, run, mask, dtype, mutate):
    B, T, Hh, G = c["B"], c["Tc"], c["H"], c["G"]
    GX, W_hh, b_hh, up, X = (t.to(dtype) for t in (GX, W_hh, b_hh, up, X))
    run_t = torch.tensor(run, dtype=torch.int64)
    halves = {k: [] for k in ("Hout", "s1", "gates", "Hprev")}
    leaves, where = [], []
    for d in (0, 1):
        if d == 1 and mutate == "rev_from_T":        # the reverse direction of every dialogue starts at T - 1, inside the padding
            S = T
            s = torch.arange(S)[:, None]
            tt = (T - 1 - s).expand(S, B)
            valid = tt < run_t[None, :]
        else:
            S = max(run)
            s = torch.arange(S)[:, None]
            valid = s < run_t[None, :]
            tt = s.expand(S, B) if d == 0 else (run_t[None, :] - 1 - s).clamp(min=0)
        bb = torch.arange(B)[None, :].expand(S, B)
        gx = GX[bb, tt, d * G:(d + 1) * G]
        if not gx.requires_grad:
            gx.requires_grad_()
        W, b = W_hh[d], b_hh[d]
        if cell == "lstm":
            h, s1, gates = lstm_scan(gx, W, b, mutate)
            leaves.append(gx)
        else:
            eps = torch.zeros(S, B, G, dtype=dtype, requires_grad=True)
            gxi = gx
            if mutate == "bhn_outside":               # n = tanh(gx_n + r (W_hn h) + b_hn)
                gxi = torch.cat([gx[..., :2 * Hh], gx[..., 2 * Hh:] + b[2 * Hh:]], -1)
                b = torch.cat([b[:2 * Hh], torch.zeros_like(b[2 * Hh:])])
            h = gru_scan(gxi, W, b, eps, ops=ops) if S else gx.new_zeros(0, B, Hh)
            leaves += [gx, eps]
        hprev = torch.cat([h.new_zeros(1, B, Hh), h[:-1]])[:S]
        if cell == "gru":                             # the saved state, from the chain's own h_{t-1}
            with torch.no_grad():
                gh = mm(hprev, W.t()) + b
                r, z = ops.sigmoid(gxi[..., :Hh] + gh[..., :Hh]), ops.sigmoid(gxi[..., Hh:2 * Hh] + gh[..., Hh:2 * Hh])
                s1, gates = gh[..., 2 * Hh:], torch.cat([r, z, ops.tanh(gxi[..., 2 * Hh:] + r * gh[..., 2 * Hh:])], -1)
        ix = (bb[valid], tt[valid])
        where.append(ix + (valid, ))
        for k, v in (("Hout", h), ("s1", s1), ("gates", gates), ("Hprev", hprev)):
            halves[k].append(v.new_zeros(B, T, v.shape[-1]).index_put(ix, v[valid] if k == "Hout" else v.detach()[valid]))
    H = torch.cat(halves["Hout"], -1)
    m = torch.ones_like(H) if mask is None else mask.to(dtype)
    loss = (H * m * up).sum()
    grads = torch.autograd.grad(loss, leaves, retain_graph=True)
    n_l = len(leaves) // 2
    out = {"Hout": H.detach(), "Cst" if cell == "lstm" else "ghn": torch.cat(halves["s1"], -1),
           "gates": torch.cat(halves["gates"], -1), "Hprev": torch.cat(halves["Hprev"], -1), "loss": loss}
    if mask is not None:
        out["Hdrop"] = (H * m).detach()
    for j, k in enumerate(("dGX", "dGH")[:n_l]):
        out[k] = torch.cat([torch.zeros(B, T, G, dtype=dtype).index_put(where[d][:2], grads[n_l * d + j][where[d][2]]) for d in (0, 1)], -1)
    out.update(contract_products(out["dGX"], out["dGX" if cell == "lstm" else "dGH"], out["Hprev"], X, G, Hh))
    return out


def reference(case, mask=None, dtype=torch.float64, run=None, mutate=None):
    """every tensor of the contract in the [B, Tc, .] layout, zero where a dialogue does not run, plus ``loss`` (the scalar
    whose gradients they are, with its graph).  ``mask`` [B, Tc, 2 H]: the inverted-dropout multiplier of the output (0 or
    1 / (1 - p)); the upstream gradient is then the gradient wrt Hdrop.  ``run``: steps per dialogue (default: the case's own;
    the unpacked forms run T everywhere).  The GRU returns a list of three (one per modality)."""
    run = case["run"] if run is None else run
    keys = ("GX", "W_hh", "b_hh", "up", "X")
    with one_thread():
        if case["cell"] == "lstm":
            return _reference_one("lstm", case, *(case[k] for k in keys), run, mask, dtype, mutate)
        return [_reference_one("gru", case, *(case[k][m] for k in keys), run, None if mask is None else mask[m], dtype, mutate)
                for m in range(3)]


# ----------------------------------------------------------------------------------------------------- errors and bounds
def rel(x, want):
    """max |x - want| relative to max |want| (absolute where the reference is identically zero)"""
    x, want = x.double(), want.double()
    if want.numel() == 0:
        return 0.0
    scale = float(want.abs().max())
    return float((x - want).abs().max()) / (scale if scale > 0 else 1.0)


def class_errors(got, ref):
    """per tensor class, max|got - ref| / max|ref| of the worst tensor of the class (and modality)"""
    got, ref = (x if isinstance(x, (list, tuple)) else [x] for x in (got, ref))
    return {cls: max(rel(g[k], w[k]) for g, w in zip(got, ref) for k in names if k in w and k in g)
            for cls, names in CLASSES.items()}


def round_up_1(x):
    """x rounded up to one significant digit"""
    if x <= 0:
        return 0.0
    p = 10.0 ** math.floor(math.log10(x))
    return float("%.0e" % (math.ceil(x / p - 1e-9) * p))


def yardstick(case):
    """the reference in float32 against itself in float64, per class: it measures the reference, never a kernel"""
    return class_errors(reference(case, dtype=torch.float32), reference(case))


def bound(y):
    """4 x the yardstick, rounded up to one significant digit (the rule of tests/test_gpu_dag_rec.py)"""
    return round_up_1(4.0 * y)


@contextlib.contextmanager
def one_thread():
    """thousands of small dependent operations: a thread pool only slows them down"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


# --------------------------------------------------------------------------------------------------------------- dropout
def drop_mask(case, form, p, rng, rng_stream):
    """the elements the kernels keep, predicted from csrc/erc_common.h erc_uniform: bool [B, Tc, 2 H] (the GRU: [3, ...]).
    LSTM: element (row, d, u) is kept iff uniform(seed = rng[1] ^ rng_stream, offset = rng[0], idx = row 200 + d 100 + u) >= p,
    row being the buffer row of the form; CIM GRU (compact rows): seed = rng[1] ^ (rng_stream + m), idx = row 400 + d 200 + u.
    Positions without a row are False."""
    Hh = case["H"]
    rows = layout(form, case["B"], case["Tc"], case["lens"])[2]
    idx = (rows.clamp(min=0).numpy().astype(np.uint64)[:, :, None] * np.uint64(2 * Hh) + np.arange(2 * Hh, dtype=np.uint64))
    has_row = (rows >= 0)[:, :, None]
    mask64 = (1 << 64) - 1

    def keep(stream):
        u = erc_uniform_np(np.uint64((int(rng[1]) ^ stream) & mask64), int(rng[0]), idx)
        return torch.from_numpy(u >= np.float32(p)) & has_row
    if case["cell"] == "lstm":
        return keep(int(rng_stream))
    return torch.stack([keep((int(rng_stream) + m) & mask64) for m in range(3)])
