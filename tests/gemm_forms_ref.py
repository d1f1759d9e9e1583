"""Case table, operands and float64 expectations of the two streaming GEMM entry points (csrc/gemm_stream.hip:
erc_gemm_f32_stream, erc_gemm_bf16a_stream), shared by the host tests (tests/test_gemm_forms_ref.py) and the GPU tests
(tests/test_gpu_gemm_forms.py).  numpy and torch on the CPU: nothing here touches a GPU.

WHICH KERNEL.  Behind each entry point the host picks a template instantiation; erc_gemm_f32_stream_form and
erc_gemm_bf16a_stream_form report the pick without launching.  `f32_form` / `bf_form` restate the pick for a case of the table:
    erc_gemm_f32_stream    (a_mode, b_mode, nw, gather_a, gather_b, vec, rm, cf): layout NT / NN / TN; nw from the 16-deep K blocks
                           per split (>= 32: 8, >= 6: 4, else 1); vec = every K-contiguous operand 16-byte aligned with ld % 4 == 0
                           (TN is built scalar only); the 32 x 64 big tile (rm, cf = 2, 4, nw 4) for ungathered NT vec at nw 8,
                           K >= 4096, M >= 2048, N >= 64 (the virtual ones line counted).
    erc_gemm_bf16a_stream  (kernel, nw, w_is_bf16, ub, a_vec, b_vec): nw from the 32-deep K blocks (>= 16: 8, >= 4: 4, else 1); access
                           widths from alignment and pitch; the persistent kernel (1, 8, 1, 6, 1, 1) for bf16 W, M >= 1024,
                           N <= 128, 32 <= K <= 1536, K, ldx, ldw multiples of 4, both operands 8-byte aligned.
The host tests compare the set of forms the table reaches with a literal list, so a threshold that moves makes a test fail.

EXACT OPERANDS.  A, B, bias, the old C and aux are integers in [-3, 3], act_scale = 2 and drop_p = 0.5: every product and every
partial sum, in any order, is an integer of magnitude <= 9 K + 6 < 2^24 (K <= 16 890 here), exact in fp32 -- and 3 is exact in bf16.
The kernel's result therefore has to EQUAL the float64 one; no tolerance exists.  The host tests prove the premise per case
(`mag` < 2^24, and the float32 CPU product equals the float64 one).

POISON.  Every operand is stored with NaN wherever the call has no business reading: columns K .. ld - 1 of a K-contiguous
operand, rows / columns past M, N or K, the rows of a gather source that no index names, the index entries past the last one
(they name a NaN row), the tails of bias and aux.  Outputs are NaN before the launch, pitch N + 3 and two extra rows; after it the
written rectangle has to equal the expectation and everything else still be NaN.  A stray read makes a NaN; nothing has to fault.

REAL-VALUED CASES catch what integers cannot (accumulation at reduced precision).  Bound per element, derived, never measured:
    |got - ref64| <= (K + NW + 3) 2^-23 (|A| |B| + |bias| + |C_old|)
the any-order forward error bound of K fp32 multiply-adds plus the NW-way reduction and the epilogue's additions, with unit
2^-23 instead of 2^-24 so that a matrix core that truncates internally still passes.  Products of two bf16 values are exact in
fp32, so the bf16 kernels are held to the same bound.
"""
import numpy as np
import torch

NAN = float("nan")
BASE = 1 << 20            # a 16-byte aligned stand-in address for the host-side form queries (nothing is dereferenced)
RNG = (7, 12345)          # {offset, seed} of the act-3 mask
ACT_SCALE, DROP_P = 2.0, 0.5
LAYOUT = {"NT": (0, 0), "NN": (0, 1), "TN": (1, 1)}       # (a_kmajor, b_kmajor)
K_OF_NW = {1: 37, 4: 213, 8: 533}                          # one K per wavefront count (f32)
BF_K_OF_NW = {1: 77, 4: 205, 8: 525}                       # (bf16a)


def cdiv(a, b):
    return -(-a // b)


def erc_uniform_np(seed, offset, idx):
    """csrc/erc_common.h erc_uniform on numpy uint64 arrays."""
    u = np.uint64
    with np.errstate(over="ignore"):
        z = u(seed) ^ (u(offset) * u(0x9E3779B97F4A7C15)) ^ ((idx.astype(np.uint64) + u(0xD1B54A32D192ED03)) * u(0xBF58476D1CE4E5B9))
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        z = z ^ (z >> u(31))
    return (z >> u(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def keep_mask(M, N):
    """act 3: element (row, col) of an [M, N] product is kept iff erc_uniform(seed, offset, row N + col) >= drop_p"""
    idx = np.arange(M * N, dtype=np.uint64)
    return torch.from_numpy(erc_uniform_np(np.uint64(RNG[1]), RNG[0], idx) >= np.float32(DROP_P)).view(M, N)


def _draw(gen, shape, c):
    if c.get("real"):
        return torch.randn(shape, generator=gen)
    lo = 1 if c.get("positive") else -3
    return torch.randint(lo, 4, shape, generator=gen).float()


def _gather_index(gen, n, n_src):
    """n source rows out of n_src, out of order and with a repeat; tail entries name a row that no index names"""
    idx = torch.randint(0, n_src, (n,), generator=gen)
    if n >= 2:
        idx[1] = idx[0]
    if n >= 3 and bool((idx[1:] >= idx[:-1]).all()):
        idx[-1], idx[0] = idx[0].clone(), idx[-1].clone()
    unused = torch.ones(n_src, dtype=torch.bool)
    unused[idx] = False
    pad = int(torch.nonzero(unused)[0])
    return idx, unused, torch.cat([idx, torch.full((4,), pad)]).int()


def _stored(vals, ld, off, dtype=torch.float32):
    """vals [R, C] inside a NaN block of R + 2 rows of pitch ld that starts `off` elements into its allocation"""
    R, Cn = vals.shape
    st = torch.full((off + (R + 2) * ld + 8,), NAN, dtype=dtype)
    st[off:off + (R + 2) * ld].view(R + 2, ld)[:R, :Cn] = vals.to(dtype)
    return st


# =============================================================================================== erc_gemm_f32_stream
def f32_nw(K, split=1):
    kbs = cdiv(cdiv(K, 16), split)
    return 8 if kbs >= 32 else (4 if kbs >= 6 else 1)


def f32case(layout, M, N, K, ga=False, gb=False, vec=True, mis="a_ptr", split=1, ones=0, bias=False, act=0, acc=False,
            positive=False, real=False, seed=0):
    """`vec`: build the K-contiguous operands 16-byte accessible; if not, `mis` says what breaks it (a_ptr / b_ptr: a pointer
    one element off, a_ld / b_ld: a pitch with ld % 4 == 1)."""
    assert layout in LAYOUT and not (ga and layout == "TN") and not (gb and layout == "NT")
    assert split == 1 or not (bias or act or acc)
    return dict(layout=layout, M=M, N=N, K=K, ga=ga, gb=gb, vec=vec, mis=mis, split=split, ones=ones, bias=bias, act=act,
                acc=acc, positive=positive, real=real, seed=seed + 7919 * M + 104729 * N + 31 * K)


def f32_form(c):
    a_k, b_k = LAYOUT[c["layout"]]
    nw = f32_nw(c["K"], c["split"])
    vec = int(c["vec"] and c["layout"] != "TN")
    Ml, Nl = c["M"] + (c["ones"] == 2), c["N"] + (c["ones"] == 1)
    if c["layout"] == "NT" and not c["ga"] and vec and nw == 8 and c["K"] >= 4096 and Ml >= 2048 and Nl >= 64:
        return (0, 0, 4, 0, 0, 1, 2, 4)
    return (a_k, b_k, nw, int(c["ga"]), int(c["gb"]), vec, 1, 2)


def f32_operands(c):
    """CPU tensors of a case: the stored operands (1-D allocations), their element offsets and pitches, the logical float64
    A [M, K] and B [K, N], and the outputs as they are before the launch."""
    gen = torch.Generator().manual_seed(c["seed"])
    M, N, K, S = c["M"], c["N"], c["K"], c["split"]
    a_k, b_k = LAYOUT[c["layout"]]
    o = dict(ia=None, ib=None, bias=None, aux=None, bias_out=None, rng=None)
    k4 = cdiv(K, 4) * 4

    def kcontig(rows, name, gathered):
        vec = c["vec"] or c["mis"][0] != name
        ld = k4 + (5 if (not vec and c["mis"] == name + "_ld") else 4)
        off = 1 if (not vec and c["mis"] == name + "_ptr") else 0
        n_src = rows + 5 if gathered else rows
        vals = _draw(gen, (n_src, K), c)
        idx = None
        if gathered:
            idx, unused, o["i" + name] = _gather_index(gen, rows, n_src)
            vals[unused] = NAN
        return _stored(vals, ld, off), ld, off, (vals[idx] if gathered else vals).double()

    if a_k == 0:
        o["A"], o["lda"], o["a_off"], o["A64"] = kcontig(M, "a", c["ga"])
    else:                                   # K-major A [K, M]
        vals = _draw(gen, (K, M), c)
        o["A"], o["lda"], o["a_off"], o["A64"] = _stored(vals, M + 3, 0), M + 3, 0, vals.t().double()
    if b_k == 0:
        o["B"], o["ldb"], o["b_off"], B64 = kcontig(N, "b", False)
        o["B64"] = B64.t()
    else:                                   # K-major B [K, N], rows optionally gathered
        n_src = K + 5 if c["gb"] else K
        vals = _draw(gen, (n_src, N), c)
        idx = None
        if c["gb"]:
            idx, unused, o["ib"] = _gather_index(gen, K, n_src)
            vals[unused] = NAN
        o["B"], o["ldb"], o["b_off"], o["B64"] = _stored(vals, N + 3, 0), N + 3, 0, (vals[idx] if c["gb"] else vals).double()
    o["C"] = torch.full((S, M + 2, N + 3), NAN)
    o["C_old"] = torch.zeros(M, N, dtype=torch.float64)
    if c["acc"]:
        o["C"][0, :M, :N] = _draw(gen, (M, N), c)
        o["C_old"] = o["C"][0, :M, :N].double()
    o["bias64"] = torch.zeros(N, dtype=torch.float64)
    if c["bias"]:
        b = _draw(gen, (N,), c)
        o["bias"], o["bias64"] = torch.cat([b, torch.full((2,), NAN)]), b.double()
    if c["act"] == 2:
        aux = torch.randint(-3, 4, (M, N), generator=gen).float()
        o["aux"], o["aux64"] = _stored(aux, N + 5, 0), aux.double()
    if c["act"] == 3:
        o["rng"] = torch.tensor(RNG, dtype=torch.int64)
    if c["ones"]:
        o["bias_out"] = torch.full((S, (M if c["ones"] == 1 else N) + 2), NAN)
    return o


def f32_args(c, o, addr):
    """positional arguments of capi.gemm_f32_stream / gemm_f32_stream_form; addr(name) = address of allocation o[name]"""
    a_k, b_k = LAYOUT[c["layout"]]
    M, N = c["M"], c["N"]

    def at(name, off=0):
        return None if o[name] is None else addr(name) + 4 * off
    return (at("A", o["a_off"]), o["lda"], a_k, at("ia"), at("B", o["b_off"]), o["ldb"], b_k, at("ib"), at("C"), N + 3, M, N,
            c["K"], c["split"], (M + 2) * (N + 3), c["ones"], at("bias_out"), (o["bias_out"].shape[1] if c["ones"] else 0),
            at("bias"), c["act"], at("aux"), N + 5, ACT_SCALE, DROP_P, at("rng"), int(c["acc"]))


def host_addr(o):
    """stand-in addresses for a host-side form query: every allocation 16-byte aligned, as the GPU allocator's are"""
    names = sorted(k for k, v in o.items() if isinstance(v, torch.Tensor))
    return lambda name: BASE * (1 + names.index(name))


def f32_expected(c, o):
    """float64: C [S, M, N], bias_out [S, M or N] (or None), and mag [M, N] = |A| |B| + |bias| + |C_old| (whole K)"""
    M, N, K, S = c["M"], c["N"], c["K"], c["split"]
    A, B = o["A64"], o["B64"]
    kbs = cdiv(cdiv(K, 16), S)
    Cs, bos = [], []
    for z in range(S):
        k0, k1 = min(K, z * kbs * 16), min(K, (z + 1) * kbs * 16)
        Cs.append(A[:, k0:k1] @ B[k0:k1])
        bos.append(A[:, k0:k1].sum(1) if c["ones"] == 1 else B[k0:k1].sum(0))
    v = torch.stack(Cs)
    if S == 1:
        v = v + o["bias64"] + o["C_old"]
        if c["act"] == 1:
            v = torch.relu(v)
        elif c["act"] == 2:
            v = torch.where(o["aux64"] > 0, v * ACT_SCALE, torch.zeros((), dtype=torch.float64))
        elif c["act"] == 3:
            v = torch.where(keep_mask(M, N), torch.relu(v) * ACT_SCALE, torch.zeros((), dtype=torch.float64))
    mag = A.abs() @ B.abs() + o["bias64"].abs() + o["C_old"].abs()
    return v, (torch.stack(bos) if c["ones"] else None), mag


def error_bound(K, nw, mag):
    return (K + nw + 3) * 2.0 ** -23 * mag


def check_written(got, exp, what, bound=None):
    """got [.., R + pad, C + pad] float32 as the launch left it, exp [.., R, C] float64: the rectangle equals the expectation
    (or lies within `bound`), everything else is still NaN.  Returns the worst error / bound (0 for exact cases)."""
    R, Cn = exp.shape[-2:]
    inner = got[..., :R, :Cn].double()
    rest = torch.ones(got.shape, dtype=torch.bool)
    rest[..., :R, :Cn] = False
    assert bool(torch.isnan(got[rest]).all()), "%s: written outside its rectangle" % what
    assert not bool(torch.isnan(inner).any()), "%s: NaN in the result (unwritten, or a stray read)" % what
    if bound is None:
        bad = torch.nonzero(inner != exp)
        assert bad.numel() == 0, "%s: %d wrong elements, first at %s: got %r want %r" % (
            what, len(bad), tuple(bad[0].tolist()), float(inner[tuple(bad[0])]), float(exp[tuple(bad[0])]))
        return 0.0
    frac = ((inner - exp).abs() / bound.clamp_min(1e-300)).max()
    assert float(frac) <= 1.0, "%s: error %.3f x the derived bound" % (what, float(frac))
    return float(frac)


def f32_check(c, o, got_C, got_bo):
    """what a launch of case c left in C [S, M + 2, N + 3] and bias_out [S, L + 2] against the float64 expectation"""
    exp, exp_bo, mag = f32_expected(c, o)
    what = "f32 %s" % (c,)
    nw = f32_form(c)[2]
    frac = check_written(got_C, exp, what, error_bound(c["K"], nw, mag) if c["real"] else None)
    if c["ones"]:
        bmag = (o["A64"].abs().sum(1) if c["ones"] == 1 else o["B64"].abs().sum(0))
        check_written(got_bo[:, None, :], exp_bo[:, None, :], what + " bias_out",
                      error_bound(c["K"], nw, bmag)[None, None, :] if c["real"] else None)
    return frac


# ---- the table
def _f32_base_forms():
    """(layout, ga, gb, vec) of the 14 base forms, with what breaks vector access in the scalar ones"""
    out = []
    for ga in (False, True):
        for vec in (True, False):
            out.append(("NT", ga, False, vec))
    for ga in (False, True):
        for gb in (False, True):
            for vec in (True, False):
                out.append(("NN", ga, gb, vec))
    for gb in (False, True):
        out.append(("TN", False, gb, False))
    return out


_MIS = {"NT": ("a_ptr", "b_ld", "a_ld", "b_ptr"), "NN": ("a_ld", "a_ptr"), "TN": ("a_ptr",)}
BIG_EVERY = ("NT", 2049, 65, 4100)


def f32_every_form(real=False):
    """all 43 forms once at tile-edge sizes (M % 16 in {1, 15}, N % 32 in {1, 17, 31}); real = the randn twins, with bias and
    accumulate so that every term of the bound is present"""
    cases, i = [], 0
    extra = dict(real=True, bias=True, acc=True) if real else {}
    for layout, ga, gb, vec in _f32_base_forms():
        for nw in (1, 4, 8):
            mis = _MIS[layout][i % len(_MIS[layout])]
            cases.append(f32case(layout, (17, 31)[i % 2], (33, 49, 63)[i % 3], K_OF_NW[nw], ga, gb, vec, mis, seed=i, **extra))
            i += 1
    layout, M, N, K = BIG_EVERY
    cases.append(f32case(layout, M, N, K, seed=i, **extra))
    return cases


SWEEP_LAYOUTS = ("NT", "NN", "TN")      # ungathered, vector access where the layout has it: every K of 1 .. SWEEP_K
SWEEP_K, SWEEP_M, SWEEP_N, SWEEP_LD = 1100, 17, 33, 1104
OTHER_K = {1: (1, 15, 16, 17, 80), 4: (81, 96, 111, 250, 496), 8: (497, 512, 527, 800, 1100)}


def f32_sweep_case(layout, K):
    return f32case(layout, SWEEP_M, SWEEP_N, K)


def f32_sweep_blocks():
    """A [M, SWEEP_K] and B [SWEEP_K, N] integer blocks (every K uses their leading K) and the float64 products of every K"""
    gen = torch.Generator().manual_seed(1100)
    A = torch.randint(-3, 4, (SWEEP_M, SWEEP_K), generator=gen).float()
    B = torch.randint(-3, 4, (SWEEP_K, SWEEP_N), generator=gen).float()
    return A, B


def prefix_products(A, B, dtype=torch.float64):
    """[K, M, N]: entry K - 1 = A[:, :K] B[:K]"""
    return torch.cumsum(A.to(dtype).t()[:, :, None] * B.to(dtype)[:, None, :], 0)


def f32_other_k():
    """the forms the K sweep leaves out, at five K per wavefront count (K % 16 in {0, 1, 15} among them)"""
    cases, i = [], 0
    for layout, ga, gb, vec in _f32_base_forms():
        if not ga and not gb and (vec or layout == "TN"):
            continue
        for nw in (1, 4, 8):
            for K in OTHER_K[nw]:
                mis = _MIS[layout][i % len(_MIS[layout])]
                cases.append(f32case(layout, SWEEP_M, SWEEP_N, K, ga, gb, vec, mis, seed=i))
                i += 1
    return cases


EDGE_M = (1, 15, 16, 17, 31, 32, 33)
EDGE_N = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65)


def f32_tile_edges(layout, nw):
    return [f32case(layout, M, N, K_OF_NW[nw], ones=ones, seed=nw) for M in EDGE_M for N in EDGE_N for ones in (0, 1, 2)]


def f32_split_cases():
    """split_k 2, 3, 5, and splits whose LAST piece gets no K block at every wavefront count: (K, S) = (100, 5): 7 blocks in
    pieces of 2; (520, 8): 33 in pieces of 5; (780, 8): 49 in pieces of 7; (16890, 34): 1056 in pieces of 32."""
    cases = []
    for layout in LAYOUT:
        for K, S in ((1100, 2), (1100, 3), (1100, 5), (300, 2), (70, 3), (100, 5), (520, 8), (780, 8), (16890, 34)):
            for ones in ((0, 1, 2) if layout == "TN" else ((K + S) % 3,)):
                cases.append(f32case(layout, 17, 33, K, split=S, ones=ones, seed=S))
    return cases


def has_empty_last_split(c):
    nkb = cdiv(c["K"], 16)
    return cdiv(nkb, c["split"]) * (c["split"] - 1) >= nkb


EPILOGUES = (dict(bias=True), dict(act=1), dict(act=2), dict(act=3, positive=True), dict(acc=True), dict(bias=True, act=1),
             dict(bias=True, acc=True), dict(act=1, acc=True), dict(bias=True, act=2, acc=True), dict(bias=True, act=3, acc=True))


def f32_epilogue_cases():
    return [f32case(layout, 31, 49, K_OF_NW[nw], seed=i, **e) for layout in LAYOUT for nw in (1, 4, 8)
            for i, e in enumerate(EPILOGUES)]


def f32_big_cases():
    """the smallest shapes that select the 32 x 64 tile, one of them in two K pieces"""
    return [f32case("NT", 2048, 64, 4096), f32case("NT", 2063, 70, 4117), f32case("NT", 2047, 64, 4112, ones=2),
            f32case("NT", 2050, 63, 4096, ones=1), f32case("NT", 2048, 64, 8200, split=2)]


def f32_integer_cases():
    """every integer case but the K sweep"""
    cases = f32_every_form() + f32_other_k() + f32_split_cases() + f32_epilogue_cases() + f32_big_cases()
    for layout in LAYOUT:
        for nw in (1, 4, 8):
            cases += f32_tile_edges(layout, nw)
    return cases


F32_FORMS = frozenset(
    [(0, 0, nw, ga, 0, vec, 1, 2) for nw in (1, 4, 8) for ga in (0, 1) for vec in (0, 1)] +
    [(0, 1, nw, ga, gb, vec, 1, 2) for nw in (1, 4, 8) for ga in (0, 1) for gb in (0, 1) for vec in (0, 1)] +
    [(1, 1, nw, 0, gb, 0, 1, 2) for nw in (1, 4, 8) for gb in (0, 1)] + [(0, 0, 4, 0, 0, 1, 2, 4)])


# ============================================================================================= erc_gemm_bf16a_stream
A_SEL = (2, 1, 4, 0, "off")                 # access width the stored operand allows; "off": pitch fine, pointer one element off
B_SEL = {True: (2, 1, 4, 0, "off"), False: (1, 3, 0, "off")}
_PITCH = {True: {2: 8, 1: 12, 4: 10, 0: 9, "off": 8}, False: {1: 8, 3: 10, 0: 9, "off": 8}}   # ld = 8 ceil(K / 8) + this


def bf_nw(K):
    nkb = cdiv(K, 32)
    return 8 if nkb >= 16 else (4 if nkb >= 4 else 1)


def bfcase(M, N, K, wb, a_sel=2, b_sel=None, gather=False, bias=False, act=0, real=False, seed=0):
    b_sel = B_SEL[wb][0] if b_sel is None else b_sel
    assert a_sel in A_SEL and b_sel in B_SEL[wb]
    return dict(M=M, N=N, K=K, wb=wb, a_sel=a_sel, b_sel=b_sel, gather=gather, bias=bias, act=act, real=real,
                seed=seed + 7919 * M + 104729 * N + 31 * K)


def bf_pitches(c):
    k8 = cdiv(c["K"], 8) * 8
    return k8 + _PITCH[True][c["a_sel"]], k8 + _PITCH[c["wb"]][c["b_sel"]]


def bf_form(c):
    ldx, ldw = bf_pitches(c)
    a_vec, b_vec = (0 if c["a_sel"] == "off" else c["a_sel"]), (0 if c["b_sel"] == "off" else c["b_sel"])
    if (c["wb"] and c["M"] >= 1024 and c["N"] <= 128 and 32 <= c["K"] <= 1536 and c["K"] % 4 == 0 and ldx % 4 == 0
            and ldw % 4 == 0 and c["a_sel"] != "off" and c["b_sel"] != "off"):
        return (1, 8, 1, 6, 1, 1)
    return (0, bf_nw(c["K"]), int(c["wb"]), 6, a_vec, b_vec)


def bf_operands(c):
    gen = torch.Generator().manual_seed(c["seed"])
    M, N, K = c["M"], c["N"], c["K"]
    ldx, ldw = bf_pitches(c)
    o = dict(idx=None, bias=None, ldx=ldx, ldw=ldw, x_off=int(c["a_sel"] == "off"), w_off=int(c["b_sel"] == "off"))
    n_src = M + 5 if c["gather"] else M
    X = _draw(gen, (n_src, K), c).bfloat16()
    W = _draw(gen, (N, K), c)
    if c["real"]:
        W = W / K ** 0.5
    W = W.bfloat16() if c["wb"] else W
    o["X64"] = X.double()
    if c["gather"]:
        idx, unused, o["idx"] = _gather_index(gen, M, n_src)
        X[unused] = NAN
        o["X64"] = X[idx].double()
    o["W64"] = W.bfloat16().double()          # fp32 W is rounded to bf16 (nearest even) while loaded
    o["X"] = _stored(X, ldx, o["x_off"], torch.bfloat16)
    o["W"] = _stored(W, ldw, o["w_off"], W.dtype)
    o["bias64"] = torch.zeros(N, dtype=torch.float64)
    if c["bias"]:
        b = _draw(gen, (N,), c)
        o["bias"], o["bias64"] = torch.cat([b, torch.full((2,), NAN)]), b.double()
    o["C"] = torch.full((M + 2, N + 3), NAN)
    return o


def bf_args(c, o, addr):
    """positional arguments of capi.gemm_bf16a_stream_form (gemm_bf16a_stream takes them without the trailing w_is_bf16)"""
    def at(name, nbytes=0):
        return None if o[name] is None else addr(name) + nbytes
    return (at("X", 2 * o["x_off"]), o["ldx"], at("idx"), at("W", (2 if c["wb"] else 4) * o["w_off"]), o["ldw"], at("C"),
            c["N"] + 3, c["M"], c["N"], c["K"], at("bias"), c["act"], int(c["wb"]))


def bf_expected(c, o):
    v = o["X64"] @ o["W64"].t() + o["bias64"]
    mag = o["X64"].abs() @ o["W64"].abs().t() + o["bias64"].abs()
    return (torch.relu(v) if c["act"] == 1 else v), mag


def bf_check(c, o, got_C):
    exp, mag = bf_expected(c, o)
    return check_written(got_C, exp, "bf16a %s" % (c,), error_bound(c["K"], bf_form(c)[1], mag) if c["real"] else None)


def bf_streaming_cases(real=False):
    """every (nw, W type, a_vec, b_vec) of the streaming kernel, the one-element-offset way to a_vec / b_vec = 0 included"""
    if real:
        return [bfcase(33, 17, BF_K_OF_NW[nw], wb, bias=True, real=True) for nw in (1, 4, 8) for wb in (True, False)]
    return [bfcase(33, 17, BF_K_OF_NW[nw], wb, a, b, seed=nw) for nw in (1, 4, 8) for wb in (True, False) for a in A_SEL
            for b in B_SEL[wb]]


BF_SWEEP_K, BF_SWEEP_M, BF_SWEEP_N, BF_SWEEP_LD = 600, 33, 17, 608


def bf_sweep_blocks():
    gen = torch.Generator().manual_seed(600)
    X = torch.randint(-3, 4, (BF_SWEEP_M, BF_SWEEP_K), generator=gen).float()
    W = torch.randint(-3, 4, (BF_SWEEP_N, BF_SWEEP_K), generator=gen).float()
    return X, W


def bf_gather_cases():
    return [bfcase(33, 17, BF_K_OF_NW[nw], wb, gather=True, bias=True, act=1, seed=1) for nw in (1, 4, 8) for wb in (True, False)]


PERSIST_M = (1024, 1025, 1039)
PERSIST_N = (1, 16, 17, 64, 65, 100, 112, 113, 128)
PERSIST_K = (32, 36, 60, 64, 100, 1380, 1532, 1536)


def bf_persist_cases(M):
    """the persistent kernel: K with and without a shifted last block, N up to both column halves' last tile; gather, bias and
    relu in every other case"""
    cases = []
    for i, (N, K) in enumerate((N, K) for N in PERSIST_N for K in PERSIST_K):
        on = bool(i % 2)
        cases.append(bfcase(M, N, K, True, a_sel=(2, 1)[(i // 2) % 2], b_sel=(1, 2)[(i // 4) % 2], gather=on, bias=on, act=int(on),
                            seed=i))
    return cases


def bf_beyond_persist_cases():
    """just past the persistent kernel's K and N limits: the streaming kernel has to take these"""
    return [bfcase(1024, 100, 1540, True, bias=True), bfcase(1024, 129, 1380, True, bias=True, act=1)]


def bf_persist_real_case():
    return bfcase(1039, 113, 1380, True, bias=True, real=True)


def bf_integer_cases():
    cases = bf_streaming_cases() + bf_gather_cases() + bf_beyond_persist_cases()
    for M in PERSIST_M:
        cases += bf_persist_cases(M)
    return cases


BF_FORMS = frozenset([(0, nw, 1, 6, a, b) for nw in (1, 4, 8) for a in (2, 1, 4, 0) for b in (2, 1, 4, 0)] +
                     [(0, nw, 0, 6, a, b) for nw in (1, 4, 8) for a in (2, 1, 4, 0) for b in (1, 3, 0)] + [(1, 8, 1, 6, 1, 1)])


# ---- fp32 W rounded to bf16 on the fly
ROUND_M, ROUND_N, ROUND_K = 33, 17, 64
ROUND_LOW16 = {"tie, even below": (0, 0x8000), "tie, even above": (1, 0x8000), "one ulp below a tie": (None, 0x7FFF),
               "one ulp above a tie": (None, 0x8001)}


def rounding_weights():
    """fp32 W [N, K] in +-[1, 2) whose low 16 bits sit on and next to the bf16 rounding boundary, by class in turn; returns
    W and the class of every element"""
    gen = torch.Generator().manual_seed(64)
    n = ROUND_N * ROUND_K
    mant = torch.randint(0, 128, (n,), generator=gen)
    sign = torch.randint(0, 2, (n,), generator=gen)
    kinds = list(ROUND_LOW16)
    cls = torch.arange(n) % len(kinds)
    bits = torch.zeros(n, dtype=torch.int64)
    for i, kind in enumerate(kinds):
        lsb, low = ROUND_LOW16[kind]
        m = mant.clone()
        if lsb is not None:
            m = (m & ~1) | lsb
        bits = torch.where(cls == i, (sign << 31) | 0x3F800000 | (m << 16) | low, bits)
    W = torch.from_numpy(bits.numpy().astype(np.uint32).view(np.float32).copy()).view(ROUND_N, ROUND_K)
    return W, cls.view(ROUND_N, ROUND_K), kinds


def rounding_case(b_sel):
    """A integers in [-2, 2]: every sum is a multiple of 2^-7 below 2^8, 15 bits, exact in fp32 in any order"""
    c = bfcase(ROUND_M, ROUND_N, ROUND_K, False, b_sel=b_sel)
    gen = torch.Generator().manual_seed(5)
    X = torch.randint(-2, 3, (ROUND_M, ROUND_K), generator=gen).float().bfloat16()
    W = rounding_weights()[0]
    ldx, ldw = bf_pitches(c)
    o = dict(idx=None, bias=None, ldx=ldx, ldw=ldw, x_off=0, w_off=int(b_sel == "off"), X64=X.double(),
             W64=W.bfloat16().double(), bias64=torch.zeros(ROUND_N, dtype=torch.float64))
    o["X"], o["W"] = _stored(X, ldx, 0, torch.bfloat16), _stored(W, ldw, o["w_off"])
    o["C"] = torch.full((ROUND_M + 2, ROUND_N + 3), NAN)
    return c, o
