"""GPU: the per-dialogue attention kernels one by one, through capi only, against the float64 restatements of
tests/att_kernels_ref.py: CIM's cross-modal attention (csrc/cim_attn.hip), the matching attention 'general2' (csrc/match_att.hip)
and the positional edge attention with erc_dgcnv2_meta (csrc/dgcnv2_att.hip), on that file's case tables.

Every case prefills every output and save buffer with NaN, keeps guard rows behind each buffer, compares each output group and
each save (Pbuf; P, TH, DZ; norm per edge) with float64 under the bound of att_kernels_ref (4 x the float32 twin's worst figure,
never a kernel's own), asserts that the inputs are bit-unchanged (dmerged[:, 0:600) included) and that everything outside the
documented write set still holds its prefill (rows beyond a dialogue, rows of empty slots, pad columns, Pbuf / P outside
[L, L], guard rows), and launches a second time on the same buffers: bit-equal.  A capacity launch (empty slots interleaved, a
larger T, dead rows) must equal the exact launch of the same dialogues bit for bit on the valid rows; erc_match_att_bwd_cap
writes rows [N, n_cap) as +0 and leaves the rows behind them alone.  The refusals no other test covers come last.

MEASURED on an MI355X, worst err / scale over the cases of a family (printed by every run):
    CIM                     out      Pbuf     ddense
      bound                 2e-6     4e-6     5e-7
      MI355X                3.67e-7  4.03e-7  1.51e-7
    matching attention      A        P        TH       DZ       dQ       dE
      bound, small scale    4e-7     2e-7     3e-6     2e-6     2e-6     4e-7
      MI355X, small scale   1.02e-7  5.96e-8  3.80e-7  2.99e-7  2.91e-7  1.02e-7
      bound, saturated      5e-7     2e-7     8e-6     2e-6     2e-6     4e-7
      MI355X, saturated     1.06e-7  7.19e-8  1.15e-6  2.71e-7  3.07e-7  9.86e-8
    edge attention          norm     dS
      bound                 4e-6     6e-5
      MI355X                9.11e-7  1.38e-5
Each of these deliberate errors in a scratch build fails at least the named test: `v.x >= 0.f` in cim_attn_bwd_kernel
(test_cim_attention_against_float64, every case); one pass of out-edges in edge_att_fwd_kernel (test_edge_attention_against_float64
on the windows (-1, -1), (-1, 3), (2, -1), (40, 40)); zero_tail_rows from n + 1 (test_matching_attention_against_float64, the
capacity cases with a tail); lddq passed for ldde in launch_bwd (test_matching_attention_against_float64, every case with more
than one row); `lane + 64 <= L` in CIM's softmax (test_cim_attention_against_float64 at L >= 64).
"""
import functools

import numpy as np
import pytest
import torch

from tests import att_kernels_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 2             # rows behind every row buffer
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from erc_amd import capi
    capi.lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def nan32(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def untouched(a):
    return bool(np.isnan(a).all())


def plus_zero(a):
    """every element is +0.0, bit for bit"""
    return bool((np.ascontiguousarray(a).view(np.uint32) == 0).all())


def padded(a, rows, ld):
    """a [n, w] in the top left corner of NaN [rows, ld]"""
    buf = np.full((rows, ld), np.nan, np.float32)
    buf[:a.shape[0], :a.shape[1]] = a
    return buf


def square_saves(flat, lens, T, lead, tag):
    """the [L, L] blocks of a [lead..., B, T, T] save with T * T guard floats behind it; everything else must be prefill"""
    B = len(lens)
    n = int(np.prod(lead)) * B * T * T
    assert untouched(flat[n:]), (tag, "guard behind the save")
    a = flat[:n].reshape(*lead, B, T, T)
    out = {}
    for idx in np.ndindex(*lead):
        for b, L in enumerate(lens):
            blk = a[idx][b]
            assert untouched(blk[L:]) and untouched(blk[:L, L:]), (tag, idx, b, "written outside [L, L]")
            if L:
                assert not np.isnan(blk[:L, :L]).any(), (tag, idx, b, "unwritten or NaN")
                out[idx + (b,) if lead != (1,) else b] = blk[:L, :L]
    return out


def report(family, name, fig, bound):
    print("att %-6s %-24s " % (family, name) + " ".join("%s=%.2e" % (k, v) for k, v in fig.items()))
    for k, v in fig.items():
        assert v <= bound[k], (family, name, k, v, bound[k])


# ===================================================================================================== CIM
@functools.lru_cache(maxsize=None)
def cim_run(name):
    """forward twice, backward twice (dmerged restored in between: its dense block is read-modified-written) on one set of buffers"""
    from erc_amd import capi
    ref = R.cim_reference(name)
    c, N = ref["c"], ref["N"]
    B, T = len(c["lens"]), c["T"]
    rows = N + c["dead"] + GUARD
    merged0 = padded(np.concatenate([np.full((N, 600), np.nan, np.float32), ref["dense"]], 1), rows, 900)
    dmerged0 = padded(np.concatenate([ref["G"], ref["Gd"]], 1), rows, 900)
    node_off = dev(R.offsets(c["lens"]).astype(np.int32))
    merged, dmerged, Pbuf = dev(merged0), dev(dmerged0), nan32(6 * B * T * T + T * T)
    fwd = []
    for _ in range(2):
        capi.cim_attn_fwd(merged, node_off, B, T, Pbuf)
        fwd.append((host(merged), host(Pbuf)))
    bwd = []
    for _ in range(2):
        dmerged.copy_(dev(dmerged0))
        capi.cim_attn_bwd(merged, dmerged, node_off, B, T, Pbuf, c["mask_scale"])
        bwd.append(host(dmerged))
    return dict(merged0=merged0, dmerged0=dmerged0, fwd=fwd, bwd=bwd, merged_after=host(merged), P_after=host(Pbuf))


def cim_outputs(name):
    run, ref = cim_run(name), R.cim_reference(name)
    c, N = ref["c"], ref["N"]
    m, P = run["fwd"][0]
    saves = square_saves(P, c["lens"], c["T"], (6,), name)
    return dict(out=m[:N, :600], P=saves, ddense=run["bwd"][0][:N, 600:])


@pytest.mark.parametrize("name", [c["name"] for c in R.CIM_CASES])
def test_cim_attention_against_float64(name):
    run, ref = cim_run(name), R.cim_reference(name)
    c, N = ref["c"], ref["N"]
    m, P = run["fwd"][0]
    # ---- forward: only the six output blocks of the dialogues' rows are written
    assert same_bits(m[:, 600:], run["merged0"][:, 600:]), "the dense block (dead and guard rows included) was written"
    assert untouched(m[N:]), "rows beyond the dialogues"
    assert not np.isnan(m[:N, :600]).any()
    got = cim_outputs(name)
    assert sorted(got["P"]) == sorted(ref["out"]["P"])
    assert same_bits(run["fwd"][1][0], m) and same_bits(run["fwd"][1][1], P), "second forward launch"
    # ---- backward: dmerged[:, 0:600) only read, the dense block of the dialogues' rows only written; merged, Pbuf only read
    d = run["bwd"][0]
    assert same_bits(d[:, :600], run["dmerged0"][:, :600]), "dmerged[:, 0:600) was written"
    assert untouched(d[N:]), "rows beyond the dialogues"
    assert same_bits(run["merged_after"], m) and same_bits(run["P_after"], P), "the backward wrote one of its inputs"
    zero = ref["dense"] == 0
    assert zero.any() and plus_zero(d[:N, 600:][zero]), "the zero arm of the mask"
    assert not np.isnan(d[:N, 600:]).any()
    assert same_bits(run["bwd"][1], d), "second backward launch"
    report("cim", name, R.cim_figures(got, ref["out"]), R.BOUND["cim"])


@pytest.mark.parametrize("name", [c["name"] for c in R.CIM_CASES if c["exact"]])
def test_cim_capacity_launch_equals_exact_launch_bit_for_bit(name):
    """empty slots at the front, in the middle and at the end, T (Pbuf and LDS pitch) above the longest dialogue, dead rows: a
    dialogue's arithmetic depends on neither"""
    cap, exact = cim_outputs(name), cim_outputs(R.CIM_CASE[name]["exact"])
    assert same_bits(cap["out"], exact["out"]) and same_bits(cap["ddense"], exact["ddense"])
    slots = [b for b, L in enumerate(R.CIM_CASE[name]["lens"]) if L]
    assert sorted(cap["P"]) == [(p, b) for p in range(6) for b in slots]
    for (p, b), blk in cap["P"].items():
        assert same_bits(blk, exact["P"][p, slots.index(b)]), (p, b)


# ===================================================================================================== matching attention
@functools.lru_cache(maxsize=None)
def match_run(name):
    from erc_amd import capi
    ref = R.match_reference(name)
    c, N, F = ref["c"], ref["N"], ref["c"]["F"]
    B, T, pit = len(c["lens"]), c["T"], R.match_pitches(F)
    n_cap = 0 if c["tail"] is None else N + c["tail"]
    rows = max(N, n_cap) + GUARD
    inp0 = dict(E=padded(ref["E"], rows, pit["lde"]), Q=padded(ref["Q"], rows, pit["ldq"]), dA=padded(ref["dA"], rows, pit["ldda"]))
    inp = {k: dev(v) for k, v in inp0.items()}
    node_off = dev(R.offsets(c["lens"]).astype(np.int32))
    A, dQ, dE = nan32(rows, pit["lda"]), nan32(rows, pit["lddq"]), nan32(rows, pit["ldde"])
    P, TH, DZ = (nan32(B * T * T + T * T) for _ in range(3))
    fwd, bwd = [], []
    for _ in range(2):
        capi.match_att_fwd(inp["E"], pit["lde"], inp["Q"], pit["ldq"], node_off, B, T, F, A, pit["lda"], P, TH)
        fwd.append(dict(A=host(A), P=host(P), TH=host(TH)))
    for _ in range(2):
        capi.match_att_bwd(inp["E"], pit["lde"], inp["Q"], pit["ldq"], inp["dA"], pit["ldda"], node_off, B, T, F, P, TH, DZ, dQ,
                           pit["lddq"], dE, pit["ldde"], n_cap=n_cap)
        bwd.append(dict(DZ=host(DZ), dQ=host(dQ), dE=host(dE)))
    after = {k: host(v) for k, v in inp.items()}
    after.update(P=host(P), TH=host(TH))
    return dict(inp0=inp0, fwd=fwd, bwd=bwd, after=after, n_cap=n_cap)


def match_outputs(name):
    run, ref = match_run(name), R.match_reference(name)
    c, N, F = ref["c"], ref["N"], ref["c"]["F"]
    got = {k: square_saves(src[k], c["lens"], c["T"], (1,), (name, k)) for k, src in (("P", run["fwd"][0]), ("TH", run["fwd"][0]), ("DZ", run["bwd"][0]))}
    got.update(A=run["fwd"][0]["A"][:N, :F], dQ=run["bwd"][0]["dQ"][:N, :F], dE=run["bwd"][0]["dE"][:N, :F])
    return got


@pytest.mark.parametrize("name", [c["name"] for c in R.MATCH_CASES])
def test_matching_attention_against_float64(name):
    run, ref = match_run(name), R.match_reference(name)
    c, N, F, n_cap = ref["c"], ref["N"], ref["c"]["F"], run["n_cap"]
    got = match_outputs(name)
    for k, a in (("A", run["fwd"][0]["A"]), ("dQ", run["bwd"][0]["dQ"]), ("dE", run["bwd"][0]["dE"])):
        assert not np.isnan(a[:N, :F]).any(), (k, "unwritten or NaN")
        assert untouched(a[:, F:]), (k, "pad columns")
        zeroed = n_cap if k != "A" else 0
        if zeroed > N:
            assert plus_zero(a[N:zeroed, :F]), (k, "capacity rows [N, n_cap) are not all +0")
        assert untouched(a[max(N, zeroed):]), (k, "rows at or beyond n_cap" if zeroed else "rows beyond the dialogues")
    for k in ("A", "P", "TH"):
        assert same_bits(run["fwd"][1][k], run["fwd"][0][k]), (k, "second forward launch")
    for k in ("DZ", "dQ", "dE"):
        assert same_bits(run["bwd"][1][k], run["bwd"][0][k]), (k, "second backward launch")
    for k in ("E", "Q", "dA"):
        assert same_bits(run["after"][k], run["inp0"][k]), (k, "an input was written")
    assert same_bits(run["after"]["P"], run["fwd"][0]["P"]) and same_bits(run["after"]["TH"], run["fwd"][0]["TH"]), "the backward wrote P or TH"
    report("match", name, {k: v for k, v in R.match_figures(got, ref["out"]).items()}, R.BOUND["match_" + c["scale"]])


@pytest.mark.parametrize("name", [c["name"] for c in R.MATCH_CASES if c["exact"]])
def test_matching_capacity_launch_equals_exact_launch_bit_for_bit(name):
    """erc_match_att_bwd_cap (and the forward at B = 6, T = 110 with empty slots) against erc_match_att_bwd on the same dialogues"""
    cap, exact = match_outputs(name), match_outputs(R.MATCH_CASE[name]["exact"])
    for k in ("A", "dQ", "dE"):
        assert same_bits(cap[k], exact[k]), k
    slots = [b for b, L in enumerate(R.MATCH_CASE[name]["lens"]) if L]
    for k in ("P", "TH", "DZ"):
        assert sorted(cap[k]) == slots
        for i, b in enumerate(slots):
            assert same_bits(cap[k][b], exact[k][i]), (k, b)


# ===================================================================================================== edge attention
def _graph(ref):
    g, c = ref["g"], ref["c"]
    tail = np.full(3, -1, np.int32)      # never read
    return dict(node_off=dev(R.offsets(c["lens"]).astype(np.int32)), out_ptr=dev(g["out_ptr"]),
                out_dst=dev(np.concatenate([g["out_dst"], tail])), out_eid=dev(np.concatenate([g["out_eid"], tail])))


@pytest.mark.parametrize("name", [c["name"] for c in R.EDGE_CASES])
def test_edge_attention_against_float64(name):
    from erc_amd import capi
    ref = R.edge_reference(name)
    c, n_e = ref["c"], ref["n_e"]
    T, B, ldS = c["T"], len(c["lens"]), c["ldS"]
    S0 = ref["S"].reshape(T * B, ldS)
    S, g = dev(S0), _graph(ref)
    norm, dS, parts = nan32(n_e + 5), nan32(T * B + GUARD, ldS), dev(ref["parts"].reshape(-1))
    runs = []
    for _ in range(2):
        capi.dgcnv2_edge_att_fwd(S, ldS, g, B, T, c["wp"], c["wf"], norm)
        capi.dgcnv2_edge_att_bwd(S, ldS, g, B, T, c["wp"], c["wf"], parts, dS, dn_parts=c["dn_parts"], dn_stride=ref["stride"])
        runs.append((host(norm), host(dS)))
    n1, d1 = runs[0]
    assert same_bits(host(S), S0) and same_bits(host(parts), ref["parts"].reshape(-1)), "an input was written"
    assert untouched(n1[n_e:]) and not np.isnan(n1[:n_e]).any()
    assert untouched(d1[T * B:]), "guard rows"
    assert untouched(d1[:, R.NSCAL:]), "pad columns"
    d = d1[:T * B].reshape(T, B, ldS)[:, :, :R.NSCAL]
    assert not np.isnan(d).any(), "dS is written for every padded row"
    for b, L in enumerate(c["lens"]):
        assert plus_zero(d[:, b, L:]), (b, "columns of absent sources")
    assert same_bits(runs[1][0], n1) and same_bits(runs[1][1], d1), "second launch"
    report("edge", name, R.edge_figures(dict(norm=n1[:n_e], dS=d), ref["out"]), R.BOUND["edge"])


# ===================================================================================================== erc_dgcnv2_meta
def _onehot(r, T, B, S):
    oh = np.zeros((T * B, S), np.float32)
    oh[np.arange(T * B), r.randint(0, S, T * B)] = 1.0
    for i in range(0, T * B, 7):          # no 1 at all: zeros, or entries that are nearly 1
        oh[i] = 0.0 if (i // 7) % 2 else 0.999
    for i in range(3, T * B, 7):          # two 1s: the first index wins
        oh[i, r.randint(0, S)] = 1.0
    for i in range(5, T * B, 7):          # 0.999 in front of the 1.0
        k = int(oh[i].argmax())
        oh[i, :k] = 0.999
    return oh.reshape(T, B, S)


@pytest.mark.parametrize("S,B,T,short", [(1, 3, 4, 0), (2, 5, 7, 6), (9, 4, 110, 0), (9, 6, 5, 1), (2, 1024, 1, 100)])
def test_dgcnv2_meta_is_integer_exact(S, B, T, short):
    """the first index whose one-hot entry equals 1 (0 if none), lengths clamped to [0, T], and node_row cut at n_cap (``short``
    entries below the node count, or 3 above it when 0), canaries behind both outputs"""
    from erc_amd import capi
    r = np.random.RandomState(S * 1000 + B)
    oh = _onehot(r, T, B, S)
    lengths = r.randint(-2, T + 3, B).astype(np.int64)
    lengths[0], lengths[-1] = T + 5, (-3 if B > 1 else T + 5)
    n = int(np.clip(lengths, 0, T).sum())
    n_cap = n - short if short else n + 3
    assert 0 < n_cap and (short == 0 or n_cap < n)
    spk_want, rows_want, n_ref = R.dgcnv2_meta(oh, lengths, B, T, n_cap)
    assert n_ref == n and len(rows_want) == min(n, n_cap)
    assert S == 1 or (len(set(spk_want.tolist())) > 1 and (oh == 1).sum(-1).max() == 2 and ((oh == 1).sum(-1) == 0).any())
    oh_d, len_d = dev(oh), dev(lengths)
    spk = torch.full((T * B + 4,), -77, dtype=torch.int64, device=DEV)
    node_row = torch.full((max(n, n_cap) + 4,), -77, dtype=torch.int32, device=DEV)
    capi.dgcnv2_meta(oh_d, S, len_d, B, T, n_cap, spk, node_row)
    spk, node_row = host(spk), host(node_row)
    assert np.array_equal(spk[:T * B], spk_want) and np.all(spk[T * B:] == -77)
    assert np.array_equal(node_row[:len(rows_want)], rows_want) and np.all(node_row[len(rows_want):] == -77)
    assert same_bits(host(oh_d), oh) and same_bits(host(len_d), lengths)


# ===================================================================================================== refusals
def _refused(call, outputs, match=None):
    from erc_amd import capi
    with pytest.raises(capi.ErcGraftError, match=match):
        call()
    for o in outputs:
        assert untouched(host(o)), "an output was written by a refused call"


def test_cim_refusals_leave_the_outputs_alone():
    from erc_amd import capi
    N = T = 4
    node_off = dev(np.array([0, N], np.int32))
    flat = nan32(N * 900 + 4)
    merged, off4 = flat[:N * 900], flat[1:N * 900 + 1]       # 4 bytes past a 16-byte boundary
    dmerged, Pbuf = nan32(N, 900), nan32(6 * 119 * 119)
    outs = (flat, dmerged, Pbuf)
    _refused(lambda: capi.cim_attn_fwd(off4, node_off, 1, T, Pbuf), outs, "aligned")
    _refused(lambda: capi.cim_attn_bwd(off4, dmerged, node_off, 1, T, Pbuf, 1.0), outs, "aligned")
    _refused(lambda: capi.cim_attn_bwd(merged, off4, node_off, 1, T, Pbuf, 1.0), outs, "aligned")
    _refused(lambda: capi.cim_attn_bwd(merged, dmerged, node_off, 1, capi.cim_max_t() + 1, Pbuf, 1.0), outs, "118")
    assert capi.cim_max_t() == 118


@pytest.mark.parametrize("F", [200, 300])
def test_matching_refusals_leave_the_outputs_alone(F):
    from erc_amd import capi
    N = T = 4
    ld = F + 8
    node_off = dev(np.array([0, N], np.int32))
    E, Q, dA, A, dQ, dE = (nan32(N, ld) for _ in range(6))
    P, TH, DZ = (nan32(T * T) for _ in range(3))
    outs = (E, Q, dA, A, dQ, dE, P, TH, DZ)

    def fwd(lde=ld, ldq=ld, lda=ld):
        return lambda: capi.match_att_fwd(E, lde, Q, ldq, node_off, 1, T, F, A, lda, P, TH)

    def bwd(dQ_=dQ, dE_=dE, lde=ld, ldq=ld, ldda=ld, lddq=ld, ldde=ld):
        return lambda: capi.match_att_bwd(E, lde, Q, ldq, dA, ldda, node_off, 1, T, F, P, TH, DZ, dQ_, lddq, dE_, ldde)

    for k in ("lde", "ldq", "lda"):
        _refused(fwd(**{k: F - 4}), outs, "pitch")
        _refused(fwd(**{k: F + 2}), outs, "aligned")
    for k in ("lde", "ldq", "ldda", "lddq", "ldde"):
        _refused(bwd(**{k: F - 4}), outs, "pitch")
        _refused(bwd(**{k: F + 2}), outs, "aligned")
    for other in (E, Q, dA):
        _refused(bwd(dQ_=other), outs, "alias")
        _refused(bwd(dE_=other), outs, "alias")
    _refused(bwd(dQ_=dE), outs, "alias")


def test_edge_attention_refusals_leave_the_outputs_alone():
    from erc_amd import capi
    ref = R.edge_reference("one-w10_10")
    g = _graph(ref)
    S, dS, norm, dn = nan32(111, 112), nan32(111, 112), nan32(8), nan32(16)
    outs = (S, dS, norm, dn)
    _refused(lambda: capi.dgcnv2_edge_att_bwd(S, 110, g, 1, 1, 10, 10, dn, S), outs, "alias")
    _refused(lambda: capi.dgcnv2_edge_att_fwd(S, 109, g, 1, 1, 10, 10, norm), outs, "ldS")
    _refused(lambda: capi.dgcnv2_edge_att_bwd(S, 109, g, 1, 1, 10, 10, dn, dS), outs, "ldS")
    _refused(lambda: capi.dgcnv2_edge_att_bwd(S, 110, g, 1, 1, 10, 10, dn, dS, dn_parts=2, dn_stride=0), outs, "dn_parts")
    _refused(lambda: capi.dgcnv2_edge_att_bwd(S, 110, g, 1, 1, 10, 10, dn, dS, dn_parts=0, dn_stride=8), outs, "dn_parts")
    _refused(lambda: capi.dgcnv2_edge_att_bwd(S, 110, g, 1, 111, 10, 10, dn, dS), outs, "110")
