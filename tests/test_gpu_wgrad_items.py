"""Every kind of work item of the bf16 weight-gradient launch (csrc/wgrad_bf16.hip), through the C ABI, on integer-valued bf16
operands: every product and every fp32 partial sum is an exact integer, so the gradients must equal an int64 product BIT FOR BIT
whatever the split count, the order of the records in the table or the order in which the loads of the K loop are issued --
and the launch with the optimizer inside (the single-rank instance, which has no peer exchange compiled in) must leave the
parameters, both moments and the bf16 shadows of the separate optimizer launch, bit for bit.

Shapes: K in {5, 64, 257, 600, 1100} (one k-step group and a ragged one, several groups, two and three passes of the ring of
load groups with the last pass partial), with and without a device-side row count below K; N in {4, 68} (one partial tile,
two tiles); M in {4, 100}; both output layouts; bias strips on either side; a gathered B operand with repeated and permuted
rows as the first, the middle and the last record of the table; 1 / 2 / 4 splits (K = 5 has two k-steps: at most 2); NaN in
the slabs and around every output; a second launch on the same workspace."""
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, B1, B2, EPS, WD = 1e-3, 0.9, 0.999, 1e-8, 1e-2


def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _build(K, k_true, splits, gather_pos, seed):
    """Three product records + one finished range in a flat gradient buffer of 64-element blocks with a block of padding
    between them; returns everything both launch forms need, and the expected gradients."""
    gen = torch.Generator().manual_seed(seed)
    R = 300
    shapes = dict(g=dict(M=100, N=68, ct=0, bias="a", gather=True), p=dict(M=4, N=68, ct=1, bias="b", gather=False),
                  q=dict(M=100, N=4, ct=0, bias=None, gather=False))
    order = {"first": "gpq", "middle": "pgq", "last": "pqg"}[gather_pos]
    nks = -(-K // 4)
    per = -(-nks // splits)
    sp = -(-nks // per)                      # no empty split (as engine.GemmPlanner.flush_wgrads_bf16)
    off, lay = 64, {}
    for name in order:
        s = shapes[name]
        lay[name + ".w"] = (off, s["M"] * s["N"])
        off += -(-s["M"] * s["N"] // 64) * 64 + 64
        if s["bias"]:
            nb = s["M"] if s["bias"] == "a" else s["N"]
            lay[name + ".b"] = (off, nb)
            off += -(-nb // 64) * 64 + 64
    lay["range"] = (off, 100)
    off += 128 + 64
    n = off
    ops, want = {}, torch.full((n, ), float("nan"))
    for name in order:
        s = shapes[name]
        M, N = s["M"], s["N"]
        lda, ldb = -(-M // 8) * 8, N + 4
        A = _ints((K, lda), -4, 4, gen)
        rows = R if s["gather"] else K
        Bm = _ints((rows, ldb), -4, 4, gen)
        idx = None
        if s["gather"]:
            idx = torch.randint(0, R, (K, ), generator=gen).to(torch.int32)      # permuted rows ...
            idx[K // 2], idx[K - 1] = idx[0], idx[0]                             # ... and repeated ones
        else:
            Bm[k_true:] = 55.0                                                   # stale rows beyond the device-side count: masked
        A[k_true:] = 33.0
        Bk = (Bm[idx.long()] if idx is not None else Bm)[:k_true, :N].to(torch.int64)
        Ak = A[:k_true, :M].to(torch.int64)
        W = Ak.t() @ Bk                                                          # [M, N]
        o, cnt = lay[name + ".w"]
        want[o:o + cnt] = (W.t() if s["ct"] else W).reshape(-1).float()
        if s["bias"]:
            o, cnt = lay[name + ".b"]
            want[o:o + cnt] = (Ak.sum(0) if s["bias"] == "a" else Bk.sum(0)).float()
        ops[name] = dict(A=A.to(torch.bfloat16).to(DEV), B=Bm.to(torch.bfloat16).to(DEV), idx=idx.to(DEV) if idx is not None else None,
                         lda=lda, ldb=ldb)
    o, cnt = lay["range"]
    rng_vals = _ints((cnt, ), -9, 9, gen)
    want[o:o + cnt] = rng_vals
    return dict(shapes=shapes, order=order, sp=sp, lay=lay, n=n, ops=ops, want=want, rng_vals=rng_vals, K=K,
                k_dev=torch.tensor([k_true], dtype=torch.int32, device=DEV) if k_true < K else None)


class _Side:
    """one launch form's buffers: NaN around (and, before the launch, in) every output"""

    def __init__(self, case, fused, p0):
        from erc_amd import capi
        n, lay = case["n"], case["lay"]
        self.case, self.fused = case, fused
        self.g = torch.full((n, ), float("nan"), device=DEV)
        o, cnt = lay["range"]
        self.g[o:o + cnt] = case["rng_vals"].to(DEV)                              # completed by "an earlier launch"
        self.p, self.m, self.v = p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        self.state = torch.zeros(4 + 512, dtype=torch.int64, device=DEV)
        self.health = torch.zeros(1, dtype=torch.int32, device=DEV)
        tab = capi.ShadowTable(DEV)
        og, cg = lay["g.w"]
        tab.add(og, cg, cg, 68, 100, (0, 1, 0), (1, 0, 0), 68, 0)                 # row-major copy
        tab.add(og, cg, cg, 68, 100, (1, 0, 0), (0, 1, 0), 100, 0)                # transposed: a quad is four 2-byte stores
        oq, cq = lay["q.w"]
        tab.add(oq, cq, cq, 4, 100, (1, 0, 0), (0, 1, 0), 100, 0)
        self.tab = tab.seal()
        raw, bases, items, tiles = [], [], 0, 0
        for name in case["order"]:
            s, op = case["shapes"][name], case["ops"][name]
            M, N = s["M"], s["N"]
            tn = -(-N // 64)
            ow = lay[name + ".w"][0]
            ob = lay[name + ".b"][0] if s["bias"] else None
            ptr = lambda o_: self.g.data_ptr() + 4 * o_
            raw.append(struct.pack("<QQQQQQQ14i", op["A"].data_ptr(), op["B"].data_ptr(), ptr(ow), ptr(ob) if s["bias"] == "a" else 0,
                                   ptr(ob) if s["bias"] == "b" else 0, op["idx"].data_ptr() if op["idx"] is not None else 0,
                                   case["k_dev"].data_ptr() if case["k_dev"] is not None else 0, op["lda"], op["ldb"],
                                   M if s["ct"] else N, M, N, case["K"], s["ct"], 1, case["sp"], tn, items, tn * case["sp"], tiles, 0))
            bases.append(items)
            items += tn * case["sp"]
            tiles += tn
        if fused:
            o, cnt = lay["range"]
            raw.append(struct.pack("<QQQQQQQ14i", 0, 0, self.g.data_ptr() + 4 * o, 0, 0, 0, 0, 0, 0, 0, cnt, 0, 0, 0, 0, 1, 1, items, 1, tiles, 1))
            bases.append(items)
            items += 1
        import ctypes
        self.table = torch.frombuffer(bytearray(b"".join(raw)), dtype=torch.uint8).to(DEV)
        self.n_desc, self.items, self.tiles = len(raw), items, tiles
        self.bases = (ctypes.c_int32 * len(bases))(*bases)
        self.slabs = torch.full((items * capi.wgrad_bf16_slab_floats(), ), float("nan"), device=DEV)
        self.counters = torch.zeros(tiles + 512, dtype=torch.int32, device=DEV)

    def launch(self):
        from erc_amd import capi
        if self.fused:
            capi.wgrad_bf16_adam(self.table, self.n_desc, self.bases, self.items, self.slabs, self.counters, self.tiles, self.p, self.g,
                                 self.m, self.v, self.case["n"], LR, B1, B2, EPS, WD, 0, 1.0, self.state, self.tab, self.health)
        else:
            capi.wgrad_bf16(self.table, self.n_desc, self.bases, self.items, self.slabs, self.counters)
        torch.cuda.synchronize()

    def separate_optimizer(self):
        """the optimizer as its own launch over the whole buffer (the padding's NaN gradients replaced by zeros)"""
        from erc_amd import capi
        g = torch.nan_to_num(self.g, nan=0.0)
        capi.adam_step_tab(self.p, g, self.m, self.v, self.case["n"], LR, B1, B2, EPS, WD, 0, 1.0, 0.0, None, self.state, self.tab,
                           skip_flag=self.health)
        torch.cuda.synchronize()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int16),
                       b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int16))


def _check_grad(side, want):
    got = side.g.cpu()
    pad = torch.isnan(want)
    assert bool(torch.isnan(got[pad]).all()), "a store outside the records' outputs"
    assert torch.equal(got[~pad], want[~pad]), (got[~pad] - want[~pad]).abs().max()


# (600 and 1100 rows in one split: a wavefront's ring of four 8-step load groups goes round more than once and stops part-way)
CASES = [(5, 5), (64, 64), (64, 61), (257, 257), (257, 254), (600, 600), (1100, 1097)]


@pytest.mark.parametrize("gather_pos", ["first", "middle", "last"])
@pytest.mark.parametrize("splits", [1, 2, 4])
@pytest.mark.parametrize("K,k_true", CASES, ids=["k5", "k64", "k64dev61", "k257", "k257dev254", "k600", "k1100dev1097"])
def test_every_item_kind_exact_and_fused_equals_separate(K, k_true, splits, gather_pos):
    from erc_amd import capi
    case = _build(K, k_true, splits, gather_pos, seed=K * 10 + splits)
    p0 = torch.randn(case["n"], generator=torch.Generator().manual_seed(1)) * 0.1
    fused, plain = _Side(case, True, p0), _Side(case, False, p0)
    rec = torch.zeros(case["n"], dtype=torch.bool)
    for o, cnt in case["lay"].values():
        rec[o:o + cnt] = True
    for step in (1, 2):          # the second launch: the same workspace (slabs, counters, sequence numbers), other operand values
        if step == 2:
            case2 = _build(K, k_true, splits, gather_pos, seed=K * 10 + splits + 1000)
            for name in case["order"]:
                case["ops"][name]["A"].copy_(case2["ops"][name]["A"])
                case["ops"][name]["B"].copy_(case2["ops"][name]["B"])
                if case["ops"][name]["idx"] is not None:
                    case["ops"][name]["idx"].copy_(case2["ops"][name]["idx"])
            o, cnt = case["lay"]["range"]
            for side in (fused, plain):
                side.g.fill_(float("nan"))
                side.g[o:o + cnt] = case2["rng_vals"].to(DEV)
            case["want"] = case2["want"]
        plain.launch()
        _check_grad(plain, case["want"])
        plain.separate_optimizer()
        fused.launch()
        _check_grad(fused, case["want"])
        assert int(fused.health[0]) == 0 and int(fused.state[0]) == step and bool((fused.state[4:] == step).all())
        assert int(plain.state[0]) == step
        for a, b in ((fused.p, plain.p), (fused.m, plain.m), (fused.v, plain.v)):
            assert _same_bits(a.cpu()[rec], b.cpu()[rec])
        assert _same_bits(fused.p.cpu()[~rec], p0[~rec]), "the fused launch updated an element outside its records"
        assert not bool(fused.m.cpu()[~rec].any()) and not bool(fused.v.cpu()[~rec].any())
        assert _same_bits(fused.tab.buf.cpu(), plain.tab.buf.cpu())
    assert capi.wgrad_bf16_slab_floats() == 128 * 64 + 192
