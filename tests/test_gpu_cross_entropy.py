"""GPU: erc_cross_entropy / erc_cross_entropy_cap (csrc/norm_loss.hip) against the float64 restatement of tests/loss_ref.py: row
counts on both sides of the grid's stride, C = 1 .. 7, class weights, row maps, padded leading dimensions, grad_scale, no
gradient buffer, four logit families (3 randn, 30 randn, 3 randn +- 100), planted ties for the maximum, guard rows and pad
columns.  Seven modules call this launch and the fused heads are tested as "equal to it"; this is what they are anchored to.
Bounds are the float32 twin's (F.cross_entropy with autograd), never a kernel's.  Figures are printed before they are asserted."""
import pytest
import torch

from erc_amd import capi
from tests import loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 3              # rows behind dlogits: nothing may touch them
SENT = -77.25
STATS = 256            # floats the header asks for


@pytest.fixture(scope="module", autouse=True)
def _lib():
    capi.lib()


def _stats():
    s = torch.full((STATS + 8, ), SENT, device=DEV)
    s[:STATS] = 0.0
    return s


def _place(c, padded):
    """the case on the device: logits [rows, ld] with NaN in the pad columns (never to be read), dlogits [rows + GUARD, lddl]
    filled with the sentinel"""
    C, rows = c["C"], c["rows"]
    ld, lddl = (C + R.PAD_LD, C + R.PAD_LDDL) if padded else (C, C)
    logits = torch.full((rows, ld), float("nan"), device=DEV)
    logits[:, :C] = c["logits"].to(DEV)
    dl = torch.full((rows + GUARD, lddl), SENT, device=DEV)
    return logits, ld, dl, lddl


def _reference(c, n=None):
    n = c["n"] if n is None else n
    args = (c["logits"], c["labels"], c["weight"], c["row_map"], n, c["grad_scale"])
    return R.cross_entropy64(*args), (R.cross_entropy32(*args) if n > 0 else None)


def _check(tag, c, n, stats, dl, r64, r32, write=True):
    """stats and dlogits of a launch over the first ``n`` samples of case ``c`` -> the figures"""
    C = c["C"]
    (loss64, hits, wsum, dl64), (loss32, dl32) = r64, r32
    s = stats.cpu()
    figs = dict(loss=(R.rel(s[0:1], torch.tensor([loss64])), R.twin_bound(loss32.reshape(1), torch.tensor([loss64]))))
    assert int(s[1]) == hits, (tag, int(s[1]), hits)
    assert abs(float(s[2]) - wsum) <= 2.0 ** -24 * wsum, (tag, float(s[2]), wsum)          # the double sum, rounded once
    assert int(s[:STATS].view(torch.int32)[4]) == 0, "arrival counter not back at 0"
    assert bool((s[STATS:] == SENT).all())
    D = dl.cpu()
    rows = c["row_map"].long()[:n] if c["row_map"] is not None else torch.arange(n)
    if write:
        figs["dlogits"] = (R.rel(D[rows, :C], dl64), R.twin_bound(dl32, dl64))
        untouched = torch.ones(D.shape, dtype=torch.bool)
        untouched[rows, :C] = False
        assert bool((D[untouched] == SENT).all()), "%s: pad columns, guard rows or unmapped rows were written" % tag
    else:
        assert bool((D == SENT).all())
    print("%s: %s" % (tag, "  ".join("%s %.2e/%.0e (twin %.2e)" % (k, g, b, t) for (k, (g, b)), t in zip(
        figs.items(), (R.rel(loss32.reshape(1), torch.tensor([loss64])), R.rel(dl32, dl64))))))
    for k, (g, b) in figs.items():
        assert g <= b, (tag, k, g, b)


# ---------------------------------------------------------------------------------------------------- 1. exact form
@pytest.mark.parametrize("family", sorted(R.FAMILIES))
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_cross_entropy(name, family):
    n, C, weighted, mapped, padded, grad_scale, write = R.CASES[name]
    c = R.case(name, family)
    logits, ld, dl, lddl = _place(c, padded)
    stats = _stats()
    for _ in range(2):          # twice into the same stats: the counter and the partials of the first call are still there
        capi.cross_entropy(logits, ld, C, n, c["row_map"].to(DEV) if mapped else None, c["labels"].to(DEV),
                           c["weight"].to(DEV) if weighted else None, grad_scale, dl if write else None, lddl, stats)
    torch.cuda.synchronize()
    r64, r32 = _reference(c)
    _check("ce %s %s" % (name, family), c, n, stats, dl, r64, r32, write)


@pytest.mark.parametrize("family", ["n3", "p100"])
def test_small_launch_after_a_large_one_into_the_same_stats(family):
    """64 workgroups leave 64 partials in stats; a one-workgroup launch behind them must read only its own"""
    big, small = R.case("n17161_c6", family), R.case("n255_c7", family)
    stats = _stats()
    for c in (big, small):
        name = c["name"]
        n, C, weighted, mapped, padded, grad_scale, _ = R.CASES[name]
        logits, ld, dl, lddl = _place(c, padded)
        capi.cross_entropy(logits, ld, C, n, c["row_map"].to(DEV) if mapped else None, c["labels"].to(DEV), None, grad_scale, dl, lddl,
                           stats)
    torch.cuda.synchronize()
    r64, r32 = _reference(small)
    _check("small after large, %s" % family, small, small["n"], stats, dl, r64, r32)


# ------------------------------------------------------------------------------------------------- 2. capacity form
def _cap_case(family, mapped):
    """CAP_N samples of C = 6, class-weighted; what lies at or beyond the count is poisoned per launch (below)"""
    gen = R._gen("ce-cap-%s" % family)
    scale, shift = R.FAMILIES[family]
    rows = R.CAP_N + (R.EXTRA_ROWS if mapped else 0)
    c = dict(n=R.CAP_N, C=R.CAP_C, rows=rows, logits=torch.randn(rows, R.CAP_C, generator=gen) * scale + shift,
             labels=torch.randint(0, R.CAP_C, (R.CAP_N, ), generator=gen), weight=torch.rand(R.CAP_C, generator=gen) * 9.0 + 1.0,
             row_map=torch.randperm(rows, generator=gen)[:R.CAP_N].to(torch.int32) if mapped else None, grad_scale=0.125)
    return c


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("count", R.CAP_COUNTS)
def test_cross_entropy_cap(count, mapped):
    """*n_dev in {0, 1, 299, 300, 5000, -3} of a capacity of 300 (the last two are clamped).  Samples at or beyond the count have
    NaN logits and labels of 2^40 (and, mapped, a row index that points at a NaN row): they are neither read nor written.  A full
    batch gives the bits of the exact form"""
    c = _cap_case("p100", mapped)
    n_cap, C = R.CAP_N, R.CAP_C
    n = min(max(count, 0), n_cap)
    ld, lddl = C + R.PAD_LD, C + R.PAD_LDDL
    live = c["row_map"].long()[:n] if mapped else torch.arange(n)
    logits = torch.full((c["rows"], ld), float("nan"))
    logits[live, :C] = c["logits"][live]
    labels = c["labels"].clone()
    labels[n:] = 1 << 40
    row_map = None
    if mapped:
        dead = [r for r in range(c["rows"]) if r not in set(live.tolist())]
        row_map = c["row_map"].clone()
        row_map[n:] = dead[0]
        row_map = row_map.to(DEV)
    logits, labels, weight = logits.to(DEV), labels.to(DEV), c["weight"].to(DEV)
    dl = torch.full((c["rows"] + GUARD, lddl), SENT, device=DEV)
    stats = _stats()
    n_dev = torch.tensor([count, -77], dtype=torch.int32, device=DEV)
    for _ in range(2):
        capi.cross_entropy_cap(logits, ld, C, n_cap, n_dev, row_map, labels, weight, c["grad_scale"], dl, lddl, stats)
    torch.cuda.synchronize()
    assert n_dev.cpu().tolist() == [count, -77]
    if n == 0:
        s = stats.cpu()
        print("cap count=%d: stats[:3] = %s" % (count, s[:3].tolist()))
        assert s[:3].tolist() == [0.0, 0.0, 0.0] and int(s[:STATS].view(torch.int32)[4]) == 0 and bool((dl == SENT).all())
        return
    r64, r32 = _reference(c, n)
    _check("cap count=%d mapped=%d" % (count, mapped), c, n, stats, dl, r64, r32)
    if n == n_cap:
        dl2, stats2 = torch.full_like(dl, SENT), _stats()
        capi.cross_entropy(logits, ld, C, n_cap, row_map, labels, weight, c["grad_scale"], dl2, lddl, stats2)
        torch.cuda.synchronize()
        assert torch.equal(dl.view(torch.int32), dl2.view(torch.int32))
        assert torch.equal(stats[:4].view(torch.int32), stats2[:4].view(torch.int32))


def test_refusals_by_status_with_nothing_written():
    c = R.case("n255_c7", "n3")
    logits, ld, dl, lddl = _place(c, True)
    stats, labels = _stats(), c["labels"].to(DEV)
    n_dev = torch.tensor([5], dtype=torch.int32, device=DEV)
    for what, call in {
        "n = 0": lambda: capi.cross_entropy(logits, ld, 7, 0, None, labels, None, 1.0, dl, lddl, stats),
        "C = 0": lambda: capi.cross_entropy(logits, ld, 0, 255, None, labels, None, 1.0, dl, lddl, stats),
        "ld < C": lambda: capi.cross_entropy(logits, 6, 7, 255, None, labels, None, 1.0, dl, lddl, stats),
        "lddl < C": lambda: capi.cross_entropy(logits, ld, 7, 255, None, labels, None, 1.0, dl, 6, stats),
        "no labels": lambda: capi.cross_entropy(logits, ld, 7, 255, None, None, None, 1.0, dl, lddl, stats),
        "cap: no count": lambda: capi.cross_entropy_cap(logits, ld, 7, 255, None, None, labels, None, 1.0, dl, lddl, stats),
        "cap: lddl < C": lambda: capi.cross_entropy_cap(logits, ld, 7, 255, n_dev, None, labels, None, 1.0, dl, 6, stats),
    }.items():
        with pytest.raises(capi.ErcGraftError):
            call()
        print("refused:", what)
    torch.cuda.synchronize()
    assert bool((dl == SENT).all()) and bool((stats[:STATS] == 0).all()) and bool((stats[STATS:] == SENT).all())
