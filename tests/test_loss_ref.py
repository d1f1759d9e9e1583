"""CPU: tests/loss_ref.py's float64 cross entropy against F.cross_entropy run in float64, the conditioning of the case table
(ties for the maximum only where they were planted, row maps without duplicates), and what the two float32 forms of the softmax
lose on the four logit families -- the figure a kernel that still uses exp(z - lse) is to be judged against."""
import pytest
import torch

from tests import loss_ref as R

PAIRS = [(name, fam) for name in sorted(R.CASES) for fam in sorted(R.FAMILIES)]


@pytest.mark.parametrize("name,family", PAIRS)
def test_cross_entropy64_is_torch_in_float64(name, family):
    c = R.case(name, family)
    n, C = c["n"], c["C"]
    z = R._select(c["logits"], c["row_map"], n).double().requires_grad_()
    w = c["weight"].double() if c["weight"] is not None else None
    want = torch.nn.functional.cross_entropy(z, c["labels"], weight=w)
    want.backward()
    want = want.detach()
    loss, hits, wsum, dl = R.cross_entropy64(c["logits"], c["labels"], c["weight"], c["row_map"], n, c["grad_scale"])
    assert abs(loss - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    assert R.rel(dl, z.grad * c["grad_scale"]) <= 1e-12
    assert wsum == pytest.approx(float(w[c["labels"]].sum()) if w is not None else float(n), rel=1e-14)
    # conditioning: the maximum is attained twice exactly where a tie was planted, so first-index argmax is the only question
    # the hit count asks, and torch.argmax (which takes the first index on the CPU) agrees with it
    assert sorted(R.tied_rows(c["logits"], c["row_map"], n)) == sorted(c["ties"])
    assert len(c["ties"]) == (min(R.N_TIES, n) if C >= 2 else 0)
    assert hits == int((z.detach().argmax(-1) == c["labels"]).sum())
    first = [int(R.first_argmax(z.detach()[i:i + 1], 1)[1]) for i in c["ties"]]
    assert [int(c["labels"][i]) == f for i, f in zip(c["ties"], first)] == [True, False, True][:len(c["ties"])]
    if c["row_map"] is not None:
        rm = c["row_map"].long()
        assert rm.unique().numel() == n and int(rm.min()) >= 0 and int(rm.max()) < c["rows"] and not torch.equal(rm, rm.sort().values)
    assert int(c["labels"].min()) >= 0 and int(c["labels"].max()) < C


def test_case_table_reaches_every_value_small_and_striding():
    small = [v for v in R.CASES.values() if v[0] <= R.STRIDE_N]
    big = [v for v in R.CASES.values() if v[0] > R.STRIDE_N]
    for part in (small, big):
        assert {v[1] for v in part} >= {1, 2, 4, 6, 7}
        for col in (2, 3, 4, 6):
            assert {v[col] for v in part} == {False, True}, col
        assert {v[5] for v in part} == {1.0, 0.125}
    assert {v[0] for v in R.CASES.values()} == {1, 255, 257, 16384, 16385, 17161}


def test_empty_batch():
    c = R.case("n255_c7", "n3")
    assert R.cross_entropy64(c["logits"], c["labels"], None, None, 0, 1.0)[:3] == (0.0, 0, 0.0)


@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_what_the_two_float32_forms_of_the_softmax_lose(family):
    """exp(z - lse) against exp(z - max) / sum, both in float32 torch on the CPU, against float64: the second stays at the
    twin's level on every family, the first does not on the three wide ones.  (CPU restatements; the kernel's own figures are
    measured in tests/test_gpu_cross_entropy.py.)"""
    c = R.case("n17161_c6", family)
    z = c["logits"][:4096]
    want = torch.softmax(z.double(), -1)
    twin = R.rel(torch.softmax(z, -1), want)
    old, new = R.rel(R.softmax_lse_form32(z), want), R.rel(R.softmax_max_form32(z), want)
    print("%s: exp(z - lse) %.2e   exp(z - max) / sum %.2e   torch float32 %.2e" % (family, old, new, twin))
    bound = R.twin_bound(torch.softmax(z, -1), want)
    assert new <= bound
    if family != "n3":
        assert old > bound
