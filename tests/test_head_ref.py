"""Host tests that tie tests/head_ref.py down: the float64 restatement against torch's float64 autograd through the layers it
restates, the recorded float32 figures (the bounds of tests/test_gpu_head.py are 4 x these), and nine deliberate errors applied to
the float32 twin, each of which the checker the GPU tests use (head_ref.check_outputs, same bounds) must reject at small shapes."""
import numpy as np
import pytest
import torch

from tests import head_ref as R


# ------------------------------------------------------------------------------------------------- against autograd
def autograd_chain(P, keep, eps):
    """nn.BatchNorm1d (training) -> leaky_relu -> Linear -> ReLU -> the given mask -> Linear -> F.cross_entropy in float64"""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    H2 = t(P["H2"]).requires_grad_(True)
    F = H2.shape[1]
    bn = torch.nn.BatchNorm1d(F, eps=eps, momentum=R.MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(t(P["gamma"]))
        bn.bias.copy_(t(P["beta"]))
    bn.train()
    y = bn(H2)
    y.retain_grad()
    h3 = torch.nn.functional.leaky_relu(y, P["slope"])
    z = torch.relu(h3 @ t(P["W0"]).T + t(P["b0"])) * t(keep)
    logits = z @ t(P["W3"]).T + t(P["b3"])
    w = t(P["weight"]) if P["weight"] is not None else None
    loss = torch.nn.functional.cross_entropy(logits, torch.from_numpy(P["labels"]), weight=w)
    loss.backward()
    n = lambda a: a.detach().numpy()
    return dict(logits=n(logits), loss=float(loss.detach()), dY=n(y.grad), dgamma=n(bn.weight.grad), dbeta=n(bn.bias.grad), dH2=n(H2.grad),
                running_mean=n(bn.running_mean), running_var=n(bn.running_var))


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max()) <= tol * max(1.0, float(np.abs(b).max()))


@pytest.mark.parametrize("N,F,C,weighted,p", [(37, 100, 6, True, 0.5), (17, 36, 7, False, 0.0), (2, 4, 1, True, 0.5), (33, 96, 8, True, 0.0),
                                              (1025, 100, 6, True, 0.5)])
def test_restatement_equals_float64_autograd(N, F, C, weighted, p):
    P = R.random_inputs(N, F, C, weighted, 11 + N)
    keep = R.keep(R.RNG[1], R.RNG[0], N, F, p)
    st = R.bn_stats(P["H2"], R.EPS, R.MOMENTUM, np.zeros(F), np.ones(F))
    out = R.head(P["H2"], st["saved"], P["gamma"], P["beta"], P["slope"], P["W0"], P["b0"], P["W3"], P["b3"], P["labels"], P["weight"], keep)
    auto = autograd_chain(P, keep, R.EPS)
    assert close(out["logits"], auto["logits"]) and close(out["stats"][0], auto["loss"])
    assert close(out["dY"], auto["dY"]) and close(out["dgamma"], auto["dgamma"]) and close(out["dbeta"], auto["dbeta"])
    assert close(R.bn_bwd_apply(P["H2"], st["saved"], P["gamma"], out["bn_bwd"], out["dY"]), auto["dH2"])
    # (torch holds momentum as a double: the restatement's float momentum moves the running statistics by 1.5e-9 relative)
    mom32 = float(np.float32(R.MOMENTUM))
    fix = lambda mine, start, new: start * (1 - R.MOMENTUM) + (mine - start * float(np.float32(1) - np.float32(R.MOMENTUM))) / mom32 * R.MOMENTUM
    assert close(fix(st["running_mean"], 0.0, None), auto["running_mean"]) and close(fix(st["running_var"], 1.0, None), auto["running_var"])
    assert int(out["stats"][1]) == int((torch.from_numpy(out["logits"]).argmax(1).numpy() == P["labels"]).sum())


def test_first_index_wins_a_tie_and_one_row_keeps_its_variance():
    lg = dict(logits=np.array([[1.0, 1.0, 0.0], [0.0, 2.0, 2.0]]))
    assert torch.from_numpy(lg["logits"]).argmax(1).tolist() == lg["logits"].argmax(1).tolist() == [0, 1]
    st = R.bn_stats(np.full((1, 4), 3.0), R.EPS, R.MOMENTUM, np.zeros(4), np.ones(4))
    assert np.allclose(st["saved"][4:], 1 / np.sqrt(np.float64(np.float32(R.EPS)))) and np.allclose(st["running_var"], float(np.float32(1) - np.float32(0.1))), st
    x = np.random.RandomState(0).randn(37, 4).astype(np.float32)
    a, b = R.bn_stats(x, R.EPS, R.MOMENTUM, np.zeros(4), np.ones(4)), R.bn_finalize(R.bn_tile_sums(x), 37, R.EPS, R.MOMENTUM, np.zeros(4), np.ones(4))
    assert close(a["saved"], b["saved"], 1e-5) and close(a["running_var"], b["running_var"], 1e-5)


def test_keep_is_the_generator_at_row_times_F_plus_col():
    from tests.test_gpu_encoder_train import erc_uniform_np
    k = R.keep(12345, 7, 5, 36, 0.5)
    u = erc_uniform_np(np.uint64(12345), 7, np.array([3 * 36 + 7], np.uint64))[0]
    assert k[3, 7] == (2.0 if u >= 0.5 else 0.0) and set(np.unique(k)) <= {0.0, 2.0}
    assert abs(float((R.keep(12345, 7, 1025, 100, 0.5) != 0).mean()) - 0.5) < 0.03


# ------------------------------------------------------------------------------------------------- the recorded float32 figures
@pytest.mark.parametrize("kind", ["random", "exact"])
def test_recorded_float32_figures_cover_every_case(kind):
    """F32_WORST (the bounds are 4 x it) is what the float32 twin measures against float64, from the restatements alone"""
    worst = {k: 0.0 for k in R.GROUPS}
    for c in R.CASES:
        for k, v in R.f32_figures(c["name"], kind).items():
            worst[k] = max(worst[k], v)
            assert v <= R.BOUND[kind][k], (c["name"], k, v)
    print(kind, {k: "%.2e" % v for k, v in worst.items()})
    for k in R.GROUPS:      # the record is reproduced: not exceeded by more than a BLAS's other summation order, not stale by 2 x
        assert worst[k] <= 1.5 * R.F32_WORST[kind][k] and worst[k] >= 0.5 * R.F32_WORST[kind][k], (k, worst[k], R.F32_WORST[kind][k])


def test_case_table_meets_every_option():
    forms = {f: [c for c in R.CASES if c["form"] == f] for f in "ABCDE"}
    small = [c for c in R.CASES if c["N"] in (17, 33)]
    nd_kind = lambda c: None if c["n_dev"] is None else "n" if c["n_dev"] == c["N"] else "1" if c["n_dev"] == 1 else \
        "n-1" if c["n_dev"] == c["N"] - 1 else "cross"
    options = dict(F=lambda c: c["F"], C=lambda c: c["C"], pad=lambda c: c["ldh"] - c["F"], weighted=lambda c: c["weighted"], p=lambda c: c["p"],
                   out=lambda c: c["out"], lddl=lambda c: c["lddl"], label_rows=lambda c: c["label_rows"], n_dev=nd_kind)
    for key, fn in options.items():
        values = {fn(c) for c in R.CASES}
        for f, cs in forms.items():
            assert {fn(c) for c in cs} == values, (key, f)
        assert {fn(c) for c in small} == values, (key, "N in {17, 33}")
    assert {c["ldb16"] for c in R.CASES if c["out"] != "f32"} == {104, 112}
    assert {c["N"] for f in "ACE" for c in forms[f] if c["N"] <= 8192} == {1, 15, 16, 17, 33, 37, 1025}
    assert {c["N"] for c in forms["B"]} == {8193, 8209, 32801} and {c["N"] for c in forms["D"]} == {8193, 8209}
    for env in {c["env"] for c in forms["E"]}:
        assert env is not None and len([c for c in forms["E"] if c["env"] == env]) <= 3


# ------------------------------------------------------------------------------------------------- mutation rejection
CHAIN_MUTATIONS = ("loss_norm_n", "unweighted_dlogits", "lrelu_sign", "dead_last_columns", "argmax_last")


def emulate(name, kind, mutation=None):
    """what a launch of the case would leave if the kernel were the float32 twin with one deliberate error: the arguments of
    head_ref.check_outputs"""
    c = R.CASE[name]
    ref = R.case_reference(name, kind)
    P = ref["P"]
    n_rows, n, F, C = c["N"], R.case_rows(c), c["F"], c["C"]
    bn = c["form"] in "CD"
    keep, saved = ref["keep"], P["saved"]
    if mutation == "dropout_pitch":      # 2: the element index taken with the pitch of H2
        from tests.test_gpu_encoder_train import erc_uniform_np
        idx = (np.arange(n, dtype=np.uint64)[:, None] * np.uint64(F + 12) + np.arange(F, dtype=np.uint64)[None, :])
        keep = (erc_uniform_np(np.uint64(R.RNG[1]), R.RNG[0], idx) >= np.float32(c["p"])) * (1.0 / (1.0 - c["p"]))
    got = {}
    if bn:
        st = R.bn_finalize(P["bn_part"], n, P["eps"], R.MOMENTUM, P["rm0"], P["rv0"], unbiased_rstd=mutation == "unbiased_rstd")      # 8
        saved = st["saved"].astype(np.float32)
        got.update(saved=saved, rm=st["running_mean"].astype(np.float32), rv=st["running_var"].astype(np.float32))
    tw = R.head_f32(P["H2"], saved, P["gamma"], P["beta"], P["slope"], P["W0"], P["b0"], P["W3"], P["b3"], P["labels"], P["weight"], keep,
                    mutation=mutation if mutation in CHAIN_MUTATIONS else None)
    mode = "f32" if c["out"] == "f32" else "both"

    def place(a, ld, prefill=np.nan, dtype=np.float32):
        full = np.full((n_rows + 2, ld), prefill, dtype)
        full[:n, :a.shape[1]] = a
        return full
    for k, ld in (("H3", F), ("Z", F), ("dZ", F), ("dY", F), ("logits", C), ("dlogits", c["lddl"] or C)):
        got[k] = place(tw[k].astype(np.float32), ld)
    if mode == "both":
        for k16, k32, ld in (("H3b", "H3", c["ldb16"]), ("Zb", "Z", c["ldb16"]), ("dZb", "dZ", c["ldb16"]), ("dlb", "dlogits", 8)):
            got[k16] = place(R.bf16_bits(tw[k32].astype(np.float32)), ld, R.NAN16, np.int16)
    groups = R.groups_of(c, n_rows, n, bn)
    rec_groups = list(groups)
    if mutation == "dropped_row":        # 1: the last valid row of the partial tile is left out of the column sums
        assert n % 16
        last = max(g for g, rows in enumerate(groups) if len(rows))
        rec_groups[last] = groups[last][:-1]
    rec = R.records(tw, rec_groups).astype(np.float32)
    if mutation == "dropped_row":
        rec[:, 224:226] = R.records(tw, groups).astype(np.float32)[:, 224:226]
    ws = np.zeros(rec.size + 16, np.float32)
    ws[:rec.size] = rec.ravel()
    got["ws"] = ws
    s = rec.astype(np.float64).sum(0)
    if mutation == "stale_record":       # 9: a record of a previous, larger launch is added to the sums
        s = s + rec[0].astype(np.float64)
    wsum = tw["wsum"]
    got.update(dbeta=s[:F].astype(np.float32), dgamma=s[112:112 + F].astype(np.float32),
               bn_bwd=(np.concatenate([s[:F], s[112:112 + F]]) / n).astype(np.float32),
               stats=np.array([s[224] / (n if mutation == "loss_norm_n" else wsum), s[225], wsum, np.nan], np.float32))
    return c, kind, ref, got, n_rows, n, mode, False


MUTATIONS = [      # (mutation, case, kinds that must reject it)
    ("dropped_row", "A-n15", ("exact", "random")), ("dropped_row", "A-n37-nd36", ("exact", "random")), ("dropped_row", "E-rows32-n17", ("exact", "random")),
    ("dropout_pitch", "A-n15", ("exact", "random")), ("dropout_pitch", "A-n37-nd36", ("exact", "random")),
    ("loss_norm_n", "A-n15", ("exact", "random")), ("loss_norm_n", "A-n33-nd15", ("exact", "random")),
    ("unweighted_dlogits", "A-n15", ("exact", "random")), ("unweighted_dlogits", "C-n17-nd17", ("exact", "random")),
    ("lrelu_sign", "A-n15", ("exact", )), ("lrelu_sign", "A-n33-nd15", ("exact", )),      # (the random inputs' gamma is positive)
    ("dead_last_columns", "A-n33-nd15", ("exact", "random")), ("dead_last_columns", "C-n17-nd17", ("exact", "random")),
    ("argmax_last", "A-n15", ("exact", )), ("argmax_last", "A-n33-nd15", ("exact", )),    # (only the exact inputs hold ties)
    ("unbiased_rstd", "C-n17-nd17", ("exact", "random")), ("unbiased_rstd", "C-n33-nd32", ("exact", "random")),
    ("stale_record", "A-n33-nd15", ("exact", "random")), ("stale_record", "C-n17-nd17", ("exact", "random")),
]


@pytest.mark.parametrize("name", sorted({m[1] for m in MUTATIONS}))
@pytest.mark.parametrize("kind", ["exact", "random"])
def test_unmutated_twin_passes_the_gpu_checker(name, kind):
    R.check_outputs(*emulate(name, kind))


@pytest.mark.parametrize("mutation,name,kinds", MUTATIONS, ids=["%s-%s" % m[:2] for m in MUTATIONS])
def test_gpu_checker_rejects_the_mutation(mutation, name, kinds):
    for kind in kinds:
        with pytest.raises(AssertionError):
            R.check_outputs(*emulate(name, kind, mutation))
