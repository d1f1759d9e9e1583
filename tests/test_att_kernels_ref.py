"""Host tests of tests/att_kernels_ref.py (no GPU): the float64 restatements of CIM's cross-modal attention, the matching attention
and the positional edge attention against independent float64 autograd forms, what the case tables claim to reach, and the
float32 twins against the recorded figures the GPU bounds are derived from."""
import numpy as np
import pytest
import torch

from tests import att_kernels_ref as R

TOL = 1e-12


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


# ----------------------------------------------------------------------------------------------------- independent forms
@pytest.mark.parametrize("name", [c["name"] for c in R.CIM_CASES if not c["exact"]])
def test_cim_restatement_equals_autograd_of_the_oracle(name):
    """tests/cim_oracle.cross_attention under torch.float64 autograd, the classifier's addend and the mask tail included"""
    from tests.cim_oracle import PAIRS, cross_attention
    ref = R.cim_reference(name)
    c, out = ref["c"], ref["out"]
    dense = {m: _t(ref["dense"][:, 100 * i:100 * i + 100]).requires_grad_() for i, m in enumerate("avt")}
    outs = torch.cat([cross_attention(dense[x], dense[y], c["lens"]) for x, y in PAIRS], -1)
    (outs * _t(ref["G"])).sum().backward()
    assert R.rel(out["out"], outs.detach().numpy()) < TOL
    grad = torch.cat([dense[m].grad for m in "avt"], -1).numpy() + ref["Gd"].astype(np.float64)
    assert R.rel(out["ddense_unmasked"], grad) < TOL
    assert R.rel(out["ddense"], np.where(ref["dense"] > 0, grad * c["mask_scale"], 0.0)) < TOL
    off = R.offsets(c["lens"])
    for (p, b), pm in out["P"].items():
        x, y = (_t(ref["dense"][off[b]:off[b + 1], 100 * m:100 * m + 100]) for m in (R.PAIR_X[p], R.PAIR_Y[p]))
        assert R.rel(pm, torch.softmax(x @ y.t(), -1).numpy()) < TOL


@pytest.mark.parametrize("name", [c["name"] for c in R.MATCH_CASES if not c["exact"]])
def test_matching_restatement_equals_autograd_of_the_padded_formula(name):
    """MatchingAttention 'general2' as the reference writes it: a softmax over all T padded positions of tanh(.) * mask, times the
    mask, renormalised.  Equality proves that the padded exp(0) terms cancel, as the kernel's header says"""
    ref = R.match_reference(name)
    c, out = ref["c"], ref["out"]
    T, F, off = c["T"], c["F"], R.offsets(c["lens"])
    E, Q = _t(ref["E"]).requires_grad_(), _t(ref["Q"]).requires_grad_()
    rows, saves = [], {}
    for b, L in enumerate(c["lens"]):
        Ep = torch.cat([E[off[b]:off[b] + L], torch.zeros(T - L, F, dtype=torch.float64)])
        mask = (torch.arange(T) < L).double()
        sc = Q[off[b]:off[b] + L] @ Ep.t()
        sc.retain_grad()
        th = torch.tanh(sc * mask)
        alpha = torch.softmax(th, -1) * mask
        alpha = alpha / alpha.sum(-1, keepdim=True)
        rows.append(alpha @ Ep)
        saves[b] = (alpha[:, :L].detach().numpy(), th[:, :L].detach().numpy(), sc)
    A = torch.cat(rows)
    (A * _t(ref["dA"])).sum().backward()
    assert R.rel(out["A"], A.detach().numpy()) < TOL
    assert R.rel(out["dQ"], Q.grad.numpy()) < TOL
    assert R.rel(out["dE"], E.grad.numpy()) < TOL
    for k, i in (("P", 0), ("TH", 1)):
        assert R.rel(R.blocks(out[k]), R.blocks({b: v[i] for b, v in saves.items()})) < TOL, k
    # DZ is the gradient wrt the pre-tanh scores
    assert R.rel(R.blocks(out["DZ"]), R.blocks({b: v[2].grad[:, :c["lens"][b]].numpy() for b, v in saves.items()})) < TOL


@pytest.mark.parametrize("name", [c["name"] for c in R.EDGE_CASES])
def test_edge_restatement_equals_autograd_of_the_padded_formula(name):
    """softmax over the T padded positions, times the mask (1 inside the window, 1e-10 outside, padded positions included),
    renormalised: on every window, with the edges in this file's own order"""
    ref = R.edge_reference(name)
    c, g, out = ref["c"], ref["g"], ref["out"]
    T, lens, off = c["T"], c["lens"], R.offsets(c["lens"])
    S = _t(ref["S"][:, :, :R.NSCAL]).requires_grad_()
    score = {}
    for b, L in enumerate(lens):
        for j in range(L):
            lo, hi = R.window(j, L, c["wp"], c["wf"])
            mask = torch.full((T,), R.LEAK, dtype=torch.float64)
            mask[lo:hi] = 1.0
            masked = torch.softmax(S[:, b, j], 0) * mask
            score[off[b] + j] = masked / masked.sum()
    assert ref["n_e"] == sum(R.window(j, L, c["wp"], c["wf"])[1] - R.window(j, L, c["wp"], c["wf"])[0] for L in lens for j in range(L))
    dlg = np.searchsorted(off, g["src"], side="right") - 1
    want = torch.stack([score[int(s)][int(d) - off[b]] for s, d, b in zip(g["src"], g["dst"], dlg)])
    assert R.rel(out["norm"], want.detach().numpy()) < TOL
    (want * _t(ref["dn"])).sum().backward()
    assert R.rel(out["dS"], S.grad.numpy()) < TOL
    for b, L in enumerate(lens):      # columns of absent sources receive nothing
        assert not out["dS"][:, b, L:].any()


def test_edge_lists_are_two_orders_of_one_edge_set():
    g = R.edge_lists([5, 0, 3], 1, -1)
    assert list(zip(g["src"], g["dst"]))[:4] == [(0, 0), (1, 0), (0, 1), (1, 1)]          # by destination, then source
    assert np.array_equal(g["dst"][g["out_eid"]], g["out_dst"])
    assert np.all(np.diff(g["src"][g["out_eid"]]) >= 0) and g["out_ptr"][-1] == len(g["src"]) and len(g["out_ptr"]) == 9
    for j in range(8):
        assert np.all(g["src"][g["out_eid"][g["out_ptr"][j]:g["out_ptr"][j + 1]]] == j)


# ----------------------------------------------------------------------------------------------------- what the tables reach
def _empty_front_middle_end(lens):
    live = [i for i, L in enumerate(lens) if L]
    return lens[0] == 0 and lens[-1] == 0 and any(L == 0 for L in lens[live[0]:live[-1]])


def test_cim_table_reaches_the_mask_arms_the_lane_split_and_the_capacity_form():
    lens = [L for c in R.CIM_CASES for L in c["lens"]]
    assert {1, 64, 65, 118, 110, 2, 17} <= set(lens)
    assert {c["mask_scale"] for c in R.CIM_CASES} == {1.0, float(np.float32(1 / 0.7)), 2.0}
    assert any(_empty_front_middle_end(c["lens"]) and c["T"] > max(c["lens"]) and c["dead"] for c in R.CIM_CASES)
    assert any(c["lens"] == [3, 40] and c["T"] == 40 for c in R.CIM_CASES)
    for c in R.CIM_CASES:
        ref = R.cim_reference(c["name"])
        dense, out = ref["dense"], ref["out"]
        zero = dense == 0
        assert 0.4 < zero.mean() < 0.7 and dense.min() == 0 and 0 < dense[~zero].min() and dense.max() <= 0.65
        # the zero arm: the gradient is exactly 0 where the unmasked one is not
        assert np.all(out["ddense"][zero] == 0) and np.all(out["ddense_unmasked"][zero] != 0)
        assert np.all(ref["Gd"] != 0)
        if c["exact"]:
            twin = R.cim_reference(c["exact"])
            assert np.array_equal(twin["dense"], dense) and [L for L in c["lens"] if L] == twin["c"]["lens"]
            assert twin["c"]["mask_scale"] == c["mask_scale"] and twin["c"]["T"] == max(c["lens"])
    live = [L for L in R.CIM_CASE["L110-2-17"]["lens"]]
    assert not R.cim_reference("L110-2-17")["dense"][live[0]:live[0] + live[1], 100:200].any()


def test_matching_table_reaches_saturation_every_tile_edge_and_the_capacity_form():
    assert all(R.MATCH_CASE["F%d-ragged-%s" % (F, s)]["lens"] == [110, 1, 37, 64, 65, 16, 17, 2] for F in (200, 300) for s in ("small", "sat"))
    for c in R.MATCH_CASES:
        out = R.match_reference(c["name"])["out"]
        th = R.blocks(out["TH"])
        if c["scale"] == "sat":
            assert (1 - th * th).min() > 1e-3, c["name"]
            if len(th) > 100:
                assert np.abs(th).max() > 0.99 and 0.15 < (np.abs(np.arctanh(th)) > 3).mean() < 0.25, c["name"]
        else:
            assert np.abs(th).max() < 0.7, c["name"]
        assert len(set(R.match_pitches(c["F"]).values())) == 6 and min(R.match_pitches(c["F"]).values()) > c["F"]
        assert all(v % 4 == 0 for v in R.match_pitches(c["F"]).values())
    caps = [c for c in R.MATCH_CASES if c["tail"] is not None]
    assert {c["tail"] for c in caps} == {0, 1, 37} and all(c["F"] == 200 and c["T"] == 110 > max(c["lens"]) for c in caps)
    assert all(_empty_front_middle_end(c["lens"]) and c["lens"] == [0, 16, 0, 65, 1, 0] for c in caps)
    for c in caps:
        a, b = R.match_reference(c["name"]), R.match_reference(c["exact"])
        assert np.array_equal(a["Q"], b["Q"]) and np.array_equal(a["E"], b["E"]) and b["c"]["tail"] is None


def test_edge_table_reaches_the_second_pass_every_window_kind_and_empty_slots():
    assert {(c["wp"], c["wf"]) for c in R.EDGE_CASES} == {(10, 10), (-1, -1), (0, 0), (-1, 3), (2, -1), (40, 40)}
    assert {(c["ldS"], c["dn_parts"]) for c in R.EDGE_CASES} == {(110, 1), (110, 3), (112, 1), (112, 3)}
    deg = {c["name"]: int(np.diff(R.edge_reference(c["name"])["g"]["out_ptr"]).max()) for c in R.EDGE_CASES}
    assert deg["ragged-w-1_-1"] == 110 and deg["ragged-w40_40"] == 81 and deg["ragged-w-1_3"] > 64 and deg["ragged-w2_-1"] > 64
    assert deg["slots-w-1_-1"] == 70 and deg["ragged-w10_10"] == 21 and deg["ragged-w0_0"] == 1
    assert any(c["lens"] == [0, 9, 0, 70] and c["T"] > max(c["lens"]) for c in R.EDGE_CASES)      # empty at the front and between
    assert any(c["lens"] == [1] and c["T"] == 1 for c in R.EDGE_CASES)
    for c in R.EDGE_CASES:
        ref = R.edge_reference(c["name"])
        S = ref["S"][:, :, :R.NSCAL].astype(np.float64)
        assert (S.max(0) - S.min(0)).max() < 60, c["name"]
        assert np.isnan(ref["S"][:, :, R.NSCAL:]).all() and ref["stride"] > ref["n_e"]
        if c["T"] > 1:      # padded rows do receive gradient
            b = int(np.argmax(np.array(c["lens"]) > 0))
            assert c["lens"][b] == c["T"] or np.abs(ref["out"]["dS"][c["lens"][b]:, b, :c["lens"][b]]).max() > 0


def test_dgcnv2_meta_restatement():
    oh = np.zeros((2, 2, 3), np.float32)
    oh[0, 0] = [0, 1, 1]
    oh[0, 1] = [0.999, 0, 1]
    oh[1, 0] = [0.5, 0.5, 0]
    spk, rows, n = R.dgcnv2_meta(oh, [5, -1], 2, 2, 8)
    assert spk.tolist() == [1, 2, 0, 0] and rows.tolist() == [0, 2] and n == 2
    assert R.dgcnv2_meta(oh, [2, 1], 2, 2, 2)[1].tolist() == [0, 2]


# ----------------------------------------------------------------------------------------------------- the recorded figures
def test_float32_twins_stay_within_the_recorded_figures():
    per_case = dict(cim=[R.cim_f32_figures(c["name"]) for c in R.CIM_CASES],
                    match_small=[R.match_f32_figures(c["name"]) for c in R.MATCH_CASES if c["scale"] == "small"],
                    match_sat=[R.match_f32_figures(c["name"]) for c in R.MATCH_CASES if c["scale"] == "sat"],
                    edge=[R.edge_f32_figures(c["name"]) for c in R.EDGE_CASES])
    for fam, figs in per_case.items():
        for k, recorded in R.F32_WORST[fam].items():
            worst = max(f[k] for f in figs)
            print("%s %s: float32 twin %.2e, recorded %.2e, bound %.0e" % (fam, k, worst, recorded, R.BOUND[fam][k]))
            assert worst <= R.BOUND[fam][k], (fam, k, worst)
            assert 0.5 * recorded <= worst <= 1.5 * recorded, (fam, k, worst, recorded)
            assert 4 * recorded <= R.BOUND[fam][k] < 40 * recorded, (fam, k)
    assert R.measure() == {fam: {k: max(f[k] for f in figs) for k in figs[0]} for fam, figs in per_case.items()}
