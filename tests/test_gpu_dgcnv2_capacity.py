"""GPU: the conv-emotion DialogueGCN (--module=dgcnv2) in capacity mode -- the positional edge attention with the step count on
the device (erc_dgcnv2_edge_att_*_cap) against the existing entry points launched with T = *t_dev (bit for bit) and against
float64, the 300-wide matching attention's tail, the capacity step against the exact-shape step and the CPU restatement after a
larger batch has used the same bucket, dropout with the applied masks, bucket graph replay against eager steps on the bucket's
buffers, resident epochs against the bucketed loop, eval_scores, and the command line.

Measured on one MI355X (every test prints its figures): the capacity step's loss differs from the
exact-shape step's by 1.2e-7 (LSTM) / 0 (base None), its gradients by at most 2.4e-7 / 1.7e-7 of a parameter's largest entry (the
weight-gradient products sum over the capacity rows), both steps within 4.7e-6 / 4.0e-7 of the CPU restatement (bound 1e-3);
parameters after three Adam steps within 3.0e-8 / 1.5e-8.  Resident epochs end bit-equal to the bucketed loop and eval_scores'
logits are bit-equal to the exact-shape eval forward's (printed, not asserted: the bounds are the issue's).  The edge attention
with t_dev = 37 of 110 is within 7.6e-8 (norm) / 7.2e-8 (dS) of float64."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from erc_amd import capi
from tests import att_kernels_ref as R
from tests import dgcnv2_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASES = ("LSTM", "None")
STALE = 12345.0
D_M = 24
W6 = torch.tensor([1 / 0.086747, 1 / 0.144406, 1 / 0.227883, 1 / 0.160585, 1 / 0.127711, 1 / 0.252668])


@pytest.fixture(scope="module", autouse=True)
def _lib():
    capi.lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stale(*shape):
    return torch.full(shape, STALE, dtype=torch.float32, device=DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def plus_zero(a):
    """every element is +0.0, bit for bit"""
    return bool((np.ascontiguousarray(a).view(np.uint32) == 0).all())


def is_stale(a):
    return bool((a == np.float32(STALE)).all())


# ------------------------------------------------------------------------------------------------------- edge attention
B_E, T_CAP_E, LDS, GUARD = 4, 110, 112, 2


@pytest.fixture(scope="module")
def edge_inputs():
    """S [T_cap, B, ldS] (pad columns stale; large scores on the rows behind every length, so the 1e-10 leak matters), shared by
    every case and left unchanged"""
    r = np.random.RandomState(77)
    S = np.full((T_CAP_E, B_E, LDS), STALE, np.float32)
    S[:, :, :R.NSCAL] = r.randn(T_CAP_E, B_E, R.NSCAL)
    S[12:, 1, :R.NSCAL] += 25.0
    S[1:, 3, :R.NSCAL] += 25.0
    return S


def _edge_graph(lens, wp, wf):
    g = R.edge_lists(lens, wp, wf)
    tail = np.full(3, -1, np.int32)      # never read
    gd = dict(node_off=dev(R.offsets(lens).astype(np.int32)), out_ptr=dev(g["out_ptr"]),
              out_dst=dev(np.concatenate([g["out_dst"], tail])), out_eid=dev(np.concatenate([g["out_eid"], tail])))
    return g, gd


def _edge_run(S, gd, n_e, parts, stride, wp, wf, T, t_dev=None):
    """forward + backward on stale outputs; t_dev None: the existing entry points with T; else the capacity ones with T_cap"""
    norm, dS = stale(n_e + 5), stale(T_CAP_E * B_E + GUARD, LDS)
    td = None if t_dev is None else torch.tensor([t_dev], dtype=torch.int32, device=DEV)
    capi.dgcnv2_edge_att_fwd(S, LDS, gd, B_E, T, wp, wf, norm, t_dev=td)
    capi.dgcnv2_edge_att_bwd(S, LDS, gd, B_E, T, wp, wf, parts, dS, dn_parts=2, dn_stride=stride, t_dev=td)
    return host(norm), host(dS)


@pytest.mark.parametrize("t_dev", [1, 37, 64, 65, 110])
@pytest.mark.parametrize("window", [(10, 10), (-1, -1)])
def test_edge_attention_with_device_step_count_equals_the_exact_launch(edge_inputs, window, t_dev):
    """B = 4, T_cap = 110, lengths [t_dev, 12, 0, 1]: norm and rows t < t_dev of dS are bit-identical to the existing entry
    points launched with T = t_dev on the same B (where t_dev < 12 the exact launch's grid covers the first ceil(t_dev / 4) * 4
    sources alone: the edges it writes are compared, the capacity launch writes every edge); rows t >= t_dev and the whole
    length-0 slot are +0 over stale values; guard rows, pad columns and norm behind the edges stay stale; a second launch is
    bit-identical"""
    wp, wf = window
    lens = [t_dev, 12, 0, 1]
    g, gd = _edge_graph(lens, wp, wf)
    n_e = len(g["src"])
    stride = n_e + 5
    r = np.random.RandomState(t_dev)
    parts_h = np.full((2, stride), STALE, np.float32)
    parts_h[:, :n_e] = r.randn(2, n_e)
    S0 = edge_inputs.reshape(T_CAP_E * B_E, LDS)
    S, parts = dev(S0), dev(parts_h.reshape(-1))
    n_x, d_x = _edge_run(S, gd, n_e, parts, stride, wp, wf, t_dev)
    n_c, d_c = _edge_run(S, gd, n_e, parts, stride, wp, wf, T_CAP_E, t_dev=t_dev)
    n_c2, d_c2 = _edge_run(S, gd, n_e, parts, stride, wp, wf, T_CAP_E, t_dev=t_dev)
    assert same_bits(host(S), S0) and same_bits(host(parts), parts_h.reshape(-1)), "an input was written"
    wrote = n_x[:n_e] != np.float32(STALE)
    assert wrote.any() and (t_dev < 12 or wrote.all())
    assert same_bits(n_c[:n_e][wrote], n_x[:n_e][wrote])
    assert not np.isnan(n_c[:n_e]).any() and not (n_c[:n_e] == np.float32(STALE)).any(), "every edge is written"
    assert is_stale(n_c[n_e:]) and is_stale(d_c[T_CAP_E * B_E:]) and is_stale(d_c[:, R.NSCAL:])
    dx = d_x[:T_CAP_E * B_E].reshape(T_CAP_E, B_E, LDS)[:, :, :R.NSCAL]
    dc = d_c[:T_CAP_E * B_E].reshape(T_CAP_E, B_E, LDS)[:, :, :R.NSCAL]
    assert same_bits(dc[:t_dev], dx[:t_dev]) and is_stale(dx[t_dev:])
    assert plus_zero(dc[t_dev:]) and plus_zero(dc[:, 2])
    for b, L in enumerate(lens):
        assert plus_zero(dc[:, b, L:]), (b, "columns of absent sources")
    assert t_dev == 1 or float(np.abs(dc[:t_dev, 0, :t_dev]).max()) > 0          # (a softmax over one row has no gradient)
    assert same_bits(n_c2, n_c) and same_bits(d_c2, d_c), "second launch"


def test_edge_attention_with_a_zero_step_count_gives_zeros(edge_inputs):
    lens = [0, 12, 0, 1]
    g, gd = _edge_graph(lens, 10, 10)
    n_e = len(g["src"])
    parts = dev(np.random.RandomState(0).randn(2 * (n_e + 5)).astype(np.float32))
    S = dev(edge_inputs.reshape(T_CAP_E * B_E, LDS))
    n_c, d_c = _edge_run(S, gd, n_e, parts, n_e + 5, 10, 10, T_CAP_E, t_dev=0)
    assert plus_zero(n_c[:n_e]) and is_stale(n_c[n_e:])
    assert plus_zero(d_c[:T_CAP_E * B_E, :R.NSCAL]) and is_stale(d_c[T_CAP_E * B_E:]) and is_stale(d_c[:, R.NSCAL:])
    # a negative count is clamped to 0 as well
    n_c, d_c = _edge_run(S, gd, n_e, parts, n_e + 5, 10, 10, T_CAP_E, t_dev=-3)
    assert plus_zero(n_c[:n_e]) and plus_zero(d_c[:T_CAP_E * B_E, :R.NSCAL])


def test_edge_attention_with_device_step_count_against_float64(edge_inputs):
    """t_dev = 37, lengths [37, 12, 0, 1], window 10/10 against the float64 restatement of tests/att_kernels_ref.py over the
    batch's own 37 rows, within that file's bounds for the exact kernels (4 x the float32 twin's worst figure)"""
    lens, t_dev = [37, 12, 0, 1], 37
    g, gd = _edge_graph(lens, 10, 10)
    n_e = len(g["src"])
    stride = n_e + 5
    parts_h = np.zeros((2, stride), np.float32)
    parts_h[:, :n_e] = np.random.RandomState(5).randn(2, n_e)
    dn = parts_h[:, :n_e].astype(np.float64).sum(0)
    want = R.edge(edge_inputs[:t_dev, :, :R.NSCAL], lens, t_dev, 10, 10, g, dn)
    S = dev(edge_inputs.reshape(T_CAP_E * B_E, LDS))
    n_c, d_c = _edge_run(S, gd, n_e, dev(parts_h.reshape(-1)), stride, 10, 10, T_CAP_E, t_dev=t_dev)
    dc = d_c[:T_CAP_E * B_E].reshape(T_CAP_E, B_E, LDS)[:t_dev, :, :R.NSCAL]
    fig = R.edge_figures(dict(norm=n_c[:n_e], dS=dc), want)
    print("edge attention (t_dev = 37 of 110) against float64: norm %.2e (bound %.0e), dS %.2e (bound %.0e)"
          % (fig["norm"], R.BOUND["edge"]["norm"], fig["dS"], R.BOUND["edge"]["dS"]))
    for k, v in fig.items():
        assert v <= R.BOUND["edge"][k], (k, v)


def test_edge_attention_capacity_refusals():
    S, dS, norm = stale(4, 110), stale(4, 110), stale(8)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)
    gd = dict(node_off=i32(2), out_ptr=i32(1), out_dst=i32(1), out_eid=i32(1))
    td = i32(1)
    with pytest.raises(capi.ErcGraftError, match="110"):
        capi.dgcnv2_edge_att_fwd(S, 110, gd, 1, 111, 10, 10, norm, t_dev=td)
    with pytest.raises(capi.ErcGraftError, match="110"):
        capi.dgcnv2_edge_att_bwd(S, 110, gd, 1, 111, 10, 10, norm, dS, t_dev=td)
    with pytest.raises(capi.ErcGraftError, match="alias"):
        capi.dgcnv2_edge_att_bwd(S, 110, gd, 1, 4, 10, 10, norm, S, t_dev=td)
    torch.cuda.synchronize()
    assert is_stale(host(S)) and is_stale(host(dS)) and is_stale(host(norm))


# ------------------------------------------------------------------------------------------- matching attention, width 300
def test_matching_attention_tail_at_width_300():
    """MatchAttHead.att_backward in capacity mode at width 300 (erc_match_att_bwd_cap is built for 200 and still refuses):
    rows < N of dQ / dE bit-identical to erc_match_att_bwd, rows [N, N_cap) +0 over stale values, rows >= N_cap untouched"""
    from erc_amd.matchhead import MatchAttHead
    F, lens, T, n_cap = 300, [12, 67, 0, 3], 70, 128
    B, N = len(lens), sum(lens)
    g = torch.Generator().manual_seed(3)
    rnd = lambda *s: (torch.randn(*s, generator=g) * 0.3).to(DEV)
    E, Q, dA = rnd(n_cap, F), rnd(n_cap, F), rnd(n_cap, F)
    node_off = dev(R.offsets(lens).astype(np.int32))
    A, P, TH = stale(n_cap, F), torch.zeros(B * T * T, device=DEV), torch.zeros(B * T * T, device=DEV)
    capi.match_att_fwd(E, F, Q, F, node_off, B, T, F, A, F, P, TH)
    n_dev = torch.tensor([N, 67], dtype=torch.int32, device=DEV)
    head = MatchAttHead(None, "", F, 100, 6, 0.0)
    pair = stale(2 * n_cap + 1 + GUARD, F)
    ws = dict(Q=Q, dA=dA, P=P, TH=TH, DZ=torch.zeros(B * T * T, device=DEV), dQdE=pair, dQ=pair[:n_cap], dE=pair[n_cap:])
    head.att_backward(ws, E, node_off, B, T, n_dev=n_dev, n_cap=n_cap)
    dQx, dEx = stale(n_cap, F), stale(n_cap, F)
    capi.match_att_bwd(E, F, Q, F, dA, F, node_off, B, T, F, P, TH, torch.zeros(B * T * T, device=DEV), dQx, F, dEx, F)
    got, dQx, dEx = host(pair), host(dQx), host(dEx)
    assert same_bits(got[:N], dQx[:N]) and same_bits(got[n_cap:n_cap + N], dEx[:N])
    assert is_stale(dQx[N:]) and is_stale(dEx[N:])
    assert plus_zero(got[N:n_cap]) and plus_zero(got[n_cap + N:2 * n_cap])
    assert is_stale(got[2 * n_cap:]), "the zero row's place behind dE and the guard rows"
    # the pinned refusal stays, and without the paired buffer the head refuses before any launch
    dQx_d = stale(n_cap, F)
    with pytest.raises(capi.ErcGraftError):
        capi.match_att_bwd(E, F, Q, F, dA, F, node_off, B, T, F, P, TH, ws["DZ"], dQx_d, F, stale(n_cap, F), F, n_cap=n_cap)
    with pytest.raises(capi.ErcGraftError, match="tail_pair"):
        head.att_backward(dict(ws, dQdE=None), E, node_off, B, T, n_dev=n_dev, n_cap=n_cap)
    assert is_stale(host(dQx_d))


# ----------------------------------------------------------------------------------------------------------- the step
def _case(lens, D, S, C, seed):
    g = torch.Generator().manual_seed(seed)
    B, T = len(lens), max(lens)
    x = torch.randn(T, B, D, generator=g) * 0.5
    onehot = torch.nn.functional.one_hot(torch.randint(0, S, (T, B), generator=g), S).float()
    for b, L in enumerate(lens):
        x[L:, b] = 0.0
        onehot[L:, b] = 0.0
    return {"input_tensor": x, "speaker_tensor": onehot, "text_length": torch.tensor(lens, dtype=torch.int64),
            "attention_mask": (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float(),
            "label": torch.randint(0, C, (sum(lens),), generator=g)}


def _trainer(base, extra=(), t_cap=70, batch_size=4):
    from track_mm.dgcnv2 import DGCNParams
    from erc_amd.dgcnv2 import DGCNv2Trainer
    params = DGCNParams().from_args(["--dataset=iemocap-cogmen-6", "--base_model=%s" % base, "--train.batch_size=%d" % batch_size]
                                    + list(extra))
    params.hidden_audio, params.hidden_text, params.hidden_visual, params.hidden_all = 4, 12, 8, D_M
    tr = DGCNv2Trainer(params, DEV)
    tr.t_cap = t_cap
    return tr


def _host_params(tr):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}


def _state(tr):
    """everything a training step changes (what StepGraphs.precapture snapshots)"""
    flat, opt = tr.model.flat, tr.optim
    ts = [t for t in (getattr(flat, n, None) for n in ("data", "exp_avg", "exp_avg_sq", "grad_full")) if t is not None]
    if getattr(opt, "state", None) is not None:
        ts.append(opt.state)
    return ts


def _snapshot(tr):
    return [(t, t.clone()) for t in _state(tr)]


def _restore(snap):
    with torch.no_grad():
        for t, keep in snap:
            t.copy_(keep)
    torch.cuda.synchronize()


def _params(tr):
    return tr.model.flat.data.detach().clone()


def _grads(tr):
    return {k: tr.model.flat.g(k).detach().cpu().clone() for k in tr.model.flat.params}


def _capacity_step(tr, static, fill, batch, step=False):
    fill(static, batch)
    tr.model.dynamic_n = True
    try:
        stats = tr.train_step(static) if step else tr.model.loss_and_grads(static, tr.class_weight)
    finally:
        tr.model.dynamic_n = False
    torch.cuda.synchronize()
    return stats


def _grad_figures(got, want):
    """worst |got - want| / (largest |want| entry) over the live parameters; the dead ones must have no gradient"""
    worst = 0.0
    for name, g in want.items():
        if name.startswith(O.DEAD):
            assert g is None and name not in got, name
            continue
        scale = float(g.abs().max()) + 1e-6
        e = float((got[name] - g).abs().max())
        assert torch.isfinite(got[name]).all() and e <= 1e-3 * scale, (name, e, scale)       # test_gpu_dgcnv2._check_grads
        worst = max(worst, e / scale)
    return worst


SMALL, BIG = [12, 67, 3], [70, 30, 20, 8]          # N = 82 (one empty slot) and N = 128: the (4, 70, 128) bucket


@pytest.mark.parametrize("base", BASES)
def test_capacity_step_matches_the_oracle_like_the_exact_step_after_a_larger_batch(base):
    """dropout 0, bucket (4, 70, 128): lengths [70, 30, 20, 8] run through the bucket first, then [12, 67, 3] from the same
    parameters.  Loss and every gradient of the capacity step AND of the exact-shape step against tests/dgcnv2_oracle.py, both
    inside the bounds tests/test_gpu_dgcnv2.py holds the exact step to (loss 1e-4, gradients 1e-3 of the largest entry); the
    first Adam step against the oracle's and three Adam steps against the exact-shape loop inside that file's Adam bounds.
    The largest deviation between the two GPU steps is printed."""
    tr = _trainer(base, ["--capacity_buckets=True", "--dropout=0"])
    tr.model.train()
    c_small, c_big = _case(SMALL, D_M, 2, 6, 1), _case(BIG, D_M, 2, 6, 2)
    small, big = tr.prepare_batch(c_small), tr.prepare_batch(c_big)
    key, make, fill = tr.capacity_bucket(small)
    assert key == ("capacity", 4, 70, 128)
    static = make()
    P = _host_params(tr)
    loss, _, _, want = O.loss_and_grads(P, c_small, base, W6)
    exact = tr.model.loss_and_grads(small, tr.class_weight)[:3].clone()
    torch.cuda.synchronize()
    g_exact = _grads(tr)
    e_exact = _grad_figures(g_exact, want)
    _capacity_step(tr, static, fill, big)
    stats = _capacity_step(tr, static, fill, small)
    ws = tr.model._last_ws
    assert ws["counts"].tolist() == [82, 67]
    g_cap = _grads(tr)
    e_cap = _grad_figures(g_cap, want)
    d_exact, d_cap = abs(float(exact[0]) - float(loss)), abs(float(stats[0]) - float(loss))
    between = max(float((g_cap[k] - g_exact[k]).abs().max()) / (float(g_exact[k].abs().max()) + 1e-6) for k in g_exact)
    print("dgcnv2 %s: |loss - oracle| exact %.3g capacity %.3g; worst gradient deviation from the oracle exact %.3g capacity "
          "%.3g; capacity vs exact: |loss diff| %.3g, worst gradient deviation %.3g of the largest entry"
          % (base, d_exact, d_cap, e_exact, e_cap, abs(float(stats[0]) - float(exact[0])), between))
    assert d_exact < 1e-4 and d_cap < 1e-4
    assert float(stats[1]) == float(exact[1]) and abs(float(stats[2]) - float(exact[2])) < 1e-3
    # what the tails own is zero past the batch, whatever the larger batch left; the padded gradients too
    for k in ("dQ", "dA", "dZc", "dlogits"):
        assert bool((ws[k][82:128] == 0).all()), k
    assert bool((ws["dE"][82:] == 0).all()) and ws["dE"].shape[0] == 129
    assert bool((ws["E"][82:, :200] == 0).all()) and bool((ws["AGG"][82:] == 0).all()) and bool((ws["dHc"][82:] == 0).all())
    dS, dM = ws["dS"].view(70, 4, 110), ws["dM"].view(70, 4, 200)
    assert bool((dS[67:] == 0).all()) and bool((dS[:, 3] == 0).all()) and bool((dM[67:] == 0).all()) and bool((dM[:, 3] == 0).all())
    assert float(dS[:67, :3].abs().max()) > 0 and bool((ws["M"][280] == 0).all())
    # Adam: the first step against the oracle's, three steps against the exact-shape loop
    snap = _snapshot(tr)
    p_want = O.adam_step(P, want, lr=3e-4)
    _capacity_step(tr, static, fill, small, step=True)
    sd = _host_params(tr)
    for k in tr.model.flat.params:
        d = (sd[k] - p_want[k]).abs()
        assert float((d > 1e-5).float().mean()) < 0.01 and float(d.max()) < 7e-4, k
    for k in P:
        if k.startswith(O.DEAD):
            assert torch.equal(sd[k], P[k]), k
    _restore(snap)
    for _ in range(3):
        tr.train_step(small)
    torch.cuda.synchronize()
    p_exact = _params(tr)
    _restore(snap)
    _capacity_step(tr, static, fill, big, step=True)              # leaves its rows in the bucket's workspace ...
    _restore(snap)                                                # ... and nothing in the parameters
    for _ in range(3):
        _capacity_step(tr, static, fill, small, step=True)
    d = (_params(tr) - p_exact).abs()
    print("dgcnv2 %s capacity vs exact after 3 Adam steps: max |dp| = %.3g, share above 1e-5 = %.3g"
          % (base, float(d.max()), float((d > 1e-5).float().mean())))
    assert float((d > 1e-5).float().mean()) < 0.01 and float(d.max()) < 7e-4


def test_capacity_dropout_step_matches_oracle_with_the_applied_masks():
    """training mode in the bucket (4, 70, 128): the masks of the LSTM's inter-layer dropout (padded row t*B_cap + b) and of
    the classifier are read back from the step's buffers; the CPU restatement given those masks reproduces loss and gradients
    within the exact step's bounds; keep rates near 0.6"""
    lens = [14, 30, 1]
    batch = _case(lens, D_M, 2, 6, 8)
    B, T, N = len(lens), max(lens), sum(lens)
    tr = _trainer("LSTM", ["--capacity_buckets=True"])
    tr.model.train()
    P = _host_params(tr)
    key, make, fill = tr.capacity_bucket(tr.prepare_batch(batch))
    assert key == ("capacity", 4, 70, 128)
    static = make()
    stats = _capacity_step(tr, static, fill, tr.prepare_batch(batch))
    ws = tr.model._last_ws
    assert ws["counts"].tolist() == [N, T]
    keep = 1.0 / 0.6
    enc = ws["lstm:lstm."]
    cut = lambda v: v.view(70, 4, 200)[:T, :B].cpu()
    pre, post = cut(enc["H0"]), cut(enc["H0d"])
    kept = post != 0
    on = kept & (pre != 0)
    assert torch.allclose(post[on], pre[on] * keep, rtol=1e-6, atol=0)
    assert bool((enc["H0"].view(70, 4, 200)[T:] == 0).all()), "rows t >= t_dev of the scan's output are written 0"
    lin = ws["A"][:N].cpu() @ P["graph_net.linear.weight"].t() + P["graph_net.linear.bias"]
    z = ws["Zc"][:N].cpu()
    mask_clf = torch.where((z != 0) | (lin <= 0), torch.full_like(lin, keep), torch.zeros_like(lin))
    r0, r1 = float(kept.float().mean()), float((z != 0).float().sum() / (lin > 0).float().sum())
    print("dgcnv2 capacity dropout: keep rates %.3f (LSTM) %.3f (classifier)" % (r0, r1))
    assert 0.55 < r0 < 0.65 and 0.5 < r1 < 0.7, (r0, r1)
    loss, _, _, grads = O.loss_and_grads(P, batch, "LSTM", W6, masks={"lstm": kept.float() * keep, "clf": mask_clf})
    assert abs(float(stats[0]) - float(loss)) < 1e-4
    _grad_figures(_grads(tr), grads)


FOUR = ([12, 67, 3], [70, 20, 8], [5] * 4, [1, 2, 60, 30])          # all in the (4, 70, 128) bucket, none of its exact shape


@pytest.mark.parametrize("base", BASES)
def test_bucket_graph_over_four_batches_equals_eager_steps_on_the_buckets_buffers(base):
    """StepGraphs with the buckets on (dropout 0.5): first batch eager + capture, three replays -- bit-identical to the same
    four steps run eagerly on the bucket's static buffers (capture=False); replaying one batch twice from a restored state is
    bit-identical"""
    from erc_amd.trainer import StepGraphs
    batches = [_case(l, D_M, 2, 6, 20 + i) for i, l in enumerate(FOUR)]
    ends = []
    for capture in (False, True):
        tr = _trainer(base, ["--capacity_buckets=True", "--dropout=0.5"])
        assert tr.model.drop_p == 0.5
        g = StepGraphs(tr, capture=capture)
        losses = []
        for b in batches:
            losses.append(g.step(tr.prepare_batch(b))[0].clone())
        torch.cuda.synchronize()
        assert list(g.cache) == [("capacity", 4, 70, 128)]
        assert (g.captures, g.replays, g.eager) == ((1, 3, 1) if capture else (0, 0, 4))
        assert not tr.model.dynamic_n
        ends.append((_params(tr), [float(v) for v in losses]))
    assert all(np.isfinite(ends[0][1]))
    assert torch.equal(ends[0][0], ends[1][0]) and ends[0][1] == ends[1][1]
    snap = _snapshot(tr)
    b = tr.prepare_batch(batches[3])
    outs = []
    for _ in range(2):
        _restore(snap)
        g.step(b)
        torch.cuda.synchronize()
        outs.append(_params(tr))
    assert g.replays == 5 and torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], ends[1][0])


def _dialogues(p, n, seed, max_len=45):
    from erc_amd.synthetic import make_dialogues
    return make_dialogues(n, p.dims(), n_speakers=p.n_speakers, n_classes=p.n_classes, min_len=1, max_len=max_len, seed=seed)


@pytest.mark.parametrize("base", BASES)
def test_resident_epochs_equal_the_bucketed_loop(base):
    """two epochs from a DeviceDialogueStore (12 dialogues, B = 4: one 2 B int32 copy + one replay per step) against StepGraphs
    fed the batches of the same permutations: per-epoch loss sums within 1e-4 per step, final parameters within the Adam bounds;
    whether they are bit-equal is printed"""
    from erc_amd.datasets import DeviceDialogueStore
    from erc_amd.trainer import ResidentEpochs, StepGraphs
    Bsz, seed = 4, 3
    ends = []
    for mode in ("resident", "bucketed"):
        tr = _trainer(base, ["--capacity_buckets=True"], t_cap=0, batch_size=Bsz)
        p = tr.params
        store = DeviceDialogueStore(_dialogues(p, 12, 9), p, torch.device(DEV))
        tr.t_cap = int(store.lengths.max())
        tr.model.train()
        sums = []
        if mode == "resident":
            res = ResidentEpochs(tr, store, Bsz, seed)
            assert res.supported()
            prev = 0.0
            for _ in range(2):
                n_utt, n_steps = res.epoch()
                torch.cuda.synchronize()
                tot = float(res.acc[0])
                sums.append(tot - prev)
                prev = tot
            assert n_steps == 3 and res.replays > 0 and res.eager == res.captures <= 2
        else:
            g, gen = StepGraphs(tr), torch.Generator().manual_seed(seed)
            for _ in range(2):
                order = torch.randperm(len(store), generator=gen)
                acc = torch.zeros((), dtype=torch.float64, device=DEV)
                for i in range(0, len(store), Bsz):
                    acc += g.step(tr.prepare_batch(store.batch(order[i:i + Bsz])))[0].double()
                torch.cuda.synchronize()
                sums.append(float(acc))
            assert g.replays > 0
        ends.append((_params(tr), sums))
    (p_res, s_res), (p_buc, s_buc) = ends
    d = (p_res - p_buc).abs()
    print("dgcnv2 %s resident vs bucketed: epoch loss sums %s vs %s, max |dp| = %.3g, bit-equal parameters: %s"
          % (base, s_res, s_buc, float(d.max()), torch.equal(p_res, p_buc)))
    assert all(np.isfinite(s_res)) and all(abs(a - b) <= 3 * 1e-4 for a, b in zip(s_res, s_buc))
    assert float((d > 1e-5).float().mean()) < 0.01 and float(d.max()) < 7e-4


@pytest.mark.parametrize("base", BASES)
def test_eval_scores_is_the_confusion_matrix_of_its_own_logits(base):
    """a resident test epoch over a 6-dialogue store (B = 4, every step eager): cm equals the confusion matrix computed on the
    host from the logits buffer of the very same steps (integer-exact); those logits are within the forward bound (1e-4) of the
    exact-shape eval forward; cm is added to; the training flag and the dropout counter stay as they were"""
    from erc_amd.datasets import DeviceDialogueStore
    from erc_amd.trainer import ResidentEval
    tr = _trainer(base, ["--device_collate", "--resident", "--resident_eval"], t_cap=0)
    p = tr.params
    store = DeviceDialogueStore(_dialogues(p, 6, 4), p, torch.device(DEV))
    tr.model.train()
    tr.train_step(tr.prepare_batch(store.batch([0, 1])))          # a non-zero dropout counter
    torch.cuda.synchronize()
    rng0, last0 = tr.model.rng_state.clone(), tr.model._last_ws
    seen = []

    class Eval(ResidentEval):
        def _step(self, batch):
            ws = super()._step(batch)
            torch.cuda.synchronize()
            seen.append((ws["logits"].cpu().clone(), ws["counts"].tolist(), ws["label"].cpu().clone()))
            return ws

    ev = Eval(tr, store, 4, capture=False)
    assert ev.supported() and ev.steps == 2
    cm = ev.epoch().numpy()
    assert tr.model.training and torch.equal(tr.model.rng_state, rng0) and tr.model._last_ws is last0
    want = np.zeros((6, 6), np.int64)
    lens = store.lengths.tolist()
    for s, (logits, counts, label) in enumerate(seen):
        idx = list(range(4 * s, min(4 * s + 4, 6)))
        n = sum(lens[i] for i in idx)
        assert counts == [n, max(lens[i] for i in idx)]
        np.add.at(want, (label[:n].numpy(), logits[:n].argmax(-1).numpy()), 1)
        batch = store.batch(idx)
        assert torch.equal(label[:n], batch["label"].cpu())
        tr.model.eval()
        exact = tr.to_logits(tr.prepare_batch(batch))
        tr.model.train()
        err = float((exact.cpu() - logits[:n]).abs().max())
        print("dgcnv2 %s eval_scores step %d: max |logit - exact-shape logit| = %.3g" % (base, s, err))
        assert err < 1e-4
    assert len(seen) == 2 and int(want.sum()) == sum(lens)
    np.testing.assert_array_equal(cm, want)
    # added to, not overwritten: the last step once more on the cm the epoch left
    last = np.zeros((6, 6), np.int64)
    logits, counts, label = seen[-1]
    np.add.at(last, (label[:counts[0]].numpy(), logits[:counts[0]].argmax(-1).numpy()), 1)
    ev._step(ev._batch(ev.caps[-1]))
    np.testing.assert_array_equal(ev.cm.cpu().numpy(), want + last)
    assert tr.model.training and torch.equal(tr.model.rng_state, rng0) and not tr.model.dynamic_n


# -------------------------------------------------------------------------------------------------------------- CLI
def _cli(args):
    res = subprocess.run([sys.executable, "train_mm.py"] + args, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    return [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]


RAGGED = ["--dataset=iemocap-cogmen-6", "--modality=atv", "--n_train=24", "--n_test=6", "--syn_min_len=3", "--syn_max_len=60",
          "--train.batch_size=4", "--test.batch_size=4"]


def test_train_mm_cli_resident_and_resident_eval():
    """``train_mm.py --module=dgcnv2 --device_collate --resident --resident_eval`` on ragged synthetic dialogues: exit 0, finite
    losses, a handful of captured bucket graphs, everything else a replay, the test line from the device-scored matrix"""
    lines = _cli(["--module=dgcnv2", "--epoch=3", "--device_collate", "--resident", "--resident_eval"] + RAGGED)
    epochs = [l for l in lines if "test" in l]
    losses = [l["Lall"] for l in lines if "Lall" in l]
    assert len(epochs) == 3 and len(losses) == 3 and all(np.isfinite(losses))
    last = epochs[-1]
    n_buckets = -(-4 * 60 // 128)
    assert last["graph_replays"] > 0 and 0 < last["graphs_captured"] <= n_buckets
    assert last["eager_steps"] == last["graphs_captured"]
    assert last["graph_replays"] + last["eager_steps"] == 3 * 6
    for e in epochs:
        assert "test_s" in e and 0.0 <= e["test"]["acc"] <= 1.0          # scored from the device's confusion matrix


@pytest.mark.parametrize("base", BASES)
def test_train_mm_cli_default_losses_are_those_of_the_exact_shape_loop(base):
    """the same command line WITHOUT the new flags prints the first-epoch step losses recorded on the commit before capacity
    mode (tests/golden/dgcnv2_cli_default_losses.json): the default path is untouched"""
    with open(os.path.join(REPO, "tests", "golden", "dgcnv2_cli_default_losses.json")) as fh:
        golden = json.load(fh)
    lines = _cli(["--module=dgcnv2", "--epoch=1", "--device_collate", "--base_model=%s" % base] + RAGGED)
    steps = [l["Lall"] for l in lines if "Lall" in l and "step" in l]
    assert steps == golden[base]
    last = [l for l in lines if "test" in l][-1]
    assert last["graphs_captured"] == 0 and last["eager_steps"] == 6      # exact shapes: none repeats in one epoch
