"""COGMEN above and at COGMENModule.BN_FUSED_MAX_N (8 192 nodes) in every compute mode.

Beyond that node count the training step takes another branch (cogmen.py, _forward_impl / loss_and_grads): BatchNorm's batch
statistics leave the forward tile kernel for a launch of their own (erc_bn_batch_stats), the head kernel reduces its own records,
bf16 drops the fused projection + graph-build launch while the split modes keep it (many row groups per workgroup), and the
weight-gradient launch runs several rounds of work items.  The B = 512 throughput figure of BASELINE.md runs there.  These tests
hold every mode to the oracle on both sides of the switch, at the benched shape, at the largest node count B = 512 / T = 110
admits, and across shape changes of one trainer -- at the bars of the small-shape tests (tests/test_gpu_cogmen.py,
tests/test_gpu_cogmen_split.py), and check that each case took the branch it was built for."""
import pytest
import torch

from erc_amd import capi
from tests.util_cases import cogmen_case, cogmen_case_lengths, run_cogmen_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ["f32", "f32x2", "f32x3", "f32x32", "bf16"]
SMALL_D = dict(a=12, t=20, v=16)
SBERT_D = dict(a=100, t=768, v=512)      # D = 1380, BASELINE.json configs[1]
LOGIT_TOL, GRAD_TOL = 1e-4, 2e-3


def _count_launches(monkeypatch):
    """count the calls of the entry points that tell the two branches apart"""
    calls = dict(cogmen_project_graph=0, bn_batch_stats=0, head_fused_bn=0)

    def wrap(name, fn):
        def inner(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return inner
    for name in calls:
        monkeypatch.setattr(capi, name, wrap(name, getattr(capi, name)))
    return calls


# An fp32-data step compared with the unrounded oracle can put a unit on the other side of a ReLU / LeakyReLU kink when its
# pre-activation lies within the step's own forward deviation of 0; that unit's whole gradient contribution then appears or
# vanishes.  At N = 8 193 in f32x3 / f32x32 one classifier unit (2.2e-7 from its kink) moved gcn.conv1.weight's gradient by 1.1e-2
# of its scale (a node's share of a sum over 8 k nodes with cancellation).  Every fp32-data mode is therefore compared with the
# oracle's backward on the compared path's activation pattern (util_cases.use_activation_pattern); without a flip this IS the
# strict comparison, and every flipped unit must lie within KINK_TOL of its kink: two terms deviate by ~5e-6 before the
# activations, exact fp32 and three terms by ~1e-6.
KINK_TOL = {"f32": 2e-6, "f32x2": 2e-5, "f32x3": 2e-6, "f32x32": 2e-6}


def _parity(case, compute):
    """run_cogmen_parity with the comparison each mode is credited with: fp32-data modes against the UNROUNDED oracle (KINK_TOL),
    bf16 against the oracle with its operand rounding and the projection reading the bf16 weight shadow, as under a trainer"""
    if compute == "bf16":
        return run_cogmen_parity(case, compute="bf16", w1_shadow=True)
    return run_cogmen_parity(case, compute=compute, kink_aware=True, kink_tol=KINK_TOL[compute])


def _report(tag, compute, res):
    kinks = res.get("kink_flips")
    print("%s %s: max|dlogit| %.2e (mean %.2e, scale %.2f), features %.2e, loss %.2e, worst gradient %.2e entry-wise (%s) / "
          "%.2e norm-wise, BN running mean / var %.1e / %.1e, units on the other side of a kink: %s"
          % (tag, compute, res["logit_err"], res["logit_err_mean"], res["logit_scale"], res["feat_err"], res["loss_err"],
             res["grad_err"], max(res["grad_errs"], key=res["grad_errs"].get), res["grad_norm_err"], res["bn_mean_err"],
             res["bn_var_err"], kinks))


def _check(compute, res):
    worst = sorted(res["grad_errs"].items(), key=lambda kv: -kv[1])[:6]
    if compute == "bf16":      # the bars of test_cogmen_bf16_many_nodes_path
        assert res["logit_err"] < 1e-3, res["logit_err"]
        assert res["loss_err"] < 1e-4, res["loss_err"]
        assert res["grad_err"] < 5e-2, worst
        assert res["grad_norm_err"] < 2e-2, res["grad_norm_err"]
        assert res["bn_mean_err"] < 1e-4 and res["bn_var_err"] < 1e-4, (res["bn_mean_err"], res["bn_var_err"])
        return
    # the bars of test_cogmen_split_parity / test_cogmen_fp32_parity
    assert res["logit_err"] < LOGIT_TOL, res["logit_err"]
    assert res["feat_err"] < LOGIT_TOL, res["feat_err"]
    assert res["loss_err"] < 1e-5, res["loss_err"]
    assert res["acc_match"]
    assert res["grad_err"] < GRAD_TOL, worst
    assert res["bn_mean_err"] < 1e-5 and res["bn_var_err"] < 1e-5, (res["bn_mean_err"], res["bn_var_err"])
    assert res["dead_ok"]


def _check_branch(compute, N, res, calls):
    """the step took the branch of its node count: a case that silently runs the other one tests nothing"""
    from erc_amd.cogmen import COGMENModule
    small = N <= COGMENModule.BN_FUSED_MAX_N
    if compute == "f32":       # unfused exact-fp32 graph kernels: no tile kernels, no projection + graph-build launch
        assert not res["fused_graph"] and res["bn_in_tile"] is None and calls["cogmen_project_graph"] == 0
        assert calls["bn_batch_stats"] == 1 and calls["head_fused_bn"] == 0
        return
    assert res["fused_graph"]
    assert res["bn_in_tile"] == small
    # statistics in the tile kernel, finished by the head (head_fused_bn) | their own launch in front of the head
    assert calls["head_fused_bn"] == (1 if small else 0) and calls["bn_batch_stats"] == (0 if small else 1), calls
    # projection + graph build in one launch: split modes on both sides (eval and train forward), bf16 only up to the switch
    want = 2 if (small or compute != "bf16") else 0
    assert calls["cogmen_project_graph"] == want, calls


BOUNDARY = {8192: [64] * 128, 8193: [64] * 128 + [1]}


@pytest.mark.parametrize("compute", MODES)
@pytest.mark.parametrize("N", sorted(BOUNDARY))
def test_cogmen_bn_fused_boundary(N, compute, monkeypatch):
    """N = BN_FUSED_MAX_N and one node more (a one-utterance dialogue), small D: every mode at its small-shape bars, and the branch
    each case took."""
    case = cogmen_case_lengths(BOUNDARY[N], dims=SMALL_D, seed=31)
    assert int(case["batch"]["label"].shape[0]) == N
    calls = _count_launches(monkeypatch)
    res = _parity(case, compute)
    _report("N=%d" % N, compute, res)
    print("  branch: bn_in_tile=%s fused_graph=%s launches %s" % (res["bn_in_tile"], res["fused_graph"], calls))
    _check_branch(compute, N, res, calls)
    _check(compute, res)


@pytest.mark.parametrize("compute", MODES)
def test_cogmen_benched_b512_shape(compute, monkeypatch):
    """The shape of the B = 512 throughput point: 512 dialogues of 20..110 utterances (config 2's distribution), D = 1380."""
    case = cogmen_case(B=512, min_len=20, max_len=110, dims=SBERT_D, seed=17)
    N = int(case["batch"]["label"].shape[0])
    assert N > 30000
    calls = _count_launches(monkeypatch)
    res = _parity(case, compute)
    _report("B=512 N=%d" % N, compute, res)
    _check_branch(compute, N, res, calls)
    _check(compute, res)


def _params(compute):
    from erc_amd.params import ERCParams
    return ERCParams().from_args(["--dataset=iemocap-cogmen-sbert-6", "--compute=" + compute, "--optim.lr=0.001",
                                  "--optim.weight_decay=1e-8"])


def _fresh_copy(tr, p):
    """a new trainer (no cached workspaces, planner tables or counters) holding ``tr``'s training state"""
    from erc_amd.cogmen import COGMENTrainer
    new = COGMENTrainer(p, DEV)
    new.model.drop_p = 0.0
    a, b = tr.model.flat, new.model.flat
    b.data.copy_(a.data), b.exp_avg.copy_(a.exp_avg), b.exp_avg_sq.copy_(a.exp_avg_sq)
    new.optim.state.copy_(tr.optim.state)
    new.model.gcn.bn.running_mean.copy_(tr.model.gcn.bn.running_mean)
    new.model.gcn.bn.running_var.copy_(tr.model.gcn.bn.running_var)
    new.model.refresh_shadows()
    return new


SWITCH = [("2k", dict(B=32, min_len=20, max_len=110, seed=60)), ("10k", dict(B=160, min_len=20, max_len=110, seed=61)),
          ("2k", None), ("31k", dict(B=512, min_len=20, max_len=110, seed=63)), ("8192", [64] * 128)]


@pytest.mark.parametrize("compute", ["f32x32", "bf16"])
def test_cogmen_trainer_switches_shapes_across_the_boundary(compute):
    """One trainer, dropout off, lr 1e-3: N ~ 2 k -> ~ 10 k -> the same 2 k batch again (its cached workspace) -> ~ 31 k -> 8 192.
    Every step is bit-identical to the same step of a NEW trainer given the same training state (weights, Adam moments and step
    count, BatchNorm running statistics): no state leaks between the cached per-shape workspaces.  f32x32 (the 1e-4 parity path)
    is also held to the oracle + torch.optim.Adam on the same batches: loss within 2e-5 at every step (the bar of
    test_cogmen_train_step_matches_torch_adam).  Its other bar, weights within 2e-4 after the steps, does not carry over to these
    node counts: Adam's first step moves EVERY entry by +-lr whatever the size of its gradient, so an entry whose gradient lies
    within the path's gradient deviation (~1e-5 of the tensor's scale) of zero may move the other way -- measured 1.2e-3 on
    rnn.1.weight after these five steps of lr 1e-3, and units 1.7e-4 from their kink in the second step's forward.  Leaked state
    is what the bit-exact comparison with the new trainer catches."""
    from oracle.cogmen import COGMENOracle, cogmen_train_step
    from erc_amd.cogmen import COGMENModule, COGMENTrainer
    p = _params(compute)
    tr = COGMENTrainer(p, DEV)
    tr.model.drop_p = 0.0
    with_oracle = compute == "f32x32"
    if with_oracle:
        ref = COGMENOracle(p.hidden_all, 100, 17, p.n_speakers, p.n_classes, dead_encoder=False)
        ref.load_state_dict({k: v.cpu() for k, v in tr.model.state_dict().items()})
        for m in ref.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        opt = torch.optim.Adam(ref.parameters(), lr=1e-3, weight_decay=1e-8)
        ref.train()
    batches, sides = [], set()
    for tag, spec in SWITCH:
        if spec is None:
            batch = batches[0]
        elif isinstance(spec, list):
            batch = cogmen_case_lengths(spec, dims=SBERT_D, seed=64)["batch"]
        else:
            batch = cogmen_case(dims=SBERT_D, **spec)["batch"]
        batches.append(batch)
        N = int(batch["label"].shape[0])
        sides.add(N <= COGMENModule.BN_FUSED_MAX_N)
        new = _fresh_copy(tr, p)
        st = tr.train_step(tr.prepare_batch(batch)).cpu()
        st_new = new.train_step(new.prepare_batch(batch)).cpu()
        torch.cuda.synchronize()
        assert torch.equal(st[:3], st_new[:3]), (tag, st[:3], st_new[:3])
        for k in ("data", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(tr.model.flat, k), getattr(new.model.flat, k)), (tag, k)
        assert torch.equal(tr.optim.state, new.optim.state), tag
        assert torch.equal(tr.model.gcn.bn.running_mean, new.model.gcn.bn.running_mean), tag
        assert torch.equal(tr.model.gcn.bn.running_var, new.model.gcn.bn.running_var), tag
        msg = "%s step %s (N=%d): loss %.6f" % (compute, tag, N, float(st[0]))
        if with_oracle:
            loss, _ = cogmen_train_step(ref, opt, batch)
            msg += ", oracle %.6f (|d| %.2e)" % (float(loss), abs(float(st[0]) - float(loss)))
            assert abs(float(st[0]) - float(loss)) < 2e-5, msg
        print(msg)
        del new
    assert sides == {True, False}
    assert int(tr.optim.state[0]) == len(SWITCH)


@pytest.mark.parametrize("compute", ["f32x32", "bf16"])
def test_cogmen_largest_b512_batch(compute, monkeypatch):
    """The largest node count B = 512 / T = 110 admits: 512 dialogues of 110 utterances, N = 56 320, D = 1380.  The step runs it
    (no size limit refuses it) and holds the parity of the mode."""
    case = cogmen_case_lengths([110] * 512, dims=SBERT_D, seed=19)
    N = int(case["batch"]["label"].shape[0])
    assert N == 56320
    calls = _count_launches(monkeypatch)
    res = _parity(case, compute)
    _report("B=512 T=110 N=%d" % N, compute, res)
    _check_branch(compute, N, res, calls)
    _check(compute, res)
