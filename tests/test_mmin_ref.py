"""CPU: the float64 restatements of tests/mmin_ref.py against torch's own float64 autograd (nn.LSTM + max_pool1d, conv2d + relu +
max_pool1d) and, for the whole model, against the reference's golden fixtures; the plugin's parameter defaults and command line,
the module's refusals, the trainer's EMA / plateau / best-checkpoint logic on stub steps, and the synthetic samples."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from erc_amd import capi
from tests import mmin_ref as R
from tests.util_cases import check_grad_digest, fill_params

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_lstm_pool_restatement_matches_float64_autograd(name):
    c = R.scan_case(name)
    f = R.lstm_pool_fwd(c["x"], c["W_ih"], c["W_hh"], c["b_ih"], c["b_hh"])
    bw = R.lstm_pool_bwd(f, c["x"], c["W_hh"], c["dpool"], f["arg"])
    lstm = torch.nn.LSTM(c["D"], 128, batch_first=True).double()
    with torch.no_grad():
        for k, v in (("weight_ih_l0", "W_ih"), ("weight_hh_l0", "W_hh"), ("bias_ih_l0", "b_ih"), ("bias_hh_l0", "b_hh")):
            getattr(lstm, k).copy_(c[v])
    out, _ = lstm(c["x"].double())
    pool, idx = torch.nn.functional.max_pool1d(out.transpose(1, 2), out.shape[1], return_indices=True)
    (pool.squeeze(-1) * c["dpool"].double()).sum().backward()
    assert torch.equal(idx.squeeze(-1), f["arg"])
    assert R.rel(f["hs"], out.detach()) < 1e-14 and R.rel(f["pool"], pool.squeeze(-1).detach()) < 1e-14
    for got, want in ((bw["dW_ih"], lstm.weight_ih_l0.grad), (bw["dW_hh"], lstm.weight_hh_l0.grad), (bw["db"], lstm.bias_ih_l0.grad),
                      (bw["db"], lstm.bias_hh_l0.grad)):
        assert R.rel(got, want) < 1e-13


def test_padding_case_has_maxima_inside_the_padding_and_near_ties():
    """case (a): a share of the maxima lies in steps whose input rows are zero, where the state creeps towards a fixed point"""
    c = R.scan_case("a")
    f = R.lstm_pool_fwd(c["x"], c["W_ih"], c["W_hh"], c["b_ih"], c["b_hh"])
    zf = torch.tensor(R.SCAN_CASES["a"][3])[:, None]
    assert 20 <= int((f["arg"] >= zf).sum()) <= 320
    assert R.arg_condition(f["hs"], f["arg"], 0.0) == 0
    worse = torch.where(f["arg"] > 0, f["arg"] - 1, f["arg"] + 1)
    assert R.arg_condition(f["hs"], worse, 1e-12) > 0


@pytest.mark.parametrize("name", sorted(R.CNN_CASES))
def test_textcnn_restatement_matches_float64_autograd(name):
    c = R.cnn_case(name)
    Ws, bs = [c["W%d" % k] for k in R.KS], [c["b%d" % k] for k in R.KS]
    f = R.textcnn_fwd(c["x"], Ws, bs)
    bw = R.textcnn_bwd(c["x"], f["pooled"], f["arg"], c["dpooled"])
    x, outs, leaves = c["x"].double().unsqueeze(1), [], []
    for k, W, b in zip(R.KS, Ws, bs):
        W, b = W.double().reshape(128, 1, k, -1).requires_grad_(), b.double().requires_grad_()
        a = torch.relu(torch.nn.functional.conv2d(x, W, b).squeeze(3))
        outs.append(torch.nn.functional.max_pool1d(a, a.shape[2]).squeeze(2))
        leaves.append((W, b))
    pooled = torch.cat(outs, 1)
    (pooled * c["dpooled"].double()).sum().backward()
    assert R.rel(f["pooled"], pooled.detach()) < 1e-13
    live = f["pooled"] > 0
    for n, k in enumerate(R.KS):
        if bool(live.any()):
            assert R.rel(bw[k][0], leaves[n][0].grad.reshape(128, k, -1)) < 1e-13 and R.rel(bw[k][1], leaves[n][1].grad) < 1e-13
        else:
            assert bool((bw[k][0] == 0).all()) and bool((bw[k][1] == 0).all())
    # the committed seeds: the float32 twin routes every live channel as float64 does, and no two best windows are close
    f32 = R.textcnn_fwd(c["x"], Ws, bs, dtype=torch.float32)
    assert bool((f32["arg"] == f["arg"])[live].all()) and R.min_live_gap(f["conv"], f["pooled"]) > 1e-5
    if name == "d":
        assert not bool(live.any()) and bool((f["arg"] == 0).all())


@pytest.mark.parametrize("name", ["mmin_base_a", "mmin_base_b2"])
def test_model_restatement_matches_reference_fixture(golden, name):
    fx = golden(name)
    assert [str(k) for k in fx["sd_keys"]] == [k for k, _ in R.SD_SHAPES]
    assert [tuple(int(d) for d in s if d >= 0) for s in fx["sd_shapes"]] == [s for _, s in R.SD_SHAPES]
    assert int(fx["n_params"]) == R.N_PARAMS == sum(int(np.prod(s)) for _, s in R.SD_SHAPES) and [str(s) for s in fx["grad_none"]] == []
    holder = torch.nn.Module()
    holder.p = torch.nn.ParameterDict({k.replace(".", "/"): torch.nn.Parameter(torch.zeros(s)) for k, s in R.SD_SHAPES})
    named = {k.replace("/", "."): p for k, p in holder.p.items()}

    class Named(torch.nn.Module):          # fill_params walks sorted(named_parameters()): the reference's dotted names
        def named_parameters(self, *a, **k):
            return iter(named.items())
    fill_params(Named(), int(fx["param_seed"]))
    P = {k: v.detach() for k, v in named.items()}
    batch = {k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("in_")}
    assert all(torch.equal(batch[k], R.make_batch(name, {"mmin_base_a": 181, "mmin_base_b2": 182}[name])[k]) for k in batch)
    r = R.model_loss_grads(P, batch)
    for k in ("logits", "feat", "audio", "visual", "text"):
        assert float((r[k] - torch.from_numpy(fx[k]).double()).abs().max()) < 1e-4, k      # the project's parity tolerance
    assert abs(float(r["loss"]) - float(fx["loss"])) < 1e-4
    assert check_grad_digest(fx, [(k, g.float()) for k, g in r["grads"].items()], 1e-4) < 1e-4


def test_params_defaults_and_debug():
    from track_mm.mmin_base import MMINBaseParams, ParamsType, main
    assert ParamsType is MMINBaseParams and callable(main)
    p = MMINBaseParams().from_args([])
    assert (p.train.batch_size, p.val.batch_size, p.test.batch_size) == (32, 32, 32)
    assert p.dataset == "iemocap-mmin-4" and p.epoch == 55 and p.ema is True and p.confuse_matrix is True and p.pretrain_path is None
    assert (p.optim.name, p.optim.lr, p.optim.weight_decay) == ("Adam", 0.0002, 0)
    assert p.n_classes == 4 and p.class_names == ["hap", "sad", "neu", "ang"] and tuple(p.mmin_frames) == (50, 400)
    d = MMINBaseParams().from_args(["--debug"])
    assert d.train.batch_size == 2 and d.test.batch_size == 2
    assert tuple(MMINBaseParams().from_args(["--mmin_frames=20,40"]).mmin_frames) == (20, 40)
    from erc_amd import params
    assert params.MMIN_DATASETS == ("iemocap-mmin-4",) and "iemocap-mmin-4" in params.ALL_DATASETS and len(params.DATASETS) == 26


def test_unknown_module_lists_mmin_base():
    res = subprocess.run([sys.executable, os.path.join(REPO, "train_mm.py"), "--module=nope"], capture_output=True, text=True,
                         env=dict(os.environ, PYTHONPATH=REPO), cwd=REPO)
    assert res.returncode == 1 and "'mmin_base'" in res.stdout


def test_refusals():
    from erc_amd.mmin import MMINBaseModule, make_loaders
    from track_mm.mmin_base import MMINBaseParams
    with pytest.raises(capi.ErcGraftError, match="compute"):
        MMINBaseModule(342, 1024, 130, 4, compute="bf16")
    for kw in ("visual_dim", "text_dim", "audio_dim"):
        with pytest.raises(capi.ErcGraftError, match=kw):
            MMINBaseModule(**dict(dict(visual_dim=342, text_dim=1024, audio_dim=130), **{kw: 0}))
    m = MMINBaseModule(342, 1024, 130, 4)
    with pytest.raises(capi.ErcGraftError, match="finalize"):
        m(audio_feature=torch.zeros(1, 5, 130), visual_feature=torch.zeros(1, 5, 342), text_feature=torch.zeros(1, 5, 1024))
    m.flat = object()        # the argument checks run before anything touches the device
    a, v, t = torch.zeros(2, 6, 130), torch.zeros(2, 5, 342), torch.zeros(2, 7, 1024)
    for miss in ("audio_feature", "visual_feature", "text_feature"):
        kw = dict(audio_feature=a, visual_feature=v, text_feature=t)
        kw[miss] = None
        with pytest.raises(capi.ErcGraftError, match=miss + " is missing"):
            m._inputs(kw["audio_feature"], kw["visual_feature"], kw["text_feature"], need_all=True)
    with pytest.raises(capi.ErcGraftError, match="text_feature has 4 tokens"):
        m._inputs(a, v, t[:, :4], need_all=True)
    with pytest.raises(capi.ErcGraftError, match="visual_feature must be fp32"):
        m._inputs(a, v[:, :, :300], t, need_all=True)
    with pytest.raises(SystemExit, match="h5py"):
        make_loaders(MMINBaseParams().from_args(["--synthetic=False"]))
    assert capi.textcnn_min_t() == 5


def test_state_dict_is_the_references():
    from erc_amd.mmin import MMINBaseModule
    m = MMINBaseModule(342, 1024, 130, 4)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == list(R.SD_SHAPES)
    assert sum(p.numel() for p in m.parameters()) == R.N_PARAMS


def test_plateau_matches_torch():
    from erc_amd.mmin import PlateauLR
    g = torch.Generator().manual_seed(3)
    seq = [1.0, 0.9, 0.8] + [0.8 + 0.01 * float(v) for v in torch.rand(30, generator=g)] + [0.5] + [0.6] * 25
    q = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([q], lr=2e-4)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, "min")
    mine = PlateauLR(2e-4)
    for v in seq:
        ref.step(v)
        assert mine.step(v) == opt.param_groups[0]["lr"]
    assert mine.lr < 2e-4 * 0.011


class _StubTrainer:
    """MMINBaseTrainer's epoch-end logic without a device"""

    def __init__(self):
        from erc_amd.mmin import PlateauLR
        self.sched, self.accuracy, self.global_steps = PlateauLR(2e-4), 0.0, 0
        self.optim = type("O", (), {"lr": 2e-4})()


def test_trainer_epoch_end_logic_on_stub_steps():
    from erc_amd.mmin import MMINBaseTrainer
    t = _StubTrainer()
    changed = [MMINBaseTrainer.on_eval_end(t, dict(Lall=1.0)) for _ in range(12)]
    assert changed == [False] * 11 + [True] and abs(t.optim.lr - 2e-5) < 1e-12       # 11 bad epochs after the first: patience 10
    best = [MMINBaseTrainer.on_test_end(t, dict(Acc=a)) for a in (0.25, 0.5, 0.5, 0.4, 0.75)]
    assert best == [True, True, False, False, True] and t.accuracy == 0.75            # strictly better only (mmin_base.py:198)


def test_ema_formula_is_the_references():
    """what erc_ema_step is compared with on the device (mmin_ref.ema_step32) against the reference's tensor expression: the float
    alpha costs at most 2^-25 |p| and one unit in the last place of the result"""
    g = torch.Generator().manual_seed(4)
    p, e = torch.randn(4096, generator=g), torch.randn(4096, generator=g)
    want = 0.999 * e + (1 - 0.999) * p
    got = R.ema_step32(e, p, 0.999)
    assert bool(((got - want).abs() <= 2.0 ** -25 * p.abs() + 2.0 ** -23 * want.abs()).all())


def test_synthetic_samples_shapes_and_determinism():
    from erc_amd.mmin import mmin_collate
    from erc_amd.synthetic import make_mmin_samples
    a = make_mmin_samples(6, "train", seed=1, frames=(5, 9))
    b = make_mmin_samples(6, "train", seed=1, frames=(5, 9))
    v = make_mmin_samples(6, "val", seed=1, frames=(5, 9))
    for s, s2, s3 in zip(a, b, v):
        assert s["visual_feature"].shape == (50, 342) and s["text_feature"].shape == (22, 1024)
        assert s["audio_feature"].shape[1] == 130 and 5 <= s["audio_feature"].shape[0] <= 9 and 0 <= s["label"] < 4
        assert all(np.array_equal(s[k], s2[k]) for k in ("audio_feature", "visual_feature", "text_feature")) and s["label"] == s2["label"]
        assert not np.array_equal(s["visual_feature"], s3["visual_feature"])
    batch = mmin_collate(a[:3])
    Ta = max(s["audio_feature"].shape[0] for s in a[:3])
    assert batch["audio_feature"].shape == (3, Ta, 130) and batch["visual_feature"].shape == (3, 50, 342)
    assert batch["text_feature"].shape == (3, 22, 1024) and batch["label"].dtype == torch.int64 and len(batch["name"]) == 3
    for i, s in enumerate(a[:3]):
        assert bool((batch["audio_feature"][i, s["audio_feature"].shape[0]:] == 0).all())
    assert batch["audio_feature_length"] == [s["audio_feature"].shape[0] for s in a[:3]]
