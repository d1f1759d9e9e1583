"""CPU: the float64 restatements of tests/mmin_miss_ref.py against float64 autograd of an independent form (torch.nn layers
composed as ResidualAE, F.mse_loss), the twins' figures against the FIGURES record, the reference's golden fixtures against the
whole-model restatement, the collate and Missing transform, the state_dict, the plugin's parameters and refusals, the trainer's
host logic (finetune, the re-initialisation rule, the checkpoint envelope) and the module listing."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch import nn

from erc_amd import capi
from tests import mmin_miss_ref as MR
from tests import mmin_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RG = 16       # erc_resae_rows_per_group(): asserted against the library below


class _TorchAE(nn.Module):
    """ResidualAE's forward (mmin_models.py:187-199) from torch.nn layers, float64: the independent form"""

    def __init__(self, P, nb):
        super().__init__()
        self.nb = nb
        self.lin = nn.ModuleList()
        for W, b in P:
            m = nn.Linear(W.shape[1], W.shape[0]).double()
            with torch.no_grad():
                m.weight.copy_(W), m.bias.copy_(b)
            self.lin.append(m)

    def forward(self, x):
        x_in, x_out, latents = x, torch.zeros_like(x), []
        leaky, relu = nn.LeakyReLU(), nn.ReLU()
        for i in range(self.nb):
            e0, e1, e2, d0, d1, d2 = self.lin[6 * i:6 * i + 6]
            x_in = x_in + x_out
            latent = e2(leaky(e1(leaky(e0(x_in)))))
            x_out = d2(relu(d1(relu(d0(latent)))))
            latents.append(latent)
        t0, t2 = self.lin[6 * self.nb:]
        return t2(relu(t0(x_in + x_out))), torch.cat(latents, -1)


@pytest.mark.parametrize("name,B,with_latents", [("a", 1, True), ("b", RG + 1, True), ("c", 5, True), ("c", 5, False), ("e", 4, True)])
def test_autoencoder_restatement_matches_float64_autograd(name, B, with_latents):
    c = MR.ae_case(name, B)
    nb = c["nb"]
    f = MR.resae_fwd(c["P"], c["x"], nb)
    dl = c["d_latents"] if with_latents else None
    bw = MR.resae_bwd(c["P"], f["acts"], MR.masks_of(f["pre"], nb), c["d_recon"], dl, nb)
    net = _TorchAE(c["P"], nb)
    x = c["x"].double().requires_grad_()
    recon, latents = net(x)
    loss = (recon * c["d_recon"].double()).sum()
    if with_latents:
        loss = loss + (latents * c["d_latents"].double()).sum()
    loss.backward()
    assert R.rel(f["recon"], recon.detach()) < 1e-13 and R.rel(f["latents"], latents.detach()) < 1e-13
    assert R.rel(bw["dx"], x.grad) < 1e-12
    for l, m in enumerate(net.lin):
        assert R.rel(bw["dW"][l], m.weight.grad) < 1e-12 and R.rel(bw["db"][l], m.bias.grad) < 1e-12, l
    assert [tuple(a.shape) for a in f["acts"]] == [(B, n_in) for _, n_in in MR.layer_dims(nb)]
    assert [tuple(d.shape) for d in bw["dY"]] == [(B, n_out) for n_out, _ in MR.layer_dims(nb)]


def test_case_e_is_relu_dead_and_leaky_on_both_sides():
    c = MR.ae_case("e", 4)
    f = MR.resae_fwd(c["P"], c["x"], c["nb"])
    bw = MR.resae_bwd(c["P"], f["acts"], MR.masks_of(f["pre"], c["nb"]), c["d_recon"], c["d_latents"], c["nb"])
    for i in range(c["nb"]):
        for l in (6 * i + 3, 6 * i + 4):
            assert bool((f["pre"][l] < -5).all()) and bool((bw["dY"][l] == 0).all()) and bool((bw["dW"][l] == 0).all())
        assert bool((bw["dW"][6 * i + 5] == 0).all()) and bool((f["acts"][6 * i + 5] == 0).all())
        for l in (6 * i, 6 * i + 1):
            pos = float((f["pre"][l] > 0).double().mean())
            assert 0.05 < pos < 0.95, (l, pos)


def test_mse_pair_matches_float64_autograd():
    g = torch.Generator().manual_seed(5)
    for B in (1, 33):
        a, b = torch.randn(B, 384, generator=g).double().requires_grad_(), torch.randn(B, 384, generator=g).double().requires_grad_()
        (3.0 * nn.functional.mse_loss(a, b)).backward()
        loss, d = MR.mse_pair(a.detach(), b.detach(), 3.0)
        assert abs(float(loss) - float(nn.functional.mse_loss(a, b).detach())) < 1e-14
        assert R.rel(d, a.grad) < 1e-14 and R.rel(-d, b.grad) < 1e-14
        loss32, d32 = MR.mse_pair(a.detach(), b.detach(), 3.0, dtype=torch.float32)
        assert abs(float(loss32) - float(loss)) < 1e-6 * float(loss) and R.rel(d32, d) < 2e-7


# ------------------------------------------------------------------------------------------------------------ the figures
_AE_SIZES = {"a": (1, ), "b": (RG - 1, RG, RG + 1), "c": (5, ), "d": (33, ), "e": (4, )}


def ae_figures(name, B, job=0):
    """the twin's deviation from float64 per quantity (per-layer quantities by their worst layer)"""
    c = MR.ae_case(name, B, job)
    f64, b64, f32, b32 = MR.ae_reference(c, with_latents=(job == 0))
    worst = lambda got, want: max(R.rel(g, w) for g, w in zip(got, want))
    return {"recon": R.rel(f32["recon"], f64["recon"]), "latents": R.rel(f32["latents"], f64["latents"]), "acts": worst(f32["acts"], f64["acts"]),
            "dx": R.rel(b32["dx"], b64["dx"]), "dY": worst(b32["dY"], b64["dY"]), "dW": worst(b32["dW"], b64["dW"]),
            "db": worst(b32["db"], b64["db"])}


@pytest.mark.parametrize("name", sorted(MR.AE_CASES))
def test_twin_figures_are_the_recorded_ones(name):
    """FIGURES' first two columns are this machine's: the twin is built from elementwise IEEE arithmetic in a fixed order"""
    assert capi.resae_rows_per_group() == RG
    for B in _AE_SIZES[name]:
        for job in range(MR.AE_CASES[name][2]):
            figs = ae_figures(name, B, job)
            print(name, B, job, {k: "%.2e" % v for k, v in figs.items()})
            for k, v in figs.items():
                twin, bnd, _ = MR.FIGURES[("resae", "%s/B%d/job%d" % (name, B, job), k)]
                assert abs(v - twin) <= 0.006 * max(twin, 1e-9), (k, v, twin)       # recorded with three significant digits
                assert bnd == R.round_up_1(MR.MARGIN * max(v, MR.FLOOR)), (k, bnd)
                assert v < 2e-6       # a float32 chain of 32 layers: orientation, torch's own fp32 forward deviates 4.3e-7


# ------------------------------------------------------------------------------------------------------------ whole model
def _fixture_inputs(fx):
    full = {k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("in_")}
    return full, MR.apply_missing(full, torch.from_numpy(fx["missing_type"]))


@pytest.mark.parametrize("name", sorted(MR.MODEL_CASES))
def test_model_restatement_matches_reference_fixture(golden, name):
    fx = golden(name)
    shapes = MR.sd_shapes()
    assert [str(k) for k in fx["sd_keys"]] == [k for k, _ in shapes] and len(shapes) == 150
    assert [tuple(int(d) for d in s if d >= 0) for s in fx["sd_shapes"]] == [s for _, s in shapes]
    assert int(fx["n_params"]) == MR.N_PARAMS == sum(int(np.prod(s)) for _, s in shapes) and [str(s) for s in fx["grad_none"]] == []
    full, batch = _fixture_inputs(fx)
    want_full, want_mt = MR.make_batch(name)
    assert all(torch.equal(full[k], want_full[k]) for k in full) and torch.equal(batch["missing_type"], want_mt)
    if name == "mmin_miss_a":
        assert sorted(map(tuple, batch["missing_type"].tolist())) == sorted(MR.MISSING_TYPES)
    P = MR.named_filled(shapes, int(fx["param_seed"]))
    Ppre = MR.named_filled(R.SD_SHAPES, int(fx["pretrained_seed"]))
    with R.one_thread():
        rev = MR.encode(Ppre, batch["audio_feature_reverse"], batch["visual_feature_reverse"], batch["text_feature_reverse"])["features"]
        r = MR.model_loss_grads(P, batch, rev)
    assert float((rev - torch.from_numpy(fx["reverse_features"]).double()).abs().max()) < 1e-4
    for k in ("logits", "fusion", "fusion_cycle", "features"):
        assert float((r[k] - torch.from_numpy(fx[k]).double()).abs().max()) < 1e-4, k      # the project's parity tolerance
    for k in ("Lce", "Lmse", "Lcycle", "Lall"):
        assert abs(float(r[k]) - float(fx[k])) < 1e-4, k
    worst = 0.0
    for k, g in r["grads"].items():
        key = k.replace(".", "__")
        want = torch.from_numpy(fx["gd__" + key]).double()
        got = MR.digest(g)
        scale = max(float(want.abs().max()), 1e-12)
        worst = max(worst, float((got - want).abs().max()) / scale, abs(float(g.norm()) - float(fx["gnorm__" + key])) / (float(fx["gnorm__" + key]) + 1e-9))
    print("%s: worst gradient digest deviation %.2e" % (name, worst))
    assert worst < 1e-4 and len(r["grads"]) == 150


def test_state_dict_is_the_references(golden):
    from erc_amd.mmin_miss import MMINMissModule, _ResidualAE
    m = MMINMissModule(342, 1024, 130, 4)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == list(MR.sd_shapes())
    fx = golden("mmin_miss_a")
    assert list(m.state_dict()) == [str(k) for k in fx["sd_keys"]]
    assert sum(p.numel() for p in m.parameters()) == MR.N_PARAMS == int(fx["n_params"])
    assert sum(p.numel() for p in m.netAE.parameters()) == 1694400 and len(list(m.netAE.parameters())) == 64
    # the chain order of the kernels is the state_dict's order with the transition moved behind the blocks
    assert capi.resae_layer_names(5) == MR.layer_names(5) and capi.resae_layer_dims(5) == MR.layer_dims(5)
    assert [tuple(m.state_dict()["netAE.%s.weight" % n].shape) for n in MR.layer_names(5)] == MR.layer_dims(5)
    for bad in (dict(layers=[256, 128, 32]), dict(input_dim=256), dict(use_bn=True), dict(dropout=0.5), dict(n_blocks=6), dict(n_blocks=0)):
        with pytest.raises(capi.ErcGraftError, match="ResidualAE"):
            _ResidualAE(**dict(dict(layers=[256, 128, 64], n_blocks=5, input_dim=384), **bad))


# ------------------------------------------------------------------------------------------------------- collate, Missing
def test_missing_and_collate():
    from erc_amd.mmin import mmin_collate
    from erc_amd.mmin_miss import MISSING_TYPES, Missing, MMINMissCollate
    from erc_amd.synthetic import make_mmin_samples
    assert MISSING_TYPES == MR.MISSING_TYPES == ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1))
    samples = make_mmin_samples(12, "train", seed=1, frames=(5, 9))
    tf = Missing()
    random.seed(3)
    drawn = [tf(dict(s))["missing_type"] for s in samples]
    random.seed(3)
    assert drawn == [random.choice([list(t) for t in MISSING_TYPES]) for _ in samples]       # one random.choice per sample read
    assert "missing_type" not in samples[0]                                                       # the stored sample is not touched
    typed = [dict(s, missing_type=list(MISSING_TYPES[i % 6])) for i, s in enumerate(samples[:6])]
    plain = mmin_collate(samples[:6])
    out = MMINMissCollate(has_miss=True)(typed)
    assert torch.equal(out["missing_type"], torch.tensor(MISSING_TYPES)) and out["missing_type"].dtype == torch.int64
    for col, key in enumerate(("visual_feature", "text_feature", "audio_feature")):      # mask column order: visual, text, audio
        for i in range(6):
            keep = MISSING_TYPES[i][col]
            assert torch.equal(out[key][i], plain[key][i] * keep)
            assert torch.equal(out[key + "_reverse"][i], plain[key][i] * (1 - keep))
        assert torch.equal(out[key] + out[key + "_reverse"], plain[key])
    assert torch.equal(out["label"], plain["label"]) and out["name"] == plain["name"]
    assert out["audio_feature_length"] == plain["audio_feature_length"]
    # validation / test: full modality, nothing added
    ev = MMINMissCollate(has_miss=False)(samples[:6])
    assert sorted(ev) == sorted(plain) and all(torch.equal(ev[k], plain[k]) for k in plain if torch.is_tensor(plain[k]))
    want = MR.apply_missing(plain, MISSING_TYPES)
    assert all(torch.equal(out[k], want[k]) for k in want if torch.is_tensor(want[k]))


def test_loaders_mask_training_batches_only():
    from track_mm.mmin_miss import MMINMissParams
    from erc_amd.mmin_miss import MMINMissTrainer
    from erc_amd.synthetic import make_mmin_samples
    p = MMINMissParams().from_args(["--n_train=6", "--n_val=3", "--n_test=3", "--train.batch_size=3", "--mmin_frames=(5,9)"])
    train, val, test = MMINMissTrainer.make_loaders(p)
    random.seed(1)
    first = [b["missing_type"].clone() for b in train]
    second = [b["missing_type"].clone() for b in train]
    assert len(first) == 2 and all(tuple(t.shape) == (3, 3) for t in first)
    assert not all(torch.equal(a, b) for a, b in zip(first, second))             # drawn again every epoch
    for loader in (val, test):
        for b in loader:
            assert "missing_type" not in b and "audio_feature_reverse" not in b
    names = sorted(n for b in train for n in b["name"])
    assert names == sorted(s["name"] for s in make_mmin_samples(6, "train", seed=p.seed, frames=(5, 9)))      # make_mmin_samples' utterances
    with pytest.raises(SystemExit, match="mmin_miss"):
        MMINMissTrainer.make_loaders(MMINMissParams().from_args(["--synthetic=False"]))


# ------------------------------------------------------------------------------------------------------- params, refusals
def test_params_defaults_and_debug():
    from track_mm.mmin_miss import MMINMissParams, ParamsType, main
    from erc_amd.mmin_miss import MMINMissTrainer
    assert ParamsType is MMINMissParams and main.args == (MMINMissTrainer, MMINMissParams)
    p = MMINMissParams().from_args([])
    assert (p.train.batch_size, p.val.batch_size, p.test.batch_size) == (32, 32, 32)
    assert p.dataset == "iemocap-mmin-4" and p.epoch == 55 and p.ema is True and p.confuse_matrix is True
    assert (p.optim.name, p.optim.lr, p.optim.weight_decay) == ("Adam", 0.0002, 0)
    assert p.pretrain_path is None and p.finetune is False and p.pretrain_reinit is True
    assert p.n_classes == 4 and p.class_names == ["hap", "sad", "neu", "ang"] and tuple(p.mmin_frames) == (50, 400)
    d = MMINMissParams().from_args(["--debug"])
    assert d.train.batch_size == 2 and d.test.batch_size == 2
    q = MMINMissParams().from_args(["--finetune", "--pretrain_reinit=False", "--pretrain_path=x.ckpt"])
    assert q.finetune is True and q.pretrain_reinit is False and q.pretrain_path == "x.ckpt"


def test_refusals_by_name():
    from track_mm.mmin_miss import MMINMissParams
    from erc_amd.mmin_miss import MMINMissModule, MMINMissTrainer
    with pytest.raises(capi.ErcGraftError, match="mmin_miss runs in fp32"):
        MMINMissModule(342, 1024, 130, 4, compute="bf16")
    with pytest.raises(capi.ErcGraftError, match="mmin_miss runs in fp32"):
        MMINMissTrainer(MMINMissParams().from_args(["--compute=bf16"]), "cpu")
    for flag, what in (("--capacity_buckets=True", "capacity buckets"), ("--resident", "--resident"), ("--resident_eval", "--resident_eval")):
        with pytest.raises(capi.ErcGraftError, match="mmin_miss: " + what):
            MMINMissTrainer(MMINMissParams().from_args([flag]), "cpu")
    m = MMINMissModule(342, 1024, 130, 4)
    with pytest.raises(capi.ErcGraftError, match="MMINMissModule.finalize"):
        m(audio_feature=torch.zeros(1, 5, 130), visual_feature=torch.zeros(1, 5, 342), text_feature=torch.zeros(1, 5, 1024))
    m.flat = object()
    with pytest.raises(capi.ErcGraftError, match="mmin_miss: visual_feature is missing"):
        m._inputs(torch.zeros(2, 6, 130), None, torch.zeros(2, 7, 1024), need_all=True)


# ------------------------------------------------------------------------------------------------------ trainer host logic
def _trainer(*argv):
    from track_mm.mmin_miss import MMINMissParams
    from erc_amd.mmin_miss import MMINMissTrainer
    return MMINMissTrainer(MMINMissParams().from_args(list(argv)), "cpu")


def _base_checkpoint(tmp_path):
    """a mmin_base checkpoint in the reference's envelope, every parameter non-zero"""
    from erc_amd.mmin import MMINBaseModule
    from tests.util_cases import fill_params
    m = MMINBaseModule(342, 1024, 130, 4)
    fill_params(m, 17)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    path = str(tmp_path / "base.ckpt")
    torch.save({"models": {"model": sd}, "optims": {}, "others": {}, "thtensor": {}, "nptensor": {}}, path)
    return path, sd


def test_finetune_is_a_no_op_and_the_optimizer_covers_the_model_alone():
    a, b = _trainer("--seed=3"), _trainer("--seed=3", "--finetune")
    assert b.finetune is True and a.finetune is False
    assert b.optim.flat is b.model.flat and b.optim.flat is not b.pretrained_model.flat
    assert b.model.flat.numel >= MR.N_PARAMS > b.pretrained_model.flat.live_numel
    assert torch.equal(a.model.flat.data, b.model.flat.data) and torch.equal(a.pretrained_model.flat.data, b.pretrained_model.flat.data)
    assert a.pretrained_model.flat.data.data_ptr() != a.model.flat.data.data_ptr()


def test_reinit_rule_after_the_checkpoint_was_loaded(tmp_path):
    """efficiency_init on both models after the load (mmin_miss.py:157-158): Conv weights re-drawn, Conv and Linear biases zero,
    LSTMs untouched; --pretrain_reinit=False keeps the loaded weights of the pretrained model"""
    path, sd = _base_checkpoint(tmp_path)
    for reinit in (True, False):
        tr = _trainer("--pretrain_path=" + path, "--pretrain_reinit=%s" % reinit)
        assert tr._model_initialised is False
        tr.load_pretrained(path)
        got = tr.pretrained_model.state_dict()
        for k, v in sd.items():
            same = torch.equal(got[k], v)
            if not reinit or ".rnn." in k or (k.endswith(".weight") and "conv" not in k):
                assert same, k
            elif k.endswith(".bias"):
                assert bool((got[k] == 0).all()), k
            else:
                assert "conv" in k and not same and abs(float(got[k].std()) - (2.0 / (v.shape[2] * v.shape[3])) ** 0.5) < 0.1 * float(got[k].std())
        # the model itself is always initialised: its Linear and Conv biases are zero, and the EMA copy is made afterwards
        own = tr.model.state_dict()
        assert all(bool((v == 0).all()) for k, v in own.items() if k.endswith(".bias") and ".rnn." not in k)
        assert any(bool((v != 0).any()) for k, v in own.items() if ".rnn.bias" in k)
        assert torch.equal(tr.ema, tr.model.flat.data)
    with pytest.raises(KeyError, match="not a mmin_base checkpoint"):
        bad = str(tmp_path / "bad.ckpt")
        torch.save({"models": {"model": {"x": torch.zeros(1)}}}, bad)
        tr.load_pretrained(bad)


def test_checkpoint_envelope_carries_the_three_models(tmp_path):
    from erc_amd import mmin
    tr = _trainer()
    path = mmin.save(tr, str(tmp_path / "miss.ckpt"))
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ckpt["models"]) == {"model", "pretrained_model", "ema_model"} and "optim" in ckpt["optims"]
    assert list(ckpt["models"]["model"]) == list(ckpt["models"]["ema_model"]) == [k for k, _ in MR.sd_shapes()]
    assert list(ckpt["models"]["pretrained_model"]) == [k for k, _ in R.SD_SHAPES]
    assert all(torch.equal(v, tr.pretrained_model.state_dict()[k]) for k, v in ckpt["models"]["pretrained_model"].items())
    assert set(torch.load(mmin.save(_trainer("--ema=False"), path), weights_only=True)["models"]) == {"model", "pretrained_model"}


def test_unknown_module_lists_mmin_miss():
    res = subprocess.run([sys.executable, os.path.join(REPO, "train_mm.py"), "--module=nope"], capture_output=True, text=True,
                         env=dict(os.environ, PYTHONPATH=REPO), cwd=REPO)
    assert res.returncode == 1 and "'mmin_miss'" in res.stdout and "'mmin_base'" in res.stdout and "mmin_miss2" not in res.stdout
