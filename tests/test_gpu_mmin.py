"""GPU: MMIN's full-modality base model (--module=mmin_base) on libercgraft -- the hidden-128 LSTM + max-pool scans and the text
CNN kernels one by one against the float64 restatements of tests/mmin_ref.py (bounds from the float32 twins, there), the
whole module against the reference's own MMINBaseModule (golden vectors) and the restatement, an Adam + EMA step, dropout with
the applied masks, checkpoints and the command line.  Every test prints its measured figures before it asserts."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from erc_amd import capi
from tests import mmin_ref as R
from tests.util_cases import check_grad_digest, fill_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, G4, EMB = 128, 512, 384
GUARD = 3              # rows behind every buffer a kernel writes: nothing may touch them
SENT = -77.25          # what the write sets are pre-filled with


@pytest.fixture(scope="module", autouse=True)
def _lib():
    capi.lib()


def _buf(rows, cols, dtype=torch.float32):
    return torch.full((rows + GUARD, cols), SENT, dtype=dtype, device=DEV)


def _intact(t):
    """the guard rows (or the whole of a buffer nothing may write) still hold the fill value"""
    return bool((t == (SENT if t.is_floating_point() else int(SENT))).all())


def _f64(t):
    return t.detach().cpu().double()


def _report(tag, figs):
    print("%s: %s" % (tag, "  ".join("%s %.2e/%.0e" % (k, got, bnd) for k, (got, bnd) in figs.items())))


# ------------------------------------------------------------------------------------------------------------------ scans
_SCAN_REF = {}


def _scan_ref(name):
    if name not in _SCAN_REF:
        c = R.scan_case(name)
        _SCAN_REF[name] = (c, ) + R.scan_reference(c)
    return _SCAN_REF[name]


@pytest.mark.parametrize("name", sorted(R.SCAN_CASES))
def test_scan(name):
    """erc_lstm128_pool_fwd / _bwd at the case's input width: pool, saved state, the arg condition, dGX and the four weight
    gradients through the caller's GEMMs on the kernel's own routing, a second launch bit-equal, guard rows intact"""
    c, f64, f32, b32 = _scan_ref(name)
    B, T, D = c["B"], c["T"], c["D"]
    rows = B * T
    x, W_ih, W_hh, b_ih, b_hh = (c[k].to(DEV).contiguous() for k in ("x", "W_ih", "W_hh", "b_ih", "b_hh"))
    GX, gates, dGX = _buf(rows, G4), _buf(rows, G4), _buf(rows, G4)
    Cst, Hprev = _buf(rows, H), _buf(rows, H)
    pool, dpool = _buf(B, EMB), _buf(B, EMB)              # the encoder's column range [128, 256) of a 384-wide buffer
    arg = _buf(B, H, torch.int32)
    dpool[:B, H:2 * H] = c["dpool"].to(DEV)
    capi.gemm_f32(x, D, 0, None, W_ih, D, 0, None, GX, G4, rows, G4, D, bias=b_ih)
    job = dict(GX=GX, W_hh=W_hh, b_hh=b_hh, pool=pool[:, H:], arg=arg, gates=gates, Cst=Cst, Hprev=Hprev, dpool=dpool[:, H:], dGX=dGX,
               B=B, T=T, ldp=EMB, lddp=EMB)
    outs = (pool, arg, gates, Cst, Hprev, dGX)
    capi.lstm128_pool_fwd([job])
    capi.lstm128_pool_bwd([job])
    first = [t.clone() for t in outs]
    capi.lstm128_pool_fwd([job])
    capi.lstm128_pool_bwd([job])
    torch.cuda.synchronize()
    for a, b in zip(first, outs):
        assert torch.equal(a, b), "a second launch into the same buffers differs"
    # write sets: the guard rows, and the columns of pool outside the encoder's range
    for t in outs:
        assert _intact(t[-GUARD:])
    assert bool((pool[:B, :H] == SENT).all()) and bool((pool[:B, 2 * H:] == SENT).all())
    k_arg = arg[:B].cpu()
    assert int(k_arg.min()) >= 0 and int(k_arg.max()) < T
    figs = {}
    got = dict(pool=pool[:B, H:2 * H], gates=gates[:rows], Cst=Cst[:rows], Hprev=Hprev[:rows])
    for k, v in got.items():
        want = f64[k].reshape(v.shape)
        figs[k] = (R.rel(_f64(v), want), R.twin_bound(f32[k].reshape(v.shape), want))
    # arg: the routed step's float64 value is within the pool's bound of the float64 maximum -- every (b, u), no exceptions
    tol = figs["pool"][1] * float(f64["pool"].abs().max())
    bad = R.arg_condition(f64["hs"], k_arg, tol)
    n_diff = int((k_arg.long() != f64["arg"]).sum())
    # backward: float64 on the kernel's own routing; the bound from the twin's backward on float64's routing
    with R.one_thread():
        b64 = R.lstm_pool_bwd(f64, c["x"], c["W_hh"], c["dpool"], k_arg.long())
        t64 = b64 if n_diff == 0 else R.lstm_pool_bwd(f64, c["x"], c["W_hh"], c["dpool"], f64["arg"])
    dW_ih, dW_hh = _buf(G4, D), _buf(G4, H)
    db_ih, db_hh = _buf(1, G4), _buf(1, G4)
    capi.gemm_f32(dGX, G4, 1, None, x, D, 1, None, dW_ih, D, G4, D, rows, ones_col=1, bias_out=db_ih)
    capi.gemm_f32(dGX, G4, 1, None, Hprev, H, 1, None, dW_hh, H, G4, H, rows, ones_col=1, bias_out=db_hh)
    torch.cuda.synchronize()
    for k, v, w in (("dGX", dGX[:rows], "dGX"), ("dW_ih", dW_ih[:G4], "dW_ih"), ("dW_hh", dW_hh[:G4], "dW_hh"), ("db_ih", db_ih[0], "db"),
                    ("db_hh", db_hh[0], "db")):
        figs[k] = (R.rel(_f64(v), b64[w].reshape(v.shape)), R.twin_bound(b32[w], t64[w]))
    _report("scan %s (B=%d T=%d D=%d; %d routed steps differ from float64's, %d outside the bound)" % (name, B, T, D, n_diff, bad), figs)
    assert bad == 0
    for k, (g, bnd) in figs.items():
        assert g <= bnd, (k, g, bnd)


def test_scan_two_jobs_equal_two_launches():
    """audio and visual in one launch (the step's form) give the bits of one launch each"""
    res = {}
    for form in ("one", "two"):
        jobs, outs = [], []
        for name in ("a", "c"):
            c = _scan_ref(name)[0]
            B, T = c["B"], c["T"]
            GX = (torch.randn(B * T, G4, generator=torch.Generator().manual_seed(T)) * 0.5).to(DEV)
            bufs = dict(pool=_buf(B, H), arg=_buf(B, H, torch.int32), gates=_buf(B * T, G4), Cst=_buf(B * T, H), Hprev=_buf(B * T, H),
                        dGX=_buf(B * T, G4))
            jobs.append(dict(GX=GX, W_hh=c["W_hh"].to(DEV), b_hh=c["b_hh"].to(DEV), dpool=c["dpool"].to(DEV), B=B, T=T, ldp=H, lddp=H, **bufs))
            outs += list(bufs.values())
        for group in ([jobs] if form == "one" else [[j] for j in jobs]):
            capi.lstm128_pool_fwd(group)
            capi.lstm128_pool_bwd(group)
        torch.cuda.synchronize()
        res[form] = outs
    for a, b in zip(res["one"], res["two"]):
        assert torch.equal(a, b)


def test_scan_refuses_bad_arguments_by_status():
    c = _scan_ref("b")[0]
    z = torch.zeros(8, G4, device=DEV)
    zi = torch.zeros(8, H, dtype=torch.int32, device=DEV)
    job = dict(GX=z, W_hh=c["W_hh"].to(DEV), b_hh=c["b_hh"].to(DEV), pool=z, arg=zi, gates=z, Cst=z, Hprev=z, dpool=z, dGX=z, B=1, T=1,
               ldp=H, lddp=H)
    for bad in (dict(T=0), dict(B=0), dict(ldp=H - 1), dict(GX=None)):
        with pytest.raises(capi.ErcGraftError, match="lstm128_pool_fwd"):
            capi.lstm128_pool_fwd([dict(job, **bad)])
    with pytest.raises(capi.ErcGraftError, match="n_jobs"):
        capi.lstm128_pool_fwd([job] * 3)
    with pytest.raises(capi.ErcGraftError, match="lstm128_pool_bwd"):
        capi.lstm128_pool_bwd([dict(job, lddp=H - 1)])
    assert capi.lstm128_hidden() == H and capi.lstm128_max_jobs() == 2


# --------------------------------------------------------------------------------------------------------------- text CNN
_CNN_REF = {}


def _cnn_ref(name):
    if name not in _CNN_REF:
        c = R.cnn_case(name)
        _CNN_REF[name] = (c, ) + R.cnn_reference(c)
    return _CNN_REF[name]


def _cnn_run(c, T=None):
    B, T, D = c["B"], c["T"] if T is None else T, c["D"]
    x = c["x"].to(DEV).contiguous()
    Ws, bs = [c["W%d" % k].to(DEV).contiguous() for k in R.KS], [c["b%d" % k].to(DEV) for k in R.KS]
    ldp = EMB + 16
    bufs = dict(conv=_buf(capi.textcnn_conv_floats(B, T) // EMB, EMB), pooled=_buf(B, ldp), arg=_buf(B, EMB, torch.int32), dpooled=_buf(B, ldp),
                dW=[_buf(H * k, D) for k in R.KS], db=[_buf(1, H) for _ in R.KS])
    bufs["dpooled"][:B, :EMB] = c["dpooled"].to(DEV)
    fwd = lambda: capi.textcnn_pool_fwd(x, B, T, D, Ws, bs, bufs["conv"], bufs["pooled"], ldp, bufs["arg"])
    bwd = lambda: capi.textcnn_pool_bwd(x, B, T, D, bufs["pooled"], ldp, bufs["arg"], bufs["dpooled"], ldp, bufs["dW"], bufs["db"])
    return bufs, fwd, bwd


@pytest.mark.parametrize("name", sorted(R.CNN_CASES))
def test_textcnn(name):
    """erc_textcnn_pool_fwd / _bwd: pooled, arg (equal to float64's on every live channel, 0 on a dead one), dW_k and db_k on the
    kernel's routing, two launches bit-equal, guard rows and pad columns intact"""
    c, f64, f32, b32 = _cnn_ref(name)
    B = c["B"]
    bufs, fwd, bwd = _cnn_run(c)
    outs = [bufs["pooled"], bufs["arg"]] + bufs["dW"] + bufs["db"]
    fwd(), bwd()
    first = [t.clone() for t in outs]
    fwd(), bwd()
    torch.cuda.synchronize()
    for a, b in zip(first, outs):
        assert torch.equal(a, b), "a second launch into the same buffers differs"
    for t in outs + [bufs["conv"]]:
        assert _intact(t[-GUARD:])
    assert bool((bufs["pooled"][:B, EMB:] == SENT).all())
    pooled, k_arg = _f64(bufs["pooled"][:B, :EMB]), bufs["arg"][:B].cpu().long()
    live = f64["pooled"] > 0
    # the committed seeds: the twin agrees with float64 on every live channel, and no two best windows are closer than 1e-5
    assert bool((f32["arg"] == f64["arg"])[live].all()) and R.min_live_gap(f64["conv"], f64["pooled"]) > 1e-5
    assert bool((k_arg == f64["arg"])[live].all()), "routing differs from float64's on a live channel"
    assert bool((k_arg[~live] == 0).all()) and bool((pooled[~live] == 0).all())
    figs = dict(pooled=(R.rel(pooled, f64["pooled"]), R.twin_bound(f32["pooled"], f64["pooled"])))
    with R.one_thread():
        b64 = R.textcnn_bwd(c["x"], f64["pooled"], k_arg, c["dpooled"])
    for n, k in enumerate(R.KS):
        dW, db = _f64(bufs["dW"][n][:H * k]).reshape(H, k, -1), _f64(bufs["db"][n][0])
        figs["dW%d" % k] = (R.rel(dW, b64[k][0]), R.twin_bound(b32[k][0], b64[k][0]))
        figs["db%d" % k] = (R.rel(db, b64[k][1]), R.twin_bound(b32[k][1], b64[k][1]))
        if not bool(live.any()):      # every channel ReLU-dead: exactly zero
            assert bool((dW == 0).all()) and bool((db == 0).all())
    _report("textcnn %s (B=%d T=%d, %d live of %d)" % (name, B, c["T"], int(live.sum()), live.numel()), figs)
    if not bool(live.any()):
        assert bool((pooled == 0).all())
    for k, (g, bnd) in figs.items():
        assert g <= bnd, (k, g, bnd)


def test_textcnn_refuses_t4_by_status_without_a_launch():
    assert capi.textcnn_min_t() == 5 and capi.textcnn_channels() == H
    c = _cnn_ref("b")[0]
    bufs, fwd, bwd = _cnn_run(c, T=4)
    with pytest.raises(capi.ErcGraftError, match="textcnn_pool_fwd: T=4"):
        fwd()
    with pytest.raises(capi.ErcGraftError, match="textcnn_pool_bwd: T=4"):
        bwd()
    torch.cuda.synchronize()
    for t in [bufs["conv"], bufs["pooled"], bufs["arg"]] + bufs["dW"] + bufs["db"]:
        assert _intact(t), "a refused call wrote"


# ----------------------------------------------------------------------------------------------------------------- module
FIXTURES = ("mmin_base_a", "mmin_base_b2")


def _gpu(batch):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _module(seed):
    from erc_amd.mmin import MMINBaseModule
    m = MMINBaseModule(visual_dim=R.VISUAL_D, text_dim=R.TEXT_D, audio_dim=R.AUDIO_D, n_classes=4)
    fill_params(m, seed)
    P = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.finalize(DEV), P


def _fixture_batch(fx):
    return {k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("in_")}


def _kernel_args(m):
    ws = m._last_ws
    return dict(audio=ws["A"]["arg"].cpu().long(), visual=ws["V"]["arg"].cpu().long(), text=ws["L"]["arg"].cpu().long())


def _err(a, b):
    return float((a.detach().cpu().double() - b.double()).abs().max())


@pytest.mark.parametrize("name", FIXTURES)
def test_module_matches_reference_fixture_and_restatement(golden, name):
    """eval-mode forward and loss_and_grads against the reference's own model (logits, feat, the three encoder outputs, loss,
    every gradient digest, state_dict keys and shapes) and against the float64 restatement on the kernels' own routing"""
    fx = golden(name)
    m, P = _module(int(fx["param_seed"]))
    assert list(m.state_dict()) == [str(k) for k in fx["sd_keys"]] == [k for k, _ in R.SD_SHAPES]
    assert [list(v.shape) for v in m.state_dict().values()] == [[int(d) for d in s if d >= 0] for s in fx["sd_shapes"]]
    assert sum(p.numel() for p in m.parameters()) == int(fx["n_params"]) == R.N_PARAMS
    batch = _fixture_batch(fx)
    dev = _gpu(batch)
    m.eval()
    enc = [t.clone() for t in m.encode(dev["audio_feature"], dev["visual_feature"], dev["text_feature"])]
    logits, feat = m(**dev)
    figs = {k: _err(v, torch.from_numpy(fx[k])) for k, v in (("logits", logits), ("feat", feat), ("audio", enc[0]), ("visual", enc[1]),
                                                             ("text", enc[2]))}
    stats = m.loss_and_grads(dev)
    figs["loss"] = abs(float(stats[0]) - float(fx["loss"]))
    grad_fix = check_grad_digest(fx, [(k, m.flat.g(k)) for k in m.flat.params], 1e-3)
    # the restatement in float64, its backward on the routing the kernels used
    r = R.model_loss_grads(P, batch, args=_kernel_args(m))
    figs64 = {k: _err(v, r[k]) for k, v in (("logits", logits), ("feat", feat), ("audio", enc[0]), ("visual", enc[1]), ("text", enc[2]))}
    grad64 = max(R.rel(_f64(m.flat.g(k)), g.reshape(m.flat.shapes[k])) for k, g in r["grads"].items())
    print("%s: vs reference fp32 %s grads %.2e | vs float64 %s loss %.2e grads %.2e"
          % (name, {k: "%.1e" % v for k, v in figs.items()}, grad_fix, {k: "%.1e" % v for k, v in figs64.items()},
             abs(float(stats[0]) - float(r["loss"])), grad64))
    assert all(v < 1e-4 for v in figs.values()), figs
    assert all(v < 1e-4 for v in figs64.values()), figs64
    assert grad_fix < 1e-3 and grad64 < 1e-3
    assert sorted(m.flat.params) == sorted(k for k, _ in m.named_parameters()) and len(m.flat.params) == 22
    assert [str(s) for s in fx["grad_none"]] == []


def test_adam_and_ema_step_against_torch(golden):
    """one Adam + EMA step from the restatement's gradients: torch.optim.Adam on fp32 copies, ema = 0.999 ema + 0.001 p.  At step 1
    the update is lr g / (|g| + eps), whose slope in g is at most 1 / (|g| + eps): an element's tolerance is lr min(2, dg /
    (|g| + eps)) with dg = 1e-3 max|g| of its tensor (the gradient tolerance of the module tests), plus roundings of p"""
    from erc_amd.engine import FusedAdam
    fx = golden("mmin_base_a")
    m, P = _module(int(fx["param_seed"]))
    batch = _fixture_batch(fx)
    m.eval()
    lr, eps = 2e-4, 1e-8
    optim = FusedAdam(m.flat, lr=lr)
    ema = m.flat.data.clone()
    m.loss_and_grads(_gpu(batch))
    r = R.model_loss_grads(P, batch, args=_kernel_args(m))
    optim.step()
    capi.ema_step(ema, m.flat.data, m.flat.numel, 0.999)
    worst = 0.0
    for k, p0 in P.items():
        g = r["grads"][k].reshape(p0.shape).float()
        q = p0.clone().requires_grad_()
        q.grad = g
        torch.optim.Adam([q], lr=lr).step()
        dg = 1e-3 * float(g.abs().max())
        tol = lr * torch.clamp(dg / (g.abs() + eps), max=2.0) + 4 * 2.0 ** -24 * p0.abs()
        got = m.flat.w(k).detach().cpu()
        assert bool(((got - q.detach()).abs() <= tol).all()), k
        want_ema = 0.999 * p0 + (1 - 0.999) * q.detach()
        got_ema = m.flat.view(ema, k).cpu()
        assert bool(((got_ema - want_ema).abs() <= 0.001 * tol + 4 * 2.0 ** -24 * p0.abs()).all()), k
        # the EMA launch itself, on the parameters the device holds: bit for bit against its statement in numpy float32
        assert torch.equal(got_ema, R.ema_step32(p0, got, 0.999)), k
        worst = max(worst, float((got - q.detach()).abs().max()))
    print("adam step: max |p - torch| %.2e (lr %.0e)" % (worst, lr))
    assert int(optim.state[0]) == 1


def test_dropout_masks_fractions_and_counter():
    """train mode at B = 32: the backward uses the forward's masks, the kept fractions lie in the binomial 5-sigma band of 0.5 /
    0.3 dropped, and the counter advances with the optimizer step (other masks in the next step)"""
    from erc_amd.engine import FusedAdam
    m, _ = _module(5)
    optim = FusedAdam(m.flat, lr=2e-4)
    m.rng_state = optim.rng_state
    B = 32
    g = torch.Generator().manual_seed(9)
    batch = _gpu(dict(audio_feature=torch.randn(B, 17, R.AUDIO_D, generator=g), visual_feature=torch.randn(B, 9, R.VISUAL_D, generator=g),
                      text_feature=torch.randn(B, 22, R.TEXT_D, generator=g), label=torch.randint(0, 4, (B, ), generator=g)))
    m.train()
    m.loss_and_grads(batch)
    ws = m._last_ws
    e = ws["L"]

    def band(kept, n, keep_p):
        sigma = math.sqrt(keep_p * (1 - keep_p) / n)
        print("kept %d of %d: %.4f (band %.4f +- %.4f)" % (kept, n, kept / n, keep_p, 5 * sigma))
        return abs(kept / n - keep_p) <= 5 * sigma
    live = e["pooled"] > 0
    kept_text = (e["pd"] != 0) & live
    assert band(int(kept_text.sum()), int(live.sum()), 0.5)
    assert torch.equal(e["pd"][kept_text], e["pooled"][kept_text] * 2.0) and bool((e["pd"][~kept_text] == 0).all())
    # backward: dpooled = dpd x the same mask
    moving = e["dpd"] != 0
    assert torch.equal((e["dpooled"] != 0) & live, (e["pd"] != 0) & moving & live)
    assert torch.equal(e["dpooled"][kept_text], e["dpd"][kept_text] * 2.0)
    # classifier layers: pre-activations recomputed with torch on the device; clearly live ones are kept with probability 0.7
    masks = []
    for name, xin, out, dout in (("netC.module.0", ws["fused"], ws["z0"], ws["dz0"]), ("netC.module.3", ws["z0"], ws["feat"], ws["dfeat"])):
        pre = xin @ m.flat.w(name + ".weight").t() + m.flat.w(name + ".bias")
        clear = pre > 1e-4
        kept = (out != 0) & clear
        assert band(int(kept.sum()), int(clear.sum()), 0.7)
        assert float((out[kept] - pre[kept] / 0.7).abs().max()) < 1e-4
        assert bool((dout[(out == 0)] == 0).all())      # the backward's mask is the forward's
        masks.append(kept.clone())
    assert not torch.equal(masks[0], masks[1])           # the two layers draw different masks
    before = optim.rng_state.clone()
    text_mask = kept_text.clone()
    optim.step()
    assert int(optim.rng_state[0]) > int(before[0]) and int(optim.rng_state[1]) == int(before[1])
    m.loss_and_grads(batch)
    live2 = m._last_ws["L"]["pooled"] > 0
    assert not torch.equal((m._last_ws["L"]["pd"] != 0) & live2 & live, text_mask & live2)


def test_refusals_on_the_device():
    from erc_amd.mmin import MMINBaseModule
    m, _ = _module(3)
    g = torch.Generator().manual_seed(1)
    a, v, t = (torch.randn(2, T, D, generator=g).to(DEV) for T, D in ((6, R.AUDIO_D), (5, R.VISUAL_D), (7, R.TEXT_D)))
    for miss in ("audio_feature", "visual_feature", "text_feature"):
        kw = dict(audio_feature=a, visual_feature=v, text_feature=t)
        kw[miss] = None
        with pytest.raises(capi.ErcGraftError, match=miss):
            m(**kw)
    with pytest.raises(capi.ErcGraftError, match="text_feature has 4 tokens"):
        m(audio_feature=a, visual_feature=v, text_feature=t[:, :4].contiguous())
    with pytest.raises(capi.ErcGraftError, match="GPU"):
        MMINBaseModule(342, 1024, 130, 4).finalize(DEV)(audio_feature=a.cpu(), visual_feature=v, text_feature=t)
    assert [tuple(x.shape) for x in m.encode(visual_feature=v)] == [(2, H)]


def _params(*argv):
    from track_mm.mmin_base import MMINBaseParams
    return MMINBaseParams().from_args(list(argv))


def test_checkpoint_round_trip_with_ema(tmp_path):
    from erc_amd import mmin
    p = _params("--n_train=4", "--n_val=2", "--n_test=2", "--train.batch_size=2", "--mmin_frames=(6,9)")
    tr = mmin.MMINBaseTrainer(p, DEV)
    train_loader = mmin.make_loaders(p)[0]
    for item in train_loader:
        tr.train_step(tr.prepare_batch(item))
    assert not torch.equal(tr.ema, tr.model.flat.data)
    path = mmin.save(tr, str(tmp_path / "m.ckpt"))
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ckpt["models"]) == {"model", "ema_model"} and "optim" in ckpt["optims"]
    assert list(ckpt["models"]["ema_model"]) == list(ckpt["models"]["model"]) == [k for k, _ in R.SD_SHAPES]
    cpu = mmin.MMINBaseModule(R.VISUAL_D, R.TEXT_D, R.AUDIO_D, 4)                # never finalised: a plain nn.Module on the CPU
    cpu.load_state_dict(ckpt["models"]["ema_model"], strict=True)
    cpu.load_state_dict(ckpt["models"]["model"], strict=True)
    tr2 = mmin.MMINBaseTrainer(_params("--seed=7"), DEV)
    mmin.load(tr2, path)
    assert torch.equal(tr2.model.flat.data, tr.model.flat.data) and torch.equal(tr2.ema, tr.ema)
    assert torch.equal(tr2.model.flat.exp_avg, tr.model.flat.exp_avg) and int(tr2.optim.state[0]) == int(tr.optim.state[0]) == 2
    # the EMA pass computes with the EMA weights and puts the model's back
    batch = tr.prepare_batch(next(iter(train_loader)))
    tr.model.eval()
    own = tr.to_logits(batch).clone()
    with tr.ema_weights():
        shadow = tr.to_logits(batch).clone()
    assert not torch.equal(own, shadow) and torch.equal(tr.to_logits(batch), own)


def test_graph_replay_equals_the_eager_step_bit_for_bit():
    """three training steps (dropout on, Adam, EMA) on one batch: eagerly, and as two warm-up steps plus one replay of the step
    captured into a HIP graph (engine.GraphedStep) -- parameters, moments and the EMA copy bit for bit"""
    from erc_amd import mmin
    from erc_amd.engine import GraphedStep
    args = ("--n_train=4", "--train.batch_size=4", "--mmin_frames=(11,19)")
    item = next(iter(mmin.make_loaders(_params(*args))[0]))
    res = []
    for graphed in (False, True):
        tr = mmin.MMINBaseTrainer(_params(*args), DEV)
        batch = tr.prepare_batch(item)
        if graphed:
            step = GraphedStep(lambda: tr.train_step(batch), warmup=2)
            step()
        else:
            for _ in range(3):
                tr.train_step(batch)
        torch.cuda.synchronize()
        f = tr.model.flat
        res.append([t.clone() for t in (f.data, f.exp_avg, f.exp_avg_sq, tr.ema, tr.optim.state[:3])])
    assert int(res[0][4][0]) == 3
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_cli_one_epoch_on_a_small_synthetic_split():
    env = dict(os.environ, PYTHONPATH=REPO)
    res = subprocess.run([sys.executable, os.path.join(REPO, "train_mm.py"), "--module=mmin_base", "--epoch=1", "--n_train=8", "--n_val=4",
                          "--n_test=4", "--train.batch_size=4", "--mmin_frames=(20,40)", "--log_every=0"], capture_output=True, text=True,
                         env=env, timeout=300, cwd=REPO)
    assert res.returncode == 0, res.stderr[-2000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    assert line["epoch"] == 0 and set(line["val"]) == set(line["test"]) == {"Lall", "Acc", "Acc2"}
    assert line["class_names"] == ["hap", "sad", "neu", "ang"] and 0.0 <= line["test"]["Acc"] <= 1.0
