"""GPU: MMIN's missing-modality model (--module=mmin_miss) on libercgraft -- erc_resae_fwd / _bwd case by case against the float64
restatements of tests/mmin_miss_ref.py (bounds from the float32 twins, there), erc_mse_grad and erc_mmin_miss_combine, the whole
module against the reference's own classes (golden vectors) and the restatement, the pretrained model's loading rules, Adam + EMA
steps eagerly and replayed, and the command line.  Every test prints its measured figures before it asserts."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from erc_amd import capi
from erc_amd.engine import GemmPlanner, linear_wgrad
from tests import mmin_miss_ref as MR
from tests import mmin_ref as R
from tests.util_cases import fill_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, LAT1 = 384, 64
GUARD = 3              # rows (flat buffers: GUARD * 64 floats) behind every buffer a kernel writes: nothing may touch them
SENT = -77.25          # what the write sets are pre-filled with


@pytest.fixture(scope="module", autouse=True)
def _lib():
    capi.lib()


def _buf(rows, cols):
    return torch.full((rows + GUARD, cols), SENT, dtype=torch.float32, device=DEV)


def _flat(n):
    return torch.full((n + GUARD * 64, ), SENT, dtype=torch.float32, device=DEV)


def _f64(t):
    return t.detach().cpu().double()


def _report(tag, figs):
    print("%s: %s" % (tag, "  ".join("%s %.2e/%.0e" % (k, got, bnd) for k, (got, bnd) in figs.items())))


def _offsets(B, nb, per_block):
    out = []
    for i in range(nb):
        out += [B * (1216 * i + o) for o in per_block]
    return out + [B * 1216 * nb, B * (1216 * nb + 384)]


def _act_offsets(B, nb):
    """float offsets of the layers' input rows in ``act`` (include/ercgraft.h)"""
    return _offsets(B, nb, (0, 384, 640, 768, 832, 960))


def _dy_offsets(B, nb):
    return _offsets(B, nb, (0, 256, 384, 448, 576, 832))


# ------------------------------------------------------------------------------------------------------------ autoencoder
_AE_REF = {}


def _ae_ref(name, B, job):
    """the case, its float64 forward / backward, the twin's: computed once, shared, never modified"""
    key = (name, B, job)
    if key not in _AE_REF:
        c = MR.ae_case(name, B, job)
        _AE_REF[key] = (c, ) + MR.ae_reference(c, with_latents=(job == 0))
    return _AE_REF[key]


def _ae_sizes(name):
    Rg = capi.resae_rows_per_group()
    return [{"R-1": Rg - 1, "R": Rg, "R+1": Rg + 1}.get(s) or int(s) for s in MR.AE_CASES[name][0]]


class _AeRun:
    """device buffers of one job with guard bands (and pad columns when ``wide``), the job dict, views of what was written"""

    def __init__(self, c, job, wide):
        B, nb = c["B"], c["nb"]
        pad = 8 if wide else 0
        self.c, self.B, self.nb, self.pad = c, B, nb, pad
        self.W = [W.to(DEV).contiguous() for W, _ in c["P"]]
        self.b = [b.to(DEV).contiguous() for _, b in c["P"]]
        n_act = capi.resae_act_floats(B, nb)
        assert n_act == B * (1216 * nb + 768)
        self.x, self.d_recon = _buf(B, D + pad), _buf(B, D + pad)
        self.x[:B, :D], self.d_recon[:B, :D] = c["x"].to(DEV), c["d_recon"].to(DEV)
        self.d_latents = None
        if job == 0:
            self.d_latents = _buf(B, LAT1 * nb + pad)
            self.d_latents[:B, :LAT1 * nb] = c["d_latents"].to(DEV)
        self.recon, self.latents, self.dx = _buf(B, D + pad), _buf(B, LAT1 * nb + 2 * pad), _buf(B, D + pad)
        self.act, self.dY = _flat(n_act), _flat(n_act)
        self.n_act = n_act
        self.job = dict(W=self.W, b=self.b, x=self.x, recon=self.recon, latents=self.latents, act=self.act, d_recon=self.d_recon,
                        d_latents=self.d_latents, dx=self.dx, dY=self.dY, B=B, ldx=D + pad, ldr=D + pad, ldl=LAT1 * nb + 2 * pad,
                        lddr=D + pad, lddl=LAT1 * nb + pad, lddx=D + pad)
        self.inputs = [self.x.clone(), self.d_recon.clone(), None if self.d_latents is None else self.d_latents.clone()]

    def outs(self):
        return [self.recon, self.latents, self.dx, self.act, self.dY]

    def check_write_sets(self):
        B, nb = self.B, self.nb
        for t, width in ((self.recon, D), (self.latents, LAT1 * nb), (self.dx, D)):
            assert bool((t[B:] == SENT).all()) and bool((t[:B, width:] == SENT).all()), "guard rows / pad columns were written"
            assert not bool((t[:B, :width] == SENT).any())
        for t in (self.act, self.dY):
            assert bool((t[self.n_act:] == SENT).all()) and not bool((t[:self.n_act] == SENT).any())
        for t, was in zip((self.x, self.d_recon, self.d_latents), self.inputs):       # inputs are read only
            assert t is None or torch.equal(t, was)

    def layer_rows(self, flat, offsets, widths):
        return [_f64(flat[o:o + self.B * w]).reshape(self.B, w) for o, w in zip(offsets, widths)]


def _launch(runs, nb):
    jobs = capi.resae_jobs([r.job for r in runs])
    capi.resae_fwd(jobs, nb, len(runs))
    capi.resae_bwd(jobs, nb, len(runs))


def _wgrads(run):
    """every dW / db of the job through erc_wgrad_table (GemmPlanner.flush_wgrads), into a guarded flat gradient buffer"""
    B, nb = run.B, run.nb
    dims = MR.layer_dims(nb)
    offs, n = [], 0
    for n_out, n_in in dims:
        offs.append((n, n + n_out * n_in))
        n += n_out * n_in + n_out
    n = (n + 63) // 64 * 64
    grad = _flat(n)
    pl = GemmPlanner(DEV, 1 << 10, grad=grad)
    for (n_out, n_in), (w_off, b_off), x_off, y_off in zip(dims, offs, _act_offsets(B, nb), _dy_offsets(B, nb)):
        linear_wgrad(pl, run.dY[y_off:], n_out, run.act[x_off:], n_in, None, n_out, n_in, B, w_off, b_off, defer=True)
    assert len(pl.deferred) == 6 * nb + 2
    pl.flush_wgrads({})
    torch.cuda.synchronize()
    assert bool((grad[n:] == SENT).all())
    dW = [_f64(grad[w:w + o * i]).reshape(o, i) for (o, i), (w, _) in zip(dims, offs)]
    db = [_f64(grad[b:b + o]) for (o, _), (_, b) in zip(dims, offs)]
    return dW, db


CASE_RUNS = [(name, i) for name in sorted(MR.AE_CASES) for i in range(len(MR.AE_CASES[name][0]))]


@pytest.mark.parametrize("name,size", CASE_RUNS, ids=["%s%d" % c for c in CASE_RUNS])
def test_resae(name, size):
    """erc_resae_fwd / _bwd on one case: recon, latents, every saved activation, the mask condition, dx, every dY_l and through
    erc_wgrad_table every dW / db against float64 on the kernel's own masks; write sets; a second launch and (two jobs) one launch
    per job bit-identical"""
    B = _ae_sizes(name)[size]
    _, nb, n_jobs, dec_bias = MR.AE_CASES[name]
    wide = name == "c"
    refs = [_ae_ref(name, B, j) for j in range(n_jobs)]
    runs = [_AeRun(ref[0], j, wide) for j, ref in enumerate(refs)]
    _launch(runs, nb)
    first = [[t.clone() for t in r.outs()] for r in runs]
    _launch(runs, nb)
    torch.cuda.synchronize()
    for r, was in zip(runs, first):
        assert all(torch.equal(a, b) for a, b in zip(r.outs(), was)), "a second launch into the same buffers differs"
        r.check_write_sets()
    if n_jobs == 2:       # two jobs in one launch give the bits of one launch each
        alone = [_AeRun(ref[0], j, wide) for j, ref in enumerate(refs)]
        for r in alone:
            _launch([r], nb)
        torch.cuda.synchronize()
        for r, s in zip(runs, alone):
            assert all(torch.equal(a, b) for a, b in zip(r.outs(), s.outs())), "two jobs in one launch differ from one launch each"
    dims = MR.layer_dims(nb)
    nL = len(dims)
    for j, (run, (c, f64, b64, f32, b32)) in enumerate(zip(runs, refs)):
        figs = dict(recon=(R.rel(_f64(run.recon[:B, :D]), f64["recon"]), MR.twin_bound(f32["recon"], f64["recon"])),
                    latents=(R.rel(_f64(run.latents[:B, :LAT1 * nb]), f64["latents"]), MR.twin_bound(f32["latents"], f64["latents"])))
        acts = run.layer_rows(run.act, _act_offsets(B, nb), [i for _, i in dims])
        act_bounds = [MR.twin_bound(f32["acts"][l], f64["acts"][l]) for l in range(nL)]
        worst = max(range(nL), key=lambda l: R.rel(acts[l], f64["acts"][l]) / act_bounds[l])
        figs["acts"] = (R.rel(acts[worst], f64["acts"][worst]), act_bounds[worst])
        record = dict(recon=figs["recon"][0], latents=figs["latents"][0], acts=max(R.rel(acts[l], f64["acts"][l]) for l in range(nL)))
        for l in range(nL):
            assert R.rel(acts[l], f64["acts"][l]) <= act_bounds[l], ("acts", l)
        assert torch.equal(acts[0], c["x"].double())
        # masks: the kernel's are its saved post-activations > 0; where one differs from float64's, the float64 pre-activation
        # lies within that layer's forward bound (absolute) of the kink
        m64 = MR.masks_of(f64["pre"], nb)
        masks, n_diff = {}, 0
        for l in m64:
            masks[l] = acts[l + 1] > 0
            differ = masks[l] != m64[l]
            n_diff += int(differ.sum())
            scale = float(f64["acts"][l + 1].abs().max())
            tol = act_bounds[l + 1] * (scale if scale > 0 else 1.0)
            assert bool((f64["pre"][l][differ].abs() <= tol).all()), ("mask", l)
        with R.one_thread():
            k64 = b64 if n_diff == 0 else MR.resae_bwd(c["P"], f64["acts"], masks, c["d_recon"], c["d_latents"] if j == 0 else None, nb)
        figs["dx"] = (R.rel(_f64(run.dx[:B, :D]), k64["dx"]), MR.twin_bound(b32["dx"], b64["dx"]))
        dY = run.layer_rows(run.dY, _dy_offsets(B, nb), [o for o, _ in dims])
        dW, db = _wgrads(run)
        for key, got in (("dY", dY), ("dW", dW), ("db", db)):
            bounds = [MR.twin_bound(b32[key][l], b64[key][l]) for l in range(nL)]
            errs = [R.rel(got[l], k64[key][l]) for l in range(nL)]
            w = max(range(nL), key=lambda l: errs[l] / bounds[l])
            figs[key] = (errs[w], bounds[w])
            record[key] = max(errs)
            for l in range(nL):
                assert errs[l] <= bounds[l], (key, l, errs[l], bounds[l])
        assert torch.equal(dY[nL - 1], c["d_recon"].double())
        record["dx"] = figs["dx"][0]
        # per-layer quantities: the layer closest to its bound above; their worst layer here (the FIGURES record's third column)
        _report("resae %s B=%d n_blocks=%d job %d of %d (%d mask elements differ from float64's)" % (name, B, nb, j, n_jobs, n_diff), figs)
        print("FIGURES %s/B%d/job%d %s" % (name, B, j, " ".join("%s=%.2e" % kv for kv in record.items())))
        for k, (g, bnd) in figs.items():
            assert g <= bnd, (k, g, bnd)
        if dec_bias is not None:       # ReLU-dead decoders: the gradients through them are exactly zero
            for i in range(nb):
                for l in (6 * i + 3, 6 * i + 4):
                    assert bool((dY[l] == 0).all()) and bool((dW[l] == 0).all()) and bool((db[l] == 0).all()) and bool((acts[l + 1] == 0).all())
                assert bool((dW[6 * i + 5] == 0).all())
                for l in (6 * i, 6 * i + 1):       # LeakyReLU on both sides
                    assert bool(masks[l].any()) and bool((~masks[l]).any())


def test_resae_refuses_bad_arguments_by_status_without_a_launch():
    assert (capi.resae_input(), capi.resae_latent(), capi.resae_max_jobs(), capi.resae_max_blocks()) == (D, LAT1, 2, 5)
    assert capi.resae_rows_per_group() >= 1 and capi.resae_act_floats(7, 3) == 7 * (1216 * 3 + 768)
    c = _ae_ref("b", _ae_sizes("b")[0], 0)[0]
    run = _AeRun(c, 0, False)
    nb = c["nb"]
    odd = torch.zeros(256 * 384 + 1, device=DEV)[1:]       # 4 bytes off a 16-byte boundary
    for fn, bads in ((capi.resae_fwd, (dict(x=None), dict(recon=None), dict(latents=None), dict(act=None), dict(B=0), dict(B=-1),
                                       dict(ldx=D - 1), dict(ldr=D - 1), dict(ldl=LAT1 * nb - 1), dict(W=[odd] + run.W[1:]),
                                       dict(W=run.W[:-1]), dict(b=run.b[:-1]), dict(act=run.act[1:]))),
                     (capi.resae_bwd, (dict(d_recon=None), dict(dx=None), dict(dY=None), dict(lddr=D - 1), dict(lddx=D - 1),
                                       dict(lddl=LAT1 * nb - 1), dict(B=0), dict(dY=run.dY[1:])))):
        for bad in bads:
            with pytest.raises(capi.ErcGraftError, match="resae_"):
                fn([dict(run.job, **bad)], nb)
        for n_blocks in (0, 6):
            with pytest.raises(capi.ErcGraftError, match="n_blocks"):
                fn([run.job], n_blocks)
        with pytest.raises(capi.ErcGraftError, match="n_jobs"):
            fn([run.job] * 3, nb)
    torch.cuda.synchronize()
    for t in run.outs():
        assert bool((t == SENT).all()), "a refused call wrote"


# ------------------------------------------------------------------------------------------------------ mse and combine
@pytest.mark.parametrize("B", [1, 33])
def test_mse_grad(B):
    g = torch.Generator().manual_seed(40 + B)
    a, b = torch.randn(B, D, generator=g), torch.randn(B, D, generator=g)
    weight = 4.0
    with R.one_thread():
        loss64, d64 = MR.mse_pair(a, b, weight)
        loss32, d32 = MR.mse_pair(a, b, weight, dtype=torch.float32)
    A, Bm, d, stats = _buf(B, D + 8), _buf(B, D + 4), _buf(B, D + 12), _buf(1, 8)
    A[:B, :D], Bm[:B, :D] = a.to(DEV), b.to(DEV)
    capi.mse_grad(A, D + 8, Bm, D + 4, B, D, weight, d, D + 12, stats[0, 2:])
    first = (d.clone(), stats.clone())
    capi.mse_grad(A, D + 8, Bm, D + 4, B, D, weight, d, D + 12, stats[0, 2:])
    torch.cuda.synchronize()
    assert torch.equal(first[0], d) and torch.equal(first[1], stats)
    assert bool((d[B:] == SENT).all()) and bool((d[:B, D:] == SENT).all()) and bool((stats[1:] == SENT).all())
    assert bool((stats[0, :2] == SENT).all()) and bool((stats[0, 3:] == SENT).all())
    figs = dict(loss=(abs(float(stats[0, 2]) - float(loss64)) / float(loss64), MR.twin_bound(loss32, loss64)),
                d=(R.rel(_f64(d[:B, :D]), d64), MR.twin_bound(d32, d64)))
    _report("mse_grad B=%d" % B, figs)
    for k, (got, bnd) in figs.items():
        assert got <= bnd, (k, got, bnd)
    for bad in (dict(B=0), dict(lda=D - 1), dict(ldd=D - 1), dict(a=None), dict(loss=None)):
        kw = dict(dict(a=A, lda=D + 8, b=Bm, ldb=D + 4, B=B, n=D, w=weight, d=d, ldd=D + 12, loss=stats[0, 2:]), **bad)
        with pytest.raises(capi.ErcGraftError, match="mse_grad"):
            capi.mse_grad(kw["a"], kw["lda"], kw["b"], kw["ldb"], kw["B"], kw["n"], kw["w"], kw["d"], kw["ldd"], kw["loss"])


def test_miss_combine_is_the_elementwise_statement():
    B = 19
    g = torch.Generator().manual_seed(6)
    dx0, dx1, dcyc, feat = (torch.randn(B, D, generator=g).to(DEV) for _ in range(4))
    ce = torch.tensor([1.25, 7.0] + [0.0] * 6, device=DEV)
    dfeat, dtext, stats = _buf(B, D + 8), _buf(B, 128 + 4), _buf(1, 8)
    stats[0, 2], stats[0, 3] = 0.5, 0.125
    capi.mmin_miss_combine(dx0, dx1, dcyc, feat, D, B, dfeat, D + 8, dtext, 128 + 4, ce, 4.0, 2.0, stats[0])
    torch.cuda.synchronize()
    want = dx0 + dx1 - dcyc
    assert torch.equal(dfeat[:B, :D], want)
    assert torch.equal(dtext[:B, :128], torch.where(feat[:, 256:] > 0, want[:, 256:], torch.zeros_like(want[:, 256:])))
    assert bool((dfeat[B:] == SENT).all()) and bool((dfeat[:B, D:] == SENT).all()) and bool((dtext[B:] == SENT).all())
    assert bool((dtext[:B, 128:] == SENT).all())
    assert stats[0, :5].tolist() == [1.25 + 4.0 * 0.5 + 2.0 * 0.125, 7.0, 0.5, 0.125, 1.25] and bool((stats[0, 5:] == SENT).all())
    with pytest.raises(capi.ErcGraftError, match="mmin_miss_combine"):
        capi.mmin_miss_combine(dx0, dx1, dcyc, feat, D - 1, B, dfeat, D + 8, dtext, 132, ce, 4.0, 2.0, stats[0])


# ----------------------------------------------------------------------------------------------------------------- module
def _gpu(batch):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _modules(fx):
    from erc_amd.mmin import MMINBaseModule
    from erc_amd.mmin_miss import MMINMissModule
    m = MMINMissModule(visual_dim=R.VISUAL_D, text_dim=R.TEXT_D, audio_dim=R.AUDIO_D, n_classes=4)
    fill_params(m, int(fx["param_seed"]))
    P = {k: v.detach().clone() for k, v in m.state_dict().items()}
    pre = MMINBaseModule(visual_dim=R.VISUAL_D, text_dim=R.TEXT_D, audio_dim=R.AUDIO_D, n_classes=4)
    fill_params(pre, int(fx["pretrained_seed"]))
    Ppre = {k: v.detach().clone() for k, v in pre.state_dict().items()}
    return m.finalize(DEV), P, pre.finalize(DEV), Ppre


def _kernel_routing(m, B):
    ws = m._last_ws
    args = dict(audio=ws["A"]["arg"].cpu().long(), visual=ws["V"]["arg"].cpu().long(), text=ws["L"]["arg"].cpu().long())
    offs, dims = _act_offsets(B, MR.N_BLOCKS), MR.layer_dims(MR.N_BLOCKS)
    masks = {}
    for j, net in enumerate(("netAE", "netAE_cycle")):
        act = ws["ae_act"][j]
        masks[net] = {l: _f64(act[offs[l + 1]:offs[l + 1] + B * dims[l][0]]).reshape(B, dims[l][0]) > 0
                      for l in range(len(dims)) if MR.activation_of(l, MR.N_BLOCKS)}
    return args, masks


@pytest.mark.parametrize("name", sorted(MR.MODEL_CASES))
def test_module_matches_reference_fixture_and_restatement(golden, name):
    """eval-mode forward and loss_and_grads against the reference's classes (logits, fusion, fusion_cycle, features, the
    pretrained model's reverse features, the four losses, every gradient digest) within the twin-derived bound plus the fixture's
    own deviation from float64 (plus, for a gradient, what float64 itself moves by between its own routing / masks and the
    kernels'), and against the float64 restatement on the kernels' own routing and masks within the twin's bound"""
    fx = golden(name)
    m, P, pre, Ppre = _modules(fx)
    assert list(m.state_dict()) == [str(k) for k in fx["sd_keys"]] == [k for k, _ in MR.sd_shapes()]
    assert sum(p.numel() for p in m.parameters()) == int(fx["n_params"]) == MR.N_PARAMS and len(m.flat.params) == 150
    full = {k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("in_")}
    batch = MR.apply_missing(full, torch.from_numpy(fx["missing_type"]))
    B = int(full["label"].shape[0])
    dev = _gpu(batch)
    m.eval(), pre.eval()
    rev = torch.cat(pre.encode(dev["audio_feature_reverse"], dev["visual_feature_reverse"], dev["text_feature_reverse"]), -1).clone()
    logits, fusion, fusion_cycle, features = (t.clone() for t in m(**dev))
    stats = m.loss_and_grads(dev, rev).clone()
    torch.cuda.synchronize()
    args, masks = _kernel_routing(m, B)
    with R.one_thread():
        rev64 = MR.encode(Ppre, batch["audio_feature_reverse"], batch["visual_feature_reverse"], batch["text_feature_reverse"])["features"]
        rev32 = MR.encode(Ppre, batch["audio_feature_reverse"], batch["visual_feature_reverse"], batch["text_feature_reverse"],
                          dtype=torch.float32)["features"]
        r64 = MR.model_loss_grads(P, batch, rev64)
        r32 = MR.model_loss_grads(P, batch, rev32, dtype=torch.float32, masks=r64["masks"], args=r64["args"])
        same = all(torch.equal(args[k], r64["args"][k]) for k in args) and \
            all(torch.equal(masks[n][l], r64["masks"][n][l]) for n in masks for l in masks[n])
        k64 = r64 if same else MR.model_loss_grads(P, batch, rev64, masks=masks, args=args)
    # the kernels' routing is a condition, not an equality (tests/mmin_ref.py): a routed step's float64 value lies within the
    # pool's bound of the float64 maximum; the text CNN routes every live channel as float64 does
    e64, e32 = r64["enc"], r32["enc"]
    for key, tag in (("audio", "A"), ("visual", "V")):
        tol = MR.twin_bound(e32[tag]["pool"], e64[tag]["pool"]) * float(e64[tag]["pool"].abs().max())
        assert R.arg_condition(e64[tag]["hs"], args[key], tol) == 0, key
    live = e64["L"]["pooled"] > 0
    assert bool((args["text"] == e64["L"]["arg"])[live].all())
    figs = {}

    def both(key, got, want64, want32, fixture):
        """(error against float64, the twin's bound), and the check against the fixture: that bound plus the fixture's own
        deviation from float64, both as absolute figures"""
        got, want64, fixture = _f64(got).reshape(want64.shape), want64.double(), torch.as_tensor(fixture).double().reshape(want64.shape)
        bnd = MR.twin_bound(want32, want64)
        scale = float(want64.abs().max()) or 1.0
        figs[key] = (R.rel(got, want64), bnd)
        assert float((got - fixture).abs().max()) <= bnd * scale + float((fixture - want64).abs().max()), (key, "fixture")
    both("reverse", rev, rev64, rev32, fx["reverse_features"])
    for key, got in (("logits", logits), ("fusion", fusion), ("fusion_cycle", fusion_cycle), ("features", features)):
        both(key, got, r64[key], r32[key], fx[key])
    for slot, key in ((0, "Lall"), (2, "Lmse"), (3, "Lcycle"), (4, "Lce")):
        both(key, stats[slot], k64[key], r32[key], fx[key])
    assert int(stats[1]) == int((r64["logits"].argmax(-1) == full["label"]).sum())
    worst = (0.0, 1.0, "")
    for k, g64 in k64["grads"].items():
        got = _f64(m.flat.g(k)).reshape(g64.shape)
        bnd = MR.twin_bound(r32["grads"][k].reshape(g64.shape), r64["grads"][k])
        err = R.rel(got, g64)
        if err / bnd > worst[0] / worst[1]:
            worst = (err, bnd, k)
        assert err <= bnd, (k, err, bnd)
        scale = float(g64.abs().max()) or 1.0
        fixture = torch.from_numpy(fx["gd__" + k.replace(".", "__")]).double()
        own = float((fixture - MR.digest(r64["grads"][k])).abs().max())
        # the fixture ran on float64's routing and masks: where the kernels' differ (within the conditions above), so does
        # float64 itself, by ``moved``
        moved = 0.0 if same else float((MR.digest(g64) - MR.digest(r64["grads"][k])).abs().max())
        assert float((MR.digest(got) - fixture).abs().max()) <= bnd * scale + own + moved, (k, "fixture")
    figs["grads (worst: %s)" % worst[2]] = worst[:2]
    _report("%s (B=%d, routing and masks %s float64's)" % (name, B, "are" if same else "differ from"), figs)
    for k, (g, bnd) in figs.items():
        assert g <= bnd, (k, g, bnd)
    assert [str(s) for s in fx["grad_none"]] == []


def test_state_dict_round_trip():
    from erc_amd.mmin_miss import MMINMissModule
    a = MMINMissModule(R.VISUAL_D, R.TEXT_D, R.AUDIO_D, 4)
    fill_params(a, 7)
    a.finalize(DEV)
    sd = {k: v.detach().cpu().clone() for k, v in a.state_dict().items()}
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == list(MR.sd_shapes())
    b = MMINMissModule(R.VISUAL_D, R.TEXT_D, R.AUDIO_D, 4).finalize(DEV)
    b.load_state_dict(sd, strict=True)
    assert torch.equal(a.flat.data, b.flat.data)
    cpu = MMINMissModule(R.VISUAL_D, R.TEXT_D, R.AUDIO_D, 4)                # never finalised: a plain nn.Module on the CPU
    cpu.load_state_dict(sd, strict=True)
    g = torch.Generator().manual_seed(2)
    batch = _gpu(dict(audio_feature=torch.randn(3, 9, R.AUDIO_D, generator=g), visual_feature=torch.randn(3, 6, R.VISUAL_D, generator=g),
                      text_feature=torch.randn(3, 7, R.TEXT_D, generator=g)))
    a.eval(), b.eval()
    for x, y in zip(a(**batch), b(**batch)):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
    assert [tuple(t.shape) for t in a(**batch)] == [(3, 4), (3, 384), (3, 384), (3, 384)]


def _params(cls, *argv):
    return cls().from_args(list(argv))


SMALL = ("--n_train=4", "--n_val=2", "--n_test=2", "--train.batch_size=4", "--mmin_frames=(11,19)")


def _base_checkpoint(tmp_path):
    from erc_amd import mmin
    from track_mm.mmin_base import MMINBaseParams
    base = mmin.MMINBaseTrainer(_params(MMINBaseParams, "--seed=5", *SMALL), DEV)
    for item in mmin.make_loaders(base.params)[0]:
        base.train_step(base.prepare_batch(item))
    return base, mmin.save(base, str(tmp_path / "base.ckpt"))


def _miss_trainer(*argv):
    from erc_amd.mmin_miss import MMINMissTrainer
    from track_mm.mmin_miss import MMINMissParams
    p = _params(MMINMissParams, *SMALL, *argv)
    tr = MMINMissTrainer(p, DEV)
    if p.pretrain_path:
        tr.load_pretrained(p.pretrain_path)
    return tr


def _train_batch(tr, seed=1):
    import random
    random.seed(seed)
    return tr.prepare_batch(next(iter(tr.make_loaders(tr.params)[0])))


def test_base_checkpoint_loads_as_the_pretrained_model(tmp_path):
    """a mmin_base checkpoint saved by this library, --pretrain_reinit=False: the pretrained model's ``encode`` on the reverse
    inputs equals the base module's bit for bit, and three training steps (also under --finetune) leave it unchanged"""
    base, path = _base_checkpoint(tmp_path)
    for extra in ((), ("--finetune", )):
        tr = _miss_trainer("--pretrain_path=" + path, "--pretrain_reinit=False", *extra)
        assert torch.equal(tr.pretrained_model.flat.data, base.model.flat.data)
        batch = _train_batch(tr)
        rev = [batch[k + "_reverse"] for k in ("audio_feature", "visual_feature", "text_feature")]
        base.model.eval(), tr.pretrained_model.eval()
        for x, y in zip(base.model.encode(*rev), tr.pretrained_model.encode(*rev)):
            assert torch.equal(x, y) and bool((x != 0).any())
        before, own = tr.pretrained_model.flat.data.clone(), tr.model.flat.data.clone()
        counter = tr.pretrained_model.rng_state.clone()
        for _ in range(3):
            stats = tr.train_step(batch)
        torch.cuda.synchronize()
        assert torch.equal(tr.pretrained_model.flat.data, before) and not torch.equal(tr.model.flat.data, own)
        assert bool(torch.isfinite(stats[:5]).all()) and tr.pretrained_model.training
        assert (tr.pretrained_model.rng_state - counter).tolist() == [3, 0]           # its dropout counter: one draw per step
        assert float(tr.pretrained_model.flat.grad.abs().max()) == 0.0                 # no gradient is ever computed for it
    # the default re-initialises it: Conv weights re-drawn, biases zero, LSTMs as loaded
    tr = _miss_trainer("--pretrain_path=" + path)
    w = lambda t, k: t.flat.w(k)
    assert not torch.equal(w(tr.pretrained_model, "netL.conv1.weight"), w(base.model, "netL.conv1.weight"))
    assert float(w(tr.pretrained_model, "netC.module.0.bias").abs().max()) == 0.0 and float(w(tr.pretrained_model, "netL.conv2.bias").abs().max()) == 0.0
    assert torch.equal(w(tr.pretrained_model, "netA.rnn.weight_hh_l0"), w(base.model, "netA.rnn.weight_hh_l0"))
    assert torch.equal(w(tr.pretrained_model, "netL.embd.0.weight"), w(base.model, "netL.embd.0.weight"))


def test_three_eager_steps_equal_the_replayed_graph_and_the_ema_statement():
    """three training steps (dropout on, Adam, EMA) on one batch: eagerly, and as two warm-up steps plus one replay of the step
    captured into a HIP graph (engine.GraphedStep) -- parameters, moments, the EMA copy and the pretrained model's counter bit for
    bit; the EMA copy after every eager step is mmin_ref.ema_step32 of the parameters the device held"""
    from erc_amd.engine import GraphedStep
    res = []
    for graphed in (False, True):
        tr = _miss_trainer()
        batch = _train_batch(tr)
        if graphed:
            step = GraphedStep(lambda: tr.train_step(batch), warmup=2)
            step()
        else:
            ema = tr.ema.cpu().clone()
            for _ in range(3):
                tr.train_step(batch)
                ema = R.ema_step32(ema, tr.model.flat.data.cpu(), 0.999)
            assert torch.equal(tr.ema.cpu(), ema) and not torch.equal(tr.ema, tr.model.flat.data)
        torch.cuda.synchronize()
        f = tr.model.flat
        res.append([t.clone() for t in (f.data, f.exp_avg, f.exp_avg_sq, tr.ema, tr.optim.state[:3], tr.pretrained_model.rng_state)])
    assert int(res[0][4][0]) == 3
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_cli_one_epoch_from_a_base_checkpoint(tmp_path):
    env = dict(os.environ, PYTHONPATH=REPO)
    small = ["--epoch=1", "--n_train=8", "--n_val=4", "--n_test=4", "--train.batch_size=4", "--mmin_frames=(20,40)"]
    base_dir, miss_dir = str(tmp_path / "base"), str(tmp_path / "miss")
    for module, extra in (("mmin_base", ["--log_every=0", "--save_dir=" + base_dir]),
                          ("mmin_miss", ["--save_dir=" + miss_dir, "--pretrain_path=" + os.path.join(base_dir, "last_model.ckpt")])):
        res = subprocess.run([sys.executable, os.path.join(REPO, "train_mm.py"), "--module=" + module] + small + extra,
                             capture_output=True, text=True, env=env, timeout=300, cwd=REPO)
        assert res.returncode == 0, res.stderr[-2000:]
    lines = [json.loads(l) for l in res.stdout.strip().splitlines() if l.startswith("{")]
    steps, line = lines[:-1], lines[-1]
    assert len(steps) == 2 and all(math.isfinite(s["Lall"]) and 0.0 <= s["Acc"] <= 1.0 for s in steps)
    assert line["epoch"] == 0 and set(line["val"]) == set(line["test"]) == {"Lall", "Acc", "Acc2"}
    assert all(math.isfinite(line[k]["Lall"]) for k in ("val", "test")) and line["class_names"] == ["hap", "sad", "neu", "ang"]
    for tag in ("best_model", "last_model"):
        if tag == "last_model" or line["is_best"]:
            ckpt = torch.load(os.path.join(miss_dir, tag + ".ckpt"), map_location="cpu", weights_only=True)
            assert set(ckpt["models"]) == {"model", "pretrained_model", "ema_model"} and len(ckpt["models"]["model"]) == 150
            assert os.path.exists(os.path.join(miss_dir, tag + ".json"))
