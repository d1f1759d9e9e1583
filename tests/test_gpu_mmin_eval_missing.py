"""GPU: ``--module=mmin_miss --eval_missing`` -- erc_resae_latents against erc_resae_fwd bit for bit, erc_mmin_miss_expand and
erc_mmin_miss_score against their torch / float64 statements (all through the C-ABI), the whole evaluation path against the naive
route (the same batches masked on the host with MMINMissCollate's arithmetic, six more passes of the unchanged forward) and against
the float64 restatement of tests/mmin_eval_missing_ref.py, and the command line.  Every test prints its figures before it asserts."""
import json
import math
import os
import random
import subprocess
import sys

import pytest
import torch

from erc_amd import capi
from tests import mmin_eval_missing_ref as ER
from tests import mmin_miss_ref as MR
from tests import mmin_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, LAT1 = 384, 64
GUARD = 3
SENT = -77.25


@pytest.fixture(scope="module", autouse=True)
def _lib():
    capi.lib()


def _buf(rows, cols):
    return torch.full((rows + GUARD, cols), SENT, dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------------------------------------------- erc_resae_latents
def _ae(B, nb):
    g = torch.Generator().manual_seed(1000 * nb + B)
    P = MR.ae_params(nb, g)
    W, b = [w.to(DEV).contiguous() for w, _ in P], [v.to(DEV).contiguous() for _, v in P]
    return W, b, torch.randn(B, D, generator=g).to(DEV)


@pytest.mark.parametrize("nb", [1, 5])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])
def test_resae_latents_carries_the_bits_of_resae_fwd(B, nb):
    """the 16-row group's edges, one block and the model's five: latents bit-equal to erc_resae_fwd's on the same x; recon / act
    handed in the job stay untouched, NULL for them is accepted; guard rows and pad columns stay; a second launch is identical"""
    W, b, x0 = _ae(B, nb)
    pad = 8
    x = _buf(B, D + pad)
    x[:B, :D] = x0
    n_act = capi.resae_act_floats(B, nb)
    full = dict(W=W, b=b, x=x, recon=_buf(B, D), latents=_buf(B, LAT1 * nb), act=torch.zeros(n_act, device=DEV), B=B, ldx=D + pad, ldr=D,
                ldl=LAT1 * nb)
    capi.resae_fwd([full], nb)
    want = full["latents"][:B].clone()
    assert not bool((want == SENT).any())
    recon, act, lat = _buf(B, D), torch.full((n_act + 64, ), SENT, device=DEV), _buf(B, LAT1 * nb + pad)
    job = dict(W=W, b=b, x=x, recon=recon, latents=lat, act=act, dx=recon, dY=act, B=B, ldx=D + pad, ldr=D, ldl=LAT1 * nb + pad)
    capi.resae_latents(job, nb)
    first = lat.clone()
    capi.resae_latents(job, nb)
    lat_null = _buf(B, LAT1 * nb)
    capi.resae_latents(dict(W=W, b=b, x=x, latents=lat_null, B=B, ldx=D + pad, ldl=LAT1 * nb), nb)
    torch.cuda.synchronize()
    assert torch.equal(lat[:B, :LAT1 * nb], want), "latents differ from erc_resae_fwd's"
    assert torch.equal(lat_null[:B], want) and bool((lat_null[B:] == SENT).all())
    assert torch.equal(first, lat), "a second launch differs"
    assert bool((lat[B:] == SENT).all()) and bool((lat[:B, LAT1 * nb:] == SENT).all())
    assert bool((recon == SENT).all()) and bool((act == SENT).all()), "recon / act were written"
    assert torch.equal(x[:B, :D], x0) and bool((x[B:] == SENT).all())


def test_resae_latents_refuses_bad_arguments_without_a_launch():
    B, nb = 5, 2
    W, b, x = _ae(B, nb)
    lat = _buf(B, LAT1 * nb)
    job = dict(W=W, b=b, x=x, latents=lat, B=B, ldx=D, ldl=LAT1 * nb)
    odd = torch.zeros(256 * 384 + 1, device=DEV)[1:]
    for bad in (dict(x=None), dict(latents=None), dict(B=0), dict(B=-3), dict(ldx=D - 1), dict(ldl=LAT1 * nb - 1), dict(W=[odd] + W[1:]),
                dict(W=W[:-1]), dict(b=b[:-1])):
        with pytest.raises(capi.ErcGraftError, match="resae_latents"):
            capi.resae_latents(dict(job, **bad), nb)
    for n_blocks in (0, 6):
        with pytest.raises(capi.ErcGraftError, match="n_blocks"):
            capi.resae_latents(job, n_blocks)
    with pytest.raises(capi.ErcGraftError, match="resae_latents"):
        capi._call("erc_resae_latents", None, nb)
    torch.cuda.synchronize()
    assert bool((lat == SENT).all()), "a refused call wrote"


# ---------------------------------------------------------------------------------------------------- erc_mmin_miss_expand
@pytest.mark.parametrize("n_cond", [6, 1])
@pytest.mark.parametrize("B", [1, 3, 33])
def test_miss_expand_is_the_column_block_selection(B, n_cond):
    g = torch.Generator().manual_seed(50 + B)
    types = MR.MISSING_TYPES if n_cond == 6 else ((1, 0, 1), )
    feat, z = _buf(B, D + 4), torch.randn(D, generator=g).to(DEV)
    feat[:B, :D] = torch.randn(B, D, generator=g).to(DEV)
    out = _buf(n_cond * B, D + 8)
    capi.mmin_miss_expand(feat, D + 4, z, capi.mmin_miss_patterns(types), B, out, D + 8)
    torch.cuda.synchronize()
    want = torch.cat([torch.where(ER.keep_columns(p).to(DEV), feat[:B, :D], z.expand(B, D)) for p in types])
    assert torch.equal(out[:n_cond * B, :D], want)
    assert bool((out[n_cond * B:] == SENT).all()) and bool((out[:n_cond * B, D:] == SENT).all()), "guard rows / pad columns were written"
    assert capi.mmin_miss_max_cond() == 8


def test_miss_expand_refuses_bad_arguments_without_a_launch():
    B = 3
    feat, z, out = torch.ones(B, D, device=DEV), torch.ones(D, device=DEV), _buf(6 * B, D)
    pat = capi.mmin_miss_patterns(MR.MISSING_TYPES)
    ok = dict(feat=feat, ldf=D, z=z, pat=pat, B=B, out=out, ldo=D)
    off = torch.full((6 * B * D + 4, ), SENT, device=DEV)
    for bad in (dict(feat=None), dict(z=None), dict(out=None), dict(pat=None), dict(B=0), dict(B=-1), dict(ldf=D - 4), dict(ldo=D - 4),
                dict(ldf=D + 1), dict(ldo=D + 2), dict(out=off[1:]), dict(z=off[1:]), dict(feat=off[3:]),
                dict(pat=capi.mmin_miss_patterns(MR.MISSING_TYPES * 2)), dict(pat=(capi.C.c_int32 * 1)(8)),
                dict(pat=(capi.C.c_int32 * 1)(-1))):
        kw = dict(ok, **bad)
        with pytest.raises(capi.ErcGraftError, match="mmin_miss_expand"):
            capi.mmin_miss_expand(kw["feat"], kw["ldf"], kw["z"], kw["pat"], kw["B"], kw["out"], kw["ldo"])
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((off == SENT).all()), "a refused call wrote"


# ----------------------------------------------------------------------------------------------------- erc_mmin_miss_score
@pytest.mark.parametrize("C,B", [(4, 7), (16, 7), (4, 300)])
def test_miss_score_counts_and_sums(C, B):
    """crafted logits (multiples of 1/8: exact in float32): ties (the first index wins), a label out of range, a row of NaN;
    two calls accumulate; cm exactly the float64 statement's, loss_sum within 1e-12 relative; guard entries stay"""
    n_cond = 3
    g = torch.Generator().manual_seed(7 * C + B)
    logits = torch.randint(-24, 25, (n_cond * B, C), generator=g).float() / 8
    labels = torch.randint(0, C, (B, ), generator=g)
    logits[0, 1], logits[0, 3] = 9.0, 9.0                  # a tie: index 1
    logits[B + 2] = 1.5                                    # all equal: index 0
    logits[2 * B + 1] = float("nan")                       # never counted
    labels[4] = C                                          # out of range: never counted, in every block
    labels[5] = -1
    assert C <= capi.rows_score_max_classes()
    pad = 3
    lg = _buf(n_cond * B, C + pad)
    lg[:n_cond * B, :C] = logits.to(DEV)
    cm = torch.zeros(n_cond * C * C + 8, dtype=torch.int64, device=DEV)
    cm[n_cond * C * C:] = -5
    sums = torch.zeros(n_cond + 2, dtype=torch.float64, device=DEV)
    sums[n_cond:] = SENT
    before = lg.clone()
    for _ in range(2):
        capi.mmin_miss_score(lg, C + pad, labels.to(DEV), B, n_cond, C, cm, sums)
    torch.cuda.synchronize()
    want_cm, want_loss = ER.score(logits, labels, n_cond)
    got_cm = cm[:n_cond * C * C].reshape(n_cond, C, C).cpu()
    assert int(want_cm.sum()) == n_cond * (B - 2) - 1
    assert want_cm[0, int(labels[0]), 1] >= 1 and want_cm[1, int(labels[2]), 0] >= 1
    err = float(((sums[:n_cond].cpu() - 2 * want_loss).abs() / (2 * want_loss).abs()).max())
    print("miss_score C=%d B=%d: loss_sum relative error %.2e (bound 1e-12)" % (C, B, err))
    assert torch.equal(got_cm, 2 * want_cm)
    assert err <= 1e-12
    assert bool((cm[n_cond * C * C:] == -5).all()) and bool((sums[n_cond:] == SENT).all()) and torch.equal(lg.isnan(), before.isnan())
    assert torch.equal(lg.nan_to_num(), before.nan_to_num())


def test_miss_score_refuses_bad_arguments_without_a_launch():
    B, C = 4, 4
    lg, y = torch.zeros(6 * B, C, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV)
    cm, sums = torch.zeros(6, C, C, dtype=torch.int64, device=DEV), torch.zeros(6, dtype=torch.float64, device=DEV)
    ok = dict(lg=lg, ld=C, y=y, B=B, n=6, C=C, cm=cm, s=sums)
    for bad in (dict(lg=None), dict(y=None), dict(cm=None), dict(s=None), dict(B=0), dict(n=0), dict(n=9), dict(C=0), dict(C=17, ld=17),
                dict(ld=C - 1)):
        kw = dict(ok, **bad)
        with pytest.raises(capi.ErcGraftError, match="mmin_miss_score"):
            capi.mmin_miss_score(kw["lg"], kw["ld"], kw["y"], kw["B"], kw["n"], kw["C"], kw["cm"], kw["s"])
    torch.cuda.synchronize()
    assert int(cm.abs().sum()) == 0 and float(sums.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------------------- whole path
def _gpu(batch):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _trainer(*extra, weights=True):
    from erc_amd.mmin_miss import MMINMissTrainer
    from track_mm.mmin_miss import MMINMissParams
    tr = MMINMissTrainer(MMINMissParams().from_args(list(ER.WHOLE_PATH_ARGS) + list(extra)), DEV)
    if weights:       # seeded weights the host test vouches for; the EMA copy gets a set of its own, so that the two passes differ
        tr.model.load_state_dict(ER.whole_path_weights(0), strict=True)
        flat = tr.model.flat
        for k, v in ER.whole_path_weights(1).items():
            flat.view(tr.ema, k).copy_(v.to(DEV))
    return tr


def _state(tr):
    f = tr.model.flat
    return [t.clone() for t in (f.data, tr.model.rng_state, tr.pretrained_model.rng_state, tr.ema, f.exp_avg, f.exp_avg_sq,
                                tr.pretrained_model.flat.data, tr.optim.state)]


def _cm_of(pred, labels, C=4):
    cm = torch.zeros(C, C, dtype=torch.int64)
    for y, p in zip(labels.tolist(), pred.tolist()):
        cm[y, p] += 1
    return cm


@pytest.fixture(scope="module")
def whole():
    """one evaluation of the validation split with the flag (both passes), the per-batch fused and naive logits of both passes,
    and the same evaluation without the flag; shared by the tests below, never modified"""
    tr = _trainer("--eval_missing")
    loaders = tr.make_loaders(tr.params)
    before = _state(tr)
    scans0 = tr.model.zero_scans
    out = tr.eval_epoch(loaders[1])
    torch.cuda.synchronize()
    scans = tr.model.zero_scans - scans0
    after = _state(tr)
    batches = ER.whole_path_batches("val")
    fused, naive = [], []
    tr.model.eval()
    for k in (0, 1):
        cm = torch.zeros(6, 4, 4, dtype=torch.int64, device=DEV)
        sums = torch.zeros(6, dtype=torch.float64, device=DEV)

        def run():
            tr.model.begin_missing_pass()
            f, n = [], []
            for b in batches:
                dev = _gpu(b)
                tr.to_logits(dev)
                f.append(tr.model.score_missing(dev["label"], cm, sums).clone().reshape(6, -1, 4).cpu())
                n.append(torch.stack([tr.to_logits(_gpu(ER.mask_batch(b, p))).clone() for p in MR.MISSING_TYPES]).cpu())
            return f, n
        if k == 0:
            f, n = run()
        else:
            with tr.ema_weights():
                f, n = run()
        fused.append(f)
        naive.append(n)
    torch.cuda.synchronize()
    plain_tr = _trainer()
    plain = plain_tr.eval_epoch(plain_tr.make_loaders(plain_tr.params)[1])
    return dict(tr=tr, out=out, before=before, after=after, scans=scans, batches=batches, fused=fused, naive=naive, plain=plain)


def test_whole_path_logits_agree_with_the_naive_route_and_float64(whole):
    """per batch (2, 2, 1 utterances, two audio lengths) and pass (model, EMA): fused against naive within twice the whole-model
    logits bound of tests/test_gpu_mmin_miss.py (the float32 twin's deviation from float64, MR.twin_bound), each within that bound
    of float64"""
    assert len({int(b["audio_feature"].shape[1]) for b in whole["batches"]}) >= 2
    for k in (0, 1):
        for i, (f64, f32) in enumerate(ER.whole_path_reference("val", k)):
            bnd = MR.twin_bound(f32, f64)
            f, n = whole["fused"][k][i].double(), whole["naive"][k][i].double()
            scale = float(f64.abs().max())
            figs = (R.rel(f, f64), R.rel(n, f64), float((f - n).abs().max()) / scale)
            print("pass %d batch %d: fused/f64 %.2e  naive/f64 %.2e  (bound %.0e)  fused/naive %.2e (bound %.0e)" % (k, i, *figs[:2], bnd, figs[2], 2 * bnd))
            assert figs[0] <= bnd and figs[1] <= bnd and figs[2] <= 2 * bnd


def test_whole_path_epoch_figures(whole):
    """eval_epoch under the flag: per pattern Lall against the naive route's (the same relative bound), confusion matrices and
    Acc / Acc2 equal to the naive route's and to float64's (the host test vouches for the margins); the full-modality figures
    are those of a run without the flag; no state tensor moved; at most one zero-input scan per pass and audio length"""
    out, plain, labels = whole["out"], whole["plain"], [b["label"] for b in whole["batches"]]
    assert list(out["missing"]) == list(ER.KEYS)
    for key in ("C", "Lall", "Acc", "Acc2", "true", "pred"):
        assert out[key] == plain[key], key
    assert "missing" not in plain
    for a, b in zip(whole["before"], whole["after"]):
        assert torch.equal(a, b), "the evaluation changed a state tensor"
    n_ta = len({int(b["audio_feature"].shape[1]) for b in whole["batches"]})
    print("zero-input scans: %d in 2 passes over %d audio lengths" % (whole["scans"], n_ta))
    assert 2 <= whole["scans"] <= 2 * n_ta
    ref = [ER.whole_path_reference("val", k) for k in (0, 1)]
    bnd = max(MR.twin_bound(f32, f64) for r in ref for f64, f32 in r)
    for c, key in enumerate(ER.KEYS):
        rec = out["missing"][key]
        ce = lambda lg, y: float(torch.nn.functional.cross_entropy(lg.double(), y))
        lall_naive = sum(ce(n[c], y) for n, y in zip(whole["naive"][0], labels))
        lall_64 = sum(ce(f64[c], y) for (f64, _), y in zip(ref[0], labels))
        # the cross entropy moves by at most twice the logits' absolute error
        scale = max(float(f64.abs().max()) for f64, _ in ref[0])
        tol = 2 * bnd * max(lall_naive, 2 * scale * len(labels))
        print("%s: Lall %.6f naive %.6f float64 %.6f (tolerance %.1e)  Acc %.2f Acc2 %.2f" % (key, rec["Lall"], lall_naive, lall_64, tol, rec["Acc"], rec["Acc2"]))
        assert abs(rec["Lall"] - lall_naive) <= 2 * bnd * lall_naive, key
        assert math.isfinite(rec["Lall"]) and abs(rec["Lall"] - lall_64) <= tol
        for k, (cm_key, acc_key) in enumerate((("cm", "Acc"), ("cm2", "Acc2"))):
            cm_naive = sum(_cm_of(n[c].argmax(-1), y) for n, y in zip(whole["naive"][k], labels))
            cm_64 = sum(_cm_of(f64[c].argmax(-1), y) for (f64, _), y in zip(ref[k], labels))
            assert torch.equal(torch.as_tensor(rec[cm_key]), cm_naive) and torch.equal(cm_naive, cm_64), (key, cm_key)
            assert rec[acc_key] == float(cm_naive.diagonal().sum()) / 5 and int(cm_naive.sum()) == out["C"] == 5


def test_two_training_epochs_are_bit_identical_with_and_without_the_flag():
    """train, validate (plateau scheduler), test, twice: parameters, moments, the EMA copy, both dropout counters and the
    pretrained model end bit-identical with --eval_missing and without; so do the full-modality figures of every epoch"""
    from erc_amd import mmin
    res = []
    for extra in ((), ("--eval_missing", )):
        random.seed(3)
        torch.manual_seed(3)
        tr = _trainer(*extra, weights=False)
        loop = mmin.MMINEpochLoop(tr.params, tr, DEV)
        figs = []
        for _ in range(2):
            loop.train_epoch()
            val, test = loop.test_epoch()
            assert ("missing" in val) == ("missing" in test) == bool(extra)
            figs.append([(r["Lall"], r["Acc"], r["Acc2"], r["pred"]) for r in (val, test)])
        torch.cuda.synchronize()
        res.append((_state(tr), figs, loop.ring.clone()))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    assert res[0][1] == res[1][1] and torch.equal(res[0][2], res[1][2])
    assert int(res[0][0][7][0]) == 4       # two epochs of two optimizer steps


def test_cli_one_epoch_with_eval_missing(tmp_path):
    env = dict(os.environ, PYTHONPATH=REPO)
    args = ["--module=mmin_miss", "--eval_missing", "--epoch=1", "--n_train=4", "--n_val=3", "--n_test=5", "--train.batch_size=4",
            "--val.batch_size=2", "--test.batch_size=2", "--mmin_frames=(3,20)", "--log_every=0"]
    res = subprocess.run([sys.executable, os.path.join(REPO, "train_mm.py")] + args, capture_output=True, text=True, env=env, timeout=300,
                         cwd=REPO)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [json.loads(l) for l in res.stdout.strip().splitlines() if l.startswith("{")][-1]
    assert set(line["val"]) == set(line["test"]) == {"Lall", "Acc", "Acc2"} and list(line["missing"]) == ["val", "test"]
    for split, n in (("val", 3), ("test", 5)):
        entries = line["missing"][split]
        assert list(entries) == list(ER.KEYS)
        for key, e in entries.items():
            assert math.isfinite(e["Lall"]) and 0.0 <= e["Acc"] <= 1.0 and 0.0 <= e["Acc2"] <= 1.0
            assert e["C"] == n == sum(sum(row) for row in e["report"]["cm"]), (split, key)
            assert all(math.isfinite(v) for k, v in e["report"].items() if k != "cm")
