"""GPU: ``--module=mmin_base`` under missing modalities (``--eval_missing``, ``--train_missing``).  The four new launches through the
C-ABI -- erc_mmin_collate_masked against its torch restatement (tests/mmin_base_missing_ref.py), erc_lstm128_prefix_max against
per-length zero-input scans bit for bit, erc_mmin_miss_expand_cap and erc_mmin_miss_score_cap against the exact forms bit for bit
-- the default-loop evaluation against the naive route (six more passes of the unchanged forward over host-masked batches) and the
float64 restatement, the resident evaluation against the default loop's, a masked bucket step and masked resident epochs against
their exact-shape / bucketed counterparts, and the command line.  Every test prints its figures before it asserts."""
import contextlib
import math
import random

import numpy as np
import pytest
import torch

from erc_amd import capi
from tests import mmin_base_missing_ref as BR
from tests import mmin_cap_ref as CR
from tests import mmin_eval_missing_ref as ER
from tests import mmin_miss_ref as MR
from tests import mmin_ref as R
from tests import test_gpu_mmin_capacity as TC

pytestmark = pytest.mark.gpu
DEV = TC.DEV
H, EMB, GUARD, SENT, TV, TT = TC.H, TC.EMB, TC.GUARD, TC.SENT, TC.TV, TC.TT
_buf, _bits, _guard_intact = TC._buf, TC._bits, TC._guard_intact
ALL_BITS = (1, 2, 4, 3, 5, 6, 7, 0)          # the six patterns of MISSING_TYPES, everything kept, nothing kept


@pytest.fixture(scope="module", autouse=True)
def _lib():
    capi.lib()


# ------------------------------------------------------------------------------------------------- erc_mmin_collate_masked
class _MaskedOut(TC._CollateOut):
    def run(self, store, desc, frames_max=None, masked=True):
        d = torch.as_tensor(desc, dtype=torch.int32).to(DEV)
        capi.mmin_collate(d, store.audio, store.visual, store.text, store.label, self.B_cap, self.T_cap,
                          self.T_cap if frames_max is None else frames_max, self.audio, self.visual, self.text, self.label, self.counts,
                          masked=masked)
        torch.cuda.synchronize()

    def snapshot(self):
        return [t.clone() for t in (self.audio, self.visual, self.text, self.label, self.counts)]

    def check_masked(self, store, desc):
        """bit for bit on kept rows, by value on masked rows (the host path's x * 0 may be -0.0; the restatement writes 0.0 as
        the kernel does, so masked rows are compared by value AND found to be +0.0), guard rows intact"""
        B, T = self.B_cap, self.T_cap
        a, v, t, y, c = BR.collate_masked_ref(store, desc, B, T)
        ma, mv, mt = BR.masked_rows(desc, B)
        for name, buf, ref, rows_per, gone in (("audio", self.audio, a, T, ma), ("visual", self.visual, v, TV, mv), ("text", self.text, t, TT, mt)):
            got = buf[:B * rows_per].reshape(B, rows_per, -1).cpu()
            assert torch.equal(got, ref), name
            assert _bits(got[~gone], ref[~gone]), name + ": kept rows"
            assert not got[gone].any(), name + ": masked rows"
            assert _guard_intact(buf, B * rows_per), name + ": guard rows"
        assert _bits(self.label[:B], y.reshape(B, 1)) and _bits(self.counts[:2], c.reshape(2, 1))
        assert _guard_intact(self.label, B) and _guard_intact(self.counts, 2)
        return c.tolist()


def _desc4(desc3, bits, B_cap):
    return torch.cat([torch.as_tensor(desc3, dtype=torch.int32).reshape(-1), torch.tensor(list(bits), dtype=torch.int32)])


@pytest.mark.parametrize("name", sorted(TC.COLLATE_CASES))
def test_collate_masked(name):
    frames, B_cap, T_cap, slots = TC.COLLATE_CASES[name]
    store = TC._device_store(frames)
    desc3 = TC._desc_of(store, slots, B_cap)
    plain = TC._CollateOut(B_cap, T_cap)
    plain.run(store, desc3)
    out, seen = _MaskedOut(B_cap, T_cap), set()
    for r in range(-(-len(ALL_BITS) // B_cap)):
        bits = [ALL_BITS[(r * B_cap + b) % len(ALL_BITS)] for b in range(B_cap)]
        seen |= set(bits)
        desc = _desc4(desc3, [v + 8 * (b % 2) for b, v in enumerate(bits)], B_cap)       # a bit beyond the three: masked off on the device
        out.run(store, desc)
        counts = out.check_masked(store, desc)
        first = out.snapshot()
        out.run(store, desc)
        assert all(_bits(x, y) for x, y in zip(first, out.snapshot())), "a second launch differs"
        assert _bits(out.counts, plain.counts) and _bits(out.label, plain.label), "counts / labels look at the keep bits"
        print("collate_masked %s bits %s: counts %s (unmasked kernel: %s)" % (name, bits, counts, plain.counts[:2, 0].tolist()))
    assert seen == set(ALL_BITS)
    out.run(store, _desc4(desc3, [7] * B_cap, B_cap))
    for x, y in zip(out.snapshot(), (plain.audio, plain.visual, plain.text, plain.label, plain.counts)):
        assert _bits(x, y), "all bits set differs from erc_mmin_collate"


def test_collate_masked_stale_rows_and_clamps():
    """a long unmasked batch, then a short masked one into the same buffers: nothing of the first survives; a wild descriptor is
    clamped as the restatement clamps it"""
    store = TC._device_store((16, 1, 7, 3, 12))
    out = _MaskedOut(4, 16)
    long_ = _desc4(TC._desc_of(store, (0, 4, 2, 3), 4), (7, 7, 7, 7), 4)
    out.run(store, long_)
    assert out.check_masked(store, long_) == [4, 16]
    short = _desc4(TC._desc_of(store, (1, 3, None, None), 4), (3, 4, 7, 7), 4)
    out.run(store, short)
    assert out.check_masked(store, short) == [2, 3]
    masked_long = _desc4(TC._desc_of(store, (0, 4, 2, 3), 4), (3, 5, 6, 0), 4)           # counts[1] = 16 though slot 0's audio is removed
    out.run(store, masked_long)
    assert out.check_masked(store, masked_long) == [4, 16]
    n_frames = int(store.audio.shape[0])
    wild = torch.tensor([40, -3, 5, 16, n_frames - 2, 7, -9, 10 ** 6, 99, 0, -1, 2, -1, 6, 1, 2 ** 20 + 5], dtype=torch.int32)
    out.run(store, wild)
    assert out.check_masked(store, wild) == [3, 16]


def test_collate_masked_refusals():
    store = TC._device_store((4, 2))
    out = _MaskedOut(2, 8)
    desc = _desc4(TC._desc_of(store, (0, 1), 2), (5, 6), 2).to(DEV)
    args = lambda **kw: {**dict(desc=desc, store_audio=store.audio, store_visual=store.visual, store_text=store.text, store_label=store.label,
                                B_cap=2, T_cap=8, frames_max=8, audio=out.audio, visual=out.visual, text=out.text, label=out.label,
                                counts=out.counts, masked=True), **kw}
    for kw in (dict(frames_max=9), dict(B_cap=0), dict(B_cap=-1), dict(desc=None), dict(audio=None), dict(counts=None), dict(store_audio=None),
               dict(store_label=None), dict(T_cap=0), dict(desc=desc[:6])):
        with pytest.raises(capi.ErcGraftError, match="mmin_collate_masked"):
            capi.mmin_collate(**args(**kw))
    torch.cuda.synchronize()
    for buf in (out.audio, out.visual, out.text, out.label, out.counts):
        assert _guard_intact(buf, 0)


# --------------------------------------------------------------------------------------------------- the whole-path trainer
def _gpu(batch):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _whole_trainer(*extra):
    """seeded weights the host test vouches for; the EMA copy gets a set of its own, so that the two passes differ"""
    tr = TC._trainer("--val.batch_size=2", *extra)
    tr.model.load_state_dict(BR.whole_weights(0), strict=True)
    for k, v in BR.whole_weights(1).items():
        tr.model.flat.view(tr.ema, k).copy_(v.to(DEV))
    return tr


def _loader(samples, batch_size):
    from torch.utils.data import DataLoader
    from erc_amd.mmin import mmin_collate
    return DataLoader(samples, batch_size=batch_size, shuffle=False, collate_fn=mmin_collate)


def _state(tr):
    f = tr.model.flat
    return [t.clone() for t in (f.data, f.exp_avg, f.exp_avg_sq, tr.ema, tr.optim.state, tr.model.rng_state)]


# -------------------------------------------------------------------------------------------------- erc_lstm128_prefix_max
def test_prefix_max_table_carries_the_bits_of_per_length_zero_scans():
    tr = _whole_trainer()
    model, t_max = tr.model, BR.T_MAX_TABLE
    model.eval()
    scans0 = model.zero_scans
    tab = model.zero_table(t_max, TV, TT, DEV)
    assert model.zero_scans == scans0 + 1 and tuple(tab["zaudio"].shape) == (t_max + 1, H) and tuple(tab["zvt"].shape) == (2 * H, )
    zeros = lambda T, d: torch.zeros(1, T, d, device=DEV)
    for Ta in BR.TABLE_TA:
        want = model._zero_encode(zeros(Ta, CR.AUDIO_D), None, None)[:H].clone()
        print("prefix max Ta=%d: bit-equal %s, max |diff| %.3g" % (Ta, _bits(tab["zaudio"][Ta], want), float((tab["zaudio"][Ta] - want).abs().max())))
        assert _bits(tab["zaudio"][Ta], want)
    vt = model._zero_encode(None, zeros(TV, CR.VISUAL_D), zeros(TT, CR.TEXT_D))[H:].clone()
    assert _bits(tab["zvt"], vt) and bool((tab["zaudio"][0] == 0).all())
    with R.one_thread():
        ref = BR.prefix_table(BR.whole_weights(0), t_max)
    err = R.rel(tab["zaudio"][1:].cpu().double(), ref[1:])
    print("prefix max table against float64: %.2e" % err)
    assert err <= 1e-5
    # the write set is the table alone; a second launch gives the same bits
    hp = model._zero_encode_ws(zeros(t_max + 1, CR.AUDIO_D), None, None)["A"]["Hprev"]
    keep, out = hp.clone(), _buf(t_max + 1, H)
    capi.lstm128_prefix_max(hp, t_max + 1, out)
    first = out.clone()
    capi.lstm128_prefix_max(hp, t_max + 1, out)
    torch.cuda.synchronize()
    assert _bits(out[:t_max + 1], tab["zaudio"]) and _bits(out, first) and _guard_intact(out, t_max + 1) and _bits(hp, keep)
    fresh = _buf(t_max + 1, H)
    for bad in (dict(Hprev=None), dict(out=None), dict(t_rows=1), dict(t_rows=0), dict(out=hp)):
        kw = dict(dict(Hprev=hp, t_rows=t_max + 1, out=fresh), **bad)
        with pytest.raises(capi.ErcGraftError, match="lstm128_prefix_max"):
            capi.lstm128_prefix_max(kw["Hprev"], kw["t_rows"], kw["out"])
    torch.cuda.synchronize()
    assert _guard_intact(fresh, 0) and _bits(hp, keep)


# ------------------------------------------------------------------------------------------------ erc_mmin_miss_expand_cap
@pytest.mark.parametrize("counts", [(2, 7), (3, 16), (3, 0), (1, 99)])
def test_miss_expand_cap_carries_the_bits_of_the_exact_form(counts):
    B_cap, t_rows, K = 3, 17, 6
    g = torch.Generator().manual_seed(60 + counts[1])
    feat = _buf(B_cap, EMB + 4)
    feat[:B_cap, :EMB] = torch.randn(B_cap, EMB, generator=g).to(DEV)
    zaudio, zvt = torch.randn(t_rows, H, generator=g).to(DEV), torch.randn(2 * H, generator=g).to(DEV)
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    pat = capi.mmin_miss_patterns(MR.MISSING_TYPES)
    out = _buf(K * B_cap, EMB + 8)
    capi.mmin_miss_expand_cap(feat, EMB + 4, zaudio, t_rows, zvt, cnt, pat, B_cap, out, EMB + 8)
    Bdev, Ta = min(max(counts[0], 0), B_cap), min(max(counts[1], 1), t_rows - 1)
    exact = _buf(K * Bdev, EMB)
    capi.mmin_miss_expand(feat, EMB + 4, torch.cat([zaudio[Ta], zvt]), pat, Bdev, exact, EMB)
    torch.cuda.synchronize()
    got = out[:K * B_cap, :EMB].reshape(K, B_cap, EMB)
    print("miss_expand_cap counts %s -> Bdev %d, table row %d: rows bit-equal %s" % (counts, Bdev, Ta, _bits(got[:, :Bdev], exact[:K * Bdev].reshape(K, Bdev, EMB))))
    assert _bits(got[:, :Bdev], exact[:K * Bdev].reshape(K, Bdev, EMB))
    assert bool(torch.isfinite(got).all()) and not bool((got == SENT).any()), "tail rows"
    assert bool((out[K * B_cap:] == SENT).all()) and bool((out[:K * B_cap, EMB:] == SENT).all()), "guard rows / pad columns were written"


def test_miss_expand_cap_refuses_bad_arguments_without_a_launch():
    B, D = 3, EMB
    feat, za, zvt, out = torch.ones(B, D, device=DEV), torch.ones(5, H, device=DEV), torch.ones(2 * H, device=DEV), _buf(6 * B, D)
    cnt, pat = torch.tensor([3, 2], dtype=torch.int32, device=DEV), capi.mmin_miss_patterns(MR.MISSING_TYPES)
    ok = dict(feat=feat, ldf=D, za=za, t_rows=5, zvt=zvt, cnt=cnt, pat=pat, B=B, out=out, ldo=D)
    off = torch.full((6 * B * D + 4, ), SENT, device=DEV)
    for bad in (dict(cnt=None), dict(t_rows=1), dict(t_rows=0), dict(feat=None), dict(za=None), dict(zvt=None), dict(out=None), dict(pat=None),
                dict(B=0), dict(B=-1), dict(ldf=D - 4), dict(ldo=D - 4), dict(ldf=D + 1), dict(ldo=D + 2), dict(out=off[1:]), dict(za=off[1:]),
                dict(zvt=off[1:]), dict(feat=off[3:]), dict(pat=capi.mmin_miss_patterns(MR.MISSING_TYPES * 2)), dict(pat=(capi.C.c_int32 * 1)(8)),
                dict(pat=(capi.C.c_int32 * 1)(-1))):
        kw = dict(ok, **bad)
        with pytest.raises(capi.ErcGraftError, match="mmin_miss_expand_cap"):
            capi.mmin_miss_expand_cap(kw["feat"], kw["ldf"], kw["za"], kw["t_rows"], kw["zvt"], kw["cnt"], kw["pat"], kw["B"], kw["out"], kw["ldo"])
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((off == SENT).all()), "a refused call wrote"


# ------------------------------------------------------------------------------------------------- erc_mmin_miss_score_cap
@pytest.mark.parametrize("Bdev", [0, 1, 3, 5])
def test_miss_score_cap_carries_the_bits_of_the_exact_form(Bdev):
    """B_cap = 5, C = 4, six blocks: a label out of range, a row of nothing but NaN; the tail (b >= Bdev) is poisoned -- label 0
    and logits of NaN, every other tail row with one finite entry so that a kernel that read it WOULD count it; both accumulators
    start non-zero (added-to semantics)"""
    B_cap, C, K, pad = 5, 4, 6, 3
    g = torch.Generator().manual_seed(77)
    logits = torch.randn(K, B_cap, C, generator=g)
    labels = torch.randint(0, C, (B_cap, ), generator=g)
    labels[2] = C + 3                                      # out of range: never counted, in every block
    logits[1, 1] = float("nan")                            # never counted
    logits[3, 0, 1] = logits[3, 0, 2] = 9.0                # a tie: the first index
    logits[:, Bdev:] = float("nan")
    logits[:, Bdev:][:, 1::2, 1] = 50.0
    labels[Bdev:] = 0
    lg = _buf(K * B_cap, C + pad)
    lg[:K * B_cap, :C] = logits.reshape(K * B_cap, C).to(DEV)
    cnt = torch.tensor([Bdev if Bdev else -2, 9], dtype=torch.int32, device=DEV)
    start = lambda: (torch.full((K * C * C + 8, ), 3, dtype=torch.int64, device=DEV), torch.full((K + 2, ), 1.5, dtype=torch.float64, device=DEV))
    (cm, sums), (cm_b, sums_b), (cm_x, sums_x) = start(), start(), start()
    before = lg.clone()
    capi.mmin_miss_score_cap(lg, C + pad, labels.to(DEV), B_cap, cnt, K, C, cm, sums)
    capi.mmin_miss_score_cap(lg, C + pad, labels.to(DEV), B_cap, cnt, K, C, cm_b, sums_b)
    if Bdev:
        rows = logits[:, :Bdev].reshape(K * Bdev, C).contiguous().to(DEV)
        capi.mmin_miss_score(rows, C, labels[:Bdev].to(DEV), Bdev, K, C, cm_x, sums_x)
    torch.cuda.synchronize()
    want_cm, want_loss = ER.score(logits[:, :Bdev].reshape(K * Bdev, C), labels[:Bdev], K) if Bdev else (torch.zeros(K, C, C, dtype=torch.int64),
                                                                                                        torch.zeros(K, dtype=torch.float64))
    got_cm = cm[:K * C * C].reshape(K, C, C).cpu() - 3
    err = float((sums[:K].cpu() - 1.5 - want_loss).abs().max())
    print("miss_score_cap Bdev=%d: counted %d rows, cm bit-equal to the exact form %s, loss_sum bit-equal %s, |loss - float64| %.2e"
          % (Bdev, int(got_cm.sum()), _bits(cm, cm_x), _bits(sums, sums_x), err))
    assert _bits(cm, cm_x) and _bits(sums, sums_x), "differs from erc_mmin_miss_score at B = Bdev"
    assert _bits(cm, cm_b) and _bits(sums, sums_b), "a second run differs"
    assert torch.equal(got_cm, want_cm) and err <= 1e-12 and bool(torch.isfinite(sums).all())
    assert int(got_cm.sum()) == sum(1 for c in range(K) for b in range(Bdev) if b != 2 and not (c == 1 and b == 1))
    assert bool((cm[K * C * C:] == 3).all()) and bool((sums[K:] == 1.5).all())
    assert torch.equal(lg.isnan(), before.isnan()) and torch.equal(lg.nan_to_num(), before.nan_to_num())


def test_miss_score_cap_refuses_bad_arguments_without_a_launch():
    B, C = 4, 4
    lg, y = torch.zeros(6 * B, C, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV)
    cm, sums = torch.zeros(6, C, C, dtype=torch.int64, device=DEV), torch.zeros(6, dtype=torch.float64, device=DEV)
    cnt = torch.tensor([B, 3], dtype=torch.int32, device=DEV)
    ok = dict(lg=lg, ld=C, y=y, B=B, cnt=cnt, n=6, C=C, cm=cm, s=sums)
    for bad in (dict(cnt=None), dict(lg=None), dict(y=None), dict(cm=None), dict(s=None), dict(B=0), dict(n=0), dict(n=9), dict(C=0),
                dict(C=17, ld=17), dict(ld=C - 1)):
        kw = dict(ok, **bad)
        with pytest.raises(capi.ErcGraftError, match="mmin_miss_score_cap"):
            capi.mmin_miss_score_cap(kw["lg"], kw["ld"], kw["y"], kw["B"], kw["cnt"], kw["n"], kw["C"], kw["cm"], kw["s"])
    torch.cuda.synchronize()
    assert int(cm.abs().sum()) == 0 and float(sums.abs().sum()) == 0.0


# --------------------------------------------------------------------------------------------- default loop, --eval_missing
def _cm_of(pred, labels, C=4):
    cm = torch.zeros(C, C, dtype=torch.int64)
    for y, p in zip(labels.tolist(), pred.tolist()):
        cm[y, p] += 1
    return cm


def _routes(tr, batches, t_max):
    """per pass (model, EMA): the fused and the naive logits of every batch, [6, B, C] on the host"""
    fused, naive = [], []
    tr.model.eval()
    for k in (0, 1):
        cm = torch.zeros(6, 4, 4, dtype=torch.int64, device=DEV)
        sums = torch.zeros(6, dtype=torch.float64, device=DEV)
        with (tr.ema_weights() if k else contextlib.nullcontext()):
            tr.model.begin_missing_pass(t_max)
            f, n = [], []
            for b in batches:
                dev = _gpu(b)
                tr.to_logits(dev)
                f.append(tr.model.score_missing(dev["label"], cm, sums).clone().reshape(6, -1, 4).cpu())
                n.append(torch.stack([tr.to_logits(_gpu(ER.mask_batch(b, p))).clone() for p in MR.MISSING_TYPES]).cpu())
        fused.append(f)
        naive.append(n)
    tr.model.begin_missing_pass()
    return fused, naive


@pytest.fixture(scope="module")
def whole():
    """one evaluation of the five utterances with the flag (both passes), the per-batch fused and naive logits of both passes,
    and the same evaluation without the flag; shared by the tests below, never modified"""
    tr = _whole_trainer("--eval_missing")
    loader = _loader(BR.whole_samples(), BR.WHOLE_BATCH)
    before, scans0 = _state(tr), tr.model.zero_scans
    out = tr.eval_epoch(loader)
    torch.cuda.synchronize()
    scans, after = tr.model.zero_scans - scans0, _state(tr)
    batches = BR.whole_batches()
    fused, naive = _routes(tr, batches, max(BR.WHOLE_FRAMES))
    torch.cuda.synchronize()
    plain_tr = _whole_trainer()
    plain_before = _state(plain_tr)
    plain = plain_tr.eval_epoch(loader)
    torch.cuda.synchronize()
    return dict(out=out, before=before, after=after, scans=scans, batches=batches, fused=fused, naive=naive, plain=plain,
                plain_state=(plain_before, _state(plain_tr)))


def test_eval_missing_logits_agree_with_float64(whole):
    """per batch (2, 2, 1 utterances, three audio lengths) and pass (model, EMA): the fused logits within the recorded bound of
    the float64 restatement (4 x the float32 twin's worst deviation, tests/mmin_base_missing_ref.py), the naive route's too"""
    bnd, worst = BR.logits_bound(), 0.0
    assert len({int(b["audio_feature"].shape[1]) for b in whole["batches"]}) == 3
    for k in (0, 1):
        for i, (f64, _) in enumerate(BR.whole_reference(k)):
            f, n = whole["fused"][k][i].double(), whole["naive"][k][i].double()
            figs = (R.rel(f, f64), R.rel(n, f64), float((f - n).abs().max()) / float(f64.abs().max()))
            worst = max(worst, figs[0])
            print("pass %d batch %d: fused/f64 %.2e  naive/f64 %.2e  fused/naive %.2e  (bound %.2e)" % (k, i, *figs, bnd))
            assert figs[0] <= bnd and figs[1] <= bnd
    print("worst fused deviation %.3g (recorded: %s)" % (worst, BR.FIGURES[("eval_missing", "logits")][2]))


def test_eval_missing_epoch_figures(whole):
    """eval_epoch under the flag: per pattern the confusion matrices, Acc and Acc2 equal the naive route's and float64's (the
    host test vouches for the margins), Lall equals the naive route's up to the logits bound (each route's logits lie within
    ``bnd`` x the largest logit of float64, a cross entropy moves by at most twice its logits' error, Lall adds one batch mean per
    batch); the full-modality figures and every state tensor are those of a run without the flag; one zero-input scan per pass"""
    out, plain, labels = whole["out"], whole["plain"], [b["label"] for b in whole["batches"]]
    assert list(out["missing"]) == list(BR.KEYS) and "missing" not in plain
    for key in ("C", "Lall", "Acc", "Acc2", "true", "pred"):
        assert out[key] == plain[key], key
    for a, b in zip(whole["before"], whole["after"]):
        assert _bits(a, b), "the evaluation changed a state tensor"
    for a, b in zip(whole["after"], whole["plain_state"][1]):
        assert _bits(a, b), "a state tensor differs from the run without the flag"
    print("zero-input scans: %d in 2 passes over 3 audio lengths" % whole["scans"])
    assert whole["scans"] == 2
    ref = [BR.whole_reference(k) for k in (0, 1)]
    bnd = BR.logits_bound()
    scale = max(float(f64.abs().max()) for f64, _ in ref[0])
    tol = len(labels) * 2 * (2 * bnd * scale)
    ce = lambda lg, y: float(torch.nn.functional.cross_entropy(lg.double(), y))
    for c, key in enumerate(BR.KEYS):
        rec = out["missing"][key]
        lall_naive = sum(ce(n[c], y) for n, y in zip(whole["naive"][0], labels))
        lall_64 = sum(ce(f64[c], y) for (f64, _), y in zip(ref[0], labels))
        print("%s: Lall %.7f naive %.7f float64 %.7f (tolerance %.1e)  Acc %.2f Acc2 %.2f" % (key, rec["Lall"], lall_naive, lall_64, tol, rec["Acc"], rec["Acc2"]))
        assert math.isfinite(rec["Lall"]) and abs(rec["Lall"] - lall_naive) <= tol and abs(rec["Lall"] - lall_64) <= tol
        for k, (cm_key, acc_key) in enumerate((("cm", "Acc"), ("cm2", "Acc2"))):
            cm_naive = sum(_cm_of(n[c].argmax(-1), y) for n, y in zip(whole["naive"][k], labels))
            cm_64 = sum(_cm_of(f64[c].argmax(-1), y) for (f64, _), y in zip(ref[k], labels))
            assert torch.equal(torch.as_tensor(rec[cm_key]), cm_naive) and torch.equal(cm_naive, cm_64), (key, cm_key)
            assert rec[acc_key] == float(cm_naive.diagonal().sum()) / 5 and int(cm_naive.sum()) == out["C"] == 5


# ------------------------------------------------------------------------------------------ --resident_eval --eval_missing
def test_resident_eval_missing_equals_the_default_loop():
    """a 7-sample split at B = 4 after three training steps: all twelve matrices equal the default-loop route's, every Lall lies
    within the bound of tests/mmin_cap_ref.lall_reference of the float64 cross entropy of the default loop's fused logits, a second
    epoch (all replays) returns the same, and nothing of the trainer's state moves"""
    from erc_amd.datasets import MMINDeviceStore
    from erc_amd.mmin import MMINResidentEval
    tr = TC._trainer("--device_collate", "--resident", "--resident_eval", "--eval_missing", t_cap=150)
    for n in range(3):
        tr.train_step(tr.prepare_batch(TC._host_batch((20, 6, 9, 14), 40 + n)))
    samples = TC._split(7, 33, "val")
    loader = _loader(samples, 4)
    host = tr.eval_epoch(loader)
    batches = list(loader)
    fused, _ = _routes_fused_only(tr, batches)
    tr.model.train()
    before = _state(tr)
    ev = MMINResidentEval(tr, MMINDeviceStore(samples, DEV), 4)
    scans0 = tr.model.zero_scans
    out = ev.epoch()
    scans = tr.model.zero_scans - scans0
    again = ev.epoch()
    torch.cuda.synchronize()
    assert tr.model.training and not tr.model.dynamic_n and tr._swap is None
    for a, b in zip(before, _state(tr)):
        assert _bits(a, b)
    assert list(out["missing"]) == list(BR.KEYS) and scans == 2
    np.testing.assert_array_equal(out["cm"], _cm_np(host))
    assert out["Acc"] == host["Acc"] and out["Acc2"] == host["Acc2"] and out["C"] == 7
    labels = [b["label"] for b in batches]
    for c, key in enumerate(BR.KEYS):
        got, want = out["missing"][key], host["missing"][key]
        l64, l32, bound = CR.lall_reference([f[c] for f in fused], labels)
        print("resident eval %s: Lall %.9g default loop %.9g float64 %.9g |diff| %.3g bound %.3g; Acc %.4f Acc2 %.4f"
              % (key, got["Lall"], want["Lall"], l64, abs(got["Lall"] - l64), bound, got["Acc"], got["Acc2"]))
        np.testing.assert_array_equal(got["cm"], want["cm"])
        np.testing.assert_array_equal(got["cm2"], want["cm2"])
        assert int(got["cm"].sum()) == int(got["cm2"].sum()) == 7 and got["Acc"] == want["Acc"] and got["Acc2"] == want["Acc2"]
        assert abs(got["Lall"] - l64) <= bound
        assert again["missing"][key]["Lall"] == got["Lall"]
        assert np.array_equal(again["missing"][key]["cm"], got["cm"]) and np.array_equal(again["missing"][key]["cm2"], got["cm2"])
    assert again["Lall"] == out["Lall"] and np.array_equal(again["cm"], out["cm"]) and np.array_equal(again["cm2"], out["cm2"])
    assert ev.eager == ev.captures == len(set(ev.caps)) and ev.replays == 4 * len(ev.caps) - ev.eager


def _cm_np(r):
    return np.bincount(np.asarray(r["true"]) * 4 + np.asarray(r["pred"]), minlength=16).reshape(4, 4)


def _routes_fused_only(tr, batches):
    """the model pass's fused logits per batch, [6, B, C] on the host"""
    tr.model.eval()
    cm, sums = torch.zeros(6, 4, 4, dtype=torch.int64, device=DEV), torch.zeros(6, dtype=torch.float64, device=DEV)
    tr.model.begin_missing_pass(max(int(b["audio_feature"].shape[1]) for b in batches))
    out = []
    for b in batches:
        dev = _gpu(b)
        tr.to_logits(dev)
        out.append(tr.model.score_missing(dev["label"], cm, sums).clone().reshape(6, -1, 4).cpu())
    tr.model.begin_missing_pass()
    return out, (cm, sums)


# ---------------------------------------------------------------------------------------------------------- --train_missing
def _masked_host_batch(frames, seed, types):
    from erc_amd.mmin import mask_collate
    samples = CR.samples_with_frames(frames, seed=seed, tv=TV, tt=TT)
    return mask_collate([dict(s, missing_type=list(t)) for s, t in zip(samples, types)])


def test_masked_bucket_step_equals_the_exact_shape_step_after_a_larger_batch():
    """test_bucket_step_equals_the_exact_shape_step_after_a_larger_batch's criterion on host-masked batches: #correct equal, loss
    within 1e-4, every gradient within 1e-3 of its largest entry"""
    T = MR.MISSING_TYPES
    tr = TC._trainer("--capacity_buckets=True", "--train_missing", dropout=False)
    small = tr.prepare_batch(_masked_host_batch(TC.SMALL, 1, (T[0], T[2], T[4])))
    big = tr.prepare_batch(_masked_host_batch(TC.BIG, 2, (T[1], T[3], T[5], T[2])))
    assert not small["audio_feature"][0].any() and small["audio_feature"][1].any() and not small["text_feature"][0].any()
    key, make, fill = tr.capacity_bucket(small)
    assert key == ("capacity", 4, 16, TV, TT)
    static = make()
    exact = tr.model.loss_and_grads(small).clone()
    torch.cuda.synchronize()
    want = TC._grads(tr)
    TC._bucket_step(tr, static, fill, big)
    stats = TC._bucket_step(tr, static, fill, small)
    ws = tr.model._last_ws
    assert ws["counts"].tolist() == [3, 11]
    d_loss, worst = abs(float(stats[0]) - float(exact[0])), 0.0
    for k, g in want.items():
        got = tr.model.flat.g(k)
        scale = float(g.abs().max()) + 1e-6
        e = float((got - g).abs().max())
        worst = max(worst, e / scale)
        assert torch.isfinite(got).all() and e <= 1e-3 * scale, (k, e, scale)
    print("mmin masked bucket vs exact: #correct %d / %d, |loss diff| = %.3g, worst gradient deviation %.3g of the largest entry"
          % (float(stats[1]), float(exact[1]), d_loss, worst))
    assert float(stats[1]) == float(exact[1]) and 0 <= float(stats[1]) <= 3
    assert torch.isfinite(exact[0]) and d_loss <= 1e-4


def test_masked_resident_epochs_equal_the_bucketed_loop():
    """two epochs of 10 samples at B = 4 from the device store -- 4 B int32 (the keep bits drawn on the host) and one replay per
    step -- against StepGraphs over the masked DataLoader from the same generator and ``random`` state:
    test_resident_epochs_equal_the_bucketed_loop's criterion (per-epoch loss sums within 4e-4, #correct equal).  Whether the
    parameters end bit-equal is printed"""
    from torch.utils.data import DataLoader
    from erc_amd.datasets import MMINMaskedDeviceStore
    from erc_amd.mmin import MMINResidentEpochs, _Transformed, mask_collate
    from erc_amd.mmin_miss import Missing
    from erc_amd.trainer import StepGraphs, train_epoch_loader
    samples, ends = TC._split(10, 21), []
    for mode in ("resident", "bucketed"):
        tr = TC._trainer("--capacity_buckets=True", "--train_missing", t_cap=max(s["audio_feature"].shape[0] for s in samples))
        gen, sums = torch.Generator().manual_seed(5), []
        random.seed(77)
        if mode == "resident":
            res = MMINResidentEpochs(tr, MMINMaskedDeviceStore(samples, DEV), 4, gen)
            prev = torch.zeros(4, dtype=torch.float64)
            for _ in range(2):
                assert res.epoch() == [4, 4, 2]
                acc = res.acc.cpu()
                sums.append((acc - prev)[:2].tolist())
                prev = acc
            assert res.replays > 0 and res.eager == res.captures <= 3 and res.replays + res.eager == 6
        else:
            loader = DataLoader(_Transformed(samples, Missing()), batch_size=4, shuffle=True, collate_fn=mask_collate, generator=gen)
            g, ring = StepGraphs(tr), torch.zeros(3, 4, device=DEV)
            for _ in range(2):
                assert train_epoch_loader(loader, g, tr, ring) == [4, 4, 2]
                sums.append(ring.double().sum(0)[:2].cpu().tolist())
            assert g.replays > 0 and g.eager == g.captures <= 3
        torch.cuda.synchronize()
        assert not tr.model.dynamic_n
        ends.append((tr.model.flat.data.clone(), tr.ema.clone(), sums, random.random()))
    (p_res, e_res, s_res, r_res), (p_buc, e_buc, s_buc, r_buc) = ends
    print("mmin masked resident vs bucketed: epoch {loss sum, #correct} %s vs %s, max |dp| = %.3g, parameters bit-equal: %s, EMA bit-equal: %s"
          % (s_res, s_buc, float((p_res - p_buc).abs().max()), _bits(p_res, p_buc), _bits(e_res, e_buc)))
    assert r_res == r_buc, "the two loops consumed ``random`` differently"
    for a, b in zip(s_res, s_buc):
        assert all(map(lambda v: v == v and abs(v) < 1e30, a)) and abs(a[0] - b[0]) <= 4e-4 and a[1] == b[1]


# -------------------------------------------------------------------------------------------------------------------- CLI
CLI = ["--module=mmin_base", "--epoch=1", "--n_train=8", "--n_val=5", "--n_test=3", "--train.batch_size=4", "--val.batch_size=2",
       "--test.batch_size=2", "--mmin_frames=5,40", "--log_every=0"]
RESIDENT = ["--device_collate", "--resident", "--resident_eval"]


def _check_missing(line):
    assert set(line["val"]) == set(line["test"]) == {"Lall", "Acc", "Acc2"} and list(line["missing"]) == ["val", "test"]
    for split, n in (("val", 5), ("test", 3)):
        entries = line["missing"][split]
        assert list(entries) == list(BR.KEYS)
        for key, e in entries.items():
            assert math.isfinite(e["Lall"]) and 0.0 <= e["Acc"] <= 1.0 and 0.0 <= e["Acc2"] <= 1.0
            assert e["C"] == n == sum(sum(row) for row in e["report"]["cm"]), (split, key)


def test_cli_eval_missing_in_the_default_loop():
    with_flag = TC._epoch_lines(TC._cli(*CLI, "--eval_missing"))
    without = TC._epoch_lines(TC._cli(*CLI))
    assert len(with_flag) == len(without) == 1
    assert set(without[0]) == TC.OLD_KEYS and set(with_flag[0]) == TC.OLD_KEYS | {"missing"}
    _check_missing(with_flag[0])
    for k in ("val", "test", "report", "best_acc", "lr"):
        assert with_flag[0][k] == without[0][k], k          # the full-modality figures are those of the run without the flag
    print("mmin_base cli --eval_missing: %s" % {k: (v["Acc"], v["C"]) for k, v in with_flag[0]["missing"]["val"].items()})


def test_cli_eval_missing_from_hbm():
    with_flag = TC._epoch_lines(TC._cli(*CLI, *RESIDENT, "--eval_missing"))
    without = TC._epoch_lines(TC._cli(*CLI, *RESIDENT))
    assert set(without[0]) == TC.OLD_KEYS | TC.COUNTERS and set(with_flag[0]) == TC.OLD_KEYS | TC.COUNTERS | {"missing"}
    _check_missing(with_flag[0])
    for k in ("val", "test", "report", "best_acc", "lr"):
        assert with_flag[0][k] == without[0][k], k
    print("mmin_base cli resident --eval_missing: %s" % {k: (v["Acc"], v["C"]) for k, v in with_flag[0]["missing"]["test"].items()})


def test_cli_train_missing_from_hbm_and_the_refusal():
    lines = TC._epoch_lines(TC._cli(*[a for a in CLI if a != "--epoch=1"], "--epoch=2", "--train_missing", "--device_collate", "--resident"))
    assert [ln["epoch"] for ln in lines] == [0, 1] and all(set(ln) == TC.OLD_KEYS | TC.COUNTERS for ln in lines)
    assert lines[1]["graph_replays"] > 0 and all(math.isfinite(ln["val"]["Lall"]) for ln in lines)
    print("mmin_base cli --train_missing resident: %s" % {k: lines[1][k] for k in sorted(TC.COUNTERS)})
    res = TC._cli("--module=mmin_miss", "--epoch=1", "--n_train=4", "--n_val=2", "--n_test=2", "--train.batch_size=2", "--mmin_frames=5,9",
                  "--train_missing")
    assert res.returncode != 0 and "--module=mmin_miss: --train_missing" in res.stderr
