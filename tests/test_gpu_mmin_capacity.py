"""GPU: --module=mmin_base from HBM.  The device collate (csrc/mmin_collate.hip) against its torch restatement
(tests/mmin_cap_ref.py) bit for bit, the T- and B-capacity forms of the hidden-128 scans (erc_lstm128_pool_*_tcap) against
the exact launches, the bucket step against the exact-shape step, one captured graph over batches of different lengths, the
resident epoch against the bucketed loop, the resident evaluation against the host path, and the command line.  Every test
prints its measured figures before it asserts."""
import json
import os
import subprocess
import sys

import pytest
import torch

from erc_amd import capi
from tests import mmin_cap_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, G4, EMB = 128, 512, 384
GUARD = 3              # rows behind every buffer a kernel writes: nothing may touch them
SENT = -77.25          # what the write sets are pre-filled with
TV, TT = 5, 6          # visual / text rows of the small stores (the feature widths are the real ones)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    capi.lib()


def _buf(rows, cols, dtype=torch.float32):
    return torch.full((rows + GUARD, cols), SENT, dtype=dtype, device=DEV)


def _guard_intact(t, rows):
    return bool((t[rows:] == (SENT if t.is_floating_point() else int(SENT))).all())


def _bits(a, b):
    """bit equality of two tensors (NaN-proof, -0 != +0)"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.is_floating_point():
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and bool((a == b).all())


# ---------------------------------------------------------------------------------------------------------------- collate
def _device_store(frames, seed=3):
    from erc_amd.datasets import MMINDeviceStore
    return MMINDeviceStore(R.samples_with_frames(frames, seed=seed, tv=TV, tt=TT), DEV)


class _CollateOut:
    def __init__(self, B_cap, T_cap):
        self.B_cap, self.T_cap = B_cap, T_cap
        self.audio, self.visual, self.text = _buf(B_cap * T_cap, R.AUDIO_D), _buf(B_cap * TV, R.VISUAL_D), _buf(B_cap * TT, R.TEXT_D)
        self.label, self.counts = _buf(B_cap, 1, torch.int64), _buf(2, 1, torch.int32)

    def run(self, store, desc, frames_max=None):
        d = torch.as_tensor(desc, dtype=torch.int32).to(DEV)
        capi.mmin_collate(d, store.audio, store.visual, store.text, store.label, self.B_cap, self.T_cap,
                          self.T_cap if frames_max is None else frames_max, self.audio, self.visual, self.text, self.label, self.counts)
        torch.cuda.synchronize()

    def check(self, store, desc):
        B, T = self.B_cap, self.T_cap
        a, v, t, y, c = R.collate_ref(store, desc, B, T)
        got = dict(audio=(self.audio, B * T, a.reshape(B * T, -1)), visual=(self.visual, B * TV, v.reshape(B * TV, -1)),
                   text=(self.text, B * TT, t.reshape(B * TT, -1)), label=(self.label, B, y.reshape(B, 1)), counts=(self.counts, 2, c.reshape(2, 1)))
        for name, (buf, rows, ref) in got.items():
            assert _bits(buf[:rows], ref), name
            assert _guard_intact(buf, rows), name + ": guard rows"
        return c.tolist()


# frames of the store's samples, B_cap, T_cap, the slots' sample indices (None: an empty slot)
COLLATE_CASES = {
    "ragged": ((16, 1, 7, 3), 4, 16, (0, 1, 2, None)),           # frames [16, 1, 7, 0]
    "equal": ((5, 5), 2, 8, (1, 0)),
    "one": ((9, ), 1, 16, (0, )),
}


def _desc_of(store, slots, B_cap):
    d = torch.zeros(3, B_cap, dtype=torch.int32)
    for b, i in enumerate(slots):
        if i is not None:
            d[0, b], d[1, b], d[2, b] = int(store.lengths[i]), int(store.offsets[i]), i
    return d.reshape(-1)


@pytest.mark.parametrize("name", sorted(COLLATE_CASES))
def test_collate(name):
    """erc_mmin_collate against the restatement, bit for bit: every output element, guard rows, counts"""
    frames, B_cap, T_cap, slots = COLLATE_CASES[name]
    store = _device_store(frames)
    desc = _desc_of(store, slots, B_cap)
    if all(s is not None for s in slots):
        assert torch.equal(desc, torch.from_numpy(store.desc([s for s in slots], B_cap)))
    out = _CollateOut(B_cap, T_cap)
    out.run(store, desc)
    counts = out.check(store, desc)
    live = [frames[s] for s in slots if s is not None]
    print("collate %s: counts %s" % (name, counts))
    assert counts == [len(live), max(live)]


def test_collate_stale_rows_and_clamps():
    """a long batch, then a short one into the same buffers: nothing of the first survives; then a descriptor whose frames, first
    row and sample index lie outside the store: clamped on the device, as the restatement clamps them"""
    store = _device_store((16, 1, 7, 3, 12))
    out = _CollateOut(4, 16)
    long_ = _desc_of(store, (0, 4, 2, 3), 4)
    out.run(store, long_)
    assert out.check(store, long_) == [4, 16]
    short = _desc_of(store, (1, 3, None, None), 4)
    out.run(store, short)
    assert out.check(store, short) == [2, 3]
    empty = torch.zeros(12, dtype=torch.int32)
    out.run(store, empty)
    assert out.check(store, empty) == [0, 0]
    n_frames = int(store.audio.shape[0])
    wild = torch.tensor([40, -3, 5, 16, n_frames - 2, 7, -9, 10 ** 6, 99, 0, -1, 2], dtype=torch.int32)
    out.run(store, wild)
    assert out.check(store, wild) == [3, 16]


def test_collate_refusals():
    store = _device_store((4, 2))
    out = _CollateOut(2, 8)
    desc = _desc_of(store, (0, 1), 2).to(DEV)
    args = lambda **kw: {**dict(desc=desc, store_audio=store.audio, store_visual=store.visual, store_text=store.text, store_label=store.label,
                                B_cap=2, T_cap=8, frames_max=8, audio=out.audio, visual=out.visual, text=out.text, label=out.label,
                                counts=out.counts), **kw}
    for kw in (dict(frames_max=9), dict(B_cap=0), dict(B_cap=-1), dict(desc=None), dict(audio=None), dict(counts=None), dict(store_audio=None),
               dict(store_label=None), dict(T_cap=0)):
        with pytest.raises(capi.ErcGraftError):
            capi.mmin_collate(**args(**kw))
    torch.cuda.synchronize()
    for buf in (out.audio, out.visual, out.text, out.label, out.counts):      # refused before any launch: nothing written
        assert _guard_intact(buf, 0)


# ------------------------------------------------------------------------------------------------------------------ scans
B_CAP, T_CAP, T_VIS = 3, 16, 5


def _scan_inputs():
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(DEV)
    return dict(GXa=rnd(B_CAP * T_CAP, G4), GXv=rnd(B_CAP * T_VIS, G4), Wa=rnd(G4, H, scale=0.088), Wv=rnd(G4, H, scale=0.088),
                ba=rnd(G4, scale=0.088), bv=rnd(G4, scale=0.088), dpool=rnd(B_CAP, EMB))


class _ScanBufs:
    """the buffers of one audio and one visual job at pitch T, pre-filled with the sentinel"""

    def __init__(self, x, B, Ta, Tv):
        self.B, self.T = B, (Ta, Tv)
        self.pool, self.jobs, self.outs = _buf(B, EMB), [], []
        for n, (T, GX, W, b) in enumerate(((Ta, x["GXa"], x["Wa"], x["ba"]), (Tv, x["GXv"], x["Wv"], x["bv"]))):
            o = dict(arg=_buf(B, H, torch.int32), gates=_buf(B * T, G4), Cst=_buf(B * T, H), Hprev=_buf(B * T, H), dGX=_buf(B * T, G4))
            self.outs.append(o)
            self.jobs.append(dict(GX=GX, W_hh=W, b_hh=b, pool=self.pool[:, n * H:], dpool=x["dpool"][:, n * H:], B=B, T=T, ldp=EMB, lddp=EMB, **o))


def _exact_audio(x, B, T):
    """erc_lstm128_pool_fwd / _bwd of the audio job at exactly T steps on the same GX values (rows re-pitched to T)"""
    GX = x["GXa"].reshape(B_CAP, T_CAP, G4)[:B, :T].reshape(B * T, G4).contiguous()
    bufs = _ScanBufs(dict(x, GXa=GX), B, T, T_VIS)
    capi.lstm128_pool_fwd(bufs.jobs[:1])
    capi.lstm128_pool_bwd(bufs.jobs[:1])
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("n_b", [3, 2, 0])
@pytest.mark.parametrize("t_dev", [1, 7, 8, 9, 16, 0, T_CAP + 3])
def test_scan_tcap(t_dev, n_b):
    """one audio job (T from the device) and one visual job (T = 5, fixed) in one launch: valid rows carry the bits of the exact
    launch at T = Tdev, dGX is zero everywhere else, the forward writes nothing outside its write set, a second launch is
    bit-equal; counts[1] = 0 and T_cap + 3 are clamped to 1 and T_cap"""
    x = _scan_inputs()
    Td = min(max(t_dev, 1), T_CAP)
    counts = torch.tensor([n_b, t_dev], dtype=torch.int32, device=DEV)
    cap = _ScanBufs(x, B_CAP, T_CAP, T_VIS)
    run = lambda: (capi.lstm128_pool_fwd_tcap(cap.jobs, counts, 1), capi.lstm128_pool_bwd_tcap(cap.jobs, counts, 1), torch.cuda.synchronize())
    run()
    first = [cap.pool.clone()] + [{k: v.clone() for k, v in o.items()} for o in cap.outs]
    run()
    assert _bits(cap.pool, first[0])
    for o, f in zip(cap.outs, first[1:]):
        for k in o:
            assert _bits(o[k], f[k]), "second launch: " + k
    sent = lambda t: bool((t == (SENT if t.is_floating_point() else int(SENT))).all())
    assert sent(cap.pool[B_CAP:]) and bool((cap.pool[:B_CAP, 2 * H:] == SENT).all())
    assert bool((cap.pool[n_b:B_CAP, :2 * H] == 0).all())                     # slots the batch does not have pool to zero
    for job, (o, T, Tj) in enumerate(zip(cap.outs, (T_CAP, T_VIS), (Td, T_VIS))):
        if n_b:
            ex = _exact_audio(x, n_b, Td) if job == 0 else None
            if job == 1:
                ex = _ScanBufs(x, n_b, T_CAP, T_VIS)
                capi.lstm128_pool_fwd(ex.jobs[1:])
                capi.lstm128_pool_bwd(ex.jobs[1:])
                torch.cuda.synchronize()
            eo = ex.outs[0] if job == 0 else ex.outs[1]
            assert _bits(cap.pool[:n_b, job * H:(job + 1) * H], ex.pool[:n_b, (0 if job == 0 else H):(H if job == 0 else 2 * H)]), "pool"
            assert _bits(o["arg"][:n_b], eo["arg"][:n_b]), "arg"
            for k, w in (("gates", G4), ("Cst", H), ("Hprev", H), ("dGX", G4)):
                got = o[k][:B_CAP * T].reshape(B_CAP, T, w)[:n_b, :Tj]
                assert _bits(got, eo[k][:n_b * Tj].reshape(n_b, Tj, w)), "job %d %s" % (job, k)
        # dGX: zero outside the valid rows, the samples the batch does not have included; guard rows intact
        d = o["dGX"][:B_CAP * T].reshape(B_CAP, T, G4)
        assert bool((d[n_b:] == 0).all()) and bool((d[:, Tj:] == 0).all()), "dGX tail"
        assert sent(o["dGX"][B_CAP * T:])
        # forward write set: nothing outside the valid rows, arg rows of missing slots untouched
        assert sent(o["arg"][n_b:])
        for k, w in (("gates", G4), ("Cst", H), ("Hprev", H)):
            t = o[k][:B_CAP * T].reshape(B_CAP, T, w)
            assert sent(t[n_b:]) and sent(t[:, Tj:]) and sent(o[k][B_CAP * T:]), "write set: " + k
    print("scan tcap: counts (%d, %d) -> Bdev %d Tdev %d: valid rows bit-equal, tails zero" % (n_b, t_dev, n_b, Td))


def test_scan_refusals():
    """the old entry points still take at most two jobs; the capacity forms refuse what they refuse, null counts and a mask bit
    beyond the jobs"""
    x = _scan_inputs()
    cap = _ScanBufs(x, B_CAP, T_CAP, T_VIS)
    counts = torch.tensor([B_CAP, T_CAP], dtype=torch.int32, device=DEV)
    assert capi.lstm128_max_jobs() == 2
    three = cap.jobs + cap.jobs[:1]
    for fn in (capi.lstm128_pool_fwd, capi.lstm128_pool_bwd):
        with pytest.raises(capi.ErcGraftError):
            fn(three)
    for fn in (capi.lstm128_pool_fwd_tcap, capi.lstm128_pool_bwd_tcap):
        for jobs, cnt, mask in ((three, counts, 1), (cap.jobs, None, 1), (cap.jobs, counts, 4), (cap.jobs[:1], counts, 2), (cap.jobs, counts, -1)):
            with pytest.raises(capi.ErcGraftError):
                fn(jobs, cnt, mask)
    torch.cuda.synchronize()
    assert bool((cap.pool == SENT).all()) and all(bool((v == (SENT if v.is_floating_point() else int(SENT))).all())
                                                  for o in cap.outs for v in o.values())


# ------------------------------------------------------------------------------------------------------------ bucket step
def _trainer(*argv, dropout=True, t_cap=16):
    from erc_amd.mmin import MMINBaseTrainer
    from track_mm.mmin_base import MMINBaseParams
    p = MMINBaseParams().from_args(["--train.batch_size=4", "--val.batch_size=4", "--test.batch_size=4"] + list(argv))
    tr = MMINBaseTrainer(p, DEV)
    tr.t_cap = t_cap
    if not dropout:
        tr.model.DROP_TEXT = tr.model.DROP_C = 0.0
    tr.model.train()
    return tr


def _host_batch(frames, seed):
    from erc_amd.mmin import mmin_collate
    return mmin_collate(R.samples_with_frames(frames, seed=seed, tv=TV, tt=TT))


def _bucket_step(tr, static, fill, batch):
    fill(static, batch)
    tr.model.dynamic_n = True
    try:
        stats = tr.model.loss_and_grads(static)
    finally:
        tr.model.dynamic_n = False
    torch.cuda.synchronize()
    return stats


def _grads(tr):
    return {k: tr.model.flat.g(k).detach().clone() for k in tr.model.flat.params}


SMALL, BIG = (11, 4, 7), (16, 9, 13, 2)          # B = 3, Ta = 11 in the bucket (B_cap, T_cap) = (4, 16), after B = 4, Ta = 16


def test_bucket_step_equals_the_exact_shape_step_after_a_larger_batch():
    """dropout off: #correct equal, loss within 1e-4, every gradient within 1e-3 of its largest magnitude (the criterion of
    tests/test_gpu_dialogrnn_capacity.py); the gradient rows of the slot the batch does not have, and of the audio steps beyond
    its longest utterance, are zero whatever the larger batch left.  As measured: loss equal, worst gradient deviation 1.5e-7 of
    the largest entry (the weight-gradient sums run over the capacity rows in another order)."""
    tr = _trainer("--capacity_buckets=True", dropout=False)
    small, big = tr.prepare_batch(_host_batch(SMALL, 1)), tr.prepare_batch(_host_batch(BIG, 2))
    key, make, fill = tr.capacity_bucket(small)
    assert key == ("capacity", 4, 16, TV, TT) and tr.capacity_bucket(big)[0] == key
    static = make()
    exact = tr.model.loss_and_grads(small).clone()
    torch.cuda.synchronize()
    assert tr.model._last_ws["counts"] is None
    want = _grads(tr)
    _bucket_step(tr, static, fill, big)
    stats = _bucket_step(tr, static, fill, small)
    ws = tr.model._last_ws
    assert ws["counts"].tolist() == [3, 11] and ws["logits"].shape[0] == 4
    d_loss, worst = abs(float(stats[0]) - float(exact[0])), 0.0
    for k, g in want.items():
        got = tr.model.flat.g(k)
        scale = float(g.abs().max()) + 1e-6
        e = float((got - g).abs().max())
        worst = max(worst, e / scale)
        assert torch.isfinite(got).all() and e <= 1e-3 * scale, (k, e, scale)
    print("mmin bucket vs exact: #correct %d / %d, |loss diff| = %.3g, worst gradient deviation %.3g of the largest entry"
          % (float(stats[1]), float(exact[1]), d_loss, worst))
    assert float(stats[1]) == float(exact[1]) and 0 <= float(stats[1]) <= 3
    assert torch.isfinite(exact[0]) and d_loss <= 1e-4
    for k in ("dlogits", "dfeat", "dz0", "dfused", "dtext"):
        assert bool((ws[k][3:] == 0).all()) and float(ws[k][:3].abs().max()) > 0, k
    assert bool((ws["L"]["dpd"][3:] == 0).all())
    dA, dV = ws["A"]["dGX"].reshape(4, 16, G4), ws["V"]["dGX"].reshape(4, TV, G4)
    assert bool((dA[3:] == 0).all()) and bool((dA[:, 11:] == 0).all()) and float(dA[:3, :11].abs().max()) > 0
    assert bool((dV[3:] == 0).all()) and float(dV[:3].abs().max()) > 0
    assert bool((ws["fused"][3:, :2 * H] == 0).all())


def test_bucket_step_draws_the_exact_steps_dropout_masks():
    """dropout on, both steps from the same counter: the kept / dropped pattern of z0, feat and the dropped text features on the
    batch's rows equals the exact-shape step's (the masks are keyed by the element index at pitches 128 / 384, not by B)"""
    tr = _trainer("--capacity_buckets=True")
    small, big = tr.prepare_batch(_host_batch(SMALL, 1)), tr.prepare_batch(_host_batch(BIG, 2))
    key, make, fill = tr.capacity_bucket(small)
    static = make()
    _bucket_step(tr, static, fill, big)
    x_stats = tr.model.loss_and_grads(small).clone()
    torch.cuda.synchronize()
    xs = tr.model._last_ws
    want = dict(z0=xs["z0"].clone(), feat=xs["feat"].clone(), pd=xs["L"]["pd"].clone(), pooled=xs["L"]["pooled"].clone())
    stats = _bucket_step(tr, static, fill, small)
    ws = tr.model._last_ws
    assert ws is not xs
    got = dict(z0=ws["z0"][:3], feat=ws["feat"][:3], pd=ws["L"]["pd"][:3], pooled=ws["L"]["pooled"][:3])
    rates = {}
    for k in ("z0", "feat", "pd"):
        assert torch.equal(got[k] != 0, want[k] != 0), k
        rates[k] = float((want[k] != 0).float().mean())
    live = want["pooled"] != 0
    keep = float(((want["pd"] != 0) & live).float().sum() / live.float().sum())
    print("mmin bucket dropout: non-zero share z0 %.3f feat %.3f, text keep rate %.3f; bit-equal z0 %s feat %s pd %s; |loss diff| %.3g"
          % (rates["z0"], rates["feat"], keep, _bits(got["z0"], want["z0"]), _bits(got["feat"], want["feat"]), _bits(got["pd"], want["pd"]),
             abs(float(stats[0]) - float(x_stats[0]))))
    assert 0.2 < keep < 0.8 and 0.05 < rates["z0"] < 0.7          # dropout ran (0.5 on 1152 text values, 0.3 behind a ReLU)
    assert abs(float(stats[0]) - float(x_stats[0])) <= 1e-4


# ------------------------------------------------------------------------------------------------ one graph, many batches
STREAM = ((16, 9, 13, 2), (9, 1, 4, 6), (3, 2, 1, 3), (12, 5, 8, 12), (7, 10))      # four batches of different Ta, a short last one


def test_one_graph_serves_batches_of_different_lengths_bit_for_bit():
    """the same five batches through StepGraphs twice from the same seed: every step eager on the bucket's buffers, and one
    eager step + one capture + four replays.  Stats of every step and the final parameters, moments and EMA are bit-equal."""
    from erc_amd.trainer import StepGraphs
    ends = []
    for capture in (False, True):
        tr = _trainer("--capacity_buckets=True")
        g = StepGraphs(tr, capture=capture)
        rows = []
        for n, frames in enumerate(STREAM):
            rows.append(g.step(tr.prepare_batch(_host_batch(frames, 10 + n)))[:2].clone())
        torch.cuda.synchronize()
        assert len(g.cache) == 1 and not tr.model.dynamic_n
        assert (g.eager, g.captures, g.replays) == ((1, 1, 4) if capture else (5, 0, 0))
        f = tr.model.flat
        ends.append((torch.stack(rows).cpu(), [t.clone() for t in (f.data, f.exp_avg, f.exp_avg_sq, tr.ema, tr.optim.state[:3])]))
    (s_eager, p_eager), (s_graph, p_graph) = ends
    print("mmin one graph over 5 batches: losses eager %s, replayed %s" % (s_eager[:, 0].tolist(), s_graph[:, 0].tolist()))
    assert torch.isfinite(s_eager).all() and _bits(s_eager, s_graph)
    for a, b in zip(p_eager, p_graph):
        assert _bits(a, b)
    assert int(p_graph[4][0]) == 5


# ----------------------------------------------------------------------------------------------------------- resident loops
def _split(n, seed, split="train"):
    return R.small_samples(n, (3, 150), seed=seed, split=split, tv=TV, tt=TT)


def test_resident_epochs_equal_the_bucketed_loop():
    """two epochs of 10 samples at B = 4 (T capacities 64, 128, 150) from the device store -- 3 B int32 and one replay per step
    -- against StepGraphs fed the host-collated batches of a DataLoader on a generator in the same state: per-epoch loss sums
    within 4e-4, #correct equal.  Whether the parameters end bit-equal is printed (as measured: they do)."""
    from torch.utils.data import DataLoader
    from erc_amd.datasets import MMINDeviceStore
    from erc_amd.mmin import MMINResidentEpochs, mmin_collate
    from erc_amd.trainer import StepGraphs, train_epoch_loader
    samples, ends = _split(10, 21), []
    for mode in ("resident", "bucketed"):
        tr = _trainer("--capacity_buckets=True", t_cap=max(s["audio_feature"].shape[0] for s in samples))
        gen, sums = torch.Generator().manual_seed(5), []
        if mode == "resident":
            res = MMINResidentEpochs(tr, MMINDeviceStore(samples, DEV), 4, gen)
            prev = torch.zeros(4, dtype=torch.float64)
            for _ in range(2):
                assert res.epoch() == [4, 4, 2]
                acc = res.acc.cpu()
                sums.append((acc - prev)[:2].tolist())
                prev = acc
            assert res.replays > 0 and res.eager == res.captures <= 3 and res.replays + res.eager == 6
        else:
            loader = DataLoader(samples, batch_size=4, shuffle=True, collate_fn=mmin_collate, generator=gen)
            g, ring = StepGraphs(tr), torch.zeros(3, 4, device=DEV)
            for _ in range(2):
                assert train_epoch_loader(loader, g, tr, ring) == [4, 4, 2]
                sums.append(ring.double().sum(0)[:2].cpu().tolist())
            assert g.replays > 0 and g.eager == g.captures <= 3
        torch.cuda.synchronize()
        assert not tr.model.dynamic_n
        ends.append((tr.model.flat.data.clone(), tr.ema.clone(), sums))
    (p_res, e_res, s_res), (p_buc, e_buc, s_buc) = ends
    print("mmin resident vs bucketed: epoch {loss sum, #correct} %s vs %s, max |dp| = %.3g, parameters bit-equal: %s, EMA bit-equal: %s"
          % (s_res, s_buc, float((p_res - p_buc).abs().max()), _bits(p_res, p_buc), _bits(e_res, e_buc)))
    for a, b in zip(s_res, s_buc):
        assert all(map(lambda v: v == v and abs(v) < 1e30, a)) and abs(a[0] - b[0]) <= 4e-4 and a[1] == b[1]


def test_resident_eval_equals_the_host_path():
    """a 7-sample split at B = 4 after three training steps (the EMA weights differ from the model's): both confusion matrices
    equal those built from ``eval_epoch``'s true / pred on the host path, Lall lies within the bound of tests/mmin_cap_ref.py of
    the float64 cross entropy of the exact path's logits, and the evaluation leaves parameters, EMA, optimizer state, dropout
    counter and training flag as they were.  A second epoch (all replays) returns the same."""
    import numpy as np
    from torch.utils.data import DataLoader
    from erc_amd.datasets import MMINDeviceStore
    from erc_amd.mmin import MMINResidentEval, mmin_collate
    tr = _trainer("--device_collate", "--resident", "--resident_eval", t_cap=150)
    for n in range(3):
        tr.train_step(tr.prepare_batch(_host_batch((20, 6, 9, 14), 40 + n)))
    samples = _split(7, 33, "val")
    loader = DataLoader(samples, batch_size=4, shuffle=False, collate_fn=mmin_collate)
    host = tr.eval_epoch(loader)
    tr.use_ema = False
    with tr.ema_weights():
        host2 = tr.eval_epoch(loader)
    tr.use_ema = True
    logits = [tr.to_logits(tr.prepare_batch(b)).cpu() for b in loader]
    l64, l32, bound = R.lall_reference(logits, [b["label"] for b in loader])
    tr.model.train()
    f = tr.model.flat
    state = lambda: [t.clone() for t in (f.data, f.exp_avg, f.exp_avg_sq, tr.ema, tr.optim.state[:3], tr.model.rng_state)]
    before = state()
    ev = MMINResidentEval(tr, MMINDeviceStore(samples, DEV), 4)
    out = ev.epoch()
    again = ev.epoch()
    torch.cuda.synchronize()
    assert tr.model.training and not tr.model.dynamic_n and tr._swap is None
    for a, b in zip(before, state()):
        assert _bits(a, b)
    cm = lambda r: np.bincount(np.asarray(r["true"]) * 4 + np.asarray(r["pred"]), minlength=16).reshape(4, 4)
    print("mmin resident eval: Lall %.9g, float64 %.9g, float32 twin %.9g: |diff| %.3g, bound %.3g; host path %.9g; Acc %.4f / %.4f, Acc2 %.4f / %.4f"
          % (out["Lall"], l64, l32, abs(out["Lall"] - l64), bound, host["Lall"], out["Acc"], host["Acc"], out["Acc2"], host["Acc2"]))
    np.testing.assert_array_equal(out["cm"], cm(host))
    np.testing.assert_array_equal(out["cm2"], cm(host2))
    assert out["C"] == host["C"] == 7 and out["Acc"] == host["Acc"] and out["Acc2"] == host["Acc2"]
    assert abs(out["Lall"] - l64) <= bound
    assert ev.eager == ev.captures == len(set(ev.caps)) and ev.replays == 4 * len(ev.caps) - ev.eager
    assert again["Lall"] == out["Lall"] and np.array_equal(again["cm"], out["cm"]) and np.array_equal(again["cm2"], out["cm2"])


# -------------------------------------------------------------------------------------------------------------------- CLI
def _cli(*argv):
    env = dict(os.environ, PYTHONPATH=REPO)
    return subprocess.run([sys.executable, os.path.join(REPO, "train_mm.py")] + list(argv), capture_output=True, text=True, env=env,
                          timeout=300, cwd=REPO)


CLI = ["--module=mmin_base", "--epoch=2", "--n_train=12", "--n_val=5", "--n_test=5", "--train.batch_size=4", "--mmin_frames=5,40"]
OLD_KEYS = {"epoch", "train_utt_per_s", "lr", "val", "test", "report", "class_names", "best_acc", "is_best"}
COUNTERS = {"graph_replays", "eager_steps", "graphs_captured"}


def _epoch_lines(res):
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [json.loads(ln) for ln in res.stdout.strip().splitlines()]
    return [ln for ln in lines if "train_utt_per_s" in ln]


def test_cli_resident_run():
    lines = _epoch_lines(_cli(*CLI, "--device_collate", "--resident", "--resident_eval"))
    assert [ln["epoch"] for ln in lines] == [0, 1]
    for ln in lines:
        assert set(ln) == OLD_KEYS | COUNTERS and set(ln["val"]) == set(ln["test"]) == {"Lall", "Acc", "Acc2"}
        assert 0.0 <= ln["test"]["Acc"] <= 1.0 and ln["val"]["Lall"] > 0 and set(ln["report"]) >= {"acc", "f1", "wa"}
    assert lines[1]["graph_replays"] > 0 and lines[1]["graphs_captured"] == lines[1]["eager_steps"] >= 1
    print("mmin cli resident: %s" % {k: lines[1][k] for k in sorted(COUNTERS)})


def test_cli_default_line_is_unchanged_and_buckets_run():
    lines = _epoch_lines(_cli(*CLI))
    assert [ln["epoch"] for ln in lines] == [0, 1] and all(set(ln) == OLD_KEYS for ln in lines)
    lines = _epoch_lines(_cli(*CLI, "--capacity_buckets=True"))
    assert all(set(ln) == OLD_KEYS | COUNTERS for ln in lines) and lines[1]["graph_replays"] > 0


def test_cli_mmin_miss_still_refuses_resident():
    res = _cli("--module=mmin_miss", "--epoch=1", "--n_train=4", "--n_val=2", "--n_test=2", "--train.batch_size=2", "--mmin_frames=5,9",
               "--resident")
    assert res.returncode != 0 and "--module=mmin_miss: --resident is not built" in res.stderr
