"""GPU: bc-LSTM / bc-GRU in capacity mode -- the scans that take the step count from the device (erc_lstm_scan_*_tcap,
erc_gru100_scan_*_tcap) against the existing entry points launched with T = *t_dev (bit for bit) and against a float64
chain, the capacity step against the exact-shape step after a larger batch has used the same bucket, dropout with the applied
masks, bucket graph replay against eager steps on the bucket's buffers, resident epochs against the bucketed loop, and the
command line.

Measured on one MI355X: the capacity step's loss is bit-equal to the exact-shape step's in both cells
(erc_head_ce forms 16-row workgroups in both launches, so the valid rows are summed in the same order) and is asserted equal;
the gradients are not (the weight-gradient products run over B_cap * T_cap / N_cap rows instead of B * T / N, so their sums
are split differently): worst deviation 5.2e-7 (bc-LSTM) / 4.7e-7 (bc-GRU) of the parameter's largest gradient entry, parameters
after three Adam steps within 1.1e-7 / 9.8e-7.  Resident epochs end bit-equal to the bucketed loop (asserted)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from erc_amd import capi
from tests import bcrnn_oracle as O
from tests.rnn_scan_ref import lstm_scan
from tests.util_cases import fill_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = ("lstm", "gru")
H, LDH = 100, 208
B_CAP, T_CAP = 32, 110
STALE = 12345.0
W6 = torch.tensor([1 / 0.086747, 1 / 0.144406, 1 / 0.227883, 1 / 0.160585, 1 / 0.127711, 1 / 0.252668])


@pytest.fixture(scope="module", autouse=True)
def _lib():
    capi.lib()


# ------------------------------------------------------------------------------------------------------------- scans
class _Scan:
    """one layer x both directions of a cell through the C-ABI on time-major padded rows (row t*B + b), every buffer
    pre-filled with a large finite stale value"""

    def __init__(self, cell, B, T_cap, drop, seed):
        self.cell, self.B, self.T_cap, self.drop = cell, B, T_cap, drop
        self.G = 400 if cell == "lstm" else 300
        self.ldgx = 2 * self.G + 16
        g = torch.Generator().manual_seed(seed)
        n = B * T_cap
        self.W = ((torch.rand(2, self.G, H, generator=g) * 2 - 1) * 0.1).to(DEV)
        self.bh = ((torch.rand(2, self.G, generator=g) * 2 - 1) * 0.1).to(DEV)
        self.GX = (torch.randn(n, self.ldgx, generator=g) * 0.5).to(DEV)
        self.up = torch.randn(n, LDH, generator=g).to(DEV)
        self.rng = torch.tensor([3, 1234 + seed], dtype=torch.int64, device=DEV) if drop else None
        self.p = 0.5 if drop else 0.0

    def stale(self, *s):
        return torch.full(s, STALE, device=DEV)

    def run(self, T, t_dev=None):
        """forward + backward; t_dev None: the existing entry points with T; else the T-capacity ones with T = T_cap"""
        n, G, B = self.B * self.T_cap, self.G, self.B
        o = dict(Hout=self.stale(n, LDH), Hdrop=self.stale(n, LDH) if self.drop else None, gates=self.stale(n, 2 * G),
                 s1=self.stale(n, 2 * H), Hprev=self.stale(n, 2 * H), dGX=self.stale(n, 2 * G), dGH=self.stale(n, 2 * G))
        ldhd = LDH if self.drop else 0
        td = None if t_dev is None else torch.tensor([t_dev], dtype=torch.int32, device=DEV)
        if self.cell == "lstm":
            capi.lstm_scan_fwd(self.GX, self.ldgx, self.W, self.bh, None, None, 1, B, B, T, o["Hout"], LDH, o["Hdrop"], ldhd,
                               self.p, self.rng, 0x77, o["gates"], o["s1"], o["Hprev"], t_dev=td)
            capi.lstm_scan_bwd(self.W, None, None, 1, B, B, T, o["gates"], o["s1"], self.up, LDH, self.p, self.rng, 0x77,
                               o["dGX"], t_dev=td)
        else:
            capi.gru100_scan_fwd(self.GX, self.ldgx, self.W, self.bh, None, None, 1, B, B, T, o["Hout"], LDH, o["Hdrop"], ldhd,
                                 self.p, self.rng, 0x77, o["gates"], o["s1"], o["Hprev"], t_dev=td)
            capi.gru100_scan_bwd(self.W, None, None, 1, B, B, T, o["gates"], o["s1"], o["Hprev"], self.up, LDH, self.p, self.rng,
                                 0x77, o["dGX"], o["dGH"], t_dev=td)
        torch.cuda.synchronize()
        return {k: v for k, v in o.items() if v is not None}


@pytest.mark.parametrize("t_dev", [1, 37, 110])
@pytest.mark.parametrize("drop", [0, 1])
@pytest.mark.parametrize("cell", CELLS)
def test_scan_with_device_step_count_equals_the_exact_launch(cell, drop, t_dev):
    """T_cap = 110, *t_dev steps: rows t < *t_dev of every output, saved buffer and gate gradient are bit-identical to the
    existing entry point launched with T = *t_dev on the same data; rows t >= *t_dev: outputs written 0, saved state left
    untouched, gate gradients exactly 0 whatever was there"""
    sc = _Scan(cell, B_CAP, T_CAP, drop, 100 * t_dev + 10 * drop + CELLS.index(cell))
    ref, got = sc.run(t_dev), sc.run(T_CAP, t_dev)
    n_run = t_dev * B_CAP                       # time-major: the rows of t < t_dev are the first t_dev * B
    grads = ("dGX", ) if cell == "lstm" else ("dGX", "dGH")
    for k in got:
        if k == "dGH" and cell == "lstm":
            continue
        w = 2 * H if k in ("Hout", "Hdrop") else got[k].shape[1]
        assert torch.equal(got[k][:n_run, :w], ref[k][:n_run, :w]), k
        assert bool((got[k][:n_run, :w] != STALE).all()), k
        tail = got[k][n_run:, :w]
        if k in ("Hout", "Hdrop") or k in grads:
            assert bool((tail == 0).all()), k          # written zero
        else:
            assert bool((tail == STALE).all()), k      # saved state of rows that are not run: untouched
    for k in ("Hout", "Hdrop"):
        if k in got:
            assert bool((got[k][:, 2 * H:] == STALE).all()), k      # nothing past the 200 columns


@pytest.mark.parametrize("cell", CELLS)
def test_scan_with_device_step_count_matches_the_float64_chain(cell):
    """*t_dev = 37 of T_cap = 110, B = 5, dropped copy on: outputs < 1e-5, gate gradients <= 1e-4 of the chain's largest entry
    (the bounds of tests/test_gpu_gru100.py)"""
    B, t_dev = 5, 37
    sc = _Scan(cell, B, T_CAP, 1, 4242)
    got = sc.run(T_CAP, t_dev)
    G, n_run = sc.G, t_dev * B
    W64, b64 = sc.W.cpu().double(), sc.bh.cpu().double()
    G64 = sc.GX.cpu().double().requires_grad_()
    eps = torch.zeros(B * T_CAP, 2 * G, dtype=torch.float64, requires_grad=True)
    rows = torch.arange(n_run).view(t_dev, B)                     # [t, b] -> row t*B + b
    halves = []
    for d in (0, 1):
        ix = rows if d == 0 else rows.flip(0)
        gx = G64[ix][..., d * G:(d + 1) * G]
        if cell == "lstm":
            h = lstm_scan(gx + eps[ix][..., d * G:(d + 1) * G], W64[d], b64[d])[0]
        else:
            h = O.gru_scan(gx, W64[d], b64[d], eps[ix][..., d * G:(d + 1) * G])
        halves.append(h if d == 0 else h.flip(0))
    H_ref = torch.cat(halves, -1).reshape(n_run, 2 * H)
    Hc, Hd = got["Hout"].cpu()[:n_run, :2 * H], got["Hdrop"].cpu()[:n_run, :2 * H]
    err = float((Hc - H_ref.detach().float()).abs().max())
    print("%s tcap t_dev=%d: |Hout - f64| = %.3g" % (cell, t_dev, err))
    assert err < 1e-5
    kept = Hd != 0
    assert abs(float(kept.float().mean()) - 0.5) < 0.03
    assert torch.allclose(Hd[kept], (Hc * 2.0)[kept], rtol=1e-6, atol=0)
    mask = torch.where(kept, 2.0, 0.0).double()
    (H_ref * mask * sc.up.cpu()[:n_run, :2 * H].double()).sum().backward()
    dgx_ref = torch.cat([G64.grad[:n_run, :G], G64.grad[:n_run, G:2 * G]], -1)
    checks = [("dGX", dgx_ref)] + ([("dGH", eps.grad[:n_run])] if cell == "gru" else [])
    for k, ref in checks:
        g = got[k].cpu()
        e, scale = float((g[:n_run] - ref.float()).abs().max()), float(ref.abs().max())
        print("%s tcap %s: error %.3g of largest entry %.3g" % (cell, k, e, scale))
        assert torch.isfinite(g).all() and e <= 1e-4 * (scale + 1e-12), (k, e, scale)
        assert bool((g[n_run:] == 0).all()), k


# ------------------------------------------------------------------------------------------------------- step level
def _case(lens, D, S, C, seed):
    g = torch.Generator().manual_seed(seed)
    B, T = len(lens), max(lens)
    x = torch.randn(T, B, D, generator=g) * 0.5
    onehot = torch.nn.functional.one_hot(torch.randint(0, S, (T, B), generator=g), S).float()
    for b, L in enumerate(lens):
        x[L:, b] = 0.0
        onehot[L:, b] = 0.0
        onehot[L:, b, 0] = 1.0                 # the speaker-0 one-hot pad rows of the real collate
    return {"input_tensor": x, "speaker_tensor": onehot, "text_length": torch.tensor(lens, dtype=torch.int64),
            "attention_mask": (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float(),
            "label": torch.randint(0, C, (sum(lens),), generator=g)}


def _trainer(cell, extra=("--capacity_buckets=True", ), t_cap=T_CAP):
    import importlib
    plugin = importlib.import_module("track_mm.bc" + cell)
    params = plugin.ParamsType().from_args(["--dataset=iemocap-cogmen-6"] + list(extra))
    tr = plugin.main.args[0](params, DEV)
    tr.t_cap = t_cap
    return tr


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
    return {k: tr.model.flat.g(k).detach().clone() for k in tr.model.flat.params}


SMALL, BIG = [12, 40, 3, 25], [110, 3, 3, 3, 3, 2, 2, 2]        # N = 80 and N = 128: both in the (32, 110, 128) bucket


def _capacity_step(tr, static, fill, batch, step=False):
    fill(static, batch)
    tr.model.dynamic_n = True
    try:
        stats = tr.train_step(static) if step else tr.model.loss_and_grads(static, tr.class_weight)
    finally:
        tr.model.dynamic_n = False
    torch.cuda.synchronize()
    return stats


@pytest.mark.parametrize("cell", CELLS)
def test_capacity_step_equals_the_exact_shape_step_after_a_larger_batch(cell):
    """dropout 0: a ragged batch (lengths 12, 40, 3, 25; D = 712) in the (B_cap, T_cap, N_cap) = (32, 110, 128) bucket, run
    AFTER a larger batch (8 dialogues, T = 110, N = 128) has used the same bucket, against the exact-shape step from the same
    parameters: loss within 1e-4, every gradient within 1e-3 of its largest entry; parameters after three Adam steps within
    the bounds of test_gpu_bcrnn's Adam check.  The largest deviations are printed (not zero: the weight-gradient sums run over
    the capacity rows in another order)."""
    tr = _trainer(cell, ["--capacity_buckets=True", "--dropout=0"])
    tr.model.train()
    small, big = tr.prepare_batch(_case(SMALL, 712, 2, 6, 1)), tr.prepare_batch(_case(BIG, 712, 2, 6, 2))
    key, make, fill = tr.capacity_bucket(small)
    assert key == ("capacity", 32, 110, 128) and tr.capacity_bucket(big)[0] == key
    static = make()
    exact = tr.model.loss_and_grads(small, tr.class_weight)[:3].clone()          # loss, correct count, weight sum
    want_loss = float(exact[0])
    want = _grads(tr)
    _capacity_step(tr, static, fill, big)
    stats = _capacity_step(tr, static, fill, small)
    ws = tr.model._last_ws
    assert ws["counts"].tolist() == [80, 40]
    # the correct count and the weight sum cover the 80 valid rows alone: equal to the exact-shape step's (the loss is
    # bit-equal, so are the logits' argmax; the weight sum is the same fp64 sum of the same 80 labels' weights)
    assert float(stats[1]) == float(exact[1]) and 0 <= float(stats[1]) <= 80
    assert float(stats[2]) == float(exact[2])
    assert abs(float(stats[2]) - float(tr.class_weight.cpu().double()[_case(SMALL, 712, 2, 6, 1)["label"]].sum())) < 1e-3
    d_loss = abs(float(stats[0]) - want_loss)
    worst = 0.0
    for k, g in want.items():
        got = tr.model.flat.g(k)
        scale = float(g.abs().max()) + 1e-6
        e = float((got - g).abs().max())
        worst = max(worst, e / scale)
        assert torch.isfinite(got).all() and e <= 1e-3 * scale, (k, e, scale)
    print("bc%s capacity vs exact: |loss diff| = %.3g, worst gradient deviation %.3g of the largest entry" % (cell, d_loss, worst))
    assert d_loss == 0.0          # measured zero (module docstring); the issue's bound was 1e-4
    # what the tails own is zero past the batch, whatever the larger batch left
    for k in ("dQ", "dE", "dA", "dZc", "dlogits", "E"):
        assert bool((ws[k][80:128] == 0).all()), k
    enc = ws["%s:%s." % (cell, cell)]
    for k in ("dGX", "dGH") if cell == "gru" else ("dGX", ):
        for layer in (0, 1):
            v = enc[k][layer].view(T_CAP, B_CAP, -1)
            assert bool((v[40:] == 0).all()) and bool((v[:, 4:] == 0).all()), (k, layer)      # t >= t_dev; phantom dialogues
    # three Adam steps
    snap = _snapshot(tr)
    for _ in range(3):
        tr.train_step(small)
    torch.cuda.synchronize()
    exact = _params(tr)
    _restore(snap)
    _capacity_step(tr, static, fill, big, step=True)              # leaves its rows in the bucket's workspace ...
    _restore(snap)                                                # ... and nothing in the parameters
    for _ in range(3):
        _capacity_step(tr, static, fill, small, step=True)
    d = (_params(tr) - exact).abs()
    print("bc%s capacity vs exact after 3 Adam steps: max |dp| = %.3g, share above 1e-5 = %.3g"
          % (cell, float(d.max()), float((d > 1e-5).float().mean())))
    assert float((d > 1e-5).float().mean()) < 0.01 and float(d.max()) < 7e-4


@pytest.mark.parametrize("cell", CELLS)
def test_capacity_dropout_step_matches_oracle_with_the_applied_masks(cell):
    """training mode in the bucket: the masks of the RNN's inter-layer dropout and of the classifier are read back from the
    step's buffers (padded row t*B_cap + b); the CPU restatement given those masks reproduces loss and gradients; keep rates
    near 0.5"""
    from erc_amd import bcrnn
    lens, D = [14, 30, 1, 9], 24
    batch = _case(lens, D, 2, 6, 8)
    B, T, N = len(lens), max(lens), sum(lens)
    m = (bcrnn.LSTMModule if cell == "lstm" else bcrnn.GRUModule)(D, 100, 100, n_classes=6, dropout=0.5)
    fill_params(m, 4)
    P = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.finalize(DEV)
    m.train()
    static = dict(input_tensor=torch.zeros(T_CAP, B_CAP, D, device=DEV), speaker_tensor=torch.zeros(T_CAP, B_CAP, 2, device=DEV),
                  text_length=torch.zeros(B_CAP, dtype=torch.int64, device=DEV), label=torch.zeros(128, dtype=torch.int64, device=DEV))
    static["input_tensor"][:T, :B] = batch["input_tensor"].to(DEV)
    static["text_length"][:B] = batch["text_length"].to(DEV)
    static["label"][:N] = batch["label"].to(DEV)
    m.dynamic_n = True
    stats = m.loss_and_grads(static, W6.to(DEV))
    m.dynamic_n = False
    torch.cuda.synchronize()
    ws = m._last_ws
    enc = ws["%s:%s." % (cell, cell)]
    cut = lambda v: v.view(T_CAP, B_CAP, 2 * H)[:T, :B].reshape(T * B, 2 * H).cpu()
    pre, post = cut(enc["H0"]), cut(enc["H0d"])
    assert float((pre == 0).float().mean()) < 1e-3
    kept = post != 0
    assert abs(float(kept.float().mean()) - 0.5) < 0.05
    on = kept & (pre != 0)
    assert torch.allclose(post[on], pre[on] * 2.0, rtol=1e-6, atol=0)
    assert not torch.equal(kept[:, :100], kept[:, 100:])
    masks = {"rnn": kept.float() * 2.0}
    lin = ws["A"][:N].cpu() @ P["linear.weight"].t() + P["linear.bias"]
    z = ws["Zc"][:N].cpu()
    masks["clf"] = torch.where((z != 0) | (lin <= 0), torch.full_like(lin, 2.0), torch.zeros_like(lin))
    assert abs(float((z != 0).float().sum() / (lin > 0).float().sum()) - 0.5) < 0.05
    loss, _, _, grads = O.loss_and_grads(P, batch, cell, W6, masks=masks)
    assert abs(float(stats[0]) - float(loss)) < 1e-4
    assert sorted(grads) == sorted(m.flat.params)
    for name, g in grads.items():
        got = m.flat.g(name).detach().cpu()
        scale = float(g.abs().max()) + 1e-6
        assert float((got - g.float()).abs().max()) <= 1e-3 * scale, name


def test_head_ce_cap_with_an_empty_batch_gives_zero_not_nan():
    """*n_dev = 0: loss 0, no correct row, weight sum 0, every gradient row written 0 over stale values"""
    g = torch.Generator().manual_seed(1)
    n, F, C = 40, 100, 6
    Z, W, b = torch.randn(n, F, generator=g).to(DEV), torch.randn(C, F, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
    y = torch.randint(0, C, (n, ), generator=g).to(DEV)
    for weight in (None, W6.to(DEV)):
        logits, dlogits, dZ = (torch.full(s, STALE, device=DEV) for s in ((n, C), (n, C), (n, F)))
        stats = torch.zeros(max(256, capi.head_ce_stats_floats(n)), device=DEV)
        capi.head_ce(Z, F, F, C, n, W, b, y, weight, 1.0, logits, C, dlogits, C, dZ, F, stats,
                     n_dev=torch.zeros(1, dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        assert stats[:3].tolist() == [0.0, 0.0, 0.0]
        assert bool((dlogits == 0).all()) and bool((dZ == 0).all())


FOUR = ([12, 40, 3, 25], [110, 3, 3, 3, 3, 2, 2, 2], [7] * 9, [1, 2, 60, 30, 11])          # all in the (32, 110, 128) bucket


@pytest.mark.parametrize("cell", CELLS)
def test_bucket_graph_over_four_batches_equals_eager_steps_on_the_buckets_buffers(cell):
    """StepGraphs with the buckets on (dropout 0.5): first batch eager + capture, three replays -- bit-identical to the same
    four steps run eagerly on the bucket's static buffers (capture=False); replaying one batch twice from a restored state is
    bit-identical"""
    from erc_amd.trainer import StepGraphs
    batches = [_case(l, 712, 2, 6, 20 + i) for i, l in enumerate(FOUR)]
    ends = []
    for capture in (False, True):
        tr = _trainer(cell)
        g = StepGraphs(tr, capture=capture)
        losses = []
        for b in batches:
            losses.append(g.step(tr.prepare_batch(b))[0].clone())
        torch.cuda.synchronize()
        assert list(g.cache) == [("capacity", 32, 110, 128)]
        assert (g.captures, g.replays, g.eager) == ((1, 3, 1) if capture else (0, 0, 4))
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


@pytest.mark.parametrize("cell", CELLS)
def test_resident_epochs_equal_the_bucketed_loop(cell):
    """two epochs from a DeviceDialogueStore (one 2 B int32 copy + one replay per step) against StepGraphs fed the batches of
    the same permutations: per-epoch loss sums within 1e-4 per step, final parameters within the Adam check's bounds -- and, as
    measured, bit-equal"""
    from erc_amd.datasets import DeviceDialogueStore
    from erc_amd.synthetic import make_dialogues
    from erc_amd.trainer import ResidentEpochs, StepGraphs
    Bsz, seed = 8, 3
    ends = []
    for mode in ("resident", "bucketed"):
        tr = _trainer(cell, ["--capacity_buckets=True", "--train.batch_size=%d" % Bsz], t_cap=0)
        p = tr.params
        dialogs = make_dialogues(28, p.dims(), n_speakers=p.n_speakers, n_classes=p.n_classes, min_len=1, max_len=45, seed=9)
        store = DeviceDialogueStore(dialogs, p, torch.device(DEV))
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
            assert n_steps == 4 and res.replays > 0 and res.eager == res.captures <= 3
        else:
            g, gen = StepGraphs(tr), torch.Generator().manual_seed(seed)
            for _ in range(2):
                order = torch.randperm(len(store), generator=gen)
                acc = torch.zeros((), dtype=torch.float64, device=DEV)
                for i in range(0, len(store), Bsz):
                    acc += g.step(tr.prepare_batch(store.batch(order[i:i + Bsz])))[0].double()
                torch.cuda.synchronize()
                sums.append(float(acc))
            assert g.replays > 0 and g.eager == g.captures <= 3
        ends.append((_params(tr), sums))
    (p_res, s_res), (p_buc, s_buc) = ends
    d = (p_res - p_buc).abs()
    print("bc%s resident vs bucketed: epoch loss sums %s vs %s, max |dp| = %.3g, bit-equal parameters: %s"
          % (cell, s_res, s_buc, float(d.max()), torch.equal(p_res, p_buc)))
    assert all(np.isfinite(s_res)) and all(abs(a - b) <= 4 * 1e-4 for a, b in zip(s_res, s_buc))
    assert float((d > 1e-5).float().mean()) < 0.01 and float(d.max()) < 7e-4
    assert s_res == s_buc and torch.equal(p_res, p_buc)      # the same launches on the same rows: measured bit-equal


# -------------------------------------------------------------------------------------------------------------- CLI
def _cli(args):
    res = subprocess.run([sys.executable, "train_mm.py"] + args, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    return [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]


RAGGED = ["--dataset=iemocap-cogmen-6", "--modality=atv", "--n_train=40", "--n_test=6", "--syn_min_len=3", "--syn_max_len=60",
          "--train.batch_size=8", "--test.batch_size=4"]


@pytest.mark.parametrize("cell", CELLS)
def test_train_mm_cli_resident(cell):
    """``train_mm.py --module=bc<cell> --device_collate --resident`` on ragged synthetic dialogues: exit 0, finite losses, a
    handful of captured bucket graphs, everything else a replay"""
    lines = _cli(["--module=bc" + cell, "--epoch=3", "--device_collate", "--resident"] + RAGGED)
    epochs = [l for l in lines if "test" in l]
    losses = [l["Lall"] for l in lines if "Lall" in l]
    assert len(epochs) == 3 and len(losses) == 3 and all(np.isfinite(losses))
    last = epochs[-1]
    n_buckets = -(-8 * 60 // 128)
    assert last["graph_replays"] > 0 and 0 < last["graphs_captured"] <= n_buckets
    assert last["eager_steps"] == last["graphs_captured"]
    assert last["graph_replays"] + last["eager_steps"] == 3 * 5


@pytest.mark.parametrize("cell", CELLS)
def test_train_mm_cli_default_losses_are_those_of_the_exact_shape_loop(golden_json, cell):
    """the same command line WITHOUT the new flags prints the first-epoch losses recorded on the commit before capacity mode
    (tests/golden/bcrnn_cli_default_losses.json): the default path is untouched"""
    lines = _cli(["--module=bc" + cell, "--epoch=1"] + RAGGED)
    steps = [l["Lall"] for l in lines if "Lall" in l and "step" in l]
    assert steps == golden_json["bc" + cell]
    last = [l for l in lines if "test" in l][-1]
    assert last["graphs_captured"] == 0 and last["eager_steps"] == 5      # exact shapes: none repeats in one epoch


@pytest.fixture
def golden_json():
    with open(os.path.join(REPO, "tests", "golden", "bcrnn_cli_default_losses.json")) as fh:
        return json.load(fh)
