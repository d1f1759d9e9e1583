"""GPU: the step's output stores in their two forms (csrc/store_dev.h, erc_set_store_mode / ERC_STEP_STORES): ``plain`` and
``through`` (write-through) write the same bits to the same places -- every logical element equal, rows behind the node
count and columns behind a row's last 16-byte piece untouched, the pad columns inside that piece zero."""
import math

import pytest
import torch

from erc_amd import capi
from tests.util_cases import cogmen_case_lengths, to_device

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIMS = dict(a=12, t=20, v=16)             # D = 48: the smallest feature widths of tests/util_cases.py
F = 100
SENT = 3.0                                # sentinel: finite, exact in bf16, never produced as a pad value (pads are 0)
EXTRA = 5                                 # sentinel rows behind the last row of every buffer
COMPUTES = ["bf16", "f32x32"]
# dialogue lengths -> N: two full 16-row tiles + a 15-row tail with dialogues shorter than, equal to and longer than the +-5
# window; one node; exactly one tile; one tile + one row
SHAPES = {"n47": (1, 5, 11, 30), "n1": (1,), "n16": (16,), "n17": (17,)}


@pytest.fixture(autouse=True)
def _default_mode_afterwards():
    yield
    capi.set_store_mode(True)


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bytes(a), _bytes(b)), what


def _sentinel_like(t, extra=EXTRA):
    """(view of the first rows, whole buffer): same shape / dtype / pitch as ``t``, every element the sentinel, ``extra`` rows behind"""
    big = torch.full((t.shape[0] + extra,) + tuple(t.shape[1:]), SENT, dtype=t.dtype, device=t.device)
    return big[:t.shape[0]], big


def _check_layout(name, big, n_rows, logical):
    """rows >= n_rows untouched; pad columns (>= logical) untouched or zero, and finite"""
    assert bool((big[n_rows:] == SENT).all()), "%s: a row behind the node count was written" % name
    if big.dim() == 2 and logical < big.shape[1]:
        pad = big[:n_rows, logical:].float()
        assert bool(torch.isfinite(pad).all()) and bool(((pad == SENT) | (pad == 0)).all()), "%s: pad columns" % name
        # a 16-byte piece made of pad columns only is never written
        per16 = 16 // big.element_size()
        first_free = -(-logical // per16) * per16
        assert bool((big[:n_rows, first_free:] == SENT).all()), "%s: a piece of pad columns only was written" % name


def _module(compute, seed=11):
    from erc_amd.cogmen import COGMENModule
    torch.manual_seed(seed)
    m = COGMENModule(sum(DIMS.values()), 100, 17, 2, 6, compute=compute).finalize(DEV)
    with torch.no_grad():
        m.gcn.conv1.bias.uniform_(-0.1, 0.1)
    m.refresh_shadows()
    return m


# -------------------------------------------------------------------------------------------------- the two tile launches
def _fwd_tile(m, through, lengths, n_cap, bn_fused):
    """one erc_cogmen_fwd_tile(_x) launch and one erc_cogmen_bwd_tile(_x) launch behind it, on sentinel-filled outputs;
    n_cap: capacity form (node count on the device)"""
    from erc_amd.cogmen import WP, WF, PM, PA
    c = cogmen_case_lengths(lengths, dims=DIMS, seed=3)
    b = to_device(c["batch"], DEV)
    B, T = b["input_tensor"].shape[:2]
    N = int(b["label"].shape[0])
    rows = n_cap or N
    ws = m._make_workspace_fused(B, T, rows, DEV, rows * (WP + WF + 1))
    g, fp = ws["g"], m.flat
    spk = b["speaker_tensor"]
    capi.window_graph_build(b["text_length"], spk, spk.stride(0), spk.stride(1), B, T, WP, WF, 2, rows, ws["E"], g)
    torch.manual_seed(5)
    H0 = torch.randn(rows, F, device=DEV)
    split = m.terms > 1
    names = dict(M="M" if split else "Mb", H1="H1" if split else "H1b")
    out, bigs = {}, {}
    for key in (names["M"], names["H1"], "QKVS", "H2", "inv_cnt"):
        out[key], bigs[key] = _sentinel_like(ws[key])
    bn = m.gcn.bn
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    kw = dict(bn_fused=bn_fused, running_mean=rm, running_var=rv, momentum=bn.momentum, eps=bn.eps, saved=ws["bn_saved"],
              bn_ws=ws["bn_tile_ws"], n_speakers=2, n_dev=g["counts"] if n_cap else None)
    if split:
        kw.update(terms=m.terms, catT_plane=m._sh_plane["catT"], q_plane=m._sh_plane["q"])
    capi.set_store_mode(through)
    capi.poison_lds()
    capi.cogmen_fwd_tile(H0, F, rows, WP, WF, g, m._sh["catT"], fp.w("gcn.conv1.bias"), m._sh["q"],
                         fp.w("gcn.conv2.lin_query.bias"), 1.0 / math.sqrt(F), out[names["M"]], 9 * F if split else PM,
                         out["inv_cnt"], out[names["H1"]], F if split else PA, out["QKVS"], out["H2"], F, ws["alpha"], **kw)
    torch.cuda.synchronize()
    E = int(g["in_ptr"][N])
    logical = {names["M"]: 9 * F, names["H1"]: F, "QKVS": 4 * F, "H2": F, "inv_cnt": 8}
    for key, big in bigs.items():
        _check_layout(key, big, N, logical[key])
    res = {key: big[:N, :logical[key]].clone() for key, big in bigs.items()}
    res["alpha"] = ws["alpha"][:E].clone()
    if bn_fused == 1:
        res.update(saved=ws["bn_saved"].clone(), running_mean=rm, running_var=rv)
    elif bn_fused == 2:
        res["bn_part"] = ws["bn_tile_ws"].clone()

    # ---- the backward tile launch on the forward's outputs: bf16 gradients (bf16 mode) / fp32 gradients (split modes)
    torch.manual_seed(6)
    dY = torch.randn(rows, F, device=DEV) * 0.1
    bn_bwd = torch.randn(2 * F, device=DEV) * 0.01
    saved = torch.cat([torch.zeros(F, device=DEV), torch.ones(F, device=DEV)])
    gnames = ("dQKVS", "dH1", "dH0") if split else ("dQKVSb", "dH1b", "dH0b")
    gout, gbigs = {}, {}
    for key in gnames:
        gout[key], gbigs[key] = _sentinel_like(ws[key])
    bkw = dict(n_speakers=2, n_dev=g["counts"] if n_cap else None)
    if split:
        bkw.update(lddh1=F, terms=m.terms_bwd, qT_plane=m._sh_plane["qT"], wb_plane=m._sh_plane["wb"])
    else:
        bkw.update(grads_bf16=True, lddh1=PA)
    capi.poison_lds()
    capi.cogmen_bwd_tile(dY, out["H2"], F, rows, WP, WF, fp.w("gcn.bn.weight"), saved, bn_bwd, out["QKVS"], ws["alpha"], g,
                         out["inv_cnt"], m._sh["qT"], m._sh["wb"], 1.0 / math.sqrt(F), gout[gnames[0]], gout[gnames[1]],
                         gout[gnames[2]], F if split else PA, **bkw)
    torch.cuda.synchronize()
    glogical = dict(zip(gnames, (4 * F, F, F)))
    for key, big in gbigs.items():
        _check_layout(key, big, N, glogical[key])
        res[key] = big[:N, :glogical[key]].clone()
    assert float(res[gnames[0]].float().abs().max()) > 0 and float(res[gnames[2]].float().abs().max()) > 0
    return res


@pytest.mark.parametrize("bn_fused", [0, 1, 2], ids=["no-bn", "bn-here", "bn-sums"])
@pytest.mark.parametrize("shape", list(SHAPES) + ["n47-cap256"])
@pytest.mark.parametrize("compute", COMPUTES)
def test_tile_launches_plain_equal_through(compute, shape, bn_fused):
    n_cap = 256 if shape.endswith("cap256") else 0
    lengths = SHAPES[shape.split("-")[0]]
    m = _module(compute)
    plain = _fwd_tile(m, False, lengths, n_cap, bn_fused)
    through = _fwd_tile(m, True, lengths, n_cap, bn_fused)
    assert plain.keys() == through.keys()
    for k in plain:
        _same_bits(plain[k], through[k], k)
    assert float(plain["QKVS"].abs().max()) > 0 and float(plain["H2"].abs().max()) > 0


def test_forward_tile_keeps_per_lane_stores_for_rows_that_are_not_16_byte_multiples():
    """pitches of 902 / 102 bf16 elements (1804 / 204 bytes): no row pieces; same logical values as the 16-byte-row buffers"""
    from erc_amd.cogmen import WP, WF, PM, PA
    m = _module("bf16")
    c = cogmen_case_lengths(SHAPES["n47"], dims=DIMS, seed=3)
    b = to_device(c["batch"], DEV)
    B, T = b["input_tensor"].shape[:2]
    N = int(b["label"].shape[0])
    ws = m._make_workspace_fused(B, T, N, DEV, N * (WP + WF + 1))
    g, fp, spk = ws["g"], m.flat, b["speaker_tensor"]
    capi.window_graph_build(b["text_length"], spk, spk.stride(0), spk.stride(1), B, T, WP, WF, 2, N, ws["E"], g)
    torch.manual_seed(5)
    H0 = torch.randn(N, F, device=DEV)
    got = {}
    for ldm, ldh in ((PM, PA), (902, 102)):
        Mb = torch.full((N + EXTRA, ldm), SENT, dtype=torch.bfloat16, device=DEV)
        H1b = torch.full((N + EXTRA, ldh), SENT, dtype=torch.bfloat16, device=DEV)
        capi.set_store_mode(True)
        capi.cogmen_fwd_tile(H0, F, N, WP, WF, g, m._sh["catT"], fp.w("gcn.conv1.bias"), m._sh["q"], fp.w("gcn.conv2.lin_query.bias"),
                             1.0 / math.sqrt(F), Mb, ldm, ws["inv_cnt"], H1b, ldh, ws["QKVS"], ws["H2"], F, ws["alpha"])
        torch.cuda.synchronize()
        assert bool((Mb[N:] == SENT).all()) and bool((H1b[N:] == SENT).all())
        if ldm == 902:
            assert bool((Mb[:N, 900:] == SENT).all()) and bool((H1b[:N, 100:] == SENT).all())     # per-lane stores: pads untouched
        got[ldm] = (Mb[:N, :900].clone(), H1b[:N, :100].clone(), ws["QKVS"].clone(), ws["H2"].clone())
    for a, b_ in zip(got[PM], got[902]):
        _same_bits(a, b_, "pitch")


# -------------------------------------------------------------------------------------------------- the step's launches
def _trainer(compute):
    from erc_amd.cogmen import COGMENTrainer
    from erc_amd.params import ERCParams
    torch.manual_seed(0)
    p = ERCParams().from_args(["--dataset=iemocap-cogmen-sbert-6", "--compute=" + compute])
    p.hidden_all = sum(DIMS.values())
    tr = COGMENTrainer(p, DEV)
    assert tr.model.drop_p > 0.0
    return tr


def _state(tr, stats):
    torch.cuda.synchronize()
    flat = tr.model.flat
    out = {"data": flat.data, "exp_avg": flat.exp_avg, "exp_avg_sq": flat.exp_avg_sq, "optim.state": tr.optim.state,
           "grad_full": flat.grad_full, "stats": stats}
    out.update({k: v for k, v in tr.model.state_dict().items() if "running_" in k or "num_batches" in k})
    assert any("running_" in k for k in out)
    return {k: v.detach().clone() for k, v in out.items()}


LOGICAL = dict(Mb=900, H1b=100, H3b=100, Zb=100, dZb=100, dH1b=100, dH0b=100, dlb=6, dlogits=6)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("compute", COMPUTES)
def test_every_launch_of_an_eager_step_plain_equals_through(compute, shape):
    """One eager training step (projection + graph, forward tile, head, backward tile, weight gradients + Adam) whose every
    two-dimensional workspace buffer is sentinel-filled with sentinel rows behind it: each launch's outputs, compared one by
    one between the modes (equal outputs of one launch are the equal inputs of the next)."""
    runs = {}
    for through in (False, True):
        tr = _trainer(compute)
        batch = tr.prepare_batch(cogmen_case_lengths(SHAPES[shape], dims=DIMS, seed=3)["batch"])
        x = batch["input_tensor"]
        B, T, N = x.shape[0], x.shape[1], int(batch["label"].shape[0])
        ws = tr.model._workspace(B, T, N, x.device)
        bigs = {}
        for k, v in list(ws.items()):
            if torch.is_tensor(v) and v.dim() == 2 and v.shape[0] == N and v.is_floating_point():
                ws[k], bigs[k] = _sentinel_like(v)
        assert {"H0", "QKVS", "H2"} <= set(bigs)
        capi.set_store_mode(through)
        stats = tr.train_step(batch)
        torch.cuda.synchronize()
        assert tr.model._last_ws is ws
        for k, big in bigs.items():
            _check_layout(k, big, N, LOGICAL.get(k, big.shape[1]))
        res = {"ws." + k: big[:N, :LOGICAL.get(k, big.shape[1])].clone() for k, big in bigs.items()}
        res.update(_state(tr, stats))
        runs[through] = res
    assert runs[False].keys() == runs[True].keys()
    for k in runs[False]:
        _same_bits(runs[False][k], runs[True][k], k)


def _graphed_run(monkeypatch, stores, compute, replays=3, after_capture=None):
    from erc_amd.engine import GraphedStep
    monkeypatch.setenv("ERC_STEP_STORES", stores)
    tr = _trainer(compute)
    batch = tr.prepare_batch(cogmen_case_lengths(SHAPES["n47"], dims=DIMS, seed=3)["batch"])
    step = GraphedStep(lambda: tr.train_step(batch))
    assert step.captured.stores == stores
    if after_capture is not None:
        after_capture()
    for _ in range(replays):
        stats = step()
    return _state(tr, stats)


@pytest.mark.parametrize("compute", COMPUTES)
def test_three_replayed_steps_with_dropout_plain_equals_through(monkeypatch, compute):
    plain = _graphed_run(monkeypatch, "plain", compute)
    through = _graphed_run(monkeypatch, "through", compute)
    assert int(plain["optim.state"][0]) == 2 + 3               # two warm-up steps, three replayed ones
    assert plain.keys() == through.keys()
    for k in plain:
        _same_bits(plain[k], through[k], k)


def test_a_captured_step_keeps_the_mode_it_was_captured_with(monkeypatch):
    """the switch is read when a launch is enqueued (captured), not when it is replayed"""
    ref = _graphed_run(monkeypatch, "through", "bf16")
    got = _graphed_run(monkeypatch, "through", "bf16", after_capture=lambda: capi.set_store_mode(False))
    for k in ref:
        _same_bits(ref[k], got[k], k)


def test_unknown_store_mode_is_refused_by_the_library():
    with pytest.raises(capi.ErcGraftError, match="set_store_mode"):
        capi._call("erc_set_store_mode", 2)
