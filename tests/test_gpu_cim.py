"""GPU: CIM (--module=cim) on libercgraft -- the GRU scans and the cross-modal attention against CPU autograd, the whole
module against the reference's own CIMModule (golden vectors) and the CPU restatement, dropout, HIP-graph replay,
reproducibility, checkpoints and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from erc_amd import capi
from tests.cim_oracle import FEATURE, adam_step, cim_loss_and_grads
from tests.util_cases import fill_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("cim_tiny", "cim_iemocap_c4", "cim_iemocap_c6")
DEAD = ("rnn_adapter.", "cls7.")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    capi.lib()


def _case(lens, dims, C, seed, garbage=False):
    g = torch.Generator().manual_seed(seed)
    B, T = len(lens), max(lens)
    batch = {"text_length": torch.tensor(lens, dtype=torch.int64),
             "attention_mask": (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float()}
    for m in "atv":
        x = torch.randn(B, T, dims[m], generator=g) * 0.5
        for b, L in enumerate(lens):
            x[b, L:] = 1e4 if garbage else 0.0      # padded positions: must not influence anything
        batch[FEATURE[m]] = x
    batch["label"] = torch.randint(0, C, (sum(lens),), generator=g)
    return batch


def _module(dims, C, seed, drop=0.3):
    from erc_amd.cim import CIMModule
    m = CIMModule(dims["t"], dims["a"], dims["v"], 200, C, drop0=drop, drop1=drop)
    fill_params(m, seed)
    P = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.finalize(DEV), P


def _gpu(batch):
    return {k: v.to(DEV) for k, v in batch.items()}


def _err(a, b):
    return float((a.detach().cpu() - b).abs().max())


def _check_grads(m, grads, tol=1e-3):
    for name, g in grads.items():
        if name.startswith(DEAD):
            assert g is None, name
            continue
        got = m.flat.g(name).detach().cpu()
        scale = float(g.abs().max()) + 1e-6
        assert _err(got, g) <= tol * scale, (name, _err(got, g), scale)


# ----------------------------------------------------------------------------------------------------- GRU scan
def _gru_case(lens, d_in, seed):
    g = torch.Generator().manual_seed(seed)
    grus = {m: torch.nn.GRU(d_in[m], 200, bidirectional=True, batch_first=True) for m in "avt"}
    for i, m in enumerate("avt"):
        torch.manual_seed(seed + i)
        grus[m].reset_parameters()
    B, T = len(lens), max(lens)
    xs = {m: torch.randn(B, T, d_in[m], generator=g) for m in "avt"}
    return grus, xs


@pytest.mark.parametrize("lens,d_in", [((1, 110, 37, 5), dict(a=100, v=512, t=768)), ((3, 1, 8), dict(a=100, v=100, t=512))])
def test_gru_scan_matches_torch_gru(lens, d_in):
    """erc_gru_scan_fwd / _bwd against torch.nn.GRU on packed ragged batches (both directions, compact rows, lengths 1 and
    110): outputs, and the weight gradients built from the kernel's dGX / dGH against autograd."""
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    grus, xs = _gru_case(lens, d_in, 5)
    B, T, N = len(lens), max(lens), sum(lens)
    lengths = torch.tensor(lens, dtype=torch.int64)
    rows = torch.cat([b * T + torch.arange(L) for b, L in enumerate(lens)])
    ref_out, dH, ref_grads = {}, {}, {}
    g = torch.Generator().manual_seed(9)
    for m in "avt":
        gru = grus[m]
        gru.zero_grad()
        out, _ = gru(pack_padded_sequence(xs[m], lengths, batch_first=True, enforce_sorted=False))
        out, _ = pad_packed_sequence(out, batch_first=True, total_length=T)
        comp = out.reshape(B * T, 400)[rows]
        dH[m] = torch.randn(N, 400, generator=g)
        (comp * dH[m]).sum().backward()
        ref_out[m] = comp.detach()
        ref_grads[m] = {k: v.grad.clone() for k, v in gru.named_parameters()}
    GX = torch.zeros(3, N, 1200)
    Whh = torch.zeros(6, 600, 200)
    bhh = torch.zeros(6, 600)
    for i, m in enumerate("avt"):
        p = dict(grus[m].named_parameters())
        W_ih = torch.cat([p["weight_ih_l0"], p["weight_ih_l0_reverse"]]).detach()
        b_ih = torch.cat([p["bias_ih_l0"], p["bias_ih_l0_reverse"]]).detach()
        GX[i] = xs[m].reshape(B * T, -1)[rows] @ W_ih.t() + b_ih
        Whh[2 * i], Whh[2 * i + 1] = p["weight_hh_l0"].detach(), p["weight_hh_l0_reverse"].detach()
        bhh[2 * i], bhh[2 * i + 1] = p["bias_hh_l0"].detach(), p["bias_hh_l0_reverse"].detach()
    f32 = lambda *s: torch.zeros(*s, device=DEV)
    node_off = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=DEV)
    Hout, gates, ghn, Hprev = f32(3, N, 400), f32(3, N, 1200), f32(3, N, 400), f32(3, N, 400)
    dGX, dGH = f32(3, N, 1200), f32(3, N, 1200)
    Wd, WT = Whh.to(DEV), Whh.transpose(1, 2).contiguous().to(DEV)
    capi.gru_scan_fwd(GX.to(DEV), WT, bhh.to(DEV), lengths.to(DEV), node_off, B, T, N, Hout, None, 0.0, None, 0, gates, ghn, Hprev)
    capi.gru_scan_bwd(Wd, lengths.to(DEV), node_off, B, T, N, gates, ghn, Hprev, torch.stack([dH[m] for m in "avt"]).to(DEV),
                      0.0, None, 0, dGX, dGH)
    torch.cuda.synchronize()
    for i, m in enumerate("avt"):
        assert _err(Hout[i], ref_out[m]) < 1e-5, m
        x = xs[m].reshape(B * T, -1)[rows]
        gx, gh, hp = dGX[i].cpu(), dGH[i].cpu(), Hprev[i].cpu()
        want = ref_grads[m]
        for d, sfx in enumerate(("", "_reverse")):
            got = {"weight_ih_l0": gx[:, 600 * d:600 * d + 600].t() @ x, "bias_ih_l0": gx[:, 600 * d:600 * d + 600].sum(0),
                   "weight_hh_l0": gh[:, 600 * d:600 * d + 600].t() @ hp[:, 200 * d:200 * d + 200],
                   "bias_hh_l0": gh[:, 600 * d:600 * d + 600].sum(0)}
            for k, v in got.items():
                ref = want[k + sfx]
                assert _err(v, ref) <= 1e-4 * (float(ref.abs().max()) + 1e-3), (m, k + sfx)


# ----------------------------------------------------------------------------------------------------- attention
def test_attention_matches_autograd():
    """erc_cim_attn_fwd / _bwd against CPU autograd of attention_op on ragged dialogues (lengths 1..110); the dense values
    are what ReLU and drop1 leave (about half exact zeros), so the backward's mask tail takes both arms at a scale other than 1"""
    from tests.cim_oracle import PAIRS, cross_attention
    lens = [7, 1, 110, 23]
    N, B, T = sum(lens), len(lens), max(lens)
    g = torch.Generator().manual_seed(2)
    keep = {m: torch.rand(N, 100, generator=g) < 0.5 for m in "avt"}
    dense = {m: ((torch.rand(N, 100, generator=g) * 0.6 + 0.05) * keep[m]).requires_grad_() for m in "avt"}
    mask_scale = 1.0 / (1.0 - 0.3)
    outs = [cross_attention(dense[x], dense[y], lens) for x, y in PAIRS]
    G = torch.randn(N, 600, generator=g)
    Gd = torch.randn(N, 300, generator=g)
    (torch.cat(outs, -1) * G).sum().backward()
    merged = torch.cat(outs + [dense[m] for m in "avt"], -1).detach()
    mg = torch.zeros(N, 900, device=DEV)
    mg[:, 600:] = merged[:, 600:].to(DEV)
    node_off = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=DEV)
    P = torch.zeros(6 * B * T * T, device=DEV)
    capi.cim_attn_fwd(mg, node_off, B, T, P)
    dm = torch.cat([G, Gd], -1).to(DEV)
    capi.cim_attn_bwd(mg, dm, node_off, B, T, P, mask_scale)
    torch.cuda.synchronize()
    assert _err(mg, merged) < 1e-5
    for i, m in enumerate("avt"):
        want = (dense[m].grad + Gd[:, 100 * i:100 * i + 100]) * keep[m] * mask_scale
        assert (~keep[m]).any() and bool((dm[:, 600 + 100 * i:700 + 100 * i].cpu()[~keep[m]] == 0).all()), m
        assert _err(dm[:, 600 + 100 * i:700 + 100 * i], want) <= 1e-5 * (float(want.abs().max()) + 1), m
    # T above the LDS limit is refused before launch
    with pytest.raises(capi.ErcGraftError):
        capi.cim_attn_fwd(mg, node_off, B, capi.cim_max_t() + 1, P)


# ----------------------------------------------------------------------------------------------------- whole module
@pytest.mark.parametrize("name", FIXTURES)
def test_module_matches_reference_fixture(golden, name):
    """CIMModule (eval-mode step: dropout off) against the reference's own CIMModule: logits2 / logits7, the loss,
    every gradient digest and the set of parameters that receive none; the state_dict key list and shapes."""
    from tests.util_cases import check_grad_digest
    fx = golden(name)
    dims = dict(zip("atv", (int(v) for v in fx["dims"])))
    C = int(fx["n_classes"])
    m, P = _module(dims, C, int(fx["param_seed"]))
    assert [k for k in m.state_dict()] == list(fx["sd_keys"])
    assert [list(v.shape) for v in m.state_dict().values()] == [list(s[s >= 0]) for s in fx["sd_shapes"]]
    batch = {k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("in_")}
    m.eval()
    l2, l7 = m(**_gpu(batch))
    assert _err(l2, torch.from_numpy(fx["logits2"])) < 1e-4
    assert _err(l7, torch.from_numpy(fx["logits7"])) < 1e-4
    stats = m.loss_and_grads(_gpu(batch))
    assert abs(float(stats[0]) - float(fx["loss"])) < 1e-5
    live = [(k, m.flat.g(k)) for k in m.flat.params]
    assert check_grad_digest(fx, live, 1e-3) < 1e-3
    none = sorted(k for k, _ in m.named_parameters() if k not in m.flat.params)
    assert none == sorted(str(s) for s in fx["grad_none"])


def test_module_step_matches_oracle_and_dead_params_stay():
    """loss, gradients and one Adam step against the CPU restatement (garbage in padded feature rows changes nothing);
    rnn_adapter.* and cls7.* stay bit-unchanged through several steps"""
    from erc_amd.engine import FusedAdam
    dims = dict(a=100, t=100, v=512)
    batch = _case([5, 1, 17, 9], dims, 6, 3, garbage=True)
    clean = _case([5, 1, 17, 9], dims, 6, 3, garbage=False)
    m, P = _module(dims, 6, 11)
    m.eval()
    opt = FusedAdam(m.flat, lr=1e-3)
    m.rng_state = opt.rng_state
    loss, l2, _, grads, _ = cim_loss_and_grads(P, clean)
    stats = m.loss_and_grads(_gpu(batch))
    assert abs(float(stats[0]) - float(loss)) < 1e-5
    assert _err(m.forward(**_gpu(batch))[0], l2) < 1e-4
    m.loss_and_grads(_gpu(batch))
    _check_grads(m, grads)
    opt.step()
    want, _ = adam_step(P, grads)
    for k in m.flat.params:
        d = (m.flat.w(k).detach().cpu() - want[k]).abs()
        assert float((d > 1e-5).float().mean()) < 0.01 and float(d.max()) < 2.1e-3, k
    for _ in range(2):
        m.loss_and_grads(_gpu(batch))
        opt.step()
    sd = m.state_dict()
    for k in P:
        if k.startswith(DEAD):
            assert torch.equal(sd[k].cpu(), P[k]), k


def test_dropout_step_matches_oracle_with_the_applied_masks():
    """training mode: drop0 (in the scan) and drop1 (GEMM epilogue, one seed per modality) read back from the step's
    buffers; the CPU restatement given those masks reproduces loss and gradients; keep rates near 0.7"""
    dims = dict(a=12, t=16, v=20)
    batch = _case([9, 30, 1, 14], dims, 4, 8)
    m, P = _module(dims, 4, 4)
    m.train()
    stats = m.loss_and_grads(_gpu(batch))
    ws = m._last_ws
    keep = 1.0 / 0.7
    masks = {}
    for i, mod in enumerate("avt"):
        hd, ho = ws["Hdrop"][i].cpu(), ws["Hout"][i].cpu()
        masks["drop0_" + mod] = (hd != 0).float() * keep
        pre = hd @ P["adapter.%s.0.weight" % mod].t() + P["adapter.%s.0.bias" % mod]
        dense = ws["merged"][:, 600 + 100 * i:700 + 100 * i].cpu()
        masks["drop1_" + mod] = torch.where((dense != 0) | (pre <= 0), torch.full_like(pre, keep), torch.zeros_like(pre))
        r0 = float((hd != 0).float().mean())
        r1 = float((dense != 0).float().sum() / (pre > 0).float().sum())
        assert 0.66 < r0 < 0.74 and 0.6 < r1 < 0.8, (mod, r0, r1)
    assert not torch.equal(masks["drop1_a"], masks["drop1_v"])
    loss, _, _, grads, _ = cim_loss_and_grads(P, batch, masks)
    assert abs(float(stats[0]) - float(loss)) < 1e-5
    _check_grads(m, grads)


# ----------------------------------------------------------------------------------------------------- trainer level
def _trainer(extra=()):
    from track_mm.cim import CIMParams
    from erc_amd.cim import CIMTrainer
    params = CIMParams().from_args(["--dataset=iemocap-cogmen-6"] + list(extra))
    return CIMTrainer(params, DEV)


def _params(tr):
    return tr.model.flat.data.detach().clone()


def test_captured_step_equals_eager_and_runs_repeat():
    """StepGraphs (first occurrence eager, second captured, then replays) ends bit-identical to k eager steps, and two
    same-seed eager runs end bit-identical"""
    from erc_amd.trainer import StepGraphs
    batch = _case([12, 40, 3, 25], dict(a=100, t=100, v=512), 6, 1)
    runs = []
    for _ in range(2):
        tr = _trainer()
        b = tr.prepare_batch(batch)
        losses = [float(tr.train_step(b)[0]) for _ in range(4)]
        torch.cuda.synchronize()
        runs.append((_params(tr), losses))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    tr = _trainer()
    graphs = StepGraphs(tr)
    b = tr.prepare_batch(batch)
    for _ in range(4):
        graphs.step(b)
    torch.cuda.synchronize()
    assert graphs.replays == 2 and graphs.captures == 1
    assert torch.equal(_params(tr), runs[0][0])


def test_checkpoint_round_trip_reference_envelope(tmp_path):
    """save -> load into a fresh trainer (parameters and Adam moments), and a reference-style envelope written from a plain
    CPU CIMModule loads as well (dead parameters included)"""
    from erc_amd import checkpoint
    from erc_amd.cim import CIMModule
    tr = _trainer()
    b = tr.prepare_batch(_case([6, 2], dict(a=100, t=100, v=512), 6, 5))
    for _ in range(2):
        tr.train_step(b)
    path = str(tmp_path / "cim.ckpt")
    checkpoint.save(tr, path)
    ck = torch.load(path, weights_only=True)
    assert len(ck["optims"]["optim"]["state"]) == len(tr.model.flat.params)
    tr2 = _trainer(["--seed=5"])
    checkpoint.load(tr2, path)
    assert torch.equal(_params(tr2), _params(tr))
    assert torch.equal(tr2.model.flat.exp_avg, tr.model.flat.exp_avg)
    ref = CIMModule(100, 100, 512, 200, 6)
    fill_params(ref, 3)
    torch.save({"models": {"model": ref.state_dict()}, "optims": {}, "others": {}, "thtensor": {}, "nptensor": {}}, path)
    checkpoint.load(tr2, path)
    sd = tr2.model.state_dict()
    for k, v in ref.state_dict().items():
        assert torch.equal(sd[k].cpu(), v), k


def test_train_mm_cli_cim():
    """``python train_mm.py --module=cim`` end to end: finite losses, test metrics, replayed step graphs"""
    args = ["--module=cim", "--dataset=iemocap-cogmen-6", "--modality=atv", "--epoch=1", "--n_train=24", "--n_test=6",
            "--syn_min_len=12", "--syn_max_len=12", "--train.batch_size=4", "--test.batch_size=4"]
    res = subprocess.run([sys.executable, "train_mm.py"] + args, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]
    steps = [l for l in lines if "Lall" in l]
    epochs = [l for l in lines if "test" in l]
    assert len(steps) == 6 and len(epochs) == 1
    assert all(np.isfinite(l["Lall"]) for l in steps)
    assert epochs[0]["graph_replays"] > 0
