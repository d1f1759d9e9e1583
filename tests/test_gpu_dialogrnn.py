"""GPU: the DialogueRNN model (--module=dialogrnn) on libercgraft -- the two scans against the float64 chain of the CPU
restatement (the matching attention: tests/test_gpu_match_att.py), the whole module against the reference's own
DialogRNNModel (golden vectors) and the restatement, dropout, HIP-graph replay, checkpoints and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from erc_amd import capi
from tests import dialogrnn_oracle as O
from tests.util_cases import check_grad_digest, fill_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("dialogrnn_s2", "dialogrnn_s9", "dialogrnn_pad0")
W6 = torch.tensor([1 / 0.086747, 1 / 0.144406, 1 / 0.227883, 1 / 0.160585, 1 / 0.127711, 1 / 0.252668])
GXW = 1050


@pytest.fixture(scope="module", autouse=True)
def _lib():
    capi.lib()


def _err(a, b):
    return float((a.detach().cpu() - b).abs().max())


def _gpu(batch):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _case(lens, D, S, C, seed, pad0=False):
    g = torch.Generator().manual_seed(seed)
    B, T = len(lens), max(lens)
    x = torch.randn(T, B, D, generator=g) * 0.5
    onehot = torch.nn.functional.one_hot(torch.randint(0, S, (T, B), generator=g), S).float()
    for b, L in enumerate(lens):
        x[L:, b] = 0.0
        onehot[L:, b] = 0.0
        if pad0:
            onehot[L:, b, 0] = 1.0
    return {"input_tensor": x, "speaker_tensor": onehot, "text_length": torch.tensor(lens, dtype=torch.int64),
            "attention_mask": (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float(),
            "label": torch.randint(0, C, (sum(lens),), generator=g)}


def _module(D, C, seed):
    from erc_amd.dialogrnn import DialogRNNModule
    m = DialogRNNModule(D, 150, 150, 100, 100, n_classes=C, context_attention="general")
    fill_params(m, seed)
    P = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.finalize(DEV), P


def _check_grads(m, grads, tol=1e-3):
    assert sorted(grads) == sorted(m.flat.params)
    for name, g in grads.items():
        got = m.flat.g(name).detach().cpu()
        g = g.float()
        scale = float(g.abs().max()) + 1e-6
        assert _err(got, g) <= tol * scale, (name, _err(got, g), scale)


# ----------------------------------------------------------------------------------------------------- the scans
def _lens(B):
    if B == 1:
        return [110]
    if B == 5:
        return [110, 1, 37, 64, 17]
    g = torch.Generator().manual_seed(7)
    lens = [int(v) for v in torch.randint(2, 111, (B,), generator=g)]
    lens[0], lens[1], lens[5] = 110, 1, 110
    return lens


@pytest.mark.parametrize("S", [2, 9])
@pytest.mark.parametrize("B", [1, 5, 32])
def test_scans_match_the_float64_chain(B, S):
    """erc_dialogrnn_scan_fwd / _bwd through the C-ABI on random hoisted products against the float64 chain of the
    restatement: emotions < 1e-5 absolute; dGX and every recurrent-side weight gradient (formed from the gate gradients and
    saved states the backward scan writes) <= 1e-4 of the reference's largest entry, for a random upstream gradient; a second
    backward run is bit-identical.  The last dialogue never hears from party S - 1."""
    D, lens = 24, _lens(B)
    T, N = max(lens), sum(lens)
    m, P = _module(D, 6, 20 + S)
    g = torch.Generator().manual_seed(100 * B + S)
    GX = torch.randn(N, 2 * GXW, generator=g) * 0.5
    spk = torch.randint(0, S, (N,), generator=g)
    off = np.concatenate([[0], np.cumsum(lens)])
    spk[off[-2]:] = torch.randint(0, S - 1, (lens[-1],), generator=g)            # one party never speaks there
    node_off = torch.tensor(off, dtype=torch.int32, device=DEV)
    f32 = lambda *s: torch.zeros(*s, device=DEV)
    GXd, spk_d, E = GX.to(DEV), spk.to(torch.int32).to(DEV), f32(N, 200)
    save = f32(capi.dialogrnn_save_floats(N, B, T))
    fp = m.flat
    capi.dialogrnn_pack(fp.data, m.offs, D, m.WT)
    capi.dialogrnn_scan_fwd(GXd, 2 * GXW, m.WT, fp.data, m.offs, D, node_off, spk_d, B, T, S, N, 0.0, 0.0, None, 0, E, 200, save)
    torch.cuda.synchronize()
    # float64 chain
    P64 = {k: v.double().requires_grad_() for k, v in P.items()}
    G64 = GX.double().requires_grad_()
    rows = []
    for b, L in enumerate(lens):
        halves = []
        for d in (0, 1):
            order = torch.arange(L) if d == 0 else torch.arange(L - 1, -1, -1)
            sl = slice(int(off[b]), int(off[b]) + L)
            e = O.scan_gx(P64, d, G64[sl, d * GXW:(d + 1) * GXW][order], spk[sl][order], D, S)
            halves.append(e[order])
        rows.append(torch.cat(halves, -1))
    E_ref = torch.cat(rows)
    assert _err(E, E_ref.detach().float()) < 1e-5
    up = torch.randn(N, 200, generator=g)
    (E_ref * up.double()).sum().backward()
    dGX, dREC = f32(N, 2 * GXW), f32(2 * N * capi.DIALOGRNN_DREC_ROW)

    def run_bwd(dGX, dREC):
        capi.dialogrnn_scan_bwd(GXd, 2 * GXW, m.WT, fp.data, m.offs, D, node_off, spk_d, B, T, S, N, 0.0, 0.0, None, 0, save, up.to(DEV),
                                200, dGX, 2 * GXW, dREC)
        torch.cuda.synchronize()
    run_bwd(dGX, dREC)

    def close(got, ref, what):
        ref = ref.float()
        assert torch.isfinite(got).all(), what
        assert _err(got, ref) <= 1e-4 * (float(ref.abs().max()) + 1e-12), (what, _err(got, ref), float(ref.abs().max()))
    close(dGX, G64.grad, "dGX")
    sv = {k: v.cpu().double() for k, v in capi.dialogrnn_planes(save, N, capi.DIALOGRNN_SAVE).items()}
    dr = {k: v.cpu().double() for k, v in capi.dialogrnn_planes(dREC, N, capi.DIALOGRNN_DREC).items()}
    dg = dGX.cpu().double()
    for d, name in enumerate(O.DIRS):
        c = name + ".dialogue_cell."
        gi_g, gi_p = dg[:, d * GXW:d * GXW + 450], dg[:, d * GXW + 450:d * GXW + 900]
        close((gi_g.t() @ sv["q_prev"][d]).float(), P64[c + "g_cell.weight_ih"].grad[:, D:], c + "g_cell.weight_ih[:, D:]")
        close((gi_p.t() @ sv["c"][d]).float(), P64[c + "p_cell.weight_ih"].grad[:, D:], c + "p_cell.weight_ih[:, D:]")
        close((dr["dgh_g"][d].t() @ sv["g_prev"][d]).float(), P64[c + "g_cell.weight_hh"].grad, c + "g_cell.weight_hh")
        close(dr["dgh_g"][d].sum(0).float(), P64[c + "g_cell.bias_hh"].grad, c + "g_cell.bias_hh")
        close((dr["dgh_p"][d].t() @ sv["q_prev"][d]).float(), P64[c + "p_cell.weight_hh"].grad, c + "p_cell.weight_hh")
        close(dr["dgh_p"][d].sum(0).float(), P64[c + "p_cell.bias_hh"].grad, c + "p_cell.bias_hh")
        close((dr["dgi_e"][d].t() @ sv["q_drop"][d]).float(), P64[c + "e_cell.weight_ih"].grad, c + "e_cell.weight_ih")
        close(dr["dgi_e"][d].sum(0).float(), P64[c + "e_cell.bias_ih"].grad, c + "e_cell.bias_ih")
        close((dr["dgh_e"][d].t() @ sv["e_prev"][d]).float(), P64[c + "e_cell.weight_hh"].grad, c + "e_cell.weight_hh")
        close(dr["dgh_e"][d].sum(0).float(), P64[c + "e_cell.bias_hh"].grad, c + "e_cell.bias_hh")
    dGX2, dREC2 = f32(N, 2 * GXW), f32(2 * N * capi.DIALOGRNN_DREC_ROW)
    run_bwd(dGX2, dREC2)
    assert torch.equal(dGX, dGX2) and torch.equal(dREC, dREC2)


def test_scans_refuse_long_dialogues_before_launch():
    m, _ = _module(8, 6, 1)
    f32 = lambda *s: torch.zeros(*s, device=DEV)
    T, N = 111, 111
    node_off = torch.tensor([0, N], dtype=torch.int32, device=DEV)
    spk = torch.zeros(N, dtype=torch.int32, device=DEV)
    GX, E, save = f32(N, 2 * GXW), f32(N, 200), f32(capi.dialogrnn_save_floats(N, 1, T))
    with pytest.raises(capi.ErcGraftError, match="110"):
        capi.dialogrnn_scan_fwd(GX, 2 * GXW, m.WT, m.flat.data, m.offs, 8, node_off, spk, 1, T, 2, N, 0.0, 0.0, None, 0, E, 200, save)
    with pytest.raises(capi.ErcGraftError, match="110"):
        capi.dialogrnn_scan_bwd(GX, 2 * GXW, m.WT, m.flat.data, m.offs, 8, node_off, spk, 1, T, 2, N, 0.0, 0.0, None, 0, save, E, 200,
                                f32(N, 2 * GXW), 2 * GXW, f32(2 * N * capi.DIALOGRNN_DREC_ROW))
    with pytest.raises(capi.ErcGraftError, match="n_speakers"):
        capi.dialogrnn_scan_fwd(GX, 2 * GXW, m.WT, m.flat.data, m.offs, 8, node_off, spk, 1, 110, 10, N, 0.0, 0.0, None, 0, E, 200, save)
    assert capi.dialogrnn_max_t() == 110


# ----------------------------------------------------------------------------------------------------- whole module
@pytest.mark.parametrize("name", FIXTURES)
def test_module_matches_reference_fixture(golden, name):
    """DialogRNNModule (eval-mode step: dropout off) against the reference's own DialogRNNModel and MaskedNLLLoss: valid-row
    log-probabilities, emotions, the loss, every gradient digest, the state_dict keys and shapes; every parameter is live"""
    fx = golden(name)
    D = int(fx["in_input_tensor"].shape[-1])
    m, P = _module(D, int(fx["n_classes"]), int(fx["param_seed"]))
    assert list(m.state_dict()) == [str(k) for k in fx["sd_keys"]]
    assert [list(v.shape) for v in m.state_dict().values()] == [[int(d) for d in s if d >= 0] for s in fx["sd_shapes"]]
    batch = _gpu({k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("in_")})
    m.eval()
    log_prob, emo = m(**batch)
    assert _err(log_prob, torch.from_numpy(fx["log_prob"])) < 1e-4
    assert _err(emo, torch.from_numpy(fx["emotions"])) < 1e-4
    w = W6.to(DEV) if bool(fx["loss_weights"]) else None
    stats = m.loss_and_grads(batch, w)
    assert abs(float(stats[0]) - float(fx["loss"])) < 1e-4
    assert check_grad_digest(fx, [(k, m.flat.g(k)) for k in m.flat.params], 1e-3) < 1e-3
    assert sorted(m.flat.params) == sorted(k for k, _ in m.named_parameters()) and len(m.flat.params) == 32
    assert [str(s) for s in fx["grad_none"]] == []


def test_module_step_matches_oracle():
    """loss, log-probabilities, gradients and one Adam step against the CPU restatement at atv width (D = 712, T = 110)"""
    from erc_amd.engine import FusedAdam
    batch = _case([110, 1, 37, 9], 712, 2, 6, 3, pad0=True)
    m, P = _module(712, 6, 11)
    m.eval()
    opt = FusedAdam(m.flat, lr=3e-4)
    m.rng_state = opt.rng_state
    loss, log_prob, emo, grads = O.loss_and_grads(P, batch, W6)
    stats = m.loss_and_grads(_gpu(batch), W6.to(DEV))
    assert abs(float(stats[0]) - float(loss)) < 1e-4
    logits = m._last_ws["logits"]
    assert _err(torch.log_softmax(logits, -1), log_prob) < 1e-4
    out = m(**_gpu(batch))
    assert _err(out[0], log_prob) < 1e-4 and _err(out[1], emo) < 1e-4
    m.loss_and_grads(_gpu(batch), W6.to(DEV))
    _check_grads(m, grads)
    opt.step()
    want = O.adam_step(P, grads, lr=3e-4)
    for k in m.flat.params:
        d = (m.flat.w(k).detach().cpu() - want[k]).abs()
        assert float((d > 1e-5).float().mean()) < 0.01 and float(d.max()) < 7e-4, k


def test_dropout_step_matches_oracle_with_the_applied_masks():
    """training mode: the masks of g, q[p], e (inside the scans), of the emotions (dropout_rec', same launch) and of the
    classifier (GEMM epilogue) are read back from the step's pre / post buffers; the CPU restatement given those masks
    reproduces loss and gradients; keep rates near 0.5 / 0.5 / 0.5 / 0.35 / 0.5; the two directions draw different masks"""
    lens = [14, 30, 1, 9]
    batch = _case(lens, 24, 2, 6, 8)
    m, P = _module(24, 6, 4)
    m.train()
    stats = m.loss_and_grads(_gpu(batch), W6.to(DEV))
    torch.cuda.synchronize()
    ws = m._last_ws
    sv = {k: v.cpu() for k, v in ws["sv"].items()}
    masks, rates = {}, {}
    for key, pre, post in (("g", "g", "g_drop"), ("q", "q", "q_drop"), ("e", "e", "e_drop")):
        assert float((sv[pre] == 0).float().mean()) < 1e-3
        kept = sv[post] != 0
        masks[key] = kept.float() * 2.0
        rates[key] = float(kept.float().mean())
        on = kept & (sv[pre] != 0)
        assert torch.allclose(sv[post][on], sv[pre][on] * 2.0, rtol=1e-6, atol=0)
        assert not torch.equal(kept[0], kept[1])                      # the two directions differ
    e_post = torch.cat([sv["e_drop"][0], sv["e_drop"][1]], -1)        # [N, 200]
    E = ws["E"].cpu()
    live = e_post != 0
    keep_emo = 1.0 / 0.35
    masks["emo"] = torch.where(E != 0, torch.full_like(E, keep_emo), torch.zeros_like(E))
    rates["emo"] = float(((E != 0) & live).float().sum() / live.float().sum())
    assert torch.allclose(E[E != 0], (e_post * keep_emo)[E != 0], rtol=1e-5, atol=0)
    pre = ws["A"].cpu() @ P["linear.weight"].t() + P["linear.bias"]
    z = ws["Zc"].cpu()
    masks["clf"] = torch.where((z != 0) | (pre <= 0), torch.full_like(pre, 2.0), torch.zeros_like(pre))
    rates["clf"] = float((z != 0).float().sum() / (pre > 0).float().sum())
    for key, want in (("g", 0.5), ("q", 0.5), ("e", 0.5), ("emo", 0.35), ("clf", 0.5)):
        assert abs(rates[key] - want) < 0.05, (key, rates)
    loss, _, _, grads = O.loss_and_grads(P, batch, W6, masks=masks)
    assert abs(float(stats[0]) - float(loss)) < 1e-4
    _check_grads(m, grads)


# ----------------------------------------------------------------------------------------------------- trainer level
def _trainer(extra=()):
    from track_mm.dialogrnn import DialogRNNParams
    from erc_amd.dialogrnn import DialogRNNTrainer
    params = DialogRNNParams().from_args(["--dataset=iemocap-cogmen-6"] + list(extra))
    return DialogRNNTrainer(params, DEV)


def _params(tr):
    return tr.model.flat.data.detach().clone()


def test_captured_step_equals_eager_and_replays_repeat():
    """StepGraphs (first occurrence eager, second captured, then replays) ends bit-identical to k eager steps, and two
    same-seed eager runs end bit-identical"""
    from erc_amd.trainer import StepGraphs
    batch = _case([12, 40, 3, 25], 712, 2, 6, 1, pad0=True)
    runs = []
    for _ in range(2):
        tr = _trainer()
        b = tr.prepare_batch(batch)
        losses = [float(tr.train_step(b)[0]) for _ in range(4)]
        torch.cuda.synchronize()
        runs.append((_params(tr), losses))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert all(np.isfinite(runs[0][1]))
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
    CPU DialogRNNModule loads as well"""
    from erc_amd import checkpoint
    from erc_amd.dialogrnn import DialogRNNModule
    tr = _trainer()
    b = tr.prepare_batch(_case([6, 2], 712, 2, 6, 5, pad0=True))
    for _ in range(2):
        tr.train_step(b)
    path = str(tmp_path / "dialogrnn.ckpt")
    checkpoint.save(tr, path)
    ck = torch.load(path, weights_only=True)
    assert len(ck["optims"]["optim"]["state"]) == len(tr.model.flat.params) == 32
    tr2 = _trainer(["--seed=5"])
    checkpoint.load(tr2, path)
    assert torch.equal(_params(tr2), _params(tr))
    assert torch.equal(tr2.model.flat.exp_avg, tr.model.flat.exp_avg)
    ref = DialogRNNModule(712, 150, 150, 100, 100, n_classes=6, context_attention="general")
    fill_params(ref, 3)
    torch.save({"models": {"model": ref.state_dict()}, "optims": {}, "others": {}, "thtensor": {}, "nptensor": {}}, path)
    checkpoint.load(tr2, path)
    sd = tr2.model.state_dict()
    for k, v in ref.state_dict().items():
        assert torch.equal(sd[k].cpu(), v), k


def test_train_mm_cli_dialogrnn():
    """``python train_mm.py --module=dialogrnn`` end to end: finite losses, test metrics, replayed step graphs"""
    args = ["--module=dialogrnn", "--dataset=iemocap-cogmen-6", "--modality=atv", "--epoch=1", "--n_train=24", "--n_test=6",
            "--syn_min_len=12", "--syn_max_len=12", "--train.batch_size=4", "--test.batch_size=4"]
    res = subprocess.run([sys.executable, "train_mm.py"] + args, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]
    steps = [l for l in lines if "Lall" in l]
    epochs = [l for l in lines if "test" in l]
    assert len(steps) == 6 and len(epochs) == 1
    assert all(np.isfinite(l["Lall"]) for l in steps)
    assert epochs[0]["graph_replays"] > 0
