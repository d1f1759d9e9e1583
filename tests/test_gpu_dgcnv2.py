"""GPU: the conv-emotion DialogueGCN (--module=dgcnv2) on libercgraft -- the positional edge attention against CPU autograd
(the nodal attention: tests/test_gpu_match_att.py), the whole module against the reference's own DGCNModule (golden
vectors) and the CPU restatement, dropout, HIP-graph replay, checkpoints and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from erc_amd import capi
from tests import dgcnv2_oracle as O
from tests.util_cases import check_grad_digest, fill_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("dgcnv2_s2", "dgcnv2_s9", "dgcnv2_none")
W6 = torch.tensor([1 / 0.086747, 1 / 0.144406, 1 / 0.227883, 1 / 0.160585, 1 / 0.127711, 1 / 0.252668])


@pytest.fixture(scope="module", autouse=True)
def _lib():
    capi.lib()


def _err(a, b):
    return float((a.detach().cpu() - b).abs().max())


def _gpu(batch):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _case(lens, D, S, C, seed):
    g = torch.Generator().manual_seed(seed)
    B, T = len(lens), max(lens)
    x = torch.randn(T, B, D, generator=g) * 0.5
    onehot = torch.nn.functional.one_hot(torch.randint(0, S, (T, B), generator=g), S).float()
    for b, L in enumerate(lens):
        x[L:, b] = 0.0
        onehot[L:, b] = 0.0
    return {"input_tensor": x, "speaker_tensor": onehot, "text_length": torch.tensor(lens, dtype=torch.int64),
            "attention_mask": (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float(),
            "label": torch.randint(0, C, (sum(lens),), generator=g)}


def _module(base, D, S, C, seed):
    from erc_amd.dgcnv2 import DGCNModule
    m = DGCNModule(base, input_size=D, n_speakers=S, n_classes=C)
    fill_params(m, seed)
    P = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.finalize(DEV), P


def _check_grads(m, grads, tol=1e-3):
    for name, g in grads.items():
        if name.startswith(O.DEAD):
            assert g is None and name not in m.flat.params, name
            continue
        got = m.flat.g(name).detach().cpu()
        scale = float(g.abs().max()) + 1e-6
        assert _err(got, g) <= tol * scale, (name, _err(got, g), scale)


# ----------------------------------------------------------------------------------------------------- edge attention
@pytest.mark.parametrize("S", [2, 9])
def test_edge_attention_matches_autograd(S):
    """erc_dgcnv2_edge_att_fwd / _bwd against CPU autograd of the masked, renormalised softmax over time (attn1).  Large
    scores outside the windows, padded rows included, make the 1e-10 leak term matter; dnorm arrives as two partial vectors."""
    lens = [40, 1, 13, 110, 7]
    B, T, N = len(lens), max(lens), sum(lens)
    g = torch.Generator().manual_seed(S)
    Sc = torch.randn(T * B, 110, generator=g)
    for b, L in enumerate(lens):
        if L < T:
            Sc.view(T, B, 110)[L:, b] += 25.0           # padded positions: exp(25) * 1e-10 is not negligible
    Sc.view(T, B, 110)[:, 0, 0] += torch.where(torch.arange(T) > 10, 24.0, 0.0)     # out-of-window, inside the dialogue
    spk = torch.randint(0, S, (T, B), generator=g)
    w = 10 + 10 + 1
    E_cap = N * min(w, T)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)
    gr = dict(node_off=i32(B + 1), node_row=i32(N), node_spk=i32(N), in_ptr=i32(N + 1), in_src=i32(E_cap), in_typ=i32(E_cap),
              out_ptr=i32(N + 1), out_dst=i32(E_cap), out_typ=i32(E_cap), out_eid=i32(E_cap), counts=i32(2))
    ei = torch.zeros(2, E_cap, dtype=torch.int64, device=DEV)
    lens_d = torch.tensor(lens, dtype=torch.int64, device=DEV)
    capi.window_graph_build(lens_d, spk.contiguous().to(DEV), 1, B, B, T, 10, 10, S, N, E_cap, gr, edge_index=ei)
    norm = torch.zeros(E_cap, device=DEV)
    Sd = Sc.to(DEV)
    capi.dgcnv2_edge_att_fwd(Sd, 110, gr, B, T, 10, 10, norm)
    torch.cuda.synchronize()
    n_e = int(gr["in_ptr"][N])
    ei = ei[:, :n_e].cpu()
    off = np.concatenate([[0], np.cumsum(lens)])
    dlg = np.searchsorted(off, ei[0].numpy(), side="right") - 1
    # reference on the CPU
    Sr = Sc.clone().requires_grad_()
    want = []
    for e in range(n_e):
        b = int(dlg[e])
        j, i, L = int(ei[0, e]) - off[b], int(ei[1, e]) - off[b], lens[b]
        col = torch.exp(Sr.view(T, B, 110)[:, b, j] - Sr.view(T, B, 110)[:, b, j].max())
        lo, hi = max(0, j - 10), min(L, j + 11)
        den = col[lo:hi].sum() + 1e-10 * (col[:lo].sum() + col[hi:].sum())
        want.append(col[i] / den)
    want = torch.stack(want)
    assert _err(norm[:n_e], want.detach()) < 1e-6
    G = torch.randn(n_e, generator=g)
    (want * G).sum().backward()
    parts = torch.zeros(2, E_cap)
    parts[0, :n_e], parts[1, :n_e] = 0.25 * G, 0.75 * G
    dS = torch.full((T * B, 110), float("nan"), device=DEV)
    capi.dgcnv2_edge_att_bwd(Sd, 110, gr, B, T, 10, 10, parts.to(DEV).view(-1), dS, dn_parts=2, dn_stride=E_cap)
    torch.cuda.synchronize()
    ref = Sr.grad
    assert torch.isfinite(dS).all()
    assert _err(dS, ref) <= 1e-5 * (float(ref.abs().max()) + 1e-6)
    assert float(ref.view(T, B, 110)[lens[0]:, 0, :lens[0]].abs().max()) > 0       # padded rows do receive gradient
    with pytest.raises(capi.ErcGraftError):
        capi.dgcnv2_edge_att_fwd(Sd, 110, gr, B, 111, 10, 10, norm)


# ----------------------------------------------------------------------------------------------------- whole module
@pytest.mark.parametrize("name", FIXTURES)
def test_module_matches_reference_fixture(golden, name):
    """DGCNModule (eval-mode step: dropout off) against the reference's own DGCNModule: logits, features, the weighted
    loss, every gradient digest, the parameters that receive none, the state_dict keys and shapes"""
    fx = golden(name)
    D = int(fx["in_input_tensor"].shape[-1])
    m, P = _module(str(fx["base_model"]), D, int(fx["n_speakers"]), int(fx["n_classes"]), int(fx["param_seed"]))
    assert list(m.state_dict()) == [str(k) for k in fx["sd_keys"]]
    assert [list(v.shape) for v in m.state_dict().values()] == [[int(d) for d in s if d >= 0] for s in fx["sd_shapes"]]
    batch = _gpu({k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("in_")})
    m.eval()
    logits, feats = m(**batch)
    assert _err(logits, torch.from_numpy(fx["logits"])) < 1e-4
    assert _err(feats, torch.from_numpy(fx["features"])) < 1e-4
    w = W6.to(DEV) if bool(fx["loss_weights"]) else None
    stats = m.loss_and_grads(batch, w)
    assert abs(float(stats[0]) - float(fx["loss"])) < 1e-4
    assert check_grad_digest(fx, [(k, m.flat.g(k)) for k in m.flat.params], 1e-3) < 1e-3
    none = sorted(k for k, _ in m.named_parameters() if k not in m.flat.params)
    assert none == sorted(str(s) for s in fx["grad_none"])


@pytest.mark.parametrize("base", ["LSTM", "None"])
def test_module_step_matches_oracle_and_dead_params_stay(base):
    """loss, gradients and one Adam step against the CPU restatement at atv width (D = 712, T = 110); the dead
    att_model.matchatt / simpleatt / att parameters stay bit-unchanged through several steps"""
    from erc_amd.engine import FusedAdam
    batch = _case([110, 1, 37, 9], 712, 2, 6, 3)
    m, P = _module(base, 712, 2, 6, 11)
    m.eval()
    opt = FusedAdam(m.flat, lr=3e-4)
    m.rng_state = opt.rng_state
    loss, logits, feats, grads = O.loss_and_grads(P, batch, base, W6)
    stats = m.loss_and_grads(_gpu(batch), W6.to(DEV))
    assert abs(float(stats[0]) - float(loss)) < 1e-4
    out = m(**_gpu(batch))
    assert _err(out[0], logits) < 1e-4 and _err(out[1], feats) < 1e-4
    m.loss_and_grads(_gpu(batch), W6.to(DEV))
    _check_grads(m, grads)
    opt.step()
    want = O.adam_step(P, grads, lr=3e-4)
    for k in m.flat.params:
        d = (m.flat.w(k).detach().cpu() - want[k]).abs()
        assert float((d > 1e-5).float().mean()) < 0.01 and float(d.max()) < 7e-4, k
    for _ in range(2):
        m.loss_and_grads(_gpu(batch), W6.to(DEV))
        opt.step()
    sd = m.state_dict()
    for k in P:
        if k.startswith(O.DEAD):
            assert torch.equal(sd[k].cpu(), P[k]), k


def test_dropout_step_matches_oracle_with_the_applied_masks():
    """training mode: the LSTM's inter-layer dropout (in the scan) and the classifier's (GEMM epilogue) read back from the
    step's buffers; the CPU restatement given those masks reproduces loss and gradients; keep rates near 0.6"""
    lens = [14, 30, 1, 9]
    batch = _case(lens, 24, 2, 6, 8)
    m, P = _module("LSTM", 24, 2, 6, 4)
    m.train()
    stats = m.loss_and_grads(_gpu(batch), W6.to(DEV))
    ws = m._last_ws
    keep = 1.0 / 0.6
    T, B = 30, 4
    lw = ws["lstm:lstm."]
    h0, h0d = lw["H0"].cpu(), lw["H0d"].cpu()
    mask_lstm = ((h0d != 0).float() * keep).view(T, B, 200)
    pre = ws["A"].cpu() @ P["graph_net.linear.weight"].t() + P["graph_net.linear.bias"]
    z = ws["Zc"].cpu()
    mask_clf = torch.where((z != 0) | (pre <= 0), torch.full_like(pre, keep), torch.zeros_like(pre))
    r0 = float((h0d != 0).float().mean())
    r1 = float((z != 0).float().sum() / (pre > 0).float().sum())
    assert 0.55 < r0 < 0.65 and 0.5 < r1 < 0.7, (r0, r1)
    loss, _, _, grads = O.loss_and_grads(P, batch, "LSTM", W6, masks={"lstm": mask_lstm, "clf": mask_clf})
    assert abs(float(stats[0]) - float(loss)) < 1e-4
    _check_grads(m, grads)


# ----------------------------------------------------------------------------------------------------- trainer level
def _trainer(extra=()):
    from track_mm.dgcnv2 import DGCNParams
    from erc_amd.dgcnv2 import DGCNv2Trainer
    params = DGCNParams().from_args(["--dataset=iemocap-cogmen-6"] + list(extra))
    return DGCNv2Trainer(params, DEV)


def _params(tr):
    return tr.model.flat.data.detach().clone()


@pytest.mark.parametrize("base", ["LSTM", "None"])
def test_captured_step_equals_eager_and_replays_repeat(base):
    """StepGraphs (first occurrence eager, second captured, then replays) ends bit-identical to k eager steps, and two
    same-seed eager runs end bit-identical"""
    from erc_amd.trainer import StepGraphs
    batch = _case([12, 40, 3, 25], 712, 2, 6, 1)
    extra = ["--base_model=%s" % base]
    runs = []
    for _ in range(2):
        tr = _trainer(extra)
        b = tr.prepare_batch(batch)
        losses = [float(tr.train_step(b)[0]) for _ in range(4)]
        torch.cuda.synchronize()
        runs.append((_params(tr), losses))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert all(np.isfinite(runs[0][1]))
    tr = _trainer(extra)
    graphs = StepGraphs(tr)
    b = tr.prepare_batch(batch)
    for _ in range(4):
        graphs.step(b)
    torch.cuda.synchronize()
    assert graphs.replays == 2 and graphs.captures == 1
    assert torch.equal(_params(tr), runs[0][0])


def test_checkpoint_round_trip_reference_envelope(tmp_path):
    """save -> load into a fresh trainer (parameters and Adam moments), and a reference-style envelope written from a plain
    CPU DGCNModule loads as well (dead parameters included)"""
    from erc_amd import checkpoint
    from erc_amd.dgcnv2 import DGCNModule
    tr = _trainer()
    b = tr.prepare_batch(_case([6, 2], 712, 2, 6, 5))
    for _ in range(2):
        tr.train_step(b)
    path = str(tmp_path / "dgcnv2.ckpt")
    checkpoint.save(tr, path)
    ck = torch.load(path, weights_only=True)
    assert len(ck["optims"]["optim"]["state"]) == len(tr.model.flat.params)
    tr2 = _trainer(["--seed=5"])
    checkpoint.load(tr2, path)
    assert torch.equal(_params(tr2), _params(tr))
    assert torch.equal(tr2.model.flat.exp_avg, tr.model.flat.exp_avg)
    ref = DGCNModule("LSTM", input_size=712, n_speakers=2, n_classes=6)
    fill_params(ref, 3)
    torch.save({"models": {"model": ref.state_dict()}, "optims": {}, "others": {}, "thtensor": {}, "nptensor": {}}, path)
    checkpoint.load(tr2, path)
    sd = tr2.model.state_dict()
    for k, v in ref.state_dict().items():
        assert torch.equal(sd[k].cpu(), v), k


def test_train_mm_cli_dgcnv2():
    """``python train_mm.py --module=dgcnv2`` end to end: finite losses, test metrics, replayed step graphs"""
    args = ["--module=dgcnv2", "--dataset=iemocap-cogmen-6", "--modality=atv", "--epoch=1", "--n_train=24", "--n_test=6",
            "--syn_min_len=12", "--syn_max_len=12", "--train.batch_size=4", "--test.batch_size=4"]
    res = subprocess.run([sys.executable, "train_mm.py"] + args, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]
    steps = [l for l in lines if "Lall" in l]
    epochs = [l for l in lines if "test" in l]
    assert len(steps) == 6 and len(epochs) == 1
    assert all(np.isfinite(l["Lall"]) for l in steps)
    assert epochs[0]["graph_replays"] > 0
