"""GPU: the bc-LSTM and bc-GRU baselines (--module=bclstm, --module=bcgru) on libercgraft -- the whole module against the
reference's own LSTMModel / GRUModel (golden vectors) and against the CPU restatement (tests/bcrnn_oracle.py), dropout with
the applied masks, HIP-graph replay, Adam steps, checkpoints and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from erc_amd import capi
from tests import bcrnn_oracle as O
from tests.util_cases import check_grad_digest, fill_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = (("bclstm_s2", "lstm"), ("bclstm_s9", "lstm"), ("bcgru_s2", "gru"), ("bcgru_s9", "gru"))
CELLS = ("lstm", "gru")
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
        onehot[L:, b, 0] = 1.0                 # the speaker-0 one-hot pad rows of the real collate
    return {"input_tensor": x, "speaker_tensor": onehot, "text_length": torch.tensor(lens, dtype=torch.int64),
            "attention_mask": (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float(),
            "label": torch.randint(0, C, (sum(lens),), generator=g)}


def _module(cell, D, C, seed, dropout=0.5):
    from erc_amd import bcrnn
    m = (bcrnn.LSTMModule if cell == "lstm" else bcrnn.GRUModule)(D, 100, 100, n_classes=C, dropout=dropout)
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


@pytest.mark.parametrize("name,cell", FIXTURES)
def test_module_matches_reference_fixture(golden, name, cell):
    """eval-mode step (dropout off) against the reference's own model and MaskedNLLLoss: valid-row log-probabilities,
    emotions, the loss, every gradient digest, the state_dict keys and shapes; every parameter is live"""
    fx = golden(name)
    D = int(fx["in_input_tensor"].shape[-1])
    m, P = _module(cell, D, int(fx["n_classes"]), int(fx["param_seed"]))
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
    assert sorted(m.flat.params) == sorted(k for k, _ in m.named_parameters()) and len(m.flat.params) == 22
    assert [str(s) for s in fx["grad_none"]] == []


def _ragged32():
    g = torch.Generator().manual_seed(5)
    lens = [int(v) for v in torch.randint(2, 111, (32,), generator=g)]
    lens[0], lens[1], lens[17] = 110, 1, 110
    return lens


@pytest.mark.parametrize("cell", CELLS)
def test_ragged_b32_t110_step_matches_oracle(cell):
    """loss, log-probabilities, emotions and every gradient against the CPU restatement on a ragged batch of 32 dialogues,
    T = 110 (lengths 1 .. 110)"""
    batch = _case(_ragged32(), 64, 2, 6, 3)
    m, P = _module(cell, 64, 6, 11)
    m.eval()
    loss, log_prob, emo, grads = O.loss_and_grads(P, batch, cell, W6)
    out = m(**_gpu(batch))
    assert _err(out[0], log_prob) < 1e-4 and _err(out[1], emo) < 1e-4
    stats = m.loss_and_grads(_gpu(batch), W6.to(DEV))
    assert abs(float(stats[0]) - float(loss)) < 1e-4
    assert _err(torch.log_softmax(m._last_ws["logits"], -1), log_prob) < 1e-4
    _check_grads(m, grads)


@pytest.mark.parametrize("cell", CELLS)
def test_more_than_8_classes_takes_the_gemm_head(cell):
    batch = _case([7, 12, 3], 24, 2, 10, 6)
    m, P = _module(cell, 24, 10, 5)
    m.eval()
    loss, log_prob, _, grads = O.loss_and_grads(P, batch, cell, None)
    stats = m.loss_and_grads(_gpu(batch), None)
    assert abs(float(stats[0]) - float(loss)) < 1e-4
    _check_grads(m, grads)


@pytest.mark.parametrize("cell", CELLS)
def test_dropout_step_matches_oracle_with_the_applied_masks(cell):
    """training mode: the mask of the RNN's inter-layer dropout (written by the layer-0 scan) and of the classifier (GEMM
    epilogue) are read back from the step's pre / post buffers; the CPU restatement given those masks reproduces loss and
    gradients; keep rates near 0.5; the two directions draw different masks"""
    lens = [14, 30, 1, 9]
    batch = _case(lens, 24, 2, 6, 8)
    m, P = _module(cell, 24, 6, 4)
    m.train()
    stats = m.loss_and_grads(_gpu(batch), W6.to(DEV))
    torch.cuda.synchronize()
    ws = m._last_ws
    enc = ws["%s:%s." % (cell, cell)]
    pre, post = enc["H0"].cpu(), enc["H0d"].cpu()
    assert float((pre == 0).float().mean()) < 1e-3
    kept = post != 0
    assert abs(float(kept.float().mean()) - 0.5) < 0.05
    on = kept & (pre != 0)
    assert torch.allclose(post[on], pre[on] * 2.0, rtol=1e-6, atol=0)
    assert not torch.equal(kept[:, :100], kept[:, 100:])
    masks = {"rnn": kept.float() * 2.0}
    lin = ws["A"].cpu() @ P["linear.weight"].t() + P["linear.bias"]
    z = ws["Zc"].cpu()
    masks["clf"] = torch.where((z != 0) | (lin <= 0), torch.full_like(lin, 2.0), torch.zeros_like(lin))
    assert abs(float((z != 0).float().sum() / (lin > 0).float().sum()) - 0.5) < 0.05
    loss, _, _, grads = O.loss_and_grads(P, batch, cell, W6, masks=masks)
    assert abs(float(stats[0]) - float(loss)) < 1e-4
    _check_grads(m, grads)


# ----------------------------------------------------------------------------------------------------- trainer level
def _trainer(cell, extra=()):
    import importlib
    plugin = importlib.import_module("track_mm.bc" + cell)
    params = plugin.ParamsType().from_args(["--dataset=iemocap-cogmen-6"] + list(extra))
    return plugin.main.args[0](params, DEV)


def _params(tr):
    return tr.model.flat.data.detach().clone()


@pytest.mark.parametrize("cell", CELLS)
def test_captured_step_equals_eager_and_replays_repeat(cell):
    """StepGraphs (first occurrence eager, second captured, then replays) ends bit-identical to k eager steps, and two
    same-seed eager runs end bit-identical"""
    from erc_amd.trainer import StepGraphs
    batch = _case([12, 40, 3, 25], 712, 2, 6, 1)
    runs = []
    for _ in range(2):
        tr = _trainer(cell)
        b = tr.prepare_batch(batch)
        losses = [float(tr.train_step(b)[0]) for _ in range(4)]
        torch.cuda.synchronize()
        runs.append((_params(tr), losses))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert all(np.isfinite(runs[0][1]))
    tr = _trainer(cell)
    graphs = StepGraphs(tr)
    b = tr.prepare_batch(batch)
    for _ in range(4):
        graphs.step(b)
    torch.cuda.synchronize()
    assert graphs.replays == 2 and graphs.captures == 1
    assert torch.equal(_params(tr), runs[0][0])


@pytest.mark.parametrize("cell", CELLS)
def test_two_adam_steps_match_torch_adam_on_the_restatement(cell):
    """two eval-mode steps (dropout 0) of the fused Adam against torch.optim.Adam on the CPU restatement"""
    from erc_amd.engine import FusedAdam
    batch = _case([20, 1, 37, 9], 712, 2, 6, 3)
    m, P = _module(cell, 712, 6, 11)
    m.eval()
    opt = FusedAdam(m.flat, lr=3e-4)
    m.rng_state = opt.rng_state
    want, losses = O.adam_steps(P, batch, cell, W6, 2)
    b = _gpu(batch)
    for k in range(2):
        stats = m.loss_and_grads(b, W6.to(DEV))
        assert abs(float(stats[0]) - losses[k]) < 1e-4
        opt.step()
    for k in m.flat.params:
        d = (m.flat.w(k).detach().cpu() - want[k]).abs()
        assert float((d > 1e-5).float().mean()) < 0.01 and float(d.max()) < 7e-4, k


@pytest.mark.parametrize("cell", CELLS)
def test_checkpoint_round_trip_reference_envelope(tmp_path, cell):
    """save -> load into a fresh trainer (parameters and Adam moments), and a reference-style envelope written from a plain
    CPU module loads as well"""
    from erc_amd import bcrnn, checkpoint
    tr = _trainer(cell)
    b = tr.prepare_batch(_case([6, 2], 712, 2, 6, 5))
    for _ in range(2):
        tr.train_step(b)
    path = str(tmp_path / "bcrnn.ckpt")
    checkpoint.save(tr, path)
    ck = torch.load(path, weights_only=True)
    assert len(ck["optims"]["optim"]["state"]) == len(tr.model.flat.params) == 22
    tr2 = _trainer(cell, ["--seed=5"])
    checkpoint.load(tr2, path)
    assert torch.equal(_params(tr2), _params(tr))
    assert torch.equal(tr2.model.flat.exp_avg, tr.model.flat.exp_avg)
    ref = (bcrnn.LSTMModule if cell == "lstm" else bcrnn.GRUModule)(712, 100, 100, n_classes=6)
    fill_params(ref, 3)
    torch.save({"models": {"model": ref.state_dict()}, "optims": {}, "others": {}, "thtensor": {}, "nptensor": {}}, path)
    checkpoint.load(tr2, path)
    sd = tr2.model.state_dict()
    for k, v in ref.state_dict().items():
        assert torch.equal(sd[k].cpu(), v), k


def test_train_mm_cli_bcgru():
    """``python train_mm.py --module=bcgru`` end to end: finite losses, test metrics, replayed step graphs"""
    args = ["--module=bcgru", "--dataset=iemocap-cogmen-6", "--modality=atv", "--epoch=1", "--n_train=24", "--n_test=6",
            "--syn_min_len=12", "--syn_max_len=12", "--train.batch_size=4", "--test.batch_size=4"]
    res = subprocess.run([sys.executable, "train_mm.py"] + args, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]
    steps = [l for l in lines if "Lall" in l]
    epochs = [l for l in lines if "test" in l]
    assert len(steps) == 6 and len(epochs) == 1
    assert all(np.isfinite(l["Lall"]) for l in steps)
    assert epochs[0]["graph_replays"] > 0
