"""GPU: CIM on CMU-MOSEI (--dataset=mosei-cim-2) -- the multi-task loss kernel (erc_ce_bce_multitask) against torch in fp64,
the multi-task module against the reference's own CIMModule (tests/golden/cim_mosei_c2.npz) and the CPU restatement with
torch Adam, the single-task MOSEI path, HIP-graph replay, checkpoints with cls7's Adam state and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from erc_amd import capi
from tests.cim_mosei_oracle import cim_mosei_loss_and_grads
from tests.cim_oracle import FEATURE, adam_step
from tests.util_cases import check_grad_digest, fill_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = dict(a=74, t=300, v=35)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    capi.lib()


def _err(a, b):
    return float((a.detach().cpu() - b).abs().max())


# ----------------------------------------------------------------------------------------------------- loss kernel
def _loss_case(N, C, seed):
    g = torch.Generator().manual_seed(seed)
    pitch = C + 7 + 3                                    # row pitch wider than the C + 7 columns
    x = torch.randn(N, pitch, generator=g, dtype=torch.float64) * 4
    big = torch.rand(N, pitch, generator=g) < 0.1
    x[big] = (torch.rand(int(big.sum()), generator=g, dtype=torch.float64) * 2 - 1) * 100
    x[0, :C + 7] = torch.tensor([100.0, -100.0] + [0.0] * (C - 2) + [100, -100, 99.5, -99.5, 80.5, -80.5, 0.0])[:C + 7]
    x = x.float()
    labels = torch.randint(0, C, (N,), generator=g)
    emo_wide = (torch.rand(N, 9, generator=g) < 0.3).long()    # emo_label read through a row pitch of 9
    emo_wide[::3, :7] = 0
    emo_wide[1::5, :7] = 1
    return x, labels, emo_wide


def _run_kernel(x, labels, emo_wide, C, w_ce=1.0, w_bce=1.0, gs=1.0):
    N, pitch = x.shape
    xd, yd, ed = x.to(DEV), labels.to(DEV), emo_wide.to(DEV)
    d = torch.full((N, pitch), 7.0, device=DEV)
    stats = torch.zeros(256, device=DEV)
    capi.ce_bce_multitask(xd, pitch, C, N, yd, ed[:, :7], ed.stride(0), w_ce, w_bce, gs, d, pitch, stats)
    torch.cuda.synchronize()
    return d.cpu(), stats.cpu()


@pytest.mark.parametrize("N,C", [(1, 2), (7, 2), (1000, 2), (40000, 2), (1000, 5)])
def test_loss_kernel_matches_torch_fp64(N, C):
    x, labels, emo_wide = _loss_case(N, C, N + C)
    d, stats = _run_kernel(x, labels, emo_wide, C)
    z = x[:, :C + 7].double().requires_grad_(True)
    emo = emo_wide[:, :7].double()
    lce = F.cross_entropy(z[:, :C], labels)
    lmulti = F.binary_cross_entropy_with_logits(z[:, C:], emo)
    (lce + lmulti).backward()
    for got, want in ((stats[0], (lce + lmulti).detach()), (stats[2], lce.detach()), (stats[3], lmulti.detach())):
        assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want)) + 1e-30, (float(got), float(want))
    assert int(stats[1]) == int((z[:, :C].argmax(-1) == labels).sum())
    assert torch.isfinite(stats[:4]).all()
    gd = z.grad.float()
    for lo, hi in ((0, C), (C, C + 7)):
        scale = float(gd[:, lo:hi].abs().max())
        assert _err(d[:, lo:hi], gd[:, lo:hi]) <= 1e-6 * scale, (lo, hi)
    assert torch.equal(d[:, C + 7:], torch.full((N, 3), 7.0))      # columns past C + 7 are never written
    # bit-identical second run
    d2, stats2 = _run_kernel(x, labels, emo_wide, C)
    assert torch.equal(d, d2) and torch.equal(stats[:4], stats2[:4])


def test_loss_kernel_term_weights_and_grad_scale():
    N, C = 1000, 2
    x, labels, emo_wide = _loss_case(N, C, 3)
    d, st = _run_kernel(x, labels, emo_wide, C)
    d0, s0 = _run_kernel(x, labels, emo_wide, C, w_bce=0.0)
    assert torch.equal(d0[:, C:C + 7], torch.zeros(N, 7)) and torch.equal(d0[:, :C], d[:, :C])
    assert float(s0[0]) == float(st[2]) and float(s0[3]) == float(st[3])
    d1, s1 = _run_kernel(x, labels, emo_wide, C, w_ce=0.0)
    assert torch.equal(d1[:, :C], torch.zeros(N, C)) and torch.equal(d1[:, C:C + 7], d[:, C:C + 7])
    assert float(s1[0]) == float(st[3])
    d2, _ = _run_kernel(x, labels, emo_wide, C, gs=0.5)
    assert _err(d2[:, :C + 7], d[:, :C + 7] * 0.5) <= 1e-7 * float(d.abs().max())


# ----------------------------------------------------------------------------------------------------- module
def _module(dims, C, seed, multitask=True, drop=0.3):
    from erc_amd.cim import CIMModule
    m = CIMModule(dims["t"], dims["a"], dims["v"], 200, C, drop0=drop, drop1=drop, multitask=multitask)
    fill_params(m, seed)
    P = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.finalize(DEV), P


def _gpu(batch):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _case(lens, dims, seed):
    g = torch.Generator().manual_seed(seed)
    B, T, N = len(lens), max(lens), sum(lens)
    batch = {"text_length": torch.tensor(lens, dtype=torch.int64),
             "attention_mask": (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float()}
    for m in "atv":
        x = torch.randn(B, T, dims[m], generator=g) * 0.5
        for b, L in enumerate(lens):
            x[b, L:] = 0.0
        batch[FEATURE[m]] = x
    batch["label"] = torch.randint(0, 2, (N,), generator=g)
    emo = (torch.rand(N, 7, generator=g) < 0.2).long()
    emo[:, 6] = 0
    emo[(emo.sum(1) == 0), 6] = 1
    batch["emo_label"] = emo
    batch["senti2_label"] = batch["label"].clone()
    return batch


def _check_grads(m, grads, tol=1e-3):
    for name, g in grads.items():
        if name.startswith("rnn_adapter."):
            assert g is None, name
            continue
        got = m.flat.g(name).detach().cpu()
        scale = float(g.abs().max()) + 1e-6
        assert _err(got, g) <= tol * scale, (name, _err(got, g), scale)


def test_module_matches_reference_fixture(golden):
    fx = golden("cim_mosei_c2")
    dims = dict(zip("atv", (int(v) for v in fx["dims"])))
    m, P = _module(dims, int(fx["n_classes"]), int(fx["param_seed"]))
    batch = _gpu({k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("in_")})
    m.eval()
    l2, l7 = m(**batch)
    assert _err(l2, torch.from_numpy(fx["logits2"])) < 1e-4
    assert _err(l7, torch.from_numpy(fx["logits7"])) < 1e-4
    stats = m.loss_and_grads(batch).cpu()
    for i, k in ((0, "Lall"), (2, "Lce"), (3, "Lmulti")):
        assert abs(float(stats[i]) - float(fx[k])) < 1e-5, k
    live = [(k, m.flat.g(k)) for k in m.flat.params]
    assert {"cls7.weight", "cls7.bias"} <= set(m.flat.params)
    assert check_grad_digest(fx, live, 1e-3) < 1e-3
    none = sorted(k for k, _ in m.named_parameters() if k not in m.flat.params)
    assert none == sorted(str(s) for s in fx["grad_none"])


@pytest.mark.parametrize("dropout", [False, True])
def test_adam_step_matches_oracle_b16_t98(dropout):
    """B = 16, T = 98 at the MOSEI feature widths: loss terms, gradients (cls7 included) and one FusedAdam step against
    the restatement + torch.optim.Adam; dropout mode with the masks the step applied; rnn_adapter.* stays put"""
    from erc_amd.engine import FusedAdam
    rng = np.random.RandomState(2)
    lens = [98] + rng.randint(1, 99, size=15).tolist()
    batch = _case(lens, DIMS, 6)
    m, P = _module(DIMS, 2, 12)
    m.train(dropout)
    opt = FusedAdam(m.flat, lr=1e-3)
    m.rng_state = opt.rng_state
    stats = m.loss_and_grads(_gpu(batch)).cpu()
    masks = None
    if dropout:
        ws, keep = m._last_ws, 1.0 / 0.7
        masks = {}
        for i, mod in enumerate("avt"):
            hd = ws["Hdrop"][i].cpu()
            masks["drop0_" + mod] = (hd != 0).float() * keep
            pre = hd @ P["adapter.%s.0.weight" % mod].t() + P["adapter.%s.0.bias" % mod]
            dense = ws["merged"][:, 600 + 100 * i:700 + 100 * i].cpu()
            masks["drop1_" + mod] = torch.where((dense != 0) | (pre <= 0), torch.full_like(pre, keep), torch.zeros_like(pre))
    losses, _, _, grads, _ = cim_mosei_loss_and_grads(P, batch, masks)
    for i, k in ((0, "Lall"), (2, "Lce"), (3, "Lmulti")):
        assert abs(float(stats[i]) - float(losses[k])) < 1e-5 * max(1.0, abs(float(losses[k]))), k
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
        if k.startswith("rnn_adapter."):
            assert torch.equal(sd[k].cpu(), P[k]), k
        if k.startswith("cls7."):
            assert not torch.equal(sd[k].cpu(), P[k]), k


# ----------------------------------------------------------------------------------------------------- trainer level
def _trainer(extra=()):
    from track_mm.cim import CIMParams
    from erc_amd.cim import CIMTrainer
    return CIMTrainer(CIMParams().from_args(["--dataset=mosei-cim-2"] + list(extra)), DEV)


def test_single_task_mosei_path():
    """--apply_multi=False: cross entropy only (the single-task launch list), cls7 stays dead"""
    tr = _trainer(["--apply_multi=False"])
    assert not tr.model.multitask and "cls7.weight" not in tr.model.flat.params
    batch = _case([9, 1, 30], DIMS, 4)
    w7 = tr.model.cls7.weight.detach().clone()
    P = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
    tr.model.eval()
    stats = tr.model.loss_and_grads(tr.prepare_batch(batch)).cpu()
    losses, _, _, grads, _ = cim_mosei_loss_and_grads(P, batch, apply_multi=False)
    assert abs(float(stats[0]) - float(losses["Lce"])) < 1e-5
    assert grads["cls7.weight"] is None
    for _ in range(2):
        tr.train_step(tr.prepare_batch(batch))
    assert torch.equal(tr.model.cls7.weight.detach(), w7)


def test_captured_step_equals_eager():
    from erc_amd.trainer import StepGraphs
    batch = _case([12, 40, 3, 25], DIMS, 1)
    tr = _trainer()
    b = tr.prepare_batch(batch)
    losses = [tr.train_step(b)[:4].clone() for _ in range(4)]
    torch.cuda.synchronize()
    eager = tr.model.flat.data.detach().clone()
    tr2 = _trainer()
    graphs = StepGraphs(tr2)
    b2 = tr2.prepare_batch(batch)
    got = [graphs.step(b2)[:4].clone() for _ in range(4)]
    torch.cuda.synchronize()
    assert graphs.replays == 2 and graphs.captures == 1
    assert torch.equal(tr2.model.flat.data, eager)
    assert all(torch.equal(a, c) for a, c in zip(losses, got))


def test_checkpoint_has_cls7_adam_state_and_loads_into_torch_adam(tmp_path):
    from erc_amd import checkpoint
    from erc_amd.cim import CIMModule
    tr = _trainer()
    b = tr.prepare_batch(_case([6, 2, 11], DIMS, 5))
    for _ in range(2):
        tr.train_step(b)
    path = str(tmp_path / "cim_mosei.ckpt")
    checkpoint.save(tr, path)
    ck = torch.load(path, weights_only=True)
    names = [n for n, _ in tr.model.named_parameters()]
    state = ck["optims"]["optim"]["state"]
    i7w, i7b = names.index("cls7.weight"), names.index("cls7.bias")
    assert i7w in state and i7b in state and len(state) == len(tr.model.flat.params)
    assert not any(n.startswith("rnn_adapter.") for i, n in enumerate(names) if i in state)
    assert torch.equal(state[i7w]["exp_avg"], tr.model.flat.view(tr.model.flat.exp_avg, "cls7.weight").cpu())
    tr2 = _trainer(["--seed=5"])
    checkpoint.load(tr2, path)
    assert torch.equal(tr2.model.flat.data, tr.model.flat.data)
    assert torch.equal(tr2.model.flat.exp_avg_sq, tr.model.flat.exp_avg_sq)
    ref = CIMModule(300, 74, 35, 200, 2)            # reference-shaped module, plain CPU parameters
    ref.load_state_dict(ck["models"]["model"])
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    opt.load_state_dict(ck["optims"]["optim"])
    assert torch.equal(opt.state[ref.cls7.weight]["exp_avg"], state[i7w]["exp_avg"])
    assert ref.rnn_adapter["t"].weight not in opt.state


def _cli(args, timeout=900):
    res = subprocess.run([sys.executable, "train_mm.py", "--module=cim", "--dataset=mosei-cim-2"] + args, cwd=REPO,
                         capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]
    steps = [l for l in lines if "Lall" in l]
    epochs = [l for l in lines if "test" in l]
    assert len(epochs) == 1 and steps
    assert all(np.isfinite(l["Lall"]) and np.isfinite(l["Lce"]) and np.isfinite(l["Lmulti"]) for l in steps)
    assert all(abs(l["Lall"] - l["Lce"] - l["Lmulti"]) < 1e-5 * max(1.0, l["Lall"]) for l in steps)
    me = epochs[0]["multiemo"]
    assert len(me["acc"]) == 7 and len(me["f1"]) == 7 and len(me["wa"]) == 7 and np.isfinite(me["mean_acc"])
    return steps, epochs[0]


@pytest.mark.parametrize("extra", [[], ["--device_collate"]])
def test_train_mm_cli_synthetic(extra):
    steps, ep = _cli(["--epoch=1", "--n_train=24", "--n_test=6", "--syn_min_len=12", "--syn_max_len=12",
                      "--train.batch_size=4", "--test.batch_size=4"] + extra)
    assert len(steps) == 6 and ep["graph_replays"] > 0


def test_train_mm_cli_real_reader():
    steps, ep = _cli(["--epoch=1", "--synthetic=False", "--data_root=tests/golden/mosei_cim", "--train.batch_size=2"])
    assert len(steps) == 2
