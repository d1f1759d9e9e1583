"""DialogueGCN in capacity mode (DGCNModule.dynamic_n) on the GPU: the step sized for bucket capacities (B_cap dialogue slots,
T_cap, N_cap rows) against the exact-shape step, the rows past the batch, several training steps with dropout and Adam, the
bucketed and the resident training loops of train_mm.py, and a bucket's captured graph replayed from the same state."""
import math

import pytest
import torch

from tests.test_gpu_cogmen import _run_cli
from tests.util_cases import make_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _trainer(S, compute, batch_size=8, lr=None):
    from erc_amd.dgcn import DGCNTrainer
    from erc_amd.params import ERCParams
    torch.manual_seed(0)
    ds = ["--dataset=meld-mmgcn-7", "--loss_weights=False"] if S == 9 else ["--dataset=iemocap-cogmen-6"]
    p = ERCParams().from_args(ds + ["--compute=" + compute, "--train.batch_size=%d" % batch_size] +
                              (["--optim.lr=%g" % lr] if lr is not None else []))
    tr = DGCNTrainer(p, DEV)
    tr.model.relation_space = False      # (two speakers default to relation space; capacity mode runs the basis-space tiles)
    return tr, p


def _batch(tr, p, B, min_len, max_len, seed):
    return tr.prepare_batch(make_batch(B, p.dims(), n_speakers=p.n_speakers, n_classes=p.n_classes, min_len=min_len,
                                       max_len=max_len, seed=seed))


def _snapshot(tr):
    f = tr.model.flat
    return [t.clone() for t in (f.data, f.exp_avg, f.exp_avg_sq, tr.optim.state)]


@pytest.mark.parametrize("S", [2, 9])
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_capacity_step_equals_exact_step(compute, S):
    """The batch sits in capacity-sized static buffers -- fewer dialogues than slots (length 0), a longer T, N far below
    N_cap -- and the launches read the true node count from the device.  Loss, #correct, weight sum and every gradient equal
    the exact-shape step (gradients up to the fp32 summation order of the weight-gradient splits, which are cut for N_cap);
    the rows past N hold finite values of an earlier, larger batch in the forward buffers and exact zeros in every gradient
    buffer the weight-gradient launch reads.  Dropout is on: masks are keyed by compact row in both paths."""
    outs = []
    for cap in (False, True):
        tr, p = _trainer(S, compute)
        big = _batch(tr, p, 8, 20, 40, seed=3)
        small = _batch(tr, p, 5, 2, 12, seed=4)
        lr, tr.optim.lr = tr.optim.lr, 0.0   # the first step only fills the buffers: the weights of the compared step are the same
        if cap:
            tr.t_cap = 48
            key, make, fill = tr.capacity_bucket(big)
            n_big = int(big["label"].shape[0])
            assert key == ("capacity", 8, 48, -(-n_big // tr.N_BUCKET) * tr.N_BUCKET)
            static = make()
            tr.model.dynamic_n = True
            fill(static, big)
            tr.train_step(static)                 # leaves rows of a LARGER batch behind in every buffer of the bucket
            fill(static, small)
            tr.optim.lr = lr
            stats = tr.train_step(static).cpu()
            tr.model.dynamic_n = False
        else:
            tr.train_step(big)
            tr.optim.lr = lr
            stats = tr.train_step(small).cpu()
        n = int(small["label"].shape[0])
        ws = tr.model._last_ws
        outs.append((stats, tr.model.flat.grad.clone(), ws["logits"][:n].clone(), ws, n))
    (s0, g0, l0, _, n), (s1, g1, l1, ws, _) = outs
    N_cap = ws["Xc"].shape[0]
    assert N_cap >= 2 * n
    assert abs(float(s0[0]) - float(s1[0])) <= 1e-5 * abs(float(s0[0])) and float(s0[1]) == float(s1[1])
    assert abs(float(s0[2]) - float(s1[2])) <= 1e-5 * abs(float(s0[2]))
    assert float((l0 - l1).abs().max()) < 1e-5
    assert float((g0 - g1).abs().max()) <= 2e-5 * float(g0.abs().max())
    lstm = ws["lstm:rnn.rnn."]
    grads = {k: ws[k] for k in ("dlogits", "dZc", "dXc", "dAGG", "dHc", "DATT")}
    grads.update(dGX0=lstm["dGX"][0], dGX1=lstm["dGX"][1], dH0d=lstm["dH0d"])
    for name, t in grads.items():
        assert t.shape[0] == N_cap and int((t[n:] != 0).sum()) == 0, name
    fwd = {k: ws[k] for k in ("Xc", "ATT", "Hc", "AGG", "Zc", "logits", "Z")}
    fwd.update(GX0=lstm["GX"][0], GX1=lstm["GX"][1], H0d=lstm["H0d"])
    for name, t in fwd.items():
        assert bool(torch.isfinite(t).all()), name


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_three_capacity_steps_with_dropout_and_adam_equal_the_exact_path(compute):
    """Three training steps (dropout on, Adam updating) through ONE bucket's static buffers equal three exact-shape steps:
    the optimizer's dropout offset advances the same way, so the masks of every step agree.  The check is each step's loss
    and #correct: the weights themselves are no measure here, since Adam's first steps move every entry by about lr
    whatever the size of its gradient, so two near-equal gradients that differ in the sign of a near-zero entry end up
    2 lr apart there."""
    runs = []
    for cap in (False, True):
        tr, p = _trainer(9, compute, lr=3e-4)
        batches = [_batch(tr, p, B, lo, hi, seed) for B, lo, hi, seed in ((8, 5, 30, 11), (6, 3, 20, 12), (7, 1, 33, 13))]
        losses = []
        if cap:
            tr.t_cap = 40
            key, make, fill = tr.capacity_bucket(max(batches, key=lambda b: int(b["label"].shape[0])))
            static = make()
            tr.model.dynamic_n = True
            for b in batches:
                fill(static, b)
                losses.append(tr.train_step(static).cpu())
            tr.model.dynamic_n = False
        else:
            for b in batches:
                losses.append(tr.train_step(b).cpu())
        runs.append(losses)
    for a, b in zip(*runs):
        assert abs(float(a[0]) - float(b[0])) <= 1e-5 * abs(float(a[0])) and float(a[1]) == float(b[1])
        assert abs(float(a[2]) - float(b[2])) <= 1e-5 * abs(float(a[2]))


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_training_loop_default_sampling_replays_capacity_buckets(compute):
    """trainer.run with the reference's sampling (reshuffled dialogues, smaller last batch): batch shapes never repeat, the
    capacity buckets do -- one eager step per bucket, every other step a replay, per-step losses IDENTICAL to the same loop
    with capture switched off (same buckets, every step eager on the static buffers)."""
    args = ["--module=dgcn", "--dataset=meld-mmgcn-7", "--loss_weights=False", "--epoch=3", "--n_train=44", "--n_test=6",
            "--train.batch_size=8", "--test.batch_size=8", "--compute=" + compute]
    g_loss, g_ep = _run_cli(args)
    e_loss, e_ep = _run_cli(args + ["--graph_capture=False"])
    assert len(g_loss) == 18 and g_loss == e_loss
    assert all(math.isfinite(v) for v in g_loss)
    assert e_ep[2]["graph_replays"] == 0 and e_ep[2]["graphs_captured"] == 0
    assert g_ep[2]["graph_replays"] + g_ep[2]["eager_steps"] == 18
    assert g_ep[2]["eager_steps"] == g_ep[2]["graphs_captured"]            # one eager step per bucket
    assert g_ep[2]["graph_replays"] >= 10


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_resident_epochs_equal_the_collated_loop(compute):
    """``--resident`` for DialogueGCN: the graph build reads lengths and speakers through the 2 B int32 descriptor, the layer-0
    LSTM projection gathers the store's feature rows through node_row and the tail reads the labels through the same map.
    Same permutations as the device-collated loop; epoch mean losses agree (the weight-gradient launch may cut K
    differently), every step after a bucket's first is a replay."""
    args = ["--module=dgcn", "--dataset=meld-mmgcn-7", "--loss_weights=False", "--epoch=3", "--n_train=44", "--n_test=6",
            "--train.batch_size=8", "--test.batch_size=8", "--compute=" + compute, "--device_collate"]
    c_loss, c_ep = _run_cli(args)
    r_loss, r_ep = _run_cli(args + ["--resident"])
    assert len(c_loss) == 18 and len(r_loss) == 3
    for e in range(3):
        want = sum(c_loss[6 * e:6 * e + 6]) / 6
        assert abs(r_loss[e] - want) < 1e-5 * max(1.0, abs(want)), (e, r_loss[e], want)
    assert r_ep[2]["graph_replays"] + r_ep[2]["eager_steps"] == 18
    assert r_ep[2]["eager_steps"] == r_ep[2]["graphs_captured"] and r_ep[2]["graph_replays"] >= 10
    assert all(abs(a["test"]["acc"] - b["test"]["acc"]) <= 0.02 for a, b in zip(r_ep, c_ep))


def test_bucket_graph_replays_bit_identically():
    """A bucket's captured step replayed twice from the same state (parameters, Adam moments, step count and dropout offset)
    gives bit-identical statistics, parameters and moments: nothing in the capacity step depends on launch timing."""
    tr, p = _trainer(9, "f32", lr=3e-4)
    b = _batch(tr, p, 8, 4, 30, seed=21)
    tr.t_cap = 36
    key, make, fill = tr.capacity_bucket(b)
    static = make()
    fill(static, b)
    tr.model.dynamic_n = True
    tr.train_step(static)                     # eager first step on the static buffers: workspace and tables exist
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = tr.train_step(static)
    tr.model.dynamic_n = False
    fill(static, _batch(tr, p, 6, 2, 25, seed=22))
    snap = _snapshot(tr)
    res = []
    for _ in range(2):
        for t, keep in zip((tr.model.flat.data, tr.model.flat.exp_avg, tr.model.flat.exp_avg_sq, tr.optim.state), snap):
            t.copy_(keep)
        g.replay()
        torch.cuda.synchronize()
        res.append([out.clone()] + [t.clone() for t in (tr.model.flat.data, tr.model.flat.exp_avg, tr.model.flat.exp_avg_sq)])
    for a, c in zip(*res):
        assert torch.equal(a, c)
    assert not torch.equal(res[0][1], snap[0])            # the replay trained
