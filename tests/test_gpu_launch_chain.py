"""GPU: a captured training step replayed as plain launches from C (engine.CapturedStep, csrc/launch_chain.hip) computes
what the replayed HIP graph computes, bit for bit, and captures that are not one path of the library's kernels keep graph
replay."""
import pytest
import torch

from erc_amd import capi
from tests.util_cases import cogmen_case_lengths

pytestmark = pytest.mark.gpu

DIMS = dict(a=100, t=768, v=512)          # D = 1380
LENGTHS = (1, 17, 21)                     # N = 39: three 16-row tiles, a ragged last tile, a one-node dialogue


def _trainer(compute, extra=()):
    from erc_amd.cogmen import COGMENTrainer
    from erc_amd.params import ERCParams
    torch.manual_seed(0)
    p = ERCParams().from_args(["--dataset=iemocap-cogmen-sbert-6", "--compute=" + compute] + list(extra))
    tr = COGMENTrainer(p, "cuda:0")
    assert tr.model.drop_p > 0.0          # dropout on: the masks follow the device-side RNG offset, which every replay advances
    return tr


def _state(tr, stats):
    """everything a step changes: parameters, both moments, the optimizer's counters (step, RNG offset, the workgroups' private
    step counts), BatchNorm's running statistics and batch counter, the health word, and the step's statistics"""
    torch.cuda.synchronize()
    flat = tr.model.flat
    out = {"data": flat.data, "exp_avg": flat.exp_avg, "exp_avg_sq": flat.exp_avg_sq, "optim.state": tr.optim.state,
           "grad_full": flat.grad_full, "stats": stats}
    out.update({k: v for k, v in tr.model.state_dict().items() if "running_" in k or "num_batches" in k})
    assert any("running_" in k for k in out)
    return {k: v.detach().clone() for k, v in out.items()}


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _assert_identical(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(_bytes(a[k]), _bytes(b[k])), k


def _graphed_run(monkeypatch, mode, compute, replays=4, steps=1, wrap=None):
    from erc_amd.engine import GraphedStep
    monkeypatch.setenv("ERC_STEP_REPLAY", mode)
    tr = _trainer(compute)
    batch = tr.prepare_batch(cogmen_case_lengths(LENGTHS, dims=DIMS, seed=3)["batch"])
    fn = (lambda: tr.train_step(batch)) if wrap is None else wrap(tr, batch)
    step = GraphedStep(fn, steps=steps)
    for _ in range(replays):
        stats = step()
    return step, _state(tr, stats)


@pytest.mark.parametrize("compute", ["bf16", "f32x32"])
def test_plain_launches_equal_graph_replay_bit_for_bit(monkeypatch, compute):
    g, by_graph = _graphed_run(monkeypatch, "graph", compute)
    c, by_chain = _graphed_run(monkeypatch, "launches", compute)
    assert g.captured.replays_by == "graph" and g.captured.chain == 0
    assert c.captured.replays_by == "launches" and c.captured.launches >= 1
    assert int(by_chain["optim.state"][0]) == 2 + 4            # two warm-up steps, four replayed ones
    _assert_identical(by_graph, by_chain)


def test_capacity_bucket_replayed_by_chain_honours_the_device_side_node_count(monkeypatch):
    """trainer.StepGraphs in capacity mode: two batches of different true N share one bucket (one captured step); the
    chain's launches are sized for the capacity and read the true node count from the device, like the graph's."""
    from erc_amd.trainer import StepGraphs
    runs = {}
    for mode in ("graph", "launches"):
        monkeypatch.setenv("ERC_STEP_REPLAY", mode)
        tr = _trainer("bf16", ["--train.batch_size=3"])
        tr.t_cap = 24
        a = tr.prepare_batch(cogmen_case_lengths(LENGTHS, dims=DIMS, seed=3)["batch"])              # N = 39
        b = tr.prepare_batch(cogmen_case_lengths((5, 9, 12), dims=DIMS, seed=4)["batch"])           # N = 26
        graphs = StepGraphs(tr)
        for batch in (a, b, a, b, a):                          # one eager step + the capture, then four replays
            stats = graphs.step(batch)
        assert (graphs.eager, graphs.captures, graphs.replays, len(graphs.cache)) == (1, 1, 4, 1)
        (ent, ) = graphs.cache.values()
        assert ent.capacity and ent.graph.replays_by == mode
        runs[mode] = _state(tr, stats)
    _assert_identical(runs["graph"], runs["launches"])


def test_two_steps_per_chain_equal_two_single_step_replays(monkeypatch):
    two, s2 = _graphed_run(monkeypatch, "launches", "bf16", replays=2, steps=2)
    one, s1 = _graphed_run(monkeypatch, "launches", "bf16", replays=4, steps=1)
    assert two.captured.launches == 2 * one.captured.launches
    _assert_identical(s1, s2)


def test_a_capture_with_a_memcpy_node_keeps_graph_replay(monkeypatch):
    src = torch.arange(4096, dtype=torch.float32, device="cuda:0")
    dst = torch.zeros_like(src)

    def with_copy(tr, batch):
        def fn():
            tr.train_step(batch)
            dst.copy_(src)                                     # contiguous device-to-device: a memcpy node
            return tr.train_step(batch)
        return fn

    monkeypatch.delenv("ERC_STEP_REPLAY", raising=False)
    from erc_amd.engine import GraphedStep
    tr = _trainer("bf16")
    batch = tr.prepare_batch(cogmen_case_lengths(LENGTHS, dims=DIMS, seed=3)["batch"])
    step = GraphedStep(with_copy(tr, batch), warmup=1)         # 2 steps of warm-up
    assert step.captured.replays_by == "graph" and "not a kernel node" in step.captured.refused
    dst.zero_()
    src += 1.0
    for _ in range(2):
        stats = step()                                         # 4 replayed steps
    fallback = _state(tr, stats)
    assert torch.equal(dst, src)
    _, by_graph = _graphed_run(monkeypatch, "graph", "bf16", replays=4)      # 2 warm-up + 4 replayed steps
    _assert_identical(by_graph, fallback)

    monkeypatch.setenv("ERC_STEP_REPLAY", "launches")
    tr2 = _trainer("bf16")
    with pytest.raises(capi.ErcGraftError, match="ERC_STEP_REPLAY=launches.*not a kernel node"):
        GraphedStep(with_copy(tr2, batch), warmup=1)


def _soft(x, y):
    capi.log_softmax_rows(x, x.shape[1], x.shape[1], x.shape[0], y, y.shape[1])


def test_a_straight_capture_of_library_kernels_is_a_chain_and_a_forked_one_is_not():
    x = torch.randn(64, 7, device="cuda:0")
    bufs = [torch.zeros_like(x) for _ in range(4)]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()

    straight = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(straight):
        _soft(x, bufs[0])
        _soft(bufs[0], bufs[1])
        _soft(bufs[1], bufs[2])
    chain, why = capi.chain_build(straight.raw_cuda_graph())
    assert chain != 0 and why is None and capi.chain_len(chain) == 3
    capi.chain_run(chain)
    torch.cuda.synchronize()
    ref = torch.log_softmax(torch.log_softmax(torch.log_softmax(x, 1), 1), 1)
    assert float((bufs[2] - ref).abs().max()) < 1e-5
    capi.chain_free(chain)

    # x -> a, then b and c side by side on two streams, then d behind both: a fork and a join.  Eligibility only -- it is
    # neither replayed as a chain nor as a graph here
    forked = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(forked):
        main = torch.cuda.current_stream()
        _soft(x, bufs[0])
        side.wait_stream(main)
        with torch.cuda.stream(side):
            _soft(bufs[0], bufs[1])
        _soft(bufs[0], bufs[2])
        main.wait_stream(side)
        _soft(bufs[1], bufs[3])
    chain, why = capi.chain_build(forked.raw_cuda_graph())
    assert chain == 0 and ("path" in why or "successors" in why or "predecessors" in why), why
