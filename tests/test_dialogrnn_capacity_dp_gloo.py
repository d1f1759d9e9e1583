"""world_size-2 gloo test (CPU) of the DialogueRNN capacity buckets under data parallelism: ranks whose shards have different
longest dialogues, one of them with a probe batch that fills its bucket exactly, precapture the SAME bucket list in the same
order (trainer.bucket_t_cap + DialogRNNTrainer.all_capacity_buckets), so every rank runs the same number of warm-up collectives
before training and one collective per step after.  The HIP runtime is replaced by a recorder that, like a real capture, does
not execute what it records; replaying it executes the step."""
import os
import types

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_dp_gloo import _free_port

D_M = 6


class _FakeGraph:
    def __init__(self, fn):
        self.fn = fn

    def replay(self):
        self.fn()


def _batch(lengths):
    B, T, N = len(lengths), max(lengths), sum(lengths)
    return dict(input_tensor=torch.zeros(T, B, D_M), speaker_tensor=torch.zeros(T, B, 2),
                text_length=torch.tensor(lengths, dtype=torch.int64), label=torch.zeros(N, dtype=torch.int64))


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from erc_amd import trainer as trainer_mod
    from erc_amd.dialogrnn import DialogRNNTrainer
    from track_mm.dialogrnn import DialogRNNParams
    p = DialogRNNParams().from_args(["--dataset=iemocap-cogmen-6", "--device=cpu", "--train.batch_size=8",
                                     "--capacity_buckets=True"])
    p.hidden_all = D_M
    tr = DialogRNNTrainer(p, "cpu")
    longest = [30, 33][rank]                       # this rank's shard: a different longest dialogue per rank
    loader = types.SimpleNamespace(dataset=types.SimpleNamespace(dialogs=[{"label": [0] * L} for L in (5, 12, longest, 7)]))
    tr.t_cap = trainer_mod.bucket_t_cap(loader, world, "cpu")
    calls = []

    def train_step(batch):
        t = torch.ones(1)
        dist.all_reduce(t)                         # the step's one collective
        assert float(t[0]) == world
        calls.append(int(batch["label"].shape[0]))
        return torch.zeros(4)
    tr.train_step = train_step

    class Graphs(trainer_mod.StepGraphs):
        def _capture(self, fn):
            return _FakeGraph(fn), torch.zeros(4)

        def _sync(self):
            pass

    g = Graphs(tr)
    # rank 1's probe fills its bucket exactly (B, T, N = 8, 33, 264): that batch itself runs the exact-shape step, the
    # bucket list must not shrink because of it
    probe = [_batch([5, 12, 30, 7, 9, 3, 20, 11]), _batch([33] * 8)][rank]
    assert (tr.capacity_bucket(probe) is None) == (rank == 1)
    g.precapture(probe)
    g.lazy = False
    warm = len(calls)
    keys = [k for k in g.cache]
    sizes = [[[3] * 8, [33] * 8, [20, 1, 2]], [[10] * 8, [33] * 8, [33] * 7 + [32]]][rank]
    for lens in sizes:
        g.step(_batch(lens))
    q.put((rank, tr.t_cap, warm, len(calls) - warm, keys, g.captures, g.replays, g.eager))
    dist.destroy_process_group()


def test_dialogrnn_buckets_are_the_same_on_every_rank():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(60)
    (r0, t0, w0, s0, k0, c0, rp0, e0), (r1, t1, w1, s1, k1, c1, rp1, e1) = res
    assert t0 == t1 == 33                          # the longest dialogue of every rank
    assert k0 == k1 and [k[3] for k in k0] == [128, 256, 264] and all(k[:3] == ("capacity", 8, 33) for k in k0)
    assert w0 == w1 == 3 and c0 == c1 == 3        # one warm-up collective per bucket on each rank, then its capture
    assert s0 == s1 == 3                           # one collective per step, replay or eager
    assert (rp0, e0) == (2, 1) and (rp1, e1) == (2, 1)    # the batches of their bucket's own shape ran eagerly
