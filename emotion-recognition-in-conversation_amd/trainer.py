"""Minimal run driver behind the reference's plugin surface.

Replaces what ``mmbase.main`` gets from lumo (track_mm/mmbase.py:483-499,
lumo/trainer/trainer.py:402-442): build params from the command line, build the
data loaders (``ERCCollate`` batch layout), loop ``epoch`` times over
``train_step``, evaluate with ``test_step`` after every epoch
(EvalCallback(test_per_epoch=1), mmbase.py:136) and report the sklearn metric
set of mmbase.py:253-323 (on CMU-MOSEI with ``mosei_metric='multiemo'``: on the binary sentiment, plus the per-emotion
block of the multi-label head, ``multiemo_report``).  One process per GPU; under torch.distributed the
trainers all-reduce the flat gradient buffer (RCCL) once per step.

There are no dataset pickles offline: ``--synthetic`` (default) draws seeded
IEMOCAP-/MELD-shaped dialogues (synthetic.py); ``--synthetic=False --data_root=<dir>``
(or $ERC_IEMOCAP_ROOT / $ERC_MELD_ROOT) reads the reference's feature pickles
(datasets.py).  ``--device_collate`` keeps the dialogues resident in HBM and builds
every batch on the device (datasets.DeviceDialogueStore) instead of in a DataLoader.
``--resident`` runs the training epochs from that store (ResidentEpochs); ``--resident_eval`` the test epochs too,
scored on the device (ResidentEval, report_from_cm).
"""
import contextlib
import dataclasses
import json
import os
import sys
import time

import numpy as np
import torch
from torch.utils.data import DataLoader

from . import capi
from .capacity import node_capacity
from .collate import ERCCollate
from .engine import CapturedStep
from .synthetic import make_dialogues, make_mosei_dialogues


def fix_seed(seed):
    """What ``trainer.rnd.mark(seed)`` amounts to on a first run (lumo/trainer/rnd.py:17-33, lumo/utils/random.py:22-43):
    python / numpy / torch generators seeded, so parameter initialisation and shuffling repeat run to run."""
    import random
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


class ListDataset(torch.utils.data.Dataset):
    """Yields 1-element lists like lumo's DatasetBuilder (lumo/data/builder.py:100-101)."""

    def __init__(self, dialogs):
        self.dialogs = dialogs

    def __len__(self):
        return len(self.dialogs)

    def __getitem__(self, i):
        return [self.dialogs[i]]


class StoreLoader:
    """DataLoader-shaped iterator over a DeviceDialogueStore: seeded shuffle on the host, batch assembly on the device."""

    def __init__(self, store, batch_size, shuffle, seed):
        self.store, self.batch_size, self.shuffle = store, batch_size, shuffle
        self.gen = torch.Generator().manual_seed(seed)

    def __len__(self):
        return -(-len(self.store) // self.batch_size)

    def __iter__(self):
        n = len(self.store)
        order = torch.randperm(n, generator=self.gen) if self.shuffle else torch.arange(n)
        for i in range(0, n, self.batch_size):
            yield self.store.batch(order[i:i + self.batch_size])


def shard_dialogues(dialogs, rank, world):
    """This rank's share of the training dialogues, EQUAL in size on every rank: the list is padded to a multiple of
    ``world`` by wrapping around (what torch's DistributedSampler -- the sampler accelerate gives the reference,
    lumo/trainer/trainer.py:377-384 -- does with drop_last=False), then dealt round-robin.  Equal shard sizes mean an
    equal number of batches, hence an equal number of gradient all-reduces per epoch on every rank: with plain
    ``dialogs[rank::world]`` 259 dialogues over 2 ranks at batch 43 gave 4 vs 3 steps and the rank with the extra
    batch waited in its all-reduce forever."""
    n = len(dialogs)
    if world <= 1 or n == 0:
        return list(dialogs)
    total = -(-n // world) * world
    idx = [i % n for i in range(total)]
    return [dialogs[i] for i in idx[rank::world]]


def load_dialogues(params, rank=0, world=1):
    """(train dialogues of this rank, test dialogues)."""
    if not params.get("synthetic", True):
        from .datasets import read_dialogues
        roots = params.get("data_root", None)
        train = read_dialogues(params.dataset, "train", roots)
        return shard_dialogues(train, rank, world), read_dialogues(params.dataset, "test", roots)
    meld, mosei = "meld" in params.dataset, "mosei" in params.dataset
    lo, hi = (1, 33) if meld else (1, 98) if mosei else (20, 110)
    lo, hi = int(params.get("syn_min_len", lo)), int(params.get("syn_max_len", hi))     # (tests: equal lengths -> repeating shapes)
    if mosei:
        mk = lambda n, seed: make_mosei_dialogues(n, params.dims(), min_len=lo, max_len=hi, seed=seed)
        return mk(params.n_train, params.seed + 1000 * rank), mk(params.n_test, params.seed + 7)
    mk = lambda n, seed: make_dialogues(n, params.dims(), n_speakers=params.n_speakers, n_classes=params.n_classes,
                                        min_len=lo, max_len=hi, seed=seed)
    return mk(params.n_train, params.seed + 1000 * rank), mk(params.n_test, params.seed + 7)   # every rank draws its own


def make_loaders(params, rank=0, world=1, device=None):
    train_d, test_d = load_dialogues(params, rank, world)
    if params.get("device_collate", False):
        from .datasets import DeviceDialogueStore
        dt = torch.bfloat16 if params.compute == "bf16" else torch.float32
        return (StoreLoader(DeviceDialogueStore(train_d, params, device, dt), params.train.batch_size, True, params.seed + rank),
                StoreLoader(DeviceDialogueStore(test_d, params, device, dt), params.test.batch_size, False, 0))
    train, test = ListDataset(train_d), ListDataset(test_d)
    collate = ERCCollate(params)
    gen = torch.Generator().manual_seed(params.seed + rank)
    tl = DataLoader(train, batch_size=params.train.batch_size, shuffle=True, collate_fn=collate,
                    num_workers=params.train.get("num_workers", 0) or 0, generator=gen)
    el = DataLoader(test, batch_size=params.test.batch_size, shuffle=False, collate_fn=collate, num_workers=0)
    return tl, el


def longest_dialogue(loader):
    """longest training dialogue of this rank's split"""
    if isinstance(loader, StoreLoader):
        return int(loader.store.lengths.max())
    return max(len(d["label"]) for d in loader.dataset.dialogs)


def bucket_t_cap(loader, world, device):
    """The T capacity of the capacity buckets: the longest training dialogue of ALL ranks.  Under data parallelism every
    rank precaptures the same bucket list (StepGraphs.precapture), and that list depends on T_cap; with each rank's own
    longest dialogue the ranks would run different numbers of warm-up collectives.  (A collective: every rank calls it.)"""
    t = longest_dialogue(loader)
    if world > 1:
        import torch.distributed as dist
        v = torch.tensor([t], dtype=torch.int64, device=device)
        dist.all_reduce(v, op=dist.ReduceOp.MAX)
        t = int(v.item())
    return t


def first_batch(loader):
    """a batch of the loader's shape WITHOUT advancing its shuffling generator (the epochs must see the same permutations
    whether or not a probe was drawn)"""
    if isinstance(loader, StoreLoader):
        return loader.store.batch(torch.arange(min(loader.batch_size, len(loader.store))))
    n = min(loader.batch_size, len(loader.dataset))
    return loader.collate_fn([loader.dataset[i] for i in range(n)])


class FixedBatches:
    """``--fixed_batches``: the training batches are collated once and kept on the device; an epoch visits them in a
    freshly shuffled ORDER.  Batch shapes then repeat every epoch, so every step after the first epoch is one HIP-graph
    replay with no host-side collate and no host-to-device copy.  (Opt-in: the reference reshuffles the dialogues
    themselves every epoch.)"""

    def __init__(self, loader, trainer, seed):
        self.batches = [(int(b["label"].shape[0]), trainer.prepare_batch(b)) for b in loader]
        self.gen = torch.Generator().manual_seed(seed)

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for i in torch.randperm(len(self.batches), generator=self.gen).tolist():
            yield i, self.batches[i]


def batch_table(lengths, offsets, order, B):
    """The int32 table [steps, 2 B] of an epoch that visits the store's dialogues in ``order``, B per step: a row holds the
    lengths, then the first store rows of its batch's dialogues; 0 in the empty slots of a smaller last batch.
    ``lengths`` / ``offsets``: int32 arrays, one entry per dialogue."""
    n = len(order)
    steps = -(-n // B)
    flat = np.zeros((2, steps * B), dtype=np.int32)
    flat[0, :n], flat[1, :n] = lengths[order], offsets[order]
    return np.concatenate([flat[0].reshape(steps, B), flat[1].reshape(steps, B)], axis=1)


@contextlib.contextmanager
def dynamic_n(model, on=True):
    """capacity mode inside the block: the module's launches are sized for the capacities and read the batch's true node
    count from the device (``model.dynamic_n``); off again afterwards, whatever the block raised"""
    if on:
        model.dynamic_n = True
    try:
        yield
    finally:
        if on:
            model.dynamic_n = False


@dataclasses.dataclass
class GraphEntry:
    """what StepGraphs keeps per key"""
    static: dict               # the static input buffers the step runs on
    fill: object               # fill(static, batch) copies a batch in; None: the batch IS the static buffers (FixedBatches)
    capacity: bool             # a capacity bucket (the step runs under dynamic_n) or an exact batch shape
    seen: int = 0              # how many times the key has occurred
    graph: object = None       # the captured step, once there is one
    out: object = None         # the captured step's output (the device stats tensor)
    workspace: object = None   # the module's workspace of this key: the graph holds raw pointers into it


class StepGraphs:
    """Captured HIP graphs of the whole training step, least-recently-used eviction.

    * CAPACITY BUCKETS (trainers with capacity.CapacityBuckets: COGMEN in the bf16 compute mode, DialogueGCN on its default
      path, bc-LSTM / bc-GRU, DialogueRNN and DAG-ERC with ``--capacity_buckets=True`` or ``--resident``).  The reference reshuffles
      the dialogues every epoch and its last batch is smaller (lumo/trainer/trainer.py:429-442, mmbase.py:468), so (B, T, N)
      almost never repeats.  A bucket is a set of static capacity-sized input buffers -- ``batch_size`` dialogues (missing
      ones get length 0), the longest training dialogue of every rank, N rounded up to the trainer's N_BUCKET (COGMEN 256,
      DialogueGCN and bc-LSTM / bc-GRU 128; DAG-ERC always B * T: none of its launches scales with N) -- plus one graph captured
      over them; the step's kernels read the true node count from the device (COGMENModule.dynamic_n; the bc-RNN scans also
      the batch's longest dialogue), so every batch
      that fits replays that graph: a reshuffled epoch hits a handful of graphs.
    * otherwise one graph per exact batch shape, captured when the shape shows up the SECOND time (under shuffling most
      shapes never repeat: capturing each one would cost a synchronisation + instantiation per step and pin a workspace).

    Whatever the key, its entry is a ``GraphEntry`` and its first step is a real training step run EAGERLY ON THE GRAPH'S OWN
    STATIC BUFFERS (the batch is copied in first): every pointer the later capture sees -- inputs, workspace, weight-gradient
    table -- already exists, so nothing is allocated or uploaded while capturing (``_eager_then_capture``, which ``step`` and
    ``precapture`` share).  Losses are those of the eager loop."""

    def __init__(self, trainer, maxsize=16, capture=True):
        import collections
        self.trainer, self.maxsize = trainer, maxsize
        self.capture = capture     # False (--graph_capture=False): same buckets and static buffers, every step eager
        self.cache = collections.OrderedDict()     # key -> GraphEntry
        self.replays = self.eager = self.captures = 0
        self.capture_failed = False
        self.lazy = True           # False (data parallel): only precaptured graphs, everything else eager

    # -- the two places that touch the HIP runtime (a test replaces them with a recorder that, like a real capture, does not
    #    execute what it records)
    def _capture(self, fn):
        torch.cuda.synchronize()
        g = CapturedStep(fn)      # .replay(): plain launches from C where the capture is one path of kernels, else the graph
        return g, g.out

    def _sync(self):
        torch.cuda.synchronize()

    @staticmethod
    def shape_key(batch):
        return tuple((k, tuple(v.shape), str(v.dtype)) for k, v in sorted(batch.items()) if torch.is_tensor(v)) + \
            tuple((k, v) for k, v in sorted(batch.items()) if isinstance(v, int))

    @staticmethod
    def _copy_in(static, batch):
        for k, v in batch.items():
            if torch.is_tensor(v):
                static[k].copy_(v, non_blocking=True)

    def _eager_then_capture(self, ent, capture=True, must=False):
        """A real step on the entry's static buffers, then (``capture``) the same step captured over them.  A step that cannot
        be captured stays eager, here and for every later key; ``must``: the failure is raised instead."""
        tr = self.trainer
        with dynamic_n(tr.model, ent.capacity):
            stats = tr.train_step(ent.static)
            if not capture:
                return stats
            try:
                ent.graph, ent.out = self._capture(lambda: tr.train_step(ent.static))
            except Exception as exc:
                if must:
                    raise
                print(json.dumps({"graph_replay": "capture failed, staying eager", "error": str(exc)[:200]}), file=sys.stderr)
                self.capture_failed = True
                return stats
        # the graph holds raw pointers into this key's workspace: keep the workspace object alive with the graph, whatever
        # the module's own LRU cache does with it (evaluation batches of other shapes come in between)
        ent.workspace = getattr(tr.model, "_last_ws", None)
        self.captures += 1
        return stats

    def precapture(self, probe):
        """Data parallel: capture every capacity bucket NOW, in the same order on every rank.  A captured step contains the
        gradient all-reduce; a rank that captured lazily (whenever ITS batch first hit a bucket) would record a collective its
        peers execute.  Each bucket runs one warm-up step on synthetic lengths -- every kernel runs (workspaces, weight-gradient
        tables, the collective) -- and is then captured.  The warm-ups are REAL steps on made-up batches (zero features, label 0;
        the same on every rank): everything they change -- parameters, Adam moments, the optimizer's step count and dropout
        offset, the bf16 weight shadows, BatchNorm's running statistics, the health word -- is snapshotted before and put back
        afterwards, bit for bit, so training starts from the state it was given.  (A raised health word does not suppress the
        update: the step's first launch rolls the word, erc_cogmen_fwd_tile.)"""
        tr = self.trainer
        flat, model = tr.model.flat, tr.model
        opt = getattr(tr, "optim", None)
        saved = {k: v.clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}
        snap = [(t, t.clone()) for t in (getattr(flat, n, None) for n in ("data", "exp_avg", "exp_avg_sq", "grad_full")) if t is not None]
        if opt is not None and getattr(opt, "state", None) is not None:
            snap.append((opt.state, opt.state.clone()))
        if getattr(flat, "p2p", None) is not None:
            snap.append((flat.p2p.epoch, flat.p2p.epoch.clone()))
        for key, make, fill, synth in tr.all_capacity_buckets(probe):
            ent = self.cache[key] = GraphEntry(make(), fill, True, seen=1)
            synth(ent.static)
            self._eager_then_capture(ent, must=True)
        self._sync()
        with torch.no_grad():
            for t, keep in snap:
                t.copy_(keep)
            sd = model.state_dict()
            for k, v in saved.items():
                sd[k].copy_(v)
        flat.health.zero_()
        flat.events.zero_()
        if getattr(model, "shadows", None) is not None:
            model.refresh_shadows()          # the bf16 copies follow the restored parameters
        self.maxsize = max(self.maxsize, len(self.cache) + 2)

    def drop_graphs(self):
        """A launch argument of the captured step changed (the learning rate): every entry keeps its static buffers and
        workspace, runs one eager step on them when its key comes up again and is captured anew"""
        for ent in self.cache.values():
            ent.graph = ent.out = None

    def step(self, batch, key=None, resident=False):
        """``resident``: ``batch`` lives in fixed device buffers of its own (FixedBatches) -- the graph binds to them."""
        bucket = None
        if key is not None:
            key = (key, )
        else:
            bucket = self.trainer.capacity_bucket(batch) if hasattr(self.trainer, "capacity_bucket") else None
            key = bucket[0] if bucket is not None else self.shape_key(batch)
        ent = self.cache.get(key)
        if ent is None and not self.lazy:
            self.eager += 1
            return self.trainer.train_step(batch)
        if ent is None:
            if bucket is not None:
                static, fill = bucket[1](), bucket[2]
            else:
                static = batch if resident else {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}
                fill = None if resident else self._copy_in
            ent = self.cache[key] = GraphEntry(static, fill, bucket is not None)
            while len(self.cache) > self.maxsize:
                self.cache.popitem(last=False)
        else:
            self.cache.move_to_end(key)
        ent.seen += 1
        if ent.fill is not None and (ent.graph is not None or ent.seen > 1 or ent.capacity):
            ent.fill(ent.static, batch)          # (a plain first occurrence was cloned above: already in place)
        if ent.graph is not None:
            self.replays += 1
            ent.graph.replay()
            return ent.out
        self.eager += 1
        # plain shapes are captured on their second occurrence
        return self._eager_then_capture(ent, capture=self.capture and not self.capture_failed and
                                        (ent.capacity or ent.seen >= 2 or resident))


class ResidentLoop:
    """What ``--resident`` and ``--resident_eval`` share: the items stay in a device store (DeviceDialogueStore; MMIN's
    utterances: MMINDeviceStore) and a step's batch is never materialised.  A step is ``store.DESC_INTS`` B int32 (2 B, a row of
    ``batch_table``; MMIN: 3 B) copied into the fixed descriptor ``cur_desc`` plus its capacity -- here the batch's node count
    rounded up to N_BUCKET, at most B * T, T the store's own longest item (``store.t_max``); MMIN's loops key by a T capacity.  The
    first visit of a capacity runs the subclass's ``_step`` eagerly on the trainer's resident batch of that capacity and then
    captures it; every later step of that capacity is one copy, one dict lookup, one replay.  A trainer whose step does not
    scale with N names its own node bucket (``RESIDENT_N_BUCKET``, clipped to B * T: DAG-ERC, one capacity per store)."""

    N_BUCKET = 128

    def __init__(self, trainer, store, batch_size, capture=True):
        self.trainer, self.store, self.B = trainer, store, int(batch_size)
        self.T = int(store.t_max)
        named = getattr(trainer, "RESIDENT_N_BUCKET", None)
        if named:
            self.N_BUCKET = max(1, min(int(named), self.B * self.T))
        self.cur_desc = torch.zeros(store.DESC_INTS * self.B, dtype=torch.int32, device=store.device)
        self.graphs, self.capture = {}, capture      # capacity -> (graph or None, batch, workspace kept alive)
        self.replays = self.eager = self.captures = 0

    def drop_graphs(self):
        """A launch argument of the captured step changed (the learning rate): every capacity keeps its buffers and workspace,
        runs one eager step on them when it comes up again and is captured anew"""
        self.graphs = {cap: (None, batch, ws) for cap, (_, batch, ws) in self.graphs.items()}

    # -- the one place that touches the HIP runtime (a test replaces it with a recorder that does not execute what it records)
    def _capture(self, fn):
        torch.cuda.synchronize()
        return CapturedStep(fn)

    def _caps_of(self, counts):
        return [node_capacity(c, self.N_BUCKET, self.B * self.T) for c in counts]

    def _visit(self, cap):
        """a capacity without a graph: a real step (it allocates the bucket's buffers), then the capture"""
        ent = self.graphs.get(cap)
        batch = ent[1] if ent is not None else self._batch(cap)
        if batch is None:
            raise capi.ErcGraftError("%s: the trainer offers no resident batch of capacity %d" % (type(self).__name__, cap))
        ws = self._step(batch)
        self.eager += 1
        graph = None
        if self.capture:
            graph = self._capture(lambda: self._step(batch))
            self.captures += 1
        self.graphs[cap] = (graph, batch, ws)      # (the graph holds raw pointers into ws: kept alive with it)

    def _steps(self, table_dev, caps):
        cur_desc, graphs = self.cur_desc, self.graphs
        for s, cap in enumerate(caps):
            cur_desc.copy_(table_dev[s], non_blocking=True)
            ent = graphs.get(cap)
            if ent is not None and ent[0] is not None:
                ent[0].replay()
                self.replays += 1
                continue
            self._visit(cap)


class ResidentEpochs(ResidentLoop):
    """``--resident``: the training dialogues live in HBM (datasets.DeviceDialogueStore, 288 GB per GPU: IEMOCAP's features are
    16 MB).  Per epoch the host draws the permutation (DataLoader(shuffle=True) semantics: every dialogue once, a smaller last
    batch) and uploads ONE int32 table [steps, 2 B] (``batch_table``); per step it copies that step's 2 B int32 into the fixed
    descriptor buffer and replays the bucket's captured graph -- the projection launch reads feature rows, speakers and labels
    straight from the store (csrc/cogmen_project.hip, resident mode).  Host work per step: one 256-byte device copy + one
    graph launch.  Trainers with ``resident_batch``: COGMEN, DialogueGCN, bc-LSTM / bc-GRU (their layer-0 input projection
    reads the store through the row map of erc_bcrnn_meta_cap), DialogueRNN (its hoisted products gather the store's rows
    through node_row of erc_dialogrnn_meta_cap), DAG-ERC (the row map of erc_dag_meta_cap)."""

    def __init__(self, trainer, store, batch_size, seed, capture=True):
        super().__init__(trainer, store, batch_size, capture)
        self.gen = torch.Generator().manual_seed(seed)
        self.acc = torch.zeros(4, dtype=torch.float64, device=store.device)      # sums of the steps' {loss, #correct, weight, -}
        self._lens32, self._offs32 = store.lengths.to(torch.int32).numpy(), store.offsets[:-1].to(torch.int32).numpy()
        self._ahead = []           # (#utterances, node capacity per step, device table) of the epochs planned ahead

    def plan(self, n_epochs):
        """Draw the permutations of the next ``n_epochs`` epochs (sequential randperm draws: the same epochs as drawing them
        one by one) and upload their batch tables in one copy: nothing but the step loop is left inside an epoch."""
        n, B = len(self.store), self.B
        tabs = np.zeros((n_epochs, -(-n // B), 2 * B), dtype=np.int32)
        for e in range(n_epochs):
            tabs[e] = batch_table(self._lens32, self._offs32, torch.randperm(n, generator=self.gen).numpy(), B)
        dev = torch.from_numpy(tabs).to(self.store.device)
        for e in range(n_epochs):
            counts = tabs[e, :, :B].sum(1).tolist()
            self._ahead.append((sum(counts), self._caps_of(counts), dev[e]))

    def supported(self):
        """Can EVERY step of an epoch run from the resident store?  Probed with the smallest bucket and with the largest a batch
        of this store can need (batch_size of its longest dialogues: above the fused path's node limit `resident_batch` returns
        None -- found here, before the first epoch, not by a step in the middle of one)."""
        lens = sorted((int(v) for v in self.store.lengths.tolist()), reverse=True)
        worst = self._caps_of([sum(lens[:self.B])])[0]
        return all(self._batch(cap) is not None for cap in sorted({self.N_BUCKET, max(worst, self.N_BUCKET)}))

    def _batch(self, cap):
        return self.trainer.resident_batch(self.store, self.cur_desc, self.B, self.T, cap)

    def _step(self, batch):
        self.acc.add_(self.trainer.train_step(batch)[:4])
        return getattr(self.trainer.model, "_last_ws", None)

    def epoch(self):
        """one pass over the store; returns (#utterances, #steps)"""
        if not self._ahead:
            self.plan(1)
        n_utt, caps, table_dev = self._ahead.pop(0)
        with dynamic_n(self.trainer.model):
            self._steps(table_dev, caps)
        return n_utt, len(caps)


class ResidentEval(ResidentLoop):
    """``--resident_eval``: the test epoch from HBM, scored on the device.  The test dialogues stay in their
    DeviceDialogueStore; the test order is fixed (sequential batches of ``batch_size`` dialogues, the last one padded with
    zero-length slots: DataLoader(shuffle=False) semantics), so the whole int32 table [steps, 2 B] (``batch_table``) is
    uploaded ONCE, here.  T is the TEST store's own longest dialogue.  The first visit of a bucket runs the trainer's
    ``resident_eval_step`` eagerly and captures it; from then on a test epoch is

        cm.zero_() ; per step: copy 2 B int32, replay ; one cm.cpu() at the end

    and every metric of the epoch line is a function of that confusion matrix (``report_from_cm``)."""

    def __init__(self, trainer, store, batch_size, capture=True, n_classes=None):
        super().__init__(trainer, store, batch_size, capture)
        self.table = batch_table(store.lengths.to(torch.int32).numpy(), store.offsets[:-1].to(torch.int32).numpy(),
                                 np.arange(len(store)), self.B)
        self.steps = len(self.table)
        self.counts = self.table[:, :self.B].sum(1).tolist()
        self.caps = self._caps_of(self.counts)
        self.table_dev = torch.from_numpy(self.table).to(store.device)
        C = int(n_classes if n_classes is not None else trainer.params.n_classes)
        self.cm = torch.zeros(C, C, dtype=torch.int64, device=store.device)

    def supported(self):
        """Can EVERY step of the test epoch run from the resident store?  (asked once, before the first epoch)"""
        return all(self._batch(cap) is not None for cap in sorted(set(self.caps)))

    def _batch(self, cap):
        return self.trainer.resident_eval_batch(self.store, self.cur_desc, self.B, self.T, cap)

    def _step(self, batch):
        return self.trainer.resident_eval_step(batch, self.cm)

    def epoch(self):
        """one pass over the test store; returns its confusion matrix (host int64 [C, C], true x predicted)"""
        self.cm.zero_()
        self._steps(self.table_dev, self.caps)
        return self.cm.cpu()


def report_from_cm(cm):
    """``classification_report``'s dict from the confusion matrix alone (rows = true class, columns = predicted): every one
    of these metrics is a function of it.  Per class: recall = tp / support, precision = tp / predicted, f1 = 2 tp /
    (support + predicted), 0 where undefined (zero_division=0).  ``wa`` (balanced accuracy) is the mean recall over the classes
    that occur in the labels; ``pre`` / ``rec`` / ``f1`` are weighted by support; ``maf1`` is the mean f1 over the classes
    that occur in the labels or the predictions (sklearn's default label set); ``mif1`` = ``acc``."""
    cm = np.asarray(cm, dtype=np.int64)
    n = int(cm.sum())
    tp, sup, prd = np.diag(cm).astype(np.float64), cm.sum(1).astype(np.float64), cm.sum(0).astype(np.float64)
    div = lambda a, b: np.divide(a, b, out=np.zeros_like(a), where=b > 0)
    rec, pre, f1 = div(tp, sup), div(tp, prd), div(2.0 * tp, sup + prd)
    weighted = lambda v: float((v * sup).sum() / n) if n else 0.0
    acc = float(tp.sum() / n) if n else 0.0
    seen = (sup > 0) | (prd > 0)
    return {
        "cm": cm.tolist(),
        "acc": acc,
        "wa": float(rec[sup > 0].mean()) if n else 0.0,
        "pre": weighted(pre),
        "rec": weighted(rec),
        "f1": weighted(f1),
        "mif1": acc,
        "maf1": float(f1[seen].mean()) if n else 0.0,
    }


def classification_report(true, pred, n_classes):
    """The metric set of mmbase.py:259-275."""
    from sklearn import metrics
    return {
        "cm": metrics.confusion_matrix(true, pred, labels=range(n_classes)).tolist(),
        "acc": metrics.accuracy_score(true, pred),
        "wa": metrics.balanced_accuracy_score(true, pred),
        "pre": metrics.precision_score(true, pred, average="weighted", zero_division=0),
        "rec": metrics.recall_score(true, pred, average="weighted", zero_division=0),
        "f1": metrics.f1_score(true, pred, average="weighted", zero_division=0),
        "mif1": metrics.f1_score(true, pred, average="micro", zero_division=0),
        "maf1": metrics.f1_score(true, pred, average="macro", zero_division=0),
    }


def weighted_accuracy(y_true, y_pred):
    """mmbase.py:231-251: (TP N / P + TN) / 2N of a binary column -- None where the column has no positives or no
    negatives (the reference divides by zero there)"""
    y_true, y_pred = np.asarray(y_true), np.asarray(y_pred)
    P = int((y_true == 1).sum())
    N = len(y_true) - P
    if P == 0 or N == 0:
        return None
    TP = int(((y_true == 1) & (y_pred == 1)).sum())
    TN = int(((y_true == 0) & (y_pred == 0)).sum())
    return (1.0 * TP * (N / (1.0 * P)) + TN) / (2.0 * N)


def multiemo_report(true_multi, prob_multi, thresh=0.5):
    """The multi-label block of mmbase.py:280-300 on sigmoid(logits7) > thresh: per emotion column the accuracy, the
    weighted F1 and the weighted accuracy, and their means.  A column without positives or without negatives reports
    ``None`` as its weighted accuracy and the mean runs over the defined columns (the reference raises
    ZeroDivisionError there)."""
    from sklearn import metrics
    true_multi, pred = np.asarray(true_multi), (np.asarray(prob_multi) > thresh).astype(int)
    acc, f1, wa = [], [], []
    for i in range(true_multi.shape[1]):
        col = pred[:, i]
        acc.append(float(metrics.accuracy_score(true_multi[:, i], col)))
        f1.append(float(metrics.precision_recall_fscore_support(true_multi[:, i], col, average="weighted", zero_division=0)[2]))
        wa.append(weighted_accuracy(true_multi[:, i], col))
    defined = [w for w in wa if w is not None]
    return {"thresh": thresh, "acc": acc, "f1": f1, "wa": wa, "mean_acc": float(np.mean(acc)), "mean_f1": float(np.mean(f1)),
            "mean_wa": float(np.mean(defined)) if defined else None}


def _setup_graphs(params, trainer, train_loader, rank, world, device):
    """(StepGraphs or None, FixedBatches or None).  Captured whole-step graphs: capacity buckets where the trainer offers
    them, exact shapes otherwise.  Under data parallelism the captured step is the same one -- forward, backward, the RCCL
    all-reduce, the optimizer -- but every capture must happen at the same point on every rank: buckets are captured up
    front, in one order (StepGraphs.precapture); a trainer without buckets keeps the eager step there."""
    if hasattr(trainer, "capacity_bucket"):
        trainer.t_cap = bucket_t_cap(train_loader, world, device)
    graphs = StepGraphs(trainer, capture=params.get("graph_capture", True)) if params.get("graph_replay", True) else None
    fixed = FixedBatches(train_loader, trainer, params.seed + rank) if params.get("fixed_batches", False) else None
    if graphs is not None and world > 1 and fixed is None:
        probe = trainer.prepare_batch(first_batch(train_loader))
        if hasattr(trainer, "all_capacity_buckets") and trainer.all_capacity_buckets(probe):
            graphs.precapture(probe)
            graphs.lazy = False         # a batch outside every bucket runs eagerly (same collectives, no capture)
        else:
            graphs = None
    return graphs, fixed


def _setup_resident(params, trainer, train_loader, test_loader, rank, world):
    """(ResidentEpochs or None, ResidentEval or None) of ``--resident`` / ``--resident_eval``; a configuration that cannot
    run that way exits here, before the first epoch"""
    resident = res_eval = None
    if params.get("resident", False):
        if world > 1 or not isinstance(train_loader, StoreLoader) or not hasattr(trainer, "resident_batch"):
            raise SystemExit("--resident needs --device_collate, one rank and a trainer with resident batches (capacity mode)")
        resident = ResidentEpochs(trainer, train_loader.store, params.train.batch_size, params.seed + rank,
                                  capture=params.get("graph_capture", True))
        if not resident.supported():
            raise SystemExit("--resident: this configuration cannot run its step in capacity mode")
        resident.plan(params.epoch)
    if params.get("resident_eval", False):      # the test epoch from HBM too, scored on the device (ResidentEval)
        if resident is None:
            raise SystemExit("--resident_eval needs --resident (the test epoch then runs from the HBM-resident test store)")
        if not hasattr(trainer, "resident_eval_step"):
            raise SystemExit("--resident_eval: this module's trainer has no resident_eval_step (--module=cogmen has one)")
        if params.get("mosei_metric", "") == "multiemo":
            raise SystemExit("--resident_eval: mosei_metric=multiemo reports multi-label metrics, which are no function of the "
                             "confusion matrix the device returns")
        res_eval = ResidentEval(trainer, test_loader.store, params.test.batch_size, capture=params.get("graph_capture", True))
        if not res_eval.supported():
            raise SystemExit("--resident_eval: this configuration cannot run its test step in capacity mode")
    return resident, res_eval


# -- one training epoch over batches, in two forms (the third, --resident, is ResidentEpochs.epoch).  They return the batches'
#    utterance counts; a step's stats go into its row of ``ring`` (no device->host synchronisation inside the epoch)
def train_epoch_fixed(fixed, graphs, trainer, ring):
    """--fixed_batches: the device batches collated once, in a fresh order; each one's graph binds to its own buffers"""
    counts = []
    for i, (bid, (n_b, dev_batch)) in enumerate(fixed):
        stats = graphs.step(dev_batch, key=bid, resident=True) if graphs is not None else trainer.train_step(dev_batch)
        ring[i].copy_(stats[:4], non_blocking=True)
        counts.append(n_b)
    return counts


def train_epoch_loader(loader, graphs, trainer, ring):
    """the default: the loader's reshuffled batches, through StepGraphs where there is one"""
    counts = []
    for i, item in enumerate(loader):
        dev_batch = trainer.prepare_batch(item)
        stats = graphs.step(dev_batch) if graphs is not None else trainer.train_step(dev_batch)
        ring[i].copy_(stats[:4], non_blocking=True)
        counts.append(int(item["label"].shape[0]))
    return counts


def print_step_lines(params, epoch, ring, counts, multitask=False):
    """every ``log_every``-th step's JSON line, from one device -> host copy of the ring"""
    rows = ring[:len(counts)].cpu().tolist()
    for i, (row, n_b) in enumerate(zip(rows, counts)):
        if (i + 1) % params.log_every == 0:
            line = {"epoch": epoch, "step": i, "Lall": row[0], "Acc": row[1] / max(1, n_b)}
            if multitask:
                line.update(Lce=row[2], Lmulti=row[3])
            print(json.dumps(line), flush=True)


# -- one test epoch (after every training epoch: mmbase.py:136,180-201) over batches (--resident_eval: ResidentEval.epoch)
def test_epoch_loader(trainer, test_loader, multiemo=False):
    """returns (true, pred, true_multi, prob_multi); the last two are filled under ``multiemo``"""
    true, pred, true_multi, prob_multi = [], [], [], []
    for batch in test_loader:
        if multiemo:           # mosei_test_step (mmbase.py:167-178)
            logits, logits7 = trainer.to_mosei_multitask_logits(trainer.prepare_batch(batch))
            true_multi.append(batch["emo_label"].cpu().numpy())
            prob_multi.append(torch.sigmoid(logits7).cpu().numpy())
            pred.extend(logits.argmax(-1).cpu().tolist())
            true.extend(batch["senti2_label"].tolist())
            continue
        logits = trainer.to_logits(trainer.prepare_batch(batch))
        if logits.dim() == 3:
            logits = logits[batch["attention_mask"].bool().to(logits.device)]
        pred.extend(logits.argmax(-1).cpu().tolist())
        true.extend(batch["label"].tolist())
    return true, pred, true_multi, prob_multi


@dataclasses.dataclass
class EvalEpoch:
    """what ``EpochLoop.test_epoch`` returns: ``cm`` is the confusion matrix of a ResidentEval epoch (host int64 [C, C]) and
    None after the host loop, whose lists follow (the last two are filled under ``multiemo``)"""
    cm: object = None
    true: list = dataclasses.field(default_factory=list)
    pred: list = dataclasses.field(default_factory=list)
    true_multi: list = dataclasses.field(default_factory=list)
    prob_multi: list = dataclasses.field(default_factory=list)


class EpochLoop:
    """One epoch as train_mm.py runs it, for ``run`` and for tools/epoch_bench.py.  The constructor does what lies between
    "trainer constructed" and "first epoch", in this order (FixedBatches draws from the loader, ``resident.plan`` draws the
    permutations of every epoch): the loaders, StepGraphs / FixedBatches, the per-step stats ring, the resident loops.
    ``train_epoch`` and ``test_epoch`` launch an epoch in the form the flags select; they do not synchronise, take no host
    clock, print nothing and leave the model's mode alone -- ``model.train()`` / ``model.eval()``, which walk every submodule,
    are the caller's part like the clock, and ``run`` keeps them outside its timed spans.  ``counters``: the ResidentEpochs
    or StepGraphs of the run (their ``replays`` / ``eager`` / ``captures``), None for the plain eager loop."""

    def __init__(self, params, trainer, device, rank=0, world=1):
        self.params, self.trainer = params, trainer
        self.train_loader, self.test_loader = make_loaders(params, rank, world, device)
        self.graphs, self.fixed = _setup_graphs(params, trainer, self.train_loader, rank, world, device)
        self.n_steps = len(self.fixed) if self.fixed is not None else len(self.train_loader)
        # per-step {loss, #correct, ...}: read once per epoch
        self.ring = torch.zeros(max(1, self.n_steps), 4, dtype=torch.float32, device=device)
        self.resident, self.res_eval = _setup_resident(params, trainer, self.train_loader, self.test_loader, rank, world)
        self.counters = self.resident or self.graphs

    def train_epoch(self):
        """(#utterances, the steps' utterance counts: [] under --resident, whose steps are never materialised)"""
        if self.resident is not None:
            return self.resident.epoch()[0], []
        if self.fixed is not None:
            counts = train_epoch_fixed(self.fixed, self.graphs, self.trainer, self.ring)
        else:
            counts = train_epoch_loader(self.train_loader, self.graphs, self.trainer, self.ring)
        return sum(counts), counts

    def test_epoch(self, multiemo=False):
        """an ``EvalEpoch``; call it with the model in eval mode"""
        if self.res_eval is not None:
            return EvalEpoch(cm=self.res_eval.epoch())
        return EvalEpoch(None, *test_epoch_loader(self.trainer, self.test_loader, multiemo))


def epoch_loop_class(trainer_cls):
    """the epoch-loop class of a trainer class: the one it names (``EPOCH_LOOP``: the MMIN trainers), else ``EpochLoop``"""
    return getattr(trainer_cls, "EPOCH_LOOP", None) or EpochLoop


def setup_device(params, local=0):
    """the process's GPU: ``--device``, else cuda:<local rank>, made current"""
    if not torch.cuda.is_available():
        raise RuntimeError("the ERC hot path runs on an MI355X through libercgraft.so; no GPU is visible "
                           "(there is no CPU fallback)")
    device = torch.device(params.device if params.device not in (None, "cuda") else "cuda:%d" % local)
    torch.cuda.set_device(device)
    return device


def _epoch_line(epoch, utt_per_s, rep, best, counters, n_steps, test_s, multiemo_rep):
    """the epoch's JSON line; ``counters``: the ResidentEpochs or StepGraphs of the run, None for a plain eager loop"""
    line = {"epoch": epoch, "train_utt_per_s": utt_per_s, "test": {k: rep[k] for k in rep if k != "cm"}, "best": best,
            "graph_replays": counters.replays if counters else 0, "eager_steps": counters.eager if counters else n_steps,
            "graphs_captured": counters.captures if counters else 0}
    if test_s is not None:
        line["test_s"] = test_s
    if multiemo_rep is not None:
        line["multiemo"] = multiemo_rep
    return line


def run(trainer_cls, params_cls, argv=None):
    params = params_cls()
    params.from_args(argv)
    if "mosei" in params.dataset and not hasattr(trainer_cls, "to_mosei_multitask_logits"):
        # the reference's test_step calls to_mosei_multitask_logits on MOSEI, which only CIM implements
        # (mmbase.py:144-145,181-182): every other module raises NotImplementedError there
        raise SystemExit("dataset %s: this module has no multi-task (sentiment + emotion) head; only --module=cim trains on "
                         "CMU-MOSEI" % params.dataset)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    device = setup_device(params, int(os.environ.get("LOCAL_RANK", "0")))
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=device)
    fix_seed(params.seed)
    trainer = trainer_cls(params, device)
    if params.get("load"):      # checkpoint in the reference's envelope (checkpoint.py)
        from . import checkpoint
        checkpoint.load(trainer, params.load)
    loop = EpochLoop(params, trainer, device, rank, world)
    best, acc_prev = {}, [0.0] * 4
    log = rank == 0 and params.log_every
    multiemo = params.get("mosei_metric", "") == "multiemo"
    check_cluster = getattr(trainer.model, "check_cluster", lambda: None)
    for epoch in range(params.epoch):
        trainer.model.train()
        t0 = time.perf_counter()
        n_utt, counts = loop.train_epoch()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if loop.resident is not None:      # no step lines: the epoch's mean loss / accuracy from the running totals
            tot = loop.resident.acc.cpu().tolist()
            acc, acc_prev = [a - b for a, b in zip(tot, acc_prev)], tot
            if log:
                print(json.dumps({"epoch": epoch, "steps": loop.n_steps, "Lall": acc[0] / loop.n_steps,
                                  "Acc": acc[1] / max(1, n_utt)}), flush=True)
        check_cluster()
        if log:
            print_step_lines(params, epoch, loop.ring, counts, getattr(trainer, "multitask", False))
        trainer.model.eval()
        t1 = time.perf_counter()
        res = loop.test_epoch(multiemo)
        test_s = None
        if res.cm is not None:             # (the host loop synchronises per batch and reports no time of its own)
            torch.cuda.synchronize()
            test_s = time.perf_counter() - t1
        check_cluster()      # a timeout inside to_logits would make the metrics below meaningless
        if rank == 0:
            rep = classification_report(res.true, res.pred, params.n_classes) if res.cm is None else report_from_cm(res.cm.numpy())
            for k in ("acc", "wa", "f1", "mif1", "maf1", "pre", "rec"):
                best[k] = max(best.get(k, 0.0), rep[k])
            multiemo_rep = multiemo_report(np.concatenate(res.true_multi), np.concatenate(res.prob_multi)) if multiemo else None
            print(json.dumps(_epoch_line(epoch, n_utt / dt, rep, best, loop.counters, len(counts), test_s, multiemo_rep)),
                  flush=True)
    if params.get("save") and rank == 0:
        from . import checkpoint
        checkpoint.save(trainer, params.save)
    if world > 1:
        # the captured step graphs hold RCCL work: they go before the process group does (bench.py saw an abort at interpreter
        # exit, once in a while, with the group torn down under live graphs)
        loop = None
        import gc
        gc.collect()
        torch.cuda.synchronize()
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    return best
