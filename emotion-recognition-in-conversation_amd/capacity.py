"""What the trainers share: the batch preparation, the plain training step and the constructor's tail (``TrainerBase``), the
constructor of the conv-emotion family (``ConvEmotionTrainer``), and capacity mode's host side (``CapacityBuckets``) -- the
buckets ``trainer.StepGraphs`` replays and the resident batch ``trainer.ResidentEpochs`` steps over --, the store extension of
a resident step (``ZeroRowStores``) and the test step ``trainer.ResidentEval`` replays (``ResidentEvalSteps``).  A trainer in
capacity mode keeps only its policy: class attributes (N_BUCKET, the layout, the exact-shape rule, CLEAR_STALE), the gate and,
where it goes through the probe, the precapture list (the table in DESIGN.md, "capacity mode: one implementation, per-trainer
policy")."""
import os

import torch

from . import capi
from .engine import FusedAdam, all_reduce_grads

IEMOCAP6_WEIGHTS = [1 / 0.086747, 1 / 0.144406, 1 / 0.227883, 1 / 0.160585, 1 / 0.127711, 1 / 0.252668]  # dgcn.py:109-110, dgcnv2.py:213-214


def node_capacity(n, bucket, limit):
    """``n`` nodes rounded up to a multiple of ``bucket``, at most ``limit`` (= B_cap * T_cap: the static block holds no more)"""
    return min(-(-n // bucket) * bucket, limit)


def bucket_sizes(bucket, top):
    """every node capacity up to ``top``, smallest first: the multiples of ``bucket`` and ``top`` itself (the clipped one)"""
    return sorted({min(n, top) for n in range(bucket, top + bucket, bucket)})


def iemocap6_class_weight(params, device, error, source):
    """the class weight of ``--loss_weights`` (None with the flag off); ``error`` / ``source``: the caller's exception type and
    the reference lines its message cites"""
    if not params.get("loss_weights", True):
        return None
    if params.n_classes != 6:
        raise error("--loss_weights uses the six hard-coded IEMOCAP-6 inverse frequencies "
                    "(%s); run %d-class datasets with --loss_weights=False" % (source, params.n_classes))
    return torch.tensor(IEMOCAP6_WEIGHTS, dtype=torch.float32, device=device)


class ZeroRowStores:
    """A resident step reads a store's feature rows through its row map, and padded positions read a zero row, which the
    store does not have: ``ext(store, feats)`` is ``feats`` (one [U, D] tensor or a dict of them) with one zero row appended,
    built once per store (a run has at most two: train and test).  The cache holds the store and the copy of its features
    for as long as the trainer lives: a tool that feeds one trainer many stores keeps all of them resident."""

    def __init__(self):
        self._ext = {}

    def __call__(self, store, feats):
        ent = self._ext.get(id(store))
        if ent is None or ent[0] is not store:
            pad = lambda x: torch.cat([x, x.new_zeros(1, x.shape[1])])
            ext = {k: pad(v) for k, v in feats.items()} if isinstance(feats, dict) else pad(feats)
            ent = self._ext[id(store)] = (store, ext)
        return ent[1]


class TrainerBase:
    """``prepare_batch`` / ``to_logits`` / the plain ``train_step`` / the constructor's tail (``_make_optim``) of a trainer with
    ``params``, ``device``, ``model`` and, where the loss takes one, ``class_weight``."""
    BF16_INPUT = False     # True: ``--compute=bf16`` casts the features once, here (COGMEN, DialogueGCN, DAG-ERC)
    CLASS_WEIGHTED = True  # False: ``model.loss_and_grads`` takes the batch alone (DAG-ERC, MMGCN, CIM)

    def _make_optim(self, weight_decay=0.0, clip_norm=0.0, health_gates=False, opt_in=False):
        """The constructor's tail.  Call it AFTER torch.manual_seed and the model's construction (parameter initialisation
        draws from that generator).  ``weight_decay``: the default where --optim.weight_decay is absent, None = it must be
        given; ``health_gates``: the health word in the tail of the flat gradient buffer makes the update skip itself on the
        device; ``opt_in``: capacity buckets only with --capacity_buckets=True or --resident (which implies them) -- the
        default stays the exact-shape step, whose dropout masks (keyed by the element index, so by the batch's shape) a
        capacity-sized step does not reproduce."""
        p, o = self.params, self.params.optim
        self.optim = FusedAdam(self.model.flat, lr=o.lr,
                               weight_decay=o.weight_decay if weight_decay is None else o.get("weight_decay", weight_decay),
                               decoupled=(o.name == "AdamW"), clip_norm=clip_norm, seed=p.seed)
        self.model.rng_state = self.optim.rng_state      # the dropout offset advances with the optimizer step
        if health_gates:
            self.optim.skip_flag = self.model.flat.health
        if opt_in:
            self.capacity = bool(p.get("capacity_buckets", False) or p.get("resident", False))

    def prepare_batch(self, batch):
        out = {k: (v.to(self.device) if torch.is_tensor(v) else v) for k, v in batch.items()}
        tl = batch.get("text_length")
        if "n_nodes" not in out and torch.is_tensor(tl) and not tl.is_cuda:
            out["n_nodes"] = int(tl.sum())      # host tensor: no device sync when a batch carries no labels
        if self.BF16_INPUT and self.model.compute == "bf16":
            out["input_tensor"] = out["input_tensor"].to(torch.bfloat16)
        return out

    def to_logits(self, batch):
        return self.model(**batch)[0]

    def train_step(self, batch):
        """forward + (class-weighted) loss + backward + (DP all-reduce) + Adam.  Returns the device stats tensor."""
        self.model.train()
        weight = (self.class_weight, ) if self.CLASS_WEIGHTED else ()
        stats = self.model.loss_and_grads(batch, *weight)
        scale = all_reduce_grads(self.model.flat)
        self.optim.step(grad_scale=scale)
        return stats


class ConvEmotionTrainer(TrainerBase):
    """What the trainers of the conv-emotion family (bc-LSTM / bc-GRU, DialogueRNN, conv-emotion DialogueGCN) share: fp32
    only, the class-weighted loss, Adam lr 3e-4 without weight decay (track_mm/dgcnv2.py:22-48,184-219), and the dropout
    counter of the model living in the optimizer.  A subclass names its ``--module`` value and builds its model."""
    NAME = None

    def __init__(self, params, device, opt_in=False):
        """``opt_in``: ``_make_optim``'s (a subclass with capacity buckets, bc-LSTM / bc-GRU, passes True)"""
        self.params, self.device = params, torch.device(device)
        compute = params.get("compute", "f32")
        if compute != "f32":
            raise capi.ErcGraftError("--module=%s runs in fp32 (the reference is fp32); --compute=%s is not supported"
                                     % (self.NAME, compute))
        self.class_weight = iemocap6_class_weight(params, self.device, capi.ErcGraftError, "dgcnv2.py:213-214")
        torch.manual_seed(params.seed)
        self.model = self._build_model(params, compute).finalize(self.device)
        self._make_optim(opt_in=opt_in)

    def _build_model(self, params, compute):
        raise NotImplementedError


class CapacityBuckets:
    """Capacity mode of a trainer.  A bucket is a set of static buffers for B_cap dialogue slots (missing ones get length 0)
    of T_cap utterances and N_cap labels, keyed ``("capacity", B_cap, T_cap, N_cap)``; B_cap is at least train.batch_size,
    T_cap at least ``self.t_cap`` (the longest training dialogue of every rank, set by trainer.run), N_cap the batch's node
    count rounded up to N_BUCKET.  The trainer supplies ``_capacity_ok`` (the gate) and ``_resident_ok`` and declares the rest
    below; it may replace ``_precapture_caps`` (a list that goes through the probe) and ``_resident_inputs``."""
    N_BUCKET = 128             # node counts are rounded up to a multiple of this (the node launches scale with N_cap)
    TIME_MAJOR = False         # the features / speaker_tensor are [T, B, ...] instead of [B, T, ...]
    EXACT_SHAPE_STAYS = True   # a batch that already has its bucket's shape gets no bucket: there is nothing to pad
    CLEAR_STALE = False        # fill clears what the previous batch left behind (the step READS padded rows); the static
    #                            dict then carries "extent", host side: the block the last batch occupied, in layout order
    capacity = True            # False: every step keeps its exact shape

    def _p2p(self):
        """the opt-in peer-to-peer gradient exchange (ERC_DP_P2P=1): capacity buckets stay off there"""
        return getattr(self.model.flat, "p2p", None) is not None or os.environ.get("ERC_DP_P2P", "0") == "1"

    def _feature_keys(self):
        """the batch's feature blocks (MMGCN: one per modality)"""
        return ("input_tensor", )

    def _absent_keys(self):
        """keys a bucket carries as None (MMGCN: the modalities the model does not have)"""
        return ()

    def _bt(self, batch):
        a, b = (int(v) for v in batch[self._feature_keys()[0]].shape[:2])
        return (b, a) if self.TIME_MAJOR else (a, b)

    def _caps(self, batch):
        B, T = self._bt(batch)
        return max(B, int(self.params.train.batch_size)), max(T, int(getattr(self, "t_cap", 0)))

    def _bucket(self, like, B_cap, T_cap, N_cap):
        """(key, make, fill) of one bucket; ``like`` gives the trailing shapes and the dtypes.  Every feature block and
        speaker_tensor is [T_cap, B_cap, ...] (TIME_MAJOR) or [B_cap, T_cap, ...] with the trailing dims of ``like``'s (speaker
        ids [B, T] have none, one-hot speakers [.., .., S] one)."""
        blocks, absent = tuple(self._feature_keys()) + ("speaker_tensor", ), self._absent_keys()
        clear, dev = self.CLEAR_STALE, self.device
        lead = (T_cap, B_cap) if self.TIME_MAJOR else (B_cap, T_cap)
        zeros = lambda k, shape: torch.zeros(tuple(shape), dtype=like[k].dtype, device=dev)

        def make():
            static = {k: zeros(k, lead + tuple(like[k].shape[2:])) for k in blocks}
            static.update({k: None for k in absent})
            static.update(text_length=zeros("text_length", (B_cap, )), label=zeros("label", (N_cap, )))
            if clear:
                static["extent"] = [0, 0, 0]
            return static

        def fill(static, b):
            # CLEAR_STALE: only what the previous batch occupied and this one does not cover is cleared (never the whole
            # capacity buffer): [r:pr, :pc] below this batch's rows, [:min(r, pr), c:pc] beside its columns
            # r, c: the batch's extent along the two leading dims -- (T, B) under TIME_MAJOR, (B, T) otherwise; pr, pc: the
            # previous batch's
            r, c = (int(v) for v in b[blocks[0]].shape[:2])
            Bb, Nb = c if self.TIME_MAJOR else r, int(b["label"].shape[0])
            pr, pc, Np = static["extent"] if clear else (0, 0, 0)
            for k in blocks:
                static[k][:r, :c].copy_(b[k], non_blocking=True)
                if pr > r:
                    static[k][r:pr, :pc].zero_()
                if pc > c:
                    static[k][:min(r, pr), c:pc].zero_()
            static["text_length"].zero_()                     # dialogues the batch does not have: length 0
            static["text_length"][:Bb].copy_(b["text_length"], non_blocking=True)
            static["label"][:Nb].copy_(b["label"], non_blocking=True)
            if Np > Nb:
                static["label"][Nb:Np].zero_()
            if clear:
                static["extent"][:] = [r, c, Nb]

        return ("capacity", B_cap, T_cap, N_cap), make, fill

    def _precapture_caps(self, batch):
        """(B_cap, T_cap, node capacities) of the buckets a data parallel run captures up front, or None.  Built from
        train.batch_size and T_cap (trainer.bucket_t_cap) ALONE, never from the probe batch's shape (``batch`` may be None;
        DialogueGCN and COGMEN go through the probe and replace this): every rank captures the same list, smallest first, the
        clipped top bucket B_cap * T_cap included.  The gate is asked for the smallest bucket."""
        B_cap, T_cap = int(self.params.train.batch_size), int(getattr(self, "t_cap", 0))
        if not self._capacity_ok(B_cap, T_cap, min(self.N_BUCKET, B_cap * T_cap), batch):
            return None
        return B_cap, T_cap, bucket_sizes(self.N_BUCKET, B_cap * T_cap)

    def _synth_lengths(self, B_cap, T_cap, n):
        """all B_cap dialogues present, lengths adding up to n (each <= T_cap as long as n <= B_cap * T_cap)"""
        lens = torch.full((B_cap, ), n // B_cap, dtype=torch.int64)
        lens[:n - int(lens.sum())] += 1
        return lens

    def capacity_bucket(self, batch):
        """trainer.StepGraphs: (key, make_static, fill) of the capacity bucket that holds ``batch`` (a prepared device batch),
        or None when the step cannot run in capacity mode (the trainer's gate) or, under EXACT_SHAPE_STAYS, the batch already
        has its bucket's shape: the exact-shape path runs then."""
        if not self.capacity:
            return None
        B_cap, T_cap = self._caps(batch)
        N = int(batch["label"].shape[0])
        N_cap = node_capacity(N, self.N_BUCKET, B_cap * T_cap)
        if not self._capacity_ok(B_cap, T_cap, N_cap, batch) or \
                (self.EXACT_SHAPE_STAYS and self._bt(batch) + (N, ) == (B_cap, T_cap, N_cap)):
            return None
        return self._bucket(batch, B_cap, T_cap, N_cap)

    def all_capacity_buckets(self, batch):
        """Every bucket a batch of this loader can fall into, smallest first, each with a synthetic filler (all B_cap
        dialogues present, lengths adding up to the capacity): data parallel runs capture all of them up front, in the
        same order on every rank (a captured step holds a collective: ranks must not capture at different times)."""
        caps = self._precapture_caps(batch)
        if caps is None:
            return []
        B_cap, T_cap, sizes = caps
        out = []
        for N_cap in sizes:
            def synth(static, n=N_cap):
                static["text_length"].copy_(self._synth_lengths(B_cap, T_cap, n))
            out.append(self._bucket(batch, B_cap, T_cap, N_cap) + (synth, ))
        return out

    def _resident_inputs(self, store):
        return store.fused, store.speaker

    def resident_batch(self, store, cur_desc, B_cap, T_cap, N_cap):
        """trainer.ResidentEpochs: the "batch" of a step whose dialogues stay in the HBM-resident store -- the store's arrays,
        the 2 B_cap int32 the host rewrites per step (lengths | first store rows of the batch's dialogue slots) and the
        capacities the launches are sized for.  None when the step cannot run that way (``_resident_ok``)."""
        if not self._resident_ok(store, B_cap, T_cap, N_cap):
            return None
        x, spk = self._resident_inputs(store)
        return dict(input_tensor=x, speaker_tensor=spk, text_length=None, label=store.label, desc=cur_desc,
                    caps=(B_cap, T_cap, N_cap))


class ResidentEvalSteps:
    """``--resident_eval`` of a capacity-mode trainer whose model has ``eval_scores``.  A mixin of its own: trainer.run asks
    ``hasattr(trainer, "resident_eval_step")``, and a trainer without a scored test step (bc-LSTM / bc-GRU) must not have it."""

    def resident_eval_batch(self, store, cur_desc, B_cap, T_cap, N_cap):
        """trainer.ResidentEval: the "batch" of a test step read from the HBM-resident test store (same dict as
        ``resident_batch``), or None under the conditions ``resident_batch`` refuses."""
        return self.resident_batch(store, cur_desc, B_cap, T_cap, N_cap)

    def resident_eval_step(self, batch, cm):
        """one forward-only step (eval mode, a workspace of its own) scored on the device: adds the batch's confusion matrix
        to ``cm`` (int64 [C, C]); no host sync; neither the training flag nor the dropout counter is touched.  Returns the
        step's buffers (the caller of a captured step keeps them alive)."""
        return self.model.eval_scores(batch, cm)
