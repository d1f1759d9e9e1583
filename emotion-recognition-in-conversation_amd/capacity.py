"""What the trainers share: the batch preparation and the plain training step (``TrainerBase``), the constructor of the
conv-emotion family (``ConvEmotionTrainer``), and capacity mode's host side (``CapacityBuckets``) -- the buckets ``trainer.StepGraphs`` replays and the resident batch ``trainer.ResidentEpochs``
steps over.  A trainer in capacity mode keeps only its policy: N_BUCKET, the layout, the gate, the precapture list and
the exact-shape rule (the table in DESIGN.md, "capacity mode: one implementation, per-trainer policy")."""
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


class TrainerBase:
    """``prepare_batch`` / ``to_logits`` / the plain ``train_step`` of a trainer with ``params``, ``device``, ``model``,
    ``optim`` and ``class_weight``."""
    BF16_INPUT = False     # True: ``--compute=bf16`` casts the features once, here (COGMEN, DialogueGCN, DAG-ERC)

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
        """forward + class-weighted loss + backward + (DP all-reduce) + Adam.  Returns the device stats tensor."""
        self.model.train()
        stats = self.model.loss_and_grads(batch, self.class_weight)
        scale = all_reduce_grads(self.model.flat)
        self.optim.step(grad_scale=scale)
        return stats


class ConvEmotionTrainer(TrainerBase):
    """What the trainers of the conv-emotion family (bc-LSTM / bc-GRU, DialogueRNN, conv-emotion DialogueGCN) share: fp32
    only, the class-weighted loss, Adam lr 3e-4 without weight decay (track_mm/dgcnv2.py:22-48,184-219), and the dropout
    counter of the model living in the optimizer.  A subclass names its ``--module`` value and builds its model."""
    NAME = None

    def __init__(self, params, device):
        self.params, self.device = params, torch.device(device)
        compute = params.get("compute", "f32")
        if compute != "f32":
            raise capi.ErcGraftError("--module=%s runs in fp32 (the reference is fp32); --compute=%s is not supported"
                                     % (self.NAME, compute))
        self.class_weight = None
        if params.get("loss_weights", True):
            if params.n_classes != 6:
                raise capi.ErcGraftError("--loss_weights uses the six hard-coded IEMOCAP-6 inverse frequencies "
                                         "(dgcnv2.py:213-214); run %d-class datasets with --loss_weights=False" % params.n_classes)
            self.class_weight = torch.tensor(IEMOCAP6_WEIGHTS, dtype=torch.float32, device=self.device)
        torch.manual_seed(params.seed)
        self.model = self._build_model(params, compute).finalize(self.device)
        o = params.optim
        self.optim = FusedAdam(self.model.flat, lr=o.lr, weight_decay=o.get("weight_decay", 0.0),
                               decoupled=(o.name == "AdamW"), seed=params.seed)
        self.model.rng_state = self.optim.rng_state

    def _build_model(self, params, compute):
        raise NotImplementedError


class CapacityBuckets:
    """Capacity mode of a trainer.  A bucket is a set of static buffers for B_cap dialogue slots (missing ones get length 0)
    of T_cap utterances and N_cap labels, keyed ``("capacity", B_cap, T_cap, N_cap)``; B_cap is at least train.batch_size,
    T_cap at least ``self.t_cap`` (the longest training dialogue of every rank, set by trainer.run), N_cap the batch's node
    count rounded up to N_BUCKET.  The trainer supplies ``_capacity_ok`` (the gate), ``_precapture_caps`` (the list a data
    parallel run captures up front) and ``_resident_ok``; it may replace ``_bucket`` (another layout) and
    ``_resident_inputs``."""
    N_BUCKET = 128             # node counts are rounded up to a multiple of this (the node launches scale with N_cap)
    TIME_MAJOR = False         # input_tensor / speaker_tensor are [T, B, ...] instead of [B, T, ...]
    EXACT_SHAPE_STAYS = True   # a batch that already has its bucket's shape gets no bucket: there is nothing to pad
    capacity = True            # False: every step keeps its exact shape

    def _p2p(self):
        """the opt-in peer-to-peer gradient exchange (ERC_DP_P2P=1): capacity buckets stay off there"""
        return getattr(self.model.flat, "p2p", None) is not None or os.environ.get("ERC_DP_P2P", "0") == "1"

    def _bt(self, batch):
        a, b = batch["input_tensor"].shape[:2]
        return (b, a) if self.TIME_MAJOR else (a, b)

    def _caps(self, batch):
        B, T = self._bt(batch)
        return max(B, int(self.params.train.batch_size)), max(T, int(getattr(self, "t_cap", 0)))

    def _bucket(self, like, B_cap, T_cap, N_cap):
        """(key, make, fill) of one bucket, batch-first; ``like`` gives the feature width and the dtypes"""
        x, spk, dev, D = like["input_tensor"], like["speaker_tensor"], self.device, like["input_tensor"].shape[2]

        def make():
            return dict(input_tensor=torch.zeros(B_cap, T_cap, D, dtype=x.dtype, device=dev),
                        speaker_tensor=torch.zeros(B_cap, T_cap, dtype=spk.dtype, device=dev),
                        text_length=torch.zeros(B_cap, dtype=like["text_length"].dtype, device=dev),
                        label=torch.zeros(N_cap, dtype=like["label"].dtype, device=dev))

        def fill(static, b):
            Bb, Tb = b["input_tensor"].shape[:2]
            static["input_tensor"][:Bb, :Tb].copy_(b["input_tensor"], non_blocking=True)
            static["speaker_tensor"][:Bb, :Tb].copy_(b["speaker_tensor"], non_blocking=True)
            static["text_length"].zero_()                     # dialogues the batch does not have: length 0
            static["text_length"][:Bb].copy_(b["text_length"], non_blocking=True)
            static["label"][:b["label"].shape[0]].copy_(b["label"], non_blocking=True)

        return ("capacity", B_cap, T_cap, N_cap), make, fill

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
