"""MMIN's full-modality base model on the MI355X hot path (drop-in for MMINBaseModule, track_mm/mmin_models.py:202-240, and the
trainer of track_mm/mmin_base.py): an utterance classifier over three encoders -- a hidden-128 LSTM with a max-pool over time
for the audio frames and one for the visual frames (LSTMEncoder 'maxpool', :43-95), a text CNN over the BERT token rows
(TextCNN, :8-40) -- and a three-layer classifier over their concatenation (Classifier, :98-130).  ``mmin_miss`` / ``mmin_miss2``
start from this model's checkpoint and reuse its encoders through ``encode``: ``mmin_miss`` is erc_amd/mmin_miss.py,
``mmin_miss2`` is not built.

``MMINBaseModule`` keeps the reference's constructor signature, its ``state_dict`` key for key and shape for shape (22 tensors,
2 063 620 parameters at 342 / 1024 / 130 / 4, all live) and ``forward(**batch) -> (logits [B, C], feat [B, 128])``.  Built: fp32,
all three modalities, text of at least erc_textcnn_min_t() = 5 tokens; anything else raises ``ErcGraftError`` naming the argument.

Batches are batch-first: audio [B, Ta, 130] zero-padded to the batch's longest utterance (the LSTM runs over ALL padded steps
and they take part in the maximum, as in the reference, which packs nothing), visual [B, 50, 342], text [B, 22, 1024].

Launches of a training step:
  forward   GX_a = x_a W_ih^T + b (GEMM) | GX_v (GEMM) | erc_lstm128_pool_fwd (both encoders, one launch) -> fused[:, 0:256]
            erc_textcnn_pool_fwd (3 GEMMs over overlapping rows, K cut in 8, + pool) | erc_dropout_fwd 0.5 | embd GEMM + ReLU -> fused[:, 256:384]
            netC.module.0 GEMM + ReLU + dropout 0.3 | netC.module.3 likewise -> feat | fc_out GEMM | erc_cross_entropy
  backward  3 GEMMs with the ReLU / dropout mask in the epilogue down to dfused | the text slice's GEMM (ReLU mask) | dpooled GEMM
            | erc_dropout_fwd on the gradient (same mask) | erc_textcnn_pool_bwd | erc_lstm128_pool_bwd (one launch)
            | erc_wgrad_table: every Linear / LSTM weight gradient and bias sum, one launch
  update    erc_adam_step | erc_ema_step

From HBM (opt-in): in capacity mode a batch that carries ``counts`` (device int32 {B, Ta}) is a BUCKET --
fixed buffers of train.batch_size slots and an audio capacity of a multiple of 64 frames -- and the step above runs on it with
erc_lstm128_pool_fwd_tcap / _bwd_tcap and erc_cross_entropy_cap + erc_mm_zero_tail; every other launch is the same.
``--capacity_buckets=True`` feeds host-collated batches through trainer.StepGraphs, ``--device_collate --resident`` keeps the
training split in a datasets.MMINDeviceStore and replays erc_mmin_collate + step + Adam + EMA per 3 B int32
(``MMINResidentEpochs``), ``--resident_eval`` scores the validation and test epochs on the device (``MMINResidentEval``).

The two baselines of the missing-modality model (opt-in; the masking is MMINMissCollate's, erc_amd/mmin_miss.py):
``--eval_missing`` also scores the validation and test epochs under the six patterns of ``MISSING_TYPES`` behind every batch's
unchanged forward -- erc_mmin_miss_expand of the batch's features against the zero-input features | the three classifier GEMMs on
6 B rows | erc_mmin_miss_score -- with the zero-input audio features of EVERY padded length from one scan over t_max + 1 zero
frames (erc_lstm128_prefix_max over its saved hidden rows); under ``--resident_eval`` the captured step gains the same route in
capacity form (erc_mmin_miss_expand_cap, erc_mmin_miss_score_cap).  ``--train_missing`` trains on inputs masked at random as
``mmin_miss`` trains: the loaders get the ``Missing`` transform and a masking collate, a resident step collates with
erc_mmin_collate_masked from 4 B int32 (the fourth block: the slots' keep bits, drawn on the host from ``random``).
"""
import json
import os
import random
import time

import numpy as np
import torch
from torch import nn

from . import capi
from .capacity import TrainerBase
from .datasets import MMINDeviceStore, MMINMaskedDeviceStore, index_batches, mmin_t_cap
from .engine import FlatParams, GemmPlanner, WorkspaceCache, _world_size, linear_fwd, linear_wgrad
from .trainer import (ResidentLoop, StepGraphs, classification_report, dynamic_n, epoch_loop_class, fix_seed, print_step_lines,
                      report_from_cm, setup_device, train_epoch_loader)

HID, EMB = 128, 384
AUDIO_DIM, VISUAL_DIM, TEXT_DIM = 130, 342, 1024     # mmin_base.py:86-91: constants of the trainer
STREAM_TEXT = 0x7E770                                  # dropout stream of the pooled text (erc_dropout_fwd)
SALT_C0, SALT_C1 = 0xC0 << 32, 0xC1 << 32             # seeds of the two classifier dropouts (the GEMM epilogue has no stream)
EMA_ALPHA = 0.999                                      # mmin_base.py:99
MISSING_TYPES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1))     # mmin_miss.py:348-353, columns visual, text, audio
MODAL_KEYS = ("visual_feature", "text_feature", "audio_feature")                        # mmin_miss.py:354, :332
# --eval_missing: a pattern's name is the modalities that REMAIN, in the project's a t v letters: "v", "t", "a", "tv", "av", "at"
MISSING_KEYS = tuple("".join(c for c, i in (("a", 2), ("t", 1), ("v", 0)) if m[i]) for m in MISSING_TYPES)
MISSING_PATTERNS = capi.mmin_miss_patterns(MISSING_TYPES)      # bit 0 visual, bit 1 text, bit 2 audio kept


# parameter holders with the reference's attribute names (state_dict keys); the math is in libercgraft
class _TextCNN(nn.Module):
    def __init__(self, input_dim):
        super().__init__()
        self.conv1 = nn.Conv2d(1, HID, (3, input_dim))
        self.conv2 = nn.Conv2d(1, HID, (4, input_dim))
        self.conv3 = nn.Conv2d(1, HID, (5, input_dim))
        self.embd = nn.Sequential(nn.Linear(3 * HID, HID), nn.ReLU(inplace=True))


class _LSTMEncoder(nn.Module):
    def __init__(self, input_size):
        super().__init__()
        self.rnn = nn.LSTM(input_size, HID, batch_first=True)


class _Classifier(nn.Module):
    def __init__(self, input_dim, n_classes):
        super().__init__()
        # creation order of the reference (the hidden layers, then fc_out), registration order of its state_dict (fc_out first)
        layers = [nn.Linear(input_dim, HID), nn.ReLU(), nn.Dropout(0.3), nn.Linear(HID, HID), nn.ReLU(), nn.Dropout(0.3)]
        self.fc_out = nn.Linear(HID, n_classes)
        self.module = nn.Sequential(*layers)


class MMINBaseModule(nn.Module):
    NAME = "mmin_base"
    DROP_TEXT, DROP_C = 0.5, 0.3
    dynamic_n = False      # capacity mode (trainer.dynamic_n): a batch with ``counts`` is a bucket, its sizes are capacities

    def __init__(self, visual_dim=0, text_dim=0, audio_dim=0, n_classes=4, compute="f32", seed=1):
        super().__init__()
        if compute != "f32":
            raise capi.ErcGraftError("%s runs in fp32 only (the reference is fp32); compute=%r is not supported" % (self.NAME, compute))
        for name, d in (("visual_dim", visual_dim), ("text_dim", text_dim), ("audio_dim", audio_dim)):
            if int(d) < 1:
                raise capi.ErcGraftError("%s: %s=%r: all three encoders are read (their outputs side by side are %d wide)" % (self.NAME, name, d, EMB))
        if int(n_classes) < 2:
            raise capi.ErcGraftError("%s: n_classes=%r" % (self.NAME, n_classes))
        self.visual_dim, self.text_dim, self.audio_dim = int(visual_dim), int(text_dim), int(audio_dim)
        self.n_classes, self.compute = int(n_classes), compute
        self.netL = _TextCNN(self.text_dim)
        self.netA = _LSTMEncoder(self.audio_dim)
        self.netV = _LSTMEncoder(self.visual_dim)
        self._build_head()
        self.flat, self._ws, self._seed = None, WorkspaceCache(), seed

    def _build_head(self):
        """what follows the encoders, in the reference's registration order (MMINMissModule: the autoencoders come first)"""
        self.netC = _Classifier(EMB, self.n_classes)

    # ------------------------------------------------------------------------------------------------------------ set-up
    def finalize(self, device):
        self.to(device)
        self.flat = FlatParams([[(n, p)] for n, p in self.named_parameters()], device)
        self.rng_state = torch.tensor([0, self._seed], dtype=torch.int64, device=device)
        self._salt = torch.tensor([[0, SALT_C0], [0, SALT_C1]], dtype=torch.int64, device=device)
        self._rng2 = torch.zeros(2, 2, dtype=torch.int64, device=device)
        return self

    @property
    def _last_ws(self):
        return self._ws.last

    def _w(self, name):
        return self.flat.w(name)

    def _off(self, name):
        return self.flat.offsets[name]

    def _make_workspace(self, B, Ta, Tv, Tt, device):
        # zeros, not empty: a stale NaN must never reach a weight-gradient GEMM through a row the step did not touch
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)
        C = self.n_classes
        ws = dict(fused=f32(B, EMB), dfused=f32(B, EMB), z0=f32(B, HID), feat=f32(B, HID), logits=f32(B, C), dlogits=f32(B, C),
                  dfeat=f32(B, HID), dz0=f32(B, HID), dtext=f32(B, HID), stats=f32(256))
        for tag, T in (("A", Ta), ("V", Tv)):
            if T:
                ws[tag] = dict(T=T, GX=f32(B * T, 4 * HID), gates=f32(B * T, 4 * HID), Cst=f32(B * T, HID), Hprev=f32(B * T, HID),
                               dGX=f32(B * T, 4 * HID), arg=i32(B, HID))
        if Tt:
            ws["L"] = dict(T=Tt, conv=f32(capi.textcnn_conv_floats(B, Tt)), pooled=f32(B, EMB), pd=f32(B, EMB), arg=i32(B, EMB), dpd=f32(B, EMB),
                           dpooled=f32(B, EMB))
        jobs = []
        for n, (tag, net) in enumerate((("A", "netA"), ("V", "netV"))):
            if tag in ws:
                e = ws[tag]
                jobs.append(dict(GX=e["GX"], W_hh=self._w(net + ".rnn.weight_hh_l0"), b_hh=self._w(net + ".rnn.bias_hh_l0"),
                                 pool=ws["fused"][:, n * HID:], arg=e["arg"], gates=e["gates"], Cst=e["Cst"], Hprev=e["Hprev"],
                                 dpool=ws["dfused"][:, n * HID:], dGX=e["dGX"], B=B, T=e["T"], ldp=EMB, lddp=EMB))
        ws["n_jobs"], ws["jobs"] = len(jobs), capi.lstm128_jobs(jobs)
        ws["dyn_mask"] = 1 if "A" in ws else 0      # capacity mode: the audio job (the first) reads its length from the device
        ws["planner"] = GemmPlanner(device, 1 << 16, grad=self.flat.grad)
        return ws

    def _inputs(self, audio, visual, text, need_all):
        got = dict(audio_feature=(audio, self.audio_dim), visual_feature=(visual, self.visual_dim), text_feature=(text, self.text_dim))
        B = None
        for name, (x, d) in got.items():
            if x is None:
                if need_all:
                    raise capi.ErcGraftError("%s: %s is missing: all three encoders are read (their outputs side by side are %d "
                                             "wide)" % (self.NAME, name, EMB))
                continue
            if x.dim() != 3 or int(x.shape[2]) != d or x.dtype != torch.float32 or int(x.shape[1]) < 1:
                raise capi.ErcGraftError("%s: %s must be fp32 [B, T >= 1, %d], got %s %s" % (self.NAME, name, d, x.dtype, tuple(x.shape)))
            if B is not None and int(x.shape[0]) != B:
                raise capi.ErcGraftError("%s: %s has %d samples, the batch %d" % (self.NAME, name, int(x.shape[0]), B))
            B = int(x.shape[0])
        if B is None:
            raise capi.ErcGraftError("%s: encode needs at least one of audio_feature, visual_feature, text_feature" % self.NAME)
        if text is not None and int(text.shape[1]) < capi.textcnn_min_t():
            raise capi.ErcGraftError("%s: text_feature has %d tokens, the widest convolution needs %d"
                                     % (self.NAME, int(text.shape[1]), capi.textcnn_min_t()))
        return B

    # ----------------------------------------------------------------------------------------------------------- forward
    def _encode(self, audio, visual, text, training, need_all=False, counts=None):
        """the encoders that have an input, into their column ranges of ws["fused"].  ``counts`` (device int32 {B, Ta}, written
        by erc_mmin_collate or by the bucket's fill): the inputs are a bucket's, B and the audio length are capacities, and the
        scans and the loss read the batch's own sizes from it; a bucket has workspaces of its own, one
        for training and one for evaluation"""
        if self.flat is None:
            raise capi.ErcGraftError("call %s.finalize(device) before forward" % type(self).__name__)
        B = self._inputs(audio, visual, text, need_all)
        T = [0 if x is None else int(x.shape[1]) for x in (audio, visual, text)]
        dev = next(x for x in (audio, visual, text) if x is not None).device
        key = (B, *T) if counts is None else (B, *T, "capacity", bool(training))
        ws = self._ws.get(key, lambda: self._make_workspace(B, *T, dev))
        ws["counts"] = counts
        pl = ws["planner"]
        pl.reset()
        for tag, net, x in (("A", "netA", audio), ("V", "netV", visual)):
            if x is not None:
                e = ws[tag]
                e["x"] = x = x.contiguous()
                linear_fwd(pl, x, int(x.shape[2]), None, self._w(net + ".rnn.weight_ih_l0"), self._w(net + ".rnn.bias_ih_l0"), e["GX"],
                           4 * HID, B * e["T"], 4 * HID, int(x.shape[2]))
        if ws["n_jobs"] and counts is None:
            capi.lstm128_pool_fwd(ws["jobs"], ws["n_jobs"])
        elif ws["n_jobs"]:
            capi.lstm128_pool_fwd_tcap(ws["jobs"], counts, ws["dyn_mask"], ws["n_jobs"])
        if text is not None:
            e = ws["L"]
            e["x"] = x = text.contiguous()
            capi.textcnn_pool_fwd(x, B, e["T"], self.text_dim, [self._w("netL.conv%d.weight" % k) for k in (1, 2, 3)],
                                  [self._w("netL.conv%d.bias" % k) for k in (1, 2, 3)], e["conv"], e["pooled"], EMB, e["arg"])
            e["p"] = self.DROP_TEXT if training else 0.0
            if e["p"] > 0:
                capi.dropout_fwd(e["pooled"], B * EMB, e["p"], self.rng_state, STREAM_TEXT, e["pd"])
            e["in"] = e["pd"] if e["p"] > 0 else e["pooled"]
            linear_fwd(pl, e["in"], EMB, None, self._w("netL.embd.0.weight"), self._w("netL.embd.0.bias"), ws["fused"][:, 2 * HID:], EMB,
                       B, HID, EMB, act=1)
        return ws, B

    def encode(self, audio_feature=None, visual_feature=None, text_feature=None, *args, **kwargs):
        """the [B, 128] features of the modalities given, in the order audio, visual, text (mmin_models.py:213-226)"""
        ws, _ = self._encode(audio_feature, visual_feature, text_feature, self.training)
        return [ws["fused"][:, n * HID:(n + 1) * HID] for n, x in enumerate((audio_feature, visual_feature, text_feature)) if x is not None]

    def _classifier_fwd(self, ws, B, xin, k_in, training):
        """netC on ``xin`` [B, k_in]: two Linear + ReLU + dropout 0.3 layers (the mask in the GEMM epilogue) -> feat, fc_out -> logits"""
        pl, C = ws["planner"], self.n_classes
        p = ws["p_c"] = self.DROP_C if training else 0.0
        if p > 0:
            torch.add(self.rng_state.unsqueeze(0), self._salt, out=self._rng2)
        for n, (name, x, k, out) in enumerate((("netC.module.0", xin, k_in, ws["z0"]), ("netC.module.3", ws["z0"], HID, ws["feat"]))):
            linear_fwd(pl, x, k, None, self._w(name + ".weight"), self._w(name + ".bias"), out, HID, B, HID, k,
                       act=3 if p > 0 else 1, drop_p=p, rng=self._rng2[n] if p > 0 else None)
        linear_fwd(pl, ws["feat"], HID, None, self._w("netC.fc_out.weight"), self._w("netC.fc_out.bias"), ws["logits"], C, B, C, HID)

    def _forward_impl(self, audio, visual, text, training, counts=None):
        ws, B = self._encode(audio, visual, text, training, need_all=True, counts=counts)
        self._classifier_fwd(ws, B, ws["fused"], EMB, training)
        return ws, B

    def _counts(self, batch):
        """the bucket's {B, Ta} in capacity mode, None for an exact-shape batch"""
        return batch.get("counts") if self.dynamic_n else None

    def forward(self, audio_feature=None, visual_feature=None, text_feature=None, *args, **kwargs):
        ws, _ = self._forward_impl(audio_feature, visual_feature, text_feature, self.training, self._counts(kwargs))
        return ws["logits"], ws["feat"]

    def eval_scores(self, batch, cm, loss_sum):
        """one evaluation step of a bucket scored on the device: the forward in eval mode (its own workspace; neither the
        training flag nor the dropout counter is touched), the batch-mean cross entropy ADDED to ``loss_sum`` (float64 [1]) and
        the batch's confusion matrix added to ``cm`` (int64 [C, C], true x predicted).  No host sync.  -> the workspace"""
        C, cnt = self.n_classes, batch["counts"]
        ws, B = self._forward_impl(batch["audio_feature"], batch["visual_feature"], batch["text_feature"], False, cnt)
        capi.cross_entropy_cap(ws["logits"], C, C, B, cnt, None, batch["label"], None, 1.0, None, C, ws["stats"])
        loss_sum.add_(ws["stats"][:1])
        capi.rows_score(ws["logits"], C, B, C, B, cnt, None, batch["label"], cm)
        ms = batch.get("missing")
        if ms is not None:      # --eval_missing: the six patterns behind it, against the pass's zero-input table (fixed buffers)
            m = self._missing_buffers(ws, B)
            capi.mmin_miss_expand_cap(ws["fused"], EMB, ms["zaudio"], int(ms["zaudio"].shape[0]), ms["zvt"], cnt, MISSING_PATTERNS, B,
                                      m["x"], EMB)
            self._classifier_rows(m["x"], EMB, m, len(MISSING_TYPES) * B)
            capi.mmin_miss_score_cap(m["logits"], C, batch["label"], B, cnt, len(MISSING_TYPES), C, ms["cm"], ms["sums"])
        return ws

    # --------------------------------------------------------------------------------- evaluation under missing modalities
    zero_scans = 0      # audio zero-input scans so far (tests count them per pass)

    def _zero_encode_ws(self, audio, visual, text):
        """the encoders on zero inputs of one sample, in workspaces of their own (the batch's workspace and ``_last_ws`` stay)"""
        if not hasattr(self, "_zero_ws"):
            self._zero_ws = WorkspaceCache(maxsize=8)
        batch_ws, self._ws = self._ws, self._zero_ws
        try:
            ws, _ = self._encode(audio, visual, text, False)
        finally:
            self._ws = batch_ws
        return ws

    def _zero_encode(self, audio, visual, text):
        return self._zero_encode_ws(audio, visual, text)["fused"][0]

    def zero_table(self, t_max, Tv, Tt, device, out=None):
        """dict(zaudio [t_max + 1, 128], zvt [256]): what the encoders make of a sample whose inputs are zero (MMINMissCollate's
        masking: a missing modality is a zero input that still runs through its encoder).  Row Ta of ``zaudio`` = the audio
        columns at a padded length of Ta frames, row 0 unused: ONE scan over t_max + 1 zero frames saves h_0 .. h_{t_max - 1}
        (Hprev[t] = h_{t-1}) and erc_lstm128_prefix_max forms the pool after every number of steps.  ``out``: buffers to fill
        in place (a captured step reads them: the EMA pass swaps their contents)"""
        zeros = lambda T, d: torch.zeros(1, T, d, dtype=torch.float32, device=device)
        if out is None:
            out = dict(zaudio=torch.zeros(t_max + 1, HID, dtype=torch.float32, device=device),
                       zvt=torch.zeros(2 * HID, dtype=torch.float32, device=device))
        if tuple(out["zaudio"].shape) != (t_max + 1, HID) or tuple(out["zvt"].shape) != (2 * HID, ):
            raise capi.ErcGraftError("%s: zero_table: buffers %s / %s for t_max=%d" % (self.NAME, tuple(out["zaudio"].shape),
                                                                                      tuple(out["zvt"].shape), t_max))
        out["zvt"].copy_(self._zero_encode(None, zeros(Tv, self.visual_dim), zeros(Tt, self.text_dim))[HID:])
        ws = self._zero_encode_ws(zeros(t_max + 1, self.audio_dim), None, None)
        capi.lstm128_prefix_max(ws["A"]["Hprev"], t_max + 1, out["zaudio"])
        self.zero_scans += 1
        return out

    def begin_missing_pass(self, t_max=None):
        """forget the zero-input features: they are constants of the weights, so a pass over other weights (the EMA copy swapped
        in, a training step in between) starts with this.  ``t_max``: the longest padded audio length the pass will meet (the
        table is rebuilt when a longer one comes up)"""
        self._ztab, self._zrow, self._z_tmax = None, {}, int(t_max or 0)

    def zero_features(self, Ta, Tv, Tt, device):
        """[384]: the zero-input features at a padded audio length of ``Ta`` frames, from the pass's table"""
        if not hasattr(self, "_zrow"):
            self.begin_missing_pass()
        z = self._zrow.get((Ta, Tv, Tt))
        if z is None:
            if self._ztab is None or self._ztab["key"] != (Tv, Tt) or Ta >= int(self._ztab["zaudio"].shape[0]):
                self._ztab = self.zero_table(max(Ta, self._z_tmax), Tv, Tt, device)
                self._ztab["key"], self._zrow = (Tv, Tt), {}
            z = self._zrow[Ta, Tv, Tt] = torch.cat([self._ztab["zaudio"][Ta], self._ztab["zvt"]])
        return z

    def _missing_buffers(self, ws, B):
        """the buffers of the 6 B rows behind the forward whose workspace is ``ws`` (they live and die with it)"""
        if "miss" not in ws:
            K, dev = len(MISSING_TYPES), ws["fused"].device
            f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
            ws["miss"] = dict(x=f32(K * B, EMB), z0=f32(K * B, HID), feat=f32(K * B, HID), logits=f32(K * B, self.n_classes))
        return ws["miss"]

    def _classifier_rows(self, x, k_in, m, rows):
        """netC in eval mode on ``x`` [rows, k_in] into m["z0"], m["feat"], m["logits"]: three GEMMs, no dropout"""
        C = self.n_classes
        for name, xin, k, out, n, act in (("netC.module.0", x, k_in, m["z0"], HID, 1), ("netC.module.3", m["z0"], HID, m["feat"], HID, 1),
                                          ("netC.fc_out", m["feat"], HID, m["logits"], C, 0)):
            capi.gemm_f32(xin, k, 0, None, self._w(name + ".weight"), k, 0, None, out, n, rows, n, k, bias=self._w(name + ".bias"), act=act)

    def score_missing(self, labels, cm, loss_sum):
        """the batch of the forward just run (eval mode), scored under the six patterns of MISSING_TYPES without a second pass
        over its inputs: its features (``fused`` of that forward) expanded against the zero-input features (1 launch), the
        classifier on the 6 B rows (3 GEMMs; this model has no autoencoder in between) and erc_mmin_miss_score, which adds the
        confusion matrices to ``cm`` (int64 [6, C, C]) and the batch-mean cross entropies to ``loss_sum`` (float64 [6]).
        Nothing is copied to the host; no random draw, no state changes.  -> the logits [6 B, C] (a workspace buffer)"""
        ws = self._last_ws
        if ws is None or self.training:
            raise capi.ErcGraftError("%s: score_missing follows a forward in eval mode" % self.NAME)
        B, C, K, dev = int(ws["fused"].shape[0]), self.n_classes, len(MISSING_TYPES), ws["fused"].device
        if tuple(labels.shape) != (B, ) or labels.dtype != torch.int64:
            raise capi.ErcGraftError("%s: score_missing: labels must be int64 [%d], got %s %s" % (self.NAME, B, labels.dtype, tuple(labels.shape)))
        z = self.zero_features(ws["A"]["T"], ws["V"]["T"], ws["L"]["T"], dev)
        m = self._missing_buffers(ws, B)
        capi.mmin_miss_expand(ws["fused"], EMB, z, MISSING_PATTERNS, B, m["x"], EMB)
        self._classifier_rows(m["x"], EMB, m, K * B)
        capi.mmin_miss_score(m["logits"], C, labels, B, K, C, cm, loss_sum)
        return m["logits"]

    # ---------------------------------------------------------------------------------------------------------- backward
    def _classifier_bwd(self, ws, B, xin, k_in, labels, stats):
        """mean cross entropy of the logits into ``stats`` and netC's backward down to ws["dz0"] (the gradient wrt the first
        layer's pre-activation).  Each layer's weight gradient joins the step's batched launch; the gradient wrt its input goes
        through the ReLU / dropout mask of the layer below in the GEMM epilogue (aux = that layer's output)"""
        pl, C, p = ws["planner"], self.n_classes, ws["p_c"]
        scale = 1.0 / (1.0 - p)
        if ws["counts"] is None:
            capi.cross_entropy(ws["logits"], C, C, B, None, labels, None, 1.0, ws["dlogits"], C, stats)
        else:      # the mean over the batch's own samples; dlogits rows beyond them are zero, and so is every gradient row below
            capi.cross_entropy_cap(ws["logits"], C, C, B, ws["counts"], None, labels, None, 1.0, ws["dlogits"], C, stats)
            capi.mm_zero_tail(ws["dlogits"], C, C, 1, B, ws["counts"])
        linear_wgrad(pl, ws["dlogits"], C, ws["feat"], HID, None, C, HID, B, self._off("netC.fc_out.weight"), self._off("netC.fc_out.bias"),
                     defer=True)
        capi.gemm_f32(ws["dlogits"], C, 0, None, self._w("netC.fc_out.weight"), HID, 1, None, ws["dfeat"], HID, B, HID, C, act=2,
                      aux=ws["feat"], ldaux=HID, act_scale=scale)
        linear_wgrad(pl, ws["dfeat"], HID, ws["z0"], HID, None, HID, HID, B, self._off("netC.module.3.weight"),
                     self._off("netC.module.3.bias"), defer=True)
        capi.gemm_f32(ws["dfeat"], HID, 0, None, self._w("netC.module.3.weight"), HID, 1, None, ws["dz0"], HID, B, HID, HID, act=2,
                      aux=ws["z0"], ldaux=HID, act_scale=scale)
        linear_wgrad(pl, ws["dz0"], HID, xin, k_in, None, HID, k_in, B, self._off("netC.module.0.weight"),
                     self._off("netC.module.0.bias"), defer=True)

    def _encoders_bwd(self, ws, B):
        """from ws["dfused"][:, 0:256] (the two scans' dpool) and ws["dtext"] (the gradient wrt embd's pre-activation) down to
        every encoder gradient"""
        pl, e = ws["planner"], ws["L"]
        linear_wgrad(pl, ws["dtext"], HID, e["in"], EMB, None, HID, EMB, B, self._off("netL.embd.0.weight"), self._off("netL.embd.0.bias"),
                     defer=True)
        capi.gemm_f32(ws["dtext"], HID, 0, None, self._w("netL.embd.0.weight"), EMB, 1, None, e["dpd"], EMB, B, EMB, HID)
        if e["p"] > 0:      # the forward's mask: same counter, same stream, same element index
            capi.dropout_fwd(e["dpd"], B * EMB, e["p"], self.rng_state, STREAM_TEXT, e["dpooled"])
        g = self.flat.g
        capi.textcnn_pool_bwd(e["x"], B, e["T"], self.text_dim, e["pooled"], EMB, e["arg"], e["dpooled"] if e["p"] > 0 else e["dpd"], EMB,
                              [g("netL.conv%d.weight" % k) for k in (1, 2, 3)], [g("netL.conv%d.bias" % k) for k in (1, 2, 3)])
        if ws["counts"] is None:
            capi.lstm128_pool_bwd(ws["jobs"], ws["n_jobs"])
        else:
            capi.lstm128_pool_bwd_tcap(ws["jobs"], ws["counts"], ws["dyn_mask"], ws["n_jobs"])
        for tag, net in (("A", "netA"), ("V", "netV")):
            s, rows = ws[tag], B * ws[tag]["T"]
            d = int(s["x"].shape[2])
            linear_wgrad(pl, s["dGX"], 4 * HID, s["x"], d, None, 4 * HID, d, rows, self._off(net + ".rnn.weight_ih_l0"),
                         self._off(net + ".rnn.bias_ih_l0"), defer=True)
            linear_wgrad(pl, s["dGX"], 4 * HID, s["Hprev"], HID, None, 4 * HID, HID, rows, self._off(net + ".rnn.weight_hh_l0"),
                         self._off(net + ".rnn.bias_hh_l0"), defer=True)

    def loss_and_grads(self, batch):
        """mean cross entropy of the logits (mmin_base.py:131) and every gradient into flat.grad; returns the device stats
        (stats[0] = loss, stats[1] = #correct)"""
        ws, B = self._forward_impl(batch.get("audio_feature"), batch.get("visual_feature"), batch.get("text_feature"), self.training,
                                   self._counts(batch))
        self._classifier_bwd(ws, B, ws["fused"], EMB, batch["label"], ws["stats"])
        # dfused: the audio | visual columns as they are (dpool of the two scans), the text columns through embd's ReLU
        W0 = self._w("netC.module.0.weight")
        capi.gemm_f32(ws["dz0"], HID, 0, None, W0, EMB, 1, None, ws["dfused"], EMB, B, 2 * HID, HID)
        capi.gemm_f32(ws["dz0"], HID, 0, None, W0[:, 2 * HID:], EMB, 1, None, ws["dtext"], HID, B, HID, HID, act=2,
                      aux=ws["fused"][:, 2 * HID:], ldaux=EMB, act_scale=1.0)
        self._encoders_bwd(ws, B)
        ws["planner"].reduce_into(ws, self.flat.grad)
        return ws["stats"]


# ---------------------------------------------------------------------------------------------------------------- training
class PlateauLR:
    """torch.optim.lr_scheduler.ReduceLROnPlateau(optim, "min") with torch's defaults (factor 0.1, patience 10, relative
    threshold 1e-4, no cooldown, min_lr 0, eps 1e-8) on a host scalar"""

    def __init__(self, lr, factor=0.1, patience=10, threshold=1e-4, eps=1e-8):
        self.lr, self.factor, self.patience, self.threshold, self.eps = lr, factor, patience, threshold, eps
        self.best, self.bad = float("inf"), 0

    def step(self, metric):
        """-> the learning rate after this epoch's metric"""
        metric = float(metric)
        if metric < self.best * (1.0 - self.threshold):
            self.best, self.bad = metric, 0
        else:
            self.bad += 1
        if self.bad > self.patience:
            new = self.lr * self.factor
            if self.lr - new > self.eps:
                self.lr = new
            self.bad = 0
        return self.lr


class MMINBaseTrainer(TrainerBase):
    """``--module=mmin_base``: mean cross entropy, Adam (lr 2e-4, no weight decay), the EMA copy stepped after every optimizer
    step, ReduceLROnPlateau on the validation loss, the best checkpoint by test accuracy (mmin_base.py:63-217).
    ``prepare_batch``, ``to_logits`` and the optimizer set-up are TrainerBase's (a batch of this module has no ``text_length``:
    no ``n_nodes`` is added)."""
    NAME = "mmin_base"
    MODULE = MMINBaseModule
    CLASS_WEIGHTED = False
    CAPACITY_MODES = True      # --capacity_buckets, --device_collate --resident, --resident_eval are built (mmin_miss: refused)
    # EPOCH_LOOP = MMINEpochLoop: assigned below the loop's definition, at the end of this file (trainer.epoch_loop_class)
    capacity = False           # --capacity_buckets / --resident: host batches go through buckets (StepGraphs.capacity_bucket)
    t_cap = 0                  # the training split's longest utterance: no bucket is longer (set by MMINEpochLoop)

    def __init__(self, params, device):
        self.params, self.device = params, torch.device(device)
        if self.CAPACITY_MODES:
            if max(_world_size(), int(os.environ.get("WORLD_SIZE", "1"))) > 1 and any(params.get(k) for k in CAPACITY_FLAGS):
                raise capi.ErcGraftError("--module=%s: %s are built for one rank; data-parallel runs keep the default loop"
                                         % (self.NAME, ", ".join("--" + k for k in CAPACITY_FLAGS)))
            self.capacity = bool(params.get("capacity_buckets", False) or params.get("resident", False))
        torch.manual_seed(params.seed)
        self.model = self.MODULE(visual_dim=VISUAL_DIM, text_dim=TEXT_DIM, audio_dim=AUDIO_DIM, n_classes=params.n_classes,
                                 compute=params.get("compute", "f32"), seed=params.seed).finalize(self.device)
        self._make_optim()
        self.use_ema = bool(params.get("ema", True))
        self.ema = self.model.flat.data.clone() if self.use_ema else None      # EMA(model): a deep copy of the parameters
        self.sched = PlateauLR(params.optim.lr)
        self.accuracy, self.global_steps = 0.0, 0
        self._swap = None
        self.eval_missing = bool(params.get("eval_missing", False))
        self.train_missing = bool(params.get("train_missing", False))      # (mmin_miss: refused)

    def train_step(self, batch):
        """TrainerBase's step with the EMA step behind the optimizer's (one rank: no gradient all-reduce).  A resident batch
        (``resident_batch``) is collated on the device first, from its store and descriptor"""
        self.model.train()
        if batch.get("desc") is not None:
            device_collate(batch)
        stats = self.model.loss_and_grads(batch)
        self.optim.step()
        if self.use_ema:
            capi.ema_step(self.ema, self.model.flat.data, self.model.flat.numel, EMA_ALPHA)
        self.global_steps += 1
        return stats

    class _EmaWeights:
        """the model computing with the EMA weights: the flat buffer's contents are exchanged on entry and exit (the kernels'
        operands stay where they are)"""

        def __init__(self, trainer):
            self.t = trainer

        def __enter__(self):
            flat, t = self.t.model.flat, self.t
            t._swap = flat.data.clone()
            flat.data.copy_(t.ema)

        def __exit__(self, *exc):
            self.t.model.flat.data.copy_(self.t._swap)
            self.t._swap = None
            return False

    def ema_weights(self):
        return self._EmaWeights(self)

    # ------------------------------------------------------------------------------------------------- capacity mode
    def make_bucket(self, B_cap, T_cap, Tv, Tt):
        """the static input buffers of bucket (B_cap, T_cap): what ``mmin_collate`` returns at capacity shape, and counts = {B, Ta}"""
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.device)
        return dict(audio_feature=f32(B_cap, T_cap, AUDIO_DIM), visual_feature=f32(B_cap, Tv, VISUAL_DIM), text_feature=f32(B_cap, Tt, TEXT_DIM),
                    label=torch.zeros(B_cap, dtype=torch.int64, device=self.device),
                    counts=torch.zeros(2, dtype=torch.int32, device=self.device))

    @staticmethod
    def fill_bucket(static, batch):
        """a host-collated batch (on the device already) into its bucket: rows and slots the batch does not have are zero"""
        B, Ta = (int(v) for v in batch["audio_feature"].shape[:2])
        static["audio_feature"].zero_()
        static["audio_feature"][:B, :Ta].copy_(batch["audio_feature"], non_blocking=True)
        for k in ("visual_feature", "text_feature", "label"):
            static[k][:B].copy_(batch[k], non_blocking=True)
            static[k][B:].zero_()
        static["counts"].copy_(torch.tensor([B, Ta], dtype=torch.int32), non_blocking=True)

    def capacity_bucket(self, batch):
        """trainer.StepGraphs: (key, make_static, fill) of the bucket of a prepared batch -- B_cap = train.batch_size, T_cap =
        the batch's audio length rounded up (datasets.mmin_t_cap) -- or None with the mode off or for a batch larger than
        train.batch_size"""
        B_cap = int(self.params.train.batch_size)
        if not self.capacity or "counts" in batch or int(batch["audio_feature"].shape[0]) > B_cap:
            return None
        T_cap = mmin_t_cap(int(batch["audio_feature"].shape[1]), self.t_cap)
        Tv, Tt = int(batch["visual_feature"].shape[1]), int(batch["text_feature"].shape[1])
        return ("capacity", B_cap, T_cap, Tv, Tt), lambda: self.make_bucket(B_cap, T_cap, Tv, Tt), self.fill_bucket

    def resident_batch(self, store, cur_desc, B_cap, T_cap):
        """the "batch" of a step whose samples stay in ``store`` (datasets.MMINDeviceStore): the bucket's buffers, which the
        step's first launch fills from the store through the 3 B_cap int32 of ``cur_desc`` (erc_mmin_collate)"""
        batch = self.make_bucket(B_cap, T_cap, int(store.visual.shape[1]), int(store.text.shape[1]))
        batch.update(store=store, desc=cur_desc)
        return batch

    def resident_eval_step(self, batch, cm, loss_sum):
        """one evaluation step from the store, scored on the device (``MMINBaseModule.eval_scores``); -> the step's workspace"""
        device_collate(batch)
        return self.model.eval_scores(batch, cm, loss_sum)

    def eval_epoch(self, loader):
        """one pass with the model and one with the EMA model over ``loader``; logits stay on the device, one copy per epoch.
        -> dict(Lall = sum over batches of the batch-mean CE (meter.sum), Acc, Acc2, C, true, pred).  ``--eval_missing``:
        ``eval_epoch_missing``"""
        if self.eval_missing:
            return self.eval_epoch_missing(loader)
        self.model.eval()
        batches = [self.prepare_batch(b) for b in loader]
        ys = torch.cat([b["label"] for b in batches])
        run = lambda: [self.to_logits(b).clone() for b in batches]
        logits = run()
        losses = torch.stack([torch.nn.functional.cross_entropy(lg, b["label"]) for lg, b in zip(logits, batches)]).sum()
        pred = torch.cat(logits).argmax(-1)
        out = dict(C=int(ys.shape[0]))
        if self.use_ema:
            with self.ema_weights():
                pred2 = torch.cat(run()).argmax(-1)
            host = torch.stack([pred, pred2, ys]).cpu()
            out["Acc2"] = float((host[1] == host[2]).sum()) / out["C"]
        else:
            host = torch.stack([pred, ys]).cpu()
        out.update(Lall=float(losses), Acc=float((host[0] == host[-1]).sum()) / out["C"], true=host[-1].tolist(), pred=host[0].tolist())
        return out

    def eval_epoch_missing(self, loader):
        """``eval_epoch`` under ``--eval_missing``: the same two passes (the same launches in the same order, so the
        full-modality figures are the ones without the flag) with the model's ``score_missing`` behind every batch's forward.
        The dict gains ``missing``: {"v" | "t" | "a" | "tv" | "av" | "at": dict(Lall, Acc, cm [C, C] true x predicted, and
        under EMA Acc2, cm2)} in MISSING_TYPES' order; the six matrices and sums of both passes reach the host in ONE copy"""
        self.model.eval()
        batches = [self.prepare_batch(b) for b in loader]
        ys = torch.cat([b["label"] for b in batches])
        t_max = max(int(b["audio_feature"].shape[1]) for b in batches)
        K, C, n_pass = len(MISSING_TYPES), int(self.model.n_classes), 2 if self.use_ema else 1
        cm = torch.zeros(n_pass, K, C, C, dtype=torch.int64, device=self.device)
        sums = torch.zeros(n_pass, K, dtype=torch.float64, device=self.device)

        def run(k):
            self.model.begin_missing_pass(t_max)
            out = []
            for b in batches:
                out.append(self.to_logits(b).clone())
                self.model.score_missing(b["label"], cm[k], sums[k])
            return out
        logits = run(0)
        losses = torch.stack([torch.nn.functional.cross_entropy(lg, b["label"]) for lg, b in zip(logits, batches)]).sum()
        pred = torch.cat(logits).argmax(-1)
        out = dict(C=int(ys.shape[0]))
        if self.use_ema:
            with self.ema_weights():
                pred2 = torch.cat(run(1)).argmax(-1)
            host = torch.stack([pred, pred2, ys]).cpu()
            out["Acc2"] = float((host[1] == host[2]).sum()) / out["C"]
        else:
            host = torch.stack([pred, ys]).cpu()
        self.model.begin_missing_pass()      # the next user of the zero-input features starts from the weights of that time
        out.update(Lall=float(losses), Acc=float((host[0] == host[-1]).sum()) / out["C"], true=host[-1].tolist(), pred=host[0].tolist())
        packed = torch.cat([cm.reshape(n_pass, -1).to(torch.float64), sums], 1).cpu()      # counts are exact in float64
        out["missing"] = missing_dict(packed, C, self.use_ema)
        return out

    def load_pretrained(self, path):
        """``--pretrain_path``: the whole trainer state of a ``mmin_base`` checkpoint"""
        return load(self, path)

    def extra_models(self):
        """further entries of the checkpoint's ``models`` (MMINMissTrainer: the pretrained model)"""
        return {}

    @staticmethod
    def make_loaders(params):
        """``--train_missing``: every training sample gets one of the six patterns at every read (``Missing``) and its batch is
        masked as MMINMissCollate masks it, without the ``_reverse`` inputs (nothing reads them here)"""
        if not params.get("train_missing", False):
            return make_loaders(params)
        from .mmin_miss import Missing
        return make_loaders(params, collate=lambda split: mask_collate if split == "train" else mmin_collate, transform=Missing())

    def on_eval_end(self, rec):
        """the plateau scheduler on the validation epoch's accumulated loss (mmin_base.py:171-177); -> True when the learning
        rate changed (a captured step holds it as a launch argument and must be dropped)"""
        lr = self.sched.step(rec["Lall"])
        changed = lr != self.optim.lr
        self.optim.lr = lr
        return changed

    def on_test_end(self, rec, save_dir=None):
        """best checkpoint by test Acc, last checkpoint always (mmin_base.py:198-201); -> True when this epoch is the best"""
        best = self.accuracy < rec["Acc"]
        if best:
            self.accuracy = rec["Acc"]
        if save_dir:
            os.makedirs(save_dir, exist_ok=True)
            for tag in (("best_model", ) if best else ()) + ("last_model", ):
                save(self, os.path.join(save_dir, tag + ".ckpt"))
                with open(os.path.join(save_dir, tag + ".json"), "w") as fh:
                    fh.write(json.dumps({"global_steps": self.global_steps, "accuracy": self.accuracy}))
        return best


CAPACITY_FLAGS = ("capacity_buckets", "device_collate", "resident", "resident_eval")


def device_collate(batch):
    """erc_mmin_collate of a resident batch: its descriptor's samples from the store into the bucket's buffers, one launch
    (a store whose descriptor carries keep bits, datasets.MMINMaskedDeviceStore: erc_mmin_collate_masked)"""
    st, a = batch["store"], batch["audio_feature"]
    B_cap, T_cap = int(a.shape[0]), int(a.shape[1])
    capi.mmin_collate(batch["desc"], st.audio, st.visual, st.text, st.label, B_cap, T_cap, min(T_cap, st.t_max), a, batch["visual_feature"],
                      batch["text_feature"], batch["label"], batch["counts"], masked=st.DESC_INTS == 4)


def state_dict(trainer):
    """the reference trainer's envelope with both registered models: {'models': {'model', 'ema_model'}, 'optims': {'optim'}}"""
    from . import checkpoint
    sd = checkpoint.state_dict(trainer)
    if trainer.use_ema:
        flat = trainer.model.flat
        sd["models"]["ema_model"] = {k: flat.view(trainer.ema, k).detach().cpu().clone() for k in trainer.model.state_dict()}
    sd["models"].update(trainer.extra_models())
    return sd


def save(trainer, path):
    torch.save(state_dict(trainer), path)
    return path


def load(trainer, path, with_optimizer=True):
    """``--pretrain_path``: a checkpoint written by ``save`` or by the reference's trainer; the EMA weights follow the file's
    ``ema_model`` (the loaded model's where the file has none)"""
    from . import checkpoint
    ckpt = checkpoint.load(trainer, path, with_optimizer=with_optimizer)
    if trainer.use_ema:
        flat = trainer.model.flat
        trainer.ema.copy_(flat.data)
        ema = ckpt.get("models", {}).get("ema_model") if isinstance(ckpt, dict) else None
        for k, v in (ema or {}).items():
            flat.view(trainer.ema, k).copy_(v.to(flat.device, torch.float32))
    trainer.sched.lr = trainer.optim.lr
    return ckpt


def mmin_collate(samples):
    """MMINBaseCollate (mmin_base.py:224-251): audio zero-padded to the batch's longest utterance, batch-first"""
    from torch.nn.utils.rnn import pad_sequence
    audio = [torch.as_tensor(s["audio_feature"], dtype=torch.float32) for s in samples]
    return dict(audio_feature=pad_sequence(audio, batch_first=True, padding_value=0.0),
                audio_feature_length=[int(a.shape[0]) for a in audio],
                visual_feature=torch.as_tensor(np.stack([s["visual_feature"] for s in samples]), dtype=torch.float32),
                text_feature=torch.as_tensor(np.stack([s["text_feature"] for s in samples]), dtype=torch.float32),
                label=torch.tensor([int(s["label"]) for s in samples], dtype=torch.long), name=[s["name"] for s in samples])


def mask_collate(samples):
    """mmin_collate of samples that carry ``missing_type`` (the ``Missing`` transform), every modality x multiplied by its 0 / 1
    entry as MMINMissCollate(has_miss=True) does (track_mm/mmin_miss.py:328-337); no ``_reverse`` inputs"""
    data = mmin_collate(samples)
    missing_type = torch.tensor([s["missing_type"] for s in samples], dtype=torch.long)
    for i, key in enumerate(MODAL_KEYS):
        data[key] = data[key] * missing_type[:, i][:, None, None]
    data["missing_type"] = missing_type
    return data


def missing_dict(packed, C, use_ema):
    """``eval_epoch``'s ``missing`` entry from the host copy ``packed`` [passes, 6 C C + 6] (per pass: the six confusion matrices,
    exact in float64, then the six loss sums), in MISSING_TYPES' order"""
    K = len(MISSING_TYPES)
    cms = packed[:, :K * C * C].round().to(torch.int64).reshape(-1, K, C, C).numpy()
    out = {}
    for i, key in enumerate(MISSING_KEYS):
        n = max(1, int(cms[0, i].sum()))
        rec = dict(Lall=float(packed[0, K * C * C + i]), Acc=float(cms[0, i].trace()) / n, cm=cms[0, i])
        if use_ema:
            rec.update(Acc2=float(cms[1, i].trace()) / n, cm2=cms[1, i])
        out[key] = rec
    return out


class _Transformed(torch.utils.data.Dataset):
    """samples with an output transform, applied at every read (one draw per sample per epoch)"""

    def __init__(self, data, fn):
        self.data, self.fn = data, fn

    def __len__(self):
        return len(self.data)

    def __getitem__(self, i):
        return self.fn(dict(self.data[i]))


def make_loaders(params, collate=None, transform=None, name="mmin_base"):
    """the synthetic train / val / test loaders; ``collate``: stage -> collate function (default: mmin_collate everywhere),
    ``transform``: applied to every TRAINING sample each time it is read (MMINMissDM's output transform)"""
    from torch.utils.data import DataLoader
    from .synthetic import make_mmin_samples
    if not params.get("synthetic", True):
        raise SystemExit("dataset %s: the .h5 feature readers of the reference need h5py, which this build cannot test against; "
                         "only --synthetic=True is built for --module=%s" % (params.dataset, name))
    lo, hi = params.get("mmin_frames", (50, 400))
    out = []
    for split, n, grp in (("train", params.n_train, params.train), ("val", params.get("n_val", params.n_test), params.val),
                          ("test", params.n_test, params.test)):
        data = make_mmin_samples(n, split, seed=params.seed, frames=(int(lo), int(hi)), n_classes=params.n_classes)
        if transform is not None and split == "train":
            data = _Transformed(data, transform)
        gen = torch.Generator().manual_seed(params.seed)
        out.append(DataLoader(data, batch_size=grp.batch_size, shuffle=(split == "train"),
                              collate_fn=mmin_collate if collate is None else collate(split), generator=gen))
    return out


class MMINResidentEpochs(ResidentLoop):
    """``--device_collate --resident`` of --module=mmin_base: the training split stays in a datasets.MMINDeviceStore.  Per epoch
    the host draws the batches' sample indices exactly as the default loop's DataLoader does (datasets.index_batches: the same
    sampler on the same generator, a short last batch) and uploads ONE int32 table [steps, 3 B]; a step copies its 3 B int32
    into the fixed descriptor and replays the graph of its bucket -- collate, forward, backward, Adam, EMA.  ResidentLoop's
    visit / capture / counters, keyed by the batch's T capacity (datasets.mmin_t_cap) instead of a node capacity."""

    def __init__(self, trainer, store, batch_size, generator, capture=True):
        super().__init__(trainer, store, batch_size, capture)
        self.gen = generator
        self.acc = torch.zeros(4, dtype=torch.float64, device=store.device)      # sums of the steps' {loss, #correct, -, -}

    def _batch(self, cap):
        return self.trainer.resident_batch(self.store, self.cur_desc, self.B, cap)

    def _step(self, batch):
        self.acc.add_(self.trainer.train_step(batch)[:4])
        return self.trainer.model._last_ws

    def tables(self):
        """(host int32 table [steps, 3 B], T capacity per step, utterances per step) of the NEXT epoch: draws from the generator.
        ``--train_missing`` (the store's descriptor has keep bits: [steps, 4 B]): one ``random.choice`` over MISSING_TYPES per
        batch in order and sample in batch order, the stream the default loop's ``Missing`` transform consumes"""
        batches = index_batches(len(self.store), self.B, True, self.gen)
        if self.store.DESC_INTS == 4:
            types = [list(t) for t in MISSING_TYPES]
            keep = [[sum(bit << i for i, bit in enumerate(random.choice(types))) for _ in b] for b in batches]
            table, caps = self.store.table(batches, self.B, keep)
        else:
            table, caps = self.store.table(batches, self.B)
        return table, caps, [len(b) for b in batches]

    def epoch(self):
        """one pass over the store; returns the steps' utterance counts"""
        table, caps, counts = self.tables()
        with dynamic_n(self.trainer.model):
            self._steps(torch.from_numpy(table).to(self.store.device), caps)
        return counts


class MMINResidentEval(ResidentLoop):
    """``--resident_eval``: a validation or test split in a datasets.MMINDeviceStore, visited in its fixed order (the table is
    uploaded once, here).  One graph per T capacity: collate, the forward in eval mode, erc_cross_entropy_cap into a float64
    accumulator (Lall = the sum of the batch means, the plateau scheduler's metric) and erc_rows_score into a confusion matrix.
    ``epoch`` runs the pass with the model's weights and, under EMA, again with the EMA weights swapped in, and copies ONE
    tensor to the host: both matrices and both sums."""

    def __init__(self, trainer, store, batch_size, capture=True):
        super().__init__(trainer, store, batch_size, capture)
        table, self.caps = store.table(index_batches(len(store), self.B, False), self.B)
        self.table_dev = torch.from_numpy(table).to(store.device)
        C = self.C = int(trainer.params.n_classes)
        self.cm = torch.zeros(C, C, dtype=torch.int64, device=store.device)
        self.loss_sum = torch.zeros(1, dtype=torch.float64, device=store.device)
        # --eval_missing: the zero-input table of the pass's weights in FIXED buffers (the captured steps read them; a pass
        # refills them, as ema_weights swaps the parameters) and the six matrices and sums, which travel with ``out``
        self.missing = None
        if getattr(trainer, "eval_missing", False):
            K, f64 = len(MISSING_TYPES), torch.float64
            self.missing = dict(zaudio=torch.zeros(self.T + 1, HID, dtype=torch.float32, device=store.device),
                                zvt=torch.zeros(2 * HID, dtype=torch.float32, device=store.device),
                                cm=torch.zeros(K, C, C, dtype=torch.int64, device=store.device),
                                sums=torch.zeros(K, dtype=f64, device=store.device))
        n_miss = 0 if self.missing is None else len(MISSING_TYPES) * (C * C + 1)
        # per pass: the matrix (exact in float64) | Lall, then under --eval_missing the six matrices | the six sums
        self.out = torch.zeros(2, C * C + 1 + n_miss, dtype=torch.float64, device=store.device)

    def _batch(self, cap):
        batch = self.trainer.resident_batch(self.store, self.cur_desc, self.B, cap)
        if self.missing is not None:
            batch["missing"] = self.missing
        return batch

    def _step(self, batch):
        return self.trainer.resident_eval_step(batch, self.cm, self.loss_sum)

    def _pass(self, k):
        self.cm.zero_()
        self.loss_sum.zero_()
        ms, n = self.missing, self.C * self.C
        if ms is not None:      # outside the captured steps: built from the weights in place now
            ms["cm"].zero_()
            ms["sums"].zero_()
            self.trainer.model.zero_table(self.T, int(self.store.visual.shape[1]), int(self.store.text.shape[1]), self.store.device, out=ms)
        with dynamic_n(self.trainer.model):
            self._steps(self.table_dev, self.caps)
        self.out[k, :n].copy_(self.cm.reshape(-1))
        self.out[k, n:n + 1].copy_(self.loss_sum)
        if ms is not None:
            self.out[k, n + 1:n + 1 + ms["cm"].numel()].copy_(ms["cm"].reshape(-1))
            self.out[k, n + 1 + ms["cm"].numel():].copy_(ms["sums"])

    def epoch(self):
        """``eval_epoch``'s dict without the per-sample lists: Lall, Acc, C, cm (host int64 [C, C], true x predicted) and, under
        EMA, Acc2 and cm2"""
        tr, C = self.trainer, self.C
        self._pass(0)
        if tr.use_ema:
            with tr.ema_weights():
                self._pass(1)
        host = self.out.cpu()
        cms = host[:, :C * C].round().to(torch.int64).reshape(2, C, C)
        n = int(cms[0].sum())
        out = dict(C=n, Lall=float(host[0, C * C]), Acc=float(cms[0].diagonal().sum()) / max(1, n), cm=cms[0].numpy())
        if tr.use_ema:
            out.update(Acc2=float(cms[1].diagonal().sum()) / max(1, n), cm2=cms[1].numpy())
        if self.missing is not None:
            out["missing"] = missing_dict(host[:2 if tr.use_ema else 1, C * C + 1:], C, tr.use_ema)
        return out


class _CounterSum:
    """the epoch line's counters of a capacity run: ``replays`` / ``eager`` / ``captures`` summed over its training, validation
    and test loops"""

    def __init__(self, parts):
        self.parts = parts

    replays = property(lambda self: sum(c.replays for c in self.parts))
    eager = property(lambda self: sum(c.eager for c in self.parts))
    captures = property(lambda self: sum(c.captures for c in self.parts))


class MMINEpochLoop:
    """trainer.EpochLoop's surface for --module=mmin_base and --module=mmin_miss (one rank), whose epoch has three loaders, a
    second pass under the EMA weights and the plateau scheduler between the validation and the test epoch.  The constructor
    does what lies between "trainer constructed" and "first epoch": the loaders, ``trainer.t_cap``, what the capacity flags
    select -- ``graphs`` (--capacity_buckets: trainer.StepGraphs over host-collated batches) or ``resident`` (--device_collate
    --resident), ``res_val`` / ``res_eval`` (--resident_eval: the validation and the test split) -- and the stats ring; a
    combination that is not built exits here.  ``fixed`` is always None.  ``counters``: None for the default loop.  Like
    EpochLoop's, ``train_epoch`` and ``test_epoch`` do not synchronise, take no clock and print nothing."""

    def __init__(self, params, trainer, device, rank=0, world=1):
        self.params, self.trainer = params, trainer
        self.train_loader, self.val_loader, self.test_loader = trainer.make_loaders(params)
        self.graphs = self.fixed = self.resident = self.res_val = self.res_eval = self.counters = None
        flags = {k: bool(params.get(k, False)) for k in CAPACITY_FLAGS}
        if trainer.CAPACITY_MODES and any(flags.values()):
            if flags["resident"] != flags["device_collate"]:
                raise SystemExit("--module=%s: --resident runs from the device store of --device_collate; give both or neither" % trainer.NAME)
            if flags["resident_eval"] and not flags["resident"]:
                raise SystemExit("--module=%s: --resident_eval needs --device_collate --resident" % trainer.NAME)
            capture = params.get("graph_capture", True)
            store = lambda loader: MMINDeviceStore(loader.dataset, device)
            train_data = self.train_loader.dataset
            if trainer.train_missing:      # (the loader's dataset draws a pattern at every read: the samples are underneath)
                train_data = train_data.data
            trainer.t_cap = max(int(s["audio_feature"].shape[0]) for s in train_data)
            if flags["resident"]:
                train_store = (MMINMaskedDeviceStore if trainer.train_missing else MMINDeviceStore)(train_data, device)
                self.resident = MMINResidentEpochs(trainer, train_store, params.train.batch_size,
                                                   self.train_loader.generator, capture=capture)
            else:
                self.graphs = StepGraphs(trainer, maxsize=64, capture=capture)
            if flags["resident_eval"]:
                self.res_val = MMINResidentEval(trainer, store(self.val_loader), params.val.batch_size, capture=capture)
                self.res_eval = MMINResidentEval(trainer, store(self.test_loader), params.test.batch_size, capture=capture)
            self.counters = _CounterSum([c for c in (self.resident or self.graphs, self.res_val, self.res_eval) if c is not None])
        self.n_steps = len(self.train_loader)
        self.ring = torch.zeros(max(1, self.n_steps), 4, dtype=torch.float32, device=device)

    def train_epoch(self):
        """(#utterances, the steps' utterance counts); a resident step leaves no row in the ring"""
        if self.resident is not None:
            counts = self.resident.epoch()
        else:
            counts = train_epoch_loader(self.train_loader, self.graphs, self.trainer, self.ring)
        return sum(counts), counts

    def test_epoch(self, multiemo=False):
        """the validation epoch, the plateau scheduler on its loss (captured training steps are dropped when the learning rate
        changes) and the test epoch -> (val, test), ``eval_epoch``'s dicts"""
        tr = self.trainer
        val = self.res_val.epoch() if self.res_val is not None else tr.eval_epoch(self.val_loader)
        if tr.on_eval_end(val) and self.counters is not None:
            (self.resident or self.graphs).drop_graphs()
        test = self.res_eval.epoch() if self.res_eval is not None else tr.eval_epoch(self.test_loader)
        return val, test


MMINBaseTrainer.EPOCH_LOOP = MMINEpochLoop      # (trainer.epoch_loop_class; MMINMissTrainer inherits it)


def missing_records(missing, with_report):
    """the epoch line's entries of ``eval_epoch``'s ``missing`` dict (MMINMissTrainer, --eval_missing), in its order: Lall, Acc,
    Acc2 under EMA, C = the utterances counted, and with ``with_report`` report_from_cm's block (the matrix included)"""
    out = {}
    for key, rec in missing.items():
        out[key] = {k: rec[k] for k in ("Lall", "Acc", "Acc2") if k in rec}
        out[key]["C"] = int(rec["cm"].sum())
        if with_report:
            out[key]["report"] = report_from_cm(rec["cm"])
    return out


def epoch_line(params, epoch, utt_per_s, lr, val, test, best_acc, is_best):
    """the epoch's JSON record from ``eval_epoch``'s dicts of the validation and the test split"""
    if not params.get("confuse_matrix", True):
        rep = {}
    elif "cm" in test:
        rep = report_from_cm(test["cm"])
    else:
        rep = classification_report(test["true"], test["pred"], params.n_classes)
    last = {"epoch": epoch, "train_utt_per_s": utt_per_s, "lr": lr,
            "val": {k: val[k] for k in ("Lall", "Acc", "Acc2") if k in val}, "test": {k: test[k] for k in ("Lall", "Acc", "Acc2") if k in test},
            "report": {k: rep[k] for k in rep if k != "cm"}, "class_names": list(params.class_names), "best_acc": best_acc,
            "is_best": is_best}
    if "missing" in test:      # --eval_missing (mmin_base, mmin_miss): both splits under the six missing-modality patterns
        last["missing"] = {split: missing_records(rec["missing"], params.get("confuse_matrix", True))
                           for split, rec in (("val", val), ("test", test))}
    return last


def run(trainer_cls, params_cls, argv=None):
    """--module=mmin_base and --module=mmin_miss: training steps (EMA after each), the validation epoch (plateau scheduler), the
    test epoch (Acc, Acc2, report, best / last checkpoints); one JSON line per epoch"""
    params = params_cls()
    params.from_args(argv)
    device = setup_device(params)
    fix_seed(params.seed)
    trainer = trainer_cls(params, device)
    if params.get("pretrain_path"):
        trainer.load_pretrained(params.pretrain_path)
    loop = epoch_loop_class(trainer_cls)(params, trainer, device)
    last = {}
    for epoch in range(params.epoch):
        t0 = time.perf_counter()
        n_utt, counts = loop.train_epoch()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        trainer.model.flat.check_health(trainer.NAME)
        if params.log_every and loop.resident is None:
            print_step_lines(params, epoch, loop.ring, counts)
        val, test = loop.test_epoch()
        best = trainer.on_test_end(test, params.get("save_dir"))
        last = epoch_line(params, epoch, n_utt / dt, trainer.optim.lr, val, test, trainer.accuracy, best)
        c = loop.counters
        if c is not None:
            last.update(graph_replays=c.replays, eager_steps=c.eager, graphs_captured=c.captures)
        print(json.dumps(last), flush=True)
    if params.get("save"):
        save(trainer, params.save)
    return last
