"""MMIN's missing-modality model on the MI355X hot path (drop-in for MMINMissModule and MMINMissTrainer,
track_mm/mmin_miss.py:68-296; ResidualAE, track_mm/mmin_models.py:133-199): the three encoders of the full-modality base model
(erc_amd/mmin.py) over inputs whose missing modalities are zeroed, two residual autoencoders over their 384 features -- ``netAE``
imagines the full-modality features and hands its 5 x 64 latents to the classifier, ``netAE_cycle`` maps the features back -- and
the base model's classifier on the 320 latents.  Training pulls ``netAE``'s reconstruction towards the features a PRETRAINED base
model extracts from the missing part of the utterance:

    Lall = Lce + 4 mse(pretrained.encode(x_reverse), fusion) + 2 mse(features, fusion_cycle)            (mmin_miss.py:206-210)

``MMINMissModule`` keeps the reference's constructor signature and ``state_dict`` key for key and shape for shape (150 tensors,
5 444 228 parameters at 342 / 1024 / 130 / 4) and ``forward(**batch) -> (logits, fusion, fusion_cycle, features)``.  ``mmin_miss2``
is not built.

Launches of a training step:
  forward   the base model's encoders on the masked batch -> features | erc_resae_fwd (both autoencoders, ONE launch) -> fusion,
            fusion_cycle, latents written straight into the classifier's input | the three classifier GEMMs
            | the pretrained model's encoders on the reverse batch (forward only: nothing reads the gradient autograd sends there)
  backward  erc_cross_entropy | the classifier's 3 GEMMs down to d_latents | erc_mse_grad x 2 | erc_resae_bwd (ONE launch): dx
            of both networks and every layer's dY | erc_mmin_miss_combine: dfeatures = dx(netAE) + dx(netAE_cycle) - d(Lcycle),
            the text columns through embd's ReLU, the loss slots | the base model's encoder backward
            | erc_wgrad_table: all 72 Linear / LSTM weight gradients and bias sums, one call (it groups equal-sized records into runs)
  update    erc_adam_step | erc_ema_step (``model`` only)

Reference behaviours kept on purpose (DESIGN.md section 8k lists them with line numbers): ``netAE_cycle`` reads ``features``, not
``fusion``; ``--finetune`` changes nothing (the optimizer is rebuilt over the model alone); ``efficiency_init`` runs on BOTH models
after the checkpoint was loaded, so the pretrained text CNN's convolutions are re-drawn and every Conv / Linear bias is zero
(``--pretrain_reinit=False`` keeps the loaded weights); the pretrained model is in training mode during training steps (its text
dropout is live, drawing from its own counter); missing modalities are zeroed inputs that still run through their encoders;
validation and test batches are full-modality.

``--eval_missing`` (default off; the reference has no counterpart) also scores the validation and test epochs
under the six patterns of ``MISSING_TYPES`` (mmin_miss.py:345-360), masked as MMINMissCollate masks a training batch
(mmin_miss.py:328-337), WITHOUT six more passes: a masked modality's 128 feature columns are those of an all-zero sample, so behind
every batch's unchanged forward ``score_missing`` launches erc_mmin_miss_expand (the batch's features against the zero-input row,
6 B rows) | erc_resae_latents (netAE's latents alone) | the three classifier GEMMs | erc_mmin_miss_score (six confusion matrices
and loss sums, kept on the device until the epoch's one copy).
"""
import math
import random

import torch
from torch import nn

from . import capi, mmin
from .engine import WorkspaceCache, _world_size, linear_wgrad
from .mmin import EMB, HID, MISSING_KEYS, MISSING_PATTERNS, MISSING_TYPES, MODAL_KEYS, MMINBaseModule, MMINBaseTrainer  # noqa: F401

AE_LAYERS, N_BLOCKS = (256, 128, 64), 5                  # mmin_miss.py:77-78
LAT = AE_LAYERS[-1] * N_BLOCKS                           # 320: the classifier's input (:82)
W_MSE, W_CYCLE = 4.0, 2.0                                # :210
PRETRAINED_SEED_SALT = 0x5EED                            # the pretrained model's dropout counter stream is its own
# MISSING_TYPES (:348-353), MODAL_KEYS (:354, :332), MISSING_KEYS and MISSING_PATTERNS: erc_amd/mmin.py (the base model's
# --eval_missing and --train_missing use them too)


class _ResidualAE(nn.Module):
    """parameter holder with the reference's attribute names (ResidualAE, mmin_models.py:140-185); the math is csrc/resae.hip"""

    def __init__(self, layers, n_blocks, input_dim, dropout=0.0, use_bn=False):
        super().__init__()
        if tuple(layers) != AE_LAYERS or input_dim != EMB or use_bn or dropout or not 1 <= n_blocks <= capi.RESAE_LAYERS // 6:
            raise capi.ErcGraftError("ResidualAE(layers=%r, n_blocks=%r, input_dim=%r, dropout=%r, use_bn=%r): erc_resae_fwd is built for "
                                     "layers [256, 128, 64], input_dim 384, 1..5 blocks, no dropout, no BatchNorm (the settings of "
                                     "MMINMissModule)" % (list(layers), n_blocks, input_dim, dropout, use_bn))
        self.n_blocks, self.input_dim = n_blocks, input_dim
        self.transition = nn.Sequential(nn.Linear(input_dim, input_dim), nn.ReLU(), nn.Linear(input_dim, input_dim))
        for i in range(n_blocks):
            dims = [input_dim] + list(layers)
            enc = []
            for a, b in zip(dims[:-1], dims[1:]):
                enc += [nn.Linear(a, b), nn.LeakyReLU()]
            setattr(self, "encoder_%d" % i, nn.Sequential(*enc[:-1]))
            dec = []
            for a, b in zip(dims[:0:-1], dims[-2::-1]):
                dec += [nn.Linear(a, b), nn.ReLU()]
            setattr(self, "decoder_%d" % i, nn.Sequential(*dec[:-1]))


class MMINMissModule(MMINBaseModule):
    NAME = "mmin_miss"

    def _build_head(self):
        self.netAE = _ResidualAE(AE_LAYERS, N_BLOCKS, EMB)
        self.netAE_cycle = _ResidualAE(AE_LAYERS, N_BLOCKS, EMB)
        self.netC = mmin._Classifier(LAT, self.n_classes)

    def _make_workspace(self, B, Ta, Tv, Tt, device):
        ws = super()._make_workspace(B, Ta, Tv, Tt, device)
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
        n_act = capi.resae_act_floats(B, N_BLOCKS)
        ws.update(fusion=f32(B, EMB), fusion_cycle=f32(B, EMB), latents=f32(B, LAT), latents_cycle=f32(B, LAT), dlat=f32(B, LAT),
                  d_fusion=f32(B, EMB), d_cycle=f32(B, EMB), dx=[f32(B, EMB), f32(B, EMB)], ae_act=[f32(n_act), f32(n_act)],
                  ae_dY=[f32(n_act), f32(n_act)], ce_stats=f32(256))
        names = capi.resae_layer_names(N_BLOCKS)
        jobs = []
        for j, net in enumerate(("netAE", "netAE_cycle")):
            jobs.append(dict(W=[self._w("%s.%s.weight" % (net, n)) for n in names], b=[self._w("%s.%s.bias" % (net, n)) for n in names],
                             x=ws["fused"], recon=ws["fusion_cycle" if j else "fusion"], latents=ws["latents_cycle" if j else "latents"],
                             act=ws["ae_act"][j], d_recon=ws["d_cycle" if j else "d_fusion"], d_latents=None if j else ws["dlat"],
                             dx=ws["dx"][j], dY=ws["ae_dY"][j], B=B, ldx=EMB, ldr=EMB, ldl=LAT, lddr=EMB, lddl=LAT, lddx=EMB))
        ws["ae_jobs"] = capi.resae_jobs(jobs)
        return ws

    # ----------------------------------------------------------------------------------------------------------- forward
    def _forward_impl(self, audio, visual, text, training):
        ws, B = self._encode(audio, visual, text, training, need_all=True)
        capi.resae_fwd(ws["ae_jobs"], N_BLOCKS, 2)
        self._classifier_fwd(ws, B, ws["latents"], LAT, training)
        return ws, B

    def forward(self, audio_feature=None, visual_feature=None, text_feature=None, *args, **kwargs):
        """-> (logits [B, C], fusion [B, 384], fusion_cycle [B, 384], features [B, 384]) (mmin_miss.py:84-107)"""
        ws, _ = self._forward_impl(audio_feature, visual_feature, text_feature, self.training)
        return ws["logits"], ws["fusion"], ws["fusion_cycle"], ws["fused"]

    # ---------------------------------------------------------------------------------------------------------- backward
    def loss_and_grads(self, batch, reverse_features):
        """Lall of the masked ``batch`` against ``reverse_features`` [B, 384] (the pretrained model's features of the reverse
        inputs, a constant) and every gradient into flat.grad.  -> the device stats: [0] Lall, [1] #correct, [2] Lmse, [3] Lcycle,
        [4] Lce"""
        ws, B = self._forward_impl(batch.get("audio_feature"), batch.get("visual_feature"), batch.get("text_feature"), self.training)
        if tuple(reverse_features.shape) != (B, EMB) or reverse_features.stride(1) != 1:
            raise capi.ErcGraftError("mmin_miss: reverse_features must be [%d, %d] with unit column stride, got %s"
                                     % (B, EMB, tuple(reverse_features.shape)))
        pl, stats = ws["planner"], ws["stats"]
        self._classifier_bwd(ws, B, ws["latents"], LAT, batch["label"], ws["ce_stats"])
        capi.gemm_f32(ws["dz0"], HID, 0, None, self._w("netC.module.0.weight"), LAT, 1, None, ws["dlat"], LAT, B, LAT, HID)
        # d(4 Lmse) / d fusion and d(2 Lcycle) / d fusion_cycle; the latter's negative is Lcycle's direct gradient wrt features
        capi.mse_grad(ws["fusion"], EMB, reverse_features, int(reverse_features.stride(0)), B, EMB, W_MSE, ws["d_fusion"], EMB, stats[2:])
        capi.mse_grad(ws["fusion_cycle"], EMB, ws["fused"], EMB, B, EMB, W_CYCLE, ws["d_cycle"], EMB, stats[3:])
        capi.resae_bwd(ws["ae_jobs"], N_BLOCKS, 2)
        dims, names = capi.resae_layer_dims(N_BLOCKS), capi.resae_layer_names(N_BLOCKS)
        for j, net in enumerate(("netAE", "netAE_cycle")):
            for (n_out, n_in), name, x_off, y_off in zip(dims, names, self._act_offsets(B), self._dy_offsets(B)):
                linear_wgrad(pl, ws["ae_dY"][j][y_off:], n_out, ws["ae_act"][j][x_off:], n_in, None, n_out, n_in, B,
                             self._off("%s.%s.weight" % (net, name)), self._off("%s.%s.bias" % (net, name)), defer=True)
        capi.mmin_miss_combine(ws["dx"][0], ws["dx"][1], ws["d_cycle"], ws["fused"], EMB, B, ws["dfused"], EMB, ws["dtext"], HID,
                               ws["ce_stats"], W_MSE, W_CYCLE, stats)
        self._encoders_bwd(ws, B)
        pl.reduce_into(ws, self.flat.grad)
        return stats

    # --------------------------------------------------------------------------------- evaluation under missing modalities
    def begin_missing_pass(self, t_max=None):
        """forget the zero-input features: they are constants of the weights, so a pass over other weights (the EMA copy swapped
        in, a training step in between) starts with this (``t_max``: the base model's table; here every audio length has its
        own scan)"""
        self._zero_feat, self._zero_vt = {}, {}

    def zero_features(self, Ta, Tv, Tt, device):
        """[384]: what the encoders make of a sample whose three inputs are zero (MMINMissCollate's masking: a missing modality is
        a zero input that still runs through its encoder), audio padded to ``Ta`` frames.  The visual and text columns are computed
        once per pass, the audio columns once per pass and distinct ``Ta`` (``zero_scans`` counts those scans)"""
        if not hasattr(self, "_zero_feat"):
            self.begin_missing_pass()
        z = self._zero_feat.get((Ta, Tv, Tt))
        if z is None:
            zeros = lambda T, d: torch.zeros(1, T, d, dtype=torch.float32, device=device)
            if (Tv, Tt) not in self._zero_vt:
                self._zero_vt[Tv, Tt] = self._zero_encode(None, zeros(Tv, self.visual_dim), zeros(Tt, self.text_dim))[HID:].clone()
            z = torch.cat([self._zero_encode(zeros(Ta, self.audio_dim), None, None)[:HID], self._zero_vt[Tv, Tt]])
            self._zero_feat[Ta, Tv, Tt] = z
            self.zero_scans += 1
        return z

    zero_scans = 0      # audio zero-input scans so far (tests count them per pass)

    def _missing_workspace(self, B, device):
        if not hasattr(self, "_miss_ws"):
            self._miss_ws = WorkspaceCache(maxsize=4)

        def make():
            K, C = len(MISSING_TYPES), self.n_classes
            f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
            m = dict(x=f32(K * B, EMB), latents=f32(K * B, LAT), z0=f32(K * B, HID), feat=f32(K * B, HID), logits=f32(K * B, C))
            names = capi.resae_layer_names(N_BLOCKS)
            m["job"] = capi.resae_jobs([dict(W=[self._w("netAE.%s.weight" % n) for n in names], b=[self._w("netAE.%s.bias" % n) for n in names],
                                             x=m["x"], latents=m["latents"], B=K * B, ldx=EMB, ldl=LAT)])
            return m
        return self._miss_ws.get(B, make)

    def score_missing(self, labels, cm, loss_sum):
        """the batch of the forward just run (eval mode), scored under the six patterns of MISSING_TYPES without a second pass
        over its inputs: its features (``fused`` of that forward) expanded against the zero-input features (1 launch), netAE's
        latents of the 6 B rows (erc_resae_latents, 1 launch), the classifier (3 GEMMs) and erc_mmin_miss_score, which adds the
        confusion matrices to ``cm`` (int64 [6, C, C]) and the batch-mean cross entropies to ``loss_sum`` (float64 [6]).
        Nothing is copied to the host; no random draw, no state changes.  -> the logits [6 B, C] (a workspace buffer)"""
        ws = self._last_ws
        if ws is None or self.training:
            raise capi.ErcGraftError("mmin_miss: score_missing follows a forward in eval mode")
        B, C, K, dev = int(ws["fused"].shape[0]), self.n_classes, len(MISSING_TYPES), ws["fused"].device
        if tuple(labels.shape) != (B, ) or labels.dtype != torch.int64:
            raise capi.ErcGraftError("mmin_miss: score_missing: labels must be int64 [%d], got %s %s" % (B, labels.dtype, tuple(labels.shape)))
        z = self.zero_features(ws["A"]["T"], ws["V"]["T"], ws["L"]["T"], dev)
        m = self._missing_workspace(B, dev)
        capi.mmin_miss_expand(ws["fused"], EMB, z, MISSING_PATTERNS, B, m["x"], EMB)
        capi.resae_latents(m["job"], N_BLOCKS)
        for name, x, k, out, n, act in (("netC.module.0", m["latents"], LAT, m["z0"], HID, 1), ("netC.module.3", m["z0"], HID, m["feat"], HID, 1),
                                        ("netC.fc_out", m["feat"], HID, m["logits"], C, 0)):
            capi.gemm_f32(x, k, 0, None, self._w(name + ".weight"), k, 0, None, out, n, K * B, n, k, bias=self._w(name + ".bias"), act=act)
        capi.mmin_miss_score(m["logits"], C, labels, B, K, C, cm, loss_sum)
        return m["logits"]

    @staticmethod
    def _act_offsets(B, n_blocks=N_BLOCKS):
        """float offset of every layer's INPUT rows in erc_resae_fwd's ``act`` buffer (ercgraft.h), in the chain's order"""
        out = []
        for i in range(n_blocks):
            out += [B * (1216 * i + o) for o in (0, 384, 640, 768, 832, 960)]
        return out + [B * 1216 * n_blocks, B * (1216 * n_blocks + 384)]

    @staticmethod
    def _dy_offsets(B, n_blocks=N_BLOCKS):
        """float offset of every layer's pre-activation gradient in erc_resae_bwd's ``dY`` buffer, in the chain's order"""
        out = []
        for i in range(n_blocks):
            out += [B * (1216 * i + o) for o in (0, 256, 384, 448, 576, 832)]
        return out + [B * 1216 * n_blocks, B * (1216 * n_blocks + 384)]


def efficiency_init(module):
    """models/init.py:23-51 as ``module.apply`` runs it: every Conv weight is drawn twice (normal(0, sqrt(2 / (kh kw out))), then
    kaiming_normal_ fan_in with the leaky_relu gain at slope 0, which is what stays), Conv and Linear biases are zeroed; LSTMs are
    untouched.  The draws come from torch's global CPU generator, in module order, and are copied into the parameters."""
    with torch.no_grad():
        for m in module.modules():
            if "Conv" in type(m).__name__:
                w = torch.empty(m.weight.shape)
                w.normal_(0, math.sqrt(2.0 / (m.kernel_size[0] * m.kernel_size[1] * m.out_channels)))
                nn.init.kaiming_normal_(w, a=0, mode="fan_in", nonlinearity="leaky_relu")
                m.weight.copy_(w)
                if m.bias is not None:
                    m.bias.zero_()
            elif isinstance(m, nn.Linear):
                m.bias.zero_()


# ---------------------------------------------------------------------------------------------------------------- training
class MMINMissTrainer(MMINBaseTrainer):
    """``--module=mmin_miss`` (mmin_miss.py:110-296).  Evaluation (with ``--eval_missing``: ``eval_epoch_missing``), the plateau
    scheduler, best / last checkpoints and the epoch loop are MMINBaseTrainer's."""
    NAME = "mmin_miss"
    MODULE = MMINMissModule
    CAPACITY_MODES = False

    def __init__(self, params, device):
        for key, what in (("capacity_buckets", "capacity buckets"), ("resident", "--resident"), ("resident_eval", "--resident_eval")):
            if params.get(key):
                raise capi.ErcGraftError("--module=mmin_miss: %s is not built (as for --module=mmin_base)" % what)
        if params.get("train_missing"):
            raise capi.ErcGraftError("--module=mmin_miss: --train_missing is the augmented baseline of --module=mmin_base; this model's "
                                     "training is always masked")
        if _world_size() > 1:
            raise capi.ErcGraftError("--module=mmin_miss: data-parallel runs are not built (as for --module=mmin_base)")
        super().__init__(params, device)
        # the pretrained full-modality model: its own flat buffer, forward only; no optimizer ever sees it (mmin_miss.py:149-154:
        # the optimizer built under --finetune is replaced by one over model.parameters() alone, so --finetune has no effect)
        self.pretrained_model = MMINBaseModule(visual_dim=mmin.VISUAL_DIM, text_dim=mmin.TEXT_DIM, audio_dim=mmin.AUDIO_DIM,
                                               n_classes=params.n_classes, seed=params.seed ^ PRETRAINED_SEED_SALT).finalize(self.device)
        self._rng_step = torch.tensor([1, 0], dtype=torch.int64, device=self.device)
        self.finetune = bool(params.get("finetune", False))
        self.reinit = bool(params.get("pretrain_reinit", True))
        self._model_initialised = False
        if not params.get("pretrain_path"):      # otherwise the epoch loop's load_pretrained runs it behind the load
            self._efficiency_init()

    def _efficiency_init(self):
        """mmin_miss.py:157-158: both models, after the checkpoint (if any) was loaded; the EMA copy is made after it (:164-165)"""
        if not self._model_initialised:
            efficiency_init(self.model)
            self._model_initialised = True
        if self.reinit:
            efficiency_init(self.pretrained_model)
        if self.use_ema:
            self.ema.copy_(self.model.flat.data)

    def load_pretrained(self, path):
        """``--pretrain_path``: ``models.model`` of a checkpoint written by ``--module=mmin_base`` here or by the reference goes
        into the pretrained model (mmin_miss.py:144-147), then efficiency_init runs (``--pretrain_reinit=False``: not on the
        pretrained model)"""
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        sd = ckpt["models"]["model"] if "models" in ckpt else ckpt
        own = self.pretrained_model.state_dict()
        if list(sd) != list(own):
            raise KeyError("--pretrain_path %s: not a mmin_base checkpoint (keys %s ...)" % (path, list(sd)[:3]))
        with torch.no_grad():
            for k, v in sd.items():
                own[k].copy_(v.to(own[k].device, own[k].dtype))
        self._efficiency_init()
        return ckpt

    def extra_models(self):
        return {"pretrained_model": {k: v.detach().cpu().clone() for k, v in self.pretrained_model.state_dict().items()}}

    def train_step(self, batch):
        self.model.train()
        self.pretrained_model.train()           # lumo's change_stage: every registered model without "ema" in its name
        enc = self.pretrained_model
        ws, _ = enc._encode(batch["audio_feature_reverse"], batch["visual_feature_reverse"], batch["text_feature_reverse"], True,
                            need_all=True)
        enc.rng_state.add_(self._rng_step)      # its own counter: one draw per step
        stats = self.model.loss_and_grads(batch, ws["fused"])
        self.optim.step()
        if self.use_ema:
            capi.ema_step(self.ema, self.model.flat.data, self.model.flat.numel, mmin.EMA_ALPHA)
        self.global_steps += 1
        return stats

    @staticmethod
    def make_loaders(params):
        return mmin.make_loaders(params, collate=lambda split: MMINMissCollate(has_miss=(split == "train")), transform=Missing(),
                                 name="mmin_miss")


class Missing:
    """the training set's output transform (mmin_miss.py:345-360): one ``random.choice`` of the six patterns per sample read"""

    def __init__(self):
        self.missing_type = [list(t) for t in MISSING_TYPES]
        self.modal_keys = list(MODAL_KEYS)
        self.missing_category = "zero"

    def __call__(self, dic):
        dic["missing_type"] = random.choice(self.missing_type)
        return dic


class MMINMissCollate:
    """MMINMissCollate (mmin_miss.py:303-342) on mmin_collate: with ``has_miss`` every modality x becomes x m and
    ``<key>_reverse`` = x (1 - m), m the sample's 0 / 1 entry of ``missing_type`` (columns visual, text, audio)"""

    def __init__(self, has_miss):
        self.has_miss = has_miss

    def __call__(self, samples):
        data = mmin.mmin_collate(samples)
        if self.has_miss:
            missing_type = torch.tensor([s["missing_type"] for s in samples], dtype=torch.long)
            for i, key in enumerate(MODAL_KEYS):
                features = data[key]
                m = missing_type[:, i][:, None, None]
                data[key] = features * m
                data[key + "_reverse"] = features * -1 * (m - 1)
            data["missing_type"] = missing_type
        return data
