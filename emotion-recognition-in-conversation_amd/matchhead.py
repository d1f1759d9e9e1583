"""The head that bc-LSTM / bc-GRU, DialogueRNN and the conv-emotion DialogueGCN end in (track_mm/dgcnv2_models.py:350-487,
:693-751): Q = E W^T + b (GEMM) -> matching attention 'general2' per dialogue over its valid rows (csrc/match_att.hip, row
width 200 or 300) -> ReLU(Linear) + dropout in the GEMM epilogue -> smax_fc + class-weighted loss in one launch, and the
backward of the same down to the gradient wrt E.  ``ConvEmotionModule`` is what the three modules share besides.
"""
import torch
from torch import nn

from . import capi
from .engine import linear_fwd, linear_wgrad


class Transform(nn.Module):           # MatchingAttention('general2'): its one parameterised layer
    def __init__(self, d):
        super().__init__()
        self.transform = nn.Linear(d, d, bias=True)


class ConvEmotionModule(nn.Module):
    """time-major batches ([T, B, D], padded row t*B + b) and a per-shape workspace cache ``self._ws``"""

    @property
    def _last_ws(self):
        """workspace of the most recent forward (tests / bench read results out of it)"""
        return self._ws.last

    def _shape(self, x, lens, label, n_nodes=None):
        T, B = int(x.shape[0]), int(x.shape[1])
        N = int(label.shape[0]) if label is not None else (int(n_nodes) if n_nodes is not None else int(lens.sum().item()))
        return B, T, N


class MatchAttHead:
    """The head over E [N, width] (row pitch ``width``, node order) with its parameters ``prefix`` + matchatt.transform.*,
    linear.*, smax_fc.* in ``flat`` and its buffers in the caller's workspace dict (``buffers``)."""
    CAP_F = 200        # the width erc_match_att_bwd_cap is built for
    NAMES = ("matchatt.transform.weight", "matchatt.transform.bias", "linear.weight", "linear.bias", "smax_fc.weight", "smax_fc.bias")

    def __init__(self, flat, prefix, width, hidden, n_classes, drop_p):
        self.flat, self.prefix, self.F, self.H, self.C, self.drop_p = flat, prefix, width, hidden, n_classes, drop_p

    @staticmethod
    def groups(prefix, owner):
        """FlatParams groups of the head's six parameters; ``owner`` holds .matchatt (Transform), .linear and .smax_fc"""
        return [[(prefix + n, owner.get_parameter(n))] for n in MatchAttHead.NAMES]

    def buffers(self, B, T, N, device, dE_rows=None, tail_pair=False):
        """``dE_rows``: rows of dE, when the caller keeps more than N (the zero row of capacity mode).  ``tail_pair``: capacity
        mode at a width erc_match_att_bwd_cap is not built for -- dQ and dE are the two halves of ONE buffer ``dQdE`` (dE
        starts at row N), so that one erc_mm_zero_tail launch clears the capacity rows of both."""
        # zeros, not empty: a stale NaN must never reach a weight-gradient GEMM through a row the step did not touch
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
        F, H, C = self.F, self.H, self.C
        dE_rows = N if dE_rows is None else dE_rows
        bufs = dict(Q=f32(N, F), A=f32(N, F), P=f32(B * T * T), TH=f32(B * T * T), Zc=f32(N, H), logits=f32(N, C), logp=f32(N, C),
                    stats=f32(max(256, capi.head_ce_stats_floats(N))), dlogits=f32(N, C), dZc=f32(N, H), dA=f32(N, F),
                    DZ=f32(B * T * T))
        if tail_pair:
            pair = f32(N + dE_rows, F)
            bufs.update(dQdE=pair, dQ=pair[:N], dE=pair[N:])
        else:
            bufs.update(dQ=f32(N, F), dE=f32(dE_rows, F))
        return bufs

    def _w(self, name):
        return self.flat.w(self.prefix + name)

    def _off(self, name):
        return self.flat.offsets[self.prefix + name]

    def forward(self, pl, ws, E, node_off, B, T, N, training, rng, with_logits=True):
        """E -> ws["Zc"] (and ws["logits"]); the log-softmax, where a model returns one, is the caller's"""
        F, H, C = self.F, self.H, self.C
        linear_fwd(pl, E, F, None, self._w("matchatt.transform.weight"), self._w("matchatt.transform.bias"), ws["Q"], F, N, F, F)
        capi.match_att_fwd(E, F, ws["Q"], F, node_off, B, T, F, ws["A"], F, ws["P"], ws["TH"])
        p = self.drop_p if training else 0.0
        linear_fwd(pl, ws["A"], F, None, self._w("linear.weight"), self._w("linear.bias"), ws["Zc"], H, N, H, F,
                   act=3 if p > 0 else 1, drop_p=p, rng=rng)
        if with_logits:
            linear_fwd(pl, ws["Zc"], H, None, self._w("smax_fc.weight"), self._w("smax_fc.bias"), ws["logits"], C, N, C, H)

    def att_backward(self, ws, E, node_off, B, T, n_dev=None, n_cap=0):
        """The matching attention's backward from ws["dA"]: ws["dQ"] and ws["dE"] (without the transform's dQ W).  Capacity mode
        (``n_cap`` > 0): rows [*n_dev, n_cap) of both are written +0 -- by erc_match_att_bwd_cap itself at width 200; at any
        other width by erc_mm_zero_tail over ws["dQdE"] (``buffers(tail_pair=True)``) behind the exact erc_match_att_bwd."""
        F = self.F
        pair = ws.get("dQdE") if n_cap else None
        if n_cap and F != self.CAP_F and pair is None:
            raise capi.ErcGraftError("MatchAttHead: capacity mode at width %d needs buffers(tail_pair=True)" % F)
        capi.match_att_bwd(E, F, ws["Q"], F, ws["dA"], F, node_off, B, T, F, ws["P"], ws["TH"], ws["DZ"], ws["dQ"], F, ws["dE"], F,
                           n_cap=0 if pair is not None else n_cap)
        if pair is not None:
            # rows [*n_dev, n_cap) of dQ (= pair rows [0, n_cap)) and of dE (= pair rows [n_cap, 2 n_cap)): one launch
            capi.mm_zero_tail(pair, F, F, 2, n_cap, n_dev)

    def backward(self, pl, ws, E, node_off, B, T, N, labels, class_weight, training, n_dev=None, n_cap=0):
        """Class-weighted cross entropy of the logits (stats in ws["stats"]), the head's weight gradients as deferred
        records of ``pl``, and ws["dE"] = the gradient wrt E, left for the caller's encoder backward.  At most 8 classes:
        smax_fc, the loss and their backward are one launch over ws["Zc"] (the forward ran with ``with_logits=False``).
        ``n_dev`` / ``n_cap``: capacity mode (erc_head_ce_cap; erc_match_att_bwd_cap at width 200, else the exact
        erc_match_att_bwd -- it walks the dialogues through node_off, empty slots have length 0 -- and erc_mm_zero_tail over
        the capacity rows of the ``tail_pair`` buffer)."""
        F, H, C = self.F, self.H, self.C
        dE = ws["dE"]
        p = self.drop_p if training else 0.0
        # smax_fc + cross entropy + their backward through the dropout / ReLU mask
        if C <= 8:
            capi.head_ce(ws["Zc"], H, H, C, N, self._w("smax_fc.weight"), self._w("smax_fc.bias"), labels, class_weight,
                         1.0 / (1.0 - p), ws["logits"], C, ws["dlogits"], C, ws["dZc"], H, ws["stats"], n_dev=n_dev)
        else:
            capi.cross_entropy(ws["logits"], C, C, N, None, labels, class_weight, 1.0, ws["dlogits"], C, ws["stats"])
            capi.gemm_f32(ws["dlogits"], C, 0, None, self._w("smax_fc.weight"), H, 1, None, ws["dZc"], H, N, H, C,
                          act=2, aux=ws["Zc"], ldaux=H, act_scale=1.0 / (1.0 - p))
        linear_wgrad(pl, ws["dlogits"], C, ws["Zc"], H, None, C, H, N, self._off("smax_fc.weight"), self._off("smax_fc.bias"),
                     defer=True)
        capi.gemm_f32(ws["dZc"], H, 0, None, self._w("linear.weight"), F, 1, None, ws["dA"], F, N, F, H)
        linear_wgrad(pl, ws["dZc"], H, ws["A"], F, None, H, F, N, self._off("linear.weight"), self._off("linear.bias"), defer=True)
        # matching attention: dQ and dE (key side + score side); E is also the query transform's input
        self.att_backward(ws, E, node_off, B, T, n_dev=n_dev, n_cap=n_cap)
        linear_wgrad(pl, ws["dQ"], F, E, F, None, F, F, N, self._off("matchatt.transform.weight"),
                     self._off("matchatt.transform.bias"), defer=True)
        capi.gemm_f32(ws["dQ"], F, 0, None, self._w("matchatt.transform.weight"), F, 1, None, dE, F, N, F, F, accumulate=1)
