"""2-layer bidirectional LSTM and GRU (hidden 100 per direction) on libercgraft: one class, ``BiRNN2``, driven by a ``Cell``.
``BiLSTM2``: the sequence-context encoder of DialogueGCN (``SeqContext``, packed; track_mm/dgcn_models.py:10-33) and of MMGCN's
text branch (unpacked over the padded length; track_mm/mmgcn.py:69,113-114).  ``torch.nn.LSTM`` parameter names / shapes are
kept (the module that owns the parameters IS an ``nn.LSTM``, used as a parameter holder only); the math runs in
``erc_gemm_*`` (hoisted input projections, all weight gradients) and ``erc_lstm_scan_*`` (the recurrence).  ``BiGRU2`` is the
same over ``erc_gru100_scan_*`` (the bc-GRU baseline, track_mm/dgcnv2_models.py:350-386).
"""
from typing import Callable, NamedTuple

import torch

from . import capi
from .engine import linear_fwd, linear_wgrad

H = 100


def lstm_groups(prefix, m):
    """FlatParams groups for an nn.LSTM(num_layers=2, bidirectional=True): forward|reverse members adjacent."""
    out = []
    for k in (0, 1):
        for base in ("weight_ih_l%d", "bias_ih_l%d", "weight_hh_l%d", "bias_hh_l%d"):
            n = base % k
            out.append([(prefix + n, getattr(m, n)), (prefix + n + "_reverse", getattr(m, n + "_reverse"))])
    return out


class Cell(NamedTuple):
    """What BiRNN2 has to know of a cell.  A new cell supplies this and its scans (csrc/rnn100_dev.h: what those share)."""
    name: str           # in error messages
    G: int              # gates: GX, the gates and the gate gradients are 2 * G * H wide
    saved: str          # the buffer [rows, 2H] the forward scan saves next to gates and Hprev
    key: str            # workspace key prefix, and "<rows_key>" the row count the workspace was made for
    rows_key: str
    rng_stream: int     # of the dropout between the layers
    scan_fwd: Callable  # (GX, ldgx, W_hh, b_hh, lengths .. T, Hout, ldh, Hdrop, ldhd, p, rng, stream, gates, saved, Hprev, t_dev=)
    scan_bwd: Callable  # (W_hh, lengths .. T, *bwd_state, dHout, lddh, p, rng, stream, *grads, t_dev=[, zero_to=])
    bwd_state: tuple    # the saved buffers the backward scan reads
    grads: tuple        # the gate gradients it writes: the input side first, the recurrent side (W_hh, b_hh) last
    zero_to: bool       # the backward scan has the compact-row capacity form (zero_to)


LSTM = Cell("BiLSTM2", 4, "Cst", "lstm:", "lstm_rows", 0x5EED0, capi.lstm_scan_fwd, capi.lstm_scan_bwd, ("gates", "Cst"), ("dGX", ),
            True)
# the GRU's recurrent side has a gradient of its own: dGH = dGX with the n block scaled by r (csrc/gru100.hip)
GRU = Cell("BiGRU2", 3, "ghn", "gru:", "gru_rows", 0x6EED0, capi.gru100_scan_fwd, capi.gru100_scan_bwd, ("gates", "ghn", "Hprev"),
           ("dGX", "dGH"), False)


class BiRNN2:
    """2-layer bidirectional recurrent encoder (hidden 100 per direction) of one ``Cell``: hoisted input projections and all
    weight gradients in ``erc_gemm_*`` / the step's ``erc_wgrad_table`` launch, the recurrence in the cell's scans.
    ``nn.LSTM`` / ``nn.GRU`` parameter names / shapes (gate order i|f|g|o / r|z|n)."""

    def __init__(self, flat, prefix, d_in, drop_p, cell):
        self.flat, self.prefix, self.d_in, self.drop_p, self.cell = flat, prefix, d_in, drop_p, cell
        self._own = {}     # buffers of callers that pass no store (tests): one set, replaced when the row count changes

    def _w(self, name):
        return self.flat.w(self.prefix + name)

    def _off(self, name):
        return self.flat.offsets[self.prefix + name]

    def _buf(self, rows, device, store=None):
        """The recurrence's saved state for ``rows`` positions.  ``store`` is the calling module's per-shape workspace
        dict: the buffers live (and are evicted, and are kept alive by a captured HIP graph) with it -- with compact rows
        the row count changes almost every step of a shuffled epoch, and a cache of its own here would grow by ~25 KB per
        row and distinct count."""
        c = self.cell
        if store is None:
            store = self._own
            if store.get(c.rows_key) != rows:
                store.clear()
        key = c.key + self.prefix
        ws = store.get(key)
        if ws is None or store.get(c.rows_key, rows) != rows:
            # zeros, not empty: rows of padded positions are never written but ARE read by the weight-gradient
            # GEMMs (times a zero gate gradient), so they must stay finite
            f32 = lambda w: torch.zeros(rows, w, dtype=torch.float32, device=device)
            two = lambda w: [f32(w), f32(w)]
            ws = dict(GX=two(2 * c.G * H), gates=two(2 * c.G * H), Hprev=two(2 * H), H0=f32(2 * H), H0d=f32(2 * H), dH0d=f32(2 * H))
            ws[c.saved] = two(2 * H)
            ws.update((g, two(2 * c.G * H)) for g in c.grads)
            store[key], store[c.rows_key] = ws, rows
        return ws

    def forward(self, pl, x, ldx, rows, B, T, sb, st, lengths, training, rng, out, ldo, x_bf16=False, node_off=None,
                node_row=None, store=None, t_dev=None):
        """x [*, d_in] -> out [rows, 200] (row pitch ldo).  Padded rows: row(b,t) = b*sb + t*st of x and of every buffer.
        ``t_dev`` (device int32; unpacked padded rows only, ``lengths`` and ``node_off`` None): T is a capacity and every
        dialogue runs *t_dev steps (erc_*_scan_fwd_tcap); ``node_row`` [rows] then only maps the rows of x.
        Compact rows (``node_off`` [B+1] and ``node_row`` [rows] given, packed sequences only): every buffer holds the
        ``rows`` = sum(lengths) valid positions in dialogue order (row = node_off[b] + t), x is read through node_row --
        the input projections, the saved state and the weight gradients shrink from B*T to sum(lengths) rows and the
        caller needs no gather / scatter between the padded and the node layout (DialogueGCN)."""
        c, W = self.cell, 2 * self.cell.G * H
        ws = self._buf(rows, out.device, store)
        p = self.drop_p if training else 0.0
        linear_fwd(pl, x, ldx, node_row, self._w("weight_ih_l0"), self._w("bias_ih_l0"), ws["GX"][0], W, rows, W,
                   self.d_in, x_bf16=x_bf16)
        c.scan_fwd(ws["GX"][0], W, self._w("weight_hh_l0"), self._w("bias_hh_l0"), lengths, node_off, sb, st, B, T, ws["H0"], 2 * H,
                   ws["H0d"], 2 * H, p, rng, c.rng_stream, ws["gates"][0], ws[c.saved][0], ws["Hprev"][0], t_dev=t_dev)
        linear_fwd(pl, ws["H0d"], 2 * H, None, self._w("weight_ih_l1"), self._w("bias_ih_l1"), ws["GX"][1], W, rows, W, 2 * H)
        c.scan_fwd(ws["GX"][1], W, self._w("weight_hh_l1"), self._w("bias_hh_l1"), lengths, node_off, sb, st, B, T, out, ldo, None, 0,
                   0.0, None, 0, ws["gates"][1], ws[c.saved][1], ws["Hprev"][1], t_dev=t_dev)
        self._last = (x, ldx, rows, B, T, sb, st, lengths, p, rng, x_bf16, node_off, node_row, store, t_dev)

    def backward(self, pl, dout, lddo, dx=None, lddx=0, zero_to=0):
        """dout = gradient wrt the layer-1 output.  Registers all weight-gradient jobs; optionally writes
        dx [rows, d_in] (needed when the encoder's input is itself trainable, MMGCN).  ``zero_to`` (compact rows, capacity mode;
        LSTM only): the gate gradients of rows [node_off[B], zero_to) are written 0, so the weight gradients may run over all
        rows; after a forward with ``t_dev`` the scans write those of rows t >= *t_dev 0 (ercgraft.h)."""
        c, W = self.cell, 2 * self.cell.G * H
        x, ldx, rows, B, T, sb, st, lengths, p, rng, x_bf16, node_off, node_row, store, t_dev = self._last
        if zero_to and not c.zero_to:
            raise capi.ErcGraftError("%s.backward: zero_to is not built (erc_%s has no capacity form)" % (c.name, c.scan_bwd.__name__))
        kw = dict(t_dev=t_dev, zero_to=zero_to) if c.zero_to else dict(t_dev=t_dev)
        ws = self._buf(rows, dout.device, store)
        # one gate-gradient buffer per layer (and side): every weight gradient of the encoder then joins the step's ONE batched
        # weight-gradient launch (erc_wgrad_table) instead of 6 split-K GEMMs + a slab reduce per layer pair
        for k in (1, 0):
            dH, lddh, pk, rngk, stream = (dout, lddo, 0.0, None, 0) if k == 1 else (ws["dH0d"], 2 * H, p, rng, c.rng_stream)
            xin, ldin, d_in, bf, gat = (ws["H0d"], 2 * H, 2 * H, False, None) if k == 1 else (x, ldx, self.d_in, x_bf16, node_row)
            grads = [ws[g][k] for g in c.grads]
            c.scan_bwd(self._w("weight_hh_l%d" % k), lengths, node_off, sb, st, B, T, *(ws[n][k] for n in c.bwd_state), dH, lddh,
                       pk, rngk, stream, *grads, **kw)
            dGX, dGH = grads[0], grads[-1]
            # W_ih (both directions stacked [2 G H, d_in]) and b_ih = the column sums of dGX
            linear_wgrad(pl, dGX, W, xin, ldin, gat, W, d_in, rows, self._off("weight_ih_l%d" % k),
                         self._off("bias_ih_l%d" % k), x_bf16=bf, defer=True)
            # W_hh per direction: dGH[:, G H d:]^T Hprev[:, H d:]; b_hh = the column sums of the direction's dGH (the bias strip
            # of this product; the LSTM's dGH is its dGX, so b_hh receives the same gradient as b_ih)
            for d in (0, 1):
                linear_wgrad(pl, dGH[:, c.G * H * d:], W, ws["Hprev"][k][:, H * d:], 2 * H, None, c.G * H, H, rows,
                             self._off("weight_hh_l%d" % k) + d * c.G * H * H, self._off("bias_hh_l%d" % k) + d * c.G * H,
                             defer=True)
            if k == 1:   # gradient wrt the (dropped) layer-0 output
                capi.gemm_f32(dGX, W, 0, None, self._w("weight_ih_l1"), 2 * H, 1, None, ws["dH0d"], 2 * H, rows, 2 * H, W)
            elif dx is not None:
                if node_row is not None:
                    raise capi.ErcGraftError("%s.backward: dx with compact rows is not built" % c.name)
                capi.gemm_f32(dGX, W, 0, None, self._w("weight_ih_l0"), self.d_in, 1, None, dx, lddx, rows, self.d_in, W)


def BiLSTM2(flat, prefix, d_in, drop_p=0.4):
    """the LSTM encoder over ``erc_lstm_scan_*`` (csrc/lstm.hip)"""
    return BiRNN2(flat, prefix, d_in, drop_p, LSTM)


def BiGRU2(flat, prefix, d_in, drop_p=0.5):
    """the GRU encoder over ``erc_gru100_scan_*`` (csrc/gru100.hip), the bc-GRU baseline"""
    return BiRNN2(flat, prefix, d_in, drop_p, GRU)


def gru_groups(prefix, m):
    """FlatParams groups for an nn.GRU(num_layers=2, bidirectional=True): forward|reverse members adjacent, so that each
    layer's input projection is one [600, d_in] GEMM and W_hh / b_hh of the two directions are one [2][300, .] operand."""
    return lstm_groups(prefix, m)
