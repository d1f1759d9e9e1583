"""ctypes binding of libercgraft.so (include/ercgraft.h).

PyTorch is plumbing here: tensors own device memory, ``data_ptr()`` and the
current stream handle are passed straight through the C-ABI.  There is NO
fallback: if the library is missing or a call fails, this raises.

The header is the only place an entry point's types are written down: every
``erc_*`` prototype is parsed at import (``parse_header``), and ``_call``
checks each wrapper's arguments against it.  A new entry point is declared in
the header and gets a wrapper here.
"""
import ctypes as C
import os
import re
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ERC_LIB_PATH") or os.path.join(_HERE, "lib", "libercgraft.so")   # override: A/B builds
CSRC = os.path.join(_HERE, "csrc")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "ercgraft.h")


class ErcGraftError(RuntimeError):
    pass


_CTYPES = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float}


def _ctype(decl, proto, ret=False):
    """ctypes type of a declaration without its name: any pointer is c_void_p, a returned ``const char*`` c_char_p"""
    t = " ".join(decl.replace("*", " * ").split())
    if ret and t == "const char *":
        return C.c_char_p
    if "*" in t:
        return C.c_void_p
    t = re.sub(r"\bconst\b", "", t).strip()
    if t not in _CTYPES:
        raise ErcGraftError("%s: type '%s' has no ctypes mapping" % (proto, t))
    return _CTYPES[t]


def parse_header(text):
    """{name: (restype, argtypes, parameter names)} of every ``erc_*`` prototype in C header ``text``."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)          # preprocessor lines
    protos = {}
    for decl in re.split(r"[;{}]", text):
        m = re.fullmatch(r"\s*(.*?)\b(erc_\w+)\s*\((.*)\)\s*", decl, flags=re.S)
        if m is None:
            continue
        ret, name, params = m.groups()
        argtypes, names = [], []
        for p in ([] if params.strip() == "void" else params.split(",")):
            pm = re.fullmatch(r"\s*(.+?)\b(\w+)\s*", p, flags=re.S)
            if pm is None:
                raise ErcGraftError("%s: cannot parse parameter '%s'" % (name, p.strip()))
            argtypes.append(_ctype(pm.group(1), name))
            names.append(pm.group(2))
        protos[name] = (_ctype(ret, name, ret=True), argtypes, tuple(names))
    return protos


with open(HEADER) as _fh:
    _header = _fh.read()
PROTOS = parse_header(_header)
EXPORTS = tuple(PROTOS)
ERC_ABI_VERSION = int(re.search(r"^\s*#\s*define\s+ERC_ABI_VERSION\s+(\d+)", _header, flags=re.M).group(1))
del _header


def _launches(name):
    """the entry point enqueues work: its last parameter is the stream"""
    return PROTOS[name][2][-1:] == ("stream",)


_lib = None
_raw = None
_record = None     # list of (entry point, argument tuple) while a recording is active (bench.py kernel probes)


def start_recording():
    """Record every C-ABI call (name + raw arguments) until stop_recording(): bench.py replays single entry points with
    the exact operands a training step gave them, to time the step's dominant kernel on its own."""
    global _record
    _record = []


def stop_recording():
    global _record
    rec, _record = _record, None
    return rec


def replay(entry):
    """Re-issue a recorded call, a launching entry point's on the CURRENT stream."""
    name, args = entry
    if _launches(name):
        args = args[:-1] + (stream(),)
    _check(getattr(_raw, name)(*args), name)


def build(verbose=False):
    """Compile csrc/*.hip for gfx950 into lib/libercgraft.so (hipcc cross-compiles without a GPU)."""
    res = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout[-4000:])
        print(res.stderr[-4000:])
    if res.returncode != 0:
        raise ErcGraftError("building libercgraft.so failed")
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ErcGraftError(
                "libercgraft.so not found at %s: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU / PyTorch fallback for the hot path)" % LIB_PATH)
        global _raw
        handle = C.CDLL(LIB_PATH)

        class _Recording:          # same attribute surface as the CDLL handle; one global test per call when idle
            pass
        rec = _Recording()
        for name, (res, args, _) in PROTOS.items():
            fn = getattr(handle, name)  # AttributeError = symbol missing: fail loudly
            fn.restype, fn.argtypes = res, args

            def call(*a, _fn=fn, _name=name):
                if _record is not None:
                    _record.append((_name, a))
                return _fn(*a)
            setattr(rec, name, call)
        if handle.erc_abi_version() != ERC_ABI_VERSION:
            raise ErcGraftError("libercgraft ABI version mismatch")
        _raw, _lib = handle, rec
    return _lib


def _check(code, name):
    if code != 0:
        raise ErcGraftError("%s failed (%d): %s" % (name, code, lib().erc_last_error().decode()))


def stream():
    return torch.cuda.current_stream().cuda_stream


def _call(name, *args):
    """Call status-returning entry point ``name`` with the arguments of its prototype, the stream excluded: a tensor (it
    must live on the GPU) becomes its data_ptr(), None NULL; ints, floats and ctypes objects pass through.  The current
    stream is appended when the prototype ends in one; a non-zero status raises."""
    names, launches = PROTOS[name][2], _launches(name)
    if len(args) != len(names) - launches:
        raise ErcGraftError("%s takes %d arguments, got %d" % (name, len(names) - launches, len(args)))
    conv = []
    for a, pname in zip(args, names):
        if isinstance(a, torch.Tensor):
            if not a.is_cuda:
                raise ErcGraftError("%s: %s must live on the GPU (got a %s tensor)" % (name, pname, a.device))
            a = a.data_ptr()
        conv.append(a)
    if launches:
        conv.append(stream())
    _check(getattr(lib(), name)(*conv), name)


# --------------------------------------------------------------------------- wrappers
def window_graph_build(lengths, speakers, spk_sb, spk_st, B, T, wp, wf, S, n_cap, e_cap, g, edge_index=None,
                       edge_type=None, desc=None):
    """``desc`` (int32 [2 B]: lengths | first store rows, or None): resident batch, node_row gets store rows (ercgraft.h)"""
    args = (lengths, speakers, spk_sb, spk_st, B, T, wp, wf, S, n_cap, e_cap, g["node_off"], g["node_row"], g["node_spk"],
            g["in_ptr"], g["in_src"], g["in_typ"], g["out_ptr"], g["out_dst"], g["out_typ"], g["out_eid"], edge_index, edge_type,
            g["counts"])
    if desc is None:
        _call("erc_window_graph_build", *args)
    else:
        _call("erc_window_graph_build_desc", *args, desc)


def gemm_f32(A, lda, a_kmajor, a_gather, B, ldb, b_kmajor, b_gather, Cmat, ldc, M, N, K, split_k=1, c_slab=0,
             ones_col=0, bias_out=None, bias_slab=0, bias=None, act=0, aux=None, ldaux=0, act_scale=1.0,
             drop_p=0.0, rng_state=None, accumulate=0):
    _call("erc_gemm_f32", A, lda, a_kmajor, a_gather, B, ldb, b_kmajor, b_gather, Cmat, ldc, M, N, K, split_k, c_slab, ones_col,
          bias_out, bias_slab, bias, act, aux, ldaux, act_scale, drop_p, rng_state, accumulate)


def gemm_f32_stream(A, lda, a_kmajor, a_gather, B, ldb, b_kmajor, b_gather, Cmat, ldc, M, N, K, split_k=1, c_slab=0,
                    ones_col=0, bias_out=None, bias_slab=0, bias=None, act=0, aux=None, ldaux=0, act_scale=1.0,
                    drop_p=0.0, rng_state=None, accumulate=0):
    """the streaming kernel under its own name (erc_gemm_f32 hands it every N <= 1024)"""
    _call("erc_gemm_f32_stream", A, lda, a_kmajor, a_gather, B, ldb, b_kmajor, b_gather, Cmat, ldc, M, N, K, split_k, c_slab,
          ones_col, bias_out, bias_slab, bias, act, aux, ldaux, act_scale, drop_p, rng_state, accumulate)


def gemm_f32_stream_form(A, lda, a_kmajor, a_gather, B, ldb, b_kmajor, b_gather, Cmat, ldc, M, N, K, split_k=1, c_slab=0,
                         ones_col=0, bias_out=None, bias_slab=0, bias=None, act=0, aux=None, ldaux=0, act_scale=1.0,
                         drop_p=0.0, rng_state=None, accumulate=0):
    """(a_mode, b_mode, nw, gather_a, gather_b, vec, rm, cf) of the kernel gemm_f32_stream runs for these arguments (ercgraft.h).
    Nothing is launched or dereferenced: operands may be GPU tensors or plain integer addresses."""
    form = (C.c_int32 * 8)()
    _call("erc_gemm_f32_stream_form", A, lda, a_kmajor, a_gather, B, ldb, b_kmajor, b_gather, Cmat, ldc, M, N, K, split_k,
          c_slab, ones_col, bias_out, bias_slab, bias, act, aux, ldaux, act_scale, drop_p, rng_state, accumulate, form)
    return tuple(form)


def gemm_bf16x(A, lda, a_kmajor, a_gather, B, ldb, b_kmajor, b_gather, x_is_a, Cmat, ldc, M, N, K, split_k=1,
               c_slab=0, ones_col=0, bias_out=None, bias_slab=0):
    _call("erc_gemm_bf16x", A, lda, a_kmajor, a_gather, B, ldb, b_kmajor, b_gather, x_is_a, Cmat, ldc, M, N, K, split_k, c_slab,
          ones_col, bias_out, bias_slab)


def gemm_x3(A, lda, B, ldb, Cmat, ldc, M, N, K, split_k=1, c_slab=0):
    """C = A B^T (both K-contiguous fp32) on the bf16 matrix cores through a three-term split: fp32-class (ercgraft.h)"""
    _call("erc_gemm_x3", A, lda, B, ldb, Cmat, ldc, M, N, K, split_k, c_slab)


def gemm_x3_grouped(A, lda, B, ldb, Cmat, pitch, node_off, n_dlg, n_mod, n_nodes, max_rows, K, split_k=1, c_slab=0):
    """per-(dialogue, modality) blocks A_rows B_rows^T with the three-term split (erc_gemm_f32_grouped form 1; ercgraft.h)"""
    _call("erc_gemm_x3_grouped", A, lda, B, ldb, Cmat, pitch, node_off, n_dlg, n_mod, n_nodes, max_rows, K, split_k, c_slab)


def gemm_bf16a_stream(X, ldx, gather, W, ldw, Cm, ldc, M, N, K, bias=None, act=0):
    _call("erc_gemm_bf16a_stream", X, ldx, gather, W, ldw, int(W.dtype == torch.bfloat16), Cm, ldc, M, N, K, bias, act)


def gemm_bf16a_stream_form(X, ldx, gather, W, ldw, Cm, ldc, M, N, K, bias=None, act=0, w_is_bf16=None):
    """(kernel, nw, w_is_bf16, ub, a_vec, b_vec) of the kernel gemm_bf16a_stream runs for these arguments (ercgraft.h).  Nothing
    is launched or dereferenced: operands may be GPU tensors or plain integer addresses (then ``w_is_bf16`` must be given)."""
    if w_is_bf16 is None:
        w_is_bf16 = W.dtype == torch.bfloat16
    form = (C.c_int32 * 6)()
    _call("erc_gemm_bf16a_stream_form", X, ldx, gather, W, ldw, int(w_is_bf16), Cm, ldc, M, N, K, bias, act, form)
    return tuple(form)


def slab_reduce(slabs, S, stride, bias, n_cols, act, out, numel, ld_out=0):
    _call("erc_slab_reduce", slabs, S, stride, bias, n_cols, act, out, ld_out, numel)


def slab_reduce_batched(ws, dst, jobs, n_jobs, max_numel):
    _call("erc_slab_reduce_batched", ws, dst, jobs, n_jobs, max_numel)


def rgcn_mean_fwd(x, ldx, F, R, N, g, Mout, ldm, inv_cnt):
    _call("erc_rgcn_mean_fwd", x, ldx, F, R, N, g["in_ptr"], g["in_src"], g["in_typ"], Mout, ldm, inv_cnt)


def rgcn_mean_bwd(dM, ldm, F, R, N, g, inv_cnt, dx, lddx):
    _call("erc_rgcn_mean_bwd", dM, ldm, F, R, N, g["out_ptr"], g["out_dst"], g["out_typ"], inv_cnt, dx, lddx)


def tconv_attn_fwd(qkvs, ld, F, N, scale, g, out, ldo, alpha):
    _call("erc_tconv_attn_fwd", qkvs, ld, F, N, scale, g["in_ptr"], g["in_src"], out, ldo, alpha)


def tconv_attn_bwd(qkvs, ld, F, N, scale, g, alpha, dout, lddo, dqkvs, dscore, bn=None):
    """``bn`` = (x, ldx, gamma, saved, bn_bwd, dout_store): ``dout`` is then dY of the BatchNorm behind the layer and the
    layer's own output gradient is derived inside the target pass (and stored in ``dout_store``)."""
    if bn is None:
        bn, dsrc = (None, 0, None, None, None, None), dout
    else:
        dsrc = bn[5]
    _call("erc_tconv_attn_bwd_target", qkvs, ld, F, N, scale, g["in_ptr"], g["in_src"], alpha, dout, lddo, dqkvs, dscore, *bn)
    _call("erc_tconv_attn_bwd_source", qkvs, ld, F, N, g["out_ptr"], g["out_dst"], g["out_eid"], alpha, dscore, dsrc, lddo, dqkvs)


def bn_ws_floats(F):
    return int(lib().erc_bn_ws_floats(F))


def bn_lrelu_fwd(x, ldx, N, F, gamma, beta, rmean, rvar, momentum, eps, slope, training, saved, y, ldy, ws):
    _call("erc_bn_lrelu_fwd", x, ldx, N, F, gamma, beta, rmean, rvar, momentum, eps, slope, int(training), saved, y, ldy, ws)


def bn_lrelu_bwd(x, ldx, N, F, gamma, beta, saved, slope, dy, lddy, dx, lddx, dgamma, dbeta, ws):
    _call("erc_bn_lrelu_bwd", x, ldx, N, F, gamma, beta, saved, slope, dy, lddy, dx, lddx, dgamma, dbeta, ws)


def cross_entropy(logits, ld, Cn, n_rows, row_map, labels, weight, grad_scale, dlogits, lddl, stats):
    _call("erc_cross_entropy", logits, ld, Cn, n_rows, row_map, labels, weight, grad_scale, dlogits, lddl, stats)


def cross_entropy_cap(logits, ld, Cn, n_cap, n_dev, row_map, labels, weight, grad_scale, dlogits, lddl, stats):
    """erc_cross_entropy over the first *n_dev (device int32) of n_cap samples (ercgraft.h)"""
    _call("erc_cross_entropy_cap", logits, ld, Cn, n_cap, n_dev, row_map, labels, weight, grad_scale, dlogits, lddl, stats)


def rows_score(logits, ld, n_logit_rows, Cn, n_cap, n_dev, row_map, labels, cm):
    """argmax of the rows row_map[i], i < *n_dev, counted into cm int64 [C, C] (true x predicted), which is added to"""
    _call("erc_rows_score", logits, ld, n_logit_rows, Cn, n_cap, n_dev, row_map, labels, cm)


def rows_score_max_classes():
    return int(lib().erc_rows_score_max_classes())


def adam_step(p, g, m, v, n, lr, b1, b2, eps, wd, decoupled, grad_scale, clip_norm, gnorm, state, shadow=None,
              shadow_off=0, shadow_n=0, skip_flag=None):
    _call("erc_adam_step", p, g, m, v, n, lr, b1, b2, eps, wd, int(decoupled), grad_scale, clip_norm, gnorm, state, shadow,
          shadow_off, shadow_n, skip_flag)


class ShadowTable:
    """Host mirror of ErcShadowTab (ercgraft.h): bf16 shadow ranges of the flat parameter buffer, all inside ONE bf16
    buffer.  ``add`` returns the index of the new range (``view(i)`` = its destination block)."""

    MAX = 8

    def __init__(self, device):
        self.device = device
        self.descs = []
        self.sizes = []
        self.numel = 0
        self.buf = None
        self._packed = None

    def add(self, src_off, n_el, dst_numel, n0, n1, sn, sk, ld, mode, terms=1):
        """digits (idx % n0, (idx / n0) % n1, idx / (n0 n1)) -> n = digits . sn, k = digits . sk; mode 0 row-major [n][ld],
        mode 1 MFMA B-fragment order with ld K blocks.  ``terms`` > 1: that many bf16 planes of ``dst_numel`` elements each
        (rounded up to 64), plane t = term t of the parameter's bf16 expansion (split compute modes)."""
        if self.buf is not None or len(self.descs) == self.MAX:
            raise ErcGraftError("shadow table is sealed or full")
        dst_off = (self.numel + 63) // 64 * 64       # 128-byte aligned blocks
        plane = (dst_numel + 63) // 64 * 64
        self.descs.append((src_off, n_el, dst_off, n0, n1) + tuple(sn) + tuple(sk) + (ld, mode, plane if terms > 1 else 0, terms, 0))
        self.sizes.append(plane * terms if terms > 1 else dst_numel)
        self.numel = dst_off + self.sizes[-1]
        return len(self.descs) - 1

    def seal(self):
        import struct
        self.buf = torch.zeros(self.numel + 64, dtype=torch.bfloat16, device=self.device)
        raw = struct.pack("<ii", len(self.descs), 0)
        for d in self.descs:
            raw += struct.pack("<qqq10iq2i", *d)
        raw += b"\0" * (8 + 80 * self.MAX - len(raw))
        self._packed = C.create_string_buffer(raw, len(raw))
        return self

    def view(self, i):
        off = self.descs[i][2]
        return self.buf[off:off + self.sizes[i]]

    def plane(self, i):
        """elements between the term planes of range i (0: a single plane)"""
        return self.descs[i][13]

    @property
    def tab_ptr(self):
        return C.addressof(self._packed)


def _shadow(table):
    """(shadow_base, shadow_numel, tab_host) arguments of a ShadowTable, or of none"""
    return (None, 0, None) if table is None else (table.buf, table.buf.numel(), table.tab_ptr)


def mfma_b_fragment_order(W, n_kblocks):
    """Reference packing of a logical B operand W [n][k] (torch tensor) into ErcShadowTab mode 1 order (tests)."""
    n, k = W.shape
    nt = (n + 15) // 16
    P = torch.zeros(nt * 16, n_kblocks * 32, dtype=W.dtype, device=W.device)
    P[:n, :k] = W
    # [ct][r][kb][g][j] -> [ct][kb][g][r][j]
    return P.view(nt, 16, n_kblocks, 4, 8).permute(0, 2, 3, 1, 4).contiguous().view(-1)


def adam_step_tab(p, g, m, v, n, lr, b1, b2, eps, wd, decoupled, grad_scale, clip_norm, gnorm, state, table, skip_flag=None):
    _call("erc_adam_step_tab", p, g, m, v, n, lr, b1, b2, eps, wd, int(decoupled), grad_scale, clip_norm, gnorm, state,
          *_shadow(table), skip_flag)


class ErcP2P(C.Structure):
    """host mirror of ErcP2P (ercgraft.h)"""
    _fields_ = [("world", C.c_int32), ("rank", C.c_int32), ("spin_limit", C.c_int32), ("pad", C.c_int32),
                ("pub", C.c_void_p * 8), ("flags", C.c_void_p * 8), ("epoch", C.c_void_p), ("health", C.c_void_p),
                ("n_pad", C.c_int64)]


def p2p_alloc(nbytes):
    """(device pointer, 64-byte IPC handle) of a zero-filled buffer other processes can map"""
    out, handle = C.c_void_p(), C.create_string_buffer(64)
    _call("erc_p2p_alloc", nbytes, C.addressof(out), C.addressof(handle))
    return out.value, handle.raw


def p2p_open(handle):
    out = C.c_void_p()
    _call("erc_p2p_open", C.c_char_p(handle), C.addressof(out))
    return out.value


def p2p_close(ptr_):
    _call("erc_p2p_close", C.c_void_p(ptr_))


def p2p_free(ptr_):
    _call("erc_p2p_free", C.c_void_p(ptr_))


def adam_step_p2p(p, g, m, v, n, lr, b1, b2, eps, wd, decoupled, grad_scale, state, table, x):
    """x: ErcP2P.  table: ShadowTable or None."""
    _call("erc_adam_step_p2p", p, g, m, v, n, lr, b1, b2, eps, wd, int(decoupled), grad_scale, state, *_shadow(table),
          C.addressof(x))


def health_roll(health, events):
    """start of a step: a health word still raised becomes one event, the word is cleared (ercgraft.h)"""
    _call("erc_health_roll", health, events)


HEALTH_RAISED = 0x3f800000


def gcnii_chain_set_spin_limit(limit):
    _call("erc_gcnii_chain_set_spin_limit", int(limit))


def shadow_refresh(p, n, table):
    _call("erc_shadow_refresh", p, n, *_shadow(table))


def cogmen_project_graph_ok(K, n_out, B, ldx, ldw):
    return bool(lib().erc_cogmen_project_graph_ok(K, n_out, B, ldx, ldw))


def cogmen_project_graph(x, ldx, W, ldw, bias, H0, ldh0, n_out, K, lengths, speakers, B, T, wp, wf, n_speakers, n_cap, e_cap, g,
                         desc=None, terms=1, w_plane=0):
    """input projection + window graph in one launch (csrc/cogmen_project.hip); g: the graph dict of window_graph_build, plus an
    optional ``node_rec`` (int32 [n_cap + 1, 4]: the node records the tile kernels derive their graph slices from, ercgraft.h).
    desc (int32 [2 B]: lengths | first store rows): resident mode -- x / speakers are a store's [U, ldx] / [U] arrays.
    terms = 2 | 3: split compute mode -- x fp32, W = that many bf16 term planes ``w_plane`` elements apart"""
    sb, st = (0, speakers.stride(0)) if desc is not None else (speakers.stride(0), speakers.stride(1))
    if terms > 1:
        if x.dtype != torch.float32:
            raise ErcGraftError("cogmen_project_graph: split modes take the fp32 feature block")
        _call("erc_cogmen_project_graph_x", terms, x, ldx, W, w_plane, ldw, bias, H0, ldh0, n_out, K, lengths, speakers, sb, st,
              B, T, wp, wf, n_speakers, n_cap, e_cap, g["node_off"], g["node_row"], g["node_spk"], g["in_ptr"], g["in_src"],
              g["in_typ"], g["out_ptr"], g["out_dst"], g["out_typ"], g["out_eid"], g["counts"], desc, g.get("node_rec"))
        return
    _call("erc_cogmen_project_graph", x, ldx, W, ldw, bias, H0, ldh0, n_out, K, lengths, speakers, sb, st, B, T, wp, wf,
          n_speakers, n_cap, e_cap, g["node_off"], g["node_row"], g["node_spk"], g["in_ptr"], g["in_src"], g["in_typ"],
          g["out_ptr"], g["out_dst"], g["out_typ"], g["out_eid"], g["counts"], desc, g.get("node_rec"))


def cogmen_set_stamps(t):
    _call("erc_cogmen_set_stamps", t)


def lstm_set_stamps(t):
    _call("erc_lstm_set_stamps", t)


def head_set_stamps(t):
    _call("erc_head_set_stamps", t)


def cogmen_fwd_tile_ws_doubles(n):
    return int(lib().erc_cogmen_fwd_tile_ws_doubles(n))


def cogmen_fwd_tile(H0, ldh0, N, wp, wf, g, WcatT, b1, Wq, bq, scale, Mb, ldmb, inv_cnt, H1b, ldh1b, QKVS, H2, ldh2, alpha,
                    bn_fused=False, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, saved=None, bn_ws=None,
                    n_speakers=2, n_dev=None, health=None, events=None, terms=1, catT_plane=0, q_plane=0):
    """terms = 2 | 3: split compute mode -- WcatT / Wq are term planes, Mb / H1b the FP32 operand buffers (erc_cogmen_fwd_tile_x)"""
    if terms > 1:
        _call("erc_cogmen_fwd_tile_x", terms, H0, ldh0, N, wp, wf, g["in_ptr"], g["in_src"], g["in_typ"], WcatT, catT_plane, b1,
              Wq, q_plane, bq, scale, Mb, ldmb, inv_cnt, H1b, ldh1b, QKVS, H2, ldh2, alpha, int(bn_fused), running_mean,
              running_var, momentum, eps, saved, bn_ws, g["node_spk"], n_speakers, n_dev, health, events, g.get("node_rec"))
        return
    _call("erc_cogmen_fwd_tile", H0, ldh0, N, wp, wf, g["in_ptr"], g["in_src"], g["in_typ"], WcatT, b1, Wq, bq, scale, Mb, ldmb,
          inv_cnt, H1b, ldh1b, QKVS, H2, ldh2, alpha, int(bn_fused), running_mean, running_var, momentum, eps, saved, bn_ws,
          g["node_spk"], n_speakers, n_dev, health, events, g.get("node_rec"))


def cogmen_bwd_tile(dY, H2, ldh2, N, wp, wf, gamma, saved, bn_bwd, QKVS, alpha, g, inv_cnt, WqT, Wb, scale, dQKVS, dH1,
                    dH0, lddh0, n_speakers=2, head_part=None, head_parts=0, dgamma=None, dbeta=None, stats=None, grads_bf16=False,
                    lddh1=100, n_dev=None, terms=1, qT_plane=0, wb_plane=0):
    """terms = 2 | 3: split compute mode -- WqT / Wb are term planes, the gradients fp32 (erc_cogmen_bwd_tile_x)"""
    if terms > 1:
        _call("erc_cogmen_bwd_tile_x", terms, dY, H2, ldh2, N, wp, wf, gamma, saved, bn_bwd, QKVS, alpha, g["in_ptr"],
              g["in_src"], g["out_ptr"], g["out_dst"], g["out_typ"], g["out_eid"], inv_cnt, WqT, qT_plane, Wb, wb_plane, scale,
              dQKVS, dH1, dH0, lddh0, g["node_spk"], n_speakers, head_part, head_parts,
              head_fused_part_floats() if head_part is not None else 0, dgamma, dbeta, stats, lddh1, n_dev, g.get("node_rec"))
        return
    _call("erc_cogmen_bwd_tile", dY, H2, ldh2, N, wp, wf, gamma, saved, bn_bwd, QKVS, alpha, g["in_ptr"], g["in_src"],
          g["out_ptr"], g["out_dst"], g["out_typ"], g["out_eid"], inv_cnt, WqT, Wb, scale, dQKVS, dH1, dH0, lddh0, g["node_spk"],
          n_speakers, head_part, head_parts, head_fused_part_floats() if head_part is not None else 0, dgamma, dbeta, stats,
          int(grads_bf16), lddh1, n_dev, g.get("node_rec"))


def grad_norm(g, n, grad_scale, gnorm, ws):
    _call("erc_grad_norm", g, n, grad_scale, gnorm, ws)


def gcnii_chain_prep(W, w_stride, lamda, alpha, VT, V, U, UT=None):
    _call("erc_gcnii_chain_prep", W, w_stride, lamda, alpha, VT, V, U, UT)


def gcnii_chain_config(B, T, Mo, P):
    out = (C.c_int * 3)()
    _call("erc_gcnii_chain_config", B, T, Mo, P, C.addressof(out), C.addressof(out) + 4, C.addressof(out) + 8)
    return int(out[0]), int(out[1]), int(out[2])


def gcnii_chain_fwd(ADJ, P, CR, node_off, N, Mo, B, T, cfg, VT, Call, ldc, HD, hd_plane, ZS, lds, ZX, state, drop_p, rng,
                    rng_stream0, health=None):
    _call("erc_gcnii_chain_fwd", ADJ, P, CR, node_off, N, Mo, B, T, cfg[0], cfg[1], cfg[2], VT, Call, ldc, HD, hd_plane, ZS, lds,
          ZX, state, health, drop_p, rng, rng_stream0)


def gcnii_chain_bwd(ADJ, P, CR, node_off, N, Mo, B, T, cfg, V, HD, hd_plane, dHin, dHout, DG, DZ, lds, ZX, state, drop_p,
                    health=None):
    _call("erc_gcnii_chain_bwd", ADJ, P, CR, node_off, N, Mo, B, T, cfg[0], cfg[1], cfg[2], V, HD, hd_plane, dHin, dHout, DG, DZ,
          lds, ZX, state, health, drop_p)


def dag_rec_config(direction, B, T, n_layers, epc_hint=0, dg_hint=0, lpl_hint=0):
    """cfg = (epc, dg, groups per launch, layers per launch) of the weight-stationary DAG-ERC recurrence (0 forward,
    1 backward) on the current device, as a ctypes int array the launch wrappers take."""
    cfg = (C.c_int * 4)()
    _call("erc_dag_rec_config", direction, B, T, n_layers, epc_hint, dg_hint, lpl_hint, C.addressof(cfg))
    return cfg


def dag_rec_set_stamps(t):
    _call("erc_dag_rec_set_stamps", t)


def dag_rec_scratch_bytes(direction, B, T, cfg):
    return int(lib().erc_dag_rec_scratch_bytes(direction, B, T, C.addressof(cfg)))


def ptr_table(tensors):
    """host array of device pointers (one per layer) for the per-layer operands of erc_dag_rec_fwd"""
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def dag_rec_fwd(H0, ldh0, n_layers, tables, pred, spk, B, T, ldo, ldgi, cfg, state, scratch, health=None):
    """tables: dict of ptr_table()s -- Wh bh W_hh_c b_hh_c W_ih_p b_ih_p Wr w_k | H1 GI Mseq GH R ks alpha"""
    t = tables
    _call("erc_dag_rec_fwd", H0, ldh0, n_layers, C.addressof(t["Wh"]), C.addressof(t["bh"]), C.addressof(t["W_hh_c"]),
          C.addressof(t["b_hh_c"]), C.addressof(t["W_ih_p"]), C.addressof(t["b_ih_p"]), C.addressof(t["Wr"]),
          C.addressof(t["w_k"]), pred, spk, B, T, C.addressof(t["H1"]), ldo, C.addressof(t["GI"]), ldgi, C.addressof(t["Mseq"]),
          C.addressof(t["GH"]), C.addressof(t["R"]), C.addressof(t["ks"]), C.addressof(t["alpha"]), C.addressof(cfg), state,
          health, scratch)


def dag_rec_bwd(n_layers, tables, ldh, ldgi, pred, spk, B, T, dHall, ldd, lddgi, cfg, state, scratch, health=None):
    """tables: ptr_table()s -- Hl GI GH Mseq R alpha Wh W_hh_c W_ih_p Wr w_k | DGI DGH dM dks"""
    t = tables
    _call("erc_dag_rec_bwd", n_layers, C.addressof(t["Hl"]), ldh, C.addressof(t["GI"]), ldgi, C.addressof(t["GH"]),
          C.addressof(t["Mseq"]), C.addressof(t["R"]), C.addressof(t["alpha"]), C.addressof(t["Wh"]), C.addressof(t["W_hh_c"]),
          C.addressof(t["W_ih_p"]), C.addressof(t["Wr"]), C.addressof(t["w_k"]), pred, spk, B, T, dHall, ldd,
          C.addressof(t["DGI"]), lddgi, C.addressof(t["DGH"]), C.addressof(t["dM"]), C.addressof(t["dks"]), C.addressof(cfg),
          state, health, scratch)


def dag_attn_sums(alpha, H1, ldo, pred, spk, B, T, A):
    _call("erc_dag_attn_sums", alpha, H1, ldo, pred, spk, B, T, A)


def dag_meta(speaker_onehot, speaker_ids, sb, st, S, lengths, B, T, spk, pred, node_off, node_row):
    _call("erc_dag_meta", speaker_onehot, speaker_ids, sb, st, S, lengths, B, T, spk, pred, node_off, node_row)


def dag_meta_cap(speaker_onehot, speaker_ids, sb, st, S, lengths, desc, store_speaker, store_label, zero_store_row, B, T, n_cap,
                 spk, pred, node_off, node_row, x_row, label_out, counts):
    """erc_dag_meta in capacity mode: bucket form (lengths + padded speakers) or resident form (desc + the store's arrays)"""
    _call("erc_dag_meta_cap", speaker_onehot, speaker_ids, sb, st, S, lengths, desc, store_speaker, store_label, zero_store_row,
          B, T, n_cap, spk, pred, node_off, node_row, x_row, label_out, counts)


def _scan(base, args, lengths_at, t_at, t_dev, zero_to=0):
    """One hidden-100 scan launch.  ``args`` is the argument tuple of ``erc_<base>``, with lengths and node_off at position
    ``lengths_at``.  ``t_dev`` chooses ``erc_<base>_tcap``, the unpacked padded-row form: it takes neither of the two and has
    t_dev at position ``t_at`` (behind T); else ``zero_to`` > 0 chooses ``erc_<base>_cap``, which takes it last."""
    if t_dev is not None:
        if args[lengths_at] is not None or args[lengths_at + 1] is not None:
            raise ErcGraftError("%s: t_dev is the unpacked padded-row form (lengths=None, node_off=None)" % base)
        args = args[:lengths_at] + args[lengths_at + 2:]
        _call("erc_%s_tcap" % base, *args[:t_at], t_dev, *args[t_at:])
    elif zero_to:
        _call("erc_%s_cap" % base, *args, zero_to)
    else:
        _call("erc_" + base, *args)


def lstm_scan_fwd(GX, ldgx, W_hh, b_hh, lengths, node_off, sb, st, B, T, Hout, ldh, Hdrop, ldhd, drop_p, rng,
                  rng_stream, gates, Cst, Hprev, t_dev=None):
    """``t_dev`` (device int32; unpacked padded rows): T is a capacity, *t_dev steps run (erc_lstm_scan_fwd_tcap, ercgraft.h)"""
    _scan("lstm_scan_fwd", (GX, ldgx, W_hh, b_hh, lengths, node_off, sb, st, B, T, Hout, ldh, Hdrop, ldhd, drop_p, rng, rng_stream,
                            gates, Cst, Hprev), 4, 8, t_dev)


def lstm_scan_bwd(W_hh, lengths, node_off, sb, st, B, T, gates, Cst, dHout, lddh, drop_p, rng, rng_stream, dGX, zero_to=0,
                  t_dev=None):
    """``zero_to`` > 0 (compact rows): dGX rows [node_off[B], zero_to) are written 0 too (capacity mode); ``t_dev`` (unpacked
    padded rows): *t_dev steps run, dGX rows t >= *t_dev are written 0 (erc_lstm_scan_bwd_tcap)"""
    _scan("lstm_scan_bwd", (W_hh, lengths, node_off, sb, st, B, T, gates, Cst, dHout, lddh, drop_p, rng, rng_stream, dGX), 1, 5,
          t_dev, zero_to)


def gru100_scan_fwd(GX, ldgx, W_hh, b_hh, lengths, node_off, sb, st, B, T, Hout, ldh, Hdrop, ldhd, drop_p, rng,
                    rng_stream, gates, ghn, Hprev, t_dev=None):
    """hidden-100 weight-stationary GRU scan, one layer x both directions (csrc/gru100.hip; ercgraft.h); ``t_dev`` as
    lstm_scan_fwd (erc_gru100_scan_fwd_tcap)"""
    _scan("gru100_scan_fwd", (GX, ldgx, W_hh, b_hh, lengths, node_off, sb, st, B, T, Hout, ldh, Hdrop, ldhd, drop_p, rng,
                              rng_stream, gates, ghn, Hprev), 4, 8, t_dev)


def gru100_scan_bwd(W_hh, lengths, node_off, sb, st, B, T, gates, ghn, Hprev, dHout, lddh, drop_p, rng, rng_stream, dGX, dGH,
                    t_dev=None):
    """``t_dev`` as lstm_scan_bwd: dGX / dGH rows t >= *t_dev are written 0 (erc_gru100_scan_bwd_tcap)"""
    _scan("gru100_scan_bwd", (W_hh, lengths, node_off, sb, st, B, T, gates, ghn, Hprev, dHout, lddh, drop_p, rng, rng_stream, dGX,
                              dGH), 1, 5, t_dev)


def gather_rows(src, lds, map_, N, F, dst, ldd, scatter=0):
    _call("erc_gather_rows", src, lds, map_, N, F, dst, ldd, scatter)


def edge_att_fwd(x, ldx, att, lda, F, N, g, norm):
    _call("erc_edge_att_fwd", x, ldx, att, lda, F, N, g["out_ptr"], g["out_dst"], g["out_eid"], norm)


def edge_att_bwd(x, ldx, att, lda, F, N, g, norm, dnorm, dx, lddx, accumulate_dx, datt, ldda, dscore, dn_parts=1, dn_stride=0):
    """dn_parts > 1: dnorm holds that many partial vectors, dn_stride floats apart (erc_brgcn_bwd_edges_tile's slabs)"""
    _call("erc_edge_att_bwd_parts", x, ldx, att, lda, F, N, g["in_ptr"], g["in_src"], g["out_ptr"], g["out_dst"], g["out_eid"],
          norm, dnorm, dn_parts, dn_stride, dx, lddx, accumulate_dx, datt, ldda, dscore)


def edge_att_bwd_fused(x, ldx, att, lda, F, N, g, norm, dnorm, dx, lddx, accumulate_dx, datt, ldda, dscore, dn_parts=1, dn_stride=0,
                       dx_slabs=None, n_dx_slabs=0, dx_slab_stride=0, rs_TT=None, rs_datt=None, rs_R=0):
    """edge_att_bwd + (dx_slabs) the slab sum of erc_brgcn_bwd_source_tile into dx + (rs_TT) the relation sums d att of
    erc_brgcn_bwd_edges_tile(datt=None), all inside the source-side launch"""
    _call("erc_edge_att_bwd_fused", x, ldx, att, lda, F, N, g["in_ptr"], g["in_src"], g["out_ptr"], g["out_dst"], g["out_eid"],
          norm, dnorm, dn_parts, dn_stride, dx, lddx, accumulate_dx, datt, ldda, dscore, dx_slabs, n_dx_slabs,
          int(dx_slab_stride), rs_TT, g["in_typ"], g["counts"], rs_datt, rs_R)


def brgcn_agg_fwd(x, ldx, F, N, g, norm, att, nb, Z):
    _call("erc_brgcn_agg_fwd", x, ldx, F, N, g["in_ptr"], g["in_src"], g["in_typ"], norm, att, nb, Z)


def brgcn_bwd_edges(x, ldx, F, N, R, g, norm, att, nb, dZ, dnorm, TT, datt):
    _call("erc_brgcn_bwd_edges", x, ldx, F, N, R, g["in_ptr"], g["in_src"], g["in_typ"], g["counts"], norm, att, nb, dZ, dnorm,
          TT, datt)


def brgcn_bwd_source(dH, lddh, O, N, g, norm, att, nb, U):
    _call("erc_brgcn_bwd_source", dH, lddh, O, N, g["out_ptr"], g["out_dst"], g["out_typ"], g["out_eid"], norm, att, nb, U)


def brgcn_set_stamps(t):
    _call("erc_brgcn_set_stamps", t)


def brgcn_bwd_source_tile(dH, lddh, F, O, N, g, norm, att, nb, basis, root, slabs):
    _call("erc_brgcn_bwd_source_tile", dH, lddh, F, O, N, g["out_ptr"], g["out_dst"], g["out_typ"], g["out_eid"], norm, att, nb,
          basis, root, slabs)


def brgcn_bwd_edges_tile(x, ldx, F, O, N, R, g, norm, att, nb, basis, dH, lddh, TT, dn_slabs, dn_stride, datt):
    _call("erc_brgcn_bwd_edges_tile", x, ldx, F, O, N, R, g["in_ptr"], g["in_src"], g["in_typ"], g["counts"], norm, att, nb,
          basis, dH, lddh, TT, dn_slabs, dn_stride, datt)


def brgcn_fwd_tile_slabs():
    return int(lib().erc_brgcn_fwd_tile_slabs())


def brgcn_fwd_tile_slab_floats(n):
    return int(lib().erc_brgcn_fwd_tile_slab_floats(n))


def brgcn_fwd_tile(x, ldx, F, O, N, g, norm, att, nb, basis, root, Z, slabs):
    _call("erc_brgcn_fwd_tile", x, ldx, F, O, N, g["in_ptr"], g["in_src"], g["in_typ"], norm, att, nb, basis, root, Z, slabs)


def rrgcn_max_relations():
    return int(lib().erc_rrgcn_max_relations())


def basis_compose(comp, basis, R, nb, F, O, Wr, WrT):
    _call("erc_basis_compose", comp, basis, R, nb, F, O, Wr, WrT)


def basis_decompose(comp, basis, dWr, R, nb, FO, dbasis, dcomp):
    _call("erc_basis_decompose", comp, basis, dWr, R, nb, FO, dbasis, dcomp)


def rrgcn_agg_fwd(x, ldx, F, N, R, g, norm, Z):
    _call("erc_rrgcn_agg_fwd", x, ldx, F, N, R, g["in_ptr"], g["in_src"], g["in_typ"], norm, Z)


def rrgcn_bwd_edges(x, ldx, F, N, R, g, dZ, dnorm):
    _call("erc_rrgcn_bwd_edges", x, ldx, F, N, R, g["in_ptr"], g["in_src"], g["in_typ"], dZ, dnorm)


def rrgcn_bwd_source(dH, lddh, O, N, R, g, norm, U):
    _call("erc_rrgcn_bwd_source", dH, lddh, O, N, R, g["out_ptr"], g["out_dst"], g["out_typ"], g["out_eid"], norm, U)


def transpose_batched(inp, nb, rows, cols, out):
    _call("erc_transpose_batched", inp, nb, rows, cols, out)


def csr_sum(x, ldx, F, N, ptr_, idx, out, ldo, accumulate=0):
    _call("erc_csr_sum", x, ldx, F, N, ptr_, idx, out, ldo, accumulate)


def gemm_grouped(form, A, lda, B, ldb, Cm, ldc, n_or_k, node_off, n_dlg, n_mod, n_nodes, max_len, pitch, accumulate=0,
                 act=0, aux=None, ldaux=0, act_scale=1.0, cross=None, planes=1, a_plane=0, b_plane=0, split=1, c_slab=0):
    _call("erc_gemm_f32_grouped", form, A, lda, B, ldb, Cm, ldc, n_or_k, node_off, n_dlg, n_mod, n_nodes, max_len, pitch,
          accumulate, act, aux, ldaux, act_scale, cross, planes, a_plane, b_plane, split, c_slab)


def gemm_f32_planes(A, lda, a_plane, B, ldb, b_plane, Cm, ldc, M, N, K, planes, split_k=1, c_slab=0, accumulate=0):
    _call("erc_gemm_f32_planes", A, lda, a_plane, B, ldb, b_plane, Cm, ldc, M, N, K, planes, split_k, c_slab, accumulate)


def gcnii_chain_set_stamps(stamps):
    _call("erc_gcnii_chain_set_stamps", stamps)


def poison_lds():
    """Test support: NaN bit patterns into the LDS of every CU (see include/ercgraft.h)."""
    _call("erc_test_poison_lds", None)


def mm_meta(lengths, qmask, q_st, q_sb, S, B, node_off, node_row, node_dlg, node_spk):
    _call("erc_mm_meta", lengths, qmask, q_st, q_sb, S, B, node_off, node_row, node_dlg, node_spk)


def mm_flatten(src, lds, row_map, emb, spk, N, dst, ldd):
    _call("erc_mm_flatten", src, lds, row_map, emb, spk, N, dst, ldd)


def mm_emb_grad_ws_floats(S):
    return int(lib().erc_mm_emb_grad_ws_floats(S))


def mm_emb_grad(dl, ld, spk, N, S, demb, ws):
    _call("erc_mm_emb_grad", dl, ld, spk, N, S, demb, ws)


def mm_row_normalize(x, R, xhat, inv):
    _call("erc_mm_row_normalize", x, R, xhat, inv)


def mm_row_normalize_bwd(xhat, inv, dxhat, R, dx):
    _call("erc_mm_row_normalize_bwd", xhat, inv, dxhat, R, dx)


def mm_adj_finish(COS, xhat, node_off, B, M, N, P, ADJ, CR, CCOS, DEG):
    _call("erc_mm_adj_finish", COS, xhat, node_off, B, M, N, P, ADJ, CR, CCOS, DEG)


def mm_adj_finish_bwd(COS, CCOS, DEG, dADJ, dCR, node_off, B, M, N, P, G, GC, DD):
    _call("erc_mm_adj_finish_bwd", COS, CCOS, DEG, dADJ, dCR, node_off, B, M, N, P, G, GC, DD)


def mm_cross_apply(CR, h, ldh, node_dlg, node_off, M, N, P, out, ldo):
    _call("erc_mm_cross_apply", CR, h, ldh, node_dlg, node_off, M, N, P, out, ldo)


def mm_cross_grad(dhi, ldd, h, ldh, node_dlg, node_off, M, N, P, dCR, planes=1, d_plane=0, h_plane=0):
    _call("erc_mm_cross_grad", dhi, ldd, h, ldh, node_dlg, node_off, M, N, P, dCR, planes, d_plane, h_plane)


def gcnii_combine_fwd(G, hi, h0, n, theta, alpha, drop_p, rng, rng_stream, hd):
    _call("erc_gcnii_combine_fwd", G, hi, h0, n, theta, alpha, drop_p, rng, rng_stream, hd)


def gcnii_combine_bwd(d_hd, hd, n, theta, alpha, keep_scale, plain, dG, dhi, dh0, F=0, ld_d=0):
    _call("erc_gcnii_combine_bwd", d_hd, hd, n, theta, alpha, keep_scale, plain, dG, dhi, dh0, F, ld_d)


def gcnii_layer_fwd(hih0, lda, W, ldw, theta, alpha, drop_p, rng, rng_stream, hd, ldo, rows, F):
    _call("erc_gcnii_layer_fwd", hih0, lda, W, ldw, theta, alpha, drop_p, rng, rng_stream, hd, ldo, rows, F)


def dropout_fwd(x, n, drop_p, rng, rng_stream, y):
    _call("erc_dropout_fwd", x, n, drop_p, rng, rng_stream, y)


def mm_regroup_fwd(xd, hl, M, N, drop_p, rng, rng_stream, FE):
    _call("erc_mm_regroup_fwd", xd, hl, M, N, drop_p, rng, rng_stream, FE)


def mm_regroup_bwd(dFE, FE, M, N, keep_scale, d_xd, d_h):
    _call("erc_mm_regroup_bwd", dFE, FE, M, N, keep_scale, d_xd, d_h)


def axpy_mask(x, mask, n, scale, accumulate, y):
    _call("erc_axpy_mask", x, mask, n, scale, accumulate, y)


# -- MMGCN in capacity mode (ercgraft.h): n_dev is the device int32 node count, n_cap the capacity the launch is sized for
def mm_meta_cap(lengths, qmask, q_st, q_sb, S, desc, store_spk, store_label, zero_store_row, B, T, n_cap, node_off, node_row,
                node_pad, node_dlg, node_spk, pad_node, x_row, label_out, counts):
    """bucket form (lengths + padded qmask) or resident form (desc + the store's speaker ids [+ labels])"""
    _call("erc_mm_meta_cap", lengths, qmask, q_st, q_sb, S, desc, store_spk, store_label, zero_store_row, B, T, n_cap, node_off,
          node_row, node_pad, node_dlg, node_spk, pad_node, x_row, label_out, counts)


def mm_flatten_cap(src, lds, row_map, emb, spk, n_cap, n_dev, dst, ldd):
    _call("erc_mm_flatten_cap", src, lds, row_map, emb, spk, n_cap, n_dev, dst, ldd)


def mm_emb_grad_cap(dl, ld, spk, n_cap, n_dev, S, demb, ws):
    _call("erc_mm_emb_grad_cap", dl, ld, spk, n_cap, n_dev, S, demb, ws)


def mm_row_normalize_cap(x, n_mod, n_cap, n_dev, xhat, inv):
    _call("erc_mm_row_normalize_cap", x, n_mod, n_cap, n_dev, xhat, inv)


def mm_row_normalize_bwd_cap(xhat, inv, dxhat, n_mod, n_cap, n_dev, dx):
    _call("erc_mm_row_normalize_bwd_cap", xhat, inv, dxhat, n_mod, n_cap, n_dev, dx)


def mm_cross_apply_cap(CR, h, ldh, node_dlg, node_off, M, n_cap, n_dev, P, out, ldo):
    _call("erc_mm_cross_apply_cap", CR, h, ldh, node_dlg, node_off, M, n_cap, n_dev, P, out, ldo)


def mm_cross_grad_cap(dhi, ldd, h, ldh, node_dlg, node_off, M, n_cap, n_dev, P, dCR, planes=1, d_plane=0, h_plane=0):
    _call("erc_mm_cross_grad_cap", dhi, ldd, h, ldh, node_dlg, node_off, M, n_cap, n_dev, P, dCR, planes, d_plane, h_plane)


def gcnii_combine_bwd_cap(d_hd, hd, n_mod, n_cap, n_dev, theta, alpha, keep_scale, plain, dG, dhi, dh0, F, ld_d=0):
    _call("erc_gcnii_combine_bwd_cap", d_hd, hd, n_mod, n_cap, n_dev, theta, alpha, keep_scale, plain, dG, dhi, dh0, F, ld_d)


def dropout_fwd_cap(x, n_mod, n_cap, n_dev, row_w, drop_p, rng, rng_stream, y):
    _call("erc_dropout_fwd_cap", x, n_mod, n_cap, n_dev, row_w, drop_p, rng, rng_stream, y)


def mm_regroup_fwd_cap(xd, hl, M, n_cap, n_dev, drop_p, rng, rng_stream, FE):
    _call("erc_mm_regroup_fwd_cap", xd, hl, M, n_cap, n_dev, drop_p, rng, rng_stream, FE)


def mm_regroup_bwd_cap(dFE, FE, M, n_cap, n_dev, keep_scale, d_xd, d_h):
    _call("erc_mm_regroup_bwd_cap", dFE, FE, M, n_cap, n_dev, keep_scale, d_xd, d_h)


def axpy_mask_cap(x, mask, n_mod, n_cap, n_dev, row_w, scale, accumulate, y):
    _call("erc_axpy_mask_cap", x, mask, n_mod, n_cap, n_dev, row_w, scale, accumulate, y)


def mm_zero_tail(buf, ld, width, n_mod, n_cap, n_dev):
    _call("erc_mm_zero_tail", buf, ld, width, n_mod, n_cap, n_dev)


def clock_probe(out, iters):
    _call("erc_clock_probe", out, iters)


def wgrad_table_x3(table, n_desc, item_base, n_items, slabs, counters):
    """erc_wgrad_table with the three-term bf16 split for records of mode 2"""
    _call("erc_wgrad_table_x3", table, n_desc, item_base, n_items, slabs, counters)


def wgrad_table(table, n_desc, item_base, n_items, slabs, counters):
    """item_base: ctypes int32 array (host) with the first work item of every descriptor."""
    _call("erc_wgrad_table", table, n_desc, item_base, n_items, slabs, counters)


def bn_batch_stats_ws_floats(F):
    return int(lib().erc_bn_batch_stats_ws_floats(F))


def bn_batch_stats(x, ldx, N, F, running_mean, running_var, momentum, eps, saved, ws):
    _call("erc_bn_batch_stats", x, ldx, N, F, running_mean, running_var, float(momentum), float(eps), saved, ws)


def head_fused_ws_floats(n_rows):
    return int(lib().erc_head_fused_ws_floats(n_rows))


def head_fused(H2, ldh, n_rows, F, C, gamma, beta, saved, slope, W0, b0, W3, b3, labels, weight, drop_p, rng_state,
               H3, Z, logits, dlogits, dZ, dY, bn_bwd, dgamma, dbeta, stats, ws, bf16_out=None, n_dev=None, label_rows=None, lddl=0):
    """bf16_out: (H3b, Zb, dZb, dlb, pitch) -- bf16 copies of the classifier's weight-gradient operands, or None; lddl: row pitch
    of dlogits (0 = C)"""
    b = bf16_out if bf16_out is not None else (None, None, None, None, 0)
    _call("erc_head_fused", H2, ldh, n_rows, F, C, gamma, beta, saved, float(slope), W0, b0, W3, b3, labels, weight,
          float(drop_p), rng_state, H3, Z, logits, dlogits, dZ, dY, bn_bwd, dgamma, dbeta, stats, ws, b[0], b[1], b[2], b[3], b[4],
          n_dev, label_rows, int(lddl))


def head_fused_bn(H2, ldh, n_rows, F, C, gamma, beta, saved, slope, W0, b0, W3, b3, labels, weight, drop_p, rng_state,
                  H3, Z, logits, dlogits, dZ, dY, bn_bwd, dgamma, dbeta, stats, ws, bn_part, bn_tiles, running_mean,
                  running_var, momentum, eps, defer_reduce=False, bf16_out=None, n_dev=None, label_rows=None, lddl=0):
    b = bf16_out if bf16_out is not None else (None, None, None, None, 0)
    _call("erc_head_fused_bn", H2, ldh, n_rows, F, C, gamma, beta, saved, float(slope), W0, b0, W3, b3, labels, weight,
          float(drop_p), rng_state, H3, Z, logits, dlogits, dZ, dY, bn_bwd, dgamma, dbeta, stats, ws, bn_part, bn_tiles,
          running_mean, running_var, float(momentum), float(eps), int(defer_reduce), b[0], b[1], b[2], b[3], b[4], n_dev,
          label_rows, int(lddl))


def head_eval(H2, ldh, n_rows, F, C, gamma, beta, running_mean, running_var, eps, slope, W0, b0, W3, b3, labels, cm, logits=None,
              n_dev=None, label_rows=None):
    """eval-mode head scored on the device: cm int64 [C, C] (true x predicted) is added to (erc_head_eval, ercgraft.h)"""
    if cm.dtype != torch.int64 or cm.numel() != C * C or not cm.is_contiguous():
        raise ErcGraftError("head_eval: cm must be a contiguous int64 [%d, %d] tensor" % (C, C))
    _call("erc_head_eval", H2, ldh, n_rows, F, C, gamma, beta, running_mean, running_var, float(eps), float(slope), W0, b0, W3, b3,
          labels, label_rows, n_dev, cm, logits)


def head_fused_rows_per_workgroup(n_rows):
    return int(lib().erc_head_fused_rows_per_workgroup(int(n_rows)))


def head_fused_part_floats():
    return int(lib().erc_head_fused_part_floats())


def bn_bwd_apply(x, ldx, N, F, gamma, saved, bn_bwd, dY, lddy, dx, lddx):
    _call("erc_bn_bwd_apply", x, ldx, N, F, gamma, saved, bn_bwd, dY, lddy, dx, lddx)


def enc_to_bf16(x, n, y):
    _call("erc_enc_to_bf16", x, n, y)


def enc_gemm_bf16(A, lda, W, ldw, bias, C_f32, C_bf16, ldc, M, N, K, relu=0):
    _call("erc_enc_gemm_bf16", A, lda, W, ldw, bias, C_f32, C_bf16, ldc, M, N, K, relu)


def enc_attention(qkv, n_seq, S, D, heads, out):
    _call("erc_enc_attention", qkv, n_seq, S, D, heads, out)


def enc_add_layernorm(a, b, D, n_rows, gamma, beta, eps, y_f32, y_bf16):
    _call("erc_enc_add_layernorm", a, b, D, n_rows, gamma, beta, float(eps), y_f32, y_bf16)


def enc_gemm_bf16_ex(A, lda, W, ldw, bias, C_f32, C_bf16, ldc, M, N, K, relu=0, epilogue=0, mask_src=None, ld_mask=0,
                     scale=1.0, drop_p=0.0, rng_state=None, rng_stream=0):
    _call("erc_enc_gemm_bf16_ex", A, lda, W, ldw, bias, C_f32, C_bf16, ldc, M, N, K, relu, epilogue, mask_src, ld_mask,
          float(scale), float(drop_p), rng_state, rng_stream)


def enc_attention_train(qkv, n_seq, S, D, heads, lengths, drop_p, rng_state, rng_stream, out):
    _call("erc_enc_attention_train", qkv, n_seq, S, D, heads, lengths, float(drop_p), rng_state, rng_stream, out)


def enc_attention_bwd(qkv, dout, n_seq, S, D, heads, lengths, drop_p, rng_state, rng_stream, dqkv):
    _call("erc_enc_attention_bwd", qkv, dout, n_seq, S, D, heads, lengths, float(drop_p), rng_state, rng_stream, dqkv)


def enc_add_layernorm_train(a, b, D, n_rows, gamma, beta, eps, drop_p, rng_state, rng_stream, y_f32, y_bf16, saved_sum,
                            saved_stats):
    _call("erc_enc_add_layernorm_train", a, b, D, n_rows, gamma, beta, float(eps), float(drop_p), rng_state, rng_stream,
          y_f32, y_bf16, saved_sum, saved_stats)


def enc_layernorm_bwd_blocks(n_rows):
    return int(lib().erc_enc_layernorm_bwd_blocks(n_rows))


def enc_layernorm_bwd(dy_a, dy_a_map, dy_b, saved_sum, saved_stats, gamma, D, n_rows, drop_p, rng_state, rng_stream, ds,
                      db_bf16, partial):
    _call("erc_enc_layernorm_bwd", dy_a, dy_a_map, dy_b, saved_sum, saved_stats, gamma, D, n_rows, float(drop_p), rng_state,
          rng_stream, ds, db_bf16, partial)


def enc_transpose_bf16(X, ldx, R, Cn, YT, ldyt, plain=None, ldp=0):
    _call("erc_enc_transpose_bf16", X, 1 if X.dtype == torch.float32 else 0, ldx, R, Cn, YT, ldyt, plain, ldp)


def enc_colsum_ws_floats(Cn):
    return int(lib().erc_enc_colsum_ws_floats(Cn))


def enc_colsum(X, ldx, R, Cn, out, ws):
    _call("erc_enc_colsum", X, 1 if X.dtype == torch.bfloat16 else 0, ldx, R, Cn, out, ws)


def enc_inverse_rows(node_row, N, inv, n_rows):
    _call("erc_enc_inverse_rows", node_row, N, inv, n_rows)


def wgrad_bf16(table, n_desc, item_base, n_items, slabs, counters, terms=1):
    """item_base: ctypes int32 array (host) of the descriptors' first work items (csrc/wgrad_bf16.hip); terms = 2 | 3: the
    records' operands are fp32, expanded into that many bf16 terms in registers (erc_wgrad_split)"""
    if terms > 1:
        _call("erc_wgrad_split", terms, table, n_desc, item_base, n_items, slabs, counters)
        return
    _call("erc_wgrad_bf16", table, n_desc, item_base, n_items, slabs, counters)


def wgrad_bf16_adam(table, n_desc, item_base, n_items, slabs, counters, n_tiles, p, g, m, v, n, lr, b1, b2, eps, wd, decoupled,
                    grad_scale, state, shadow_table, health, terms=1, p2p_desc=None):
    """erc_wgrad_bf16 (terms > 1: erc_wgrad_split) with the optimizer fused in (ercgraft.h); p2p_desc (an ErcP2P): data
    parallel with the gradient exchange inside the launch (erc_wgrad_adam_p2p; health = the descriptor's health word)"""
    args = (table, n_desc, item_base, n_items, slabs, counters, int(n_tiles), p, g, m, v, n, lr, b1, b2, eps, wd, int(decoupled),
            grad_scale, state) + _shadow(shadow_table)
    if p2p_desc is not None:
        _call("erc_wgrad_adam_p2p", terms, *args, C.addressof(p2p_desc))
    elif terms > 1:
        _call("erc_wgrad_split_adam", terms, *args, health)
    else:
        _call("erc_wgrad_bf16_adam", *args, health)


def wgrad_bf16_wide(table, n_desc, wg_base, n_wgs, slabs, counters):
    """erc_wgrad_bf16 for large K: four neighbouring column tiles per workgroup (ercgraft.h)"""
    _call("erc_wgrad_bf16_wide", table, n_desc, wg_base, n_wgs, slabs, counters)


def wgrad_bf16_set_spin_limit(limit):
    _call("erc_wgrad_bf16_set_spin_limit", int(limit))


def wgrad_bf16_set_stamps(t, item=0):
    _call("erc_wgrad_bf16_set_stamps", t, int(item))


def wgrad_bf16_slab_floats():
    return int(lib().erc_wgrad_bf16_slab_floats())


def wgrad_bf16_max_k_per_split():
    return int(lib().erc_wgrad_bf16_max_k_per_split())


def wgrad_slab_floats():
    return int(lib().erc_wgrad_slab_floats())


def wgrad_max_k_per_split():
    return int(lib().erc_wgrad_max_k_per_split())


def dgcn_tail_limits():
    """(max rows, max window) of erc_dgcn_tail"""
    return int(lib().erc_dgcn_tail_max_rows()), int(lib().erc_dgcn_tail_max_window())


def dgcn_tail_set_stamps(stamps):
    _call("erc_dgcn_tail_set_stamps", stamps)


def dgcn_tail_stats_floats(n_rows):
    return int(lib().erc_dgcn_tail_stats_floats(n_rows))


def dgcn_tail(slabs, n_slabs, slab_stride, rgcn_bias, g, window, W_rel, b_rel, W_root, W1, b1, W2, b2, labels, weight, n_classes,
              n_rows, drop_p, rng, Xc, ldx, Hc, AGG, Zc, logits, dlogits, dZc, dXc, lddx, dAGG, dHc, stats, n_dev=None, label_rows=None):
    """DialogueGCN: RGCN slab sum .. GraphConv .. classifier .. cross entropy .. dXc, dAGG, dHc in one launch (include/ercgraft.h).
    ``n_dev`` (device int32, e.g. g["counts"]): capacity mode, n_rows is the capacity; ``label_rows``: resident label map."""
    args = (slabs, n_slabs, int(slab_stride), rgcn_bias, g["in_ptr"], g["in_src"], window, W_rel, b_rel, W_root, W1, b1, W2, b2,
            labels, weight, n_classes, n_rows, float(drop_p), rng, Xc, ldx, Hc, AGG, Zc, logits, dlogits, dZc, dXc, lddx, dAGG, dHc,
            stats)
    if n_dev is None and label_rows is None:
        _call("erc_dgcn_tail", *args)
    else:
        _call("erc_dgcn_tail_cap", *args, n_dev, label_rows)


def dgcn_tail_eval(slabs, n_slabs, slab_stride, rgcn_bias, g, window, W_rel, b_rel, W_root, W1, b1, W2, b2, labels, n_classes,
                   n_rows, Xc, ldx, cm, logits=None, n_dev=None, label_rows=None):
    """DialogueGCN's tail in eval mode, scored on the device: cm int64 [C, C] (true x predicted) is added to
    (erc_dgcn_tail_eval, ercgraft.h)"""
    if cm.dtype != torch.int64 or cm.numel() != n_classes * n_classes or not cm.is_contiguous():
        raise ErcGraftError("dgcn_tail_eval: cm must be a contiguous int64 [%d, %d] tensor" % (n_classes, n_classes))
    _call("erc_dgcn_tail_eval", slabs, n_slabs, int(slab_stride), rgcn_bias, g["in_ptr"], g["in_src"], window, W_rel, b_rel, W_root,
          W1, b1, W2, b2, labels, label_rows, n_classes, n_rows, n_dev, Xc, ldx, cm, logits)


def head_ce_stats_floats(n_rows):
    return int(lib().erc_head_ce_stats_floats(n_rows))


def head_ce(Z, ldz, F, Cn, n_rows, W, bias, labels, weight, mask_scale, logits, ldl, dlogits, lddl, dZ, lddz, stats, n_dev=None):
    """``n_dev`` (device int32): capacity mode, n_rows is the capacity and the batch its first *n_dev rows (ercgraft.h)"""
    args = (Z, ldz, F, Cn, n_rows, W, bias, labels, weight, float(mask_scale), logits, ldl, dlogits, lddl, dZ, lddz, stats)
    if n_dev is None:
        _call("erc_head_ce", *args)
    else:
        _call("erc_head_ce_cap", *args, n_dev)


# --------------------------------------------------------------------------- CIM (csrc/gru.hip, csrc/cim_attn.hip)
def cim_meta(lengths, B, T, n_cap, node_off, node_row):
    _call("erc_cim_meta", lengths, B, T, n_cap, node_off, node_row)


def gru_scan_fwd(GX, W_hhT, b_hh, lengths, node_off, B, T, rows, Hout, Hdrop, drop_p, rng, rng_stream, gates, ghn, Hprev):
    _call("erc_gru_scan_fwd", GX, W_hhT, b_hh, lengths, node_off, B, T, rows, Hout, Hdrop, drop_p, rng, rng_stream, gates, ghn,
          Hprev)


def gru_scan_bwd(W_hh, lengths, node_off, B, T, rows, gates, ghn, Hprev, dH, drop_p, rng, rng_stream, dGX, dGH):
    _call("erc_gru_scan_bwd", W_hh, lengths, node_off, B, T, rows, gates, ghn, Hprev, dH, drop_p, rng, rng_stream, dGX, dGH)


def cim_meta_cap(lengths, desc, store_label, store_emo, tail_row, B, T, n_cap, node_off, node_row, lengths_out, label_out, emo_out,
                 counts):
    """the tables of a capacity-sized CIM step, from lengths (bucket form) or desc (resident form) (ercgraft.h)"""
    _call("erc_cim_meta_cap", lengths, desc, store_label, store_emo, tail_row, B, T, n_cap, node_off, node_row, lengths_out,
          label_out, emo_out, counts)


def gru_scan_bwd_cap(W_hh, lengths, node_off, B, T, rows, gates, ghn, Hprev, dH, drop_p, rng, rng_stream, dGX, dGH, zero_to):
    """gru_scan_bwd, and rows [node_off[B], zero_to) of dGX / dGH written 0"""
    _call("erc_gru_scan_bwd_cap", W_hh, lengths, node_off, B, T, rows, gates, ghn, Hprev, dH, drop_p, rng, rng_stream, dGX, dGH,
          zero_to)


def cim_max_t():
    return int(lib().erc_cim_max_t())


def cim_attn_fwd(merged, node_off, B, T, Pbuf):
    _call("erc_cim_attn_fwd", merged, node_off, B, T, Pbuf)


def cim_attn_bwd(merged, dmerged, node_off, B, T, Pbuf, mask_scale):
    _call("erc_cim_attn_bwd", merged, dmerged, node_off, B, T, Pbuf, mask_scale)


def ce_bce_multitask(logits, ld, Cn, n_rows, labels, emo_label, lde, w_ce, w_bce, grad_scale, dlogits, lddl, stats):
    """cross entropy on logits[:, :Cn] + 7-way BCE on logits[:, Cn:Cn+7] (ercgraft.h erc_ce_bce_multitask)"""
    if labels.dtype != torch.int64 or emo_label.dtype != torch.int64:
        raise ErcGraftError("ce_bce_multitask: label and emo_label must be int64")
    if labels.numel() < n_rows or emo_label.dim() != 2 or emo_label.shape[0] < n_rows or emo_label.shape[1] < 7 \
            or emo_label.stride(1) != 1 or logits.numel() < (n_rows - 1) * ld + Cn + 7:
        raise ErcGraftError("ce_bce_multitask: operands smaller than %d rows (label %s, emo_label %s)"
                            % (n_rows, tuple(labels.shape), tuple(emo_label.shape)))
    _call("erc_ce_bce_multitask", logits, ld, Cn, n_rows, labels, emo_label, lde, w_ce, w_bce, grad_scale, dlogits, lddl,
          stats)


def ce_bce_multitask_cap(logits, ld, Cn, n_cap, n_dev, labels, emo_label, lde, w_ce, w_bce, grad_scale, dlogits, lddl, stats):
    """ce_bce_multitask over the first *n_dev (device int32) of n_cap rows; dlogits rows beyond are written 0 (ercgraft.h)"""
    if labels.dtype != torch.int64 or emo_label.dtype != torch.int64 or n_dev.dtype != torch.int32:
        raise ErcGraftError("ce_bce_multitask_cap: label and emo_label must be int64, n_dev int32")
    if labels.numel() < n_cap or emo_label.dim() != 2 or emo_label.shape[0] < n_cap or emo_label.shape[1] < 7 \
            or emo_label.stride(1) != 1 or logits.numel() < (n_cap - 1) * ld + Cn + 7:
        raise ErcGraftError("ce_bce_multitask_cap: operands smaller than %d rows (label %s, emo_label %s)"
                            % (n_cap, tuple(labels.shape), tuple(emo_label.shape)))
    _call("erc_ce_bce_multitask_cap", logits, ld, Cn, n_cap, n_dev, labels, emo_label, lde, w_ce, w_bce, grad_scale, dlogits,
          lddl, stats)


# --------------------------------------------------------------------------- conv-emotion DialogueGCN (csrc/dgcnv2_att.hip)
def dgcnv2_max_t():
    return int(lib().erc_dgcnv2_max_t())


def dgcnv2_meta(onehot, S, lengths, B, T, n_cap, spk, node_row):
    _call("erc_dgcnv2_meta", onehot, S, lengths, B, T, n_cap, spk, node_row)


def dgcnv2_edge_att_fwd(S, ldS, g, B, T, wp, wf, norm, t_dev=None):
    """``t_dev`` (device int32): capacity mode, B / T are capacities and the batch's longest dialogue is *t_dev (ercgraft.h)"""
    args = (S, ldS, g["node_off"], B, T, wp, wf, g["out_ptr"], g["out_dst"], g["out_eid"], norm)
    if t_dev is None:
        _call("erc_dgcnv2_edge_att_fwd", *args)
    else:
        _call("erc_dgcnv2_edge_att_fwd_cap", *args, t_dev)


def dgcnv2_edge_att_bwd(S, ldS, g, B, T, wp, wf, dnorm, dS, dn_parts=1, dn_stride=0, t_dev=None):
    """``t_dev``: capacity mode, every row of dS [B * T, 110] is written, rows t >= *t_dev as zeros (ercgraft.h)"""
    args = (S, ldS, g["node_off"], B, T, wp, wf, g["out_ptr"], g["out_dst"], g["out_eid"], dnorm, dn_parts, dn_stride, dS)
    if t_dev is None:
        _call("erc_dgcnv2_edge_att_bwd", *args)
    else:
        _call("erc_dgcnv2_edge_att_bwd_cap", *args, t_dev)


# --------------------------------------------------------------------------- matching attention 'general2' (csrc/match_att.hip)
def match_att_fwd(E, lde, Q, ldq, node_off, B, T, F, A, lda, P, TH):
    _call("erc_match_att_fwd", E, lde, Q, ldq, node_off, B, T, F, A, lda, P, TH)


def match_att_bwd(E, lde, Q, ldq, dA, ldda, node_off, B, T, F, P, TH, DZ, dQ, lddq, dE, ldde, n_cap=0):
    """``n_cap`` > 0: capacity mode, rows [node_off[B], n_cap) of dQ and dE are written 0 (ercgraft.h)"""
    args = (E, lde, Q, ldq, dA, ldda, node_off, B, T, F, P, TH, DZ, dQ, lddq, dE, ldde)
    if n_cap:
        _call("erc_match_att_bwd_cap", *args, n_cap)
    else:
        _call("erc_match_att_bwd", *args)


# --------------------------------------------------------------------------- DialogueRNN (csrc/dialogrnn.hip)
DIALOGRNN_SAVE = {"gates_g": (0, 450), "ghn_g": (450, 150), "g_prev": (600, 150), "g": (750, 150), "g_drop": (900, 150),
                  "c": (1050, 150), "gates_p": (1200, 450), "ghn_p": (1650, 150), "q_prev": (1800, 150), "q": (1950, 150),
                  "q_drop": (2100, 150), "gates_e": (2250, 300), "ghn_e": (2550, 100), "e_prev": (2650, 100), "e": (2750, 100),
                  "e_drop": (2850, 100)}
DIALOGRNN_DREC = {"dgh_g": (0, 450), "dgh_p": (450, 450), "dgi_e": (900, 300), "dgh_e": (1200, 300)}
DIALOGRNN_DREC_ROW = 1500
DIALOGRNN_GXW = 1050


def dialogrnn_max_t():
    return int(lib().erc_dialogrnn_max_t())


def dialogrnn_wt_floats():
    return int(lib().erc_dialogrnn_wt_floats())


def dialogrnn_save_floats(N, B, T):
    return int(lib().erc_dialogrnn_save_floats(N, B, T))


def dialogrnn_planes(buf, N, layout):
    """{name: [2, N, w] view} of the planes of a save / dREC buffer (ercgraft.h)"""
    return {k: buf[o * 2 * N:(o + w) * 2 * N].view(2, N, w) for k, (o, w) in layout.items()}


def dialogrnn_alpha(save, N, B, T):
    o = 2950 * 2 * N
    return save[o:o + 2 * B * T * T].view(2, B, T, T)


def dialogrnn_offsets(offs):
    """host int64[20] of the parameter offsets erc_dialogrnn_* take"""
    if len(offs) != 20:
        raise ErcGraftError("dialogrnn: 20 parameter offsets expected, got %d" % len(offs))
    return (C.c_int64 * 20)(*[int(o) for o in offs])


def dialogrnn_meta(onehot, S, lengths, B, T, n_cap, node_off, node_row, node_spk):
    _call("erc_dialogrnn_meta", onehot, S, lengths, B, T, n_cap, node_off, node_row, node_spk)


def dialogrnn_pack(params, offs, D_m, WT):
    _call("erc_dialogrnn_pack", params, C.addressof(offs), D_m, WT)


def dialogrnn_scan_fwd(GX, ldgx, WT, params, offs, D_m, node_off, node_spk, B, T, S, N, drop_p, drop_rec, rng, rng_stream,
                       emotions, lde, save):
    _call("erc_dialogrnn_scan_fwd", GX, ldgx, WT, params, C.addressof(offs), D_m, node_off, node_spk, B, T, S, N, float(drop_p),
          float(drop_rec), rng, rng_stream, emotions, lde, save)


def dialogrnn_scan_bwd(GX, ldgx, WT, params, offs, D_m, node_off, node_spk, B, T, S, N, drop_p, drop_rec, rng, rng_stream, save,
                       dEmo, ldde, dGX, lddgx, dREC, n_dev=None):
    """``n_dev`` (device int32): capacity form -- N is the capacity, rows [*n_dev, N) of dGX and dREC are written +0 (ercgraft.h)"""
    args = (GX, ldgx, WT, params, C.addressof(offs), D_m, node_off, node_spk, B, T, S, N, float(drop_p), float(drop_rec), rng,
            rng_stream, save, dEmo, ldde, dGX, lddgx, dREC)
    if n_dev is None:
        _call("erc_dialogrnn_scan_bwd", *args)
    else:
        _call("erc_dialogrnn_scan_bwd_cap", *args, n_dev)


def dialogrnn_meta_cap(onehot, S, lengths, desc, store_speaker, store_label, zero_store_row, B, T, n_cap, node_off, node_row,
                       node_spk, label_out, counts):
    """index tables of a DialogueRNN step in capacity mode, bucket form (onehot + lengths) or resident form (desc + the store's
    speaker ids and labels); counts = [n_dev, longest dialogue] (ercgraft.h)"""
    _call("erc_dialogrnn_meta_cap", onehot, S, lengths, desc, store_speaker, store_label, zero_store_row, B, T, n_cap, node_off,
          node_row, node_spk, label_out, counts)


def bcrnn_meta_cap(lengths, desc, store_label, zero_store_row, B, T, n_cap, node_off, node_row, pad_node, x_row, label_out, counts):
    """index tables of a bc-LSTM / bc-GRU step in capacity mode; counts = [n_dev, t_dev] (ercgraft.h)"""
    _call("erc_bcrnn_meta_cap", lengths, desc, store_label, zero_store_row, B, T, n_cap, node_off, node_row, pad_node, x_row,
          label_out, counts)


def log_softmax_rows(x, ldx, Cn, n_rows, y, ldy):
    _call("erc_log_softmax_rows", x, ldx, Cn, n_rows, y, ldy)


# --------------------------------------------------------------------------- launch chain (csrc/launch_chain.hip)
def chain_order(n_nodes, edges):
    """path order of nodes 0 .. n_nodes-1 under ``edges`` [(from, to), ...]; raises unless they form one simple path"""
    ne = len(edges)
    fr, to = (C.c_int32 * max(1, ne))(*[e[0] for e in edges]), (C.c_int32 * max(1, ne))(*[e[1] for e in edges])
    order = (C.c_int32 * max(1, n_nodes))()
    _call("erc_chain_order", n_nodes, ne, C.addressof(fr), C.addressof(to), C.addressof(order))
    return list(order)[:n_nodes]


def chain_build(raw_graph):
    """(chain handle, None), or (0, reason) when the hipGraph_t ``raw_graph`` is not one path of kernel nodes.  The handle
    points INTO the graph: keep the graph alive and free the chain first (ercgraft.h)."""
    handle = int(lib().erc_chain_build(raw_graph))
    return (handle, None) if handle else (0, lib().erc_last_error().decode())


def chain_len(chain):
    n = int(lib().erc_chain_len(chain))
    if n < 0:
        _check(n, "erc_chain_len")
    return n


def set_tile_slices(closed):
    """erc_set_tile_slices: the tile kernels derive their graph slices from the node records (True, the library's default) or read
    the CSR (ercgraft.h)"""
    _call("erc_set_tile_slices", 1 if closed else 0)


def set_store_mode(through):
    """erc_set_store_mode: the step's 16-byte output stores write-through (True, the library's default) or plain (ercgraft.h)"""
    _call("erc_set_store_mode", 1 if through else 0)


def chain_run(chain):
    """the chain's launches, in order, on the current stream"""
    _check(lib().erc_chain_run(chain, stream()), "erc_chain_run")


def chain_free(chain):
    _check(lib().erc_chain_free(chain), "erc_chain_free")


# --------------------------------------------------------------------------- MMIN base model (csrc/lstm128.hip, textcnn.hip, ema.hip)
class ErcLstm128Job(C.Structure):
    """host mirror of ErcLstm128Job (ercgraft.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("GX", "W_hh", "b_hh", "pool", "arg", "gates", "Cst", "Hprev", "dpool", "dGX")] + \
               [(n, C.c_int32) for n in ("B", "T", "ldp", "lddp")]


def lstm128_hidden():
    return int(lib().erc_lstm128_hidden())


def lstm128_max_jobs():
    return int(lib().erc_lstm128_max_jobs())


def lstm128_jobs(jobs):
    """ErcLstm128Job array of ``jobs``: dicts of the struct's fields, tensors (on the GPU) or None for the pointers"""
    arr = (ErcLstm128Job * max(1, len(jobs)))()
    for dst, job in zip(arr, jobs):
        for name, ctype in ErcLstm128Job._fields_:
            v = job.get(name)
            if isinstance(v, torch.Tensor):
                if not v.is_cuda:
                    raise ErcGraftError("lstm128 job: %s must live on the GPU (got a %s tensor)" % (name, v.device))
                v = v.data_ptr()
            setattr(dst, name, v if ctype is C.c_void_p else int(v or 0))
    return arr


def lstm128_pool_fwd(jobs, n_jobs=None):
    """``jobs``: a list of job dicts, or the array lstm128_jobs made of one (a step keeps it: nothing is rebuilt per launch)"""
    arr = jobs if isinstance(jobs, C.Array) else lstm128_jobs(jobs)
    _call("erc_lstm128_pool_fwd", C.addressof(arr), len(jobs) if n_jobs is None else n_jobs)


def lstm128_pool_bwd(jobs, n_jobs=None):
    arr = jobs if isinstance(jobs, C.Array) else lstm128_jobs(jobs)
    _call("erc_lstm128_pool_bwd", C.addressof(arr), len(jobs) if n_jobs is None else n_jobs)


def lstm128_pool_fwd_tcap(jobs, counts, dyn_mask, n_jobs=None):
    """capacity form: the jobs' B / T are capacities, ``counts`` = {B, Ta} int32 on the device, bit i of ``dyn_mask``: job i
    runs counts[1] steps (ercgraft.h)"""
    arr = jobs if isinstance(jobs, C.Array) else lstm128_jobs(jobs)
    _call("erc_lstm128_pool_fwd_tcap", C.addressof(arr), len(jobs) if n_jobs is None else n_jobs, counts, dyn_mask)


def lstm128_pool_bwd_tcap(jobs, counts, dyn_mask, n_jobs=None):
    arr = jobs if isinstance(jobs, C.Array) else lstm128_jobs(jobs)
    _call("erc_lstm128_pool_bwd_tcap", C.addressof(arr), len(jobs) if n_jobs is None else n_jobs, counts, dyn_mask)


def lstm128_prefix_max(Hprev, t_rows, out):
    """out [t_rows, 128]: row t = the max-pool of one sample after t steps, from the Hprev rows of a forward at T = t_rows (ercgraft.h)"""
    for name, x in (("Hprev", Hprev), ("out", out)):
        if x is not None and (x.dtype != torch.float32 or not x.is_contiguous() or x.numel() < max(0, t_rows) * 128):
            raise ErcGraftError("lstm128_prefix_max: %s must be a contiguous float32 tensor of at least %d x 128" % (name, t_rows))
    _call("erc_lstm128_prefix_max", Hprev, t_rows, out)


def mmin_collate_width(modality):
    return int(lib().erc_mmin_collate_width(modality))


def mmin_collate(desc, store_audio, store_visual, store_text, store_label, B_cap, T_cap, frames_max, audio, visual, text, label,
                 counts, masked=False):
    """``store_*``: the split in HBM (audio [n_frames, 130] ragged, visual [n, Tv, 342], text [n, Tt, 1024], label [n]); ``desc``
    int32 [3 B_cap] on the device: frames | first frame row | sample index; writes every element of the five outputs.
    ``masked``: erc_mmin_collate_masked, ``desc`` int32 [4 B_cap] with the slots' keep bits behind the three blocks"""
    entry = "mmin_collate_masked" if masked else "mmin_collate"
    for name, x, dt in (("desc", desc, torch.int32), ("store_label", store_label, torch.int64), ("label", label, torch.int64),
                        ("counts", counts, torch.int32), ("store_audio", store_audio, torch.float32),
                        ("store_visual", store_visual, torch.float32), ("store_text", store_text, torch.float32),
                        ("audio", audio, torch.float32), ("visual", visual, torch.float32), ("text", text, torch.float32)):
        if x is not None and (x.dtype != dt or not x.is_contiguous()):
            raise ErcGraftError("%s: %s must be a contiguous %s tensor" % (entry, name, dt))
    n, Tv, Tt = (int(store_visual.shape[0]), int(store_visual.shape[1]), int(store_text.shape[1])) \
        if store_visual is not None and store_text is not None else (0, 0, 0)
    need = dict(desc=(4 if masked else 3) * B_cap, audio=B_cap * T_cap * 130, visual=B_cap * Tv * 342, text=B_cap * Tt * 1024, label=B_cap, counts=2)
    for name, x in (("desc", desc), ("audio", audio), ("visual", visual), ("text", text), ("label", label), ("counts", counts)):
        if x is not None and B_cap > 0 and T_cap > 0 and x.numel() < need[name]:
            raise ErcGraftError("%s: %s holds %d elements, B_cap=%d T_cap=%d needs %d" % (entry, name, x.numel(), B_cap, T_cap, need[name]))
    _call("erc_" + entry, desc, store_audio, 0 if store_audio is None else int(store_audio.shape[0]), store_visual, store_text,
          store_label, n, Tv, Tt, B_cap, T_cap, frames_max, audio, visual, text, label, counts)


def textcnn_min_t():
    return int(lib().erc_textcnn_min_t())


def textcnn_channels():
    return int(lib().erc_textcnn_channels())


def textcnn_conv_floats(B, T):
    return int(lib().erc_textcnn_conv_floats(B, T))


def textcnn_pool_fwd(x, B, T, D, Ws, bs, conv, pooled, ldp, arg):
    """``Ws`` / ``bs``: the weights [128, k*D] and biases [128] of k = 3, 4, 5; ``conv``: textcnn_conv_floats(B, T) of scratch"""
    if conv.numel() < textcnn_conv_floats(B, T):
        raise ErcGraftError("textcnn_pool_fwd: conv holds %d floats, B=%d T=%d needs %d" % (conv.numel(), B, T, textcnn_conv_floats(B, T)))
    _call("erc_textcnn_pool_fwd", x, B, T, D, *Ws, *bs, conv, pooled, ldp, arg)


def textcnn_pool_bwd(x, B, T, D, pooled, ldp, arg, dpooled, lddp, dWs, dbs):
    _call("erc_textcnn_pool_bwd", x, B, T, D, pooled, ldp, arg, dpooled, lddp, *dWs, *dbs)


def ema_step(ema, p, n, alpha):
    _call("erc_ema_step", ema, p, n, alpha)


# --------------------------------------------------------------------------- MMIN missing-modality model (csrc/resae.hip)
RESAE_LAYERS = 32


class ErcResaeJob(C.Structure):
    """host mirror of ErcResaeJob (ercgraft.h)"""
    _fields_ = [("W", C.c_void_p * RESAE_LAYERS), ("b", C.c_void_p * RESAE_LAYERS)] + \
               [(n, C.c_void_p) for n in ("x", "recon", "latents", "act", "d_recon", "d_latents", "dx", "dY")] + \
               [(n, C.c_int32) for n in ("B", "ldx", "ldr", "ldl", "lddr", "lddl", "lddx", "reserved")]


def resae_input():
    return int(lib().erc_resae_input())


def resae_latent():
    return int(lib().erc_resae_latent())


def resae_max_jobs():
    return int(lib().erc_resae_max_jobs())


def resae_max_blocks():
    return int(lib().erc_resae_max_blocks())


def resae_rows_per_group():
    return int(lib().erc_resae_rows_per_group())


def resae_act_floats(B, n_blocks):
    return int(lib().erc_resae_act_floats(B, n_blocks))


def resae_layer_names(n_blocks):
    """the chain's Linear layers in the kernels' order, as state_dict prefixes of a ResidualAE"""
    names = []
    for i in range(n_blocks):
        names += ["encoder_%d.%d" % (i, k) for k in (0, 2, 4)] + ["decoder_%d.%d" % (i, k) for k in (0, 2, 4)]
    return names + ["transition.0", "transition.2"]


def resae_layer_dims(n_blocks):
    """(out, in) of every layer, in the kernels' order"""
    return [(256, 384), (128, 256), (64, 128), (128, 64), (256, 128), (384, 256)] * n_blocks + [(384, 384), (384, 384)]


def _gpu_ptr(what, name, v):
    if isinstance(v, torch.Tensor):
        if not v.is_cuda:
            raise ErcGraftError("%s: %s must live on the GPU (got a %s tensor)" % (what, name, v.device))
        return v.data_ptr()
    return v


def resae_jobs(jobs):
    """ErcResaeJob array of ``jobs``: dicts of the struct's fields; ``W`` / ``b`` are lists of up to 32 tensors in the chain's
    order, the other pointers tensors (on the GPU) or None"""
    arr = (ErcResaeJob * max(1, len(jobs)))()
    for dst, job in zip(arr, jobs):
        for name, ctype in ErcResaeJob._fields_:
            v = job.get(name)
            if name in ("W", "b"):
                v = list(v or [])
                if len(v) > RESAE_LAYERS:
                    raise ErcGraftError("resae job: %s has %d entries, the chain at most %d" % (name, len(v), RESAE_LAYERS))
                for l in range(RESAE_LAYERS):
                    getattr(dst, name)[l] = _gpu_ptr("resae job", "%s[%d]" % (name, l), v[l]) if l < len(v) else None
            elif ctype is C.c_void_p:
                setattr(dst, name, _gpu_ptr("resae job", name, v))
            else:
                setattr(dst, name, int(v or 0))
    return arr


def resae_fwd(jobs, n_blocks, n_jobs=None):
    """``jobs``: a list of job dicts, or the array resae_jobs made of one (a step keeps it)"""
    arr = jobs if isinstance(jobs, C.Array) else resae_jobs(jobs)
    _call("erc_resae_fwd", C.addressof(arr), len(jobs) if n_jobs is None else n_jobs, n_blocks)


def resae_bwd(jobs, n_blocks, n_jobs=None):
    arr = jobs if isinstance(jobs, C.Array) else resae_jobs(jobs)
    _call("erc_resae_bwd", C.addressof(arr), len(jobs) if n_jobs is None else n_jobs, n_blocks)


def resae_latents(job, n_blocks):
    """the latents of ONE job alone (inference): ``job`` a job dict, or the array resae_jobs made of one"""
    arr = job if isinstance(job, C.Array) else resae_jobs([job])
    _call("erc_resae_latents", C.addressof(arr), n_blocks)


def mmin_miss_max_cond():
    return int(lib().erc_mmin_miss_max_cond())


def mmin_miss_patterns(missing_types):
    """host int32 array of erc_mmin_miss_expand's patterns from rows (visual, text, audio) of 0 / 1, 1 = kept (MISSING_TYPES)"""
    return (C.c_int32 * len(missing_types))(*[int(v) | int(t) << 1 | int(a) << 2 for v, t, a in missing_types])


def mmin_miss_expand(feat, ldf, zfeat, patterns, B, out, ldo):
    """``patterns``: mmin_miss_patterns' array (or None: refused by the library)"""
    _call("erc_mmin_miss_expand", feat, ldf, zfeat, None if patterns is None else C.addressof(patterns),
          0 if patterns is None else len(patterns), B, out, ldo)


def mmin_miss_score(logits, ld, labels, B, n_cond, Cn, cm, loss_sum):
    _call("erc_mmin_miss_score", logits, ld, labels, B, n_cond, Cn, cm, loss_sum)


def mmin_miss_expand_cap(feat, ldf, zaudio, t_rows, zvt, counts, patterns, B_cap, out, ldo):
    """capacity form: block c at row c * B_cap, a removed modality's columns from zaudio[clamp(counts[1], 1, t_rows - 1)] | zvt"""
    _call("erc_mmin_miss_expand_cap", feat, ldf, zaudio, t_rows, zvt, counts, None if patterns is None else C.addressof(patterns),
          0 if patterns is None else len(patterns), B_cap, out, ldo)


def mmin_miss_score_cap(logits, ld, labels, B_cap, counts, n_cond, Cn, cm, loss_sum):
    """capacity form: rows b < clamp(counts[0], 0, B_cap) of every block of B_cap rows"""
    _call("erc_mmin_miss_score_cap", logits, ld, labels, B_cap, counts, n_cond, Cn, cm, loss_sum)


def mse_grad(a, lda, b, ldb, B, n_cols, weight, d, ldd, loss_out):
    """loss_out[0] = mean((a - b)^2); d = weight * 2 (a - b) / (B n_cols)"""
    _call("erc_mse_grad", a, lda, b, ldb, B, n_cols, weight, d, ldd, loss_out)


def mmin_miss_combine(dx0, dx1, dcyc, feat, ldf, B, dfeat, lddf, dtext, lddt, ce_stats, w_mse, w_cyc, stats):
    _call("erc_mmin_miss_combine", dx0, dx1, dcyc, feat, ldf, B, dfeat, lddf, dtext, lddt, ce_stats, w_mse, w_cyc, stats)
