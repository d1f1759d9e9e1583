"""GPU: the two cross-launch record sums of the COGMEN step -- every workgroup of erc_head_fused_bn adds up the forward tile's
BatchNorm records, every workgroup of erc_cogmen_bwd_tile (head_part) the head's records -- through the C ABI, with records this
file writes itself.  A wavefront loads whole records as float4 and takes a contiguous chunk of the list (csrc/record_chunks.h;
the arithmetic alone: tests/test_record_chunks_host.py), so the record counts below hit every chunk boundary of 8 and of 16
wavefronts, empty chunks included, at 16 G and 16 G - 5 rows (a full and a partial last tile).

Record contents
  int       integer values: every sum is exact in any order.  Backward tile: every output bit for bit the float64 sum (and its one
            division) rounded once.  Head: the mean half of ``saved`` bit for bit; rstd and the running statistics go through a
            square root and a float update, so they are held to 2^-23 of the float64 finalisation and, bit for bit, to a launch
            on the same records in another order
  position  record g is nonzero only in slot g mod slots, with value g + 1: a skipped, repeated or shifted (record, slot) changes
            an exact integer
  random    BatchNorm: float32 tile sums of rows at |mean| / std = 0 and 10, held to 2^-23 of the float64 finalisation of those
            records (the bound of tests/test_gpu_head.py); head records: random floats, the sums held to 2^-22 + 2^-45 of the
            absolute sum (the bound of its deferred chain)
The record buffer is allocated for more records than the launch is told about and holds NaN behind them; the outputs must be
finite, and neither the records nor the guard words around the outputs may change.  A second launch on the same workspace and
the capacity form (n_dev) against the exact form are bit-identical."""
import numpy as np
import pytest
import torch

from erc_amd import capi
from tests import head_ref as R
from tests.head_ref import same_bits, untouched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F, C = 100, 6
U = R.U
COUNTS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 33, 124, 125)
SPARE = 3                                   # records behind the list, NaN


@pytest.fixture(autouse=True)
def _default_form_afterwards():
    yield
    capi.set_tile_slices(True)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def nan32(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def rows_of(G):
    return (16 * G, 16 * G - 5)


# ------------------------------------------------------------------------------------------------- record contents
def int_records(G, width, seed):
    return np.random.RandomState(seed).randint(-1000, 1001, (G, width)).astype(np.float32)


def position_records(G, width, slots):
    rec = np.zeros((G, width), np.float32)
    rec[np.arange(G), np.arange(G) % slots] = np.arange(G) + 1.0
    return rec


def with_nan_tail(rec):
    return np.concatenate([rec, np.full((SPARE, rec.shape[1]), np.nan, np.float32)])


# ------------------------------------------------------------------------------------------------- the head
_inputs = {}


def head_inputs(N):
    if N not in _inputs:
        _inputs[N] = R.random_inputs(N, F, C, True, 1000 + N)
    return _inputs[N]


def head_launch(rec, G, n_rows, n_dev=None, ws=None):
    """erc_head_fused_bn (defer_reduce = 1) over n_rows random rows with BatchNorm records ``rec`` [G, 2F] followed by NaN records"""
    n = n_rows if n_dev is None else n_dev
    P = head_inputs(n)
    H2 = np.full((n_rows + 2, F), np.nan, np.float32)
    H2[:n] = P["H2"]
    labels = np.full(n_rows, 99, np.int64)
    labels[:n] = P["labels"]
    part = dev(with_nan_tail(rec))
    part_before = part.clone()
    o = dict(H3=nan32(n_rows + 2, F), Z=nan32(n_rows + 2, F), dZ=nan32(n_rows + 2, F), dlogits=nan32(n_rows + 2, C), logits=nan32(n_rows + 2, C),
             dY=nan32(n_rows + 2, F), bn_bwd=nan32(2 * F), dgamma=nan32(F), dbeta=nan32(F), stats=nan32(4), saved=nan32(2 * F + 4),
             rm=torch.cat([torch.zeros(F, device=DEV), nan32(4)]), rv=torch.cat([torch.ones(F, device=DEV), nan32(4)]))
    if ws is None:
        ws = torch.zeros(capi.head_fused_ws_floats(n_rows), dtype=torch.float32, device=DEV)
    nd = torch.tensor([n_dev, 12345], dtype=torch.int32, device=DEV) if n_dev is not None else None
    rng = torch.tensor(list(R.RNG), dtype=torch.int64, device=DEV)
    capi.head_fused_bn(dev(H2), F, n_rows, F, C, dev(P["gamma"]), dev(P["beta"]), o["saved"], P["slope"], dev(P["W0"]), dev(P["b0"]), dev(P["W3"]),
                       dev(P["b3"]), dev(labels), dev(P["weight"]), 0.5, rng, o["H3"], o["Z"], o["logits"], o["dlogits"], o["dZ"], o["dY"],
                       o["bn_bwd"], o["dgamma"], o["dbeta"], o["stats"], ws, part, G, o["rm"], o["rv"], R.MOMENTUM, R.EPS, defer_reduce=True, n_dev=nd)
    torch.cuda.synchronize()
    assert torch.equal(part.view(torch.int32), part_before.view(torch.int32)), "the records were written"
    got = {k: v.cpu().numpy() for k, v in o.items()}
    got["ws"], got["ws_dev"], got["P"] = ws.cpu().numpy(), ws, P
    return got


def head_check(rec, G, N, got, exact):
    """saved / running statistics against the float64 finalisation of the records; H3 of the first, a middle and the last
    workgroup against the PUBLISHED mean | rstd: every workgroup summed the same thing"""
    tag = (G, N)
    want = R.bn_finalize(rec[:G], N, R.EPS, R.MOMENTUM, np.zeros(F), np.ones(F))
    for k in ("saved", "rm", "rv", "H3", "Z", "dZ", "dY", "logits", "dlogits"):
        live = got[k][:N] if got[k].ndim == 2 else got[k][:-4]
        assert np.isfinite(live).all(), (tag, k, "not finite")
        assert untouched(got[k][N:] if got[k].ndim == 2 else got[k][-4:]), (tag, k, "guard words")
    for k in ("bn_bwd", "dgamma", "dbeta", "stats"):
        assert untouched(got[k]), (tag, k, "written by a deferred launch")
    saved = got["saved"][:2 * F].astype(np.float64)
    assert np.all(np.abs(saved - want["saved"]) <= 2 * U * np.abs(want["saved"])), (tag, "saved", float(np.abs(saved - want["saved"]).max()))
    assert np.all(np.abs(got["rm"][:F] - want["running_mean"]) <= 2 * U * want["scale_mean"]), (tag, "running_mean")
    assert np.all(np.abs(got["rv"][:F] - want["running_var"]) <= 2 * U * np.abs(want["running_var"])), (tag, "running_var")
    if exact:      # an exact sum, one division, one rounding
        assert same_bits(got["saved"][:F], (rec[:G, :F].astype(np.float64).sum(0) / N).astype(np.float32)), (tag, "mean bits")
    P = got["P"]
    mean, rstd = saved[:F], saved[F:]
    tiles = -(-N // 16)
    for t in sorted({0, tiles // 2, tiles - 1}):
        x = P["H2"][16 * t:min(16 * t + 16, N)].astype(np.float64)
        z = (x - mean) * rstd * P["gamma"] + P["beta"]
        h = np.where(z > 0, z, z * np.float64(np.float32(P["slope"])))
        lim = 8 * U * (np.abs(x - mean) * rstd * np.abs(P["gamma"]) + np.abs(P["beta"])) + 1e-30
        err = np.abs(got["H3"][16 * t:16 * t + x.shape[0]] - h)
        assert np.all(err <= lim), (tag, "H3 of workgroup %d against the published statistics" % t, float((err / lim).max()))


@pytest.mark.parametrize("G", COUNTS)
def test_head_sums_the_batchnorm_records(G):
    for N in rows_of(G):
        r = np.random.RandomState(G)
        contents = {"int": int_records(G, 2 * F, G), "position": position_records(G, 2 * F, 2 * F)}
        for ratio in (0, 10):
            contents["random-%d" % ratio] = R.bn_tile_sums((r.randn(N, F) + ratio).astype(np.float32))
            assert contents["random-%d" % ratio].shape == (G, 2 * F)
        for kind, rec in contents.items():
            got = head_launch(rec, G, N)
            head_check(rec, G, N, got, exact=kind in ("int", "position"))
            if kind == "int":      # the same records in another order: other chunks, the same exact sums, the same bits
                perm = head_launch(rec[np.random.RandomState(G + 1).permutation(G)], G, N)
                for k in ("saved", "rm", "rv", "H3", "dY"):
                    assert same_bits(got[k], perm[k]), (G, N, k, "permuted records")
            if kind == "random-10":
                ws_before = got["ws"].copy()
                again = head_launch(rec, G, N, ws=got["ws_dev"])
                for k in ("saved", "rm", "rv", "H3", "Z", "dZ", "dY", "logits", "dlogits"):
                    assert same_bits(got[k], again[k]), (G, N, k, "second launch")
                assert same_bits(ws_before, again["ws"]), (G, N, "workspace after the second launch")
                # capacity form: a grid for 32 more rows, two more (zero) tiles in the list, the count on the device
                cap = head_launch(np.concatenate([rec, np.zeros((2, 2 * F), np.float32)]), G + 2, N + 32, n_dev=N)
                for k in ("saved", "rm", "rv"):
                    assert same_bits(got[k], cap[k]), (G, N, k, "capacity form")
                for k in ("H3", "Z", "dZ", "dY", "logits", "dlogits"):
                    assert same_bits(got[k][:N], cap[k][:N]), (G, N, k, "capacity form")
                    assert untouched(cap[k][N:]), (G, N, k, "capacity form: rows beyond the count")


def test_head_refuses_misaligned_records():
    rec = dev(np.zeros(2 * F * 2 + 2, np.float32))[2:]      # 8 bytes past a 16-byte boundary
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(capi.ErcGraftError, match="16-byte alignment"):
        capi.head_fused_bn(z(18, F), F, 16, F, C, z(F), z(F), z(2 * F), 0.01, z(F, F), z(F), z(C, F), z(C), torch.zeros(16, dtype=torch.int64, device=DEV),
                           None, 0.0, None, z(16, F), z(16, F), z(16, C), z(16, C), z(16, F), z(16, F), z(2 * F), z(F), z(F), z(4), z(4096),
                           rec, 1, z(F), z(F), 0.1, 1e-5)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- the backward tile
def _lengths(N):
    return [50] * (N // 50) + ([N % 50] if N % 50 else [])


DIMS16 = dict(a=4, t=8, v=4)              # 16 feature columns in a block of 32 (the projection launch's smallest K): zero columns behind them
K_PAD = 32
_trainers = {}


def _trainer(compute, n_speakers):
    from erc_amd import cogmen as cg
    from erc_amd.params import ERCParams
    key = (compute, n_speakers)
    if key not in _trainers:
        torch.manual_seed(0)
        p = ERCParams().from_args(["--dataset=iemocap-cogmen-sbert-6", "--compute=" + compute, "--train.batch_size=8"])
        p.hidden_all, p.n_speakers = K_PAD, n_speakers
        _trainers[key] = cg.COGMENTrainer(p, DEV)
    return _trainers[key]


def _batch(lengths, n_speakers):
    from tests.util_cases import cogmen_case_lengths
    b = dict(cogmen_case_lengths(lengths, dims=DIMS16, seed=3, n_speakers=n_speakers)["batch"])
    x = b["input_tensor"]
    b["input_tensor"] = torch.cat([x, x.new_zeros(x.shape[0], x.shape[1], K_PAD - x.shape[2])], dim=2).contiguous()
    if n_speakers == 3:      # every speaker next to every other one: all 18 relation ids of a three-speaker window graph occur
        T = x.shape[1]
        b["speaker_tensor"] = (torch.arange(T) % 3).repeat(x.shape[0], 1).to(b["speaker_tensor"].dtype)
    return b


def _arg(call, key):
    name, args = call
    return args[capi.PROTOS[name][2].index(key)]


def _recorded_backward(form, compute, N, n_speakers=2):
    """one eager training step of N nodes; returns the raw erc_cogmen_bwd_tile call of that step -- replayed below with records,
    counts and outputs of this file.  Two speakers: the step goes through the projection + graph launch, so the node records of
    the closed form exist.  Three speakers: the speaker tensor really holds 0, 1 and 2, the CSR holds relation ids up to 17 (the
    kernels ignore ids >= 8, as the reference's loop over its 8 relations does) and the kernel reads the CSR in either mode."""
    capi.set_tile_slices(form == "closed")
    tr = _trainer(compute, n_speakers)
    batch = tr.prepare_batch(_batch(_lengths(N), n_speakers))
    assert int(batch["label"].shape[0]) == N
    assert sorted(set(batch["speaker_tensor"].reshape(-1).tolist())) == list(range(min(n_speakers, max(_lengths(N)))))
    capi.start_recording()
    tr.train_step(batch)
    rec = capi.stop_recording()
    torch.cuda.synchronize()
    calls = [e for e in rec if e[0].startswith("erc_cogmen_bwd_tile")]
    heads = [e for e in rec if e[0] == "erc_head_fused_bn"]
    assert len(calls) == 1 and len(heads) == 1
    call = calls[0]
    # the step deferred the head's reduction to this launch, for this speaker count, and wrote the node records
    assert _arg(heads[0], "defer_reduce") == 1 and _arg(call, "head_part") and _arg(call, "head_parts") == -(-N // 16)
    assert _arg(call, "n_speakers") == n_speakers and _arg(call, "n_nodes") == N
    assert _arg(call, "node_rec")      # (with three speakers the records are there too: the entry point takes the CSR for the speaker count)
    return call


def bwd_replay(call, rec, G, pitch, n_nodes=None, n_dev=None):
    name, args = call
    names = capi.PROTOS[name][2]
    args = list(args)
    part = dev(with_nan_tail(rec))
    part_before = part.clone()
    o = dict(dgamma=nan32(F + 4), dbeta=nan32(F + 4), stats=nan32(4), bn_bwd=nan32(2 * F + 4))
    sub = dict(head_part=part.data_ptr(), head_parts=G, head_part_floats=pitch, **{k: v.data_ptr() for k, v in o.items()})
    nd = None
    if n_dev is not None:
        nd = torch.tensor([n_dev, 12345], dtype=torch.int32, device=DEV)
        sub["n_dev"] = nd.data_ptr()
    if n_nodes is not None:
        sub["n_nodes"] = n_nodes
    for k, v in sub.items():
        args[names.index(k)] = v
    capi.poison_lds()
    capi.replay((name, tuple(args)))
    torch.cuda.synchronize()
    assert torch.equal(part.view(torch.int32), part_before.view(torch.int32)), "the records were written"
    return {k: v.cpu().numpy() for k, v in o.items()}


def bwd_check(rec, G, N, got, exact, tag):
    for k, n_live in (("dgamma", F), ("dbeta", F), ("bn_bwd", 2 * F), ("stats", 3)):
        assert np.isfinite(got[k][:n_live]).all(), (tag, k, "not finite")
        assert untouched(got[k][n_live:]), (tag, k, "guard words")
    s = rec[:G].astype(np.float64).sum(0)
    absum = np.abs(rec[:G].astype(np.float64)).sum(0)
    wmean = s[226] / G
    want = dict(dbeta=s[:F], dgamma=s[112:112 + F], bn_bwd=np.concatenate([s[:F], s[112:112 + F]]) / N, stats=np.array([s[224] / wmean, s[225], wmean]))
    slack = dict(dbeta=absum[:F], dgamma=absum[112:112 + F], bn_bwd=np.concatenate([absum[:F], absum[112:112 + F]]) / N, stats=np.array([absum[224] / wmean, 0, 0]))
    for k, w in want.items():
        g = got[k][:w.shape[0]]
        if exact:
            assert same_bits(g, w.astype(np.float32)), (tag, k, "bits")
        else:
            assert np.all(np.abs(g - w) <= 2.0 ** -22 * np.abs(w) + 2.0 ** -45 * slack[k]), (tag, k, float(np.abs(g - w).max()))


def head_records(kind, G, pitch, seed):
    if kind == "int":
        rec = int_records(G, pitch, seed)
        rec[:, 226] = 3.0                      # every record carries the same weight sum
    elif kind == "position":
        rec = position_records(G, pitch, 224)
        rec[:, 226] = 1.0
    else:
        r = np.random.RandomState(seed)
        rec = (r.randn(G, pitch) * np.exp(r.uniform(-3, 3, (1, pitch)))).astype(np.float32)
        rec[:, 226] = np.float32(123.456)
    rec[:, 227] = 0.0
    return rec


@pytest.mark.parametrize("form", ["closed", "csr"])
@pytest.mark.parametrize("G", COUNTS)
def test_backward_tile_sums_the_head_records(G, form):
    for N in rows_of(G):
        call = _recorded_backward(form, "bf16", N)
        for pitch in (228, 232, 256):
            for kind in ("int", "position", "random"):
                rec = head_records(kind, G, pitch, 10 * G + pitch)
                got = bwd_replay(call, rec, G, pitch)
                bwd_check(rec, G, N, got, kind != "random", (form, G, N, pitch, kind))
                if kind == "int":
                    perm = bwd_replay(call, rec[np.random.RandomState(G + 1).permutation(G)], G, pitch)
                    for k in got:
                        assert same_bits(got[k], perm[k]), (form, G, N, pitch, k, "permuted records")
                if kind == "random" and pitch == 228:
                    again = bwd_replay(call, rec, G, pitch)
                    for k in got:
                        assert same_bits(got[k], again[k]), (form, G, N, k, "second launch")
                    if N > 16:      # the capacity form: the grid of N nodes, N - 3 on the device, against the exact launch at N - 3
                        cap, ex = bwd_replay(call, rec, G, pitch, n_dev=N - 3), bwd_replay(call, rec, G, pitch, n_nodes=N - 3)
                        bwd_check(rec, G, N - 3, cap, False, (form, G, N, "capacity"))
                        for k in cap:
                            assert same_bits(cap[k], ex[k]), (form, G, N, k, "capacity form")


@pytest.mark.parametrize("compute", ["f32x2", "f32x3"])
@pytest.mark.parametrize("form", ["closed", "csr"])
def test_backward_tile_split_instances(form, compute):
    """the two- and three-term instances of the kernel (fp32-class compute modes) on the counts around the chunk boundaries of 16 wavefronts"""
    for G in (15, 17, 33):
        N = 16 * G - 5
        call = _recorded_backward(form, compute, N)
        for kind in ("int", "position", "random"):
            rec = head_records(kind, G, 228, G)
            bwd_check(rec, G, N, bwd_replay(call, rec, G, 228), kind != "random", (form, compute, G, kind))


def test_backward_tile_on_a_three_speaker_graph():
    """a graph with speakers 0, 1 and 2 (18 relation ids in the CSR, 8 of them used): n_speakers = 3 takes the CSR instance without
    the two-speaker prefix sums, whatever the slice mode"""
    for G in (9, 17, 124):
        for N in rows_of(G):
            call = _recorded_backward("closed", "bf16", N, n_speakers=3)
            for pitch in (228, 256):
                for kind in ("int", "position", "random"):
                    rec = head_records(kind, G, pitch, G + pitch)
                    bwd_check(rec, G, N, bwd_replay(call, rec, G, pitch), kind != "random", ("three speakers", G, N, pitch, kind))


@pytest.mark.parametrize("pitch,offset", [(227, 0), (229, 0), (230, 0), (228, 1), (260, 0)])
def test_backward_tile_refuses_records_it_cannot_load_as_float4(pitch, offset):
    call = _recorded_backward("closed", "bf16", 27)
    name, args = call
    names = capi.PROTOS[name][2]
    args = list(args)
    part = torch.zeros(4 * 260 + 4, device=DEV)[offset:]
    args[names.index("head_part")], args[names.index("head_parts")], args[names.index("head_part_floats")] = part.data_ptr(), 2, pitch
    with pytest.raises(capi.ErcGraftError, match="head record operands"):
        capi.replay((name, tuple(args)))
    torch.cuda.synchronize()
