"""GPU: MMGCN's GCNII chain kernels (csrc/gcnii_chain.hip) through the C ABI, in every launch form, against the float64 chain
of tests/mmgcn_chain_ref.py (the reference formula, not the kernels' re-association).

The launch form is chosen at run time: 16-row or 32-row parts (on the device, from the lengths: RW = 16 when the launch's
dialogues fit the grid with 16-row parts), one launch or several per direction (the host, ``dialogues_per_launch``).  The
tests force each form by LOWERING ``grid_cap`` / ``dialogues_per_launch`` below what erc_gcnii_chain_config returns (never
raising them: every workgroup of a launch must be resident) and assert the form's precondition, computed as chain_launch and
the kernel's work table compute it.

Tolerances: 1e-5 x max|reference| for planes, saves and gradients.  A correct fp32 chain, measured against float64 on the
CPU with torch, is within 1.2e-6 of it on plane 65 (relative to max|h|; lengths 110, 97, 33, 17, 1 and three modalities)
and within 4.2e-7 on dW (lengths 128, 64, 16).  The kernels on an MI355X, all forms alike: planes <= 1.3e-6, saves
<= 1.5e-6, dHout <= 3.3e-6 (the smallest gradient: it has gone back through 64 layers), dW / dADJ / dCR <= 1.6e-6.  One
cross-modal coefficient of one utterance off by 1 % moves the planes by 8e-5 and dW by 3e-5.
The backward follows the kernels' relu pattern (mmgcn_chain_ref ``act``): an output within rounding of zero may take the
other sign in fp32, and then its gradient is entirely different; the test asserts that every such flip sits at
|out| < 1e-5 max|out|.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests.mmgcn_chain_ref import ALPHA, FD, LAMDA, MAXRW, NL, build_adjacency, chain_ref, launches, pre_activations, theta, \
    u_matrix, v_matrix

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KP = 208              # V / VT row pitch (FD padded to 13 groups of 16)
TOL = 1e-5
SENT = 12345.0        # sentinel in pitch slack the kernels must not write


def _capi():
    from erc_amd import capi
    return capi


# ---------------------------------------------------------------------------------------------------------------- cases
CASES = {
    # lengths 1, 15, 16, 17, 31, 32, 33 and 110; enough long dialogues that one launch can be forced to 32-row parts
    "mix3": ((1, 15, 16, 17, 31, 32, 33, 110, 110, 110, 110, 110, 105), 3),
    "mix2": ((33, 110, 1, 17, 104, 31, 110, 16, 110, 32, 110, 15, 110), 2),
    "t128": ((128, 1, 64, 127, 128, 100, 120), 2),
}


@functools.lru_cache(maxsize=None)
def case(name):
    lens, Mo = CASES[name]
    g = torch.Generator().manual_seed(sum(lens) * 7 + Mo)
    B, N, T = len(lens), sum(lens), max(lens)
    P = (T + 3) // 4 * 4
    node_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    feats = [torch.randn(N, FD, generator=g, dtype=torch.float64) + 0.3 for _ in range(Mo)]
    ADJ, CR = build_adjacency(feats, node_off, P)
    stdv = 1.0 / math.sqrt(FD)
    W = (torch.rand(NL, 2 * FD, FD, generator=g) * 2 - 1) * stdv
    h0 = torch.relu(torch.randn(Mo * N, FD, generator=g))
    dHin = torch.randn(Mo * N, FD, generator=g)
    c = dict(name=name, lens=lens, Mo=Mo, B=B, N=N, T=T, P=P, node_off=node_off, ADJ=ADJ.float(), CR=CR.float(), W=W, h0=h0,
             dHin=dHin, refs=[])
    d = lambda t: t.to(DEV).contiguous()
    c["dev"] = dict(ADJ=d(c["ADJ"]), CR=d(c["CR"]), node_off=d(torch.from_numpy(node_off)), h0=d(h0), dHin=d(dHin))
    c["dev"].update(prep(c["dev"], W))
    return c


def prep(dv, W):
    """V, VT (zero pad columns, as the module allocates them), U, Call = h0 U for all layers"""
    capi = _capi()
    w_stride = 2 * FD * FD + 64
    Wb = torch.zeros(NL * w_stride, device=DEV)
    Wb.view(NL, w_stride)[:, :2 * FD * FD] = W.reshape(NL, -1).to(DEV)
    VT, V = torch.zeros(NL + 1, FD, KP, device=DEV), torch.zeros(NL + 1, FD, KP, device=DEV)
    U = torch.zeros(FD, NL * FD, device=DEV)
    capi.gcnii_chain_prep(Wb, w_stride, LAMDA, ALPHA, VT, V, U, None)
    return dict(VT=VT, V=V, U=U, Call=(dv["h0"].double() @ U.double()).float())


def reference(c, act):
    """float64 chain of the case with the given relu pattern; cached per pattern (forms usually agree bit for bit)"""
    for pat, ref in c["refs"]:
        if torch.equal(pat, act):
            return ref
    ref = chain_ref(c["ADJ"], c["CR"], c["node_off"], c["h0"], c["h0"], c["W"], c["Mo"], dHin=c["dHin"], act=act.double())
    ref = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in ref.items()}
    c["refs"].append((act, ref))
    return ref


def run(c, cfg, state=None, drop_p=0.0, rng=None):
    """forward + backward of the case with ``cfg``, outputs with slack in every pitch (hd_plane > Mo N FD, lds > NL FD)"""
    capi = _capi()
    Mo, N, B, T, P, dv = c["Mo"], c["N"], c["B"], c["T"], c["P"], c["dev"]
    R3 = Mo * N
    hd_plane, lds = R3 * FD + 36, NL * FD + 12
    if state is None:
        state = torch.zeros(1 + B + B * Mo * cfg[0], dtype=torch.int32, device=DEV)
    health = torch.zeros(1, dtype=torch.int32, device=DEV)
    HD = torch.full(((NL + 2) * hd_plane + 40,), SENT, device=DEV)
    HD[hd_plane:hd_plane + R3 * FD] = dv["h0"].reshape(-1)
    ZS, DG, DZ = (torch.full((R3, lds), SENT, device=DEV) for _ in range(3))
    ZX = torch.zeros(2, R3, FD, device=DEV)
    dHout = torch.full((R3, FD), SENT, device=DEV)
    capi.poison_lds()
    capi.gcnii_chain_fwd(dv["ADJ"], P, dv["CR"], dv["node_off"], N, Mo, B, T, cfg, dv["VT"], dv["Call"], NL * FD, HD, hd_plane,
                         ZS, lds, ZX, state, drop_p, rng, 2000, health=health)
    torch.cuda.synchronize()
    assert int(health[0]) == 0, "forward raised the health word"
    capi.poison_lds()
    capi.gcnii_chain_bwd(dv["ADJ"], P, dv["CR"], dv["node_off"], N, Mo, B, T, cfg, dv["V"], HD, hd_plane, dv["dHin"], dHout, DG,
                         DZ, lds, ZX, state, drop_p, health=health)
    torch.cuda.synchronize()
    assert int(health[0]) == 0, "backward raised the health word"
    hd = HD[:(NL + 2) * hd_plane].view(NL + 2, hd_plane)
    # untouched slack: plane 0, the tail of every plane, the columns past NL FD of the saves
    assert bool((hd[0] == SENT).all()) and bool((hd[:, R3 * FD:] == SENT).all()) and bool((HD[(NL + 2) * hd_plane:] == SENT).all())
    for t in (ZS, DG, DZ):
        assert bool((t[:, NL * FD:] == SENT).all())
    planes = hd[1:, :R3 * FD].reshape(NL + 1, R3, FD)
    sv = lambda t: t[:, :NL * FD].reshape(R3, NL, FD).transpose(0, 1)
    return dict(planes=planes, ZS=sv(ZS), DG=sv(DG), DZ=sv(DZ), dHout=dHout, state=state)


def _err(got, want):
    got, want = got.double(), want.double()
    return float((got - want).abs().max() / want.abs().max())


def check(c, out, form, keep=None, ks=1.0):
    """every output of ``out`` and the host's post-chain products rebuilt from the saves, against the float64 chain"""
    if keep is None:
        ref = reference(c, (out["planes"][1:] > 0).cpu())
    else:
        ref = chain_ref(c["ADJ"], c["CR"], c["node_off"], c["h0"], c["h0"], c["W"], c["Mo"], dHin=c["dHin"], keep=keep, ks=ks,
                        act=(out["planes"][1:] > 0).cpu().double())
        ref = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in ref.items()}
    assert ref["kink_max"] < 1e-5 * float(ref["planes"].abs().max()), (ref["kinks"], ref["kink_max"])
    Mo, N, lens, off = c["Mo"], c["N"], c["lens"], c["node_off"]
    e = {"planes": _err(out["planes"][1:], ref["planes"][1:]), "ZS": _err(out["ZS"], ref["z"]), "DG": _err(out["DG"], ref["dg"]),
         "DZ": _err(out["DZ"], ref["dz"]), "dHout": _err(out["dHout"], ref["dh1"])}
    # what the host's products after the chain (mmgcn.py, chain backward) make of the saves, in float64
    H, Z, G, D = out["planes"].double(), out["ZS"].double(), out["DG"].double(), out["DZ"].double()
    h0 = c["dev"]["h0"].double()
    th = torch.tensor([theta(l) for l in range(1, NL + 1)], dtype=torch.float64, device=DEV)[:, None, None]
    dW = torch.cat([H[:NL].transpose(1, 2) @ D, h0.t() @ G], dim=1) * th
    e["dW"] = _err(dW, ref["dW"])
    Zr, Gr = Z.transpose(0, 1).reshape(Mo * N, NL * FD), G.transpose(0, 1).reshape(Mo * N, NL * FD)
    dA, dC = torch.zeros_like(ref["dADJ"]), torch.zeros_like(ref["dCR"])
    for b, L in enumerate(lens):
        o = int(off[b])
        for m in range(Mo):
            rm = slice(m * N + o, m * N + o + L)
            dA[b * Mo + m, :L, :L] = Gr[rm] @ Zr[rm].t()
            for n in range(Mo):
                if n != m:
                    dC[b, m * Mo + n, :L] = (Gr[rm] * Zr[n * N + o:n * N + o + L]).sum(1)
    e["dADJ"], e["dCR"] = _err(dA, ref["dADJ"]), _err(dC, ref["dCR"])
    print("chain-err %s %s %s" % (c["name"], form, " ".join("%s=%.2e" % kv for kv in e.items())))
    bad = {k: v for k, v in e.items() if not v < TOL}
    assert not bad, (form, e)
    return ref


def assert_same(a, b):
    for k in ("planes", "ZS", "DG", "DZ", "dHout"):
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------------------ the forms
def forced(c, form):
    """cfg for a form of case c, its launches asserted to be that form; cfg only ever lowers the configuration's grid cap
    and dialogues per launch.  Several launches: the largest dialogues_per_launch that leaves the last launch ragged and
    (32xN) gives a launch with b0 > 0 32-row parts"""
    lens, Mo, T, B = c["lens"], c["Mo"], c["T"], c["B"]
    cfg0 = _capi().gcnii_chain_config(B, T, Mo, c["P"])
    parts, cap0, dpl0 = cfg0
    w32 = Mo * ((T + MAXRW - 1) // MAXRW)                 # a dialogue's workgroups in the worst case (T long, 32-row parts)
    if form == "16x1":
        cands = [cfg0]
    elif form == "32x1":
        cands = [(parts, B * w32, B)]                     # the least cap the host accepts for one launch
    elif form == "16xN":
        cands = [(parts, cap0, d) for d in range(min(B - 1, dpl0), 0, -1) if B % d]
    else:
        cands = [(parts, d * w32, d) for d in range(min(B - 1, dpl0), 0, -1) if B % d]
    want = {"16x1": lambda ls: len(ls) == 1 and ls[0][3] == 16,
            "32x1": lambda ls: len(ls) == 1 and ls[0][3] == 32,
            "16xN": lambda ls: len(ls) > 1 and all(x[3] == 16 for x in ls),
            "32xN": lambda ls: len(ls) > 1 and any(x[3] == 32 and x[0] > 0 for x in ls)}[form]
    for cfg in cands:
        assert cfg[1] <= cap0 and cfg[2] <= dpl0, (cfg, cfg0)
        ls = launches(lens, Mo, T, cfg)
        if want(ls):
            return cfg, ls
    raise AssertionError("case %s has no %s form under %s" % (c["name"], form, cfg0))


FORMS = ["16x1", "32x1", "16xN", "32xN"]


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("form", FORMS)
def test_chain_form_matches_float64(name, form):
    """one launch form on one batch: planes, saves, dHout and the post-chain products vs float64; the same call twice is
    bit-identical"""
    c = case(name)
    cfg, ls = forced(c, form)
    out = run(c, cfg)
    check(c, out, form)
    assert_same(out, run(c, cfg, state=out["state"]))


def test_chain_state_reused_across_forms():
    """one chain_state through 16-row, 32-row, several launches with 32-row parts, 16-row again (a workspace of one shape
    whose batches differ in lengths): every call matches float64"""
    c = case("mix3")
    state = None
    for form in ("16x1", "32x1", "32xN", "16x1"):
        cfg, _ = forced(c, form)
        if state is None:
            state = torch.zeros(1 + c["B"] + c["B"] * c["Mo"] * cfg[0], dtype=torch.int32, device=DEV)
        out = run(c, cfg, state=state)
        check(c, out, "reuse:" + form)


def test_chain_configuration_own_choice_b32_t110():
    """B = 32 dialogues at T = 110 with three modalities: the configuration itself splits the batch (ragged last launch)"""
    lens = tuple([110] + [int(x) for x in np.random.RandomState(3).randint(1, 111, size=31)])
    CASES["b32"] = (lens, 3)
    c = case("b32")
    cfg = _capi().gcnii_chain_config(c["B"], c["T"], 3, c["P"])
    assert cfg[2] < c["B"] and c["B"] % cfg[2] != 0, cfg
    ls = launches(lens, 3, c["T"], cfg)
    assert len(ls) == 2
    check(c, run(c, cfg), "config %s" % (ls,))


def test_chain_prep_matches_float64():
    """erc_gcnii_chain_prep: V, VT, U, UT from the layer weights (w_stride past 2 FD FD) vs the float64 formula; the pad
    columns 200..207 of V / VT (and the spare layer) are not written"""
    capi = _capi()
    g = torch.Generator().manual_seed(5)
    W = (torch.rand(NL, 2 * FD, FD, generator=g) * 2 - 1) / math.sqrt(FD)
    w_stride = 2 * FD * FD + 100
    Wb = torch.full((NL * w_stride,), float("nan"), device=DEV)
    Wb.view(NL, w_stride)[:, :2 * FD * FD] = W.reshape(NL, -1).to(DEV)
    VT, V = torch.full((NL + 1, FD, KP), SENT, device=DEV), torch.full((NL + 1, FD, KP), SENT, device=DEV)
    U, UT = torch.full((FD, NL * FD), SENT, device=DEV), torch.full((NL * FD, FD), SENT, device=DEV)
    capi.gcnii_chain_prep(Wb, w_stride, LAMDA, ALPHA, VT, V, U, UT)
    torch.cuda.synchronize()
    W64 = W.double()
    Vr = torch.stack([v_matrix(W64, l) for l in range(1, NL + 1)])
    Ur = torch.stack([u_matrix(W64, l) for l in range(1, NL + 1)])
    cpu = lambda t: t.double().cpu()
    errs = [float((cpu(V[:NL, :, :FD]) - Vr).abs().max()), float((cpu(VT[:NL, :, :FD]) - Vr.transpose(1, 2)).abs().max()),
            float((cpu(U).view(FD, NL, FD).transpose(0, 1) - Ur).abs().max()),
            float((cpu(UT).view(NL, FD, FD) - Ur.transpose(1, 2)).abs().max())]
    print("chain-err prep V=%.2e VT=%.2e U=%.2e UT=%.2e" % tuple(errs))
    assert max(errs) < 3e-7, errs        # |V|, |U| < 1: a few fp32 ulps (theta itself is computed in fp32)
    for t in (V, VT):
        assert bool((t[:, :, FD:] == SENT).all()) and bool((t[NL] == SENT).all())


def test_chain_dropout_masks_and_backward():
    """p = 0.4 inside the chain: each layer's keep mask, recovered from the kernel's planes where the float64
    pre-activation (from the kernel's own previous plane) is clearly positive, keeps relu(out) / (1 - p), drops a share
    within 5 sigma of p, differs between layers and equals gcnii_layer_fwd's for the same rng state and stream 2000 + l;
    the backward with those masks matches float64"""
    capi = _capi()
    CASES["drop"] = ((1, 17, 33, 64, 110), 3)
    c = case("drop")
    Mo, N, p = c["Mo"], c["N"], 0.4
    R3, ks = Mo * N, 1.0 / (1.0 - p)
    rng = torch.tensor([3, 0x5EED], dtype=torch.int64, device=DEV)
    cfg = capi.gcnii_chain_config(c["B"], c["T"], Mo, c["P"])
    out = run(c, cfg, drop_p=p, rng=rng)
    planes = out["planes"].double().cpu()
    pre = pre_activations(c["ADJ"], c["CR"], c["node_off"], c["h0"], planes[:NL], c["W"], Mo)
    ones, zw = torch.ones(R3, 2 * FD, device=DEV), torch.zeros(2 * FD, FD, device=DEV)
    hd = torch.empty(R3, FD, device=DEV)
    keep, prev, shares = [], None, []
    for l in range(1, NL + 1):
        # gcnii_layer_fwd with W = 0 and hi = h0 = 1: out = 1 - theta > 0 everywhere, so its output shows the keep mask
        capi.gcnii_layer_fwd(ones, 2 * FD, zw, FD, theta(l), ALPHA, p, rng, 2000 + l, hd, FD, R3, FD)
        mask = (hd != 0).cpu()
        keep.append(mask.double())
        o, h = pre[l - 1], planes[l]
        clear = o > 1e-3 * float(o.abs().max())
        got = h[clear] != 0
        assert torch.equal(got, mask[clear]), "layer %d: keep mask differs from gcnii_layer_fwd's" % l
        kept = clear & (h != 0)
        assert float((h[kept] - o[kept] * ks).abs().max()) < TOL * float(h.abs().max()), l
        n = int(clear.sum())
        share = 1.0 - float(got.double().mean())
        shares.append(share)
        assert abs(share - p) < 5 * math.sqrt(p * (1 - p) / n), (l, share, n)
        if prev is not None:
            assert not torch.equal(mask, prev), l
            assert float((mask == prev).double().mean()) < 0.7, l          # independent masks agree on ~p^2 + (1-p)^2 = 0.52
        prev = mask
    print("chain-err drop dropped share %.4f..%.4f" % (min(shares), max(shares)))
    check(c, out, "dropout", keep=torch.stack(keep), ks=ks)

