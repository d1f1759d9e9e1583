"""GPU: the DAG-ERC recurrence kernels (csrc/dag_rec.hip) through the C ABI -- erc_dag_rec_fwd / _bwd in every launch form,
erc_dag_attn_sums, erc_dag_meta -- against the float64 recurrence of tests/dag_rec_ref.py (the reference's formula, not the
kernels' slicing).  Every tensor of the contract in include/ercgraft.h (K6) is compared: H1, GI, GH, Mseq, R, ks, alpha, A,
DGI, DGH, dM, dks, the masked gradient wrt H_0 and the weight gradients formed from the saves as the header says.

The launch form cfg = {epc, dg, groups per launch, layers per launch} is picked at run time per direction; the tests force
each value through erc_dag_rec_config's hints and only ever LOWER groups / layers per launch below what it returned (every
workgroup of a launch must be resident), and assert the form's precondition (launches and layer chunks computed as the
host loops of erc_dag_rec_fwd / _bwd compute them) instead of skipping.

TOLERANCES (see TOL below).  Yardstick: the same reference function in float32 on the CPU (torch, one thread) against its
float64 run, per tensor class as max|x32 - x64| / max|x64|, worst tensor and layer of the class.  The bound is 4 x that,
rounded up to one significant digit, per case and class:
    case    fwd saves, alpha, bwd saves, dH0, contract wgrads: bound (yardstick)
    mix     4e-6 (8.11e-7)  4e-7 (7.65e-8)  3e-6 (6.15e-7)  1e-6 (2.35e-7)  4e-6 (9.07e-7)
    meld    4e-6 (8.03e-7)  3e-7 (7.16e-8)  3e-6 (5.77e-7)  2e-6 (2.55e-7)  3e-6 (6.59e-7)
    mono    3e-6 (6.18e-7)  0 (0)            2e-6 (3.19e-7)  2e-6 (2.54e-7)  2e-6 (3.58e-7)
    t1      9e-7 (2.14e-7)  0 (0)            9e-7 (2.00e-7)  6e-7 (1.38e-7)  1e-6 (2.38e-7)
    t2      2e-6 (2.80e-7)  0 (0)            2e-6 (3.29e-7)  6e-7 (1.48e-7)  2e-6 (3.68e-7)
    t3      2e-6 (4.33e-7)  2e-7 (3.04e-8)  5e-6 (1.13e-6)  7e-7 (1.68e-7)  5e-6 (1.19e-6)
    l5      4e-6 (8.19e-7)  3e-7 (5.56e-8)  2e-6 (4.93e-7)  2e-6 (2.74e-7)  3e-6 (7.50e-7)
    l1      3e-6 (5.53e-7)  3e-7 (5.49e-8)  2e-6 (3.18e-7)  8e-7 (1.86e-7)  2e-6 (4.05e-7)
    b33     4e-6 (8.85e-7)  3e-7 (7.04e-8)  3e-6 (6.29e-7)  2e-6 (2.58e-7)  4e-6 (8.16e-7)
    long    4e-6 (8.13e-7)  3e-7 (6.82e-8)  2e-6 (4.78e-7)  9e-7 (2.13e-7)  5e-6 (1.08e-6)
    limit   4e-6 (7.58e-7)  4e-7 (7.85e-8)  2e-6 (4.09e-7)  1e-6 (2.35e-7)  6e-6 (1.43e-6)
A class whose reference is identically zero (alpha of one-speaker / one-step cases is 1 or absent, its error exactly 0) is
compared absolutely with bound 0.
The kernels on an MI355X (worst form of each case; same columns), within 2.7 x the float32 yardstick (the bound is 4 x):
    mix     3.01e-7  6.76e-8  6.72e-7  3.59e-7  5.91e-7
    l5      3.17e-7  6.36e-8  5.01e-7  3.24e-7  6.07e-7
    meld    4.15e-7  5.59e-8  9.92e-7  4.83e-7  6.13e-7
    mono    2.48e-7  0.00e+00  6.85e-7  5.53e-7  3.75e-7
    t1      2.32e-7  0.00e+00  4.81e-7  3.63e-7  3.97e-7
    t2      5.25e-7  0.00e+00  6.39e-7  2.92e-7  5.53e-7
    t3      2.95e-7  3.04e-8  7.05e-7  3.52e-7  6.18e-7
    l1      2.34e-7  6.18e-8  7.94e-7  3.76e-7  3.75e-7
    b33     3.15e-7  7.22e-8  8.13e-7  5.48e-7  7.40e-7
    long    3.26e-7  6.57e-8  9.62e-7  5.33e-7  5.23e-7
    limit   2.50e-7  7.34e-8  7.32e-7  4.86e-7  4.59e-7
Sensitivity, reference alone on the CPU (float64, relative change of the worst tensor of the class), for (a) one edge of one
utterance taking Wr1 instead of Wr0, (b) one window starting one utterance early, (c) b_hn of cell P outside r * (.):
    (a) mix   fwd=3.05e-1  alpha=6.42e-3  bwd=2.70e-1  dH0=4.95e-2  wgrad=5.82e-2
    (b) mix   fwd=1.54e-1  alpha=2.08e-1  bwd=1.48e-1  dH0=3.60e-2  wgrad=2.98e-2
    (c) mix   fwd=6.40e-2  alpha=1.37e-3  bwd=9.41e-2  dH0=5.39e-3  wgrad=5.67e-1
    (a) meld  fwd=3.40e-1  alpha=6.27e-3  bwd=4.29e-1  dH0=8.71e-2  wgrad=1.32e-1
    (b) meld  fwd=1.38e-1  alpha=1.76e-1  bwd=1.84e-1  dH0=3.22e-2  wgrad=5.00e-2
    (c) meld  fwd=8.45e-2  alpha=9.97e-4  bwd=1.35e-1  dH0=6.34e-3  wgrad=5.87e-1
i.e. every one of them moves every class by more than 1000 x its bound at the weights' init scale.
The file takes 16 s on an MI355X box (half of it the float64 references on the CPU: `long` 4 s, `mix` 2 s, `limit` 2 s).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle.graph import dag_pred_closed_form
from tests.dag_rec_ref import CASES, CLASSES, HID, MAX_T, PARAMS, class_errors, contract_products, make_case, reference, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 12345.0          # sentinel in pitch slack (and in alpha outside the windows) the kernels must not write
ML = 4                  # csrc/dag_rec.hip: layers per launch at most
N_STATE = 1 + 64

# 4 x the float32 yardstick, one significant digit up: (fwd, alpha, bwd, dH0, wgrad)
TOL = {
    "mix": (4e-06, 4e-07, 3e-06, 1e-06, 4e-06),
    "meld": (4e-06, 3e-07, 3e-06, 2e-06, 3e-06),
    "mono": (3e-06, 0.0, 2e-06, 2e-06, 2e-06),
    "t1": (9e-07, 0.0, 9e-07, 6e-07, 1e-06),
    "t2": (2e-06, 0.0, 2e-06, 6e-07, 2e-06),
    "t3": (2e-06, 2e-07, 5e-06, 7e-07, 5e-06),
    "l5": (4e-06, 3e-07, 2e-06, 2e-06, 3e-06),
    "l1": (3e-06, 3e-07, 2e-06, 8e-07, 2e-06),
    "b33": (4e-06, 3e-07, 3e-06, 2e-06, 4e-06),
    "long": (4e-06, 3e-07, 2e-06, 9e-07, 5e-06),
    "limit": (4e-06, 4e-07, 2e-06, 1e-06, 6e-06),
}


def _capi():
    from erc_amd import capi
    return capi


def cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def case(name, variant=0):
    c = make_case(name, variant)
    d = lambda t: t.to(DEV).contiguous()
    c["dev"] = dict(layers=[{k: d(v) for k, v in ly.items()} for ly in c["layers"]], H0=d(c["H0"]).view(-1, HID),
                    dHall=d(c["dHall"]).view(c["B"] * c["T"], -1), spk=d(torch.from_numpy(c["spk"]).int()),
                    pred=d(torch.from_numpy(c["pred"]).int()))
    c["ref"] = reference(c)
    lo, ar = torch.from_numpy(np.maximum(c["pred"], 0)), torch.arange(c["T"])
    c["adj"] = (ar[None, None, :] >= lo[:, :, None]) & (ar[None, None, :] < ar[None, :, None])
    return c


def config(c, direction, epc=0, dg=0, lpl=0):
    return tuple(_capi().dag_rec_config(direction, c["B"], c["T"], c["L"], epc, dg, lpl))


def cfg_arr(cfg):
    return (C.c_int * 4)(*cfg)


def layer_chunks(L, lpl, direction):
    """[l0, l1) of every launch over the layers, in launch order, as erc_dag_rec_fwd / _bwd chunk them"""
    if direction == 0:
        return [(l0, min(l0 + lpl, L)) for l0 in range(0, L, lpl)]
    return [(max(hi - lpl, 0), hi) for hi in range(L, 0, -lpl)]


def launches(c, cfg, direction):
    return len(layer_chunks(c["L"], cfg[3], direction)) * cdiv(cdiv(c["B"], cfg[1]), cfg[2])


def new_scratch(c, *cfgs):
    """(forward, backward) record scratch, zero-filled once, large enough for every (cfg_f, cfg_b) of ``cfgs``"""
    capi = _capi()
    n = [max(capi.dag_rec_scratch_bytes(d, c["B"], c["T"], cfg_arr(pair[d])) for pair in cfgs) for d in (0, 1)]
    assert min(n) > 0
    return [torch.zeros(x // 8 + 1, dtype=torch.int64, device=DEV) for x in n]


def run(c, cfg_f, cfg_b, state=None, scratch=None):
    """forward, attention sums and backward of case c; every pitch has slack (filled with SENT, which must survive), LDS is
    poisoned before each direction, a private health word must stay 0"""
    capi = _capi()
    B, T, L, dv = c["B"], c["T"], c["L"], c["dev"]
    BT, W5 = B * T, HID * (L + 1)
    ldh, ldgi, lddgi, ldd = W5 + 12, 6 * HID + 1 + 11, 6 * HID + 1 + 15, W5 + 8
    if state is None:
        state = torch.zeros(N_STATE, dtype=torch.int32, device=DEV)
    assert cdiv(B, min(cfg_f[1], cfg_b[1])) < N_STATE
    if scratch is None:
        scratch = new_scratch(c, (cfg_f, cfg_b))
    health = torch.zeros(1, dtype=torch.int32, device=DEV)
    full = lambda *s: torch.full(s, SENT, device=DEV)
    Hall, dHall = full(BT, ldh), full(BT, ldd)
    Hall[:, :HID] = dv["H0"]
    dHall[:, :W5] = dv["dHall"]
    per = lambda *s: [full(*s) for _ in range(L)]
    b = dict(GI=per(BT, ldgi), GH=per(BT, 6 * HID), Mseq=per(BT, HID), R=per(BT, 2 * HID), ks=per(BT), alpha=per(B, T, T),
             DGI=per(BT, lddgi), DGH=per(BT, 6 * HID), dM=per(BT, HID), dks=per(BT), A=per(BT, 2 * HID))
    tb = {k: capi.ptr_table([ly[k] for ly in dv["layers"]]) for k in PARAMS}
    tb.update(H1=capi.ptr_table([Hall[:, HID * (l + 1):] for l in range(L)]), Hl=capi.ptr_table([Hall[:, HID * l:] for l in range(L)]),
              **{k: capi.ptr_table(b[k]) for k in ("GI", "Mseq", "GH", "R", "ks", "alpha", "DGI", "DGH", "dM", "dks")})
    capi.poison_lds()
    capi.dag_rec_fwd(Hall, ldh, L, tb, dv["pred"], dv["spk"], B, T, ldh, ldgi, cfg_arr(cfg_f), state, scratch[0], health=health)
    torch.cuda.synchronize()
    assert int(health[0]) == 0, "forward raised the health word"
    for l in range(L):
        capi.dag_attn_sums(b["alpha"][l], Hall[:, HID * (l + 1):], ldh, dv["pred"], dv["spk"], B, T, b["A"][l])
    capi.poison_lds()
    capi.dag_rec_bwd(L, tb, ldh, ldgi, dv["pred"], dv["spk"], B, T, dHall, ldd, lddgi, cfg_arr(cfg_b), state, scratch[1],
                     health=health)
    torch.cuda.synchronize()
    assert int(health[0]) == 0, "backward raised the health word"
    assert int(state[0]) == 0                                       # the private health word was used, not state[0]
    # untouched slack
    assert bool((Hall[:, W5:] == SENT).all()) and bool((dHall[:, W5:] == SENT).all())
    assert torch.equal(Hall[:, :HID], dv["H0"])
    adj = c["adj"].to(DEV)
    out = []
    for l in range(L):
        assert bool((b["GI"][l][:, 6 * HID + 1:] == SENT).all()) and bool((b["DGI"][l][:, 6 * HID + 1:] == SENT).all())
        assert bool((b["alpha"][l][~adj] == SENT).all()), "alpha written outside the windows"
        v3 = lambda t: t.reshape(B, T, -1).cpu()
        o = dict(H1=v3(Hall[:, HID * (l + 1):HID * (l + 2)]), GI=v3(b["GI"][l][:, :6 * HID + 1]), GH=v3(b["GH"][l]),
                 Mseq=v3(b["Mseq"][l]), R=v3(b["R"][l]), ks=b["ks"][l].view(B, T).cpu(),
                 alpha=torch.where(adj, b["alpha"][l], torch.zeros((), device=DEV)).cpu(), A=v3(b["A"][l]),
                 DGI=v3(b["DGI"][l][:, :6 * HID + 1]), DGH=v3(b["DGH"][l]), dM=v3(b["dM"][l]), dks=b["dks"][l].view(B, T).cpu())
        out.append(o)
    out[0]["dH0"] = dHall[:, :HID].view(B, T, HID).cpu()
    return dict(out=out, state=state, scratch=scratch)


WORST = {}


def check(c, res, form):
    """every output of a run, and the weight gradients the header derives from them (formed in float64), vs the reference"""
    out, ref = res["out"], c["ref"]
    Hl = c["H0"]
    for o in out:
        o.update(contract_products(o, Hl))
        Hl = o["H1"]
    e = class_errors(out, ref)
    tol = dict(zip(CLASSES, TOL[c["name"]]))
    print("dag-rec-err %-5s %-28s %s" % (c["name"], form, "  ".join("%s=%.2e" % kv for kv in e.items())))
    w = WORST.setdefault(c["name"], dict.fromkeys(CLASSES, 0.0))
    for k in e:
        w[k] = max(w[k], e[k])
    bad = {}
    for cls in CLASSES:
        if not e[cls] <= tol[cls]:
            bad[cls] = {k: max(rel(g[k], r[k]) for g, r in zip(out, ref) if k in r) for k in CLASSES[cls]}
    assert not bad, (c["name"], form, "per tensor of the failing classes: %s" % bad, "bounds: %s" % tol)


# ------------------------------------------------------------------------------------------------------------ the forms
# (forward epc, dg, layers per launch | backward epc, dg, layers per launch | lower the groups per launch to 1); 0 = the
# configuration's own choice.  Every value of every axis, in both directions: epc 5 / 4 / 2, dg 1 / 3 / 16, layers per launch
# 1 / 2 / 3 / 4 (150 workgroups per group and layer at epc 2 leave room for one layer per launch, 75 at epc 4 for three).
FULL = {
    "default": ((0, 0, 0), (0, 0, 0), False),
    "f5.1.1-b4.3.2": ((5, 1, 1), (4, 3, 2), False),
    "f4.3.2-b2.16.1": ((4, 3, 2), (2, 16, 1), False),
    "f2.16.1-b5.1.4": ((2, 16, 1), (5, 1, 4), False),
    "f5.16.4-b5.3.3": ((5, 16, 4), (5, 3, 3), False),
    "f4.1.3-b4.16.1": ((4, 1, 3), (4, 16, 1), False),
    "f5.3.4-b5.3.4-gpl1": ((5, 3, 4), (5, 3, 4), True),
}


def forced(c, form):
    """(cfg_f, cfg_b) of a form for case c; the hints are clipped to what the case admits (layers, LDS)"""
    hf, hb, gpl1 = form
    cfgs = []
    for d, (epc, dg, lpl) in enumerate((hf, hb)):
        if lpl:
            lpl = min(lpl, c["L"], ML)
        if dg and c["T"] > 200:
            dg = 1                      # the histories of dg dialogues x T steps live in LDS
        cfg = config(c, d, epc, dg, lpl)
        if epc:
            assert cfg[0] == epc and cfg[1] == dg and cfg[3] == lpl, (cfg, form)
        if gpl1:
            cfg = (cfg[0], cfg[1], 1, cfg[3])
        cfgs.append(cfg)
    return cfgs


@pytest.mark.parametrize("form", list(FULL))
@pytest.mark.parametrize("name", ["mix", "l5"])
def test_every_form_matches_float64(name, form):
    c = case(name)
    cfg_f, cfg_b = forced(c, FULL[form])
    B, L = c["B"], c["L"]
    if form.endswith("gpl1"):           # several launches over the groups, in both directions
        assert cdiv(B, 3) > 1 and launches(c, cfg_f, 0) == cdiv(L, cfg_f[3]) * cdiv(B, 3) == launches(c, cfg_b, 1)
    if name == "mix" and 16 in (cfg_f[1], cfg_b[1]):
        assert B % 16 == 1              # a last group of one dialogue
    if name == "l5" and cfg_f[3] == 4:
        assert layer_chunks(L, 4, 0) == [(0, 4), (4, 5)]
    if name == "l5" and cfg_b[3] == 4:
        assert layer_chunks(L, 4, 1) == [(1, 5), (0, 1)]       # the directions chunk differently
    check(c, run(c, cfg_f, cfg_b), form)


OTHER = ((4, 3, 2), (2, 1, 1), True)


@pytest.mark.parametrize("form", ["default", "f4.3.2-b2.1.1-gpl1"])
@pytest.mark.parametrize("name", [n for n in CASES if n not in ("mix", "l5")])
def test_case_matches_float64(name, form):
    """the default configuration and one forced form (other epc, dg and layers per launch in each direction, one group per
    launch) on the edge shapes"""
    c = case(name)
    if form == "default":
        cfg_f, cfg_b = config(c, 0), config(c, 1)
    else:
        cfg_f, cfg_b = forced(c, OTHER)
    if name == "long":
        assert cdiv(c["B"], cfg_f[1]) >= 2 and cdiv(c["B"], cfg_b[1]) >= 2, (cfg_f, cfg_b)      # LDS: dg <= 4
    if name == "limit":
        assert c["T"] == MAX_T
    if name == "b33" and form == "default":
        assert cdiv(c["B"], cfg_f[1]) >= 3
    check(c, run(c, cfg_f, cfg_b), form)


def test_reuse_of_state_and_scratch():
    """one state and one pair of scratch buffers through three calls with different inputs of one shape, then the same three
    through buffers that another configuration (dg = 1: every group's epoch advances alike) used first: each call against
    its own reference -- a stale record taken for a fresh one would show"""
    cs = [case("meld", v) for v in range(3)]
    cfg = (config(cs[0], 0), config(cs[0], 1))
    other = (config(cs[0], 0, 5, 1, 1), config(cs[0], 1, 4, 1, 2))
    state, scratch = None, None
    for v, c in enumerate(cs):
        res = run(c, cfg[0], cfg[1], state, scratch)
        state, scratch = res["state"], res["scratch"]
        check(c, res, "reuse-%d" % v)
    assert int(state[1]) > 0
    scratch = new_scratch(cs[0], cfg, other)
    res = run(cs[1], other[0], other[1], None, scratch)
    check(cs[1], res, "reuse-other-first")
    for v, c in enumerate(cs):
        res = run(c, cfg[0], cfg[1], res["state"], scratch)
        check(c, res, "reuse-after-other-%d" % v)


def test_epoch_words_just_below_2_to_22():
    """tag = epoch * 1024 + step + 1 leaves 32 bits when the epoch reaches 2^22: the launches of this call (two layer chunks
    per direction) take the epochs 2^22 - 1 .. 2^22 + 2"""
    c = case("meld")
    state = torch.zeros(N_STATE, dtype=torch.int32, device=DEV)
    state[1:] = (1 << 22) - 2
    cfg_f, cfg_b = config(c, 0, 0, 0, 2), config(c, 1, 0, 0, 2)
    assert len(layer_chunks(c["L"], cfg_f[3], 0)) == 2 and len(layer_chunks(c["L"], cfg_b[3], 1)) == 2
    res = run(c, cfg_f, cfg_b, state)
    check(c, res, "epoch 2^22")
    assert int(res["state"][1]) == (1 << 22) + 2


def test_attn_sums_on_reference_inputs():
    """erc_dag_attn_sums on the reference's alpha and H1 (run() checks it on the kernels' own): [B*T, 600] vs float64"""
    capi = _capi()
    for name in ("meld", "mono", "t1"):
        c = case(name)
        B, T, dv = c["B"], c["T"], c["dev"]
        for o in c["ref"]:
            ldo = HID + 20
            H1 = torch.full((B * T, ldo), SENT, device=DEV)
            H1[:, :HID] = o["H1"].float().view(B * T, HID).to(DEV)
            alpha = torch.where(c["adj"], o["alpha"].float(), torch.full((), float("nan"))).to(DEV).contiguous()
            A = torch.full((B * T, 2 * HID), SENT, device=DEV)
            capi.dag_attn_sums(alpha, H1, ldo, dv["pred"], dv["spk"], B, T, A)
            assert rel(A.view(B, T, -1).cpu(), o["A"]) <= TOL[name][0], name


def _meta_expect(ids, lens):
    B, T = ids.shape
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rows = np.concatenate([b * T + np.arange(n) for b, n in enumerate(lens)]).astype(np.int32)
    return ids.astype(np.int32), dag_pred_closed_form(ids).astype(np.int32), off, rows


@pytest.mark.parametrize("S", [1, 2, 9])
@pytest.mark.parametrize("B,T", [(1, 1), (1, 110), (1, MAX_T), (5, 110), (3, MAX_T)])
def test_dag_meta_bit_exact(B, T, S):
    capi = _capi()
    rs = np.random.RandomState(B * 1000 + T + S)
    lens = rs.randint(1, T + 1, size=B).astype(np.int64)
    lens[0] = T
    ids = rs.randint(0, S, size=(B, T)).astype(np.int64)
    for b in range(B):
        ids[b, lens[b]:] = 0
    want = _meta_expect(ids, lens)
    N = int(lens.sum())
    d_lens = torch.from_numpy(lens).to(DEV)

    def outputs():
        return (torch.full((B, T), -7, dtype=torch.int32, device=DEV), torch.full((B, T), -7, dtype=torch.int32, device=DEV),
                torch.full((B + 1,), -7, dtype=torch.int32, device=DEV), torch.full((N + 3,), -7, dtype=torch.int32, device=DEV))

    def compare(o):
        torch.cuda.synchronize()
        spk, pred, off, row = (t.cpu().numpy() for t in o)
        np.testing.assert_array_equal(spk, want[0])
        np.testing.assert_array_equal(pred, want[1])
        np.testing.assert_array_equal(off, want[2])
        np.testing.assert_array_equal(row[:N], want[3])
        assert (row[N:] == -7).all()

    # one-hot rows (all-zero on the padded steps: the first maximum is speaker 0), batch stride with a gap
    oh = torch.zeros(B, T + 3, S)
    for b in range(B):
        oh[b, np.arange(lens[b]), ids[b, :lens[b]]] = 1.0
    d_oh = oh.to(DEV)[:, :T]
    assert d_oh.stride(0) == (T + 3) * S and float(d_oh[0, T - 1].sum()) == 1.0
    o = outputs()
    capi.dag_meta(d_oh, None, d_oh.stride(0), d_oh.stride(1), S, d_lens, B, T, *o)
    compare(o)
    # int64 ids, time-major
    d_ids = torch.from_numpy(ids.T.copy()).to(DEV).as_strided((B, T), (1, B))
    assert torch.equal(d_ids.cpu(), torch.from_numpy(ids))
    o = outputs()
    capi.dag_meta(None, d_ids, d_ids.stride(0), d_ids.stride(1), 1 << 30, d_lens, B, T, *o)
    compare(o)


def test_refusals():
    """each a clean ErcGraftError before any launch: T one above the maximum, a dg * T that does not fit the LDS, a cfg
    outside the accepted values"""
    capi = _capi()
    E = capi.ErcGraftError
    T1 = MAX_T + 1
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)
    with pytest.raises(E):
        capi.dag_meta(None, torch.zeros(1, T1, dtype=torch.int64, device=DEV), T1, 1, 2,
                      torch.tensor([T1], device=DEV), 1, T1, i32(1, T1), i32(1, T1), i32(2), i32(T1))
    capi.dag_rec_config(0, 1, MAX_T, 2), capi.dag_rec_config(1, 1, MAX_T, 2)        # the maximum itself is accepted
    for d in (0, 1):
        with pytest.raises(E):
            capi.dag_rec_config(d, 1, T1, 2)
        with pytest.raises(E):
            capi.dag_rec_config(d, 5, 513, 4, 0, 16, 0)          # dg hint: 16 x 513 steps of history exceed 160 KB
    c = case("t1")                                               # real buffers of a B = 4, T = 1 call; nothing is launched

    def call(direction, T, cfg, B=4):
        dv, L = c["dev"], c["L"]
        W5 = HID * (L + 1)
        f = lambda *s: torch.full(s, SENT, device=DEV)
        per = lambda *s: [f(*s) for _ in range(L)]
        Hall, dHall = f(4, W5), f(4, W5)
        b = dict(GI=per(4, 1801), GH=per(4, 1800), Mseq=per(4, HID), R=per(4, 600), ks=per(4), alpha=per(4, 1, 1),
                 DGI=per(4, 1801), DGH=per(4, 1800), dM=per(4, HID), dks=per(4))
        tb = {k: capi.ptr_table([ly[k] for ly in dv["layers"]]) for k in PARAMS}
        tb.update(H1=capi.ptr_table([Hall[:, HID * (l + 1):] for l in range(L)]),
                  Hl=capi.ptr_table([Hall[:, HID * l:] for l in range(L)]), **{k: capi.ptr_table(v) for k, v in b.items()})
        state, scratch = i32(N_STATE), torch.zeros(1 << 16, dtype=torch.int64, device=DEV)
        with pytest.raises(E):
            if direction == 0:
                capi.dag_rec_fwd(Hall, W5, L, tb, dv["pred"], dv["spk"], B, T, W5, 1801, cfg_arr(cfg), state, scratch)
            else:
                capi.dag_rec_bwd(L, tb, W5, 1801, dv["pred"], dv["spk"], B, T, dHall, W5, 1801, cfg_arr(cfg), state, scratch)
        torch.cuda.synchronize()
        assert int(state.abs().sum()) == 0 and int(scratch.abs().sum()) == 0          # no launch: no epoch, no record
        for t in [Hall[:, HID:], dHall] + [x for v in b.values() for x in v]:
            assert bool((t == SENT).all())

    for d in (0, 1):
        call(d, T1, (5, 1, 1, 1), B=1)
        call(d, 513, (5, 16, 1, 1))                              # forced dg * T beyond the LDS
        for bad in ((3, 1, 1, 1), (5, 17, 1, 1), (5, 0, 1, 1), (5, 1, 0, 1), (5, 1, 1, 5), (5, 1, 1, 0)):
            call(d, 1, bad)
        assert capi.dag_rec_scratch_bytes(d, 4, 1, cfg_arr((3, 1, 1, 1))) == -1


def test_report_worst_errors():
    """prints the worst error per case and class over the forms that ran (the figures of the module docstring)"""
    for name, w in WORST.items():
        print("dag-rec-worst %-6s %s" % (name, "  ".join("%s=%.2e" % kv for kv in w.items())))
