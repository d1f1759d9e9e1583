"""GPU: the launches every trainer's step ends in -- erc_adam_step / erc_adam_step_tab, erc_grad_norm, erc_ema_step,
erc_health_roll, erc_shadow_refresh (csrc/optim.hip, csrc/optim_dev.h, csrc/ema.hip) -- against the float64 restatements of
tests/optim_ref.py, at every launch shape, option and step count, with guard elements behind every buffer.  The fused forms
(the optimizer inside the weight-gradient launch, the peer-to-peer exchange) are tested as "fused equals separate" elsewhere;
these launches are what they are anchored to.  Bounds come from the float32 twins and from bc_term (tests/optim_ref.py), never
from a kernel.  Every test prints its measured figures before it asserts."""
import pytest
import torch

from erc_amd import capi
from tests import optim_ref as R
from tests.test_gpu_cogmen_split import _terms_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8              # elements behind every buffer a kernel writes: nothing may touch them
SENT = -77.25          # what they are filled with (-77 in bf16 and integer buffers)
LR, B1, B2, EPS = R.LR, R.B1, R.B2, R.EPS
WORDS = 4 + 512        # ERC_ADAM_STATE_WORDS


@pytest.fixture(scope="module", autouse=True)
def _lib():
    capi.lib()


def _dev(t, guard=GUARD):
    """``t`` on the device, with ``guard`` sentinel elements behind it"""
    fill = SENT if t.dtype == torch.float32 else -77
    out = torch.full((t.numel() + guard, ), fill, dtype=t.dtype, device=DEV)
    out[:t.numel()] = t.to(DEV)
    return out


def _intact(buf, n):
    return bool((buf[n:] == (SENT if buf.dtype == torch.float32 else -77)).all())


def _state(t_prev, rng=7):
    st = torch.zeros(WORDS, dtype=torch.int64)
    st[0], st[1], st[2], st[3] = t_prev, rng, 1234, -5
    st[4:] = t_prev
    return st.to(DEV)


def _report(tag, figs):
    print("%s: %s" % (tag, "  ".join("%s %.2e/%.1e" % (k, got, bnd) for k, (got, bnd) in figs.items())))


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def _check_step(tag, c, bufs, n, t, wd=0.0, decoupled=False, grad_scale=1.0, clip=0.0, gnorm=0.0):
    """the buffers after ONE launch on case ``c`` (the inputs, on the CPU) against the float64 step: m and v to twin_bound; the
    update, read off the p = 0 group, to twin_bound + bc_term; every other element to others_allowance; guards; g untouched"""
    args = (t, LR, B1, B2, EPS, wd, decoupled, grad_scale, clip, gnorm)
    ins = (c["p"], c["g"], c["m"], c["v"])
    r64, r32 = R.adam_step64(*ins, *args), R.adam_step32(*ins, *args)
    for k in "pgmv":
        assert _intact(bufs[k], n), "guard behind %s" % k
    assert torch.equal(bufs["g"][:n].cpu(), c["g"]), "the gradient was written"
    P, M, V = (bufs[k][:n].cpu() for k in "pmv")
    z = c["grp"] == 0
    figs = dict(m=(R.rel(M, r64[1]), R.twin_bound(r32[1], r64[1])), v=(R.rel(V, r64[2]), R.twin_bound(r32[2], r64[2])))
    bound0 = R.update_bound(r32[3][z], r64[3][z], B1, B2, t)
    if bool((c["p"][z] == 0).all()):          # p_out = -u there: the update's own relative error
        figs["u0"] = (R.rel(P[z], r64[0][z]), bound0)
    if bool((~z).any()) or "u0" not in figs:
        rest = ~z if "u0" in figs else torch.ones_like(z)
        allow = R.others_allowance(r64[0], r64[3], bound0)
        figs["rest"] = (float(((P.double() - r64[0]).abs()[rest] / allow[rest].clamp_min(1e-300)).max()), 1.0)
    _report("%s (n=%d t=%d bc_term %.2e, the twin's update %.2e)" % (tag, n, t, R.bc_term(B1, B2, t), R.rel(r32[3][z], r64[3][z])), figs)
    for k, (got, bnd) in figs.items():
        assert got <= bnd, (tag, k, got, bnd)
    if wd == 0.0:      # nothing to do, nothing done: a zero gradient on zero moments leaves the element's bits alone
        still = (c["g"] == 0) & (c["m"] == 0) & (c["v"] == 0)
        assert torch.equal(_bits(P[still]), _bits(c["p"][still])) and bool((M[still] == 0).all()) and bool((V[still] == 0).all())
    return r64


def _launch(c, n, state, wd=0.0, decoupled=False, grad_scale=1.0, clip=0.0, gnorm=None, **kw):
    bufs = {k: _dev(c[k]) for k in "pgmv"}
    capi.adam_step(bufs["p"], bufs["g"], bufs["m"], bufs["v"], n, LR, B1, B2, EPS, wd, decoupled, grad_scale, clip, gnorm, state, **kw)
    torch.cuda.synchronize()
    return bufs


# ------------------------------------------------------------------------------------------- 1. every launch shape
@pytest.mark.parametrize("n", R.SIZES)
def test_one_step_at_every_launch_shape(n):
    """n < 4: no whole quad, only the tail threads of workgroup 0 work; 524288: exactly one pass of the 512-workgroup grid;
    524292 / 524295: one quad of a second pass (and a tail); 1049607: a third pass begins"""
    c = R.adam_case("block1-%d" % n, n)
    state = _state(0)
    bufs = _launch(c, n, state)
    _check_step("shape", c, bufs, n, 1)
    st = state.cpu()
    assert st[:4].tolist() == [1, 8, 1234, -5] and bool((st[4:] == 1).all())


# --------------------------------------------------------------------------------------------------------- 2. options
@pytest.mark.parametrize("n", R.OPTION_SIZES)
@pytest.mark.parametrize("name", sorted(R.OPTIONS))
def test_options(name, n):
    """Adam with and without L2, AdamW, grad_scale, clipping that bites and clipping that does not; the norm comes from
    erc_grad_norm on the device and the reference is fed the device's value"""
    decoupled, wd, grad_scale, clip_mult = R.OPTIONS[name]
    c = R.adam_case("opt-%s-%d" % (name, n), n)
    gnorm_d, clip, gn = None, 0.0, 0.0
    if clip_mult > 0:
        gnorm_d, ws = _dev(torch.zeros(1)), _dev(torch.zeros(1024))
        capi.grad_norm(c["g"].to(DEV), n, grad_scale, gnorm_d, ws)
        gn = float(gnorm_d[0].cpu())
        want = R.grad_norm64(c["g"], grad_scale)
        print("gnorm %.8e, float64 %.8e: off by %.2e / %.1e" % (gn, want, abs(gn - want) / want, R.norm_bound(c["g"], grad_scale)))
        assert abs(gn - want) <= R.norm_bound(c["g"], grad_scale) * want and _intact(gnorm_d, 1) and _intact(ws, 1024)
        clip = R.f32(clip_mult * gn)
    bufs = _launch(c, n, _state(0), wd=wd, decoupled=decoupled, grad_scale=grad_scale, clip=clip, gnorm=gnorm_d)
    _check_step("options %s" % name, c, bufs, n, 1, wd=wd, decoupled=decoupled, grad_scale=grad_scale, clip=clip, gnorm=gn)
    if clip_mult > 0:
        assert float(gnorm_d[0].cpu()) == gn


# ----------------------------------------------------------------------------------------------------- 3. step counts
@pytest.mark.parametrize("t", R.STEP_COUNTS)
def test_step_count_without_running_the_steps(t):
    """state[0] and all 512 private copies preset to t - 1, moments of plausible size: one launch is step t.  Afterwards every
    copy is t -- those of workgroups this grid does not have included -- and a launch with another grid makes them t + 1"""
    n, n2 = R.STEP_N
    c = R.adam_case("step-%d" % t, n, with_moments=True)
    state = _state(t - 1)
    bufs = _launch(c, n, state)
    _check_step("step", c, bufs, n, t)
    st = state.cpu()
    assert st[:4].tolist() == [t, 8, 1234, -5] and bool((st[4:] == t).all())
    c2 = R.adam_case("step-%d-b" % t, n2, with_moments=True)
    bufs2 = _launch(c2, n2, state)
    _check_step("step, next grid", c2, bufs2, n2, t + 1)
    st = state.cpu()
    assert st[:4].tolist() == [t + 1, 9, 1234, -5] and bool((st[4:] == t + 1).all())


# --------------------------------------------------------------------------------------------- 4. consecutive steps
def test_five_consecutive_steps():
    """each step against the float64 step of the kernel's OWN previous p, m, v: five one-step comparisons, nothing compounds.
    A second run from the same start gives the same bits"""
    n = R.CHAIN_N
    c0 = R.adam_case("chain", n)
    grads = [R.adam_case("chain-g%d" % k, n)["g"] * (0.01 if k % 2 else 1.0) for k in range(R.CHAIN_STEPS)]
    runs = []
    for run in range(2):
        bufs = {k: _dev(c0[k]) for k in "pmv"}
        state = _state(0)
        trace = []
        for k, g in enumerate(grads):
            before = dict(p=bufs["p"][:n].cpu(), m=bufs["m"][:n].cpu(), v=bufs["v"][:n].cpu(), g=g, grp=c0["grp"])
            bufs["g"] = _dev(g)
            capi.adam_step(bufs["p"], bufs["g"], bufs["m"], bufs["v"], n, LR, B1, B2, EPS, 3e-5, False, 1.0, 0.0, None, state)
            torch.cuda.synchronize()
            if run == 0:
                _check_step("chain", before, bufs, n, k + 1, wd=3e-5)
            trace.append([bufs[q].clone() for q in "pmv"])
        assert state.cpu()[:2].tolist() == [R.CHAIN_STEPS, 7 + R.CHAIN_STEPS]
        runs.append(trace)
    for a, b in zip(runs[0], runs[1]):
        for x, y in zip(a, b):
            assert torch.equal(_bits(x), _bits(y))


# ------------------------------------------------------------------------------------------------------ 5. skip_flag
def test_skip_flag_and_health_roll():
    n, sn = 1027, 1024
    c = R.adam_case("skip", n, with_moments=True)

    def run(flag):
        shadow = torch.full((sn + GUARD, ), -77.0, dtype=torch.bfloat16, device=DEV)
        state = _state(41)
        word = None if flag is None else torch.tensor([flag, -77], dtype=torch.int32, device=DEV)
        bufs = _launch(c, n, state, shadow=shadow, shadow_off=0, shadow_n=sn, skip_flag=word)
        assert word is None or word.cpu().tolist() == [flag, -77]          # the optimizer reads the word, erc_health_roll clears it
        return bufs, state, shadow

    bufs, state, shadow = run(capi.HEALTH_RAISED)
    for k in "pgmv":
        assert torch.equal(_bits(bufs[k].cpu()), _bits(_dev(c[k]).cpu())), k
    assert torch.equal(state, _state(41)) and bool((shadow == -77.0).all())
    bufs, state, shadow = run(1)[0:3]
    assert torch.equal(_bits(bufs["p"].cpu()), _bits(_dev(c["p"]).cpu())) and torch.equal(state, _state(41))
    plain, flagged = run(None), run(0)
    for k in "pmv":
        assert torch.equal(_bits(plain[0][k]), _bits(flagged[0][k])), k
    assert torch.equal(plain[1], flagged[1]) and torch.equal(_bits(plain[2]), _bits(flagged[2]))
    assert int(plain[1][0]) == 42 and not torch.equal(plain[0]["p"][:n].cpu(), c["p"])
    assert torch.equal(plain[2][:sn].float(), plain[0]["p"][:sn].to(torch.bfloat16).float()) and bool((plain[2][sn:] == -77.0).all())
    # erc_health_roll: a raised word becomes one event and is cleared; a clear word leaves both alone
    health = torch.tensor([capi.HEALTH_RAISED, -77], dtype=torch.int32, device=DEV)
    events = torch.tensor([5, -77], dtype=torch.int32, device=DEV)
    capi.health_roll(health, events)
    assert health.cpu().tolist() == [0, -77] and events.cpu().tolist() == [6, -77]
    capi.health_roll(health, events)
    assert health.cpu().tolist() == [0, -77] and events.cpu().tolist() == [6, -77]


# --------------------------------------------------------------------------------------------------- 6. shadow paths
SH_ROWS, SH_K = 10, 230        # K % 4 = 2: the 16-byte shadow store path is off for the whole table
SH_OFF0 = 64
SH_ROWS1, SH_K1 = 5, 16
SH_OFF1 = SH_OFF0 + SH_ROWS * SH_K + 1        # 2365: not on a quad
SH_N = SH_OFF1 + SH_ROWS1 * SH_K1 + 6         # 2451: three elements of scalar tail


def _shadow_table(terms):
    t = capi.ShadowTable(DEV)
    i0 = t.add(SH_OFF0, SH_ROWS * SH_K, SH_ROWS * SH_K, SH_K, SH_ROWS, (0, 1, 0), (1, 0, 0), SH_K, 0, terms=terms)       # row-major, odd K
    i1 = t.add(SH_OFF1, SH_ROWS1 * SH_K1, SH_ROWS1 * SH_K1, SH_K1, SH_ROWS1, (0, 1, 0), (1, 0, 0), SH_K1, 0, terms=terms)  # odd source offset
    i2 = t.add(SH_OFF0, SH_ROWS * SH_K, 8 * 512, SH_K, SH_ROWS, (0, 1, 0), (1, 0, 0), 8, 1, terms=terms)                  # fragment order, odd K
    t.seal()
    t.buf.fill_(-77.0)
    return t, (i0, i1, i2)


def _expected_shadow(t, idx, p, terms):
    """the whole bf16 buffer from the bf16 expansion of the parameters ``p`` (CPU), -77 wherever no range maps"""
    want = torch.full((t.buf.numel(), ), -77.0, dtype=torch.bfloat16)
    W0 = p[SH_OFF0:SH_OFF0 + SH_ROWS * SH_K].view(SH_ROWS, SH_K)
    W1 = p[SH_OFF1:SH_OFF1 + SH_ROWS1 * SH_K1].view(SH_ROWS1, SH_K1)
    mapped = capi.mfma_b_fragment_order(torch.ones(SH_ROWS, SH_K), 8) > 0
    for ti in range(terms):
        for i, W in ((idx[0], W0), (idx[1], W1)):
            off = t.descs[i][2] + ti * t.plane(i)
            want[off:off + W.numel()] = _terms_of(W, terms)[ti].to(torch.bfloat16).flatten()
        off = t.descs[idx[2]][2] + ti * t.plane(idx[2])
        frag = capi.mfma_b_fragment_order(_terms_of(W0, terms)[ti].to(torch.bfloat16), 8)
        want[off:off + 8 * 512] = torch.where(mapped, frag, want[off:off + 8 * 512])
    return want


@pytest.mark.parametrize("terms", [1, 2, 3])
def test_shadow_ranges_off_the_quad_path(terms):
    """erc_adam_step_tab with a row-major range of K = 230 (n0 % 4 != 0), one whose source offset is not a multiple of 4 and a
    fragment-order range of the same odd K: the planes are the bf16 expansion of the UPDATED parameters, bit for bit, equal to
    erc_shadow_refresh on them, and the rest of the shadow buffer is untouched"""
    c = R.adam_case("shadow", SH_N)
    t, idx = _shadow_table(terms)
    spans = sorted((t.descs[i][2], t.descs[i][2] + t.sizes[i]) for i in idx)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "destination ranges overlap"
    bufs = {k: _dev(c[k]) for k in "pgmv"}
    capi.adam_step_tab(bufs["p"], bufs["g"], bufs["m"], bufs["v"], SH_N, LR, B1, B2, EPS, 0.0, False, 1.0, 0.0, None, _state(0), t)
    torch.cuda.synchronize()
    _check_step("shadow terms=%d" % terms, c, bufs, SH_N, 1)
    p_new = bufs["p"][:SH_N].cpu()
    want = _expected_shadow(t, idx, p_new, terms)
    assert torch.equal(_bits(t.buf.cpu()), _bits(want))
    assert int((want == -77.0).sum()) > 64          # there is something outside the ranges to be left alone
    t2, _ = _shadow_table(terms)
    capi.shadow_refresh(bufs["p"], SH_N, t2)
    assert torch.equal(_bits(t2.buf), _bits(t.buf))
    # without the table the step itself is the same
    plain = _launch(c, SH_N, _state(0))
    for k in "pmv":
        assert torch.equal(_bits(plain[k]), _bits(bufs[k])), k


# ------------------------------------------------------------------------------------------------------ 7. grad norm
def _norm_check(tag, g, n, scale):
    gnorm, ws = _dev(torch.zeros(1)), _dev(torch.zeros(1024))
    gd = _dev(g)
    capi.grad_norm(gd, n, scale, gnorm, ws)
    first = gnorm.clone()
    capi.grad_norm(gd, n, scale, gnorm, ws)           # the workspace holds the first call's partial sums
    torch.cuda.synchronize()
    got, want, bound = float(gnorm[0].cpu()), R.grad_norm64(g, scale), R.norm_bound(g, scale)
    print("%s n=%d scale=%.3f: %.8e against %.8e: %.2e / %.1e (twin %.2e)" % (
        tag, n, scale, got, want, abs(got - want) / want, bound, abs(R.grad_norm32(g, scale) - want) / want))
    assert abs(got - want) <= bound * want
    assert torch.equal(_bits(first), _bits(gnorm)) and _intact(gnorm, 1) and _intact(ws, 1024) and torch.equal(gd[:n].cpu(), g)


@pytest.mark.parametrize("n", R.NORM_SIZES)
def test_grad_norm(n):
    """the grid is 512 x 256: one element, one short of and one over a workgroup, one full pass, one element of a second"""
    for scale in R.NORM_SCALES:
        _norm_check("norm", R.norm_case("n%d" % n, n), n, scale)


@pytest.mark.parametrize("name", sorted(R.NORM_WIDE))
def test_grad_norm_outside_float32_squares(name):
    """magnitudes whose squares overflow float32 when summed (1e-25 .. 1e18), or vanish in it (below 1e-23): the kernel
    accumulates in double"""
    n, lo, hi = R.NORM_WIDE[name]
    _norm_check(name, R.norm_case(name, n, lo, hi), n, 1.0)


# ------------------------------------------------------------------------------------------------------------- 8. EMA
@pytest.mark.parametrize("n", R.EMA_SIZES)
def test_ema_step_bit_for_bit(n):
    gen = R._gen("ema-%d" % n)
    ema, p = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    e_d, p_d = _dev(ema), _dev(p)
    capi.ema_step(e_d, p_d, n, 0.999)
    torch.cuda.synchronize()
    assert torch.equal(_bits(e_d[:n].cpu()), _bits(R.ema_step32(ema, p, 0.999)))
    assert _intact(e_d, n) and _intact(p_d, n) and torch.equal(p_d[:n].cpu(), p)


# ------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_by_status_with_nothing_written():
    n = SH_N
    c = R.adam_case("refuse", n, with_moments=True)
    bufs = {k: _dev(c[k]) for k in "pgmv"}
    state = _state(3)
    gnorm, ws = _dev(torch.ones(1)), _dev(torch.zeros(1024))
    t, _ = _shadow_table(1)
    short = capi.ShadowTable(DEV)
    short.descs, short.sizes, short.numel = t.descs, t.sizes, t.numel
    short.seal()
    short.buf = torch.full((t.numel - 1, ), -77.0, dtype=torch.bfloat16, device=DEV)     # the last range reaches one element past it
    p, g, m, v = (bufs[k] for k in "pgmv")
    tail = (LR, B1, B2, EPS, 0.0, False, 1.0)
    calls = {
        "n = 0": lambda: capi.adam_step(p, g, m, v, 0, *tail, 0.0, None, state),
        "misaligned p": lambda: capi.adam_step(p[1:], g, m, v, n - 1, *tail, 0.0, None, state),
        "misaligned g": lambda: capi.adam_step(p, g[2:], m, v, n - 2, *tail, 0.0, None, state),
        "misaligned v": lambda: capi.adam_step(p, g, m, v[3:], n - 3, *tail, 0.0, None, state),
        "clip_norm without gnorm": lambda: capi.adam_step(p, g, m, v, n, *tail, 1.0, None, state),
        "shadow range past the buffer": lambda: capi.adam_step_tab(p, g, m, v, n, *tail, 0.0, None, state, short),
        "shadow range past the parameters": lambda: capi.adam_step_tab(p, g, m, v, SH_OFF1, *tail, 0.0, None, state, t),
        "refresh past the buffer": lambda: capi.shadow_refresh(p, n, short),
        "grad_norm n = 0": lambda: capi.grad_norm(g, 0, 1.0, gnorm, ws),
        "grad_norm workspace off 8 bytes": lambda: capi.grad_norm(g, n, 1.0, gnorm, ws[1:]),
        "ema n = 0": lambda: capi.ema_step(p, g, 0, 0.999),
        "ema alpha > 1": lambda: capi.ema_step(p, g, n, 1.5),
    }
    for what, call in calls.items():
        with pytest.raises(capi.ErcGraftError):
            call()
        print("refused:", what)
    torch.cuda.synchronize()
    for k in "pgmv":
        assert torch.equal(_bits(bufs[k].cpu()), _bits(_dev(c[k]).cpu())), k
    assert torch.equal(state, _state(3)) and bool((t.buf == -77.0).all()) and bool((short.buf == -77.0).all())
    assert gnorm.cpu().tolist()[0] == 1.0 and _intact(gnorm, 1) and bool((ws[:1024] == 0).all())
