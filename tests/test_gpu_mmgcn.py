"""MMGCN on the GPU vs (a) golden vectors produced by the REFERENCE's own MMGCNModule and (b) the reference-pinned
CPU oracle at larger shapes (eval mode: every dropout off), and (c) the training-mode step, dropout on, against the float64
restatement of tests/mmgcn_step_ref.py given the masks the step applied."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

from tests.util_cases import poison_lds_before, check_grad_digest, fill_params, make_batch, rel_err, to_device

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dense_adj(ws, B, Mo, N, lens):
    """expand blocks + cross entries to the reference's (M*N)^2 matrix."""
    P = ws["P"]
    ADJ, CR = ws["ADJ"].cpu(), ws["CR"].cpu()
    A = torch.zeros(Mo * N, Mo * N)
    off = 0
    for b, L in enumerate(lens):
        for m in range(Mo):
            A[m * N + off:m * N + off + L, m * N + off:m * N + off + L] = ADJ[b * Mo + m, :L, :L]
            for n in range(Mo):
                if n != m:
                    idx = torch.arange(L)
                    A[m * N + off + idx, n * N + off + idx] = CR[b, m * Mo + n, :L]
        off += L
    return A


@pytest.mark.parametrize("name", ["mmgcn_atv", "mmgcn_tv_s3"])
def test_mmgcn_matches_reference_golden(golden, name):
    from erc_amd.mmgcn import MMGCNModule
    fx = golden(name)
    batch = {k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("in_")}
    da, dt, dv = [int(v) for v in fx["dims"]]
    mods = str(fx["modality"])
    model = MMGCNModule(hidden_text=dt, hidden_visual=dv, hidden_audio=da, n_speakers=int(fx["n_speakers"]),
                        n_classes=int(fx["n_classes"]), modals=mods)
    fill_params(model, int(fx["param_seed"]))
    model.finalize(DEV)
    model.eval()
    dbatch = to_device(batch, DEV)
    for k in ("text_feature", "audio_feature", "visual_feature"):
        dbatch.setdefault(k, None)
    stats = model.loss_and_grads(dbatch).cpu()
    T, B = batch["speaker_tensor"].shape[:2]
    N = int(batch["label"].shape[0])
    ws = model._last_ws
    A = _dense_adj(ws, B, len(mods), N, batch["text_length"].tolist())
    np.testing.assert_allclose(A.numpy(), fx["adj"], atol=2e-5, rtol=1e-4)
    assert float((ws["logits"].cpu() - torch.from_numpy(fx["logits"])).abs().max()) < 1e-4
    assert abs(float(stats[0]) - float(fx["loss"])) < 1e-5
    check_grad_digest(fx, [(n, model.flat.g(n)) for n in model.flat.params], tol=5e-3)
    assert set(model.flat.params).isdisjoint(set(fx["grad_none"].tolist()))
    assert len(model.flat.params) + len(fx["grad_none"]) == len(list(model.named_parameters()))


LARGE = [(16, (20, 110), dict(a=100, t=768, v=512), 2, 6, "atv"), (5, (1, 30), dict(a=30, t=60, v=34), 9, 7, "at")]


@pytest.mark.parametrize("B,lens,dims,S,C,mods", LARGE)
def test_mmgcn_parity_vs_oracle_large(B, lens, dims, S, C, mods, monkeypatch):
    """BASELINE config-3 shape (iemocap-cogmen-sbert-6 atv, B=16, T=110) and a ragged two-modality MELD-like case."""
    _parity_large(B, lens, dims, S, C, mods, monkeypatch)


@pytest.mark.parametrize("env", [dict(ERC_MM_CHAIN="0"), dict(ERC_MM_GEMM_X3="0", ERC_MM_X3="0")], ids=["per_layer", "exact_fp32"])
@pytest.mark.parametrize("B,lens,dims,S,C,mods", LARGE)
def test_mmgcn_parity_vs_oracle_large_env(B, lens, dims, S, C, mods, env, monkeypatch):
    """the same cases and bounds on the per-layer chain (ERC_MM_CHAIN=0: gcnii_layer_fwd, gcnii_combine_bwd) and on the
    exact-fp32 step (ERC_MM_GEMM_X3=0 ERC_MM_X3=0: no three-term bf16 products)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ws = _parity_large(B, lens, dims, S, C, mods, monkeypatch)
    assert ws["chain"] == ("ERC_MM_CHAIN" not in env)
    assert ws.get("gemm_x3", False) == (not env) and ws["planner"].mma_bf16 == (2 if "ERC_MM_X3" not in env else 0)


def _parity_large(B, lens, dims, S, C, mods, monkeypatch):
    from oracle.mmgcn import MMGCNOracle
    from erc_amd.mmgcn import MMGCNModule
    batch = make_batch(B, dims, n_speakers=S, n_classes=C, min_len=lens[0], max_len=lens[1], seed=9, modality=mods,
                       batch_first=False, speaker_onehot=True, force_max=True)
    torch.manual_seed(4)
    ref = MMGCNOracle(hidden_text=dims["t"], hidden_visual=dims["v"], hidden_audio=dims["a"], n_speakers=S, n_classes=C,
                      modals=mods)
    mine = MMGCNModule(hidden_text=dims["t"], hidden_visual=dims["v"], hidden_audio=dims["a"], n_speakers=S, n_classes=C,
                       modals=mods)
    mine.load_state_dict(ref.state_dict())
    mine.finalize(DEV)
    ref.eval(), mine.eval()
    torch.set_num_threads(8)
    logits, _ = ref(**batch)
    loss = F.cross_entropy(logits, batch["label"])
    loss.backward()
    poison_lds_before(monkeypatch, "gcnii_chain_fwd", "gcnii_chain_bwd")       # uninitialised LDS shows up as NaN, on every box
    stats = mine.loss_and_grads(to_device(batch, DEV)).cpu()
    T = batch["speaker_tensor"].shape[0]
    got = mine._last_ws["logits"].cpu()
    assert float((got - logits.detach()).abs().max()) < 1e-4
    assert abs(float(stats[0]) - float(loss.detach())) < 1e-5
    refp = dict(ref.named_parameters())
    errs = {n: rel_err(mine.flat.g(n).cpu(), refp[n].grad) for n in mine.flat.params}
    assert max(errs.values()) < 5e-3, sorted(errs.items(), key=lambda kv: -kv[1])[:6]
    return mine._last_ws


def _dims():
    return dict(a=100, t=768, v=512)


@pytest.mark.parametrize("form", ["rows32", "two_launches", "t128"])
def test_mmgcn_parity_vs_float64_per_dialogue(form, monkeypatch):
    """The real host path in the chain forms the two cases above never take, against MMGCNOracle in float64 run dialogue by
    dialogue (tests/mmgcn_chain_ref.oracle_per_dialogue; exact: test_oracle_mmgcn): B=16 long dialogues (32-row parts),
    B=32 at T=110 (two launches per direction), a batch holding a 128-utterance dialogue"""
    from oracle.mmgcn import MMGCNOracle
    from erc_amd.mmgcn import MMGCNModule
    from tests.mmgcn_chain_ref import launches, oracle_per_dialogue
    from tests.util_cases import make_batch_lengths
    dims, S, C, mods = _dims(), 2, 6, "atv"
    if form == "rows32":
        batch = make_batch(16, dims, n_speakers=S, n_classes=C, min_len=90, max_len=110, seed=21, batch_first=False,
                           speaker_onehot=True, force_max=True)
    elif form == "two_launches":
        batch = make_batch(32, dims, n_speakers=S, n_classes=C, min_len=1, max_len=110, seed=22, batch_first=False,
                           speaker_onehot=True, force_max=True)
    else:
        batch = make_batch_lengths((64, 128, 1, 97, 33), dims, n_speakers=S, n_classes=C, seed=23, batch_first=False,
                                   speaker_onehot=True)
    torch.manual_seed(4)
    ref = MMGCNOracle(hidden_text=dims["t"], hidden_visual=dims["v"], hidden_audio=dims["a"], n_speakers=S, n_classes=C,
                      modals=mods)
    mine = MMGCNModule(hidden_text=dims["t"], hidden_visual=dims["v"], hidden_audio=dims["a"], n_speakers=S, n_classes=C,
                       modals=mods)
    mine.load_state_dict(ref.state_dict())
    mine.finalize(DEV)
    ref.double().eval(), mine.eval()
    torch.set_num_threads(8)
    logits, loss, grads = oracle_per_dialogue(ref, batch)
    poison_lds_before(monkeypatch, "gcnii_chain_fwd", "gcnii_chain_bwd")
    stats = mine.loss_and_grads(to_device(batch, DEV)).cpu()
    ws = mine._last_ws
    lens = [int(v) for v in batch["text_length"]]
    T, B = batch["speaker_tensor"].shape[:2]
    ls = launches(lens, len(mods), T, ws["chain_cfg"])
    if form == "rows32":
        assert B == 16 and len(ls) == 1 and ls[0][3] == 32, ls
    elif form == "two_launches":
        assert B == 32 and T == 110 and len(ls) == 2, ls
    else:
        assert T == 128 and ws["chain"], T
    assert int(mine.flat.health[0]) == 0
    got = ws["logits"].cpu()
    assert float((got.double() - logits).abs().max()) < 1e-4
    assert abs(float(stats[0]) - float(loss)) < 1e-5
    errs = {n: rel_err(mine.flat.g(n).cpu(), grads[n]) for n in mine.flat.params}
    print("mmgcn-err %s launches=%s logits=%.2e loss=%.2e grad=%.2e" % (form, ls, float((got.double() - logits).abs().max()),
                                                                       abs(float(stats[0]) - float(loss)), max(errs.values())))
    assert max(errs.values()) < 5e-3, sorted(errs.items(), key=lambda kv: -kv[1])[:6]


def test_mmgcn_t129_raises_size_error():
    """one utterance past the chain's and the adjacency kernels' limit (T <= 128): a clean ErcGraftError, no launch fault"""
    from erc_amd import capi
    from erc_amd.mmgcn import MMGCNModule
    from tests.util_cases import make_batch_lengths
    dims = dict(a=12, t=20, v=16)
    batch = make_batch_lengths((129, 5), dims, n_speakers=2, n_classes=6, seed=2, batch_first=False, speaker_onehot=True)
    mine = MMGCNModule(hidden_text=dims["t"], hidden_visual=dims["v"], hidden_audio=dims["a"], n_speakers=2, n_classes=6)
    mine.finalize(DEV)
    mine.eval()
    with pytest.raises(capi.ErcGraftError, match="P=132"):
        mine.loss_and_grads(to_device(batch, DEV))
    torch.cuda.synchronize()


def test_mmgcn_train_steps_with_dropout_run():
    import math
    from erc_amd.mmgcn import MMGCNTrainer
    from erc_amd.params import ERCParams, Group
    p = ERCParams().from_args(["--dataset=iemocap-cogmen-6", "--modality=atv"])
    p.optim = Group(name="Adam", lr=3e-4, weight_decay=3e-5)
    p.batch_first, p.speaker_onehot = False, True
    tr = MMGCNTrainer(p, DEV)
    batch = make_batch(4, p.dims(), n_classes=6, min_len=5, max_len=20, seed=6, batch_first=False, speaker_onehot=True)
    losses = [float(tr.train_step(tr.prepare_batch(batch)).cpu()[0]) for _ in range(3)]
    assert all(math.isfinite(l) for l in losses)


def _mmgcn_trainer():
    from erc_amd.mmgcn import MMGCNTrainer
    from erc_amd.params import ERCParams, Group
    p = ERCParams().from_args(["--dataset=iemocap-cogmen-6", "--modality=atv"])
    p.optim = Group(name="Adam", lr=3e-4, weight_decay=3e-5)
    p.batch_first, p.speaker_onehot = False, True
    tr = MMGCNTrainer(p, DEV)
    batch = tr.prepare_batch(make_batch(4, p.dims(), n_classes=6, min_len=17, max_len=40, seed=6, batch_first=False,
                                        speaker_onehot=True))
    return tr, batch


def test_chain_timeout_protocol():
    """health word raised in the middle of a step -> update skipped on the device, next step counts + clears, reported once"""
    from tests.test_gpu_dagerc import _timeout_protocol
    _timeout_protocol(*_mmgcn_trainer())


def test_chain_poll_timeout_fails_the_step_on_the_device():
    """The real thing: with the poll bound at 1 the GCNII chain kernels (several workgroups per dialogue and modality that
    exchange rows every layer) run into it, raise the health word themselves and drain; the optimizer launch of that step
    leaves parameters, moments and the step count alone; check_cluster() reports it; the next step, with the default
    bound, trains."""
    from erc_amd import capi
    tr, batch = _mmgcn_trainer()
    tr.train_step(batch)
    before, m_before, step = tr.model.flat.data.clone(), tr.model.flat.exp_avg.clone(), int(tr.optim.state[0])
    assert tr.model._last_ws["chain"] and step == 1
    capi.gcnii_chain_set_spin_limit(1)
    try:
        tr.train_step(batch)
        torch.cuda.synchronize()
    finally:
        capi.gcnii_chain_set_spin_limit(0)
    assert int(tr.model.flat.health[0]) == capi.HEALTH_RAISED
    assert torch.equal(tr.model.flat.data, before) and torch.equal(tr.model.flat.exp_avg, m_before)
    assert int(tr.optim.state[0]) == step
    with pytest.raises(capi.ErcGraftError, match="GCNII chain"):
        tr.model.check_cluster()
    tr.train_step(batch)
    assert int(tr.optim.state[0]) == step + 1 and int(tr.model.flat.health[0]) == 0
    tr.model.check_cluster()


# ----------------------------------------------------------------------------- the training-mode step (dropout on)
STEP_LENS, STEP_DIMS = (33, 1, 17, 5), dict(a=12, t=20, v=16)


def _step_pair(mods, lens=STEP_LENS, S=2, C=6, seed=31):
    from oracle.mmgcn import MMGCNOracle
    from erc_amd.mmgcn import MMGCNModule
    from tests.util_cases import make_batch_lengths
    dims = STEP_DIMS
    batch = make_batch_lengths(lens, dims, n_speakers=S, n_classes=C, seed=seed, modality=mods, batch_first=False,
                               speaker_onehot=True)
    for k in ("text_feature", "audio_feature", "visual_feature"):
        batch.setdefault(k, None)
    torch.manual_seed(4)
    ref = MMGCNOracle(hidden_text=dims["t"], hidden_visual=dims["v"], hidden_audio=dims["a"], n_speakers=S, n_classes=C,
                      modals=mods)
    mine = MMGCNModule(hidden_text=dims["t"], hidden_visual=dims["v"], hidden_audio=dims["a"], n_speakers=S, n_classes=C,
                       modals=mods)
    mine.load_state_dict(ref.state_dict())
    mine.finalize(DEV)
    return ref, mine, batch


def _regroup(xd, h, Mo, N):
    cat = torch.cat([xd, h], dim=-1)
    return torch.cat([cat[N * i:N * (i + 1)] for i in range(Mo)], dim=-1)


def _applied_masks(mine, ws, B, T, N):
    """the 0/1 keep masks of the step just run, read back from its own buffers (tests/mmgcn_step_ref.py's layouts)"""
    from erc_amd.mmgcn import NLAYERS
    Mo = len(mine.order)
    X, XD, HD, H0, FE = ws["X"].cpu(), ws["XD"].cpu(), ws["HD"].cpu(), ws["_H0"].cpu(), ws["FE"].cpu()
    assert ws["_XD"] is ws["XD"] and ws["_H0"] is ws["H0"], "dropout on: the separate XD / H0 buffers"
    masks = {"x": XD != 0, "h0": (HD[1] != 0) | (H0 == 0), "layers": HD[2:NLAYERS + 2] != 0}
    masks["fe"] = (FE != 0) | (_regroup(XD, HD[NLAYERS + 1], Mo, N) <= 0)
    if "t" in mine.order:
        lw = ws["lstm:lstm_l."]
        l0, l0d = lw["H0"].cpu().view(T, B, 200), lw["H0d"].cpu().view(T, B, 200)
        masks["lstm"] = (l0d != 0) | (l0 == 0)
        _kept_scaled(l0d, l0, l0d != 0, mine.drop_p, "lstm")
    _kept_scaled(XD, X, masks["x"], mine.drop_p, "x")
    _kept_scaled(HD[1], H0, HD[1] != 0, mine.drop_p, "h0")
    return masks


def _kept_scaled(y, x, keep, p, site):
    """kept entries are x * ks: the fp32 keep scale 1 / (1 - p) and the product round once each (2^-22 covers both and the
    rounding of p itself)"""
    want = x.double()[keep] / (1.0 - p)
    assert bool(((y.double()[keep] - want).abs() <= 2.0 ** -22 * want.abs()).all()), site


def _dropped_shares(masks, pre, p):
    """per site the share of dropped entries among those the float64 step has clearly non-zero (> 1e-3: above any fp32 / float64
    disagreement about a ReLU).  sigma <= sqrt(p (1 - p) / 5000) = 0.007 at the smallest site"""
    shares = {}
    for site, keep in masks.items():
        v = pre[site]
        clear = (v.abs() if site in ("x", "lstm") else v) > 1e-3
        if site == "layers":
            each = [1.0 - float(keep[l][clear[l]].double().mean()) for l in range(keep.shape[0])]
            assert min(int(c.sum()) for c in clear) > 2000
            assert all(abs(s - p) < 0.06 for s in each), each
            shares["layers_min"], shares["layers_max"] = min(each), max(each)
        assert int(clear.sum()) > 4000, (site, int(clear.sum()))
        shares[site] = 1.0 - float(keep[clear].double().mean())
        assert abs(shares[site] - p) < 0.04, (site, shares[site])
    return shares


@pytest.mark.parametrize("mods", ["atv", "av"])
@pytest.mark.parametrize("form", ["chain", "per_layer"])
def test_dropout_step_matches_oracle_with_the_applied_masks(form, mods, monkeypatch):
    """One training-mode step (p = 0.4 at every site) against tests/mmgcn_step_ref.py in float64, which is given the keep masks
    the step applied, read back from the step's own buffers.  What keeps the read-back from hiding an error: kept entries equal
    the input times 1 / (1 - p); per site the dropped share among clearly non-zero entries is p within 0.04 (each of the 64
    layers within 0.06); the masks of the streams 1000 (x) and 1001 (h0) are independent (agreeing on p^2 + (1 - p)^2 of the
    entries, within 0.04).  Bounds: the eval-mode parity bounds of this file (logits 1e-4, loss 1e-5, gradients 5e-3 of each
    parameter's largest entry); the float32 CPU run of the same restatement with the same masks is printed next to the step's
    errors as the yardstick of fp32 rounding.
    Measured (MI355X; the step against float64 | the float32 CPU run against float64; no bound had to be derived from the latter):
        chain atv      logits 4.2e-07 loss 2.6e-08 grad 5.4e-06 | logits 8.0e-07 loss 1.5e-07 grad 1.2e-05
        chain av       logits 5.8e-07 loss 9.4e-08 grad 9.1e-06 | logits 9.0e-06 loss 9.4e-08 grad 1.6e-05
        per_layer atv  logits 5.4e-07 loss 9.4e-08 grad 4.3e-06 | as chain atv
        per_layer av   logits 7.6e-07 loss 9.4e-08 grad 2.1e-06 | as chain av
    dropped shares (atv): x 0.400, h0 0.400, layers 0.400 pooled (0.392 .. 0.405), fe 0.398, lstm 0.404; streams 1000 / 1001
    agree on 0.524 of the entries (p^2 + (1 - p)^2 = 0.52)."""
    from tests.mmgcn_step_ref import mmgcn_step_ref
    if form == "per_layer":
        monkeypatch.setenv("ERC_MM_CHAIN", "0")
    ref, mine, batch = _step_pair(mods)
    mine.train()
    p, ks = mine.drop_p, 1.0 / (1.0 - mine.drop_p)
    assert p == 0.4
    stats = mine.loss_and_grads(to_device(batch, DEV)).cpu()
    ws = mine._last_ws
    assert ws["chain"] == (form == "chain") and ws["_p"] == p
    assert int(mine.flat.health[0]) == 0
    T, B = batch["speaker_tensor"].shape[:2]
    N = int(batch["label"].shape[0])
    masks = _applied_masks(mine, ws, B, T, N)
    torch.set_num_threads(8)
    want = mmgcn_step_ref(ref, batch, masks=masks, ks=ks)
    shares = _dropped_shares(masks, want["pre"], p)
    seen = ws["_H0"].cpu() != 0                     # where stream 1001's mask shows
    agree = float((masks["x"][seen] == masks["h0"][seen]).double().mean())
    assert abs(agree - (p * p + (1 - p) * (1 - p))) < 0.04, agree
    assert not torch.equal(masks["layers"][0], masks["layers"][1])
    f32 = mmgcn_step_ref(ref, batch, masks=masks, ks=ks, dtype=torch.float32)
    got = ws["logits"].cpu().double()
    e_logits, e_loss = float((got - want["logits"]).abs().max()), abs(float(stats[0]) - float(want["loss"]))
    assert sorted(mine.flat.params) == sorted(want["grads"])
    errs = {n: rel_err(mine.flat.g(n).cpu(), want["grads"][n]) for n in mine.flat.params}
    y_errs = {n: rel_err(f32["grads"][n], want["grads"][n]) for n in mine.flat.params}
    worst = max(errs, key=errs.get)
    print("mmgcn-err dropout %s %s logits=%.2e loss=%.2e grad=%.2e (%s) | float32 cpu: logits=%.2e loss=%.2e grad=%.2e "
          "grad(%s)=%.2e | dropped %s agree(1000,1001)=%.3f"
          % (form, mods, e_logits, e_loss, errs[worst], worst, float((f32["logits"].double() - want["logits"]).abs().max()),
             abs(float(f32["loss"]) - float(want["loss"])), max(y_errs.values()), worst, y_errs[worst],
             " ".join("%s=%.3f" % kv for kv in sorted(shares.items())), agree))
    assert e_logits < 1e-4
    assert e_loss < 1e-5
    assert errs[worst] < 5e-3, sorted(errs.items(), key=lambda kv: -kv[1])[:6]


def test_consecutive_train_steps_draw_different_masks():
    """two MMGCNTrainer.train_step calls on one batch: the input dropout (stream 1000) keeps different entries, independently"""
    tr, batch = _mmgcn_trainer()
    keeps = []
    for _ in range(2):
        tr.train_step(batch)
        keeps.append((tr.model._last_ws["XD"] != 0).cpu())
    p = tr.model.drop_p
    assert not torch.equal(keeps[0], keeps[1])
    assert abs(float((keeps[0] == keeps[1]).double().mean()) - (p * p + (1 - p) * (1 - p))) < 0.04
    assert all(abs(1.0 - float(k.double().mean()) - p) < 0.04 for k in keeps)
    assert int(tr.model.flat.health[0]) == 0


def test_reused_workspace_carries_nothing_over():
    """The workspace is cached per (B, T, N): a step on lengths (40, 10, 30) and then one on (10, 40, 30) share it.  Logits and
    gradients of the second equal, bit for bit, those of a freshly finalised module that sees only the second batch."""
    from erc_amd.mmgcn import MMGCNModule
    ref, mine, first = _step_pair("atv", lens=(40, 10, 30), seed=41)
    _, _, second = _step_pair("atv", lens=(10, 40, 30), seed=42)
    fresh = MMGCNModule(hidden_text=STEP_DIMS["t"], hidden_visual=STEP_DIMS["v"], hidden_audio=STEP_DIMS["a"], n_speakers=2,
                        n_classes=6, modals="atv")
    fresh.load_state_dict(ref.state_dict())
    fresh.finalize(DEV)
    mine.eval(), fresh.eval()
    mine.loss_and_grads(to_device(first, DEV))
    ws1 = mine._last_ws
    s_mine = mine.loss_and_grads(to_device(second, DEV)).cpu()
    assert mine._last_ws is ws1, "both batches have (B, T, N) = (3, 40, 80)"
    s_fresh = fresh.loss_and_grads(to_device(second, DEV)).cpu()
    assert torch.equal(mine._last_ws["logits"], fresh._last_ws["logits"])
    assert float(s_mine[0]) == float(s_fresh[0])
    for n in mine.flat.params:
        assert torch.equal(mine.flat.g(n), fresh.flat.g(n)), n
    assert int(mine.flat.health[0]) == 0 and int(fresh.flat.health[0]) == 0
