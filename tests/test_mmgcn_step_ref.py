"""CPU: tests/mmgcn_step_ref.py (the float64 MMGCN step with given dropout masks, against which the GPU's training-mode step is
compared) reproduces the pinned oracle where the two must agree, and applies its masks where it says it does."""
import pytest
import torch
from torch.nn import functional as F

from oracle.mmgcn import MMGCNOracle
from tests.mmgcn_step_ref import FD, NL, SITES, mmgcn_step_ref
from tests.util_cases import make_batch_lengths

CASES = {"atv_ragged": ((7, 1, 12), dict(a=12, t=20, v=16), 2, 6, "atv"), "at_s9": ((5, 9, 2), dict(a=10, t=14, v=8), 9, 7, "at")}


def _case(name):
    lens, dims, S, C, mods = CASES[name]
    batch = make_batch_lengths(lens, dims, n_speakers=S, n_classes=C, seed=5, modality=mods, batch_first=False,
                               speaker_onehot=True)
    torch.manual_seed(3)
    ref = MMGCNOracle(hidden_text=dims["t"], hidden_visual=dims["v"], hidden_audio=dims["a"], n_speakers=S, n_classes=C,
                      modals=mods)
    return ref, batch


def _oracle_f64(ref, batch):
    import copy
    o = copy.deepcopy(ref).double().eval()
    b = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
    logits, _ = o(**b)
    loss = F.cross_entropy(logits, batch["label"])
    loss.backward()
    return logits.detach(), loss.detach(), {n: p.grad for n, p in o.named_parameters() if p.grad is not None}


def _rel(a, b):
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    return err / scale if scale > 0 else err


def _same(got, logits, loss, grads, tol=1e-10):
    assert got["logits"].dtype == torch.float64
    assert _rel(got["logits"], logits) < tol and _rel(got["loss"], loss) < tol
    assert sorted(got["grads"]) == sorted(grads)
    for n in grads:
        assert _rel(got["grads"][n], grads[n]) < tol, n


def _ones(got):
    m = {k: torch.ones_like(v) for k, v in got["pre"].items()}
    assert set(m) <= set(SITES)
    return m


@pytest.mark.parametrize("name", list(CASES))
def test_step_ref_without_masks_is_the_eval_mode_oracle(name):
    ref, batch = _case(name)
    want = _oracle_f64(ref, batch)
    got = mmgcn_step_ref(ref, batch)
    _same(got, *want)
    T, B = batch["speaker_tensor"].shape[:2]
    N, Mo = int(batch["label"].shape[0]), len(ref.modals)
    assert got["pre"]["x"].shape == (Mo * N, FD) and got["pre"]["layers"].shape == (NL, Mo * N, FD)
    assert got["pre"]["fe"].shape == (N, Mo * 2 * FD) and ("lstm" in got["pre"]) == ("t" in ref.modals)
    assert got["pre"]["lstm"].shape == (T, B, FD)
    # all-ones masks and ks = 1: the same step
    _same(mmgcn_step_ref(ref, batch, masks=_ones(got), ks=1.0), *want)
    assert all(p.grad is None for p in ref.parameters())


def test_step_ref_applies_each_mask_at_its_site():
    """one zero in a site's mask: the gradient through that site's entry vanishes, its neighbour's does not; and with ks = 2
    on all-ones masks of ONE site the step equals the step on inputs scaled there (the scale is applied, once)"""
    ref, batch = _case("atv_ragged")
    base = mmgcn_step_ref(ref, batch)
    for site, at, nb in (("lstm", (2, 1, 7), (2, 1, 8)), ("x", (21, 5), (21, 6)), ("h0", (3, 150), (4, 150)),
                         ("layers", (40, 17, 3), (39, 17, 3)), ("fe", (11, 2 * FD + 9), (11, 2 * FD + 10))):
        # entries that carry a value and a gradient in the unmasked step (a ReLU may have closed the ones named above)
        live = (base["site_grads"][site] != 0) & (base["pre"][site] != 0)
        if not (bool(live[at]) and bool(live[nb])):
            nz = live.nonzero()
            at, nb = tuple(int(v) for v in nz[0]), tuple(int(v) for v in nz[1])
        masks = _ones(base)
        masks[site][at] = 0
        got = mmgcn_step_ref(ref, batch, masks=masks, ks=1.0)
        assert float(got["site_grads"][site][at]) == 0.0, site
        assert float(got["site_grads"][site][nb]) != 0.0, site
        assert _rel(got["logits"], base["logits"]) > 0, site
    masks = {"h0": torch.ones_like(base["pre"]["h0"])}
    got = mmgcn_step_ref(ref, batch, masks=masks, ks=2.0)
    assert _rel(got["pre"]["layers"][0], base["pre"]["layers"][0]) > 1e-3
    assert torch.equal(got["pre"]["h0"], base["pre"]["h0"])


def test_step_ref_float32_run_is_close_to_float64():
    """the float32 run the GPU tests take as their yardstick is the same computation (fp32 rounding apart)"""
    ref, batch = _case("atv_ragged")
    a, b = mmgcn_step_ref(ref, batch), mmgcn_step_ref(ref, batch, dtype=torch.float32)
    assert b["logits"].dtype == torch.float32
    assert _rel(b["logits"].double(), a["logits"]) < 1e-4
