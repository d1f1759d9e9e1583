"""Host: ``--module=mmin_miss --eval_missing`` -- the flag and its keys, the float64 restatement of the fused route
(tests/mmin_eval_missing_ref.py) against the whole-model restatement of tests/mmin_miss_ref.py on inputs masked as MMINMissCollate
masks them, the conditions the GPU whole-path test relies on (tests/test_gpu_mmin_eval_missing.py), and the epoch line."""
import numpy as np
import torch

from tests import mmin_eval_missing_ref as ER
from tests import mmin_miss_ref as MR
from tests import mmin_ref as R


def test_flag_defaults_to_off_and_parses():
    from track_mm.mmin_miss import MMINMissParams
    assert MMINMissParams().eval_missing is False
    assert MMINMissParams().from_args([]).eval_missing is False
    assert MMINMissParams().from_args(["--eval_missing"]).eval_missing is True
    assert MMINMissParams().from_args(["--eval_missing=True"]).eval_missing is True


def test_keys_name_the_remaining_modalities_in_missing_types_order():
    from erc_amd import mmin_miss as M
    assert M.MISSING_TYPES == MR.MISSING_TYPES and M.MISSING_KEYS == ER.KEYS == ("v", "t", "a", "tv", "av", "at")
    for key, (v, t, a) in zip(M.MISSING_KEYS, M.MISSING_TYPES):
        assert key == "a" * a + "t" * t + "v" * v
    # the kernel's pattern word: bit 0 visual, bit 1 text, bit 2 audio kept
    assert list(M.MISSING_PATTERNS) == [v | t << 1 | a << 2 for v, t, a in M.MISSING_TYPES] == [1, 2, 4, 3, 5, 6]
    for p in MR.MISSING_TYPES:
        keep = ER.keep_columns(p)
        assert keep[:128].all() == bool(p[2]) and keep[128:256].all() == bool(p[0]) and keep[256:].all() == bool(p[1])
        assert int(keep.sum()) == 128 * sum(p)


def _small_batch(B=3, Ta=9, Tv=6, Tt=7, seed=77):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, Ta, R.AUDIO_D, generator=g)
    for b, z in enumerate((Ta, 4, 1)[:B]):      # zero-padded as the collate pads
        a[b, z:] = 0.0
    return dict(audio_feature=a, visual_feature=torch.randn(B, Tv, R.VISUAL_D, generator=g),
                text_feature=torch.randn(B, Tt, R.TEXT_D, generator=g), label=torch.tensor([1, 3, 0][:B]))


def test_fused_restatement_equals_the_whole_model_on_masked_inputs():
    """expand -> latents-only chain -> classifier -> score in float64, against MR.model_loss_grads run six times on the batch
    masked with MMINMissCollate's arithmetic: all six patterns, B = 3.  Both are float64 evaluations of the same expressions in
    the same order (a sample's encoders do not see its neighbours), so they agree to rounding of the last place"""
    P = MR.named_filled(MR.sd_shapes(), 41)
    batch = _small_batch()
    B = 3
    with R.one_thread():
        fused = ER.fused_logits(P, batch)
        assert tuple(fused.shape) == (6, B, 4)
        cm, loss = ER.score(fused.reshape(6 * B, -1), batch["label"], 6)
        for c, pattern in enumerate(MR.MISSING_TYPES):
            masked = ER.mask_batch(batch, pattern)
            for i, key in enumerate(MR.MODAL_KEYS):      # the collate's arithmetic: x m, a zero where m = 0
                assert bool((masked[key] == (batch[key] if pattern[i] else torch.zeros_like(batch[key]))).all())
            whole = MR.model_loss_grads(P, masked, torch.zeros(B, 384))
            err = R.rel(fused[c], whole["logits"])
            print("pattern %s: fused vs whole-model logits %.2e, Lce %.3e vs %.3e" % (ER.KEYS[c], err, float(loss[c]), float(whole["Lce"])))
            assert err <= 1e-13
            assert abs(float(loss[c]) - float(whole["Lce"])) <= 1e-12 * abs(float(whole["Lce"]))
            want = torch.zeros(4, 4, dtype=torch.int64)
            for y, p in zip(batch["label"].tolist(), whole["logits"].argmax(-1).tolist()):
                want[y, p] += 1
            assert torch.equal(cm[c], want) and int(cm[c].sum()) == B
            # the latents-only chain is the full chain's latents
            x = ER.expand(whole["features"], whole["features"][0], [(1, 1, 1)])
            assert torch.equal(ER.latents_chain(MR._ae_of(P, "netAE"), x, MR.N_BLOCKS), whole["latents"])
    # the six patterns are six different problems
    assert len({tuple(fused[c].flatten().tolist()) for c in range(6)}) == 6


def test_score_restatement_rules():
    nan = float("nan")
    logits = torch.tensor([[1.0, 3.0, 3.0, 0.0], [nan, nan, nan, nan], [2.0, nan, 5.0, 5.0], [0.5, 0.25, 0.125, 0.0]])
    cm, loss = ER.score(logits, torch.tensor([2, 1, 7, 0]), 1)
    assert cm.sum() == 2 and cm[0, 2, 1] == 1 and cm[0, 0, 0] == 1      # ties: the first index; NaN row and bad label: nowhere
    lse = lambda z: float(torch.logsumexp(torch.tensor(z, dtype=torch.float64), 0))
    assert abs(float(loss[0]) - ((lse([1.0, 3.0, 3.0, 0.0]) - 3.0) + (lse([0.5, 0.25, 0.125, 0.0]) - 0.5)) / 2) < 1e-15


def test_whole_path_seeds_have_a_safe_top_two_margin_on_every_row():
    """what tests/test_gpu_mmin_eval_missing.py's equality of confusion matrices rests on: under both weight sets, on both splits,
    every one of the 6 x 5 rows has a float64 top-two logit margin of at least MIN_MARGIN -- no row is excluded; another seed is
    picked in ER.PARAM_SEEDS if one fails.  Also the shape of the run: batches of 2, 2, 1 and at least two audio lengths"""
    for split in ("val", "test"):
        batches = ER.whole_path_batches(split)
        assert [int(b["label"].shape[0]) for b in batches] == [2, 2, 1]
        assert len({int(b["audio_feature"].shape[1]) for b in batches}) >= 2
        for k in (0, 1):
            rows, worst = 0, float("inf")
            for f64, _ in ER.whole_path_reference(split, k):
                top = f64.reshape(-1, f64.shape[-1]).topk(2, -1).values
                worst = min(worst, float((top[:, 0] - top[:, 1]).min()))
                rows += top.shape[0]
            print("%s weights %d: %d rows, smallest top-two margin %.3e" % (split, k, rows, worst))
            assert rows == 6 * 5 and worst >= ER.MIN_MARGIN


def test_epoch_line_has_no_missing_key_without_the_flag_and_six_entries_with_it():
    from erc_amd import mmin
    cmx = np.array([[2, 0], [1, 1]])
    rec = {k: dict(Lall=0.5, Acc=0.75, Acc2=0.5, cm=cmx, cm2=cmx) for k in ER.KEYS}
    out = mmin.missing_records(rec, True)
    assert list(out) == list(ER.KEYS)
    assert all(set(v) == {"Lall", "Acc", "Acc2", "C", "report"} and v["C"] == 4 and v["report"]["cm"] == cmx.tolist() for v in out.values())
    assert all(set(v) == {"Lall", "Acc", "Acc2", "C"} for v in mmin.missing_records(rec, False).values())
    # the epoch line: what MMINBaseTrainer.eval_epoch returns (the flag off) gives the line of before, key for key
    from track_mm.mmin_miss import MMINMissParams
    params = MMINMissParams().from_args([])
    plain = dict(C=4, Lall=1.5, Acc=0.5, Acc2=0.25, true=[0, 1, 1, 0], pred=[0, 0, 1, 1])
    line = mmin.epoch_line(params, 0, 10.0, 2e-4, plain, plain, 0.5, True)
    assert list(line) == ["epoch", "train_utt_per_s", "lr", "val", "test", "report", "class_names", "best_acc", "is_best"]
    assert "missing" not in line and set(line["val"]) == set(line["test"]) == {"Lall", "Acc", "Acc2"}
    with_missing = dict(plain, missing=rec)
    line2 = mmin.epoch_line(params, 0, 10.0, 2e-4, with_missing, with_missing, 0.5, True)
    assert {k: v for k, v in line2.items() if k != "missing"} == line
    assert list(line2["missing"]) == ["val", "test"] and all(list(v) == list(ER.KEYS) for v in line2["missing"].values())
    import json
    json.dumps(line2)
