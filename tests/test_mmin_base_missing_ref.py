"""CPU: the host side of ``--module=mmin_base --eval_missing / --train_missing`` -- the float64 restatement of the fused route
(tests/mmin_base_missing_ref.py) against the whole-model restatement on host-masked inputs, the prefix-maximum table against
per-length zero-input scans, the float32 twin and the margins behind the GPU test's bounds, the masked collate's restatement
against MMINMissCollate, the 4 B_cap descriptor tables and their pattern draws, and the refusals.  No library is loaded."""
import random
import types

import pytest
import torch
from torch.utils.data import DataLoader

from erc_amd import capi, mmin
from erc_amd.datasets import MMINDeviceStore, MMINMaskedDeviceStore
from erc_amd.mmin_miss import Missing, MMINMissCollate
from tests import mmin_base_missing_ref as BR
from tests import mmin_cap_ref as CR
from tests import mmin_eval_missing_ref as ER
from tests import mmin_miss_ref as MR
from tests import mmin_ref as R


def _batch3():
    return mmin.mmin_collate(CR.samples_with_frames((6, 3, 5), seed=8, tv=BR.TV, tt=BR.TT))


def test_fused_route_equals_the_whole_model_on_host_masked_inputs():
    """float64, B = 3, all six patterns: expand + classifier against six forwards of tests/mmin_ref.py on masked inputs"""
    P, batch = BR.whole_weights(0), _batch3()
    with R.one_thread():
        fused, naive = BR.fused_logits(P, batch), BR.naive_logits(P, batch)
    err = R.rel(fused, naive)
    print("mmin_base fused vs whole model, float64: %.2e" % err)
    assert fused.shape == (6, 3, 4) and err <= 1e-13
    full = R.model_forward(P, batch)["logits"]
    assert all(R.rel(fused[c], full) > 1e-3 for c in range(6))        # masking moves every pattern's logits


def test_prefix_maximum_table_equals_per_length_zero_scans():
    P = BR.whole_weights(0)
    with R.one_thread():
        table = BR.prefix_table(P, BR.T_MAX_TABLE)
        assert table.shape == (BR.T_MAX_TABLE + 1, 128) and bool((table[0] == 0).all())
        for Ta in BR.TABLE_TA:
            want = ER.zero_features(P, Ta, BR.TV, BR.TT)[:128]
            assert torch.equal(table[Ta], want), Ta
        assert torch.equal(BR.zero_vt(P, BR.TV, BR.TT), ER.zero_features(P, 3, BR.TV, BR.TT)[128:])
    assert bool((table[1:].diff(dim=0) >= 0).all()) and not torch.equal(table[1], table[BR.T_MAX_TABLE])


def test_twin_bound_and_margins_of_the_whole_path_cases():
    """the float32 twin's worst deviation (the GPU test's logits bound is 4 times it) and every row's float64 top-two margin:
    no row is exempt from the confusion-matrix comparison"""
    dev, bound = BR.twin_deviation(), BR.logits_bound()
    rec = BR.FIGURES[("eval_missing", "logits")]
    print("mmin_base eval_missing twin: worst deviation %.3g, bound %.3g (recorded %.3g / %.3g)" % (dev, bound, rec[0], rec[1]))
    assert 0 < dev < 1e-5 and bound == BR.LOGITS_MARGIN * max(dev, R.FLOOR)
    assert abs(dev - rec[0]) <= 0.25 * rec[0] and abs(bound - rec[1]) <= 0.25 * rec[1]      # the recorded figures are these
    lens = set()
    for k in (0, 1):
        P = BR.whole_weights(k)
        for b, (f64, f32) in zip(BR.whole_batches(), BR.whole_reference(k)):
            lens.add(int(b["audio_feature"].shape[1]))
            with R.one_thread():
                full = R.model_forward(P, b)["logits"]
            m = min(BR.top_two_margin(f64), BR.top_two_margin(full))
            print("pass %d Ta %d: smallest top-two margin %.3g" % (k, int(b["audio_feature"].shape[1]), m))
            assert m >= BR.MIN_MARGIN
            assert torch.equal(f64.argmax(-1), f32.argmax(-1))
    assert [int(b["label"].shape[0]) for b in BR.whole_batches()] == [2, 2, 1] and len(lens) == 3


# ------------------------------------------------------------------------------------------------------------ masked collate
def _samples(n=11, frames=(3, 40), seed=5):
    return CR.small_samples(n, frames, seed=seed, tv=BR.TV, tt=BR.TT)


@pytest.mark.parametrize("idx, B_cap, T_cap", [((4, 0, 9, 2, 7, 1), 6, 64), ((2, ), 1, 40), ((7, 1), 3, 48)])
def test_masked_collate_restatement_equals_mmin_miss_collate(idx, B_cap, T_cap):
    samples = _samples()
    store = MMINMaskedDeviceStore(samples, None)
    picked = [dict(samples[i], missing_type=list(MR.MISSING_TYPES[n % 6])) for n, i in enumerate(idx)]
    host = MMINMissCollate(has_miss=True)(picked)
    own = mmin.mask_collate(picked)
    bits = [BR.keep_bits(s["missing_type"]) for s in picked]
    table, caps = store.table([list(idx)], B_cap, [bits])
    a, v, t, y, c = BR.collate_masked_ref(store, table[0], B_cap, T_cap)
    B, Ta = len(idx), host["audio_feature"].shape[1]
    assert c.tolist() == [B, Ta] and caps == [min(-(-Ta // 64) * 64, store.t_max)]
    for got, key in ((a[:B, :Ta], "audio_feature"), (v[:B], "visual_feature"), (t[:B], "text_feature"), (y[:B], "label")):
        assert torch.equal(got, host[key]), key                     # by value: x * 0 is -0.0 for a negative x
        assert torch.equal(own[key], host[key]), key
    assert not any(k.endswith("_reverse") for k in own) and torch.equal(own["missing_type"], host["missing_type"])
    assert not a[:B, Ta:].any() and not a[B:].any() and not v[B:].any() and not t[B:].any() and not y[B:].any()
    ma, mv, mt = BR.masked_rows(table[0], B_cap)
    assert ma[:B].tolist() == [not s["missing_type"][2] for s in picked] and mv[:B].tolist() == [not s["missing_type"][0] for s in picked]
    assert mt[:B].tolist() == [not s["missing_type"][1] for s in picked]
    if B >= 6:
        assert all(bool(x[:B].any()) and not bool(x[:B].all()) for x in (ma, mv, mt))
    full = torch.cat([torch.as_tensor(table[0][:3 * B_cap]), torch.full((B_cap, ), 7 + 8, dtype=torch.int32)])      # bit 3: masked off
    for got, want in zip(BR.collate_masked_ref(store, full, B_cap, T_cap), CR.collate_ref(store, table[0][:3 * B_cap], B_cap, T_cap)):
        assert torch.equal(got, want)


def test_descriptor_tables_have_four_blocks():
    samples = _samples()
    plain, masked = MMINDeviceStore(samples, None), MMINMaskedDeviceStore(samples, None)
    assert MMINDeviceStore.DESC_INTS == 3 and MMINMaskedDeviceStore.DESC_INTS == 4
    batches, B = [[3, 0, 10], [5]], 4
    t3, caps3 = plain.table(batches, B)
    t4, caps4 = masked.table(batches, B, [[1, 6, 5], [2]])
    assert t3.shape == (2, 3 * B) and t4.shape == (2, 4 * B) and str(t4.dtype) == "int32" and caps3 == caps4
    assert (t4[:, :3 * B] == t3).all()
    assert t4[:, 3 * B:].tolist() == [[1, 6, 5, 0], [2, 0, 0, 0]]
    assert masked.table(batches, B)[0][:, 3 * B:].tolist() == [[7, 7, 7, 0], [7, 0, 0, 0]]
    with pytest.raises(ValueError):
        masked.table(batches, B, [[1, 2], [3]])
    assert plain.table(batches, B)[0].shape == (2, 3 * B)                # MMINDeviceStore.table is what it was


class _Trainer:
    use_ema = True
    train_missing = True

    def __init__(self):
        self.model = types.SimpleNamespace(dynamic_n=False, _last_ws="ws")
        self.params = types.SimpleNamespace(n_classes=4)


def test_pattern_draws_follow_the_transformed_dataloader():
    """two epochs: the (sample, pattern) pairs of MMINResidentEpochs.tables equal those of a DataLoader over
    _Transformed(samples, Missing()) from the same generator and ``random`` state"""
    samples, B = _samples(n=11), 4
    random.seed(31)
    loader = DataLoader(mmin._Transformed(samples, Missing()), batch_size=B, shuffle=True, generator=torch.Generator().manual_seed(9),
                        collate_fn=lambda ss: [(s["name"], BR.keep_bits(s["missing_type"])) for s in ss])
    want = [list(loader) for _ in range(2)]
    tail = random.random()
    random.seed(31)
    store = MMINMaskedDeviceStore(samples, None)
    res = mmin.MMINResidentEpochs(_Trainer(), store, B, torch.Generator().manual_seed(9))
    assert res.cur_desc.shape == (4 * B, )
    names = [s["name"] for s in samples]
    seen = set()
    for epoch in range(2):
        table, caps, counts = res.tables()
        assert table.shape == (3, 4 * B) and counts == [4, 4, 3]
        got = [[(names[row[2 * B + b]], int(row[3 * B + b])) for b in range(n)] for row, n in zip(table, counts)]
        assert got == want[epoch]
        seen |= {bits for batch in got for _, bits in batch}
        assert all(int(row[3 * B + b]) == 0 for row, n in zip(table, counts) for b in range(n, B))
    assert random.random() == tail and seen <= {1, 2, 4, 3, 5, 6} and len(seen) >= 4
    plain = mmin.MMINResidentEpochs(_Trainer(), MMINDeviceStore(samples, None), B, torch.Generator().manual_seed(9))
    random.seed(31)
    assert plain.tables()[0].shape == (3, 3 * B) and random.random() == random.Random(31).random()      # no draw without keep bits


# ------------------------------------------------------------------------------------------------------------ flags, refusals
def _base_trainer(*argv):
    from track_mm.mmin_base import MMINBaseParams
    return mmin.MMINBaseTrainer(MMINBaseParams().from_args(["--train.batch_size=4"] + list(argv)), "cpu")


def test_flags_default_off_and_loaders():
    tr = _base_trainer()
    assert tr.eval_missing is False and tr.train_missing is False
    tr = _base_trainer("--eval_missing", "--train_missing", "--n_train=5", "--n_val=3", "--n_test=3", "--mmin_frames=3,20")
    assert tr.eval_missing and tr.train_missing
    random.seed(2)
    train, val, test = tr.make_loaders(tr.params)
    b = next(iter(train))
    assert "missing_type" in b and "audio_feature_reverse" not in b and tuple(b["missing_type"].shape) == (4, 3)
    for i, key in enumerate(mmin.MODAL_KEYS):
        gone = b["missing_type"][:, i] == 0
        assert not b[key][gone].any() and (b[key][~gone].any() or bool(gone.all()))
    assert "missing_type" not in next(iter(val)) and "missing_type" not in next(iter(test))
    assert mmin.MISSING_KEYS == ER.KEYS and mmin.MISSING_TYPES == MR.MISSING_TYPES


def test_mmin_miss_refuses_train_missing():
    from erc_amd.mmin_miss import MMINMissTrainer
    from track_mm.mmin_miss import MMINMissParams
    with pytest.raises(capi.ErcGraftError, match="--train_missing.*always masked"):
        MMINMissTrainer(MMINMissParams().from_args(["--train_missing"]), "cpu")


def test_new_capacity_paths_stay_refused_under_data_parallel(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    for argv in (("--eval_missing", "--device_collate", "--resident", "--resident_eval"), ("--train_missing", "--device_collate", "--resident"),
                 ("--train_missing", "--capacity_buckets=True")):
        with pytest.raises(capi.ErcGraftError, match="one rank"):
            _base_trainer(*argv)
    tr = _base_trainer("--eval_missing", "--train_missing")           # the default loop takes both flags
    assert tr.capacity is False and tr.eval_missing and tr.train_missing
