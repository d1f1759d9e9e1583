"""CPU: CIM on CMU-MOSEI (--dataset=mosei-cim-2) -- the CIM-release reader against the reference's own mosei_cim
(tests/golden/mosei_cim_reader.npz, written by tests/golden/make_golden_cim_mosei.py from the tiny release in
tests/golden/mosei_cim/), parameters, synthetic videos, the collate and the device store, the multiemo metric block, the
multi-task restatement against the reference's own CIMModule, refusals and the C-ABI entry point."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.util_cases import check_grad_digest, fill_params

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOSEI_ROOT = os.path.join(REPO, "tests", "golden", "mosei_cim")


# ----------------------------------------------------------------------------------------------------- reader
@pytest.mark.parametrize("split", ["train", "test"])
def test_reader_matches_reference_bit_for_bit(golden, split):
    from erc_amd.datasets import read_dialogues
    fx = golden("mosei_cim_reader")
    got = read_dialogues("mosei-cim-2", split, MOSEI_ROOT)
    want = sorted({k for k in fx.files if k.startswith(split + "_")})
    n = len({k.split("_")[1] for k in want})
    assert len(got) == n and n > 0
    seen = set()
    for i, s in enumerate(got):
        for k, v in s.items():
            key = "%s_%d_%s" % (split, i, k)
            ref = fx[key]
            v = np.asarray(v)
            assert v.dtype == ref.dtype and v.shape == ref.shape and np.array_equal(v, ref), key
            seen.add(key)
    assert seen == set(want)


def test_reader_covers_the_edge_cases(golden):
    from erc_amd.datasets import read_dialogues
    train, test = (read_dialogues("mosei-cim-2", s, MOSEI_ROOT) for s in ("train", "test"))
    lens = [len(d["label"]) for d in train + test]
    assert 1 in lens and 98 in lens
    emo = np.concatenate([d["emo_label"] for d in train + test])
    assert emo.shape[1] == 7 and (emo[:, 6] == 1).any() and (emo.sum(1) >= 1).all()
    s7 = np.concatenate([d["senti7_label"] for d in train + test])
    assert set(s7.tolist()) == set(range(7))
    for d in train:
        assert d["speakers"] == [0] and d["text"].dtype == np.float32 and d["text"].shape[1] == 300
        assert d["audio"].shape[1] == 74 and d["visual"].shape[1] == 35
        assert np.array_equal(d["label"], d["senti2_label"])


def test_reader_refuses_val_and_uses_the_env_root(monkeypatch):
    from erc_amd.datasets import read_dialogues
    with pytest.raises(ValueError, match="train_idName|training ids"):
        read_dialogues("mosei-cim-2", "val", MOSEI_ROOT)
    monkeypatch.setenv("ERC_MOSEI_ROOT", MOSEI_ROOT)
    assert len(read_dialogues("mosei-cim-2", "test")) == 2


def test_binning_matches_reference_rules():
    from erc_amd.datasets import emotion_multi_hot, senti2, senti7
    a = np.array([-3, -2.0001, -2, -1.5, -1, -0.5, -0.0, 0, 0.5, 1, 1.5, 2, 2.5, 3])
    assert senti7(a).tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6]
    assert senti2(a).tolist() == [0] * 6 + [1] * 8
    with pytest.raises(ValueError):
        senti7(np.array([np.nan]))
    e = emotion_multi_hot(np.array([[0, 0, 0, 0, 0, 0], [0.3, 0, 0, 0, 0, 1.0]]))
    assert e.tolist() == [[0, 0, 0, 0, 0, 0, 1], [1, 0, 0, 0, 0, 1, 0]] and e.dtype == np.int64


# ----------------------------------------------------------------------------------------------------- parameters
def test_params_mosei_branch():
    from track_mm.cim import CIMParams
    p = CIMParams().from_args(["--dataset=mosei-cim-2"])
    assert (p.hidden_text, p.hidden_audio, p.hidden_visual, p.n_classes) == (300, 74, 35, 2)
    assert p.class_names == ["hap", "sad", "disgust", "fear", "surprise", "ang"]
    assert p.apply_multi is True and p.apply_bin is True and p.mosei_metric == "multiemo"
    q = CIMParams().from_args(["--dataset=iemocap-cogmen-6"])
    assert q.apply_multi is False and q.mosei_metric == ""
    r = CIMParams().from_args(["--dataset=mosei-cim-2", "--apply_multi=False"])
    assert r.apply_multi is False and r.mosei_metric == "multiemo"


def test_generic_params_mosei_metric_default():
    from erc_amd.params import ERCParams
    assert ERCParams().from_args(["--dataset=mosei-cim-2"]).mosei_metric == "multiemo"
    assert ERCParams().from_args(["--dataset=meld-mmgcn-7"]).mosei_metric == ""


# ----------------------------------------------------------------------------------------------------- batches
def _mosei_params(extra=()):
    from track_mm.cim import CIMParams
    return CIMParams().from_args(["--dataset=mosei-cim-2"] + list(extra))


def test_synthetic_mosei_videos():
    from erc_amd.trainer import load_dialogues
    p = _mosei_params(["--n_train=40", "--n_test=5"])
    train, test = load_dialogues(p)
    assert len(train) == 40 and len(test) == 5
    lens = [len(d["label"]) for d in train]
    assert min(lens) >= 1 and max(lens) <= 98
    emo = np.concatenate([d["emo_label"] for d in train])
    assert emo.shape[1] == 7 and (emo.sum(1) >= 1).all() and (emo[:, 6] == 1).any() and (emo[:, :6].sum(1) == 0).any()
    assert set(np.concatenate([d["label"] for d in train]).tolist()) == {0, 1}
    assert all(d["speakers"] == [0] for d in train)
    train2, _ = load_dialogues(p)
    assert all(np.array_equal(a["text"], b["text"]) for a, b in zip(train, train2))


def test_collate_carries_mosei_keys_only_for_mosei():
    from erc_amd.collate import ERCCollate
    from erc_amd.datasets import read_dialogues
    from erc_amd.params import ERCParams
    from erc_amd.synthetic import make_dialogues
    p = _mosei_params()
    dl = read_dialogues("mosei-cim-2", "train", MOSEI_ROOT)
    b = ERCCollate(p)([[d] for d in dl])
    N = sum(len(d["label"]) for d in dl)
    assert b["emo_label"].dtype == torch.int64 and tuple(b["emo_label"].shape) == (N, 7)
    assert b["senti2_label"].dtype == torch.int64 and torch.equal(b["senti2_label"], b["label"])
    assert torch.equal(b["emo_label"], torch.from_numpy(np.concatenate([d["emo_label"] for d in dl])))
    assert int(b["speaker_tensor"].abs().sum()) == 0
    q = ERCParams().from_args(["--dataset=iemocap-cogmen-6"])
    keys = set(ERCCollate(q)([[d] for d in make_dialogues(3, q.dims(), min_len=2, max_len=5)]))
    assert not keys & {"emo_label", "senti2_label"}


@pytest.mark.parametrize("synthetic", [False, True])
def test_device_store_equals_collate_on_mosei(synthetic):
    from erc_amd.collate import ERCCollate
    from erc_amd.datasets import DeviceDialogueStore, read_dialogues
    from erc_amd.synthetic import make_mosei_dialogues
    p = _mosei_params()
    dl = make_mosei_dialogues(7, p.dims(), max_len=20, seed=3) if synthetic else read_dialogues("mosei-cim-2", "train", MOSEI_ROOT)
    store = DeviceDialogueStore(dl, p, "cpu")
    idx = [2, 0, 1] if len(dl) > 2 else [1, 0]
    got = store.batch(torch.tensor(idx))
    want = ERCCollate(p)([[dl[i]] for i in idx])
    for k in ("attention_mask", "text_length", "text_feature", "audio_feature", "visual_feature", "input_tensor",
              "speaker_tensor", "label", "emo_label", "senti2_label"):
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


# ----------------------------------------------------------------------------------------------------- metrics
def _ref_weighted_accuracy(y_true, y_pred):
    """mmbase.py:231-251 restated"""
    TP, TN, FN, FP, N, P = 0, 0, 0, 0, 0, 0
    for i, j in zip(y_true, y_pred):
        if i == 1 and i == j:
            TP += 1
        elif i == 0 and i == j:
            TN += 1
        if i == 1 and i != j:
            FN += 1
        elif i == 0 and i != j:
            FP += 1
        if i == 1:
            P += 1
        else:
            N += 1
    return (1.0 * TP * (N / (1.0 * P)) + TN) / (2.0 * N)


def test_multiemo_report_matches_reference_restatement():
    from sklearn import metrics
    from erc_amd.trainer import multiemo_report
    rng = np.random.RandomState(4)
    true = (rng.rand(60, 7) < 0.3).astype(int)
    true[:, 6] = 0
    true[::5, 6] = 1
    prob = rng.rand(60, 7)
    rep = multiemo_report(true, prob)
    accs, f1s, was = [], [], []
    for i in range(7):
        col = (prob[:, i] > 0.5).astype(int)
        accs.append(metrics.accuracy_score(true[:, i], col))
        f1s.append(metrics.precision_recall_fscore_support(true[:, i], col, average="weighted")[2])
        was.append(_ref_weighted_accuracy(true[:, i], col))
    assert np.allclose(rep["acc"], accs, rtol=0, atol=1e-12) and np.allclose(rep["f1"], f1s, rtol=0, atol=1e-12)
    assert np.allclose(rep["wa"], was, rtol=0, atol=1e-12)
    assert abs(rep["mean_acc"] - np.mean(accs)) < 1e-12 and abs(rep["mean_f1"] - np.mean(f1s)) < 1e-12
    assert abs(rep["mean_wa"] - np.mean(was)) < 1e-12


def test_multiemo_report_null_for_degenerate_columns():
    from erc_amd.trainer import multiemo_report
    rng = np.random.RandomState(1)
    true = (rng.rand(30, 7) < 0.4).astype(int)
    true[:, 2] = 0          # no positives
    true[:, 4] = 1          # no negatives
    rep = multiemo_report(true, rng.rand(30, 7))
    assert rep["wa"][2] is None and rep["wa"][4] is None
    defined = [w for w in rep["wa"] if w is not None]
    assert len(defined) == 5 and abs(rep["mean_wa"] - np.mean(defined)) < 1e-12
    with pytest.raises(ZeroDivisionError):
        _ref_weighted_accuracy(true[:, 2], true[:, 2])


# ----------------------------------------------------------------------------------------------------- restatement
def test_multitask_oracle_matches_reference_fixture(golden):
    from erc_amd.cim import CIMModule
    from tests.cim_mosei_oracle import cim_mosei_loss_and_grads
    fx = golden("cim_mosei_c2")
    dims = dict(zip("atv", (int(v) for v in fx["dims"])))
    assert dims == dict(a=74, t=300, v=35)
    m = CIMModule(dims["t"], dims["a"], dims["v"], 200, int(fx["n_classes"]))
    fill_params(m, int(fx["param_seed"]))
    P = {k: v.detach().clone() for k, v in m.state_dict().items()}
    batch = {k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("in_")}
    losses, l2, l7, grads, _ = cim_mosei_loss_and_grads(P, batch)
    assert float((l2 - torch.from_numpy(fx["logits2"])).abs().max()) < 1e-5
    assert float((l7 - torch.from_numpy(fx["logits7"])).abs().max()) < 1e-5
    for k in ("Lall", "Lce", "Lmulti"):
        assert abs(float(losses[k]) - float(fx[k])) < 1e-5, k
    assert check_grad_digest(fx, [(k, g) for k, g in grads.items() if g is not None], 1e-5) < 1e-5
    none = sorted(k for k, g in grads.items() if g is None)
    assert none == sorted(str(s) for s in fx["grad_none"]) and all(k.startswith("rnn_adapter.") for k in none)


def test_multitask_layout_puts_both_heads_back_to_back():
    """live_groups: cls2 | cls7 weights in one group and biases in another -- one [C + 7, 900] head; without multitask the
    groups are the single-task ones"""
    from erc_amd.cim import CIMModule
    m = CIMModule(300, 74, 35, 200, 2, multitask=True)
    g = m.live_groups()
    names = [[n for n, _ in grp] for grp in g]
    assert ["cls2.weight", "cls7.weight"] in names and ["cls2.bias", "cls7.bias"] in names
    single = [[n for n, _ in grp] for grp in CIMModule(300, 74, 35, 200, 2).live_groups()]
    assert ["cls2.weight"] in single and not any("cls7" in n for grp in single for n in grp)
    assert single[:-2] == names[:-2]


# ----------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("module", ["cogmen", "dagerc", "mmgcn", "dgcn", "dgcnv2"])
def test_other_modules_refuse_mosei(module):
    res = subprocess.run([sys.executable, "train_mm.py", "--module=" + module, "--dataset=mosei-cim-2", "--epoch=1"], cwd=REPO,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode != 0
    assert "only --module=cim trains on CMU-MOSEI" in res.stderr, res.stderr[-2000:]


def test_cim_refuses_apply_bin_false():
    from erc_amd import capi
    from erc_amd.cim import CIMTrainer
    with pytest.raises(capi.ErcGraftError, match="apply_bin"):
        CIMTrainer(_mosei_params(["--apply_bin=False"]), "cpu")


def test_cim_on_mosei_passes_the_refusal_check():
    """--module=cim on MOSEI gets past the dataset check; without a GPU it stops at the device check instead"""
    res = subprocess.run([sys.executable, "train_mm.py", "--module=cim", "--dataset=mosei-cim-2", "--epoch=1"], cwd=REPO,
                         capture_output=True, text=True, timeout=300, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert "only --module=cim" not in res.stderr


def test_cabi_exports_the_multitask_loss():
    from erc_amd import capi
    assert "erc_ce_bce_multitask" in capi.EXPORTS
    capi.build()
    assert hasattr(capi.lib(), "erc_ce_bce_multitask")
    rc = capi.lib().erc_ce_bce_multitask(None, 9, 2, 4, None, None, 7, 1.0, 1.0, 1.0, None, 9, None, None)
    assert rc == -1 and b"ce_bce_multitask" in capi.lib().erc_last_error()
