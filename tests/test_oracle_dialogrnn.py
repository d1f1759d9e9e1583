"""CPU: the DialogueRNN restatement (tests/dialogrnn_oracle.py) reproduces the reference's own DialogRNNModel and
MaskedNLLLoss (golden vectors written by tests/golden/make_golden_dialogrnn.py); the module keeps the reference's
state_dict; padding never reaches a valid row; the plugin surface and its refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dialogrnn_oracle as O
from tests.util_cases import check_grad_digest, fill_params

FIXTURES = ("dialogrnn_s2", "dialogrnn_s9", "dialogrnn_pad0")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W6 = torch.tensor([1 / 0.086747, 1 / 0.144406, 1 / 0.227883, 1 / 0.160585, 1 / 0.127711, 1 / 0.252668])


def _fixture_model(fx):
    from erc_amd.dialogrnn import DialogRNNModule
    m = DialogRNNModule(int(fx["in_input_tensor"].shape[-1]), 150, 150, 100, 100, n_classes=int(fx["n_classes"]),
                        context_attention="general")
    fill_params(m, int(fx["param_seed"]))
    return m


def _batch(fx):
    return {k[3:]: torch.from_numpy(fx[k]).clone() for k in fx.files if k.startswith("in_")}


def _load(name):
    return np.load(os.path.join(REPO, "tests", "golden", name + ".npz"))


@pytest.mark.parametrize("name", FIXTURES)
def test_dialogrnn_oracle_matches_reference(golden, name):
    fx = golden(name)
    P = {k: v.detach().clone() for k, v in _fixture_model(fx).state_dict().items()}
    w = W6 if bool(fx["loss_weights"]) else None
    loss, log_prob, emo, grads = O.loss_and_grads(P, _batch(fx), w)
    assert float((log_prob - torch.from_numpy(fx["log_prob"])).abs().max()) < 1e-5
    assert float((emo - torch.from_numpy(fx["emotions"])).abs().max()) < 1e-5
    assert abs(float(loss) - float(fx["loss"])) < 1e-5
    assert len(grads) == 32 and all(g is not None for g in grads.values())
    assert check_grad_digest(fx, list(grads.items()), 1e-4) < 1e-4
    assert [str(s) for s in fx["grad_none"]] == []


@pytest.mark.parametrize("name", FIXTURES)
def test_dialogrnn_state_dict_matches_reference(golden, name):
    fx = golden(name)
    m = _fixture_model(fx)
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in fx["sd_keys"]]
    assert [list(v.shape) for v in sd.values()] == [[int(d) for d in s if d >= 0] for s in fx["sd_shapes"]]
    live = sorted(n for grp in m.live_groups() for n, _ in grp)
    assert live == sorted(sd) and len(live) == 32          # every parameter is live


def test_dialogrnn_speaker_padding_does_not_reach_valid_rows():
    """zero pad rows of the speaker tensor and the speaker-0 one-hot pad rows of the real collate give the same valid rows,
    in the reference (the two fixtures) and in the restatement"""
    a, b = _load("dialogrnn_s2"), _load("dialogrnn_pad0")
    assert not np.array_equal(a["in_speaker_tensor"], b["in_speaker_tensor"])
    assert np.array_equal(a["in_input_tensor"], b["in_input_tensor"])
    assert np.array_equal(a["log_prob"], b["log_prob"]) and np.array_equal(a["emotions"], b["emotions"])
    assert float(a["loss"]) == float(b["loss"])
    P = {k: v.detach().clone() for k, v in _fixture_model(a).state_dict().items()}
    la, ea = O.forward(P, _batch(a))
    lb, eb = O.forward(P, _batch(b))
    assert torch.equal(la, lb) and torch.equal(ea, eb)


def test_dialogrnn_dialogue_alone_equals_dialogue_in_batch():
    """the property that lets the kernel skip padded steps (the opposite of test_dgcnv2_lstm_is_unpacked): a dialogue alone
    and the same dialogue batched with longer ones give the same rows within 1e-6"""
    fx = _load("dialogrnn_s2")
    P = {k: v.detach().clone() for k, v in _fixture_model(fx).state_dict().items()}
    b = _batch(fx)
    lb, eb = O.forward(P, b)
    assert torch.allclose(lb, torch.from_numpy(fx["log_prob"]), atol=1e-5)
    lens, off = [int(v) for v in b["text_length"]], 0
    for i, L in enumerate(lens):
        alone = {"input_tensor": b["input_tensor"][:L, i:i + 1], "speaker_tensor": b["speaker_tensor"][:L, i:i + 1],
                 "text_length": b["text_length"][i:i + 1], "label": b["label"][off:off + L]}
        la, ea = O.forward(P, alone)
        assert float((ea - eb[off:off + L]).abs().max()) < 1e-6
        assert float((la - lb[off:off + L]).abs().max()) < 1e-6
        assert torch.allclose(ea, torch.from_numpy(fx["emotions"][off:off + L]), atol=1e-5)   # ... and the reference's rows
        off += L


def test_dialogrnn_params_defaults():
    from track_mm.dialogrnn import DialogRNNParams
    p = DialogRNNParams().from_args([])
    assert (p.train.batch_size, p.val.batch_size, p.test.batch_size) == (32, 32, 32)
    assert (p.dataset, p.epoch, p.loss_weights) == ("iemocap-cogmen-6", 55, True)
    assert p.optim.name == "Adam" and p.optim.lr == 3e-4 and not p.optim.weight_decay
    assert p.speaker_onehot is True and p.batch_first is False
    assert (p.dropout_rec, p.dropout) == (0.5, 0.5)
    assert p.n_classes == 6


def test_train_mm_lists_dialogrnn():
    res = subprocess.run([sys.executable, "train_mm.py", "--module=nope"], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and "'dialogrnn'" in res.stdout


@pytest.mark.parametrize("kwargs,msg", [(dict(listener_state=True), "listener_state"),
                                        (dict(context_attention="simple"), "context_attention"),
                                        (dict(context_attention="dot"), "context_attention"),
                                        (dict(context_attention="concat"), "context_attention"),
                                        (dict(context_attention="general2"), "context_attention"),
                                        (dict(D_g=200), "D_g"), (dict(D_p=100), "D_p"), (dict(D_e=150), "D_e"),
                                        (dict(D_h=64), "D_h"), (dict(compute="bf16"), "fp32")])
def test_dialogrnn_refuses_what_is_not_built(kwargs, msg):
    from erc_amd import capi
    from erc_amd.dialogrnn import DialogRNNModule
    args = dict(D_m=16, D_g=150, D_p=150, D_e=100, D_h=100, context_attention="general")
    args.update(kwargs)
    with pytest.raises(capi.ErcGraftError, match=msg):
        DialogRNNModule(**args)


def test_dialogrnn_default_attention_of_the_signature_is_refused():
    """the constructor keeps the reference's signature, whose default context_attention is 'simple': not built"""
    from erc_amd import capi
    from erc_amd.dialogrnn import DialogRNNModule
    with pytest.raises(capi.ErcGraftError, match="context_attention"):
        DialogRNNModule(16, 150, 150, 100, 100)


@pytest.mark.parametrize("args,msg", [(["--compute=bf16"], "fp32"), (["--compute=split"], "fp32"),
                                      (["--dataset=meld-mmgcn-7"], "loss_weights")])
def test_dialogrnn_trainer_refuses_unsupported_modes(args, msg):
    from erc_amd import capi
    from erc_amd.dialogrnn import DialogRNNTrainer
    from track_mm.dialogrnn import DialogRNNParams
    params = DialogRNNParams().from_args(args)
    with pytest.raises(capi.ErcGraftError, match=msg):
        DialogRNNTrainer(params, "cpu")


def test_dialogrnn_refuses_dialogues_longer_than_the_history():
    """the scan keeps 110 global states in LDS: a batch with T = 111 is refused before anything is launched"""
    from erc_amd import capi
    from erc_amd.dialogrnn import DialogRNNModule
    m = DialogRNNModule(8, 150, 150, 100, 100, n_classes=6, context_attention="general").finalize("cpu")
    T, B = 111, 2
    batch = {"input_tensor": torch.zeros(T, B, 8), "speaker_tensor": torch.zeros(T, B, 2),
             "text_length": torch.tensor([T, 3]), "attention_mask": torch.ones(B, T)}
    with pytest.raises(capi.ErcGraftError, match="110"):
        m(**batch)
    batch = {"input_tensor": torch.zeros(5, B, 8), "speaker_tensor": torch.zeros(5, B, 10),
             "text_length": torch.tensor([5, 3]), "attention_mask": torch.ones(B, 5)}
    with pytest.raises(capi.ErcGraftError, match="n_speakers"):
        m(**batch)
