"""CPU: the conv-emotion DialogueGCN restatement (tests/dgcnv2_oracle.py) reproduces the reference's own DGCNModule (golden
vectors written by tests/golden/make_golden_dgcnv2.py); the module keeps the reference's state_dict; the plugin surface and
its refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dgcnv2_oracle as O
from tests.util_cases import check_grad_digest, fill_params

FIXTURES = ("dgcnv2_s2", "dgcnv2_s9", "dgcnv2_none")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W6 = torch.tensor([1 / 0.086747, 1 / 0.144406, 1 / 0.227883, 1 / 0.160585, 1 / 0.127711, 1 / 0.252668])


def _fixture_model(fx):
    from erc_amd.dgcnv2 import DGCNModule
    m = DGCNModule(str(fx["base_model"]), input_size=int(fx["in_input_tensor"].shape[-1]), n_speakers=int(fx["n_speakers"]),
                   n_classes=int(fx["n_classes"]))
    fill_params(m, int(fx["param_seed"]))
    return m


def _batch(fx):
    return {k[3:]: torch.from_numpy(fx[k]).clone() for k in fx.files if k.startswith("in_")}


@pytest.mark.parametrize("name", FIXTURES)
def test_dgcnv2_oracle_matches_reference(golden, name):
    fx = golden(name)
    P = {k: v.detach().clone() for k, v in _fixture_model(fx).state_dict().items()}
    w = W6 if bool(fx["loss_weights"]) else None
    loss, logits, feats, grads = O.loss_and_grads(P, _batch(fx), str(fx["base_model"]), w)
    assert float((logits - torch.from_numpy(fx["logits"])).abs().max()) < 1e-5
    assert float((feats - torch.from_numpy(fx["features"])).abs().max()) < 1e-5
    assert abs(float(loss) - float(fx["loss"])) < 1e-5
    assert check_grad_digest(fx, [(k, g) for k, g in grads.items() if g is not None], 1e-4) < 1e-4
    assert sorted(k for k, g in grads.items() if g is None) == sorted(str(s) for s in fx["grad_none"])


@pytest.mark.parametrize("name", FIXTURES)
def test_dgcnv2_state_dict_matches_reference(golden, name):
    fx = golden(name)
    sd = _fixture_model(fx).state_dict()
    assert list(sd) == [str(k) for k in fx["sd_keys"]]
    assert [list(v.shape) for v in sd.values()] == [[int(d) for d in s if d >= 0] for s in fx["sd_shapes"]]


def test_dgcnv2_lstm_is_unpacked():
    """the reverse direction of a short dialogue starts inside its padding: the same dialogue batched with a longer one
    (larger T) gets different features and logits, while padded input rows stay zero"""
    fx = np.load(os.path.join(REPO, "tests", "golden", "dgcnv2_s2.npz"))
    P = {k: v.detach().clone() for k, v in _fixture_model(fx).state_dict().items()}
    b = _batch(fx)
    L = int(b["text_length"][0])                       # dialogue 0 (9 utterances) in a batch with T = 23
    alone = {"input_tensor": b["input_tensor"][:L, :1], "speaker_tensor": b["speaker_tensor"][:L, :1],
             "text_length": b["text_length"][:1], "label": b["label"][:L]}
    la, fa = O.forward(P, alone)
    lb, fb = O.forward(P, b)
    assert float((fa - fb[:L]).abs().max()) > 1e-4
    assert float((la - lb[:L]).abs().max()) > 1e-4
    assert torch.allclose(lb, torch.from_numpy(fx["logits"]), atol=1e-5)


def test_dgcnv2_params_defaults():
    from track_mm.dgcnv2 import DGCNParams
    p = DGCNParams().from_args([])
    assert (p.train.batch_size, p.val.batch_size, p.test.batch_size) == (32, 32, 32)
    assert (p.base_model, p.dataset, p.epoch, p.loss_weights) == ("LSTM", "iemocap-cogmen-6", 55, True)
    assert p.optim.name == "Adam" and p.optim.lr == 3e-4 and not p.optim.weight_decay
    assert p.speaker_onehot is True and p.batch_first is False
    assert p.n_classes == 6


def test_train_mm_lists_dgcnv2():
    res = subprocess.run([sys.executable, "train_mm.py", "--module=nope"], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and "'dgcnv2'" in res.stdout


@pytest.mark.parametrize("base", ["GRU", "DialogRNN"])
def test_dgcnv2_refuses_other_base_models(base):
    from erc_amd import capi
    from erc_amd.dgcnv2 import DGCNModule
    with pytest.raises(capi.ErcGraftError, match="base_model"):
        DGCNModule(base, input_size=16)


@pytest.mark.parametrize("args,msg", [(["--compute=bf16"], "fp32"), (["--compute=split"], "fp32"),
                                      (["--dataset=meld-mmgcn-7"], "loss_weights")])
def test_dgcnv2_trainer_refuses_unsupported_modes(args, msg):
    from erc_amd import capi
    from erc_amd.dgcnv2 import DGCNv2Trainer
    from track_mm.dgcnv2 import DGCNParams
    params = DGCNParams().from_args(args)
    with pytest.raises(capi.ErcGraftError, match=msg):
        DGCNv2Trainer(params, "cpu")


def test_dgcnv2_refuses_dialogues_longer_than_wscalar():
    """MaskedEdgeAttention.scalar has 110 rows: a batch with T = 111 is refused before anything is launched"""
    from erc_amd import capi
    from erc_amd.dgcnv2 import DGCNModule
    m = DGCNModule("LSTM", input_size=8, n_classes=6).finalize("cpu")
    T, B = 111, 2
    batch = {"input_tensor": torch.zeros(T, B, 8), "speaker_tensor": torch.zeros(T, B, 2),
             "text_length": torch.tensor([T, 3]), "attention_mask": torch.ones(B, T)}
    with pytest.raises(capi.ErcGraftError, match="110"):
        m(**batch)
    with pytest.raises(capi.ErcGraftError, match="fp32"):
        DGCNModule("LSTM", input_size=8, compute="bf16")
