"""CPU: the CIM restatement (tests/cim_oracle.py) reproduces the reference's own CIMModule (golden vectors written by
tests/golden/make_golden_cim.py); the module keeps the reference's state_dict; the plugin surface and its refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.cim_oracle import cim_loss_and_grads
from tests.util_cases import check_grad_digest, fill_params

FIXTURES = ("cim_tiny", "cim_iemocap_c4", "cim_iemocap_c6")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixture_model(fx):
    from erc_amd.cim import CIMModule
    dims = dict(zip("atv", (int(v) for v in fx["dims"])))
    m = CIMModule(dims["t"], dims["a"], dims["v"], 200, int(fx["n_classes"]))
    fill_params(m, int(fx["param_seed"]))
    return m


@pytest.mark.parametrize("name", FIXTURES)
def test_cim_oracle_matches_reference(golden, name):
    fx = golden(name)
    m = _fixture_model(fx)
    P = {k: v.detach().clone() for k, v in m.state_dict().items()}
    batch = {k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("in_")}
    loss, l2, l7, grads, _ = cim_loss_and_grads(P, batch)
    assert float((l2 - torch.from_numpy(fx["logits2"])).abs().max()) < 1e-5
    assert float((l7 - torch.from_numpy(fx["logits7"])).abs().max()) < 1e-5
    assert abs(float(loss) - float(fx["loss"])) < 1e-6
    assert check_grad_digest(fx, [(k, g) for k, g in grads.items() if g is not None], 1e-4) < 1e-4
    assert sorted(k for k, g in grads.items() if g is None) == sorted(str(s) for s in fx["grad_none"])


@pytest.mark.parametrize("name", FIXTURES)
def test_cim_state_dict_matches_reference(golden, name):
    fx = golden(name)
    sd = _fixture_model(fx).state_dict()
    assert list(sd) == [str(k) for k in fx["sd_keys"]]
    assert [list(v.shape) for v in sd.values()] == [[int(d) for d in s if d >= 0] for s in fx["sd_shapes"]]


def test_cim_oracle_ignores_padded_features(golden):
    fx = golden("cim_tiny")
    P = {k: v.detach().clone() for k, v in _fixture_model(fx).state_dict().items()}
    batch = {k[3:]: torch.from_numpy(fx[k]).clone() for k in fx.files if k.startswith("in_")}
    base = cim_loss_and_grads(P, batch)[1]
    for key in ("text_feature", "audio_feature", "visual_feature"):
        x = batch[key]
        for b, L in enumerate(batch["text_length"].tolist()):
            x[b, L:] = 1e4
    assert torch.equal(cim_loss_and_grads(P, batch)[1], base)


def test_cim_params_defaults():
    from track_mm.cim import CIMParams
    p = CIMParams().from_args([])
    assert (p.seed, p.train.batch_size, p.val.batch_size, p.test.batch_size) == (1, 16, 32, 32)
    assert (p.dataset, p.epoch, p.num_heads, p.modality) == ("iemocap-cogmen-6", 55, 17, "atv")
    assert p.optim.name == "Adam" and p.optim.lr == 1e-3 and not p.optim.weight_decay
    assert p.apply_multi is False and p.apply_bin is True          # no MOSEI: the multi-task loss is off
    assert p.dims() == {"a": 100, "t": 100, "v": 512} and p.n_classes == 6


def test_train_mm_lists_cim():
    res = subprocess.run([sys.executable, "train_mm.py", "--module=nope"], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and "'cim'" in res.stdout


@pytest.mark.parametrize("args,msg", [(["--modality=at"], "--modality=atv"), (["--modality=t"], "--modality=atv"),
                                      (["--compute=bf16"], "fp32")])
def test_cim_trainer_refuses_unsupported_modes(args, msg):
    """the GRUs need text, audio and visual (the reference crashes on None); the reference is fp32"""
    from erc_amd.cim import CIMTrainer
    from track_mm.cim import CIMParams
    params = CIMParams().from_args(args)
    with pytest.raises(ValueError, match=msg):
        CIMTrainer(params, "cpu")


def test_cim_module_refuses_other_hidden_sizes():
    from erc_amd import capi
    from erc_amd.cim import CIMModule
    with pytest.raises(capi.ErcGraftError):
        CIMModule(100, 100, 512, 128, 6)
    with pytest.raises(capi.ErcGraftError):
        CIMModule(100, 100, 512, 200, 6, compute="bf16")
