"""CPU: the bc-LSTM / bc-GRU restatement (tests/bcrnn_oracle.py) reproduces the reference's own LSTMModel, GRUModel and
MaskedNLLLoss (golden vectors written by tests/golden/make_golden_bcrnn.py); the modules keep the reference's state_dict;
the RNNs are unpacked (a dialogue alone differs from the same dialogue in its batch); the plugin surface and its refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import bcrnn_oracle as O
from tests.util_cases import check_grad_digest, fill_params

FIXTURES = (("bclstm_s2", "lstm"), ("bclstm_s9", "lstm"), ("bcgru_s2", "gru"), ("bcgru_s9", "gru"))
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W6 = torch.tensor([1 / 0.086747, 1 / 0.144406, 1 / 0.227883, 1 / 0.160585, 1 / 0.127711, 1 / 0.252668])


def _cls(cell):
    from erc_amd import bcrnn
    return bcrnn.LSTMModule if cell == "lstm" else bcrnn.GRUModule


def _fixture_model(fx, cell):
    m = _cls(cell)(int(fx["in_input_tensor"].shape[-1]), 100, 100, n_classes=int(fx["n_classes"]))
    fill_params(m, int(fx["param_seed"]))
    return m


def _batch(fx):
    return {k[3:]: torch.from_numpy(fx[k]).clone() for k in fx.files if k.startswith("in_")}


@pytest.mark.parametrize("name,cell", FIXTURES)
def test_bcrnn_oracle_matches_reference(golden, name, cell):
    fx = golden(name)
    P = {k: v.detach().clone() for k, v in _fixture_model(fx, cell).state_dict().items()}
    w = W6 if bool(fx["loss_weights"]) else None
    loss, log_prob, emo, grads = O.loss_and_grads(P, _batch(fx), cell, w)
    assert float((log_prob - torch.from_numpy(fx["log_prob"])).abs().max()) < 1e-5
    assert float((emo - torch.from_numpy(fx["emotions"])).abs().max()) < 1e-5
    assert abs(float(loss) - float(fx["loss"])) < 1e-5
    assert len(grads) == 22 and all(g is not None for g in grads.values())
    assert check_grad_digest(fx, list(grads.items()), 1e-4) < 1e-4
    assert [str(s) for s in fx["grad_none"]] == []


@pytest.mark.parametrize("name,cell", FIXTURES)
def test_bcrnn_state_dict_matches_reference(golden, name, cell):
    fx = golden(name)
    m = _fixture_model(fx, cell)
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in fx["sd_keys"]]
    assert [list(v.shape) for v in sd.values()] == [[int(d) for d in s if d >= 0] for s in fx["sd_shapes"]]
    assert sum(k.startswith(cell + ".") for k in sd) == 16
    live = sorted(n for grp in m.live_groups() for n, _ in grp)
    assert live == sorted(sd) and len(live) == 22          # every parameter is live


def test_gru_scan_is_the_layer_and_torch_gru():
    """the per-dialogue chain the kernel test uses (gru_scan), the batched layer of the whole-model paths and torch.nn.GRU
    agree in float64"""
    torch.manual_seed(3)
    gru = torch.nn.GRU(12, 100, num_layers=1, bidirectional=True).double()
    x = torch.randn(9, 3, 12, dtype=torch.float64)
    want = gru(x)[0].detach()
    for d, sfx in enumerate(("", "_reverse")):
        w = [getattr(gru, n + "_l0" + sfx).detach() for n in ("weight_ih", "bias_ih", "weight_hh", "bias_hh")]
        a, b = O.gru_layer(x, *w, reverse=bool(d)), O.gru_layer_batched(x, *w, reverse=bool(d))
        assert float((a - want[..., 100 * d:100 * d + 100]).abs().max()) < 1e-12
        assert float((a - b).abs().max()) < 1e-12


@pytest.mark.parametrize("name,cell", [("bclstm_s2", "lstm"), ("bcgru_s2", "gru")])
def test_bcrnn_is_unpacked(golden, name, cell):
    """both RNNs run over the padded tensor: the reverse direction of a short dialogue starts inside the zero padding, so a
    dialogue alone differs from the same dialogue inside a longer batch by more than 1e-4 (measured on the reference:
    1.4e-3 .. 5.3e-3); the longest dialogue of the batch has no padding and is the same either way"""
    fx = golden(name)
    P = {k: v.detach().clone() for k, v in _fixture_model(fx, cell).state_dict().items()}
    b = _batch(fx)
    lb, eb = O.forward(P, b, cell)
    assert torch.allclose(lb, torch.from_numpy(fx["log_prob"]), atol=1e-5)
    lens, off = [int(v) for v in b["text_length"]], 0
    for i, L in enumerate(lens):
        alone = {"input_tensor": b["input_tensor"][:L, i:i + 1], "speaker_tensor": b["speaker_tensor"][:L, i:i + 1],
                 "text_length": b["text_length"][i:i + 1], "label": b["label"][off:off + L]}
        la, ea = O.forward(P, alone, cell)
        diff = float((la - lb[off:off + L]).abs().max())
        if L == max(lens):
            assert diff < 1e-5
        else:
            assert diff > 1e-4, (L, diff)
        off += L


def test_bcrnn_params_defaults():
    from track_mm.bclstm import BcRnnParams
    from track_mm import bcgru, bclstm
    assert bcgru.ParamsType is bclstm.ParamsType is BcRnnParams
    p = BcRnnParams().from_args([])
    assert (p.train.batch_size, p.val.batch_size, p.test.batch_size) == (32, 32, 32)
    assert (p.dataset, p.epoch, p.loss_weights) == ("iemocap-cogmen-6", 55, True)
    assert p.optim.name == "Adam" and p.optim.lr == 3e-4 and not p.optim.weight_decay
    assert p.speaker_onehot is True and p.batch_first is False
    assert p.dropout == 0.5
    assert p.n_classes == 6
    assert bclstm.main.func is bcgru.main.func
    assert bclstm.main.args[0].MODULE.CELL == "lstm" and bcgru.main.args[0].MODULE.CELL == "gru"


def test_train_mm_lists_bclstm_and_bcgru():
    res = subprocess.run([sys.executable, "train_mm.py", "--module=nope"], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and "'bclstm'" in res.stdout and "'bcgru'" in res.stdout


@pytest.mark.parametrize("cell", ["lstm", "gru"])
@pytest.mark.parametrize("kwargs,msg", [(dict(D_e=150), "D_e"), (dict(D_e=200), "D_e"), (dict(D_h=64), "D_h"),
                                        (dict(compute="bf16"), "fp32"), (dict(dropout=1.0), "dropout")])
def test_bcrnn_refuses_what_is_not_built(cell, kwargs, msg):
    from erc_amd import capi
    args = dict(D_m=16, D_e=100, D_h=100)
    args.update(kwargs)
    with pytest.raises(capi.ErcGraftError, match=msg):
        _cls(cell)(**args)


@pytest.mark.parametrize("mod", ["bclstm", "bcgru"])
@pytest.mark.parametrize("args,msg", [(["--compute=bf16"], "fp32"), (["--compute=split"], "fp32"),
                                      (["--dataset=meld-mmgcn-7"], "loss_weights")])
def test_bcrnn_trainer_refuses_unsupported_modes(mod, args, msg):
    import importlib
    from erc_amd import capi
    plugin = importlib.import_module("track_mm." + mod)
    params = plugin.ParamsType().from_args(args)
    with pytest.raises(capi.ErcGraftError, match=msg):
        plugin.main.args[0](params, "cpu")


@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_bcrnn_refuses_long_dialogues_and_att2_false(cell):
    """the 200-wide matching attention is built for T <= 110: a batch with T = 111 is refused before anything is launched;
    so is att2=False"""
    from erc_amd import capi
    m = _cls(cell)(8, 100, 100, n_classes=6).finalize("cpu")
    T, B = 111, 2
    batch = {"input_tensor": torch.zeros(T, B, 8), "speaker_tensor": torch.zeros(T, B, 2),
             "text_length": torch.tensor([T, 3]), "attention_mask": torch.ones(B, T)}
    with pytest.raises(capi.ErcGraftError, match="110"):
        m(**batch)
    batch = {"input_tensor": torch.zeros(5, B, 8), "speaker_tensor": torch.zeros(5, B, 2),
             "text_length": torch.tensor([5, 3]), "attention_mask": torch.ones(B, 5)}
    with pytest.raises(capi.ErcGraftError, match="att2"):
        m(att2=False, **batch)
    with pytest.raises(capi.ErcGraftError, match="features"):
        m(**dict(batch, input_tensor=torch.zeros(5, B, 9)))
