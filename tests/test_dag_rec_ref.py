"""The float64 reference of the DAG-ERC recurrence (tests/dag_rec_ref.py) against the reference-pinned fp32 oracle
(oracle/dagerc.py DAGERCOracle): the layer outputs H_1 .. H_L as the oracle's own forward produces them, and the gradient
of every parameter of grus_c, grus_p and gather (and of the input features, which carries the masked gradient wrt H_0) for
a random head gradient.  Small ragged batches with 1, 2 and 3 speakers, 1, 4 and 5 layers.  Runs without a GPU.

Bounds: the oracle is fp32, so the comparison carries ITS rounding: 2e-5 of the tensor's scale (a correct fp32 recurrence
is within 1e-6 of float64 at these sizes, see the yardsticks in tests/test_gpu_dag_rec.py; the oracle's gradients go
through up to 5 layers of 14 steps)."""
import numpy as np
import pytest
import torch

from oracle.dagerc import DAGERCOracle
from tests.dag_rec_ref import HID, PARAMS, contract_products, dag_rec_ref, layers_from_oracle, one_thread, rel
from tests.util_cases import make_batch

TOL = 2e-5


def _oracle_run(S, L, seed):
    dims = dict(a=10, t=14, v=8)
    batch = make_batch(4, dims, n_speakers=S, n_classes=5, min_len=1, max_len=14, seed=seed, speaker_onehot=False,
                       force_max=True)
    torch.manual_seed(seed)
    ref = DAGERCOracle(emb_dim=sum(dims.values()), dropout=0.0, n_classes=5, gnn_layers=L)
    x = batch["input_tensor"].clone().requires_grad_(True)
    seen = {}
    # the concatenation [H_0 | H_1 | .. | H_L | x] the oracle's own forward hands to its head
    ref.attentive_node_features.register_forward_hook(lambda mod, args, out: seen.update(H=args[0]))
    with one_thread():
        ref(input_tensor=x, text_length=batch["text_length"], speaker_tensor=batch["speaker_tensor"])
        Hcat = seen["H"][:, :, :HID * (L + 1)]
        G = torch.randn(Hcat.shape, generator=torch.Generator().manual_seed(seed + 1))
        (Hcat * G).sum().backward()
    return ref, batch, x, Hcat.detach(), G


@pytest.mark.parametrize("S,L", [(1, 1), (2, 4), (3, 5), (3, 1), (1, 4), (2, 5)])
def test_reference_matches_oracle(S, L):
    ref, batch, x, Hcat, G = _oracle_run(S, L, seed=10 * S + L)
    spk = batch["speaker_tensor"].numpy()
    assert spk.ndim == 2 and len(np.unique(spk)) == S
    with one_thread():
        out = dag_rec_ref(Hcat[:, :, :HID], layers_from_oracle(ref), spk, dHall=G)
    assert len(out) == L
    for l in range(L):
        assert rel(out[l]["H1"], Hcat[:, :, HID * (l + 1):HID * (l + 2)]) < TOL, l
        o, c, p, g = out[l], ref.grus_c[l], ref.grus_p[l], ref.gather[l]
        want = {"grus_c.weight_ih": (o["dWh"][:3 * HID], c.weight_ih), "grus_p.weight_hh": (o["dWh"][3 * HID:6 * HID], p.weight_hh),
                "grus_c.bias_ih": (o["dbh"][:3 * HID], c.bias_ih), "grus_p.bias_hh": (o["dbh"][3 * HID:6 * HID], p.bias_hh),
                "grus_c.weight_hh": (o["dW_hh_c"], c.weight_hh), "grus_c.bias_hh": (o["db_hh_c"], c.bias_hh),
                "grus_p.weight_ih": (o["dW_ih_p"], p.weight_ih), "grus_p.bias_ih": (o["db_ih_p"], p.bias_ih),
                "gather.linear.weight": (torch.cat([o["dWh"][6 * HID], o["dw_k"]])[None], g.linear.weight),
                "gather.linear.bias": (o["dbh"][6 * HID:], g.linear.bias),
                "gather.Wr0.weight": (o["dWr"][:HID], g.Wr0.weight), "gather.Wr1.weight": (o["dWr"][HID:], g.Wr1.weight)}
        assert set("d" + k for k in PARAMS) <= set(o)
        for name, (mine, prm) in want.items():
            if S == 1 and name == "gather.Wr1.weight":      # one speaker: Wr1 is never used
                assert float(mine.abs().max()) == 0 and float(prm.grad.abs().max()) == 0
                continue
            if name == "gather.linear.bias" or (S == 1 and name == "gather.linear.weight"):
                # a softmax ignores a shift of its scores, so the bias has no gradient; with one speaker every window has
                # length 1 and the weights have none either (fp32 leaves rounding noise)
                assert float(mine.abs().max()) < 1e-12 and float(prm.grad.abs().max()) < 1e-5
                continue
            assert rel(mine, prm.grad) < TOL, (l, name)
    # the masked gradient wrt H_0, seen through fc1: dx = dH0 fc1.weight
    dx = out[0]["dH0"] @ ref.fc1.weight.detach().double()
    assert rel(dx, x.grad) < TOL


def test_contract_products_reproduce_the_autograd_gradients():
    """the statement of include/ercgraft.h that DAGERCModule.loss_and_grads relies on, within the reference itself:
    DGI^T H_l, DGH^T Mseq, dM^T A, dks^T H1 and the column sums equal the autograd gradients"""
    ref, batch, x, Hcat, G = _oracle_run(3, 4, seed=77)
    out = dag_rec_ref(Hcat[:, :, :HID], layers_from_oracle(ref), batch["speaker_tensor"].numpy(), dHall=G)
    Hl = Hcat[:, :, :HID].double()
    for o in out:
        for k, v in contract_products(o, Hl).items():
            assert rel(v, o[k]) < 1e-12, k
        Hl = o["H1"]


def test_leaving_out_the_zero_weights_changes_nothing():
    """dag_rec_ref leaves the utterances before the batch's earliest window start out of the weighted sum (their weights
    are exactly 0.0); spelled out over the whole prefix it gives the same values and gradients: alpha bit for bit, the
    rest up to the order of a float64 sum"""
    ref, batch, x, Hcat, G = _oracle_run(2, 4, seed=5)
    spk = batch["speaker_tensor"].numpy()
    with one_thread():
        a = dag_rec_ref(Hcat[:, :, :HID], layers_from_oracle(ref), spk, dHall=G)
        b = dag_rec_ref(Hcat[:, :, :HID], layers_from_oracle(ref), spk, dHall=G, full_prefix=True)
    for oa, ob in zip(a, b):
        assert torch.equal(oa["alpha"], ob["alpha"])
        assert float(oa["alpha"].sum(2)[:, 1:].sub(1).abs().max()) < 1e-14
        for k in ob:
            assert rel(oa[k], ob[k]) < 1e-13, k
