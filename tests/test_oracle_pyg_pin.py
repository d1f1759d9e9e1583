"""CPU: the restated PyG operators of oracle/pyg.py -- RGCNConvMean (COGMEN's gcn.conv1) and GraphConvAdd (DialogueGCN's
gcn.conv2) -- against the vendored PyG 1.4.2 RGCNConv the reference ships, set up as each operator (golden vectors written by
tests/golden/make_golden_pyg_pin.py).  Forward output and the gradients of the input and of every parameter for a fixed output
gradient, fp32 on both sides."""
import pytest
import torch

from oracle import graph as og
from oracle.pyg import GraphConvAdd, RGCNConvMean
from tests.util_cases import fill_params, rel_err

TOL = 1e-5     # of each tensor's scale


def _t(fx, key):
    return torch.from_numpy(fx[key])


def _graph_matches_fixture(fx):
    """the oracle's window graph on the fixture's dialogues is the reference's (the fixture's edge list)"""
    lengths, spk = _t(fx, "lengths"), _t(fx, "speakers")
    feats = torch.zeros(lengths.numel(), int(lengths.max()), 1)
    _, ei, et, _ = og.window_graph_loop(feats, lengths, spk, int(fx["wp"]), int(fx["wf"]), int(fx["n_speakers"]))
    ei_s, et_s = og.canonical_edges(ei.numpy(), et.numpy())
    assert (ei_s == fx["edge_index"]).all()
    if "edge_type" in fx.files:
        assert (et_s == fx["edge_type"]).all()


def _close(got, fx, key):
    e = rel_err(got.detach(), _t(fx, key))
    assert e < TOL, (key, e)
    return e


@pytest.mark.parametrize("name", ["rgcn_mean_s2", "rgcn_mean_s3"])
def test_rgcn_conv_mean_matches_vendored_rgcn(golden, name):
    """RGCNConvMean == RGCNConv(num_bases=R, att=I, edge_norm = 1 / per-relation in-degree).  The S = 3 graph has relation ids
    >= 8 that COGMEN's R = 8 ignores: the oracle gets every edge, the reference call got only the edges with ids < 8."""
    fx = golden(name)
    _graph_matches_fixture(fx)
    R = int(fx["num_relations"])
    keep = _t(fx, "in_reference_call")
    assert bool((keep == (_t(fx, "edge_type") < R)).all())
    if name.endswith("s3"):
        assert not bool(keep.all())
    conv = RGCNConvMean(100, 100, R)
    fill_params(conv, int(fx["param_seed"]))
    x = _t(fx, "x").clone().requires_grad_(True)
    out = conv(x, _t(fx, "edge_index"), _t(fx, "edge_type"))
    _close(out, fx, "out")
    out.backward(_t(fx, "gout"))
    _close(x.grad, fx, "dx")
    _close(conv.weight.grad, fx, "dweight")
    _close(conv.root.grad, fx, "droot")
    _close(conv.bias.grad, fx, "dbias")


@pytest.mark.parametrize("name", ["graphconv_add", "graphconv_add_w2_4"])
def test_graph_conv_add_matches_vendored_rgcn(golden, name):
    """GraphConvAdd == RGCNConv(R = 1, att = [[1]], no edge_norm) with basis[0] = lin_rel.weight^T, root = lin_root.weight^T,
    bias = lin_rel.bias.  The second graph has an asymmetric window (2 past / 4 future): the message direction shows."""
    fx = golden(name)
    _graph_matches_fixture(fx)
    conv = GraphConvAdd(100, 100)
    fill_params(conv, int(fx["param_seed"]))
    x = _t(fx, "x").clone().requires_grad_(True)
    out = conv(x, _t(fx, "edge_index"))
    _close(out, fx, "out")
    out.backward(_t(fx, "gout"))
    _close(x.grad, fx, "dx")
    _close(conv.lin_rel.weight.grad, fx, "dlin_rel_weight")
    _close(conv.lin_rel.bias.grad, fx, "dlin_rel_bias")
    _close(conv.lin_root.weight.grad, fx, "dlin_root_weight")
