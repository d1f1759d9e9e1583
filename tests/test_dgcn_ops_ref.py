"""CPU: tests/dgcn_ops_ref.py (the float64 reference of tests/test_gpu_dgcn_ops.py) is the oracle's EdgeAtt + batch_graphify +
RGCNConv -- oracle.dgcn, which tests/test_oracle_dgcn.py ties to the reference's own files -- and reproduces the reference
fixtures; the host-built edge list is the fixtures'."""
import numpy as np
import pytest
import torch

from oracle import graph as og
from oracle.dgcn import EdgeAtt, RGCNConvBasis, dgcn_graphify
from tests import dgcn_ops_ref as ref
from tests.util_cases import check_grad_digest, fill_params, rel_err

NB = ref.NB


def _params(S, Fd, O, att_seed, conv_seed):
    att = EdgeAtt(Fd, 10, 10)
    fill_params(att, att_seed)
    conv = RGCNConvBasis(Fd, O, 2 * S * S, NB)
    fill_params(conv, conv_seed)
    return att, conv


def _nodes(feats, lengths):
    return torch.cat([feats[b, :int(L)] for b, L in enumerate(lengths)], 0)


@pytest.mark.parametrize("S,lengths", [(2, (1, 17, 12, 2)), (9, (23, 1, 14))], ids=["s2", "s9"])
def test_restatement_is_the_oracle_in_float64(S, lengths):
    Fd, O, R = 24, 10, 2 * S * S
    g = torch.Generator().manual_seed(7 + S)
    B, T = len(lengths), max(lengths)
    assert sum(lengths) <= 40
    feats = torch.randn(B, T, Fd, generator=g)
    spk = torch.randint(0, S, (B, T), generator=g)
    gout = torch.randn(sum(lengths), O, generator=g)
    att, conv = _params(S, Fd, O, 3, 4)
    with torch.no_grad():
        att.weight.mul_(3.0)                              # scores of order 1: a softmax that is not nearly uniform
    ei, et = ref.host_graph(lengths, spk, 10, 10, S)
    mine = ref.restate(ei, et, R, _nodes(feats, lengths), att.weight, conv.att, conv.basis, conv.root, conv.bias, gout)
    torch.set_default_dtype(torch.float64)                # (EdgeAtt allocates its alpha table in the default dtype)
    try:
        att, conv = att.double(), conv.double()
        f64 = feats.double().requires_grad_()
        x, oei, onorm, oet = dgcn_graphify(f64, torch.tensor(lengths), spk, 10, 10, S, att)
        out = conv(x, oei, oet, onorm)
        onorm.retain_grad()
        out.backward(gout.double())
    finally:
        torch.set_default_dtype(torch.float32)
    order = np.lexsort((oei[0].numpy(), oei[1].numpy()))
    assert torch.equal(oei[:, order], ei) and torch.equal(oet[order], et)
    want = dict(norm=onorm.detach()[order], out=out.detach(), dx=_nodes(f64.grad, lengths), dW=att.weight.grad, dbasis=conv.basis.grad,
                dcomp=conv.att.grad, droot=conv.root.grad, dbias=conv.bias.grad, dnorm=onorm.grad[order])
    for k, w in want.items():
        assert mine[k].dtype == torch.float64 and rel_err(mine[k], w, floor=0) < 1e-10, (k, rel_err(mine[k], w, floor=0))
    # the intermediates say the same thing as autograd
    Fo = lambda t, *s: t.reshape(*s)
    checks = dict(
        out=(Fo(mine["Z"], -1, NB * Fd) @ Fo(conv.basis.detach(), NB * Fd, O) + x.detach() @ conv.root.detach() + conv.bias.detach(), mine["out"]),
        out_rel=(mine["Z_rel"] @ Fo(mine["Wr"], R * Fd, O) + x.detach() @ conv.root.detach() + conv.bias.detach(), mine["out"]),
        dnorm=((conv.att.detach()[et] * mine["TT"]).sum(1), mine["norm"] * mine["dnorm"]),
        dcomp=(ref.relation_sums(mine["TT"], et, R), mine["dcomp"]),
        dbasis=(Fo(mine["Z"].t() @ gout.double(), NB, Fd, O), mine["dbasis"]),
        dWr=(Fo(mine["Z_rel"].t() @ gout.double(), R, Fd, O), mine["dWr"]),
        dZ=(gout.double() @ Fo(conv.basis.detach(), NB * Fd, O).t(), mine["dZ"]),
        dx_rgcn=(Fo(mine["U_rel"], -1, R, O).transpose(0, 1).bmm(mine["WrT"]).sum(0) + gout.double() @ conv.root.detach().t(), mine["dx_rgcn"]),
        dx=(mine["dx_rgcn"] + mine["dx_att"] + mine["DATT"] @ att.weight.detach(), mine["dx"]),
        dscore=(mine["dscore_closed"], mine["dscore"]), DATT=(mine["DATT_closed"], mine["DATT"]),
        dW=(mine["DATT"].t() @ x.detach(), mine["dW"]))
    for k, (a, b) in checks.items():
        assert rel_err(a, b, floor=0) < 1e-10, (k, rel_err(a, b, floor=0))
    occupied = torch.zeros(R, dtype=torch.bool).index_fill(0, et, True)
    assert bool((mine["dcomp"][~occupied] == 0).all()) and (S == 2 or int((~occupied).sum()) > 0)


@pytest.mark.parametrize("name", ["dgcn_s2", "dgcn_s9"])
def test_restatement_and_host_graph_reproduce_the_reference_fixtures(golden, name):
    """the tolerances are those of tests/test_gpu_dgcn.py for the same quantities"""
    fx = golden(name)
    S, Fd, O = int(fx["n_speakers"]), 200, 100
    lengths, spk = fx["lengths"], torch.from_numpy(fx["speakers"])
    feats = torch.from_numpy(fx["features"])
    ei, et = ref.host_graph(lengths, spk, 10, 10, S)
    np.testing.assert_array_equal(ei.numpy(), fx["edge_index"])
    np.testing.assert_array_equal(et.numpy(), fx["edge_type"])
    att, conv = _params(S, Fd, O, int(fx["att_seed"]), int(fx["conv_seed"]))
    m = ref.restate(ei, et, 2 * S * S, _nodes(feats, lengths), att.weight, conv.att, conv.basis, conv.root, conv.bias,
                    torch.from_numpy(fx["gout"]))
    np.testing.assert_allclose(m["norm"].numpy(), fx["edge_norm"], atol=2e-6, rtol=2e-5)
    np.testing.assert_allclose(m["out"].numpy(), fx["rgcn_out"], atol=1e-4, rtol=1e-4)
    dfeat = torch.zeros(feats.shape, dtype=torch.float64)
    off = 0
    for b, L in enumerate(lengths):
        dfeat[b, :int(L)] = m["dx"][off:off + int(L)]
        off += int(L)
    np.testing.assert_allclose(dfeat.numpy(), fx["dfeatures"], atol=2e-4, rtol=2e-3)
    check_grad_digest(fx, [("edge_att.weight", m["dW"]), ("conv1.basis", m["dbasis"]), ("conv1.att", m["dcomp"]),
                           ("conv1.root", m["droot"]), ("conv1.bias", m["dbias"])], tol=2e-3)
