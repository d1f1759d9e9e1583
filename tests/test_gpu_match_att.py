"""GPU: the matching attention 'general2' (csrc/match_att.hip: erc_match_att_fwd / _bwd / _bwd_cap) at both built row widths
against CPU autograd, and what it refuses before a launch."""
import numpy as np
import pytest
import torch

from erc_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the longest dialogue the kernel takes, one row, the 64-lane boundary from both sides, one 16-row tile and one row past it
LENS = [110, 1, 37, 64, 65, 16, 17, 2]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    capi.lib()


def _err(a, b):
    return float((a.detach().cpu() - b).abs().max())


def _f32(*s):
    return torch.zeros(*s, device=DEV)


@pytest.mark.parametrize("F", [200, 300])
def test_matching_attention_matches_autograd(F):
    """erc_match_att_fwd / _bwd against CPU autograd of softmax(tanh(Q E^T)) E per dialogue (ragged lengths 1..110); E enters
    as keys and values, Q as the queries"""
    B, T, N = len(LENS), max(LENS), sum(LENS)
    g = torch.Generator().manual_seed(4)
    E = (torch.randn(N, F, generator=g) * 0.1).requires_grad_()
    Q = (torch.randn(N, F, generator=g) * 0.1).requires_grad_()
    outs, off = [], 0
    for L in LENS:
        e, q = E[off:off + L], Q[off:off + L]
        outs.append(torch.softmax(torch.tanh(q @ e.t()), -1) @ e)
        off += L
    A_ref = torch.cat(outs)
    G = torch.randn(N, F, generator=g)
    (A_ref * G).sum().backward()
    node_off = torch.tensor([0] + list(np.cumsum(LENS)), dtype=torch.int32, device=DEV)
    Ed, Qd, Gd, A = E.detach().to(DEV), Q.detach().to(DEV), G.to(DEV), _f32(N, F)
    P, TH, DZ, dQ, dE = _f32(B * T * T), _f32(B * T * T), _f32(B * T * T), _f32(N, F), _f32(N, F)
    capi.match_att_fwd(Ed, F, Qd, F, node_off, B, T, F, A, F, P, TH)
    capi.match_att_bwd(Ed, F, Qd, F, Gd, F, node_off, B, T, F, P, TH, DZ, dQ, F, dE, F)
    torch.cuda.synchronize()
    assert _err(A, A_ref.detach()) < 1e-5
    assert _err(dQ, Q.grad) <= 1e-5 * (float(Q.grad.abs().max()) + 1e-6)
    assert _err(dE, E.grad) <= 1e-5 * (float(E.grad.abs().max()) + 1e-6)
    # a second run is bit-identical (fixed summation order, no atomics)
    dE2 = _f32(N, F)
    capi.match_att_bwd(Ed, F, Qd, F, Gd, F, node_off, B, T, F, P, TH, DZ, dQ, F, dE2, F)
    torch.cuda.synchronize()
    assert torch.equal(dE, dE2)


def _operands(F, T, N):
    node_off = torch.tensor([0, N], dtype=torch.int32, device=DEV)
    return node_off, [_f32(N, F) for _ in range(6)], [_f32(T * T) for _ in range(3)]


def test_unbuilt_width_is_refused_and_names_the_built_ones():
    F, T, N = 256, 4, 4
    node_off, (E, Q, A, dA, dQ, dE), (P, TH, DZ) = _operands(F, T, N)
    with pytest.raises(capi.ErcGraftError, match="200 and 300"):
        capi.match_att_fwd(E, F, Q, F, node_off, 1, T, F, A, F, P, TH)
    with pytest.raises(capi.ErcGraftError, match="200 and 300"):
        capi.match_att_bwd(E, F, Q, F, dA, F, node_off, 1, T, F, P, TH, DZ, dQ, F, dE, F)


@pytest.mark.parametrize("F", [200, 300])
def test_dialogues_above_110_are_refused(F):
    T = N = 111
    node_off, (E, Q, A, dA, dQ, dE), (P, TH, DZ) = _operands(F, T, N)
    with pytest.raises(capi.ErcGraftError, match="110"):
        capi.match_att_fwd(E, F, Q, F, node_off, 1, T, F, A, F, P, TH)
    with pytest.raises(capi.ErcGraftError, match="110"):
        capi.match_att_bwd(E, F, Q, F, dA, F, node_off, 1, T, F, P, TH, DZ, dQ, F, dE, F)


def test_capacity_form_is_refused_at_width_300():
    F, T, N = 300, 4, 4
    node_off, (E, Q, A, dA, dQ, dE), (P, TH, DZ) = _operands(F, T, N)
    with pytest.raises(capi.ErcGraftError, match="capacity.*200"):
        capi.match_att_bwd(E, F, Q, F, dA, F, node_off, 1, T, F, P, TH, DZ, dQ, F, dE, F, n_cap=N)
