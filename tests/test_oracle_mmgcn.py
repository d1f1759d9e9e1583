"""CPU: the MMGCN oracle reproduces the reference's own MMGCNModule (golden vectors): normalised adjacency,
logits, loss, gradients, and the set of never-trained parameters."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

from oracle.mmgcn import MMGCNOracle
from tests.util_cases import check_grad_digest, fill_params


@pytest.mark.parametrize("name", ["mmgcn_atv", "mmgcn_tv_s3"])
def test_mmgcn_oracle_matches_reference(golden, name):
    fx = golden(name)
    batch = {k[3:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("in_")}
    for k in ("text_feature", "audio_feature", "visual_feature"):
        batch.setdefault(k, None)
    da, dt, dv = [int(v) for v in fx["dims"]]
    model = MMGCNOracle(hidden_text=dt, hidden_visual=dv, hidden_audio=da, n_speakers=int(fx["n_speakers"]),
                        n_classes=int(fx["n_classes"]), modals=str(fx["modality"]))
    fill_params(model, int(fx["param_seed"]))
    model.eval()
    logits, _ = model(**batch)
    loss = F.cross_entropy(logits, batch["label"])
    loss.backward()
    np.testing.assert_allclose(model.graph_model.last_adj.detach().numpy(), fx["adj"], atol=2e-6, rtol=1e-5)
    np.testing.assert_allclose(logits.detach().numpy(), fx["logits"], atol=5e-6, rtol=1e-4)
    assert abs(float(loss) - float(fx["loss"])) < 1e-6
    none = sorted(n for n, p in model.named_parameters() if p.grad is None)
    assert none == sorted(fx["grad_none"].tolist())
    check_grad_digest(fx, [(n, p.grad) for n, p in model.named_parameters() if p.grad is not None], tol=2e-4)


@pytest.mark.parametrize("Mo,lens", [(2, (6, 1, 11)), (3, (9, 1, 17, 4))])
def test_chain_reference_matches_dense_oracle(Mo, lens):
    """tests/mmgcn_chain_ref.py (the float64 chain on the kernels' block inputs) equals the pinned oracle's GCNII run on the
    dense (Mo N)^2 adjacency of big_adjacency: every plane, out_l's gradients, the weight, adjacency and input gradients."""
    from oracle.mmgcn import GCNII, big_adjacency
    from tests.mmgcn_chain_ref import ALPHA, FD, LAMDA, NL, build_adjacency, chain_ref
    torch.manual_seed(11 + Mo)
    f64 = torch.float64
    N, T = sum(lens), max(lens)
    node_off = np.concatenate([[0], np.cumsum(lens)])
    P = (T + 3) // 4 * 4
    feats = [torch.randn(N, FD, dtype=f64) for _ in range(Mo)]
    net = GCNII(FD, NL, FD, 0.4, LAMDA, ALPHA).to(f64).eval()
    seen, outs = {}, []

    def keep(store):
        def hook(mod, inp, out):
            out.retain_grad()
            store(out)
        return hook
    net.fcs[0].register_forward_hook(keep(lambda o: seen.setdefault("pre", o)))
    for conv in net.convs:
        conv.register_forward_hook(keep(outs.append))
    adj = big_adjacency(feats, lens).requires_grad_()
    x = torch.cat(feats)
    res = net(x, adj)[:, FD:]
    dHin = torch.randn_like(res)
    (res * dHin).sum().backward()

    ADJ, CR = build_adjacency(feats, node_off, P)
    h0 = torch.relu(seen["pre"]).detach()
    W = torch.stack([c.weight.detach() for c in net.convs])
    ref = chain_ref(ADJ, CR, node_off, h0, h0, W, Mo, dHin=dHin)

    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-9, atol=1e-11 * float(b.abs().max()))
    close(ref["planes"][1:], torch.stack([torch.relu(o) for o in outs]).detach())
    close(ref["dg"], torch.stack([o.grad for o in outs]))
    close(ref["dz"], torch.stack([adj.detach().t() @ o.grad for o in outs]))
    close(ref["z"], torch.stack([p @ (th * w[:FD] + (1 - th) * (1 - ALPHA) * torch.eye(FD, dtype=f64))
                                 for p, w, th in zip(ref["planes"][:NL], W, [np.log(LAMDA / l + 1) for l in range(1, NL + 1)])]))
    close(ref["dW"], torch.stack([c.weight.grad for c in net.convs]))
    # h0 is plane 1 here: the oracle's gradient at the input layer is the sum of both paths
    close((ref["dh1"] + ref["dh0"]) * (seen["pre"] > 0), seen["pre"].grad)
    dA = adj.grad
    for b, L in enumerate(lens):
        o, idx = int(node_off[b]), torch.arange(L)
        for m in range(Mo):
            close(ref["dADJ"][b * Mo + m, :L, :L], dA[m * N + o:m * N + o + L, m * N + o:m * N + o + L])
            for n in range(Mo):
                want = dA[m * N + o + idx, n * N + o + idx] if n != m else torch.zeros(L, dtype=f64)
                close(ref["dCR"][b, m * Mo + n, :L], want)
    assert float(ref["dADJ"].abs().sum()) > 0 and float(ref["dCR"].abs().sum()) > 0


def test_oracle_per_dialogue_decomposition_is_exact():
    """The batch's logits / loss / gradients of MMGCNOracle (float64) equal the per-dialogue runs combined as
    sum_b (L_b / N) g_b: what the module-level tests at large B compare against."""
    from oracle.mmgcn import MMGCNOracle
    from tests.mmgcn_chain_ref import oracle_per_dialogue
    from tests.util_cases import make_batch_lengths
    dims = dict(a=20, t=24, v=18)
    batch = make_batch_lengths((7, 1, 12, 5), dims, n_speakers=3, n_classes=6, seed=5, modality="atv", batch_first=False,
                               speaker_onehot=True)
    for k in ("text_feature", "audio_feature", "visual_feature"):
        batch[k] = batch[k].double()
    torch.manual_seed(3)
    ref = MMGCNOracle(hidden_text=dims["t"], hidden_visual=dims["v"], hidden_audio=dims["a"], n_speakers=3, n_classes=6,
                      modals="atv").double().eval()
    logits, _ = ref(**batch)
    loss = F.cross_entropy(logits, batch["label"])
    loss.backward()
    want = {n: p.grad.clone() for n, p in ref.named_parameters() if p.grad is not None}
    got_logits, got_loss, got = oracle_per_dialogue(ref, batch)
    assert logits.dtype == torch.float64
    torch.testing.assert_close(got_logits, logits.detach(), rtol=1e-10, atol=1e-12)
    assert abs(float(got_loss) - float(loss)) < 1e-12
    assert sorted(got) == sorted(want)
    for n in want:
        torch.testing.assert_close(got[n], want[n], rtol=1e-9, atol=1e-12 * (1 + float(want[n].abs().max())), msg=n)
