"""K9, training half (the opt-in chained COGMEN variant): every new kernel against torch (autograd for the
backward), then the whole chained train step against the oracle.

"parity unpinned": the reference never runs this variant (it discards the encoder output, track_mm/cogmen.py:145-147), so
there is nothing of the reference's to pin it to; the checker is torch.nn.TransformerEncoder (the class the reference
instantiates, contrib/nn.py being a vendored copy) under autograd.  Kernels work on bf16 operands with fp32 accumulation:
tolerances are those of bf16 rounding (2^-8 relative per operand), stated per test.  Dropout decisions come from the
library's counter-based generator; ``erc_uniform_np`` restates it so that the checker can apply the same masks."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.gemm_forms_ref import erc_uniform_np  # the one restatement of the generator (csrc/erc_common.h erc_uniform)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def keep_mask(shape, p, seed, offset, stream):
    """1/(1-p) where the generator keeps element idx (row-major over ``shape``), 0 elsewhere."""
    if p == 0:
        return torch.ones(shape)
    idx = np.arange(int(np.prod(shape)), dtype=np.uint64)
    u = erc_uniform_np(np.uint64(seed) ^ np.uint64(stream), offset, idx)
    return torch.from_numpy((u >= np.float32(p)).astype(np.float32) / np.float32(1.0 - p)).view(shape)


def bf(t):
    return t.to(torch.bfloat16)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-9))


RNG = (7, 12345)   # {offset, seed}


def rng_state():
    return torch.tensor(RNG, dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("R,C", [(37, 24), (3520, 1380), (130, 2048), (65, 4140)])
def test_transpose_and_colsum(R, C):
    from erc_amd import capi
    torch.manual_seed(R)
    for dt in (torch.float32, torch.bfloat16):
        x = torch.randn(R, C).to(dt).to(DEV)
        Rp = (R + 7) // 8 * 8
        yt = torch.full((C, Rp), 3.0, dtype=torch.bfloat16, device=DEV)
        plain = torch.zeros(R, C, dtype=torch.bfloat16, device=DEV)
        capi.enc_transpose_bf16(x, C, R, C, yt, Rp, plain, C)
        want = x.to(torch.bfloat16)
        assert torch.equal(yt[:, :R], want.t())
        assert float(yt[:, R:].float().abs().max() if Rp > R else 0.0) == 0.0
        assert torch.equal(plain, want)
        out = torch.zeros(C, device=DEV)
        ws = torch.zeros(capi.enc_colsum_ws_floats(C), device=DEV)
        capi.enc_colsum(x, C, R, C, out, ws)
        ref = x.double().sum(0)
        assert float((out.double() - ref).abs().max()) < 1e-3 * max(1.0, float(ref.abs().max()))
        out2 = torch.zeros(C, device=DEV)
        capi.enc_colsum(x, C, R, C, out2, ws)
        assert torch.equal(out, out2)          # fixed summation order


@pytest.mark.parametrize("M,N,K", [(50, 40, 24), (3520, 2048, 1380), (300, 712, 2048)])
def test_gemm_epilogues(M, N, K):
    from erc_amd import capi
    torch.manual_seed(M)
    a, w = bf(torch.randn(M, K)).to(DEV), bf(torch.randn(N, K) / math.sqrt(K)).to(DEV)
    bias = torch.randn(N, device=DEV)
    base = F.relu(a.float() @ w.float().t() + bias)
    # 1: ReLU + dropout
    p = 0.5
    out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    capi.enc_gemm_bf16_ex(a, K, w, K, bias, None, out, N, M, N, K, relu=1, epilogue=1, scale=1 / (1 - p), drop_p=p,
                          rng_state=rng_state(), rng_stream=0x102)
    keep = keep_mask((M, N), p, RNG[1], RNG[0], 0x102).to(DEV)
    want = base * keep
    assert rel(out.float(), want) < 1e-2
    frac = float((keep > 0).float().mean())
    assert abs(frac - 0.5) < 0.02 if M * N > 10000 else True
    # 2: mask-multiply (backward of ReLU + dropout read off the forward output)
    dy = bf(torch.randn(M, K)).to(DEV)
    got = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    capi.enc_gemm_bf16_ex(dy, K, w, K, None, None, got, N, M, N, K, epilogue=2, mask_src=out, ld_mask=N, scale=2.0)
    want2 = (dy.float() @ w.float().t()) * (out != 0).float() * 2.0
    assert rel(got.float(), want2) < 1e-2


def _attention_reference(qkv, B, T, D, heads, lengths, keep):
    """softmax(q k^T / sqrt(hd) + key padding) * keep @ v on fp32 copies of the bf16 operands (autograd-able)."""
    hd = D // heads
    q, k, v = qkv.view(B, T, 3, heads, hd).permute(2, 0, 3, 1, 4)          # [B, h, T, hd]
    s = q @ k.transpose(-1, -2) / math.sqrt(hd)
    if lengths is not None:
        pad = torch.arange(T)[None, :] >= lengths[:, None]
        s = s.masked_fill(pad[:, None, None, :], float("-inf"))
    pr = torch.softmax(s, -1) * keep
    return (pr @ v).permute(0, 2, 1, 3).reshape(B * T, D)


@pytest.mark.parametrize("B,T,D,heads,p,masked", [(3, 13, 24, 6, 0.0, True), (2, 37, 712, 8, 0.5, True),
                                                   (2, 110, 1380, 6, 0.5, True), (2, 128, 96, 6, 0.0, False),
                                                   (1, 1, 24, 6, 0.0, True), (4, 33, 1380, 6, 0.3, True)])
def test_attention_train_forward_backward(B, T, D, heads, p, masked):
    from erc_amd import capi
    torch.manual_seed(T + D)
    qkv = bf(torch.randn(B * T, 3 * D) * 0.7)
    dout = bf(torch.randn(B * T, D))
    lengths = torch.randint(1, T + 1, (B,), dtype=torch.int64) if masked else None
    if masked:
        lengths[0] = T
    keep = keep_mask((B, heads, T, T), p, RNG[1], RNG[0], 0x100)
    x = qkv.float().requires_grad_(True)
    want = _attention_reference(x, B, T, D, heads, lengths, keep)
    want.backward(dout.float())
    out = torch.zeros(B * T, D, dtype=torch.bfloat16, device=DEV)
    dl = lengths.to(DEV) if masked else None
    capi.enc_attention_train(qkv.to(DEV), B, T, D, heads, dl, p, rng_state() if p > 0 else None, 0x100, out)
    # probabilities are rounded to bf16 before the p v product: 2^-8 relative on O(1) sums
    assert rel(out.float(), want.detach()) < 2e-2
    dqkv = torch.full((B * T, 3 * D), 7.0, dtype=torch.bfloat16, device=DEV)
    capi.enc_attention_bwd(qkv.to(DEV), dout.to(DEV), B, T, D, heads, dl, p, rng_state() if p > 0 else None, 0x100, dqkv)
    g = x.grad
    for part, name in ((slice(0, D), "dq"), (slice(D, 2 * D), "dk"), (slice(2 * D, 3 * D), "dv")):
        assert rel(dqkv[:, part].float(), g[:, part]) < 3e-2, name
    if masked:   # keys behind the padding mask receive no gradient
        for b in range(B):
            L = int(lengths[b])
            if L < T:
                assert float(dqkv[b * T + L:(b + 1) * T, D:].float().abs().max()) == 0.0


@pytest.mark.parametrize("M,D,p", [(9, 24, 0.0), (3520, 1380, 0.5), (130, 712, 0.5), (70, 2048, 0.3)])
def test_layernorm_train_forward_backward(M, D, p):
    from erc_amd import capi
    torch.manual_seed(M + D)
    a, b = torch.randn(M, D), torch.randn(M, D) * 2
    gamma, beta = torch.rand(D) + 0.5, torch.randn(D) * 0.3
    keep = keep_mask((M, D), p, RNG[1], RNG[0], 0x101)
    av, bv, gv, bev = (t.clone().requires_grad_(True) for t in (a, b, gamma, beta))
    want = F.layer_norm(av + bv * keep, (D,), gv, bev, 1e-5)
    yf, yh = torch.zeros(M, D, device=DEV), torch.zeros(M, D, dtype=torch.bfloat16, device=DEV)
    ssum, stats = torch.zeros(M, D, device=DEV), torch.zeros(2 * M, device=DEV)
    rs = rng_state() if p > 0 else None
    capi.enc_add_layernorm_train(a.to(DEV), b.to(DEV), D, M, gamma.to(DEV), beta.to(DEV), 1e-5, p, rs, 0x101, yf, yh, ssum, stats)
    assert float((yf.cpu() - want.detach()).abs().max()) < 1e-4
    assert torch.equal(yh, yf.to(torch.bfloat16))
    # backward: dy = dy_a[map] + dy_b with a row map holding -1 (zero rows)
    n_src = max(1, M // 2)
    dy_src = torch.randn(n_src, D)
    row_map = torch.full((M,), -1, dtype=torch.int32)
    perm = torch.randperm(M)[:n_src]
    row_map[perm] = torch.arange(n_src, dtype=torch.int32)
    dy_b = torch.randn(M, D)
    dy = dy_b.clone()
    dy[perm] += dy_src
    want.backward(dy)
    nb = capi.enc_layernorm_bwd_blocks(M)
    ds, db = torch.zeros(M, D, device=DEV), torch.zeros(M, D, dtype=torch.bfloat16, device=DEV)
    partial = torch.zeros(nb, 2 * D, device=DEV)
    capi.enc_layernorm_bwd(dy_src.to(DEV), row_map.to(DEV), dy_b.to(DEV), ssum, stats, gamma.to(DEV), D, M, p, rs, 0x101, ds, db,
                           partial)
    assert rel(ds, av.grad) < 1e-4
    assert rel(db.float(), bv.grad) < 1e-2                      # bf16 output
    out = torch.zeros(2 * D, device=DEV)
    capi.enc_colsum(partial, 2 * D, nb, 2 * D, out, torch.zeros(capi.enc_colsum_ws_floats(2 * D), device=DEV))
    assert rel(out[:D], gv.grad) < 1e-4 and rel(out[D:], bev.grad) < 1e-4


def _chained_pair(D, C, case_seed, B, T):
    from bench import synthetic_batch
    from erc_amd.cogmen import COGMENModule
    from erc_amd.params import ERCParams
    from oracle.cogmen import COGMENOracle
    torch.manual_seed(case_seed)
    ref = COGMENOracle(D, 100, 17, 2, C, chained=True)
    with torch.no_grad():
        for lyr in ref.rnn[0].layers:
            lyr.norm1.weight.uniform_(0.5, 1.5), lyr.norm1.bias.uniform_(-0.3, 0.3)
            lyr.norm2.weight.uniform_(0.5, 1.5), lyr.norm2.bias.uniform_(-0.3, 0.3)
        ref.gcn.bn.weight.uniform_(0.5, 1.5), ref.gcn.bn.bias.uniform_(-0.3, 0.3)
        for name, prm in ref.named_parameters():     # bf16-representable encoder / projection weights: the comparison
            if name.startswith("rnn.") and prm.dim() == 2:   # then sees activation rounding only, not weight rounding
                prm.copy_(prm.to(torch.bfloat16).float())
    mine = COGMENModule(D, 100, 17, 2, C, compute="f32", chained_encoder=True)
    mine.load_state_dict(ref.state_dict())
    mine.finalize(DEV)
    ds = "iemocap-cogmen-6" if D == 712 else "iemocap-cogmen-sbert-6"
    p = ERCParams().from_args(["--dataset=" + ds])
    batch = synthetic_batch(p, B, T, seed=case_seed)
    batch["input_tensor"] = batch["input_tensor"].to(torch.bfloat16).float()
    return ref, mine, batch


@pytest.mark.parametrize("D,B,T", [(712, 3, 21), (1380, 4, 110)])
def test_chained_cogmen_step_matches_oracle(D, B, T):
    """Whole chained train step (dropout off) against the oracle under autograd.
    Eval logits: against the plain fp32 torch module -- bf16 accuracy of O(1) activations through two layers.
    Loss and every gradient: against the oracle with the bf16 rounding hook at the points where the HIP path stores bf16
    (oracle/encoder.py): the forwards then agree to 0.1 % (projection output and logits, measured; what is left is the
    1-ulp disagreement of the final bf16 rounding).  Gradients: relative L2 error per tensor < 8 %, cosine > 0.996.
    Measured 3 - 5 % on every tensor, the fp32 graph layers behind the encoder included (cls.0.weight 3 %, which no bf16
    kernel touches): with random labels on an untrained net a weight gradient is a sum over nodes of terms of random
    sign, so 0.1 % forward noise is amplified by the cancellation; a wiring error (missing residual branch, wrong mask)
    shows up as cosine << 0.99.  The sharp check of the encoder backward itself is
    test_encoder_train_with_dropout_matches_oracle below (linear loss, same masks)."""
    from oracle.encoder import round_bf16
    from tests.util_cases import to_device
    ref, mine, batch = _chained_pair(D, 6, 5, B, T)
    dbatch = to_device(batch, DEV)
    ref.eval(), mine.eval()
    with torch.no_grad():
        want, _ = ref(**batch)
    got, _ = mine(**dbatch)
    assert float((got.cpu() - want).abs().max()) < 0.15 * max(1.0, float(want.abs().max()))
    ref.train(), mine.train()
    for m in ref.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    mine.drop_p, mine.enc_train.drop_p = 0.0, 0.0
    ref.enc_rnd = round_bf16
    logits, _ = ref(**batch)
    loss = F.cross_entropy(logits, batch["label"])
    ref.zero_grad()
    loss.backward()
    stats = mine.loss_and_grads(dbatch).cpu()
    assert abs(float(stats[0]) - float(loss.detach())) < 2e-3 * max(1.0, float(loss.detach()))
    ref_params = dict(ref.named_parameters())
    checked, worst = 0, (0.0, "")
    top = max(float(ref_params[n].grad.norm()) for n in mine.flat.params)
    for name in mine.flat.params:
        want_g = ref_params[name].grad
        got_g = mine.flat.g(name).cpu()
        if float(want_g.norm()) < 2e-3 * top:
            # (nearly) cancelling gradients -- biases in front of BatchNorm / softmax -- are all noise at this accuracy:
            # bounded in absolute terms instead
            assert float((got_g - want_g).norm()) < 2e-3 * top, name
            continue
        err = float((got_g - want_g).norm() / want_g.norm())
        cos = float(F.cosine_similarity(got_g.flatten(), want_g.flatten(), dim=0))
        worst = max(worst, (err, name))
        assert err < 8e-2 and cos > 0.996, (name, err, cos)
        checked += 1
    print("worst gradient error", worst)
    assert checked >= 30 and all(n in mine.flat.params for n in ("rnn.0.layers.0.self_attn.in_proj_weight",
                                                                "rnn.0.layers.1.linear2.bias"))


@pytest.mark.parametrize("D,B,T,p", [(24, 3, 13, 0.5), (712, 2, 37, 0.5), (1380, 2, 110, 0.3)])
def test_encoder_train_with_dropout_matches_oracle(D, B, T, p):
    """EncoderTrain forward + backward with all four dropout sites per layer active, against the functional oracle
    given the SAME keep decisions (numpy restatement of the generator) and the bf16 rounding hook."""
    from erc_amd.cogmen import COGMENModule
    from oracle.encoder import encoder, round_bf16
    torch.manual_seed(D + T)
    mine = COGMENModule(D, 100, 17, 2, 6, chained_encoder=True)
    ref_enc = mine.rnn[0]
    with torch.no_grad():
        for lyr in ref_enc.layers:
            lyr.norm1.weight.uniform_(0.5, 1.5), lyr.norm1.bias.uniform_(-0.3, 0.3)
            lyr.norm2.weight.uniform_(0.5, 1.5), lyr.norm2.bias.uniform_(-0.3, 0.3)
    import copy
    ref_enc = copy.deepcopy(ref_enc)
    mine.finalize(DEV)
    et = mine.enc_train
    et.drop_p = p
    h, Fd, M = et.heads, et.ffn, B * T
    x = torch.randn(B, T, D).to(torch.bfloat16).float()
    lengths = torch.randint(1, T + 1, (B,), dtype=torch.int64)
    lengths[0] = T
    pad = torch.arange(T)[None, :] >= lengths[:, None]
    keeps = {}
    for layer in range(2):
        for site, shape in enumerate([(B, h, T, T), (M, D), (M, Fd), (M, D)]):
            keeps[(layer, site)] = keep_mask(shape, p, RNG[1], RNG[0], 0x100 + 4 * layer + site)
    want = encoder(x, ref_enc, pad, keeps, round_bf16)
    d_out = torch.randn(M, D) * (~pad).reshape(M, 1)          # padded rows carry no gradient (they are never gathered)
    ref_enc.zero_grad()
    (want.reshape(M, D) * d_out).sum().backward()
    got = et.forward(x.to(DEV), lengths.to(DEV), True, rng_state())
    valid = (~pad).reshape(M)
    assert rel(got.float().cpu()[valid], round_bf16(want).detach().reshape(M, D)[valid]) < 2e-2
    mine.flat.grad.zero_()
    et.backward(d_out.to(DEV))
    ref_params = dict(ref_enc.named_parameters())
    worst = (0.0, "")
    for name in mine.flat.params:
        if not name.startswith("rnn.0."):
            continue
        want_g = ref_params[name[len("rnn.0."):]].grad
        got_g = mine.flat.g(name).cpu()
        err = float((got_g - want_g).norm() / want_g.norm())
        worst = max(worst, (err, name))
        assert err < 3e-2, (name, err)
    print("worst encoder gradient error", worst)


def test_chained_training_is_reproducible_and_learns():
    """Dropout on (4 sites per layer + head), HIP-graph replay: two trainers with the same seed produce bit-identical
    losses, and the loss on a fixed batch goes down."""
    from bench import synthetic_batch
    from erc_amd.cogmen import COGMENTrainer
    from erc_amd.engine import GraphedStep
    from erc_amd.params import ERCParams
    runs = []
    for _ in range(2):
        p = ERCParams().from_args(["--dataset=iemocap-cogmen-6", "--chained_encoder", "--optim.lr=0.0003"])
        tr = COGMENTrainer(p, DEV)
        assert tr.model.enc_train is not None and "rnn.0.layers.1.norm2.bias" in tr.model.flat.params
        b = tr.prepare_batch(synthetic_batch(p, 6, 40, seed=3))
        step = GraphedStep(lambda: tr.train_step(b))
        runs.append([float(step().cpu()[0]) for _ in range(30)])
    assert runs[0] == runs[1]
    assert sum(runs[0][-5:]) < sum(runs[0][:5]) * 0.9
    # the trained encoder weights reach the state dict under the reference's names
    sd = tr.model.state_dict()
    assert "rnn.0.layers.0.self_attn.in_proj_weight" in sd


def test_training_attention_rejects_long_sequences():
    """The matrix-core attention holds one sequence per workgroup (S <= 128): longer ones are refused, not truncated."""
    from erc_amd import capi
    qkv = torch.zeros(2 * 130, 3 * 24, dtype=torch.bfloat16, device=DEV)
    out = torch.zeros(2 * 130, 24, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(capi.ErcGraftError):
        capi.enc_attention_train(qkv, 2, 130, 24, 6, None, 0.0, None, 0, out)
