"""The DAG-ERC recurrence as the reference states it (oracle/dagerc.py GatherV1 / DAGERCOracle.forward, i.e. dagerc.py:167-189
and dagerc_models.py:326-365), in plain torch at a chosen precision -- float64 for the tests, float32 for the yardstick.  No
GPU, no library, nothing of the kernels' slicing: per step the scores of the WHOLE prefix are masked with -1e30 outside the
DAG window and go through one softmax, Wr0 h / Wr1 h are picked by the speaker mask, h_t = GRUCell_c(x = H_l[t], h = M_t) +
GRUCell_p(x = M_t, h = H_l[t]), M_0 = 0.  It runs over all T padded steps of every dialogue, like the reference.

Parameters are held per layer in the stacking of the C contract (include/ercgraft.h, K6):
  Wh [1801, 300] = grus_c.weight_ih ; grus_p.weight_hh ; w_q     bh [1801] = grus_c.bias_ih ; grus_p.bias_hh ; gather.linear.bias
  W_hh_c [900, 300], b_hh_c [900] = grus_c.weight_hh / bias_hh    W_ih_p, b_ih_p = grus_p.weight_ih / bias_ih
  Wr [600, 300] = Wr0 ; Wr1                                       w_k [300] (gather.linear.weight = [w_q | w_k])
What dag_rec_ref returns per layer is every tensor of that contract: H1, GI (1801 columns: hoisted gate pre-activations and
the query score), GH, Mseq, R, ks, alpha [B, T, T], the attention sums A; and, for a head gradient dHall, by autograd: DGI, DGH,
dM, dks as the gradients wrt GI, GH, Mseq (row 0, the constant M_0, is 0) and ks, the gradient wrt every parameter tensor and
the complete gradient wrt H_0 through the H_0 > 0 mask.

The histories R and ks are lists of per-step tensors, stacked per step from the batch's earliest window start on (no
torch.cat regrowth of a [B, t, .] state): T = 1021 takes seconds.

``python -m tests.dag_rec_ref`` prints, for the cases of tests/test_gpu_dag_rec.py, the float32-vs-float64 yardstick per
tensor class and the sensitivity of the compared tensors to three subtly wrong recurrences.
"""
import contextlib
import math
import sys

import numpy as np
import torch

from oracle.graph import dag_pred_closed_form

HID = 300
MAX_T = 1021            # csrc/dag_rec.hip MAX_T, include/ercgraft.h
PARAMS = ("Wh", "bh", "W_hh_c", "b_hh_c", "W_ih_p", "b_ih_p", "Wr", "w_k")
CLASSES = {"fwd": ("H1", "GI", "GH", "Mseq", "R", "ks", "A"), "alpha": ("alpha",), "bwd": ("DGI", "DGH", "dM", "dks"),
           "dH0": ("dH0",), "wgrad": tuple("d" + k for k in PARAMS)}


def init_layers(L, gen, scale=1.0):
    """per-layer parameters at nn.GRUCell / nn.Linear's init scale (uniform +- 1 / sqrt(fan_in)), times ``scale``"""
    u = lambda bound, *s: (torch.rand(*s, generator=gen, dtype=torch.float64) * 2 - 1) * bound * scale
    a, b = 1.0 / math.sqrt(HID), 1.0 / math.sqrt(2 * HID)
    out = []
    for _ in range(L):
        ly = dict(Wh=torch.cat([u(a, 6 * HID, HID), u(b, 1, HID)]), bh=torch.cat([u(a, 6 * HID), u(b, 1)]),
                  W_hh_c=u(a, 3 * HID, HID), b_hh_c=u(a, 3 * HID), W_ih_p=u(a, 3 * HID, HID), b_ih_p=u(a, 3 * HID),
                  Wr=u(a, 2 * HID, HID), w_k=u(b, HID))
        out.append({k: v.float() for k, v in ly.items()})       # fp32-representable: the kernels get the same numbers
    return out


def layers_from_oracle(model):
    """the contract's stacking of a DAGERCOracle's (or DAGERCModule's) per-layer parameters"""
    out = []
    for l in range(model.gnn_layers):
        c, p, g = model.grus_c[l], model.grus_p[l], model.gather[l]
        lw = g.linear.weight.detach().view(-1)
        out.append(dict(Wh=torch.cat([c.weight_ih, p.weight_hh, lw[None, :HID]]).detach(),
                        bh=torch.cat([c.bias_ih, p.bias_hh, g.linear.bias]).detach(),
                        W_hh_c=c.weight_hh.detach(), b_hh_c=c.bias_hh.detach(), W_ih_p=p.weight_ih.detach(),
                        b_ih_p=p.bias_ih.detach(), Wr=torch.cat([g.Wr0.weight, g.Wr1.weight]).detach(), w_k=lw[HID:].clone()))
    return out


def dag_rec_ref(H0, layers, spk, pred=None, dHall=None, dtype=torch.float64, wrong=None, full_prefix=False):
    """H0 [B, T, 300], layers (see above), spk [B, T] ids, pred [B, T] (default: dag_pred_closed_form(spk)), dHall [B, T,
    300 (L + 1)] the head's part of dL/d[H_0 | .. | H_L] (None: forward only).  Returns a list of per-layer dicts and, with
    dHall, the masked gradient wrt H_0 as out[0]["dH0"].
    ``wrong`` (sensitivity only): ("edge", b, i, j) lets utterance j take the other relation matrix in step i of dialogue b;
    ("early", b, i) starts that step's window one utterance early; ("bhn",) moves cell P's b_hn outside r * (.)."""
    spk = np.asarray(spk)
    pred = dag_pred_closed_form(spk) if pred is None else np.asarray(pred)
    B, T = spk.shape
    L = len(layers)
    lo = torch.from_numpy(np.maximum(pred, 0))                                  # window of step i: [lo, i - 1]
    spk_t = torch.from_numpy(spk.astype(np.int64))
    same = spk_t[:, :, None] == spk_t[:, None, :]                               # s_mask[b, i, j]
    ar = torch.arange(T)
    adj = (ar[None, None, :] >= lo[:, :, None]) & (ar[None, None, :] < ar[None, :, None])    # [b, i, j]
    if wrong and wrong[0] == "edge":
        same = same.clone()
        same[wrong[1], wrong[2], wrong[3]] ^= True
    if wrong and wrong[0] == "early":
        adj = adj.clone()
        assert lo[wrong[1], wrong[2]] > 0
        adj[wrong[1], wrong[2], lo[wrong[1], wrong[2]] - 1] = True
    first = adj.any(0).int().argmax(1)                                          # earliest unmasked utterance of step i in the batch
    grad = dHall is not None
    W = [{k: v.detach().to(dtype).clone().requires_grad_(grad) for k, v in ly.items()} for ly in layers]
    Hl = H0.detach().to(dtype).clone().requires_grad_(grad)
    Hs, out, keep = [Hl], [], []
    with torch.set_grad_enabled(grad):
        for l in range(L):
            w = W[l]
            GI = Hl @ w["Wh"].t() + w["bh"]                                      # [B, T, 1801]; column 1800 = w_q.H_l[t] + b
            Wseq, bseq = torch.cat([w["W_hh_c"], w["W_ih_p"]]), torch.cat([w["b_hh_c"], w["b_ih_p"]])
            Wr0, Wr1 = w["Wr"][:HID], w["Wr"][HID:]
            b_hn_p = w["bh"][5 * HID:6 * HID]
            GIs, xs = GI.unbind(1), Hl.unbind(1)                                 # one node each, not a [B, T, .] gradient per step
            alpha = torch.zeros(B, T, T, dtype=dtype)
            hs, Ms, GHs, Rs, kss = [], [], [], [], []
            for i in range(T):
                if i == 0:
                    M = torch.zeros(B, HID, dtype=dtype)                        # M_0 = 0 (dagerc.py:168-174)
                else:
                    # Utterances before j0, the earliest window start of the batch, are masked in every dialogue: their score
                    # is -1e30 whatever w_k.h_j is (|x| - 1e30 rounds to -1e30), their weight exp(-1e30 - max) is exactly 0.
                    # So their scores are written as the constant and their zero terms left out of the sum; the softmax still
                    # runs over the whole prefix.  full_prefix = True spells everything out (tests/test_dag_rec_ref.py).
                    j0 = 0 if full_prefix else int(first[i])
                    score = GIs[i][:, 6 * HID, None] + torch.stack(kss[j0:i], 1)  # linear([Q | K_j])
                    score = score - (~adj[:, i, j0:i]).to(dtype) * 1e30         # mask_logic, dagerc_models.py:83-90
                    if j0:
                        score = torch.cat([torch.full((B, j0), -1e30, dtype=dtype), score], 1)
                    a = torch.softmax(score, dim=1)
                    alpha[:, i, :i] = a.detach()
                    Rw = torch.stack(Rs[j0:i], 1)
                    Vr = torch.where(same[:, i, j0:i, None], Rw[:, :, :HID], Rw[:, :, HID:])
                    M = torch.bmm(a[:, None, j0:], Vr)[:, 0]
                    if grad:
                        M.retain_grad()
                gh = M @ Wseq.t() + bseq                                        # [B, 1800]: cell C's hidden side, cell P's input side
                if grad:
                    gh.retain_grad()
                gi, x = GIs[i], xs[i]
                r = torch.sigmoid(gi[:, :HID] + gh[:, :HID])                    # cell C: x = H_l[i], h = M
                z = torch.sigmoid(gi[:, HID:2 * HID] + gh[:, HID:2 * HID])
                n = torch.tanh(gi[:, 2 * HID:3 * HID] + r * gh[:, 2 * HID:3 * HID])
                c = (1 - z) * n + z * M
                r = torch.sigmoid(gh[:, 3 * HID:4 * HID] + gi[:, 3 * HID:4 * HID])      # cell P: x = M, h = H_l[i]
                z = torch.sigmoid(gh[:, 4 * HID:5 * HID] + gi[:, 4 * HID:5 * HID])
                if wrong and wrong[0] == "bhn":
                    n = torch.tanh(gh[:, 5 * HID:] + r * (gi[:, 5 * HID:6 * HID] - b_hn_p) + b_hn_p)
                else:
                    n = torch.tanh(gh[:, 5 * HID:] + r * gi[:, 5 * HID:6 * HID])
                h = c + (1 - z) * n + z * x
                R = torch.cat([h @ Wr0.t(), h @ Wr1.t()], dim=1)
                ks = h @ w["w_k"]
                if grad:
                    ks.retain_grad()
                hs.append(h), Ms.append(M), GHs.append(gh), Rs.append(R), kss.append(ks)
            H1 = torch.stack(hs, dim=1)
            if grad:
                GI.retain_grad()
            keep.append((GI, GHs, Ms, kss))
            d = lambda t: t.detach()
            o = dict(H1=d(H1), GI=d(GI), GH=d(torch.stack(GHs, 1)), Mseq=d(torch.stack(Ms, 1)), R=d(torch.stack(Rs, 1)),
                     ks=d(torch.stack(kss, 1)), alpha=alpha)
            sm = same.to(dtype)
            o["A"] = torch.cat([(alpha * sm) @ o["H1"], (alpha * (1 - sm)) @ o["H1"]], dim=2)
            out.append(o)
            Hl = H1
            Hs.append(H1)
        if not grad:
            return out
        # the head's part of the gradient enters as an inner product with [H_0 | H_1 | .. | H_L]
        G = dHall.detach().to(dtype)
        loss = sum((h * G[:, :, HID * l:HID * (l + 1)]).sum() for l, h in enumerate(Hs))
    loss.backward()
    zero = lambda t: torch.zeros_like(t)
    g = lambda t: t.grad if t.grad is not None else zero(t)
    for l in range(L):
        GI, GHs, Ms, kss = keep[l]
        out[l].update(DGI=g(GI), DGH=torch.stack([g(t) for t in GHs], 1), dks=torch.stack([g(t) for t in kss], 1),
                      dM=torch.stack([zero(Ms[0])] + [g(t) for t in Ms[1:]], 1))
        out[l].update({"d" + k: g(W[l][k]) for k in PARAMS})
    out[0]["dH0"] = Hs[0].grad * (Hs[0].detach() > 0).to(dtype)
    return out


# ------------------------------------------------------------------------------------------------------------------- cases
# name -> (B, T, speakers, layers); inputs are seeded, weights at the module's init scale (softmax windows neither flat nor
# saturated: the scores of a window spread by a few tenths)
CASES = {
    "mix": (17, 110, 2, 4), "meld": (5, 40, 9, 4), "mono": (3, 33, 1, 2), "t1": (4, 1, 2, 4), "t2": (2, 2, 2, 4),
    "t3": (2, 3, 2, 4), "l5": (6, 37, 3, 5), "l1": (6, 37, 3, 1), "b33": (33, 24, 2, 4), "long": (5, 513, 3, 4),
    "limit": (1, MAX_T, 2, 2),
}
MIX_LENS = (110, 1, 2, 3, 17, 33, 64, 97, 109, 110, 50, 16, 15, 31, 32, 75, 100)


def make_case(name, variant=0):
    """inputs of a case as CPU tensors: H0 (relu of a normal draw, like relu(fc1 x)), layers, spk / pred / lengths, dHall.
    ``variant`` draws other values of the same shape (the reuse test)."""
    B, T, S, L = CASES[name]
    seed = sum(ord(ch) for ch in name) * 131 + 977 * variant
    gen = torch.Generator().manual_seed(seed)
    rs = np.random.RandomState(seed)
    if name == "mix":
        lens = np.array(MIX_LENS)
    else:
        lens = rs.randint(1, T + 1, size=B)
        lens[0] = T
    spk = rs.randint(0, S, size=(B, T))
    if name == "meld":              # speaker 8 speaks once, late: pred = -1 at t = 33, the window is the whole prefix
        spk[spk == 8] = 7
        spk[0, 33] = 8
    for b in range(B):
        spk[b, lens[b]:] = 0        # the collate pads with speaker 0, and the recurrence runs over the padded steps
    H0 = torch.relu(torch.randn(B, T, HID, generator=gen)).float()
    dHall = torch.randn(B, T, HID * (L + 1), generator=gen).float()
    return dict(name=name, B=B, T=T, S=S, L=L, lens=lens.astype(np.int64), spk=spk.astype(np.int64),
                pred=dag_pred_closed_form(spk), H0=H0, dHall=dHall, layers=init_layers(L, gen))


def rel(x, want):
    """max |x - want| relative to max |want| (absolute where the reference is identically zero)"""
    x, want = x.double(), want.double()
    if want.numel() == 0:
        return 0.0
    scale = float(want.abs().max())
    return float((x - want).abs().max()) / (scale if scale > 0 else 1.0)


def class_errors(got, want):
    """per tensor class, the worst rel() over its tensors and the layers"""
    e = {}
    for cls, names in CLASSES.items():
        e[cls] = max(rel(g[k], w[k]) for g, w in zip(got, want) for k in names if k in w)
    return e


def round_up_1(x):
    """x rounded up to one significant digit"""
    if x <= 0:
        return 0.0
    p = 10.0 ** math.floor(math.log10(x))
    return math.ceil(x / p - 1e-9) * p


@contextlib.contextmanager
def one_thread():
    """thousands of small dependent operations: a thread pool only slows them down (8 threads: 15 x)"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def reference(c, dtype=torch.float64, wrong=None):
    with one_thread():
        return dag_rec_ref(c["H0"], c["layers"], c["spk"], c["pred"], c["dHall"], dtype=dtype, wrong=wrong)


def wrong_forms(c):
    """the three subtly wrong recurrences of the sensitivity check, placed in the middle of dialogue 0"""
    T, pred = c["T"], c["pred"]
    i = next(t for t in range(T // 2, T) if pred[0, t] > 0 and t - pred[0, t] >= 2)
    return {"edge": ("edge", 0, i, i - 1), "early": ("early", 0, i), "bhn": ("bhn",)}


def contract_products(o, Hl):
    """the weight gradients formed from the saved tensors exactly as the header says, in float64"""
    f = lambda t: t.double().reshape(-1, t.shape[-1]) if t.dim() == 3 else t.double().reshape(-1, 1)
    DGI, DGH, dM, dks, Mseq, A, H1, Hl = (f(t) for t in (o["DGI"], o["DGH"], o["dM"], o["dks"], o["Mseq"], o["A"], o["H1"], Hl))
    dWseq, dbseq = DGH.t() @ Mseq, DGH.sum(0)
    return dict(dWh=DGI.t() @ Hl, dbh=DGI.sum(0), dW_hh_c=dWseq[:3 * HID], dW_ih_p=dWseq[3 * HID:], db_hh_c=dbseq[:3 * HID],
                db_ih_p=dbseq[3 * HID:], dWr=torch.cat([dM.t() @ A[:, :HID], dM.t() @ A[:, HID:]]), dw_k=(dks.t() @ H1)[0])


if __name__ == "__main__":
    import time
    names = sys.argv[1:] or list(CASES)
    for name in names:
        c = make_case(name)
        t0 = time.time()
        r64 = reference(c)
        t1 = time.time()
        y = class_errors(reference(c, torch.float32), r64)
        print("yardstick %-6s %s   (float64 %.1f s)" % (name, "  ".join("%s=%.2e" % kv for kv in y.items()), t1 - t0), flush=True)
        print("tolerance %-6s %s" % (name, "  ".join("%s=%.0e" % (k, round_up_1(4 * v)) for k, v in y.items())), flush=True)
        if name in ("mix", "meld"):
            for wname, wr in wrong_forms(c).items():
                e = class_errors(reference(c, wrong=wr), r64)
                print("wrong %-5s %-6s %s" % (wname, name, "  ".join("%s=%.2e" % kv for kv in e.items())), flush=True)
