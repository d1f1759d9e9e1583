"""Float64 restatement of the cross-entropy launch (csrc/norm_loss.hip: erc_cross_entropy, erc_cross_entropy_cap), its float32
twin, the case table and the bounds of tests/test_loss_ref.py and tests/test_gpu_cross_entropy.py.  Written from the math, in
plain torch on the CPU; nothing of the kernel's grid or its partial sums.

Math.  Sample i < n reads row r_i = row_map[i] (or i) of the logits, z = logits[r_i, :C]; with w_i = weight[y_i] (or 1):
  loss = sum_i w_i (logsumexp(z) - z[y_i]) / sum_i w_i,   dlogits[r_i] = grad_scale w_i / (sum w) (softmax(z) - onehot(y_i)),
  hits = #{i: y_i = the FIRST index of max z}.
The twin is torch.nn.functional.cross_entropy in float32 with autograd.  Bounds are tests/mmin_ref.py's twin_bound.

Logit families.  "n3": 3 randn, what the suite used so far.  "n30": 30 randn, "p100" / "m100": 3 randn +- 100.  The last three are
where exp(z - lse) with lse = max + log(sum) goes wrong: lse is rounded at the unit in the last place of the largest logit
(7.6e-6 at 100), and the softmax inherits that as a relative error.  exp(z - max) / sum does not.
"""
import zlib

import torch

from tests.mmin_ref import first_argmax, rel, twin_bound  # noqa: F401

FAMILIES = {"n3": (3.0, 0.0), "n30": (30.0, 0.0), "p100": (3.0, 100.0), "m100": (3.0, -100.0)}
STRIDE_N = 16384          # 64 workgroups of 256 rows: above it the grid strides
PAD_LD, PAD_LDDL = 3, 5   # ld = C + 3, lddl = C + 5
EXTRA_ROWS = 37           # a mapped launch selects its n rows from n + EXTRA_ROWS
N_TIES = 3                # rows with two equal maxima, where n allows

# name -> (n, C, weighted, mapped, padded (ld = C + 3, lddl = C + 5), grad_scale, dlogits written).  Every value of the issue's
# lists occurs at a small n and at one that strides the grid.
CASES = {
    "n1":          (1, 6, False, False, False, 1.0, True),
    "n1_c1":       (1, 1, True, False, True, 0.125, True),
    "n255_c2":     (255, 2, True, True, True, 0.125, True),
    "n255_c7":     (255, 7, False, False, True, 1.0, True),
    "n257_c4":     (257, 4, False, True, False, 1.0, True),
    "n257_c6_nod": (257, 6, True, True, True, 1.0, False),
    "n257_c1":     (257, 1, False, False, False, 1.0, True),
    "n16384_c6":   (16384, 6, True, False, False, 1.0, True),
    "n16385_c7":   (16385, 7, True, True, True, 0.125, True),
    "n16385_c2":   (16385, 2, False, False, False, 1.0, True),
    "n17161_c4":   (17161, 4, True, False, True, 1.0, True),
    "n17161_c6":   (17161, 6, False, True, True, 0.125, True),
    "n17161_c1":   (17161, 1, True, True, False, 1.0, True),
    "n17161_nod":  (17161, 7, False, False, True, 1.0, False),
}
CAP_N, CAP_C = 300, 6
CAP_COUNTS = (0, 1, 299, 300, 5000, -3)


def _gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()))


def case(name, family):
    """dict(logits [rows, C] fp32, labels [n], weight [C] | None, row_map int32 [n] | None, ties: the rows of two equal maxima)"""
    n, C, weighted, mapped, _, grad_scale, _ = CASES[name]
    scale, shift = FAMILIES[family]
    gen = _gen("ce-%s-%s" % (name, family))
    rows = n + EXTRA_ROWS if mapped else n
    logits = torch.randn(rows, C, generator=gen) * scale + shift
    if C >= 2:        # two float32 draws do coincide now and then (3 randn + 100 has 7.6e-6 between neighbours): part such rows
        top = logits.max(-1, keepdim=True)
        twice = (logits == top.values).sum(-1) > 1
        logits[twice, top.indices[twice, 0]] += 1.0
    labels = torch.randint(0, C, (n, ), generator=gen)
    row_map = torch.randperm(rows, generator=gen)[:n].to(torch.int32) if mapped else None      # a subset, permuted, no duplicates
    weight = (torch.rand(C, generator=gen) * 9.0 + 1.0) if weighted else None
    ties = []
    if C >= 2:
        for k in range(min(N_TIES, n)):
            i = (k * 97) % n
            r = int(row_map[i]) if mapped else i
            a, b = k % C, (k + 1 + k % (C - 1)) % C            # two different columns
            if a == b:
                b = (a + 1) % C
            top = logits[r].max() + 0.5
            logits[r, a] = logits[r, b] = top
            labels[i] = (min(a, b), max(a, b), min(a, b))[k % 3]       # the first index (a hit), the second (not a hit)
            ties.append(i)
    return dict(name=name, family=family, n=n, C=C, rows=rows, logits=logits, labels=labels, weight=weight, row_map=row_map,
                grad_scale=grad_scale, ties=ties)


def _select(logits, row_map, n):
    return logits[row_map.long()[:n]] if row_map is not None else logits[:n]


def cross_entropy64(logits, labels, weight, row_map, n, grad_scale):
    """-> (loss, hits, weight sum, dlogits [n, C] in SAMPLE order), in float64.  n = 0: (0, 0, 0, empty)"""
    z = _select(logits, row_map, n).double()
    y = labels[:n].long()
    C = z.shape[1]
    if n == 0:
        return 0.0, 0, 0.0, z.new_zeros(0, C)
    w = weight.double()[y] if weight is not None else z.new_ones(n)
    wsum = w.sum()
    lse = torch.logsumexp(z, -1)
    loss = (w * (lse - z.gather(1, y[:, None]).squeeze(1))).sum() / wsum
    dl = float(torch.tensor(grad_scale, dtype=torch.float32)) * (w / wsum)[:, None] * (torch.softmax(z, -1) - torch.nn.functional.one_hot(y, C).double())
    hits = int((first_argmax(z, 1)[1] == y).sum())
    return float(loss), hits, float(wsum), dl


def cross_entropy32(logits, labels, weight, row_map, n, grad_scale):
    """the twin: F.cross_entropy in float32 and its autograd gradient (times grad_scale) -> (loss, dlogits [n, C])"""
    z = _select(logits, row_map, n).float().clone().requires_grad_()
    loss = torch.nn.functional.cross_entropy(z, labels[:n].long(), weight=weight)
    loss.backward()
    return loss.detach(), z.grad * torch.tensor(grad_scale, dtype=torch.float32)


def tied_rows(logits, row_map, n):
    """the samples whose maximum is attained more than once"""
    z = _select(logits, row_map, n)
    return torch.nonzero((z == z.max(-1, keepdim=True).values).sum(-1) > 1).flatten().tolist()


def softmax_lse_form32(z):
    """the form cross_entropy_kernel had, and csrc/head.hip (twice), head_ce_kernel and csrc/dgcn_tail.hip still have, in
    float32 torch: exp(z - lse), lse = max + log(sum exp(z - max))"""
    z = z.float()
    mx = z.max(-1, keepdim=True).values
    lse = mx + torch.log(torch.exp(z - mx).sum(-1, keepdim=True))
    return torch.exp(z - lse)


def softmax_max_form32(z):
    """exp(z - max) * (1 / sum): the form of ce_bce_multitask_kernel, and of cross_entropy_kernel now"""
    z = z.float()
    e = torch.exp(z - z.max(-1, keepdim=True).values)
    return e * (1.0 / e.sum(-1, keepdim=True))
