"""Plain restatements of the pair stage's training kernels (csrc/pair_train.hip), shared by the tests that pin them:
tests/test_gpu_train.py, tests/test_gpu_train_kernels.py (device) and tests/test_train_reference_host.py (CPU).

Everything here is torch on whatever device and in whatever dtype its floating-point inputs have -- float64 for the
reference proper (hence the names), float32 for the yardstick that tells the limit of fp32 from a defect -- except
``segment_sum_seq32``, which is numpy and bit-exact by construction.  Nothing imports the package under test.

Layout, as in the kernels: the entries are sorted by (type, pair); ``seg`` [n_t, bs + 1] holds the first entry of pair
p's type-t segment as a global entry index, ``tbase`` [n_t + 1] the first entry of each type (tbase[t] == seg[t, 0],
tbase[t + 1] == seg[t, bs])."""
import numpy as np
import torch


def pair_of_entries(seg, device=None):
    """The pair of every entry, [n] int64, from ``seg`` [n_t, bs + 1] (numpy or nested lists)."""
    seg = np.asarray(seg, dtype=np.int64)
    bs = seg.shape[1] - 1
    pair = np.concatenate([np.repeat(np.arange(bs, dtype=np.int64), np.diff(seg[t])) for t in range(seg.shape[0])])
    return torch.from_numpy(pair).to(device) if device is not None else torch.from_numpy(pair)


def layout(counts):
    """``counts`` [n_t, bs] entries per (type, pair) -> (seg [n_t, bs + 1] int64 numpy, tbase list, n)."""
    counts = np.asarray(counts, dtype=np.int64)
    n_t, bs = counts.shape
    seg = np.zeros((n_t, bs + 1), np.int64)
    base, tbase = 0, [0]
    for t in range(n_t):
        seg[t, 0] = base
        seg[t, 1:] = base + np.cumsum(counts[t])
        base = int(seg[t, bs])
        tbase.append(base)
    return seg, tbase, base


def pe_hidden64(w1, b1, gamma, beta, pa, pb, relu_args=False):
    """The PE hidden layer of ONE type: ReLU(LN(W1 [pa, pb] + b1)) + ReLU(LN(W1 [pb, pa] + b1)) -> [m, dh], LayerNorm with
    the biased variance and eps 1e-5.  w1 [dh, 2]; b1 / gamma / beta [dh]; pa / pb [m].  ``relu_args``: also the two
    [m, dh] arguments of the ReLUs (a test keeps its inputs away from the kink with them)."""
    def g(x, y):
        u = x[:, None] * w1[:, 0] + y[:, None] * w1[:, 1] + b1
        mu, var = u.mean(1, keepdim=True), u.var(1, unbiased=False, keepdim=True)
        return (u - mu) / torch.sqrt(var + 1e-5) * gamma + beta
    a1, a2 = g(pa, pb), g(pb, pa)
    h = torch.relu(a1) + torch.relu(a2)
    return (h, a1, a2) if relu_args else h


def attention64(z, q, att, bias, wfold, bfold, w1s, b1s, gams, bets, e_node, e_pa, e_pb, pair, tbase, detail=False):
    """What ``train.PairAttentionFn`` computes, [bs, d]: per type t the hidden layer h (width dh), the folded key
    projection kp = h Wfold_t^T + bfold_t (one product per type; wfold [n_t, d, dh]), k = Z[node] + kp, the score
    s = att . leaky_relu(k * q_pair, 0.2), PyG's segment softmax over the entries of a pair (max-shifted, denominator
    + 1e-16), out = scatter-sum of alpha k + bias.  ``pair``: ``pair_of_entries(seg)`` on the inputs' device; ``e_node``
    any integer dtype; ``e_pa`` / ``e_pb`` in the dtype of ``z``.  ``detail``: (out, scores s, leaky-ReLU arguments)."""
    bs, d = q.shape
    kps = []
    for t in range(wfold.shape[0]):
        lo, hi = tbase[t], tbase[t + 1]
        h = pe_hidden64(w1s[t], b1s[t], gams[t], bets[t], e_pa[lo:hi], e_pb[lo:hi])
        kps.append(h @ wfold[t].t() + bfold[t])
    k = z[e_node.long()] + torch.cat(kps)
    x = k * q[pair]
    s = (torch.nn.functional.leaky_relu(x, 0.2) * att).sum(1)
    smax = torch.full((bs,), -float("inf"), dtype=z.dtype, device=z.device).scatter_reduce(0, pair, s.detach(), "amax")
    w = torch.exp(s - smax[pair])
    den = torch.zeros(bs, dtype=z.dtype, device=z.device).index_add(0, pair, w) + 1e-16
    out = torch.zeros(bs, d, dtype=z.dtype, device=z.device).index_add(0, pair, (w / den[pair])[:, None] * k) + bias
    return (out, s, x) if detail else out


def score_ranges(s, pair, bs):
    """max - min of the scores of every pair, [bs] (0 for a pair without entries)."""
    s = s.detach()
    hi = torch.full((bs,), -float("inf"), dtype=s.dtype, device=s.device).scatter_reduce(0, pair, s, "amax")
    lo = torch.full((bs,), float("inf"), dtype=s.dtype, device=s.device).scatter_reduce(0, pair, s, "amin")
    return torch.where(torch.isfinite(hi), hi - lo, torch.zeros_like(hi))


def pair_gather64(x, batch, product):
    """x[a] * x[b] (``product``) or x[a] + x[b] of the pairs ``batch`` [2, bs], in the dtype of ``x``."""
    xa, xb = x[batch[0]], x[batch[1]]
    return xa * xb if product else xa + xb


def segment_sum_seq32(keys_sorted, order, src):
    """``segment_sum_kernel`` restated exactly: for each run of equal keys in ``keys_sorted`` [n] the rows
    ``src[order[j]]`` added in ascending j in float32, starting from 0 -> (keys [r] int64, one per run, ascending with
    the list; sums [r, D] float32).  The kernel only adds, so there is nothing a compiler could contract: the result is
    the kernel's bit for bit."""
    keys_sorted, order = np.asarray(keys_sorted).astype(np.int64), np.asarray(order).astype(np.int64)
    src = np.ascontiguousarray(np.asarray(src), dtype=np.float32)
    n = keys_sorted.shape[0]
    keys, sums = [], []
    acc = None
    for j in range(n):
        if j == 0 or keys_sorted[j] != keys_sorted[j - 1]:
            acc = np.zeros(src.shape[1], np.float32)
            keys.append(int(keys_sorted[j]))
            sums.append(acc)
        acc += src[order[j]]          # (in place: float32 + float32 -> float32, one rounding per addition)
    if not keys:
        return np.zeros(0, np.int64), np.zeros((0, src.shape[1]), np.float32)
    return np.asarray(keys, np.int64), np.stack(sums)
