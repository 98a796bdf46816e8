"""Shared cases of tests/test_bootstrap_host.py and tests/test_gpu_bootstrap.py: the draw restated on Python integers,
tables with awkward values, scores with ties and NaNs, and the float bounds both files assert."""
import numpy as np
import torch

from lpformer_amd import negatives

SEEDS = (0, 2 ** 63 + 5, 2 ** 64 - 1)
G = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
EPS = 2.0 ** -52


def py_mix64(z: int) -> int:
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def py_indices(p: int, b: int, seed: int) -> list:
    """idx(b, j), j < p, one draw at a time on Python integers -- (u * p) >> 64 included."""
    key = py_mix64(seed + G * (b + 1))
    return [(py_mix64(key + G * (j + 1)) * p) >> 64 for j in range(p)]


def tables(p: int, ci: int, cf: int, rng_seed: int = 0):
    """int64 [p, ci] with negatives and +-2^32 among the values, float64 [p, cf] of mixed sign and magnitude."""
    rng = np.random.default_rng(rng_seed)
    icols = rng.integers(-1000, 1000, size=(p, ci), dtype=np.int64)
    big = rng.random((p, ci))
    icols[big < 0.05] = 1 << 32
    icols[big > 0.95] = -(1 << 32)
    fcols = rng.standard_normal((p, cf)) * np.exp(rng.uniform(-20, 20, size=(p, cf)))
    return icols, fcols


def sum_bound(fcols: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """P 2^-52 sum_j |fcols[idx_j]| per (replicate, column): twice the worst case of summing P terms in any order."""
    return idx.shape[1] * EPS * np.abs(fcols[idx]).sum(axis=1)


def mrr_bound(p: int, mrr: float) -> float:
    """The same bound for a mean of P reciprocal ranks (sum_j |x_j| = P * MRR), plus an ulp of 1 for the division."""
    return p * EPS * abs(mrr) + EPS


def scores(p: int, layout: str, rng_seed: int = 1, k: int = 12, m: int = 300):
    """(pos float32 [p], neg float32 [m] or [p, k]) on a coarse grid -- many ties -- with NaNs on both sides."""
    g = torch.Generator().manual_seed(rng_seed)
    pos = torch.randint(0, 40, (p,), generator=g).float() / 4
    neg = torch.randint(0, 40, (p, k) if layout == "rows" else (m,), generator=g).float() / 4
    if p > 4:
        pos[3] = float("nan")
        pos[p // 2] = float("nan")
    neg.view(-1)[1] = float("nan")
    neg.view(-1)[neg.numel() // 3] = float("nan")
    return pos, neg


def np_indices(p: int, b: int, seed: int, first: int = 0) -> np.ndarray:
    key = negatives.draw_key(seed, np.arange(first, first + b, dtype=np.uint64))
    return negatives.draw_node(negatives.draw_u(key[:, None], np.arange(p, dtype=np.uint64)[None, :]), p)
