"""Synthetic selections for the set-up of ``pair_rows_kernel`` in its PT form (test helper, plain numpy, not collected):
the kernel's split of a batch into workgroup ranges restated, and the batches whose ranges hit the set-up's edges.

The kernel (csrc/pair_rows.hip) balances  EW * entries + pairs.  With  f(p) = p + EW * (entries of the pairs in front of
p)  and  total = f(bs),  workgroup b of ``grid`` owns the pairs [P_b, P_{b+1}):

    P_0 = 0,   P_grid = bs,   P_b = number of pairs p with f(p) < (total * b) // grid     (integer division)

(f is strictly increasing, so that number is the first pair with f(p) >= target; the kernel finds it in two steps -- the
block of 64 pairs from ``blk_cnt``, the pair from the block's 64 ``pair_tab`` entries.)  A range is staged in chunks of
PR_CHUNK pairs; the first chunk by one wavefront from block P_b // 64 on.
"""
from __future__ import annotations

import numpy as np

EW = 4            # weight of an entry against a pair (pair_rows.hip)
SB = 64           # LPF_SELECT4_BLOCK
PR_CHUNK = 512    # pairs of a range staged at a time
UNIT = 16         # entries of a unit


def grid_size(bs: int, n_cu: int, lb_words: int) -> int:
    """Workgroups of the D = 128 / 256 launch: one per CU, at least 16 pairs each, at most the scan words."""
    return int(max(1, min(n_cu, (bs + 15) // 16, lb_words)))


def range_starts(counts, grid: int) -> np.ndarray:
    """P_0 ... P_grid of a batch whose pair p has counts[p] entries (the kernel's integer formula)."""
    counts = np.asarray(counts, np.int64)
    bs = counts.size
    f = np.arange(bs, dtype=np.int64) + EW * (np.cumsum(counts) - counts)
    total = int(bs + EW * counts.sum())
    target = (total * np.arange(grid + 1, dtype=np.int64)) // grid
    p = np.searchsorted(f, target, side="left").astype(np.int64)
    p[0], p[grid] = 0, bs
    return p


def brute_starts(counts, grid: int) -> np.ndarray:
    """The same split, pair by pair: workgroup b starts at the first pair whose weight in front reaches its target."""
    counts = [int(c) for c in counts]
    bs = len(counts)
    total = bs + EW * sum(counts)
    out = [0]
    for b in range(1, grid):
        target = (total * b) // grid
        p, front = 0, 0
        while p < bs and front < target:
            front += 1 + EW * counts[p]
            p += 1
        out.append(p)
    out.append(bs)
    return np.array(out, np.int64)


def split3(counts, rng) -> np.ndarray:
    """[bs, 3] common neighbours / one-hop / further nodes summing to ``counts``."""
    counts = np.asarray(counts, np.int64)
    a = rng.integers(0, counts + 1)
    b = rng.integers(0, counts - a + 1)
    return np.stack([a, b, counts - a - b], axis=1)


def random_counts(bs: int, rng, empty=0.4, top=40) -> np.ndarray:
    c = rng.integers(1, top + 1, bs)
    c[rng.random(bs) < empty] = 0
    return c.astype(np.int64)


def one_pair(bs: int, where: str, n: int) -> np.ndarray:
    """Exactly one pair with entries, in the first, a middle or the last block of 64 pairs."""
    c = np.zeros(bs, np.int64)
    nblk = (bs + SB - 1) // SB
    p = {"first": 5, "middle": (nblk // 2) * SB + 31, "last": bs - 1}[where]
    c[p] = n
    return c


def lane_edges(grid: int, bs: int = 3000, seed: int = 0):
    """A batch in which some range starts on lane 0 of a block and some on lane 63 (and the two workgroups)."""
    for s in range(seed, seed + 200):
        c = random_counts(bs, np.random.default_rng(s))
        p = range_starts(c, grid)[1:grid]
        lane = p % SB
        if (lane == 0).any() and (lane == SB - 1).any():
            return c, int(np.flatnonzero(lane == 0)[0]) + 1, int(np.flatnonzero(lane == SB - 1)[0]) + 1
    raise AssertionError("no batch with range ends on lanes 0 and 63")


def hub(grid: int, bs: int = 2000, n_hub: int = 5000, seed: int = 0):
    """One pair whose entries alone exceed a workgroup's share: (counts, the hub pair)."""
    rng = np.random.default_rng(seed)
    c = random_counts(bs, rng, empty=0.5, top=6)
    p = bs // 2 + 7
    c[p] = n_hub
    return c, p


def long_ranges(grid: int, seed: int = 0):
    """Ranges longer than PR_CHUNK pairs: (PR_CHUNK + 38) pairs per workgroup, almost all of them empty."""
    rng = np.random.default_rng(seed)
    bs = (PR_CHUNK + 38) * grid
    c = np.zeros(bs, np.int64)
    pick = rng.choice(bs, 6 * grid, replace=False)
    c[pick] = rng.integers(1, 4, pick.size)
    c[pick[:8]] = 40                                   # (a few pairs of several units)
    return c


def range_facts(counts, grid: int) -> dict:
    """What the cases assert about their own split."""
    p = range_starts(counts, grid)
    n = np.diff(p)
    counts = np.asarray(counts, np.int64)
    ne = np.flatnonzero(counts > 0)
    b_of = np.searchsorted(p, ne, side="right") - 1       # workgroup of every pair with entries
    ofs = ne - p[b_of]
    return {"starts": p, "len": n, "nonempty": ne, "wg": b_of, "ofs": ofs}
