"""The numpy restatement of pair_rows' range split (tests/rows_setup_cases.py) against a pair-by-pair split, and the
properties the GPU cases of tests/test_gpu_rows_setup.py rely on, pinned on the CPU."""
import numpy as np
import pytest

from tests import rows_setup_cases as C

GRID = 256          # workgroups of the D = 128 launch on a 256-CU device
LB = 1023


@pytest.mark.parametrize("bs,grid", [(1, 1), (63, 4), (64, 4), (65, 5), (130, 9), (1000, 63), (3000, 188), (5000, 256)])
def test_range_formula_matches_brute_force(bs, grid):
    assert C.grid_size(bs, GRID, LB) == grid
    for seed in range(4):
        rng = np.random.default_rng(100 * bs + seed)
        for counts in (C.random_counts(bs, rng), C.random_counts(bs, rng, empty=0.95, top=3),
                       np.zeros(bs, np.int64), C.random_counts(bs, rng, empty=0.0, top=700 if bs < 200 else 60)):
            p = C.range_starts(counts, grid)
            assert np.array_equal(p, C.brute_starts(counts, grid))
            assert p[0] == 0 and p[-1] == bs and (np.diff(p) >= 0).all()


def test_fewer_pairs_than_workgroups_gives_target_zero_ranges():
    # bs = 1: one workgroup; bs = 17 ... : (total * b) // grid is 0 for no b > 0 as soon as a pair has entries, but an
    # all-empty batch of 16 g pairs has targets 16 b: no range is cut inside a unit of 16 pairs
    assert np.array_equal(C.range_starts(np.zeros(1, np.int64), 1), [0, 1])
    assert np.array_equal(C.range_starts(np.zeros(130, np.int64), 9), (130 * np.arange(10)) // 9)
    # one pair with all the entries in a batch smaller than the grid: the workgroups behind its own start where it ends
    c = C.one_pair(63, "first", 700)
    p = C.range_starts(c, 4)
    assert np.array_equal(p, C.brute_starts(c, 4)) and (np.diff(p) == 0).any()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("n", [1, 16, 17, 700])
def test_one_pair_cases(where, n):
    c = C.one_pair(1000, where, n)
    assert (c > 0).sum() == 1 and c.sum() == n
    p = int(np.flatnonzero(c)[0])
    assert p // C.SB == {"first": 0, "middle": 8, "last": 15}[where]
    assert np.array_equal(C.range_starts(c, 63), C.brute_starts(c, 63))


def test_lane_edges_case():
    grid = C.grid_size(3000, GRID, LB)
    c, b0, b63 = C.lane_edges(grid)
    p = C.brute_starts(c, grid)
    assert p[b0] % C.SB == 0 and p[b63] % C.SB == C.SB - 1 and 0 < b0 < grid and 0 < b63 < grid


def test_hub_case():
    grid = C.grid_size(2000, GRID, LB)
    c, hp = C.hub(grid)
    f = C.range_facts(c, grid)
    total = c.size + C.EW * c.sum()
    assert C.EW * c[hp] > 20 * (total // grid)                    # the hub alone: more than twenty shares
    assert c[hp] > 64 * C.UNIT                                    # ... and many units
    b = int(f["wg"][np.flatnonzero(f["nonempty"] == hp)[0]])
    assert (f["len"][b + 1:b + 20] == 0).all()                    # the neighbours behind it own nothing
    assert np.array_equal(f["starts"], C.brute_starts(c, grid))


def test_long_range_case():
    c = C.long_ranges(GRID)
    assert c.size >= 140000 and (c > 0).mean() < 0.02
    f = C.range_facts(c, GRID)
    long_ = f["len"] > C.PR_CHUNK
    assert long_.sum() > GRID // 2
    second = long_[f["wg"]] & (f["ofs"] >= C.PR_CHUNK)            # pairs with entries in a second chunk
    first = long_[f["wg"]] & (f["ofs"] < C.PR_CHUNK)
    assert second.sum() >= 8 and first.sum() >= 8
    assert len(set(f["wg"][second]) & set(f["wg"][first])) >= 4   # ... both in one range
