"""Graphs, sources and numpy references shared by tests/test_negatives_host.py and tests/test_gpu_negatives.py.

S  n = 70, about 200 undirected edges.  A round of the row kernel draws 64 ids out of 70, so almost every round repeats
   an id within itself ("the earliest draw wins").  Node 0 has degree 40 (avail = 29 < K for K >= 63); nodes 1, 4, 5
   have degrees 4, 5, 6, so avail is exactly 65, 64, 63; node 2 has degree 0; node 3 stores a self-loop.
H  n = 5,000: node 0 is a hub of degree 4,000 (avail = 999 < 1,024: long binary searches, four of five draws rejected,
   the set at its capacity), the rest a sparse random graph.
C  the complete graph on 6 nodes: no free target and no free pair.

Every reference is computed once per process and handed out read-only."""
from functools import lru_cache
from typing import NamedTuple

import numpy as np

from lpformer_amd import graph
from lpformer_amd.negatives import negatives_reference

ROW_KS = (1, 63, 64, 65)
PAIR_MS = (1, 64, 1000)
SEED = 0x5EED0123456789AB                      # (above 2^62: the seed travels as an unsigned 64-bit integer)


class Case(NamedTuple):
    n: int
    csr: graph.CSR
    und: np.ndarray                             # int64 [2, E]: the undirected edges once, a < b (self-loops apart)
    sources: np.ndarray                         # int64 [R]: the rows of the row form
    held: np.ndarray                            # int64 [2, 40]: free pairs handed to exclude=


def _free_pairs(n, csr, rng, count):
    keys = set((np.repeat(np.arange(n), np.diff(csr.rowptr)) * n + csr.col).tolist())
    out = []
    while len(out) < count:
        a, b = (int(v) for v in rng.integers(0, n, 2))
        if a != b and a * n + b not in keys and b * n + a not in keys and (a, b) not in out and (b, a) not in out:
            out.append((a, b))
    return np.array(out, np.int64).T


def _case_s() -> Case:
    n, rng = 70, np.random.default_rng(11)
    ab = rng.integers(6, n, (2, 400))
    ab = ab[:, ab[0] != ab[1]]
    key = np.unique(np.minimum(ab[0], ab[1]) * n + np.maximum(ab[0], ab[1]))[:150]
    fixed = [(0, v) for v in range(20, 60)] + [(1, v) for v in (10, 11, 12, 13)] + \
            [(4, v) for v in (14, 15, 16, 17, 18)] + [(5, v) for v in (30, 31, 32, 33, 34, 35)]
    und = np.concatenate([np.stack([key // n, key % n]), np.array(fixed, np.int64).T], axis=1)
    csr = graph.mask_csr(np.concatenate([und, np.array([[3], [3]])], axis=1), n, symmetric=True)
    deg = np.diff(csr.rowptr)
    assert deg[0] == 40 and deg[1] == 4 and deg[4] == 5 and deg[5] == 6 and deg[2] == 0 and 3 in csr.col[csr.rowptr[3]:csr.rowptr[4]]
    sources = np.concatenate([[0, 1, 4, 5, 2, 3, -1, n, 7, 7, 7], rng.integers(0, n, 29)]).astype(np.int64)
    return Case(n, csr, und, sources, _free_pairs(n, csr, rng, 40))


def _case_h() -> Case:
    n, rng = 5000, np.random.default_rng(12)
    hub = rng.choice(np.arange(1, n), 4000, replace=False)
    ab = rng.integers(1, n, (2, 5000))
    ab = ab[:, ab[0] != ab[1]]
    key = np.unique(np.concatenate([np.minimum(ab[0], ab[1]) * n + np.maximum(ab[0], ab[1]), hub.astype(np.int64)]))
    und = np.stack([key // n, key % n])
    csr = graph.mask_csr(und, n, symmetric=True)
    assert np.diff(csr.rowptr)[0] == 4000
    sources = np.concatenate([[0, 17, 0], rng.integers(0, n, 297)]).astype(np.int64)
    return Case(n, csr, und, sources, _free_pairs(n, csr, rng, 40))


def _case_c() -> Case:
    n = 6
    a, b = np.triu_indices(n, 1)
    und = np.stack([a, b]).astype(np.int64)
    return Case(n, graph.mask_csr(und, n, symmetric=True), und, np.array([0, 1, 2, 3, 4, 5, 3], np.int64),
                np.zeros((2, 0), np.int64))


_MAKE = {"S": _case_s, "H": _case_h, "C": _case_c}


@lru_cache(maxsize=None)
def case(name: str) -> Case:
    c = _MAKE[name]()
    c.und.setflags(write=False)                 # (sources and held are handed to torch, which wants writable arrays)
    return c


def rows_for(name: str, k: int) -> np.ndarray:
    """The sources of the row tests: H with K = 1,024 takes 12 rows (the hub twice), everything else all of them."""
    src = case(name).sources
    return src[:12] if (name == "H" and k == 1024) else src


@lru_cache(maxsize=None)
def ref_rows(name: str, k: int, exclude: bool = False):
    """(int64 [R, k], short rows), read-only."""
    c = case(name)
    out, short = negatives_reference(c.csr, rows_for(name, k), k, seed=SEED, exclude=c.held if exclude else None,
                                     return_short=True)
    out = out.numpy()
    out.setflags(write=False)
    return out, short


@lru_cache(maxsize=None)
def ref_pairs(name: str, m: int, unique: bool, rounds: int = 8, exclude: bool = False):
    """(int64 [2, m], unresolved slots), read-only."""
    c = case(name)
    out, short = negatives_reference(c.csr, num=m, seed=SEED, unique=unique, rounds=rounds,
                                     exclude=c.held if exclude else None, return_short=True)
    out = out.numpy()
    out.setflags(write=False)
    return out, short


def edge_keys(csr: graph.CSR) -> np.ndarray:
    """row * n + col of every stored entry, ascending."""
    return np.repeat(np.arange(csr.n, dtype=np.int64), np.diff(csr.rowptr)) * csr.n + csr.col.astype(np.int64)


def is_stored(csr: graph.CSR, a, b) -> np.ndarray:
    return np.isin(np.asarray(a, np.int64) * csr.n + np.asarray(b, np.int64), edge_keys(csr))


def check_rows(csr: graph.CSR, sources, rows, extra=None) -> None:
    """No target is the source, in the source's row (or in ``extra``, int64 [2, E], either direction) or out of range;
    the targets of a row are distinct; -1 only as a suffix."""
    n = csr.n
    rows, sources = np.asarray(rows), np.asarray(sources)
    for s, row in zip(sources.tolist(), rows):
        got = row[row >= 0]
        assert (row[got.size:] == -1).all()
        if not 0 <= s < n:
            assert got.size == 0
            continue
        assert got.size == np.unique(got).size and (got < n).all() and s not in got
        assert not is_stored(csr, np.full(got.size, s), got).any()
        if extra is not None and extra.size:
            for a, b in extra.T.tolist():
                assert not (s == a and b in got) and not (s == b and a in got)


def check_pairs(csr: graph.CSR, pairs, unique: bool, extra=None) -> None:
    """Resolved slots hold a != b in [0, n), stored in neither direction (nor in ``extra``); under ``unique`` they are
    distinct as unordered pairs; an unresolved slot is (-1, -1)."""
    n = csr.n
    a, b = np.asarray(pairs)
    ok = a >= 0
    assert ((a < 0) == (b < 0)).all() and (a[~ok] == -1).all() and (b[~ok] == -1).all()
    a, b = a[ok], b[ok]
    assert (a != b).all() and (a < n).all() and (b < n).all() and (b >= 0).all()
    assert not is_stored(csr, a, b).any() and not is_stored(csr, b, a).any()
    key = np.minimum(a, b) * n + np.maximum(a, b)
    if extra is not None and extra.size:
        assert not np.isin(key, np.minimum(extra[0], extra[1]) * n + np.maximum(extra[0], extra[1])).any()
    if unique:
        assert np.unique(key).size == key.size
