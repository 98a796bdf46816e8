"""Uniform negatives that avoid known edges, drawn on the device.

``train_epoch`` draws ``torch.randint`` pairs as the reference does (src/train/train_model.py:64): on a dense graph a
good share of those "negatives" are edges.  ``heart_negatives`` makes HARD negatives; nothing else in the package samples
a pair that is known not to be an edge.  Here

    negative_rows(source, nodes, k, seed=...)      int64 [R, k]: k distinct non-neighbours per source (citation2 / HeaRT)
    negative_pairs(source, num, seed=...)          int64 [2, num]: non-edges, distinct as unordered pairs (collab / ppa / ddi)
    UniformNegatives(source, seed=...)             (step, edges) -> [2, B * num_negative] for train_epoch(negatives=...)
    negatives_reference(...)                       the numpy restatement of both, what a host CSR without a GPU runs

One definition of the draw is shared by the kernels (csrc/neg_sample.hip, include/lpformer_hip.h) and the restatement,
all in uint64::

    mix64(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
    G = 0x9E3779B97F4A7C15;  key(seed, i) = mix64(seed + G (i + 1));  u(seed, i, j) = mix64(key(seed, i) + G (j + 1))
    node(u, n) = (u * n) >> 64

Rows.  Row r (slot ``row_base + r``) has the source ``s = nodes[r]`` and the stream ``c_j = node(u(seed, slot, j), n)``.
A draw is accepted iff ``c_j != s``, ``c_j`` is not in row s of the known graph and ``c_j`` is no earlier accepted draw
of the row.  The row is the first ``min(k, avail)`` accepted draws in stream order, ``avail = n - deg(s) - [s not in row
s]``, then -1; it stops after ``max_draws`` draws; a source outside [0, n) gives -1 throughout.  So the k'-prefix of a row
is the row for k', a row depends on its slot only (rows [lo, hi) with ``row_base=lo`` are those rows of the whole call)
and a source named twice gets two different rows.

Pairs.  Slot i (``slot_base + i``) draws ``a = node(u(seed, slot, 2 j), n)``, ``b = node(u(seed, slot, 2 j + 1), n)``
for j = 0, 1, ... and takes the first with ``a != b`` that is stored in neither direction; after ``max_draws`` draws it
holds (-1, -1).  ``unique=True`` removes repeats ACROSS slots by a rule that does not depend on any order of execution:
with the canonical key ``min * n + max``, a slot is a loser iff a slot with a smaller index holds the same key; losers
draw on from where their stream stands, ``rounds`` draws in all, and whoever is a loser after the last becomes (-1, -1).

The known graph is the source's typing adjacency united with ``exclude`` (held-out positives, say), both directions of
every excluded edge.  Every output is a pure function of (seed, slot, graph, options); two runs are bitwise equal.
"""
from __future__ import annotations

import weakref

import numpy as np
import torch

from . import _lib, graph, ops, sources
from ._lib import check as _check_rc, ptr

MAX_K = _lib.CONST["LPF_NEGATIVE_MAX_K"]
MAX_DRAWS = _lib.CONST["LPF_NEGATIVE_MAX_DRAWS"]
ROW_DRAWS = _lib.CONST["LPF_NEGATIVE_ROW_DRAWS_DEFAULT"]
PAIR_DRAWS = _lib.CONST["LPF_NEGATIVE_PAIR_DRAWS_DEFAULT"]
G = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1

_UNION: dict = {}                     # per adjacency object: {id(exclude): (weak reference, union CSR)}


# --------------------------------------------------------------------------------------------------------- the draw
def mix64(z: int) -> int:
    """The finaliser of splitmix64 on a Python integer (taken modulo 2^64)."""
    z &= _M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def step_seed(seed: int, step: int) -> int:
    """``mix64(seed + G (step + 1))``: the seed ``UniformNegatives`` gives step ``step``."""
    return mix64(int(seed) + G * (int(step) + 1))


def _u64(v) -> np.ndarray:
    if isinstance(v, (int, np.integer)):
        return np.array([int(v) & _M64], dtype=np.uint64)
    return np.asarray(v).astype(np.uint64)


def mix64_np(z) -> np.ndarray:
    """``mix64`` on a uint64 array (wrapping arithmetic)."""
    z = _u64(z).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def draw_key(seed: int, slot) -> np.ndarray:
    """``key(seed, i) = mix64(seed + G (i + 1))`` for the slots ``slot`` (uint64 array out)."""
    with np.errstate(over="ignore"):
        return mix64_np(_u64(seed) + np.uint64(G) * (_u64(slot) + np.uint64(1)))


def draw_u(key, j) -> np.ndarray:
    """``u = mix64(key + G (j + 1))``: draw j of the stream that starts at ``key`` (broadcasts)."""
    with np.errstate(over="ignore"):
        return mix64_np(_u64(key) + np.uint64(G) * (_u64(j) + np.uint64(1)))


def draw_node(u, n: int) -> np.ndarray:
    """``(u * n) >> 64`` as int64, exact for n < 2^31 from the two 32-bit halves of u:
    ``((u >> 32) n + (((u & 0xffffffff) n) >> 32)) >> 32`` -- neither product nor the sum reaches 2^64."""
    if not 0 < int(n) < 1 << 31:
        raise ValueError("n must be in [1, 2^31)")
    u, n64, s32 = _u64(u), np.uint64(int(n)), np.uint64(32)
    return (((u >> s32) * n64 + (((u & np.uint64(0xFFFFFFFF)) * n64) >> s32)) >> s32).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------- options
def _check_seed(seed) -> int:
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"seed must be an integer; got {seed!r}")
    return int(seed) & _M64


def _check_count(v, what: str, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{what} must be an integer in [{lo}, {hi}]; got {v!r}")
    return int(v)


def _check_n(n: int) -> int:
    if not 0 < int(n) < (1 << 31) - 1:
        raise ValueError(f"the graph must have between 1 and 2^31 - 2 nodes; got {n}")
    return int(n)


# ------------------------------------------------------------------------------------------------- the known graph
def _exclude_coo(exclude, n: int):
    """(row, col) int64 numpy arrays or torch tensors of ``exclude`` as given (one direction)."""
    if isinstance(exclude, graph.DeviceCSR):
        rows = torch.repeat_interleave(torch.arange(exclude.n, dtype=torch.int64, device=exclude.col.device),
                                       exclude.rowptr[1:] - exclude.rowptr[:-1])
        return rows, exclude.col.long()
    if isinstance(exclude, graph.CSR):
        rows = np.repeat(np.arange(exclude.n, dtype=np.int64), np.diff(exclude.rowptr))
        return torch.from_numpy(rows), torch.from_numpy(exclude.col.astype(np.int64))
    e = sources.as_pairs(exclude, what="exclude")
    return e[0].to(torch.int64), e[1].to(torch.int64)


def _cached_union(adj, exclude, make):
    """``make()`` once per live (adjacency object, ``exclude`` object): the union is kept while both live.  An
    ``exclude`` that cannot be weakly referenced (a list) is united on every call."""
    try:
        weakref.ref(exclude)
    except TypeError:
        return make()
    return sources.per_object(sources.per_object(_UNION, adj, dict), exclude, make)


def _known_device(adj: graph.DeviceCSR, exclude, dev) -> graph.DeviceCSR:
    """The adjacency united with both directions of ``exclude`` (ids outside [0, n) dropped), on the device, built once
    per object pair.  An ``exclude`` tensor changed in place afterwards is NOT seen: pass a new tensor."""
    if exclude is None:
        return adj

    def make():
        n = adj.n
        r, c = _exclude_coo(exclude, n)
        r, c = r.to(dev), c.to(dev)
        ok = (r >= 0) & (r < n) & (c >= 0) & (c < n)
        r, c = r[ok], c[ok]
        arow = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), adj.rowptr[1:] - adj.rowptr[:-1])
        return graph.csr_from_coo_device(torch.cat([arow, r, c]), torch.cat([adj.col.long(), c, r]), None, n,
                                         keep_val=False)
    return _cached_union(adj, exclude, make)


def _known_host(adj: graph.CSR, exclude) -> graph.CSR:
    if exclude is None:
        return adj

    def make():
        n = int(adj.n)
        if isinstance(exclude, graph.DeviceCSR):
            r, c = _exclude_coo(exclude.to_host(), n)
        else:
            r, c = _exclude_coo(exclude, n)
        r, c = r.cpu().numpy(), c.cpu().numpy()
        ok = (r >= 0) & (r < n) & (c >= 0) & (c < n)
        r, c = r[ok], c[ok]
        arow = np.repeat(np.arange(n, dtype=np.int64), np.diff(adj.rowptr))
        return graph.csr_from_coo(np.concatenate([arow, r, c]), np.concatenate([adj.col.astype(np.int64), c, r]), None, n)
    return _cached_union(adj, exclude, make)


# ------------------------------------------------------------------------------------------------- host restatement
def _entry_keys(adj: graph.CSR) -> np.ndarray:
    """row * n + col of every stored entry: ascending, the CSR's own order."""
    n = int(adj.n)
    return np.repeat(np.arange(n, dtype=np.int64), np.diff(adj.rowptr)) * n + np.asarray(adj.col).astype(np.int64)


def _stored(keys: np.ndarray, n: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    if not keys.size:
        return np.zeros(a.shape, bool)
    q = a * np.int64(n) + b
    return keys[np.minimum(np.searchsorted(keys, q), keys.size - 1)] == q


def _rows_np(adj: graph.CSR, nodes: np.ndarray, k: int, seed: int, row_base: int, max_draws: int):
    n = int(adj.n)
    rowptr, col = np.asarray(adj.rowptr, np.int64), np.asarray(adj.col).astype(np.int64)
    out = np.full((nodes.size, k), -1, np.int64)
    blocked = np.zeros(n, bool)                  # the source, its row and what the row accepted; cleared per row
    short = 0
    for r, s in enumerate(nodes.tolist()):
        if not 0 <= s < n:
            short += 1
            continue
        row = col[rowptr[s]:rowptr[s + 1]]
        avail = n - row.size - (0 if _row_has(row, s) else 1)
        want = min(k, max(avail, 0))
        blocked[row] = True
        blocked[s] = True
        key = draw_key(seed, (int(row_base) + r) & _M64)
        kept, j0 = 0, 0
        while kept < want and j0 < max_draws:
            m = min(max(64, 4 * (want - kept)), max_draws - j0)
            c = draw_node(draw_u(key, np.arange(j0, j0 + m, dtype=np.uint64)), n)
            cand = c[~blocked[c]]
            if cand.size:                        # the first occurrence of each id, in stream order
                _, first = np.unique(cand, return_index=True)
                new = cand[np.sort(first)][:want - kept]
                out[r, kept:kept + new.size] = new
                blocked[new] = True
                kept += new.size
            j0 += m
        blocked[row] = False
        blocked[s] = False
        blocked[out[r, :kept]] = False
        short += kept < k
    return out, short


def _row_has(row: np.ndarray, s: int) -> bool:
    """Whether the sorted row holds s."""
    i = int(np.searchsorted(row, s))
    return i < row.size and int(row[i]) == s


def _has_free_pair(keys: np.ndarray, n: int) -> bool:
    """Whether any unordered pair {a, b}, a != b, is stored in neither direction."""
    r, c = keys // n, keys % n
    off = r != c
    taken = np.unique(np.minimum(r[off], c[off]) * np.int64(n) + np.maximum(r[off], c[off])).size
    return taken < n * (n - 1) // 2


def _draw_pairs_np(keys, n, free, seed, slot_base, todo, nxt, pairs, max_draws) -> int:
    """One launch of the pair kernel for the slots ``todo`` (ascending indices): ``pairs`` [2, M] and ``nxt`` [M] are
    updated in place; returns the number of slots left at (-1, -1).  ``free``: ``_has_free_pair`` of the graph."""
    if not todo.size:
        return 0
    if not free:                                 # no draw can be accepted: what max_draws rejections end in
        pairs[:, todo] = -1
        nxt[todo] = max_draws
        return int(todo.size)
    skey = draw_key(seed, (todo.astype(np.uint64) + np.uint64(int(slot_base) & _M64)))
    nxt[todo] = np.maximum(nxt[todo], 0)
    lost, chunk = 0, 4
    while todo.size:
        j = nxt[todo].astype(np.int64)[:, None] + np.arange(chunk, dtype=np.int64)[None, :]
        ju = j.astype(np.uint64)
        a = draw_node(draw_u(skey[:, None], np.uint64(2) * ju), n)
        b = draw_node(draw_u(skey[:, None], np.uint64(2) * ju + np.uint64(1)), n)
        ok = (j < max_draws) & (a != b) & ~_stored(keys, n, a, b) & ~_stored(keys, n, b, a)
        hit = ok.any(axis=1)
        first = ok.argmax(axis=1)
        rows = np.flatnonzero(hit)
        pairs[0, todo[rows]], pairs[1, todo[rows]] = a[rows, first[rows]], b[rows, first[rows]]
        nxt[todo[rows]] = j[rows, first[rows]] + 1
        rest = np.flatnonzero(~hit)
        nxt[todo[rest]] = np.minimum(nxt[todo[rest]].astype(np.int64) + chunk, max_draws)
        out = rest[nxt[todo[rest]] >= max_draws]
        pairs[:, todo[out]] = -1
        lost += out.size
        go = rest[nxt[todo[rest]] < max_draws]
        todo, skey = todo[go], skey[go]
        chunk = max(4, min(chunk * 4, (1 << 20) // max(todo.size, 1)))
    return lost


def _losers_np(pairs: np.ndarray, n: int) -> np.ndarray:
    """bool [M]: slots whose canonical key ``min * n + max`` a slot with a smaller index holds too."""
    m = pairs.shape[1]
    key = np.where(pairs[0] >= 0, np.minimum(pairs[0], pairs[1]) * np.int64(n) + np.maximum(pairs[0], pairs[1]),
                   np.int64(n) * n + np.arange(m, dtype=np.int64))
    order = np.argsort(key, kind="stable")
    dup = np.zeros(m, bool)
    dup[1:] = key[order][1:] == key[order][:-1]
    lose = np.zeros(m, bool)
    lose[order] = dup
    return lose


def _pairs_np(adj: graph.CSR, num: int, seed: int, slot_base: int, unique: bool, rounds: int, max_draws: int):
    n = int(adj.n)
    keys = _entry_keys(adj)
    pairs = np.full((2, num), -1, np.int64)
    nxt = np.zeros(num, np.int32)
    free = _has_free_pair(keys, n)
    short = _draw_pairs_np(keys, n, free, seed, slot_base, np.arange(num), nxt, pairs, max_draws)
    if unique:
        for _ in range(1, rounds):
            _draw_pairs_np(keys, n, free, seed, slot_base, np.flatnonzero(_losers_np(pairs, n)), nxt, pairs, max_draws)
        pairs[:, _losers_np(pairs, n)] = -1
        short = int((pairs[0] < 0).sum())
    return pairs, short


def negatives_reference(adj: graph.CSR, nodes=None, k=None, num=None, *, seed, exclude=None, unique: bool = True,
                        rounds: int = 8, row_base: int = 0, slot_base: int = 0, max_draws=None,
                        return_short: bool = False):
    """The numpy restatement of both forms on a host CSR (CPU int64 tensors out): with ``nodes`` and ``k`` the rows of
    ``negative_rows`` [R, k], with ``num`` the pairs of ``negative_pairs`` [2, num], the rounds of ``unique`` included.
    ``return_short``: (tensor, the number of rows with a -1 / of slots at (-1, -1)).  What the kernels are tested
    against, and what a host ``graph.CSR`` source runs when there is no GPU."""
    if not isinstance(adj, graph.CSR):
        raise TypeError("negatives_reference takes a host graph.CSR")
    _check_n(adj.n)
    seed = _check_seed(seed)
    known = _known_host(adj, exclude)
    if (nodes is None) == (num is None):
        raise ValueError("give either nodes and k (rows) or num (pairs)")
    if nodes is not None:
        k = _check_count(k, "k", 1, MAX_K)
        md = _check_count(ROW_DRAWS if max_draws is None else max_draws, "max_draws", 1, MAX_DRAWS)
        ids = sources.node_ids(nodes, "nodes", ValueError).reshape(-1).cpu().to(torch.int64).numpy()
        out, short = _rows_np(known, ids, k, seed, int(row_base), md)
    else:
        num = _check_count(num, "num", 0, (1 << 31) - 2)
        md = _check_count(PAIR_DRAWS if max_draws is None else max_draws, "max_draws", 1, MAX_DRAWS)
        out, short = _pairs_np(known, num, seed, int(slot_base), bool(unique), _check_count(rounds, "rounds", 1, 1 << 16), md)
    out = torch.from_numpy(out)
    return (out, int(short)) if return_short else out


# ------------------------------------------------------------------------------------------------------ device path
def _raise_short(short: int, total: int, what: str, who: str) -> None:
    if short:
        raise ValueError(f"{who}: {short} of {total} {what} came up short (-1 entries): the known graph leaves too few "
                         "free targets; ask for fewer, or pass check=False and handle the -1 entries")


def _as_row_pairs(nodes: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """[R, k, 2]: (source, target) as ``score_negatives`` / ``heart=True`` evaluation take it."""
    return torch.stack([nodes.to(rows.device)[:, None].expand_as(rows), rows], dim=-1)


@torch.no_grad()
def negative_rows(source, nodes, k, *, seed, test_set: bool = False, exclude=None, as_pairs: bool = False,
                  check: bool = True, row_base: int = 0, max_draws=None) -> torch.Tensor:
    """``k`` distinct uniform non-neighbours for each source in ``nodes`` [R]: int64 [R, k] on the device, -1 where a
    row ran out (module docstring: the contract).  ``as_pairs``: [R, k, 2] = (source, target).

    ``source``: a ``LinkTransformer`` (the typing adjacency of the split ``test_set`` selects), a ``graph.DeviceCSR``
    or a ``graph.CSR``.  ``exclude``: further edges to avoid, [2, E] / [E, 2] or a CSR, both directions; united with
    the adjacency once per object.  ``row_base``: the slot of row 0.  ``check=True`` reads the one counter of the call
    and raises ``ValueError`` naming how many rows came up short; ``check=False`` reads nothing back.
    A host ``graph.CSR`` with CPU ``nodes`` and no GPU present goes through ``negatives_reference``."""
    k = _check_count(k, "k", 1, MAX_K)
    seed = _check_seed(seed)
    md = _check_count(ROW_DRAWS if max_draws is None else max_draws, "max_draws", 1, MAX_DRAWS)
    ids = sources.node_ids(nodes, "nodes", ValueError).reshape(-1)
    dev, adj, _, _ = sources.resolve(source, test_set, ids, who="negative_rows", host_ok=True)
    _check_n(adj.n)
    R = ids.numel()
    if dev is None:
        out, short = negatives_reference(adj, ids, k, seed=seed, exclude=exclude, row_base=row_base, max_draws=md,
                                         return_short=True)
        ids = ids.to(torch.int64)
    else:
        ids = ids.to(dev, dtype=torch.int64).contiguous()
        with torch.cuda.device(dev):
            known = _known_device(adj, exclude, dev)
            out = torch.empty((R, k), dtype=torch.int64, device=dev)
            short = torch.zeros(1, dtype=torch.int64, device=dev)
            _check_rc(_lib.hip().lpf_negative_rows(R, known.n, ptr(ids), k, ptr(known.rowptr), ptr(known.col), seed,
                                                   int(row_base), md, ptr(out), ptr(short), ops.raw_stream(dev)),
                      "lpf_negative_rows")
    if check:
        _raise_short(int(short), R, "rows", "negative_rows")
    return _as_row_pairs(ids, out) if as_pairs else out


def _losers(pairs: torch.Tensor, n: int) -> torch.Tensor:
    """bool [M] on the device, nothing read back: a stable sort of the canonical keys and a neighbour compare."""
    m = pairs.shape[1]
    idx = torch.arange(m, dtype=torch.int64, device=pairs.device)
    key = torch.where(pairs[0] >= 0, torch.minimum(pairs[0], pairs[1]) * n + torch.maximum(pairs[0], pairs[1]),
                      n * n + idx)
    skey, order = torch.sort(key, stable=True)
    dup = torch.zeros(m, dtype=torch.bool, device=pairs.device)
    dup[1:] = skey[1:] == skey[:-1]
    return torch.zeros(m, dtype=torch.bool, device=pairs.device).index_put_((order,), dup)


@torch.no_grad()
def negative_pairs(source, num, *, seed, test_set: bool = False, exclude=None, unique: bool = True, rounds: int = 8,
                   check: bool = True, slot_base: int = 0, max_draws=None) -> torch.Tensor:
    """``num`` uniform pairs (a, b), a != b, stored in the known graph in neither direction: int64 [2, num] on the
    device, (-1, -1) where a slot found none (module docstring: the contract).

    ``unique``: no unordered pair twice -- ``rounds`` launches, losers by slot index drawing on, the losers of the last
    round (-1, -1).  ``source``, ``exclude``, ``check``: as for ``negative_rows``; ``slot_base``: the slot of pair 0.
    Loser detection is a torch sort on the device; with ``check=False`` nothing is read back.
    A host ``graph.CSR`` and no GPU present goes through ``negatives_reference``."""
    num = _check_count(num, "num", 0, (1 << 31) - 2)
    seed = _check_seed(seed)
    rounds = _check_count(rounds, "rounds", 1, 1 << 16)
    md = _check_count(PAIR_DRAWS if max_draws is None else max_draws, "max_draws", 1, MAX_DRAWS)
    dev, adj, _, _ = sources.resolve(source, test_set, torch.empty(0), who="negative_pairs", host_ok=True)
    n = _check_n(adj.n)
    if dev is None:
        out, short = negatives_reference(adj, num=num, seed=seed, exclude=exclude, unique=unique, rounds=rounds,
                                         slot_base=slot_base, max_draws=md, return_short=True)
    else:
        with torch.cuda.device(dev):
            known = _known_device(adj, exclude, dev)
            out = torch.full((2, num), -1, dtype=torch.int64, device=dev)
            nxt = torch.zeros(max(num, 1), dtype=torch.int32, device=dev)
            short = torch.zeros(1, dtype=torch.int64, device=dev)
            hip, st = _lib.hip(), ops.raw_stream(dev)

            def launch(active):
                _check_rc(hip.lpf_negative_pairs(num, n, ptr(known.rowptr), ptr(known.col), seed, int(slot_base), md,
                                                 ptr(active), ptr(nxt), ptr(out), num, ptr(short), st),
                          "lpf_negative_pairs")
            launch(None)
            if unique and num:
                for _ in range(1, rounds):
                    launch(_losers(out, n).to(torch.uint8))
                out = torch.where(_losers(out, n)[None, :], torch.full_like(out, -1), out)
                short = (out[0] < 0).sum()
    if check:
        _raise_short(int(short), num, "pairs", "negative_pairs")
    return out


class UniformNegatives:
    """Fresh non-edges per training step: a callable ``(step, edges) -> int64 [2, B * num_negative]`` for
    ``train_epoch(negatives=...)`` / ``fit(negatives=...)``, B the batch's positives (``edges`` [2, B]).

    The draw of step ``step`` uses the seed ``mix64(seed + G (step + 1))`` (``step_seed``, computed on the host), so
    the steps differ and a run repeats under its seed.  ``train_epoch`` counts its steps from 0 in every epoch: a call
    whose ``step`` is not above the previous call's starts the next epoch, and epoch e > 0 replaces ``seed`` by
    ``step_seed(seed, 2^32 + e)`` (``epoch`` may also be set by hand).

    ``mode="pairs"``: ``negative_pairs(..., unique=False, check=False)``.  ``mode="tail"``: ``negative_rows`` with the
    positives' first endpoints as sources, each target paired with its source (the positive's head stays, the tail is
    replaced).  Nothing is read back, so a slot that found nothing cannot raise: it becomes the self pair of node 0
    (``"pairs"``) or of its source (``"tail"``), which keeps every id in range -- on a graph with free pairs to spare
    that is 2^16 rejected draws in a row away."""

    def __init__(self, source, *, seed, num_negative: int = 1, mode: str = "pairs", exclude=None,
                 test_set: bool = False):
        if mode not in ("pairs", "tail"):
            raise ValueError(f"mode must be 'pairs' or 'tail'; got {mode!r}")
        self.source, self.seed, self.mode, self.exclude, self.test_set = source, _check_seed(seed), mode, exclude, test_set
        self.num_negative = _check_count(num_negative, "num_negative", 1, MAX_K)
        self.epoch, self._last = 0, -1

    def seed_of(self, step: int) -> int:
        base = self.seed if self.epoch == 0 else step_seed(self.seed, (1 << 32) + self.epoch)
        return step_seed(base, step)

    def __call__(self, step: int, edges: torch.Tensor) -> torch.Tensor:
        step = int(step)
        if step <= self._last:
            self.epoch += 1
        self._last = step
        seed = self.seed_of(step)
        edges = sources.as_pairs(edges)
        B = edges.shape[1]
        if self.mode == "pairs":
            neg = negative_pairs(self.source, B * self.num_negative, seed=seed, test_set=self.test_set,
                                 exclude=self.exclude, unique=False, check=False)
            return neg.clamp_(min=0).to(edges.device)
        heads = edges[0]
        rows = negative_rows(self.source, heads, self.num_negative, seed=seed, test_set=self.test_set,
                             exclude=self.exclude, check=False)
        heads = heads.to(rows.device, dtype=torch.int64)[:, None].expand_as(rows)
        return torch.stack([heads, torch.where(rows >= 0, rows, heads)]).reshape(2, -1).to(edges.device)
