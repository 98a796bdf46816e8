"""Graph edits with an EXACT incremental refresh of the PPR matrix.

Once a recommended link is accepted, or an edge retracted, the graph has changed.  ``update_ppr`` / ``update_data`` /
``update_graph`` apply such an edit without the full producer run that ``data.build_data`` on the new edge list costs.

The fact this rests on: the push of source ``s`` (csrc/ppr_push.hip, csrc/host_ppr.cpp) stores EVERY node it popped in
row ``s`` (zero values included), reads a node's neighbour list and out-degree only when it pops it, and of a node that
merely receives residual only its degree (the queue test ``r >= alpha * eps * deg``).  With the key set

    K = endpoints(added edges) | endpoints(removed edges) | N_G(endpoints(removed edges))

a row of PPR(G) that holds no node of K is bit-identical in PPR(G'): by induction over pops the push on G' replays the
push on G.  No endpoint of a removed edge ever receives residual (none of its G-neighbours pops; its new neighbours are
keys and do not pop either); an endpoint that only gained edges receives the same residual in the same order, stayed
below ``alpha * eps * deg_G`` on G and faces a larger threshold on G'; every popped node has an unchanged CSR row and
neighbours of unchanged degree.  ``s`` is in its own row, so a source that is a key is always flagged.  It is therefore
enough to push the flagged sources again and splice their rows into the old matrix.

Preconditions: the old matrix came from this package's producers (``calc_ppr`` / ``calc_ppr_gpu``) with the SAME
``alpha`` and ``eps`` on exactly the old edge set, with no entry dropped, and the node count does not change.  ``verify=k``
is the cheap guard: it pushes ``k`` unflagged sources again and raises when a row differs.

Which part runs where.  Host: the edit of the edge keys and the key bitmap (numpy; a few thousand ids plus one pass over
the edge list when edges are removed), the adjacency CSRs of the new data dict (``graph.csr_from_coo`` / ``mask_csr``, the
same builders ``build_data`` uses).  Device (``device=``): the detection of the affected rows (``lpf_ppr_affected_rows``),
the push over the source list (``lpf_ppr_push_f64_sources``) and the splice (``lpf_ppr_splice_csr``).  Without a device
the host twin ``lpf_ppr_push_cpu_sources`` and numpy do the same three steps.
"""
from __future__ import annotations

import ctypes as C
import time

import numpy as np
import torch

from . import _lib, graph
from .graph import CSR, DeviceCSR
from .ppr import calc_ppr, calc_ppr_gpu
from .ops import raw_stream

# Flagged share of the sources above which the ordinary full producer runs instead (same result by definition: a speed
# knob).  Measured on the MI355X (tools/graph_update_timing.py, profiles/graph_update_timing.json, table in DESIGN 5.11):
# on the collab-like graph the incremental path is ahead up to a share of 0.89 (0.226 s against 0.232 s) and behind at
# 0.99 (0.239 against 0.233); on the ppa-like graph, where the host's work on the 42 M-entry edge list weighs as much
# as the push, the curves cross at 0.48 (0.476 against 0.473).  The smaller crossing is the default.
FULL_ABOVE_DEFAULT = 0.5


# ------------------------------------------------------------------------------------------------ edge keys
def _as_pairs(pairs, n: int, what: str) -> np.ndarray:
    """[2, K] int64 undirected pairs; ids outside [0, n) and self-loops raise ``ValueError``."""
    if pairs is None:
        return np.zeros((2, 0), np.int64)
    a = pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)
    if a.size == 0:
        return np.zeros((2, 0), np.int64)
    if a.ndim != 2 or a.shape[0] != 2:
        raise ValueError(f"{what}: expected [2, K] node ids, got shape {tuple(a.shape)}")
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{what}: node ids must be integers")
    a = a.astype(np.int64)
    if a.min() < 0 or a.max() >= n:
        raise ValueError(f"{what}: node ids outside [0, {n})")
    if np.any(a[0] == a[1]):
        raise ValueError(f"{what}: self-loops are not accepted")
    return a


def _both_directions(pairs: np.ndarray, n: int) -> np.ndarray:
    """Sorted distinct directed keys ``row * n + col`` of both directions of the pairs (``data.to_undirected``)."""
    return np.unique(np.concatenate([pairs[0] * n + pairs[1], pairs[1] * n + pairs[0]]))


def _edge_keys(edge_index, n: int) -> np.ndarray:
    """Sorted distinct keys of a directed edge list (the coalescing ``calc_ppr`` applies)."""
    ei = edge_index.detach().cpu().numpy() if isinstance(edge_index, torch.Tensor) else np.asarray(edge_index)
    ei = ei.astype(np.int64, copy=False).reshape(2, -1)
    if ei.size and (ei.min() < 0 or ei.max() >= n):
        raise ValueError(f"edge_index: node ids outside [0, {n})")
    key = ei[0] * np.int64(n) + ei[1]
    if key.size > 1 and not bool(np.all(key[1:] > key[:-1])):
        key = np.unique(key)
    return key


def _member(sorted_keys: np.ndarray, query: np.ndarray) -> np.ndarray:
    if sorted_keys.size == 0 or query.size == 0:
        return np.zeros(query.size, bool)
    pos = np.searchsorted(sorted_keys, query)
    pos[pos >= sorted_keys.size] = sorted_keys.size - 1
    return sorted_keys[pos] == query


def _apply(old: np.ndarray, gone: np.ndarray, came: np.ndarray) -> np.ndarray:
    """``(old - gone) | came`` for sorted distinct keys with ``gone`` inside and ``came`` outside ``old``: two copies of
    the list, no sort."""
    kept = np.delete(old, np.searchsorted(old, gone)) if gone.size else old
    return np.insert(kept, np.searchsorted(kept, came), came) if came.size else kept


def _edit_keys(old: np.ndarray, add: np.ndarray, remove: np.ndarray, n: int):
    """``(new, gone, came, noop)``: the sorted key set ``(old | add) - remove`` (both directions of every pair), the
    keys that went away and the keys that came, and the no-op counts."""
    addk, remk = _both_directions(add, n), _both_directions(remove, n)
    came = addk[~_member(old, addk) & ~_member(remk, addk)]
    gone = remk[_member(old, remk)]
    noop = {"n_add_noop": int(addk.size - came.size + 1) // 2, "n_remove_noop": int(remk.size - gone.size + 1) // 2}
    return _apply(old, gone, came), gone, came, noop


def _key_mask(old: np.ndarray, gone: np.ndarray, came: np.ndarray, n: int) -> np.ndarray:
    """bool [n]: endpoints of the keys that went or came, plus every old neighbour (either direction) of an endpoint of
    a key that went away."""
    mask = np.zeros(n, bool)
    for k in (gone, came):
        mask[k // n] = True
        mask[k % n] = True
    if gone.size:
        ends = np.zeros(n, bool)
        ends[gone // n] = True
        ends[gone % n] = True
        r = old // n
        c = old - r * n
        mask[c[ends[r]]] = True
        mask[r[ends[c]]] = True
    return mask


def _csr_from_keys(keys: np.ndarray, n: int):
    """(rowptr int64, col int32) of sorted distinct keys: what ``graph.csr_from_coo`` gives for the edge list."""
    r = keys // n
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=rowptr[1:])
    return rowptr, (keys - r * n).astype(np.int32)


def _keys_to_edge_index(keys: np.ndarray, n: int) -> np.ndarray:
    return np.stack([keys // n, keys % n]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ PPR containers
def _as_host_ppr(ppr) -> CSR:
    if isinstance(ppr, CSR):
        if ppr.val is None:
            raise ValueError("the PPR matrix needs values")
        return ppr
    if isinstance(ppr, DeviceCSR):
        return ppr.to_host()
    if isinstance(ppr, (tuple, list)) and len(ppr) == 3 and isinstance(ppr[0], torch.Tensor):
        rp, c, v = ppr
        return CSR(rp.cpu().numpy(), c.cpu().numpy(), v.cpu().numpy(), int(rp.numel()) - 1)
    row, col, val, n = graph.as_coo_numpy(ppr)
    if val is None:
        raise ValueError("the PPR matrix needs values")
    return graph.csr_from_coo(row, col, val, n)


def _on_device(ppr) -> bool:
    return isinstance(ppr, DeviceCSR) or (isinstance(ppr, (tuple, list)) and len(ppr) == 3 and
                                          isinstance(ppr[0], torch.Tensor) and ppr[0].is_cuda)


def _ppr_n(ppr) -> int:
    if isinstance(ppr, (CSR, DeviceCSR)):
        return int(ppr.n)
    if isinstance(ppr, (tuple, list)) and len(ppr) == 3 and isinstance(ppr[0], torch.Tensor):
        return int(ppr[0].numel()) - 1
    return int(graph.as_coo_numpy(ppr)[3])


def _as_device_ppr(ppr, dev) -> DeviceCSR:
    if isinstance(ppr, DeviceCSR) and ppr.rowptr.device == dev:
        return ppr
    if isinstance(ppr, (tuple, list)) and len(ppr) == 3 and isinstance(ppr[0], torch.Tensor):
        rp, c, v = (t.to(dev) for t in ppr)
        return DeviceCSR(rp, c, v, int(rp.numel()) - 1, None)
    return _as_host_ppr(ppr).to_device(dev)


# ------------------------------------------------------------------------------------------------ host path
def _affected_host(ppr: CSR, mask: np.ndarray) -> np.ndarray:
    hit = np.flatnonzero(mask[ppr.col])
    return np.unique(np.searchsorted(ppr.rowptr, hit, side="right") - 1).astype(np.int32)


def _push_sources_host(rowptr, col, n: int, sources: np.ndarray, alpha: float, eps: float, num_threads: int = 0):
    """(rowptr int64 [S + 1], col, val) of the rows of ``sources`` (ascending int32) on the graph (rowptr, col)."""
    lib = _lib.host()
    rowptr = np.ascontiguousarray(rowptr, np.int64)
    col = np.ascontiguousarray(col, np.int32)
    sources = np.ascontiguousarray(sources, np.int32)
    out_rp = np.zeros(sources.size + 1, np.int64)
    col_p, val_p = C.c_void_p(), C.c_void_p()
    rc = lib.lpf_ppr_push_cpu_sources(n, rowptr.ctypes.data, col.ctypes.data, float(alpha), float(eps), sources.size,
                                      sources.ctypes.data, out_rp.ctypes.data, C.byref(col_p), C.byref(val_p),
                                      int(num_threads))
    if rc != 0:
        raise _lib.LpfError(f"lpf_ppr_push_cpu_sources failed with code {rc}")
    nnz = int(out_rp[-1])
    try:
        c = np.ctypeslib.as_array(C.cast(col_p, C.POINTER(C.c_int32)), shape=(max(nnz, 1),))[:nnz].copy()
        v = np.ctypeslib.as_array(C.cast(val_p, C.POINTER(C.c_float)), shape=(max(nnz, 1),))[:nnz].copy()
    finally:
        lib.lpf_host_free(col_p)
        lib.lpf_host_free(val_p)
    return out_rp, c, v


def _splice_host(old: CSR, sources: np.ndarray, rp, c, v) -> CSR:
    n = old.n
    old_len = np.diff(old.rowptr)
    new_len = old_len.copy()
    new_len[sources] = np.diff(rp)
    flag = np.zeros(n, bool)
    flag[sources] = True
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(new_len, out=rowptr[1:])
    fresh = np.repeat(flag, new_len)            # entries of the new matrix that come from the re-pushed rows
    keep = ~np.repeat(flag, old_len)            # entries of the old matrix that stay (same order in both)
    col = np.empty(int(rowptr[-1]), np.int32)
    val = np.empty(int(rowptr[-1]), np.float32)
    col[fresh], val[fresh] = c, v
    col[~fresh], val[~fresh] = old.col[keep], old.val[keep]
    return CSR(rowptr, col, val, n)


def _verify(old: CSR, unflagged: np.ndarray, k: int, rowptr, col, alpha, eps, num_threads):
    """Push ``k`` randomly chosen unflagged sources on the new graph (host twin) and compare with their old rows."""
    if k <= 0 or unflagged.size == 0:
        return 0
    pick = np.sort(np.random.default_rng(0).choice(unflagged, size=min(int(k), unflagged.size), replace=False))
    rp, c, v = _push_sources_host(rowptr, col, old.n, pick.astype(np.int32), alpha, eps, num_threads)
    for i, s in enumerate(pick):
        a0, a1 = old.rowptr[s], old.rowptr[s + 1]
        if not (np.array_equal(old.col[a0:a1], c[rp[i]:rp[i + 1]]) and
                np.array_equal(old.val[a0:a1].view(np.uint32), v[rp[i]:rp[i + 1]].view(np.uint32))):
            raise _lib.LpfError(f"update_ppr(verify=): row {int(s)} meets no key of the edit, yet its fresh push differs "
                                "from the stored row -- the matrix was not produced by this package with the same "
                                "alpha / eps on exactly the old edge set")
    return int(pick.size)


# ------------------------------------------------------------------------------------------------ device path
def affected_rows_device(ppr: DeviceCSR, mask: np.ndarray, bitmap_mode: int = -1):
    """``lpf_ppr_affected_rows``: (flag int32 [n], list int32 [n] -- ascending ids in its first ``count`` entries --,
    count int64 [1]) on the device of ``ppr``; ``mask``: bool [n] key nodes (host).  Nothing is read back."""
    dev, n = ppr.rowptr.device, ppr.n
    lib = _lib.hip()
    words = np.zeros(((n + 31) // 32) * 4, np.uint8)
    packed = np.packbits(np.asarray(mask, bool), bitorder="little")
    words[:packed.size] = packed
    bitmap = torch.from_numpy(words.view(np.int32)).to(dev) if n else torch.zeros(1, dtype=torch.int32, device=dev)
    flag = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    lst = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(lib.lpf_ppr_affected_workspace_bytes(n)), 256), dtype=torch.uint8, device=dev)
    _lib.check(lib.lpf_ppr_affected_rows(n, _lib.ptr(ppr.rowptr), _lib.ptr(ppr.col), _lib.ptr(bitmap), int(bitmap_mode),
                                         _lib.ptr(flag), _lib.ptr(lst), _lib.ptr(count), _lib.ptr(ws), ws.numel(),
                                         raw_stream(dev)), "lpf_ppr_affected_rows")
    return flag[:n], lst, count


def push_sources_device(rowptr: torch.Tensor, col: torch.Tensor, n: int, sources: torch.Tensor, alpha: float,
                        eps: float, *, n_waves: int = 0, state_budget_bytes: int = 8 << 30, pool_capacity: int = 0):
    """``lpf_ppr_push_f64_sources`` for the ascending int32 device list ``sources``: (row_off int64 [S], row_len int32
    [S], pool_col, pool_val, nnz).  The rows lie unsorted in the pool, as ``lpf_ppr_push_f64`` leaves them.
    ``n_waves`` (0 = min(list length, what ``state_budget_bytes`` allows, 8192)): the dense state cleared per call is
    32 n bytes per wavefront, so a short list must not pay for thousands of them."""
    dev, lib = rowptr.device, _lib.hip()
    S = int(sources.numel())
    if n_waves <= 0:
        per_wave = max(1, lib.lpf_ppr_push_workspace_bytes(n, 4, float(alpha), float(eps)) // 4)
        n_waves = int(min(8192, max(4, state_budget_bytes // per_wave), 4 * ((S + 3) // 4)))
    n_waves = max(4, n_waves - n_waves % 4)
    ws_bytes = lib.lpf_ppr_push_workspace_bytes(n, n_waves, float(alpha), float(eps))
    if ws_bytes <= 0:
        raise _lib.LpfError("lpf_ppr_push_workspace_bytes: invalid arguments")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    row_off = torch.empty(max(S, 1), dtype=torch.int64, device=dev)
    row_len = torch.empty(max(S, 1), dtype=torch.int32, device=dev)
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    cap = int(pool_capacity) if pool_capacity > 0 else max(1 << 16, 384 * S)
    while True:
        pool_col = torch.empty(cap, dtype=torch.int32, device=dev)
        pool_val = torch.empty(cap, dtype=torch.float32, device=dev)
        _lib.check(lib.lpf_ppr_push_f64_sources(n, _lib.ptr(rowptr), _lib.ptr(col), S, _lib.ptr(sources), float(alpha),
                                                float(eps), n_waves, _lib.ptr(ws), ws_bytes, _lib.ptr(pool_col),
                                                _lib.ptr(pool_val), cap, _lib.ptr(row_off), _lib.ptr(row_len),
                                                _lib.ptr(counters), raw_stream(dev)), "lpf_ppr_push_f64_sources")
        _, nnz, bad, _ = (int(x) for x in counters.tolist())
        if bad:
            raise _lib.LpfError(f"lpf_ppr_push_f64_sources: {bad} rows exceeded the 1/(alpha*eps) list bound")
        if nnz <= cap:
            break
        cap = nnz  # deterministic: the second run needs exactly this many slots
    return row_off[:S], row_len[:S], pool_col, pool_val, nnz


def splice_device(old: DeviceCSR, sources: torch.Tensor, row_off, row_len, pool_col, pool_val, nnz_pool: int,
                  out_nnz: int):
    """``lpf_ppr_splice_csr``: the device triple (rowptr int64, col int32, val fp32) of the refreshed matrix."""
    dev, n, lib = old.rowptr.device, old.n, _lib.hip()
    S = int(sources.numel())
    ws_bytes = lib.lpf_ppr_splice_workspace_bytes(n, S, nnz_pool)
    if ws_bytes <= 0:
        raise _lib.LpfError("lpf_ppr_splice_workspace_bytes: invalid arguments")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out_rowptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
    out_col = torch.empty(max(out_nnz, 1), dtype=torch.int32, device=dev)
    out_val = torch.empty(max(out_nnz, 1), dtype=torch.float32, device=dev)
    _lib.check(lib.lpf_ppr_splice_csr(n, _lib.ptr(old.rowptr), _lib.ptr(old.col), _lib.ptr(old.val), S,
                                      _lib.ptr(sources), _lib.ptr(row_off), _lib.ptr(row_len), _lib.ptr(pool_col),
                                      _lib.ptr(pool_val), nnz_pool, _lib.ptr(out_rowptr), _lib.ptr(out_col),
                                      _lib.ptr(out_val), out_nnz, _lib.ptr(ws), ws_bytes, raw_stream(dev)),
               "lpf_ppr_splice_csr")
    return out_rowptr, out_col[:out_nnz], out_val[:out_nnz]


# ------------------------------------------------------------------------------------------------ the refresh
def _refresh(ppr, old_keys: np.ndarray, new_keys: np.ndarray, gone: np.ndarray, came: np.ndarray, n: int, *, alpha: float, eps: float, device,
             full_above: float, verify: int, num_threads: int, n_waves: int, state_budget_bytes: int,
             bitmap_mode: int, to_host, stats: dict):
    """PPR(new_keys) from ``ppr`` = PPR(old_keys), new_keys = (old_keys - gone) | came; fills ``stats``."""
    dev = None if device is None else torch.device(device)
    if dev is not None and dev.type != "cuda":
        raise _lib.LpfError("update_ppr(device=) needs an MI355X device; leave device=None for the host path")
    if to_host is None:
        to_host = not _on_device(ppr)

    def mark(name, t0):
        if dev is not None:
            torch.cuda.synchronize(dev)
        stats[name] = stats.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    t_all = t = time.perf_counter()
    mask = _key_mask(old_keys, gone, came, n)
    stats["n_keys"] = int(mask.sum())
    t = mark("keys_s", t)

    def finish(result, path, n_aff):
        stats.update(n_affected=int(n_aff), fraction=(n_aff / n if n else 0.0), path=path,
                     total_s=time.perf_counter() - t_all)
        return result

    if dev is None:
        old = _as_host_ppr(ppr)
        if old.n != n:
            raise ValueError(f"the PPR matrix has {old.n} rows, the graph {n} nodes")
        sources = _affected_host(old, mask)
        t = mark("flag_s", t)
        rowptr, col = _csr_from_keys(new_keys, n)
        if sources.size > full_above * n:
            out = calc_ppr(_keys_to_edge_index(new_keys, n), n, alpha, eps, num_threads)
            mark("full_s", t)
            return finish(out, "full", sources.size)
        if sources.size == 0:
            out = old
        else:
            rp, c, v = _push_sources_host(rowptr, col, n, sources, alpha, eps, num_threads)
            t = mark("push_s", t)
            out = _splice_host(old, sources, rp, c, v)
            t = mark("splice_s", t)
        if verify:
            unflagged = np.setdiff1d(np.arange(n, dtype=np.int64), sources.astype(np.int64), assume_unique=True)
            stats["n_verified"] = _verify(old, unflagged, verify, rowptr, col, alpha, eps, num_threads)
            mark("verify_s", t)
        return finish(out, "incremental", sources.size)

    with torch.cuda.device(dev):
        old_d = _as_device_ppr(ppr, dev)
        if old_d.n != n:
            raise ValueError(f"the PPR matrix has {old_d.n} rows, the graph {n} nodes")
        t = mark("upload_s", t)
        flag, lst, count = affected_rows_device(old_d, mask, bitmap_mode)
        n_aff = int(count.item())
        t = mark("flag_s", t)
        if n_aff > full_above * n:
            tm = {}
            out = calc_ppr_gpu(_keys_to_edge_index(new_keys, n), n, alpha, eps, device=dev, n_waves=n_waves,
                               state_budget_bytes=state_budget_bytes, to_host=to_host, timings=tm)
            stats["full_phases"] = tm
            mark("full_s", t)
            return finish(out, "full", n_aff)
        rowptr, col = _csr_from_keys(new_keys, n)
        if n_aff == 0:
            triple = (old_d.rowptr, old_d.col, old_d.val)
        else:
            sources = lst[:n_aff]
            old_len = old_d.rowptr[1:] - old_d.rowptr[:-1]
            old_aff = int(old_len[sources.long()].sum().item())
            g_rowptr, g_col = torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev)
            t = mark("upload_s", t)
            row_off, row_len, pool_col, pool_val, nnz_pool = push_sources_device(
                g_rowptr, g_col, n, sources, alpha, eps, n_waves=n_waves, state_budget_bytes=state_budget_bytes,
                pool_capacity=int(old_aff * 1.25) + (1 << 16))
            t = mark("push_s", t)
            triple = splice_device(old_d, sources, row_off, row_len, pool_col, pool_val, nnz_pool,
                                   old_d.nnz - old_aff + nnz_pool)
            t = mark("splice_s", t)
        if verify:
            old_h = old_d.to_host()
            unflagged = np.flatnonzero(flag.cpu().numpy() == 0)
            stats["n_verified"] = _verify(old_h, unflagged, verify, rowptr, col, alpha, eps, num_threads)
            t = mark("verify_s", t)
        out = CSR(triple[0].cpu().numpy(), triple[1].cpu().numpy(), triple[2].cpu().numpy(), n) if to_host else triple
        if to_host:
            mark("download_s", t)
        return finish(out, "incremental", n_aff)


# ------------------------------------------------------------------------------------------------ public entry points
def ppr_affected_sources(ppr, adj, add=None, remove=None):
    """``(sources, stats)``: the ascending int32 ids of the sources whose row of ``ppr`` must be pushed again when the
    undirected pairs ``add`` / ``remove`` ([2, K]) are applied to the graph ``adj`` (a ``graph.CSR``, a [2, E] directed
    edge list, or any container ``graph.as_coo_numpy`` reads), and ``stats`` = ``n_keys``, ``n_affected``, ``fraction``,
    ``n_add_noop``, ``n_remove_noop``.  A device-resident ``ppr`` (``graph.DeviceCSR`` or the triple of
    ``calc_ppr_gpu(to_host=False)``) is searched by ``lpf_ppr_affected_rows`` and ``sources`` is a device tensor."""
    if isinstance(adj, np.ndarray) or (isinstance(adj, torch.Tensor) and adj.layout == torch.strided):
        n = _ppr_n(ppr)
        old = _edge_keys(adj, n)
    else:
        row, col, _, n = graph.as_coo_numpy(adj)
        old = _edge_keys(np.stack([row, col]), n)
    _, gone, came, stats = _edit_keys(old, _as_pairs(add, n, "add"), _as_pairs(remove, n, "remove"), n)
    mask = _key_mask(old, gone, came, n)
    if _on_device(ppr):
        dev = ppr.rowptr.device if isinstance(ppr, DeviceCSR) else ppr[0].device
        with torch.cuda.device(dev):
            _, lst, count = affected_rows_device(_as_device_ppr(ppr, dev), mask)
            sources = lst[:int(count.item())]
    else:
        sources = _affected_host(_as_host_ppr(ppr), mask)
    k = int(sources.numel() if isinstance(sources, torch.Tensor) else sources.size)
    stats.update(n_keys=int(mask.sum()), n_affected=k, fraction=k / n if n else 0.0)
    return sources, stats


def update_ppr(ppr, edge_index, add=None, remove=None, *, alpha: float = 0.15, eps: float = 5e-5, device=None,
               full_above: float = FULL_ABOVE_DEFAULT, verify: int = 0, num_threads: int = 0, n_waves: int = 0,
               state_budget_bytes: int = 8 << 30, bitmap_mode: int = -1, to_host=None):
    """``(new_ppr, stats)``: the PPR matrix of the edited graph, bit-identical to ``calc_ppr`` / ``calc_ppr_gpu`` on the
    edited edge list, from ``ppr`` = the matrix of ``edge_index`` (see the module docstring for the preconditions).

    ``edge_index``: the old [2, E] directed edge list (both directions of every undirected edge; coalesced first, as the
    producers do).  ``add`` / ``remove``: [2, K] undirected pairs -- both directions are edited and the result is
    coalesced, as ``data.to_undirected`` does; a pair in both lists ends up removed.  Additions that already exist and
    removals that do not are no-ops: counted (``stats["n_add_noop"]``, ``["n_remove_noop"]``), no keys.  Self-loops and
    ids outside [0, N) raise ``ValueError``.

    ``device=None``: host path (``lpf_ppr_push_cpu_sources`` + numpy), result a ``graph.CSR``.  A device: the three HIP
    entry points; the result is the device triple ``(rowptr int64, col int32, val fp32)`` when ``ppr`` was
    device-resident, a host ``CSR`` when it was a host container (``to_host=`` overrides).
    ``full_above``: flagged share of the sources above which the ordinary full producer runs (identical result by
    definition: a speed knob, not a correctness one).  ``verify=k``: push ``k`` randomly chosen UNFLAGGED sources again
    (host twin) and raise ``LpfError`` if a row differs -- the cheap guard for a matrix that did not meet the
    preconditions.  ``stats``: ``n_keys``, ``n_affected``, ``fraction``, ``path`` ("incremental" / "full"), the no-op
    counts and the seconds per phase (``keys_s``, ``flag_s``, ``push_s``, ``splice_s``, ``full_s``, ..., ``total_s``;
    synchronising, like ``calc_ppr_gpu(timings=)``)."""
    n = _ppr_n(ppr)
    t0 = time.perf_counter()
    old = _edge_keys(edge_index, n)
    new, gone, came, stats = _edit_keys(old, _as_pairs(add, n, "add"), _as_pairs(remove, n, "remove"), n)
    stats["edit_s"] = time.perf_counter() - t0
    out = _refresh(ppr, old, new, gone, came, n, alpha=alpha, eps=eps, device=device, full_above=full_above, verify=verify,
                   num_threads=num_threads, n_waves=n_waves, state_budget_bytes=state_budget_bytes,
                   bitmap_mode=bitmap_mode, to_host=to_host, stats=stats)
    return out, stats


def _sorted_coo(obj):
    """(keys ascending, values aligned or None, n) of a graph container of the data dict."""
    row, col, val, n = graph.as_coo_numpy(obj)
    key = np.asarray(row, np.int64) * n + np.asarray(col, np.int64)
    if key.size > 1 and not bool(np.all(key[1:] > key[:-1])):
        order = np.argsort(key, kind="stable")
        key, val = key[order], (None if val is None else np.asarray(val)[order])
        if np.any(key[1:] == key[:-1]):
            raise ValueError("update_data: the adjacency holds duplicate entries; coalesce it first")
    return key, (None if val is None else np.asarray(val, np.float32)), n


def update_data(data: dict, add=None, remove=None, *, alpha: float = 0.15, eps: float = 5e-5, device=None,
                edge_weight: float = 1.0, full_above: float = FULL_ABOVE_DEFAULT, verify: int = 0,
                num_threads: int = 0, stats: dict = None) -> dict:
    """A NEW dict in ``data.build_data``'s schema for the edited graph: ``adj_t``, ``adj_mask``, ``full_adj_t``,
    ``full_adj_mask``, ``ppr``, ``ppr_test`` are new ``graph.CSR`` containers equal, array by array, to
    ``build_data(edited edge list, ...)``; every other entry (``x``, splits) is shared; ``data`` and its arrays are left
    untouched.  Where ``full_adj_t is adj_t`` / ``ppr_test is ppr`` (no validation edges) the identities are preserved
    and one refresh serves both.  The edit applies to the TRAINING edges; the validation edges of the full graph stay
    (they are recovered as the entries where ``full_adj_t`` exceeds ``adj_t`` by their weight 1).  Added edges get
    ``edge_weight``.  ``alpha`` / ``eps`` must be the ones ``data["ppr"]`` was built with.  ``stats`` (optional dict)
    receives ``update_ppr``'s statistics under ``"ppr"`` and ``"ppr_test"``."""
    stats = {} if stats is None else stats
    keys, w, n = _sorted_coo(data["adj_t"])
    w = np.ones(keys.size, np.float32) if w is None else w
    addp, remp = _as_pairs(add, n, "add"), _as_pairs(remove, n, "remove")
    new_keys, gone, came, noop = _edit_keys(keys, addp, remp, n)
    stats.update(noop)
    w_new = np.full(new_keys.size, np.float32(edge_weight), np.float32)
    pos = np.searchsorted(keys, new_keys)
    pos[pos >= max(keys.size, 1)] = max(keys.size - 1, 0)
    was = keys[pos] == new_keys if keys.size else np.zeros(new_keys.size, bool)
    w_new[was] = w[pos[was]]
    ei = _keys_to_edge_index(new_keys, n)
    out = dict(data)
    out["adj_t"] = graph.csr_from_coo(ei[0], ei[1], w_new, n)
    out["adj_mask"] = graph.mask_csr(ei, n, symmetric=True)
    kw = dict(alpha=alpha, eps=eps, device=device, full_above=full_above, verify=verify, num_threads=num_threads,
              n_waves=0, state_budget_bytes=8 << 30, bitmap_mode=-1, to_host=True)
    stats["ppr"] = {}
    out["ppr"] = _refresh(data["ppr"], keys, new_keys, gone, came, n, stats=stats["ppr"], **kw)
    shared = data.get("full_adj_t") is data["adj_t"] or "full_adj_t" not in data
    if shared:
        for k, src in (("full_adj_t", "adj_t"), ("full_adj_mask", "adj_mask")):
            if k in data:
                out[k] = out[src]
    else:
        fkeys, fw, _ = _sorted_coo(data["full_adj_t"])
        fw = np.ones(fkeys.size, np.float32) if fw is None else fw
        base = np.zeros(fkeys.size, np.float32)
        hit = _member(keys, fkeys)
        base[hit] = w[np.searchsorted(keys, fkeys[hit])]
        vkeys = fkeys[(fw - base) > 0.5]                     # the validation edges (weight 1 each, coalesced)
        full = np.concatenate([ei, _keys_to_edge_index(vkeys, n)], axis=1)
        out["full_adj_t"] = graph.csr_from_coo(full[0], full[1],
                                               np.concatenate([w_new, np.ones(vkeys.size, np.float32)]), n)
        out["full_adj_mask"] = graph.mask_csr(full, n, symmetric=False)
    if "ppr_test" in data:
        if data["ppr_test"] is data["ppr"]:
            out["ppr_test"] = out["ppr"]
        else:
            if shared:
                f_old, f_new, f_gone, f_came = keys, new_keys, gone, came
            else:   # (a removed training edge that is a validation edge too stays in the full graph, and so on)
                f_gone, f_came = gone[~_member(vkeys, gone)], came[~_member(fkeys, came)]
                f_old, f_new = fkeys, _apply(fkeys, f_gone, f_came)
            stats["ppr_test"] = {}
            out["ppr_test"] = _refresh(data["ppr_test"], f_old, f_new, f_gone, f_came, n, stats=stats["ppr_test"],
                                       **kw)
    return out


def update_graph(model, add=None, remove=None, *, alpha: float = 0.15, eps: float = 5e-5, device=None,
                 edge_weight: float = 1.0, full_above: float = FULL_ABOVE_DEFAULT, verify: int = 0,
                 rebuild: bool = True) -> dict:
    """Apply the edit to a live ``LinkTransformer``: ``update_data`` on ``model.data``, then the new dict is swapped in
    and every piece of state derived from the old graph objects is dropped -- the resident CSR uploads, walk indexes and
    T0 indexes (``_graphs``), the override slots, the mask-delta cache, the encoder output and the node tables keyed on
    it, the entry sample with the kernel choices and pattern tables made from it, and the per-stream workspaces (their
    calibration came from batches of the old graph).  Nothing is keyed on an address here: the old objects are simply
    released, and the per-graph caches of ``heuristics`` / ``recommend`` / ``hard_negatives`` hold weak references that
    die with them.  A ``PlannedScorer`` / ``GraphedScorer`` recorded before the update holds pointers into the old
    graph and an encoder output of the old graph: its next call RAISES (``model._graph_epoch`` moved); build a new
    scorer from ``model.propagate()``.

    ``device`` (default: the model's, when it is a GPU) runs the PPR refresh on the device.  ``rebuild`` (default): the
    uploads, the walk index, ``gcn_norm`` and -- in eval mode -- one encoder pass are redone now, in full (they are
    whole-graph operations), and timed separately: ``stats["upload_s"]``, ``["walk_index_s"]``, ``["gcn_norm_s"]``,
    ``["encoder_s"]``; otherwise they happen lazily on the next call.  Returns ``stats`` (``update_data``'s, plus
    ``data_s`` and those)."""
    stats = {}
    if device is None and model.device.type == "cuda":
        device = model.device
    t = time.perf_counter()
    new = update_data(model.data, add, remove, alpha=alpha, eps=eps, device=device, edge_weight=edge_weight,
                      full_above=full_above, verify=verify, stats=stats)
    stats["data_s"] = time.perf_counter() - t
    model.data = new
    model._drop_graph_state()
    if rebuild and model.device.type == "cuda":
        dev = model.device

        def mark(name, t0):
            torch.cuda.synchronize(dev)
            stats[name] = time.perf_counter() - t0
            return time.perf_counter()

        with torch.cuda.device(dev):
            t = time.perf_counter()
            seen = []
            for ts in (False, True):
                for kind in ("mask", "ppr"):
                    obj = model._data_obj(kind, ts)
                    if not any(obj is o for o in seen):
                        seen.append(obj)
                        model._device_graph(kind, obj)
            t = mark("upload_s", t)
            if model.use_select_index:
                model._select_graphs(False, None)
            t = mark("walk_index_s", t)
            model._device_graph("prop", model._data_obj("adj", False))
            t = mark("gcn_norm_s", t)
            if not model.training and model._shard[1] == 1:
                model._propagate_reusing(None, False)
                mark("encoder_s", t)
    return stats
