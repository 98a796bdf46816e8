"""Bootstrap intervals and paired tests for the ranking metrics, resampled on the device.

Every metric of ``evaluate.link_metrics`` except AP is a sum over positives of a per-positive value derived from the two
counts ``(ge, gt)``, so a bootstrap replicate is a sum of P gathered table rows, not a re-ranking:

    bootstrap_sums(int_cols, float_cols, replicates, seed)      column sums of ``replicates`` resamples of the rows
    bootstrap_metrics(pos, neg, ...)                            value, standard error and percentile interval per metric
    compare_metrics(pos_a, neg_a, pos_b, neg_b, ...)            paired difference b - a of two systems, with a p-value
    bootstrap_by_bin(pos, neg, values, bins, ...)               ``bootstrap_metrics`` per bin of ``metrics_by_bin``
    bootstrap_sums_reference / bootstrap_indices                the numpy restatement, integer for integer

The draw is the negatives' (``negatives.draw_key`` / ``draw_u`` / ``draw_node``; csrc/draw_common.h on the device): row
``idx(b, j) = (u * P) >> 64`` with ``u = mix64(mix64(seed + G (b + 1)) + G (j + 1))`` is draw j of replicate b.  Replicate
b is a pure function of (seed, b, tables): not of how the replicates are chunked (``first``), of ``n_groups`` or of
timing.  Integer sums are exact and equal on the device and in the restatement; fp64 sums are added in the one order
csrc/bootstrap.hip writes down, and differ from the restatement's (numpy's pairwise sum) by at most
``P 2^-52 sum_j |x_j|`` -- twice the worst case of summing P terms in any order.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, evaluate, negatives, ops
from ._lib import check as _check_rc, ptr

MAX_COLS = _lib.CONST["LPF_BOOTSTRAP_MAX_COLS"]
SEGMENT = _lib.CONST["LPF_BOOTSTRAP_SEGMENT"]
MAX_P = (1 << 31) - 1
_TWIN_DRAWS = 1 << 22                 # draws the restatement holds at once
_WORKSPACE_BYTES = 64 << 20           # the device path cuts the replicates so that the partial sums stay below this


# ------------------------------------------------------------------------------------------------------ arguments
def _check_replicates(replicates, first):
    b = negatives._check_count(replicates, "replicates", 1, (1 << 31) - 1)
    f = negatives._check_count(first, "first", 0, (1 << 62))
    return b, f


def _check_p(p: int) -> int:
    if not 1 <= int(p) <= MAX_P:
        raise ValueError(f"the table must have between 1 and 2^31 - 1 rows; got {p}")
    return int(p)


def _table_shape(cols, what: str):
    """(P, C) of a [P] or [P, C] table, from its shape alone."""
    shape = tuple(cols.shape)
    if len(shape) == 1:
        return shape[0], 1
    if len(shape) != 2:
        raise ValueError(f"{what} must be [P] or [P, C]; got shape {shape}")
    return shape[0], shape[1]


def _shapes(int_cols, float_cols):
    """(P, Ci, Cf) after the checks that need no data: nothing has been allocated or copied when this raises."""
    if int_cols is None and float_cols is None:
        raise ValueError("bootstrap_sums needs int_cols, float_cols or both")
    p = ci = cf = None
    if int_cols is not None:
        p, ci = _table_shape(int_cols, "int_cols")
    if float_cols is not None:
        pf, cf = _table_shape(float_cols, "float_cols")
        if p is not None and pf != p:
            raise ValueError(f"int_cols has {p} rows, float_cols {pf}")
        p = pf
    ci, cf = ci or 0, cf or 0
    _check_p(p)
    if ci > MAX_COLS or cf > MAX_COLS or ci + cf < 1:
        raise ValueError(f"at most {MAX_COLS} integer and {MAX_COLS} float columns, and at least one; got {ci} and {cf}")
    return p, ci, cf


# ---------------------------------------------------------------------------------------------- the restatement
def bootstrap_indices(p: int, replicates: int = 1, seed: int = 0, *, first: int = 0) -> np.ndarray:
    """int64 [replicates, p]: row r holds ``idx(first + r, j)`` for j = 0 .. p - 1 -- the rows replicate ``first + r``
    sums.  The whole matrix: for tests and small tables."""
    p = _check_p(p)
    b, first = _check_replicates(replicates, first)
    seed = negatives._check_seed(seed)
    key = negatives.draw_key(seed, np.arange(first, first + b, dtype=np.uint64))
    return negatives.draw_node(negatives.draw_u(key[:, None], np.arange(p, dtype=np.uint64)[None, :]), p)


def bootstrap_sums_reference(int_cols=None, float_cols=None, replicates: int = 1000, seed: int = 0, *, first: int = 0):
    """The numpy restatement of ``lpf_bootstrap_sums``: ``(int64 [B, Ci], float64 [B, Cf])`` for numpy arrays.  It walks
    the replicates (and, for long tables, the draws) in chunks of ``2^22`` draws, so the [B, P] index matrix never
    exists.  Integer sums equal the kernel's; float sums are numpy's pairwise sums of each chunk, chunks in order."""
    p, ci, cf = _shapes(int_cols, float_cols)
    b, first = _check_replicates(replicates, first)
    seed = negatives._check_seed(seed)
    icols = None if int_cols is None else np.ascontiguousarray(np.asarray(int_cols, dtype=np.int64).reshape(p, ci))
    fcols = None if float_cols is None else np.ascontiguousarray(np.asarray(float_cols, dtype=np.float64).reshape(p, cf))
    isum = np.zeros((b, ci), dtype=np.int64)
    fsum = np.zeros((b, cf), dtype=np.float64)
    jstep = min(p, _TWIN_DRAWS)
    bstep = max(1, _TWIN_DRAWS // jstep)
    for r0 in range(0, b, bstep):
        r1 = min(b, r0 + bstep)
        key = negatives.draw_key(seed, np.arange(first + r0, first + r1, dtype=np.uint64))[:, None]
        for j0 in range(0, p, jstep):
            j = np.arange(j0, min(p, j0 + jstep), dtype=np.uint64)[None, :]
            idx = negatives.draw_node(negatives.draw_u(key, j), p)
            if ci:
                isum[r0:r1] += icols[idx].sum(axis=1)
            if cf:
                fsum[r0:r1] += fcols[idx].sum(axis=1)
    return isum, fsum


# ------------------------------------------------------------------------------------------------ the device path
def _sums_device(icols, fcols, p, ci, cf, b, first, seed, n_groups, dev):
    isum = torch.empty(b, ci, dtype=torch.int64, device=dev)
    fsum = torch.empty(b, cf, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        hip = _lib.hip()
        per_rep = int(hip.lpf_bootstrap_workspace_bytes(p, 1, ci, cf, n_groups))
        if per_rep < 0:
            raise ValueError(f"lpf_bootstrap_sums takes 0 <= n_groups <= 65535; got {n_groups}")
        step = b if per_rep == 0 else max(1, min(b, _WORKSPACE_BYTES // per_rep))
        ws = torch.empty(step * per_rep, dtype=torch.uint8, device=dev) if per_rep else None
        stream = ops.raw_stream(dev)
        for r0 in range(0, b, step):                 # replicate b is a pure function of (seed, b): any cut gives the same
            n = min(step, b - r0)
            _check_rc(hip.lpf_bootstrap_sums(p, n, first + r0, seed, ptr(icols), ci, ptr(fcols), cf,
                                             ptr(isum[r0:]) if ci else None, ptr(fsum[r0:]) if cf else None, n_groups,
                                             ptr(ws), n * per_rep, stream), "lpf_bootstrap_sums")
    return isum, fsum


def bootstrap_sums(int_cols=None, float_cols=None, replicates: int = 1000, seed: int = 0, *, first: int = 0,
                   n_groups: int = 0):
    """Column sums of ``replicates`` bootstrap resamples of the rows of a table: ``(int64 [B, Ci], float64 [B, Cf])``
    with row r = the sums over the P rows ``idx(first + r, j)``, j < P, of ``int_cols`` ([P] or [P, Ci], any integer or
    bool dtype, |value| <= 2^32) and ``float_cols`` ([P] or [P, Cf]); at most 8 columns of each kind.

    Tensors on a GPU go through ``lpf_bootstrap_sums`` on the current stream; nothing is read back.  CPU tensors and
    numpy arrays go through ``bootstrap_sums_reference`` (numpy arrays in, numpy arrays out).  ``first``: the index of
    the first replicate -- replicates [0, 64) in one call equal [0, 20) and [20, 64) in two, bit for bit.  ``n_groups``:
    the number of workgroups (0: eight per CU); the result does not depend on it."""
    p, ci, cf = _shapes(int_cols, float_cols)
    b, first = _check_replicates(replicates, first)
    seed = negatives._check_seed(seed)
    n_groups = negatives._check_count(n_groups, "n_groups", 0, 65535)
    tensors = [t for t in (int_cols, float_cols) if isinstance(t, torch.Tensor)]
    dev = tensors[0].device if tensors else None
    if dev is None or dev.type != "cuda":
        as_np = lambda t: None if t is None else (t.detach().numpy() if isinstance(t, torch.Tensor) else np.asarray(t))
        isum, fsum = bootstrap_sums_reference(as_np(int_cols), as_np(float_cols), b, seed, first=first)
        return (torch.from_numpy(isum), torch.from_numpy(fsum)) if tensors else (isum, fsum)
    icols = fcols = None
    if int_cols is not None:
        icols = torch.as_tensor(int_cols, device=dev).to(torch.int64).reshape(p, ci).contiguous()
    if float_cols is not None:
        fcols = torch.as_tensor(float_cols, device=dev).to(torch.float64).reshape(p, cf).contiguous()
    return _sums_device(icols, fcols, p, ci, cf, b, first, seed, n_groups, dev)


def _sums_wide(icols: list, fcols: list, b: int, seed: int):
    """``bootstrap_sums`` of any number of [P] columns: groups of at most 8, every group under the same seed -- the same
    draws.  Returns (int64 [B, len(icols)], float64 [B, len(fcols)]) on the columns' device."""
    dev = (icols + fcols)[0].device
    iparts, fparts = [], []
    for lo in range(0, max(len(icols), len(fcols)), MAX_COLS):
        ic, fc = icols[lo:lo + MAX_COLS], fcols[lo:lo + MAX_COLS]
        i, f = bootstrap_sums(torch.stack(ic, dim=1) if ic else None, torch.stack(fc, dim=1) if fc else None, b, seed)
        iparts.append(i)
        fparts.append(f)
    cat = lambda parts, dt: torch.cat(parts, dim=1) if parts else torch.empty(b, 0, dtype=dt, device=dev)
    return cat(iparts, torch.int64), cat(fparts, torch.float64)


# ------------------------------------------------------------------------------------------------------- metrics
class _Columns:
    """The per-positive columns of one system: what ``link_metrics`` sums, before the sum."""

    def __init__(self, pos, neg, ks, mrr, auc):
        pos, rows, sn = evaluate._prepare(pos, neg)
        self.p = pos.numel()
        if self.p < 1:
            raise ValueError("a bootstrap needs at least one positive")
        _check_p(self.p)
        self.per_row = rows is not None
        if auc is None:
            auc = not self.per_row
        if auc and self.per_row:
            raise ValueError("AUC over [P, K] negatives is not bootstrapped: the flattened negative pool would have to "
                             "be resampled with the positives")
        self.m = rows.shape[1] if self.per_row else sn.numel
        self.dev = pos.device
        ge, gt, _ = evaluate._counts_rows(pos, rows) if self.per_row else evaluate._counts_shared(pos, sn)
        both = ge.to(torch.int64) + gt
        self.names, self.icols, self.fcols, self.fixed = [], [], [], {}
        for k in ks:
            name = f"Hits@{k}"
            if not self.per_row and self.m < k:
                self.fixed[name] = 1.0              # hits_at_k: fewer than K negatives
            else:
                # rank <= K  <=>  0.5 (ge + gt) + 1 <= K; one shared set: pos > K-th largest negative  <=>  ge < K
                self.icols.append(((both <= 2 * k - 2) if self.per_row else (ge < k)).to(torch.int64))
            self.names.append(name)
        if mrr:
            self.names.append("MRR")
            self.fcols.append(2.0 / (both + 2).to(torch.float64))       # 1 / rank, correctly rounded as link_metrics'
        if auc:
            self.names.append("AUC")
            self.icols.append(2 * self.m - both)    # twice the AUC numerator's term, an exact integer
        # the point estimates are link_metrics' own (AP left out: it is not bootstrapped)
        self.value = evaluate._link_metrics(pos, rows, sn, ks, mrr, False, torch.float64)
        if auc:
            self.value["AUC"] = (int(self.icols[-1].sum()) / (2 * self.p * self.m)) if self.m else float("nan")

    def replicates(self, isum, fsum, count):
        """{name: float64 [B]} from this system's column sums; ``count`` float64 [B] or a float: positives per replicate."""
        out, i, f = {}, 0, 0
        for name in self.names:
            if name in self.fixed:
                out[name] = torch.full((isum.shape[0],), self.fixed[name], dtype=torch.float64, device=isum.device)
            elif name == "MRR":
                out[name] = fsum[:, f] / count
                f += 1
            elif name == "AUC":
                out[name] = isum[:, i].to(torch.float64) / (count * (2.0 * self.m)) if self.m else \
                    torch.full((isum.shape[0],), float("nan"), dtype=torch.float64, device=isum.device)
                i += 1
            else:
                out[name] = isum[:, i].to(torch.float64) / count
                i += 1
        return out


def _check_options(replicates, level, seed):
    b, _ = _check_replicates(replicates, 0)
    if not (isinstance(level, (int, float)) and 0.0 < float(level) < 1.0):
        raise ValueError(f"level must lie in (0, 1); got {level!r}")
    return b, float(level), negatives._check_seed(seed)


def _by_unit(systems, unit):
    """Per-unit sums of every column of ``systems`` plus a count column, units ascending: the table a cluster
    bootstrap resamples.  Returns (icols, fcols, number of units)."""
    s0 = systems[0]
    unit = torch.as_tensor(unit).reshape(-1).to(s0.dev)
    if unit.is_floating_point() or unit.numel() != s0.p:
        raise ValueError(f"unit must hold one integer per positive ({s0.p}); got {tuple(unit.shape)} {unit.dtype}")
    uniq, inv, counts = torch.unique(unit.to(torch.int64), return_inverse=True, return_counts=True)   # ascending
    n_units = uniq.numel()
    icols = [c for s in systems for c in s.icols] + [torch.ones(s0.p, dtype=torch.int64, device=s0.dev)]
    fcols = [c for s in systems for c in s.fcols]
    isum = torch.zeros(n_units, len(icols), dtype=torch.int64, device=s0.dev)
    isum.index_add_(0, inv, torch.stack(icols, dim=1))              # integers: exact in any order
    if n_units * int(isum.abs().max()) >= 1 << 63:
        raise ValueError("the per-unit sums are too large for int64 replicate sums")
    out_f = []
    if fcols:                                                        # floats: each unit's rows in their order, no atomics
        order = torch.sort(inv, stable=True).indices
        for c in fcols:
            out_f.append(torch.segment_reduce(c[order], "sum", lengths=counts))
    return [isum[:, c] for c in range(isum.shape[1])], out_f, n_units


def _replicates(systems, b, seed, unit):
    """Per system {name: float64 [B]} under one set of draws, and the number of rows resampled."""
    if unit is None:
        icols = [c for s in systems for c in s.icols]
        fcols = [c for s in systems for c in s.fcols]
        n = systems[0].p
    else:
        icols, fcols, n = _by_unit(systems, unit)
    isum, fsum = _sums_wide(icols, fcols, b, seed)
    # the B x C sums become metrics on the host: a division by a scalar is a multiplication by its reciprocal in
    # torch's device kernels, and the replicates are to be the same numbers whichever device summed them
    isum, fsum = isum.cpu(), fsum.cpu()
    count = float(n) if unit is None else isum[:, -1].to(torch.float64)
    out, i, f = [], 0, 0
    for s in systems:
        out.append(s.replicates(isum[:, i:i + len(s.icols)], fsum[:, f:f + len(s.fcols)], count))
        i, f = i + len(s.icols), f + len(s.fcols)
    return out, n


def _interval(reps: torch.Tensor, level: float):
    """(se, lo, hi) of fp64 replicates: standard deviation (ddof 1; 0 for a single replicate) and percentiles."""
    a = (1.0 - level) / 2.0
    se = float(reps.std(unbiased=True)) if reps.numel() > 1 else 0.0
    if bool(torch.isnan(reps).any()):
        return float("nan"), float("nan"), float("nan")
    q = torch.quantile(reps, torch.tensor([a, 1.0 - a], dtype=torch.float64, device=reps.device))
    return se, float(q[0]), float(q[1])


def bootstrap_metrics(pos, neg, k_list=(20, 50, 100), mrr: bool = True, auc=None, replicates: int = 1000, seed: int = 0,
                      level: float = 0.95, unit=None, return_replicates: bool = False) -> dict:
    """Standard errors and percentile intervals of ``link_metrics``' Hits@K, MRR and AUC by a bootstrap over the
    positives: ``{"Hits@K": {"value", "se", "lo", "hi"}, ..., "n": positives, "replicates": B}``.

    ``value`` is ``link_metrics``' float64 result; ``se`` the standard deviation of the B replicates (ddof 1); ``lo`` and
    ``hi`` ``torch.quantile`` of them at (1 - level) / 2 and 1 - (1 - level) / 2.  A replicate draws P positives with
    replacement (``bootstrap_sums``) and equals ``link_metrics`` of the drawn positives (with ``neg`` [P, K]: and their
    rows): Hits@K and AUC exactly, MRR to the rounding of an fp64 sum.  NaN scores count as in ``link_metrics``; one
    shared set with fewer than K negatives gives Hits@K = 1 with se 0.  ``return_replicates``: every metric also
    carries ``"replicates"``, its float64 [B] (a CPU tensor: the sums are turned into metrics on the host).

    NOT bootstrapped: AP -- it is no sum over positives (tp_i depends on the resampled set); AUC with ``neg`` [P, K]
    -- its negatives are the flattened pool, which would have to be resampled too: ``auc=None`` means on for one shared
    set and off for rows, ``auc=True`` with rows raises ValueError.  With one shared set the intervals are CONDITIONAL
    on the negatives: they say how the metric moves with the positives, not with the negative sample.

    ``unit`` (one integer per positive: the source node of citation2 / HeaRT positives, a user): a cluster bootstrap.
    The columns are summed per distinct unit (ascending, with a count column), units are resampled, and a replicate's
    metric is a ratio of sums; ``"units"`` reports how many there are."""
    ks = evaluate._check_ks(k_list)
    b, level, seed = _check_options(replicates, level, seed)
    cols = _Columns(pos, neg, ks, mrr, auc)
    (reps,), n = _replicates([cols], b, seed, unit)
    out = {}
    for name in cols.names:
        se, lo, hi = _interval(reps[name], level)
        out[name] = {"value": cols.value[name], "se": se, "lo": lo, "hi": hi}
        if return_replicates:
            out[name]["replicates"] = reps[name]
    out["n"], out["replicates"] = cols.p, b
    if unit is not None:
        out["units"] = n
    return out


def compare_metrics(pos_a, neg_a, pos_b, neg_b, k_list=(20, 50, 100), mrr: bool = True, auc=None,
                    replicates: int = 1000, seed: int = 0, level: float = 0.95, unit=None,
                    return_replicates: bool = False) -> dict:
    """Paired bootstrap of two systems scored on the SAME positives in the same order -- the model against a heuristic:
    ``compare_metrics(model_pos, model_neg, ra_pos, ra_neg)`` with ``ra_* = pair_heuristics(...)`` scores.  Both
    systems' columns sit in one table, so every replicate draws the same positives for both.

    Per metric ``{"a", "b", "diff", "se", "lo", "hi", "p"}``: the two values, ``diff = b - a``, the standard error and
    percentile interval of the replicates' differences d_r, and the two-sided
    ``p = min(1, 2 min((1 + #{d_r <= 0}) / (B + 1), (1 + #{d_r >= 0}) / (B + 1)))``.  Options, and what is not
    bootstrapped, as in ``bootstrap_metrics``; the two systems' negatives have the same layout."""
    ks = evaluate._check_ks(k_list)
    b, level, seed = _check_options(replicates, level, seed)
    a_cols, b_cols = _Columns(pos_a, neg_a, ks, mrr, auc), _Columns(pos_b, neg_b, ks, mrr, auc)
    if a_cols.p != b_cols.p:
        raise ValueError(f"the two systems score the same positives: got {a_cols.p} and {b_cols.p}")
    if a_cols.per_row != b_cols.per_row or a_cols.dev != b_cols.dev:
        raise ValueError("the two systems' negatives must have the same layout and device")
    (ra, rb), n = _replicates([a_cols, b_cols], b, seed, unit)
    out = {}
    for name in a_cols.names:
        d = rb[name] - ra[name]
        se, lo, hi = _interval(d, level)
        le, ge = int((d <= 0).sum()), int((d >= 0).sum())
        p = min(1.0, 2.0 * min((1 + le) / (b + 1), (1 + ge) / (b + 1)))
        va, vb = a_cols.value[name], b_cols.value[name]
        out[name] = {"a": va, "b": vb, "diff": vb - va, "se": se, "lo": lo, "hi": hi,
                     "p": p if not math.isnan(se) else float("nan")}
        if return_replicates:
            out[name]["replicates"] = d
    out["n"], out["replicates"] = a_cols.p, b
    if unit is not None:
        out["units"] = n
    return out


def bootstrap_by_bin(pos, neg, values, bins=evaluate.CN_BINS, k_list=(20, 50, 100), mrr: bool = True, auc=None,
                     replicates: int = 1000, seed: int = 0, level: float = 0.95,
                     return_replicates: bool = False) -> list:
    """``bootstrap_metrics`` per bin of ``metrics_by_bin``: the same half-open bins [lo, hi) of ``values`` and the same
    ``count``; each bin's positives are resampled within the bin (against ALL shared negatives, or with their own
    rows), bin i under the seed ``negatives.step_seed(seed, i)``.  One dict per bin: ``bin``, ``count`` and per metric
    ``{"value", "se", "lo", "hi"}`` -- NaN throughout for an empty bin, which launches nothing."""
    ks = evaluate._check_ks(k_list)
    _, level, seed = _check_options(replicates, level, seed)
    pos = torch.as_tensor(pos).reshape(-1)
    values = torch.as_tensor(values).reshape(-1).to(pos.device)
    if values.numel() != pos.numel():
        raise ValueError(f"values has {values.numel()} entries, pos {pos.numel()}")
    if not isinstance(neg, evaluate.SortedNegatives):
        neg = torch.as_tensor(neg)
        if neg.dim() == 2 and neg.shape[0] != pos.numel():
            raise ValueError(f"neg [P, K] must have one row per positive ({pos.numel()}), got {tuple(neg.shape)}")
        if neg.dim() not in (1, 2):
            raise ValueError("neg must be 1-D (shared negatives) or [P, K] (per-positive negatives)")
        neg = neg.to(pos.device)
    per_row = isinstance(neg, torch.Tensor) and neg.dim() == 2
    if auc and per_row:
        raise ValueError("AUC over [P, K] negatives is not bootstrapped")
    if not per_row:
        neg = evaluate.sort_negatives(neg)          # one sort for every bin
    names = [f"Hits@{k}" for k in ks] + (["MRR"] if mrr else []) + (["AUC"] if (auc or (auc is None and not per_row)) else [])
    nan = float("nan")
    out = []
    for i, (lo, hi) in enumerate(bins):
        m = (values >= lo) & (values < hi)
        count = int(m.sum().item())
        res = {"bin": (lo, hi), "count": count}
        if count == 0:
            res.update({name: {"value": nan, "se": nan, "lo": nan, "hi": nan} for name in names})
        else:
            r = bootstrap_metrics(pos[m], neg[m] if per_row else neg, ks, mrr, auc, replicates,
                                  negatives.step_seed(seed, i), level, None, return_replicates)
            res.update({name: r[name] for name in names})
        out.append(res)
    return out
