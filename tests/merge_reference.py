"""Synthetic online-softmax records and their fp64 merge (test helper; plain numpy, no GPU).

The record-merging kernels (``lpf_pair_attention_merge_f32``, the merge stage of ``lpf_tail_chain_merge_f32``) take the
records ``(acc[D], m, l)`` of the one-pass attention kernels as INPUTS.  This module makes such records from entries it
draws itself and states in fp64 what the merge has to return, so that a kernel is compared with a reference of the same
operation and the rounding of the scores stays out of the comparison.

Layout (include/lpformer_hip.h, comment of ``lpf_pair_attention_fused_f32``).  ``type_ptr`` int32 [3][bs + 1]: the
entries of (type t, pair p) are [type_ptr[t][p], type_ptr[t][p + 1]) of type t's region; a region is cut into units of
16 entries.  A segment inside one unit leaves ONE record in ``part[(t*bs + p)*(D + 4)]``; a segment that crosses units
leaves one boundary record per unit it touches in ``bnd[((t*units_cap + U)*2 + slot)*(D + 4)]``, slot 1 in the unit it
starts in and slot 0 in every later unit.  A record is ``acc[D], m, l, -, -`` over the entries of that piece:
m = max s_e, l = sum e^{s_e - m}, acc = sum e^{s_e - m} k_e.

Every float of ``part`` and ``bnd`` that this layout does not name is NaN here (the two pad floats of a record too), so
that a read of a wrong address shows as NaN and not as a small error.

Scores lie on a grid of 2^-8.  Every score, and every score shifted by +-1e4, is then an fp32 number (as the scores of
the real kernels are), so a record's ``m`` is exact and a shifted case holds exactly the shifted records.
"""
from __future__ import annotations

import numpy as np

UNIT = 16
LN_EPS = 1e-5
U32 = 2.0 ** -24                 # unit roundoff of fp32
SCORE_GRID = 2.0 ** -8
FAMILIES = ("equal", "pm3", "pm80", "pm300", "tie", "pm3_up", "pm3_down")
SHIFT = {"pm3_up": 1e4, "pm3_down": -1e4}
F32_EXP_ZERO = -104.0            # e^x rounds to 0 in fp32 (smallest denormal 2^-149 = e^-103.28, half of it e^-103.97)


# ------------------------------------------------------------------------------------------------- structure
def structure_counts(n_counts: int, bs: int = 149, seed: int = 0) -> np.ndarray:
    """Entry counts int64 [3, bs] of the structural case: per type a designed run of segments (see the comments), then
    random ones; the last pair rounds every region up to whole units, so that the case can be tiled.  Types that
    ``n_counts`` does not use (1: common neighbours only, 3: no >1-hop nodes) have empty segments."""
    designed = [
        # type 0, from entry 0:
        [1,      # [0, 1)      one entry
         15,     # [1, 16)     inside unit 0, ends exactly on a unit boundary
         16,     # [16, 32)    aligned, exactly one unit: a `part` record, not a boundary record
         17,     # [32, 49)    starts on a boundary, crosses one
         0,      #             empty between two crossing segments
         20,     # [49, 69)    starts in unit 3, where the segment before ends: slots 0 and 1 of unit 3 are two pairs'
         11,     # [69, 80)    inside unit 4 behind the tail of the segment before, ends on a boundary
         33,     # [80, 113)   starts on a boundary, crosses two
         3,      # [113, 116)  inside unit 7
         28,     # [116, 144)  crosses one, ends exactly on a boundary
         645,    # [144, 789)  41 units, crosses forty
         2, 0, 0, 16, 5],
        # type 1: the same kinds at other offsets (three leading pairs have no entry of this type)
        [0, 0, 0, 7, 17, 16, 1, 40, 0, 15, 9, 32, 18, 0, 0, 0, 0, 31],
        # type 2
        [0, 5, 0, 0, 27, 0, 650, 6, 16, 0, 0, 0, 0, 1, 15, 17],
    ]
    rng = np.random.default_rng(1000 + seed)
    pool = np.array([0, 0, 0, 0, 1, 2, 3, 5, 8, 15, 16, 17, 18, 31, 32, 33, 40])
    out = np.zeros((3, bs), np.int64)
    used = {1: 1, 3: 2, 4: 3}[n_counts]
    for t in range(used):
        seq = designed[t][:bs - 1]
        out[t, :len(seq)] = seq
        out[t, len(seq):bs - 1] = rng.choice(pool, size=bs - 1 - len(seq))
    if bs > 21:
        out[:, 19] = 0       # a pair without any entry in the random part, and pairs with one type only
        out[1:, 20] = 0
        out[0, 20] = 4
        out[0, 21] = out[2, 21] = 0
        out[1, 21] = 19 if used > 1 else 0
    out[:used, bs - 1] = (-out[:used, :bs - 1].sum(axis=1)) % UNIT
    return out


def single_pair_counts(n_counts: int) -> np.ndarray:
    """bs = 1: a crossing segment, a segment inside a unit and (n_counts 4) an aligned unit."""
    c = np.array([[37], [5], [16]], np.int64)
    c[{1: 1, 3: 2, 4: 3}[n_counts]:] = 0
    return c


def _pieces(type_ptr):
    """Per type: pair and unit of every entry, and the piece (run of entries with the same pair and unit) it is in."""
    out = []
    for t in range(3):
        tp = type_ptr[t].astype(np.int64)
        n = int(tp[-1] - tp[0])
        pair = np.repeat(np.arange(tp.size - 1), np.diff(tp))
        idx = tp[0] + np.arange(n)
        unit = idx >> 4
        new = np.ones(n, bool)
        new[1:] = (pair[1:] != pair[:-1]) | (unit[1:] != unit[:-1])
        start = np.flatnonzero(new)
        out.append({"pair": pair, "unit": unit, "start": start, "piece": np.cumsum(new) - 1,
                    "piece_pair": pair[start], "piece_unit": unit[start]})
    return out


def _grid(x):
    return np.round(np.asarray(x, np.float64) / SCORE_GRID) * SCORE_GRID


def _piece_maxima(family: str, rng, piece_pair: np.ndarray, bs: int) -> np.ndarray:
    """The score recipe: the maximum m of every piece (all types of a pair together; ``piece_pair`` sorted or not)."""
    n = piece_pair.size
    if family == "equal":
        return np.full(n, 1.5)
    if family in ("pm3", "pm3_up", "pm3_down", "tie"):
        m = _grid(rng.uniform(-3.0, 3.0, n))
        if family == "tie":      # two pieces of a pair share a maximum above every other piece: the last one and the
            for p in np.unique(piece_pair):      # second (a merge in this order has rescaled once before it meets it)
                ix = np.flatnonzero(piece_pair == p)
                if ix.size >= 2:
                    m[ix[1 if ix.size >= 3 else 0]] = m[ix[-1]] = m[ix].max() + 0.5
        return m + SHIFT.get(family, 0.0)
    if family == "pm80":
        return _grid(rng.uniform(-80.0, 80.0, n))
    if family == "pm300":
        # every third pair: all pieces within 1 of the pair's maximum (somewhere in +-300); the others: anywhere in
        # +-300, so most of their pieces have a weight that underflows to exactly 0
        m = _grid(rng.uniform(-300.0, 300.0, n))
        top = _grid(rng.uniform(-300.0, 300.0, bs))
        close = piece_pair % 3 == 0
        m[close] = top[piece_pair[close]] - _grid(rng.uniform(0.0, 1.0, int(close.sum())))
        return m
    raise ValueError(family)


# ------------------------------------------------------------------------------------------------- case
def make_case(counts: np.ndarray, D: int, n_counts: int, family: str, seed: int = 0) -> dict:
    """Entries (fp64 scores and keys), parameters and records of one case.  ``counts`` int [3, bs]."""
    counts = np.asarray(counts, np.int64)
    bs = counts.shape[1]
    rng = np.random.default_rng([seed, D, bs])     # (the family only shapes the maxima: pm3 / pm3_up / pm3_down share
    type_ptr = np.zeros((3, bs + 1), np.int32)     #  every draw)
    type_ptr[:, 1:] = np.cumsum(counts, axis=1)
    pcs = _pieces(type_ptr)
    # maxima per piece, drawn over the pieces of all types at once (the tie recipe looks at a pair's pieces together)
    all_pair = np.concatenate([pc["piece_pair"] for pc in pcs])
    m_all = _piece_maxima(family, np.random.default_rng([seed, D, bs, 1]), all_pair, bs)
    pair_dir = rng.standard_normal((bs, D))
    split = np.cumsum([0] + [pc["start"].size for pc in pcs])
    scores, keys, piece_m = [], [], []
    for t, pc in enumerate(pcs):
        n = pc["pair"].size
        m_t = m_all[split[t]:split[t + 1]]
        drop = _grid(rng.uniform(0.0, 2.0, n))
        drop[pc["start"]] = 0.0                    # a piece's first entry carries its maximum
        scores.append(m_t[pc["piece"]] - drop if n else np.zeros(0))
        piece_dir = rng.standard_normal((pc["start"].size, D))
        keys.append(pair_dir[pc["pair"]] + piece_dir[pc["piece"]] + 0.5 * rng.standard_normal((n, D)))
        piece_m.append(m_t)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731  (parameters the kernel reads as fp32)
    case = {"bs": bs, "D": D, "n_counts": n_counts, "family": family, "type_ptr": type_ptr, "scores": scores,
            "keys": keys, "pair": [pc["pair"] for pc in pcs], "piece_m": piece_m,
            "piece_pair": [pc["piece_pair"] for pc in pcs],
            "att_bias": f32(rng.standard_normal(D)), "ln_g": f32(1.0 + 0.2 * rng.standard_normal(D)),
            "ln_b": f32(0.1 * rng.standard_normal(D))}
    build_records(case, pcs)
    return case


def build_records(case: dict, pcs=None) -> None:
    """part float32 [3, bs, D + 4], bnd float32 [3, units_cap, 2, D + 4], NaN wherever the layout names no float."""
    bs, D, tp = case["bs"], case["D"], case["type_ptr"].astype(np.int64)
    pcs = _pieces(case["type_ptr"]) if pcs is None else pcs
    units_cap = int(max(1, -(-int(tp[:, -1].max()) // UNIT))) + 1     # (one spare unit: the type stride is not the
    part = np.full((3, bs, D + 4), np.nan, np.float32)                #  number of units in use)
    bnd = np.full((3, units_cap, 2, D + 4), np.nan, np.float32)
    for t, pc in enumerate(pcs):
        if pc["pair"].size == 0:
            continue
        s, k = case["scores"][t], case["keys"][t]
        m = np.maximum.reduceat(s, pc["start"])
        w = np.exp(s - m[pc["piece"]])
        rec = np.empty((pc["start"].size, D + 2))
        rec[:, :D] = np.add.reduceat(w[:, None] * k, pc["start"], axis=0)
        rec[:, D] = m
        rec[:, D + 1] = np.add.reduceat(w, pc["start"])
        assert np.array_equal(m.astype(np.float32).astype(np.float64), m), "scores must be fp32 numbers"
        pp, pu = pc["piece_pair"], pc["piece_unit"]
        lo, hi = tp[t, pp], tp[t, pp + 1]
        u0 = lo >> 4
        one = ((hi - 1) >> 4) == u0
        assert np.unique(pp[one]).size == one.sum()
        part[t, pp[one], :D + 2] = rec[one]
        slot = (pu == u0).astype(np.int64)[~one]
        flat = pu[~one] * 2 + slot
        assert np.unique(flat).size == flat.size, "two records for one boundary slot"
        bnd[t, pu[~one], slot, :D + 2] = rec[~one]
    case["part"], case["bnd"], case["units_cap"] = part, bnd, units_cap


def tile_case(case: dict, reps: int, drop_last: int = 0) -> dict:
    """``reps`` copies of a case whose regions are whole units (structure_counts), one behind the other, without the
    last ``drop_last`` pairs: pointers, records and NaN are those of the copies, so a reference row of the tiled case
    is the reference row of the pair it copies (``tiled_rows``)."""
    bs0, D = case["bs"], case["D"]
    tp0 = case["type_ptr"].astype(np.int64)
    length = tp0[:, -1]
    assert (length % UNIT == 0).all() and (tp0[:, 0] == 0).all()
    bs = bs0 * reps - drop_last
    tp = np.concatenate([(tp0[:, :-1, None] + length[:, None, None] * np.arange(reps)).transpose(0, 2, 1)
                         .reshape(3, -1), (length * reps)[:, None]], axis=1)[:, :bs + 1]
    assert tp.max() < 2 ** 31
    units = length // UNIT
    units_cap = int(units.max()) * reps + 1
    bnd = np.full((3, units_cap, 2, D + 4), np.nan, np.float32)
    for t in range(3):
        bnd[t, :units[t] * reps] = np.tile(case["bnd"][t, :units[t]], (reps, 1, 1))
    out = {k: case[k] for k in ("D", "n_counts", "family", "att_bias", "ln_g", "ln_b")}
    out.update(bs=bs, type_ptr=tp.astype(np.int32), part=np.tile(case["part"], (1, reps, 1))[:, :bs].copy(), bnd=bnd,
               units_cap=units_cap, tiled_from=bs0)
    return out


def tiled_rows(rows0: np.ndarray, bs: int) -> np.ndarray:
    return np.tile(rows0, (-(-bs // rows0.shape[0]), 1))[:bs]


# ------------------------------------------------------------------------------------------------- references
def direct_softmax(case: dict) -> np.ndarray:
    """(a) PyG's segment softmax over ALL entries of a pair, fp64: alpha_e = e^{s_e - M} / (sum e^{s_e - M} + 1e-16),
    out = sum alpha_e k_e + att_bias; a pair without entries gives att_bias.  [bs, D], before post_att_norm."""
    bs, D = case["bs"], case["D"]
    pair = np.concatenate(case["pair"])
    s = np.concatenate(case["scores"])
    k = np.concatenate(case["keys"])
    top = np.full(bs, -np.inf)
    np.maximum.at(top, pair, s)
    e = np.exp(s - top[pair])
    den = np.zeros(bs)
    np.add.at(den, pair, e)
    out = np.zeros((bs, D))
    np.add.at(out, pair, k * (e / (den[pair] + 1e-16))[:, None])
    return out + case["att_bias"]


def pair_records(case: dict, p: int):
    """The records of pair p, read from ``part`` / ``bnd`` at the addresses the header documents: (acc [n, D], m, l)."""
    bs, D, tp = case["bs"], case["D"], case["type_ptr"]
    rs = D + 4
    part, bnd = case["part"].reshape(-1), case["bnd"].reshape(-1)
    recs = []
    for t in range(3):
        lo, hi = int(tp[t, p]), int(tp[t, p + 1])
        if hi <= lo:
            continue
        u0, u1 = lo // UNIT, (hi - 1) // UNIT
        if u0 == u1:
            at = [(t * bs + p) * rs]
        else:
            at = [((t * case["units_cap"] + u) * 2 + (1 if u == u0 else 0)) * rs for u in range(u0, u1 + 1)]
        src = part if u0 == u1 else bnd
        recs += [src[a:a + D + 2].astype(np.float64) for a in at]
    r = np.array(recs).reshape(-1, D + 2)
    return r[:, :D], r[:, D], r[:, D + 1]


def merged_records(case: dict) -> np.ndarray:
    """(b) the merge of the fp32 records in fp64:  sum_P e^{m_P - M} acc_P / (sum_P e^{m_P - M} l_P + 1e-16) +
    att_bias, M = max_P m_P; no record gives att_bias.  [bs, D], before post_att_norm."""
    out = np.zeros((case["bs"], case["D"]))
    for p in range(case["bs"]):
        acc, m, l = pair_records(case, p)
        if m.size:
            w = np.exp(m - m.max())
            out[p] = (w[:, None] * acc).sum(axis=0) / ((w * l).sum() + 1e-16)
    return out + case["att_bias"]


def layer_norm(x, g, b):
    mu = x.mean(axis=-1, keepdims=True)
    xc = x - mu
    return xc / np.sqrt((xc * xc).mean(axis=-1, keepdims=True) + LN_EPS) * g + b


def count_features(type_ptr, n_counts: int) -> np.ndarray:
    """get_structure_cnts: n_cn, n_1hop, [n_non1hop,] n_cn + n_1hop; n_cn alone for n_counts == 1.  [bs, n_counts]."""
    c = np.diff(np.asarray(type_ptr, np.int64), axis=1).astype(np.float64)
    if n_counts == 1:
        return c[0][:, None]
    if n_counts == 3:
        return np.stack([c[0], c[1], c[0] + c[1]], axis=1)
    return np.stack([c[0], c[1], c[2], c[0] + c[1]], axis=1)


def features(case: dict, pre: np.ndarray) -> np.ndarray:
    """What lpf_pair_attention_merge_f32 writes: [post_att_norm(pre) (D) | count features (n_counts)]."""
    return np.concatenate([layer_norm(pre, case["ln_g"], case["ln_b"]),
                           count_features(case["type_ptr"], case["n_counts"])], axis=1)


def record_rounding_bound(case: dict) -> np.ndarray:
    """|(a) - (b)| before the norm, per element, first order.  A record's m is exact (scores are fp32 numbers); its acc
    and l carry one fp32 rounding each, relative error <= 2^-24 =: u.  With N = sum w_P acc_P, den = sum w_P l_P:
        |d(N / den)| <= u sum w_P |acc_P| / den + u |N| / den.
    [bs, D]; second-order terms and the fp64 evaluation are left to the caller's slack."""
    out = np.zeros((case["bs"], case["D"]))
    for p in range(case["bs"]):
        acc, m, l = pair_records(case, p)
        if m.size:
            w = np.exp(m - m.max())
            den = (w * l).sum()
            out[p] = U32 * ((w[:, None] * np.abs(acc)).sum(axis=0) + np.abs((w[:, None] * acc).sum(axis=0))) / den
    return out


def layer_norm_bound(x, dx, g):
    """|d LayerNorm(x)| for |dx| elementwise, first order: dy = g / sd (dx - mean dx - xhat mean(xhat dx))."""
    mu = x.mean(axis=-1, keepdims=True)
    sd = np.sqrt(((x - mu) ** 2).mean(axis=-1, keepdims=True) + LN_EPS)
    xhat = np.abs(x - mu) / sd
    return np.abs(g) / sd * (dx + dx.mean(axis=-1, keepdims=True) + xhat * (xhat * dx).mean(axis=-1, keepdims=True))


# ------------------------------------------------------------------------------------------------- dense tail
def tail_weights(D: int, n_counts: int, seed: int = 0) -> dict:
    """Unpacked weights of the dense tail, fp32 numbers held in fp64: pairwise_lin's first layer W_p0 [pd, pd] with its
    LayerNorm, the folded score head [A_e | A_p] [2D, D + pd] with bias c, and the final dot; pd = D + n_counts."""
    rng = np.random.default_rng([seed, D, n_counts, 7])
    pd = D + n_counts
    f32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    w_p0 = rng.standard_normal((pd, pd)) / np.sqrt(pd)
    w_p0[:, D:] *= 0.05          # counts run to several hundred: keep them from drowning the attention features
    return {"w_p0": f32(w_p0), "b_p0": f32(0.1 * rng.standard_normal(pd)),
            "lnB_g": f32(1.0 + 0.2 * rng.standard_normal(pd)), "lnB_b": f32(0.1 * rng.standard_normal(pd)),
            "A": f32(rng.standard_normal((2 * D, D + pd)) / np.sqrt(D + pd)), "c": f32(0.1 * rng.standard_normal(2 * D)),
            "w_dot": f32(rng.standard_normal(2 * D) / np.sqrt(D)), "b_dot": f32(0.1 * rng.standard_normal(1))}


def tail_ref(rows: np.ndarray, counts: np.ndarray, r_e: np.ndarray, w: dict):
    """What lpf_tail_chain_merge_f32 does behind the merge and post_att_norm, fp64:
        r_p = ReLU(LayerNorm(W_p0 [row | counts] + b_p0)),  logit = w_dot . ReLU(A [r_e | r_p] + c) + b_dot,
        prob = sigmoid(logit).
    rows [bs, D] (post_att_norm output), counts [bs, n_counts], r_e [bs, D]."""
    x = np.concatenate([rows, counts], axis=1)
    r_p = np.maximum(layer_norm(x @ w["w_p0"].T + w["b_p0"], w["lnB_g"], w["lnB_b"]), 0.0)
    hid = np.concatenate([r_e, r_p], axis=1) @ w["A"].T + w["c"]
    logit = np.maximum(hid, 0.0) @ w["w_dot"] + float(w["b_dot"][0])
    return logit, 1.0 / (1.0 + np.exp(-logit))


# ------------------------------------------------------------------------------------------------- conditions
def structure_facts(type_ptr) -> dict:
    """What the structural case has to contain, read back from its segment pointers."""
    tp = np.asarray(type_ptr, np.int64)
    lo, hi = tp[:, :-1], tp[:, 1:]
    n = hi - lo
    some = n > 0
    u0, u1 = lo >> 4, (np.maximum(hi, 1) - 1) >> 4
    crossed = np.where(some, u1 - u0, 0)
    cross = some & (crossed > 0)
    slot1 = {(t, int(u)) for t in range(3) for u in u0[t][cross[t]]}
    slot0_last = {(t, int(u)) for t in range(3) for u in u1[t][cross[t]]}
    types_used = some.sum(axis=0)
    return {"lengths": set(np.unique(n).tolist()),
            "empty_pairs": int((types_used == 0).sum()),
            "one_type_pairs": int((types_used == 1).sum()),
            "cross_from_boundary": int((cross & (lo % UNIT == 0)).sum()),
            "end_on_boundary": int((some & (hi % UNIT == 0)).sum()),
            "aligned_unit": int((some & (n == UNIT) & (lo % UNIT == 0)).sum()),
            "boundaries": set(np.unique(crossed[cross]).tolist()),
            "shared_units": len(slot1 & slot0_last),
            "empty_segments": int((~some).sum())}


def nan_share(case: dict):
    return float(np.isnan(case["part"]).mean()), float(np.isnan(case["bnd"]).mean())
