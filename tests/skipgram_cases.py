"""Graphs, walk buffers, tables, references and error bounds shared by tests/test_skipgram_host.py and
tests/test_gpu_skipgram.py.  Every reference is computed once per process and handed out; nothing changes it.

Graphs: S and C of tests/random_walks_cases.py; ``star`` -- hub 0 and 300 leaves, so every pair touches the hub and its
segment of the occurrence list crosses dozens of chunks; ``iso`` -- a path, a triangle and two isolated nodes, whose
walks stay where they are, so pairs with c == x exist (the star's walks return to their start as well).

Tables are standard normal times min(1, sqrt(0.8 / sqrt(dim))): the logits of a dim-512 standard normal table have a
standard deviation of 22.6, and ``(1 - s) + 1e-15`` of the loss as PyG writes it has no digits left in fp64 once a
negative pair's logit passes about 25 (the reference itself is then noise; lpformer_amd/skipgram.py's docstring).  The
scale keeps the logits of pairs with c != x at about 0.8.  A pair with c == x has the logit |E[c]|^2, about
0.8 sqrt(dim): 9 at dim 128, 18 at dim 512; tests/test_skipgram_host.py asserts that every logit is below 25.

Error model of the three entries (u = 2^-23; everything here fp64, from the reference's own magnitudes):

  logit        |dl| <= C1 u L1,                L1 = sum_j |E[c]_j E[x]_j|
  coefficient  |dg| <= scale / 4 * C1 u L1 + C1 u |g|          (|dg/dl| = scale |s (1 - s) ...| <= scale / 4)
  gradient     |d grad[u]_j| <= C2 u sum_occ |g| |E[other]_j| + sum_occ b_g |E[other]_j|        (b_g the line above)
  Adam         |d m| <= C3 u (|m| + (|g| + |m|)(1 - beta1)),   |d v| <= C3 u (|v| + (g^2 + |v|)(1 - beta2)),
               |d p| <= C3 u (|p| + |upd|) + step_size (b_m / den + |m'| b_v / (2 sqrt(v') den^2)),
               upd = step_size m' / den, den = sqrt(v') + eps  (m', v' the new moments; the second term carries their
               bounds into the quotient)

C1, C2, C3: the next power of two at or above twice the worst ratio error / (u magnitude) measured over all cases on
an MI355X (tests/test_gpu_skipgram.py prints the ratios):
  coefficient 0.444 (bad_d36; 0.135 .. 0.444 over the cases)                      -> C1 = 1
  gradient    4.465 (iso_d512, a row of 62 occurrences of one sign; 1.09 .. 4.47)  -> C2 = 16
  Adam        m 1.123, v 1.870, p 0.897 (C_d128, iso_d512, S_d36_ctx2)             -> C3 = 4
The gradient ratios are those of fp32 itself: a sequential fused-multiply-add sum emulated on the CPU in the kernel's
order gives the same three leading figures (4.465, 3.764, 1.765 for iso_d512, S_d36_ctx2, C_d128).
"""
from functools import lru_cache
from typing import NamedTuple

import numpy as np
import torch

from lpformer_amd import graph, skipgram
from lpformer_amd.random_walks import walks_reference
from tests import pair_distance_cases as DC
from tests import random_walks_cases as RC

U23 = 2.0 ** -23
C1, C2, C3 = 1.0, 16.0, 4.0
CHUNK = skipgram.CHUNK
LR = 0.05
STAR_LEAVES = 300


def _csr(rows, cols, n) -> graph.CSR:
    A = DC._adjacency(np.asarray(rows), np.asarray(cols), n)
    return graph.CSR(A.indptr.astype(np.int64), A.indices.astype(np.int32), None, n)


@lru_cache(maxsize=None)
def graph_star() -> graph.CSR:
    leaves = np.arange(1, STAR_LEAVES + 1)
    return _csr(np.zeros(STAR_LEAVES, np.int64), leaves, STAR_LEAVES + 1)


@lru_cache(maxsize=None)
def graph_iso() -> graph.CSR:
    """Path 0-1-2-3, triangle 4-5-6, nodes 7 and 8 isolated."""
    return _csr([0, 1, 2, 4, 5, 6], [1, 2, 3, 5, 6, 4], 9)


GRAPHS = {"S": lambda: RC.case("S").csr, "C": lambda: RC.case("C").csr, "star": graph_star, "iso": graph_iso}


class Spec(NamedTuple):
    graph: str
    dim: int
    length: int
    context: int
    walks: int                 # W: the first W of the start list (every node, repeated); never a multiple of 64
    pad: int                   # ld - W of both walk buffers
    bad: bool = False          # one start outside [0, n)


# dims 4, 36 (% 4 but not % 16), 128, 512; context 2 (one pair per window) and L + 1 (one window per walk); ld > W
SPECS = {
    "C_d128": Spec("C", 128, 10, 5, 100, 0),
    "S_d36_ctx2": Spec("S", 36, 6, 2, 150, 7),
    "S_d4_onewindow": Spec("S", 4, 5, 6, 70, 0),
    "star_d128": Spec("star", 128, 8, 4, 301, 3),
    "iso_d512": Spec("iso", 512, 4, 3, 27, 0),
    "C_d512_long": Spec("C", 512, 20, 10, 33, 0),
    "bad_d36": Spec("S", 36, 6, 3, 70, 2, True),
}
NAMES = tuple(SPECS)
GOOD = tuple(k for k, s in SPECS.items() if not s.bad)


class Case(NamedTuple):
    spec: Spec
    n: int
    table: torch.Tensor        # float32 [n, dim]
    pos: torch.Tensor          # int32 [L + 1, W], row stride W + pad
    neg: torch.Tensor


def _buffer(walks: torch.Tensor, pad: int) -> torch.Tensor:
    """[W, L + 1] -> the step-major [L + 1, W] view of a buffer [L + 1, W + pad] whose padding holds a bad id."""
    W = walks.shape[0]
    buf = torch.full((walks.shape[1], W + pad), 1 << 30, dtype=torch.int32)
    buf[:, :W] = walks.t()
    return buf[:, :W]


@lru_cache(maxsize=None)
def case(name: str) -> Case:
    sp = SPECS[name]
    csr = GRAPHS[sp.graph]()
    n = int(csr.n)
    gen = torch.Generator().manual_seed(1000 + NAMES.index(name))
    starts = torch.arange(n).repeat(-(-sp.walks // n))[:sp.walks].clone()
    if sp.bad:
        starts[5] = n + 3
    walks = walks_reference(csr, starts, length=sp.length, seed=11).walks
    noise = torch.randint(n, (sp.walks, sp.length), generator=gen)
    negw = torch.cat([walks[:, :1].to(torch.int64), noise], dim=1).to(torch.int32)    # the start (a bad one: -1), then noise
    scale = min(1.0, (0.8 / sp.dim ** 0.5) ** 0.5)
    table = (torch.randn((n, sp.dim), generator=gen, dtype=torch.float64) * scale).to(torch.float32)
    return Case(sp, n, table, _buffer(walks, sp.pad), _buffer(negw, sp.pad))


def state_of(ref) -> skipgram.SkipGramState:
    """The fp32 state a device run has after the step ``ref`` describes."""
    return skipgram.SkipGramState(ref.exp_avg.to(torch.float32), ref.exp_avg_sq.to(torch.float32), ref.step)


@lru_cache(maxsize=None)
def reference(name: str):
    """``skipgram_reference`` of the first step of a case (zero state, lr ``LR``)."""
    c = case(name)
    return skipgram.skipgram_reference(c.table, skipgram.skipgram_state(c.table), c.pos, c.neg, c.spec.context, lr=LR)


@lru_cache(maxsize=None)
def second(name: str):
    """(table float32, state float32, reference) of a second step: from the first step's result rounded to fp32."""
    c, first = case(name), reference(name)
    table, state = first.table.to(torch.float32), state_of(first)
    return table, state, skipgram.skipgram_reference(table, state, c.pos, c.neg, c.spec.context, lr=LR)


# ------------------------------------------------------------------------------------------------------ the bounds
def occurrences(ref):
    """(row, other, pair) int64 [2 M'] of a reference's good pairs, sorted by row and within a row by occurrence id."""
    M = ref.coef.numel()
    keys = torch.cat([ref.centre, ref.other])
    order = torch.sort(keys, stable=True).indices
    order = order[keys[order] >= 0]
    return keys[order], torch.cat([ref.other, ref.centre])[order], order % M


def logit_magnitude(table, ref) -> torch.Tensor:
    """L1 [M] = sum_j |E[c]_j E[x]_j| (0 for a bad pair)."""
    E = table.to(torch.float64)
    ok = ref.centre >= 0
    mag = torch.zeros(ref.coef.numel(), dtype=torch.float64)
    mag[ok] = (E[ref.centre[ok]] * E[ref.other[ok]]).abs().sum(dim=1)
    return mag


def pair_scale(c: Case, M: int) -> torch.Tensor:
    """1 / Mp for the positive pairs, 1 / Mn for the negative ones [M]."""
    nwin = c.spec.length + 2 - c.spec.context
    Mp = c.pos.shape[1] * nwin * (c.spec.context - 1)
    out = torch.full((M,), 1.0 / max(M - Mp, 1), dtype=torch.float64)
    out[:Mp] = 1.0 / max(Mp, 1)
    return out


def coef_bound(c: Case, table, ref, c1=C1):
    """(b_l, b_g) [M]: the logit's and the coefficient's bound."""
    b_l = c1 * U23 * logit_magnitude(table, ref)
    return b_l, pair_scale(c, ref.coef.numel()) / 4.0 * b_l + c1 * U23 * ref.coef.abs()


def grad_bound(table, ref, b_g, c2=C2, own_only=False):
    """[U, dim]: C2 u sum_occ |g| |E[other]| plus the coefficients' bound carried through the same sum."""
    E = table.to(torch.float64).abs()
    row, other, pair = occurrences(ref)
    u_of = torch.searchsorted(ref.rows, row)
    own = torch.zeros_like(ref.grad).index_add_(0, u_of, ref.coef.abs()[pair, None] * E[other])
    if own_only:
        return own
    return c2 * U23 * own + torch.zeros_like(ref.grad).index_add_(0, u_of, b_g[pair, None] * E[other])


def adam_expected(table, state, rows, grad, lr=LR, betas=(0.9, 0.999), eps=1e-8, c3=C3):
    """SparseAdam's formulas in fp64 on the given (fp32) inputs for the listed rows: dict of the new m, v, p [U, dim]
    and their bounds b_m, b_v, b_p."""
    f = torch.float64
    g, m, v, p = grad.to(f), state.exp_avg.to(f)[rows], state.exp_avg_sq.to(f)[rows], table.to(f)[rows]
    b1, b2 = betas
    step = state.step + 1
    m2 = m + (g - m) * (1.0 - b1)
    v2 = v + (g * g - v) * (1.0 - b2)
    step_size = lr * (1.0 - b2 ** step) ** 0.5 / (1.0 - b1 ** step)
    den = v2.sqrt() + eps
    upd = step_size * m2 / den
    b_m = c3 * U23 * (m.abs() + (g.abs() + m.abs()) * (1.0 - b1))
    b_v = c3 * U23 * (v.abs() + (g * g + v.abs()) * (1.0 - b2))
    carried = step_size * (b_m / den + torch.where(v2 > 0, m2.abs() * b_v / (2.0 * v2.sqrt() * den * den), 0.0))
    return {"m": m2, "v": v2, "p": p - upd, "b_m": b_m, "b_v": b_v, "b_p": c3 * U23 * (p.abs() + upd.abs()) + carried}


# ----------------------------------------------------------------------- occurrence lists built directly (grad kernel)
EDGE_LENGTHS = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 1, 3)


@lru_cache(maxsize=None)
def integer_lists(dim: int = 36, n: int = 50):
    """An integer-valued problem for ``lpf_skipgram_grad_rows_f32``: table entries in -3 .. 3, coefficients in -4 .. 4,
    one segment per length of ``EDGE_LENGTHS`` (every chunk edge) -- every partial sum stays below
    (2 CHUNK + 1) * 12 < 2^24, so fp32 adds them exactly in any order and grad must EQUAL the integer sums.
    Returns dict: table float32 [n, dim], coef float32 [M], occ_other, occ_pair int32, seg int64, want float64."""
    rng = np.random.default_rng(5)
    M = 400
    table = rng.integers(-3, 4, (n, dim)).astype(np.float32)
    coef = rng.integers(-4, 5, M).astype(np.float32)
    total = sum(EDGE_LENGTHS)
    other = rng.integers(0, n, total).astype(np.int32)
    pair = rng.integers(0, M, total).astype(np.int32)
    seg = np.concatenate([[0], np.cumsum(EDGE_LENGTHS)]).astype(np.int64)
    want = np.stack([(coef[pair[a:b], None].astype(np.float64) * table[other[a:b]]).sum(axis=0)
                     for a, b in zip(seg[:-1], seg[1:])])
    return {k: torch.from_numpy(v) for k, v in dict(table=table, coef=coef, occ_other=other, occ_pair=pair, seg=seg,
                                                    want=want).items()}
