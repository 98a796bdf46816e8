"""Plain fp64 restatements and seeded input builders for the node-stage training kernels -- the LayerNorm backward family
of csrc/rowwise.hip, C = A^T B of csrc/gemm_f32.hip and the operators of train.py that the one-launch layer does not
take -- shared by tests/test_gpu_node_train_kernels.py (device) and tests/test_node_train_reference_host.py (CPU).

The restatements are torch on whatever device their inputs live on, in float64 whatever dtype those have.  The builders
draw on the CPU from seeded generators, so that the host test sees the very data the device test runs.  The launch
arithmetic of the kernels is restated here (``ln_lanes``, ``tn_chunk_rows``, ...); the device tests tie it to the
library through the workspace sizes the library reports, so that a changed cap fails loudly.  No GPU is needed to
import this module."""
import types

import numpy as np
import torch

# ------------------------------------------------------------------------------------------------ (A) LayerNorm backward
LN_EPS = 1e-5
LN_WIDTHS = (4, 32, 36, 64, 128, 132, 256)
LN_BLOCK_CAP = 1024                     # ln_bwd_launch: at most this many workgroups of 256 lanes
# rows above one trip of the capped grid: odd and 500 .. 1500, so that a few lane groups only take a second trip
LN_ABOVE_CAP = {4: 701, 32: 1001, 36: 777, 64: 1233, 128: 907, 132: 555, 256: 1499}
LN_KINK = 1e-4                          # ten times a 1e-5 bound on the fp32 error of gamma xhat + beta at |beta| <= 10
LN_DROP_P = 0.25
LN_DROP_SEED = 0xC2B2AE3D27D4EB4F       # high 32 bits non-zero
UNDECIDED_CAP = 0.01
COL_OFF, COL_ON = 1, 2                  # the columns with beta = -10 (never active) and beta = +10 (always active)


def ln_lanes(d):
    """Lanes that own a row (G of ln_bwd_launch)."""
    return 8 if d <= 32 else (16 if d <= 64 else (32 if d <= 128 else 64))


def ln_trip_rows(d):
    """Rows the capped grid holds in one trip: 32768 / 16384 / 8192 / 4096 at G = 8 / 16 / 32 / 64."""
    return LN_BLOCK_CAP * (256 // ln_lanes(d))


def ln_row_counts(d):
    """No row; one row; one row into a second workgroup; an odd count just above one trip of the capped grid."""
    return (0, 1, 256 // ln_lanes(d) + 1, ln_trip_rows(d) + LN_ABOVE_CAP[d])


def ln_stats64(x):
    """(xhat, rstd [M, 1]) of the rows of x in fp64: biased variance, eps 1e-5, the variance from the centred row."""
    x = x.double()
    c = x - x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt((c * c).mean(1, keepdim=True) + LN_EPS)
    return c * rstd, rstd


def ln_bwd64(x, dy, gamma, beta=None, relu=False, keep=None, drop_p=0.0):
    """Closed-form backward of y = dropout(ReLU(LN(x))) (``relu`` off: y = LN(x); ``keep`` None: no dropout) for the
    upstream gradient dy -> (dx, dgamma, dbeta, dxsum), all fp64; dxsum = column sums of dx, the gradient of a bias
    added in front of the LayerNorm.
        d = dy * keep / (1 - p) where gamma xhat + beta > 0, else 0;   g = d gamma
        dx = rstd (g - mean(g) - xhat mean(g xhat));   dgamma = sum_rows d xhat;   dbeta = sum_rows d"""
    xh, rstd = ln_stats64(x)
    gamma = gamma.double()
    d = dy.double()
    if keep is not None:
        d = torch.where(keep, d / (1.0 - drop_p), torch.zeros_like(d))
    if relu:
        d = torch.where(xh * gamma + beta.double() > 0, d, torch.zeros_like(d))
    g = d * gamma
    dx = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return dx, (d * xh).sum(0), d.sum(0), dx.sum(0)


def ln_row_tol(want, rel=1e-4):
    """rel * max(1, max|want|) row by row, [M, 1]: dx of a row scales with that row's rstd (0.1 .. 316 in ``ln_case``),
    so a bound taken over the whole tensor is set by the constant rows and lets every other row off."""
    return rel * want.abs().amax(1, keepdim=True).clamp_min(1.0)


def ln_pre64(x, gamma, beta):
    """The argument of the ReLU, gamma xhat + beta, in fp64."""
    return ln_stats64(x)[0] * gamma.double() + beta.double()


def ln_params(d):
    """gamma around 1 with every fifth entry negative and gamma[0] exactly 0; beta around 0 with beta[1] = -10 and
    beta[2] = +10 (beta[0] = 0.07: where gamma is 0 the ReLU's argument is beta alone, kept away from the kink)."""
    g = torch.Generator().manual_seed(7000 + d)
    gamma = 1 + 0.1 * torch.randn(d, generator=g)
    gamma[3::5] *= -1
    gamma[0] = 0.0
    beta = 0.1 * torch.randn(d, generator=g)
    beta[0], beta[COL_OFF], beta[COL_ON] = 0.07, -10.0, 10.0
    assert float(gamma[COL_OFF]) > 0.5 and float(gamma[COL_ON]) > 0.5 and int((gamma < 0).sum()) >= 1
    return gamma, beta


def ln_case(d, m):
    """Inputs of one LayerNorm backward launch, fp32 on the CPU: x [m, d] with a per-row scale in [0.1, 10] (log-uniform)
    and a per-row mean in [-5, 5] -- at scale 0.1 and mean 5 a one-pass variance E[x^2] - mean^2 loses four digits --,
    rows 0, m // 2 and m - 1 constant at 1.0 (var = 0, rstd = 1 / sqrt(eps); from m = 4 on), ``ln_params(d)``, and dy
    set to 0 where the fp64 argument of the ReLU lies within LN_KINK of 0 (``undecided``: its share of the elements)."""
    g = torch.Generator().manual_seed(100003 * d + m)
    scale = 10.0 ** (2 * torch.rand(m, 1, generator=g) - 1)
    mean = 10 * torch.rand(m, 1, generator=g) - 5
    x = (mean + scale * torch.randn(m, d, generator=g)).float()
    const = torch.zeros(m, dtype=torch.bool)
    if m >= 4:
        const[[0, m // 2, m - 1]] = True
        x[const] = 1.0
    gamma, beta = ln_params(d)
    dy = torch.randn(m, d, generator=g)
    pre = ln_pre64(x, gamma, beta)
    near = pre.abs() <= LN_KINK
    dy[near] = 0.0
    c = types.SimpleNamespace(d=d, m=m, x=x, dy=dy, gamma=gamma, beta=beta, const=const,
                              undecided=float(near.double().mean()) if m else 0.0)
    if m:
        # the -10 column is never active and the +10 column always is, by a margin no rounding crosses
        assert float(pre[:, COL_OFF].max()) < -1.0 and float(pre[:, COL_ON].min()) > 1.0
        assert int(const.sum()) in (0, 3) and bool((pre[const] == beta.double()).all())
        assert 0.1 <= float(scale.min()) and float(scale.max()) <= 10.0 and float(mean.abs().max()) <= 5.0
    return c


# ------------------------------------------------------------------------------------------------ (B) C = A^T B, exact
TN_ROWS = (1, 9, 63, 65, 257, 32837)
TN_SHAPES = ((32, 32), (36, 64), (64, 128), (132, 260), (7, 5), (1, 1433))


def tn_chunk_rows(m):
    """Rows of a chunk: max(64, ceil(M / 512)), rounded up to whole rounds of eight rows."""
    return (max(64, -(-m // 512)) + 7) // 8 * 8


def tn_chunks(m):
    return -(-m // tn_chunk_rows(m))


def tn_groups(n):
    """Row groups of a workgroup: its four wavefronts split the rounds of a chunk when the output is narrow."""
    return 4 if n <= 32 else (2 if n <= 64 else 1)


def tn_workspace_floats(m, n, k):
    return 0 if min(m, n, k) <= 0 else tn_chunks(m) * tn_groups(n) * (n * k + n)


def tn_case(m, n, k):
    """A [m, n], B [m, k] as fp32 with integer values in {-2 .. 2}, drawn with unequal weights (mean 0.5: no sum
    cancels by symmetry).  |sum| <= 4 m < 2^24, so every fp32 partial sum is exact in any order."""
    assert 4 * m < 2 ** 24
    g = torch.Generator().manual_seed(m * 1_000_003 + n * 1009 + k)
    p = torch.tensor([0.1, 0.15, 0.2, 0.25, 0.3])
    draw = lambda cols: (torch.multinomial(p, max(m, 1) * cols, replacement=True, generator=g)[:m * cols]
                         .reshape(m, cols) - 2).float()
    return draw(n), draw(k)


def tn_exact(a, b):
    """(A^T B, column sums of A) in int64."""
    ai = a.long()
    return ai.t() @ b.long(), ai.sum(0)


# ------------------------------------------------------------------------------------------------ (C) operators
GCN_NODES = 4603
GCN_IN = 40
LONG_ROW = 128                          # LPF_SPMM_LONG_ROW
FWD_REL, KINK_MARGIN = 2e-5, 10.0       # the forward tolerance u is held to, and the margin over it


def _plant(r, c, v, n, rng):
    """A row of more than LONG_ROW entries and a row of none, in A and in A^T: planted where the draw lacks them."""
    for hub_is_row in (True, False):
        deg = np.bincount(r if hub_is_row else c, minlength=n)
        if deg.max() <= LONG_ROW:
            hub = np.full(LONG_ROW + 40, int(deg.argmax()), np.int64)
            far = rng.choice(n, LONG_ROW + 40, replace=False).astype(np.int64)
            r = np.concatenate([r, hub if hub_is_row else far])
            c = np.concatenate([c, far if hub_is_row else hub])
            v = np.concatenate([v, ((rng.random(far.size) + 0.1) / 8).astype(np.float32)])
            _, first = np.unique(r * n + c, return_index=True)
            r, c, v = r[first], c[first], v[first]
    for idx in (0, 1):
        ends = (r, c)[idx]
        deg = np.bincount(ends, minlength=n)
        if deg.min() > 0:
            keep = ends != int(deg.argmin())
            r, c, v = r[keep], c[keep], v[keep]
    return r, c, v


def gcn_graph(n=GCN_NODES, n_edges=40000, seed=2):
    """A directed weighted graph as COO (r, c, v): ``data.chung_lu_graph`` with 40 % of the directed entries dropped (no
    symmetry left) and weights in (0.1, 1.1) / 8; A and A^T each with a hub row and an empty row."""
    from lpformer_amd import data
    ei, _ = data.chung_lu_graph(n, n_edges, gamma=2.1, seed=seed)
    rng = np.random.default_rng(n)
    keep = rng.random(ei.shape[1]) < 0.6
    r, c = ei[0][keep].astype(np.int64), ei[1][keep].astype(np.int64)
    v = ((rng.random(r.size) + 0.1) / 8).astype(np.float32)
    r, c, v = _plant(r, c, v, n, rng)
    for ends in (r, c):
        deg = np.bincount(ends, minlength=n)
        assert deg.max() > LONG_ROW and deg.min() == 0
    assert np.unique(r * n + c).size == r.size
    return r, c, v


def layer_params(m, d_in, d_out, seed):
    """x [m, d_in], W [d_out, d_in] / sqrt(d_in), a bias 0.1 randn, gamma 1 + 0.1 randn, beta 0.1 randn and the upstream
    gradient ``up`` [m, d_out], fp32 on the CPU (the draws of test_fused_layer_backward_matches_fp64_autograd)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    return types.SimpleNamespace(x=rn(m, d_in), w=rn(d_out, d_in) / d_in ** 0.5, b=0.1 * rn(d_out),
                                 g=1 + 0.1 * rn(d_out), be=0.1 * rn(d_out), up=rn(m, d_out))


def relu_ln_undecided(u64, gamma, beta):
    """Elements of ReLU(LN(u)) whose side of the kink an fp32 u within the forward tolerance may change:
    |gamma xhat + beta| <= 10 * 2e-5 max(1, max|u64|) * rstd_i |gamma_j|  ->  bool mask [M, D]."""
    xh, rstd = ln_stats64(u64)
    pre = xh * gamma.double() + beta.double()
    delta = KINK_MARGIN * FWD_REL * max(1.0, float(u64.abs().max())) * rstd * gamma.double().abs()
    return pre.abs() <= delta
