"""Plain fp64 restatements, restated launch arithmetic and seeded input builders for the encoder's forward kernels --
csrc/spmm_csr.hip (GCN normalisation, CSR SpMM with the fused epilogue, hub-row slices), csrc/gcn_fused.hip (the
one-launch layer) and the forward part of csrc/rowwise.hip (LayerNorm, endpoint gather, dot + sigmoid) -- shared by
tests/test_gpu_node_forward_kernels.py (device) and tests/test_node_forward_reference_host.py (CPU).

The restatements are torch on whatever device their inputs live on, in float64 whatever dtype those have.  The builders
draw on the CPU from seeded generators, so that the host test sees the very data the device test runs.  Two of the
edges are data-dependent -- the SPMM_LONG boundary and the hub / ordinary lane pair of gcn_fused.hip -- and a random
graph meets them by luck: ``planted_graph`` builds a CSR whose rows have exactly the lengths asked for.  Its columns
never name row 0 of the gathered table: lanes past the end of a row gather (row 0, weight 0) in both kernels, and the
device tests pin that row 0 reaches no output that way.  No GPU is needed to import this module."""
import types

import numpy as np
import torch

FWD_TOL = 2e-5                          # x max(1, max|ref|): test_fused_gcn_layer_matches_two_launches, the training file
LN_EPS = 1e-5
SENTINEL = 7.0
LONG_ROW = 128                          # LPF_SPMM_LONG_ROW: spmm_csr.hip's hub threshold
FUSED_LONG, FUSED_PART = 64, 256        # graph.fused_row_order: hub threshold and slice length of the one-launch layer
BLOCK_CAP = 8192                        # spmm_launch / grid_for_rows: at most 256 x 32 workgroups of four wavefronts
# + bias always; then (LayerNorm, ReLU, residual, final LayerNorm): the four combinations of test_spmm_fused_epilogue
EPILOGUES = ((True, True, True, True), (False, False, False, False), (True, False, False, True), (False, True, True, False))

SPMM_F32_WIDTHS = (4, 24, 36, 64, 96, 128, 132, 256)
SPMM_BF16_WIDTHS = (8, 64, 136, 256)
SPMM_TRIP_CASES = ((132, 5), (128, 7))  # (D, rows above one trip of the capped grid)
PARTS_F32_WIDTHS, PARTS_BF16_WIDTHS = (8, 24, 64, 128), (64, 128)
PARTS_MANY = 70000
FUSED_F32_WIDTHS, FUSED_BF16_WIDTHS = (32, 64, 128), (64, 128)
FUSED_SMALL_TILES = (1, 8, 9)
LN_WIDTHS = (1, 3, 63, 64, 65, 1000, 1024)
GATHER_WIDTHS = (4, 36, 64, 132, 256)
ROWDOT_WIDTHS = (1, 63, 64, 65, 130)
NC_BASE, NC_DELTA = 5.0, 3 * 2.0 ** -11  # the near-constant rows: 5 +- 3 / 2048
U32 = 2.0 ** -24                         # the unit roundoff of fp32
LN_COND_WIDTHS = (3,)                    # widths whose drawn rows are held to ``ln_cond_ratio`` (see there)
LN_COND_K = 16.0                         # 4 x the worst ratio an MI355X measured over three seeds (3.63, 3.74, 3.76), rounded
                                         # up to a power of two: the rule of tests/test_gpu_f32_reference.py


# ------------------------------------------------------------------------------------------------ launch arithmetic
def spmm_shape(d, bf16=False):
    """(V, G, rows per wavefront, NG) of spmm_launch: V float4 per lane -- 2 for a bf16 table, else 1 when D % 8 != 0 or
    D > 128 and 2 otherwise --, G = (16 / 32 / 64 at D <= 64 / <= 128 / above) / V lanes per row, NG = 256 / G lane
    groups of a hub row's workgroup."""
    v = 2 if bf16 else (1 if (d % 8 != 0 or d > 128) else 2)
    g = (16 if d <= 64 else (32 if d <= 128 else 64)) // v
    return v, g, 64 // g, 256 // g


def spmm_trip_rows(d, bf16=False):
    """Rows the capped grid of spmm_csr_kernel holds in one trip."""
    return BLOCK_CAP * 4 * spmm_shape(d, bf16)[2]


def rowwise_trip_rows():
    """Rows one trip of layernorm_kernel / rowdot_sigmoid_kernel holds: 8192 workgroups x 4 wavefronts, a row each."""
    return BLOCK_CAP * 4


def gather_trip_rows(d):
    """Pairs one trip of pair_gather_kernel holds: G = 16 / 32 / 64 lanes per pair at D <= 64 / <= 128 / above."""
    g = 16 if d <= 64 else (32 if d <= 128 else 64)
    return BLOCK_CAP * 4 * (64 // g)


def parts_shape(d):
    """(G, NG) of spmm_row_parts_kernel: always two float4 per lane."""
    g = 8 if d <= 64 else 16
    return g, 256 // g


def fused_nbp(d):
    """Neighbours of each row of a lane pair requested per step of gcn_fused_kernel."""
    return 4 if d == 128 else 2


def fused_cap_tiles(d, cu):
    """Tiles the first round of gcn_fused_kernel takes by position: 8 wavefronts x (1 workgroup per CU at D = 128, 2
    below) x CUs; tiles past it are drawn from the LDS ticket."""
    return 8 * (1 if d == 128 else 2) * cu


def spmm_lengths(d, bf16=False):
    """Row lengths at the edges of spmm_accumulate (four gathers a step, chunks of G), of SPMM_LONG and of the hub
    kernel's round-robin (NG groups x G entries a round)."""
    _, g, _, ng = spmm_shape(d, bf16)
    return sorted({0, 1, 3, 4, 5, g - 1, g, g + 1, 2 * g + 3, 127, 128, 129, g * ng - 1, g * ng, g * ng + 1,
                   3 * g * ng + 7})


def fused_lengths(d):
    """Row lengths at the edges of gcn_fused_kernel's steps of NBP entries, of the hub threshold and of the slices."""
    nbp = fused_nbp(d)
    return sorted({0, 1, nbp - 1, nbp, nbp + 1, 2 * nbp + 1, 63, 64, 65, 256, 257, 700})


# ------------------------------------------------------------------------------------------------ planted graphs
def planted_graph(lengths, n_cols, seed):
    """CSR (rowptr int64, col int32, val fp32; numpy) whose row r has exactly ``lengths[r]`` entries: columns distinct
    and ascending within a row, in [1, n_cols) -- never 0 --, weights in (0.5, 1.5).  A row's columns are
    1 + (start + k step) mod m with m the largest power of two <= n_cols - 1 and an odd step: distinct up to m entries."""
    lengths = np.asarray(lengths, np.int64)
    assert n_cols >= 2 and lengths.ndim == 1 and (lengths.size == 0 or lengths.min() >= 0)
    m = 1 << int(np.floor(np.log2(n_cols - 1)))
    assert lengths.size == 0 or lengths.max() <= m, (int(lengths.max()), m)
    rng = np.random.default_rng(seed)
    rowptr = np.zeros(lengths.size + 1, np.int64)
    np.cumsum(lengths, out=rowptr[1:])
    nnz = int(rowptr[-1])
    rows = np.repeat(np.arange(lengths.size), lengths)
    k = np.arange(nnz, dtype=np.int64) - rowptr[rows]
    start = rng.integers(0, m, lengths.size)
    step = 2 * rng.integers(0, max(1, m // 2), lengths.size) + 1
    col = 1 + (start[rows] + k * step[rows]) % m
    col = col[np.lexsort((col, rows))]
    val = (0.501 + 0.998 * rng.random(nnz)).astype(np.float32)
    return rowptr, col.astype(np.int32), val


def _classes_by_length(lengths, planted, long_row):
    lengths = torch.as_tensor(np.asarray(lengths))
    classes = {"hub rows": lengths > long_row, "empty rows": lengths == 0}
    for length in planted:
        classes[f"len {length}"] = lengths == length
    return classes


def _randn(g, *shape, scale=1.0, shift=0.0):
    return (shift + scale * torch.randn(*shape, generator=g)).float()


def _epilogue_params(g, d):
    return types.SimpleNamespace(bias=_randn(g, d, scale=0.5), g1=_randn(g, d, scale=0.3, shift=1.0),
                                 b1=_randn(g, d, scale=0.3), g2=_randn(g, d, scale=0.3, shift=1.0),
                                 b2=_randn(g, d, scale=0.3))


def _graph_case(d, lengths, planted, n_cols, seed, long_row):
    rowptr, col, val = planted_graph(lengths, n_cols, seed)
    g = torch.Generator().manual_seed(seed)
    n = len(lengths)
    c = _epilogue_params(g, d)
    c.d, c.n, c.n_cols, c.lengths, c.planted = d, n, n_cols, np.asarray(lengths), tuple(planted)
    c.rowptr, c.col, c.val = torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(val)
    c.h = _randn(g, n_cols, d)
    c.res = _randn(g, n, d)
    c.classes = _classes_by_length(lengths, planted, long_row)
    return c


def spmm_case(d, bf16=False):
    """(B) / (C): ``spmm_lengths`` planted, each once, among 300 rows of 0 .. 12 entries, in a seeded row order; a table
    of 1025 rows; the row block [37, n - 29) of the wrapper form."""
    planted = spmm_lengths(d, bf16)
    rng = np.random.default_rng(5000 + 2 * d + bf16)
    lengths = rng.permutation(np.concatenate([np.asarray(planted), rng.integers(0, 13, 300)]))
    c = _graph_case(d, lengths, planted, 1025, 5000 + 2 * d + bf16, LONG_ROW)
    c.lo, c.hi, c.bf16 = 37, c.n - 29, bf16
    if bf16:
        c.h = bf16_rne(c.h)
    return c


def spmm_trip_case(d, above):
    """(B) the grid-stride second trip: one trip of the capped grid + ``above`` rows of 0 .. 3 entries."""
    n = spmm_trip_rows(d) + above
    lengths = np.random.default_rng(7000 + d).integers(0, 4, n)
    c = _graph_case(d, lengths, (0, 1, 2, 3), 4097, 7000 + d, LONG_ROW)
    c.classes["second trip"] = torch.arange(n) >= spmm_trip_rows(d)
    return c


def parts_slice_lengths(d):
    g, ng = parts_shape(d)
    return sorted({1, g - 1, g + 1, g * ng, 255, 256})


def parts_case(d, n_parts, bf16p=False):
    """(D): entry ranges [e0, e1) of the planted lengths into one entry list of 4096 (they may overlap: a slice is a
    range, nothing more), starting anywhere -- so mid-row of whatever CSR the list belongs to -- and not aligned to
    anything; one slice: the longest, starting at entry 3."""
    rng = np.random.default_rng(9000 + d + n_parts)
    _, col, val = planted_graph([1024] * 4, 1025, 9000 + d)
    lens = np.asarray(parts_slice_lengths(d))
    length = lens[np.arange(n_parts) % lens.size] if n_parts > 1 else lens[-1:]
    e0 = rng.integers(0, col.size - 256, n_parts) if n_parts > 1 else np.asarray([3])
    g = torch.Generator().manual_seed(9000 + d)
    c = types.SimpleNamespace(d=d, n_parts=n_parts, col=torch.from_numpy(col), val=torch.from_numpy(val),
                              parts=torch.from_numpy(np.stack([e0, e0 + length], 1).astype(np.int64)),
                              h=_randn(g, 1025, d), length=length)
    if bf16p:
        c.h = bf16_rne(c.h)
    c.classes = {f"len {n}": torch.from_numpy(length == n) for n in lens}
    return c


def fused_case(d, bf16=False):
    """(E): ``fused_lengths`` planted, 65 twice -- five hub rows (> 64 entries), an odd number, so that in
    fused_row_order's own order the last hub shares a lane pair with the longest ordinary row --, among 300 rows of
    0 .. 12 entries; W [D, D] / sqrt(D); the row block [21, n - 14)."""
    planted = fused_lengths(d)
    rng = np.random.default_rng(11000 + 2 * d + bf16)
    lengths = rng.permutation(np.concatenate([np.asarray(planted + [65]), rng.integers(0, 13, 300)]))
    c = _graph_case(d, lengths, planted, 1025, 11000 + 2 * d + bf16, FUSED_LONG)
    g = torch.Generator().manual_seed(11001 + d)
    c.w = _randn(g, d, d, scale=d ** -0.5)
    c.lo, c.hi, c.bf16 = 21, c.n - 14, bf16
    if bf16:
        c.h = bf16_rne(c.h)
    return c


def fused_tiles_case(d, n_tiles):
    """(E) the tile counts: 16 n_tiles - 5 rows of 1 .. 3 entries (five -1 codes pad the last tile)."""
    n = 16 * n_tiles - 5
    lengths = np.random.default_rng(13000 + d + n_tiles).integers(1, 4, n)
    c = _graph_case(d, lengths, (1, 2, 3), 4097, 13000 + d, FUSED_LONG)
    g = torch.Generator().manual_seed(13001 + d)
    c.w = _randn(g, d, d, scale=d ** -0.5)
    c.lo, c.hi, c.bf16 = 0, n, False
    return c


def _pad16(codes):
    pad = (-codes.numel()) % 16
    return torch.cat([codes, torch.full((pad,), -1, dtype=codes.dtype)]) if pad else codes


def fused_orders(rowptr, lo, hi, pad_hubs, seed):
    """The three work orders of (E) -> ({name: int32 codes}, hubs, parts): ``fused_row_order``'s own; the ordinary rows
    by RISING degree behind the hubs (the shortest rows next to the hubs, the partners of a pair maximally unequal); a
    seeded shuffle of every code with seven -1 codes inside it.  ``pad_hubs``: the hub codes fill tiles of their own
    with -1 in all three (the bf16-table kernel wants that); the shuffle then permutes the hub tile and the rest apart."""
    from lpformer_amd import graph
    own, hubs, parts = graph.fused_row_order(rowptr, lo, hi, pad_hubs=pad_hubs)
    own = own.to(torch.int64)
    codes = own[own != -1]
    hub_codes, rows = codes[codes < -1], codes[codes >= 0]
    deg = rowptr[rows + 1] - rowptr[rows]
    rising = rows[torch.sort(deg, stable=True)[1]]
    hub_block = _pad16(hub_codes) if pad_hubs else hub_codes
    g = torch.Generator().manual_seed(seed)
    gaps = torch.full((7,), -1, dtype=torch.int64)
    if pad_hubs:
        body = torch.cat([rows, gaps])
        shuffled = torch.cat([hub_block[torch.randperm(hub_block.numel(), generator=g)],
                              body[torch.randperm(body.numel(), generator=g)]])
    else:
        body = torch.cat([codes, gaps])
        shuffled = body[torch.randperm(body.numel(), generator=g)]
    orders = {"own": own, "rising": _pad16(torch.cat([hub_block, rising])), "shuffled": _pad16(shuffled)}
    return {k: v.to(torch.int32).contiguous() for k, v in orders.items()}, hubs, parts


def with_dummy_slice(hubs, parts):
    """The same hub tables with an empty slice 0 in front that no hub names: row 0 of the slice sums is then free to
    hold anything, as row 0 of the gathered table is."""
    hubs = hubs.clone()
    hubs[:, 1] += 1
    return hubs, torch.cat([torch.zeros(1, 2, dtype=parts.dtype), parts])


def norm_case(n):
    """(A): n = 1: the diagonal alone, stored with weight 3.  Else rows of 0, 1 (the diagonal only), 63, 64, 65 and 700
    entries among rows of 0 .. 12; two rows in three (and the planted ones) hold their diagonal, stored with weight 3."""
    if n == 1:
        return types.SimpleNamespace(n=1, rowptr=torch.tensor([0, 1]), col=torch.zeros(1, dtype=torch.int32),
                                     val=torch.full((1,), 3.0), lengths=np.asarray([1]), diag_only=0,
                                     planted=(1,))
    planted = (0, 1, 63, 64, 65, 700)
    rng = np.random.default_rng(3000 + n)
    lengths = rng.integers(0, 13, n)
    at = rng.choice(n, len(planted), replace=False)
    lengths[at] = planted
    rowptr, col, val = planted_graph(lengths, n, 3000 + n)
    rows = np.repeat(np.arange(n), lengths)
    want = (np.arange(n) % 3 != 0) & (lengths > 0)
    want[at[1:]] = True
    has = np.zeros(n, bool)
    has[rows[col == rows]] = True
    put = want & ~has
    col = col.astype(np.int64)
    col[rowptr[:-1][put]] = np.nonzero(put)[0]              # the row's first entry becomes its diagonal
    order = np.lexsort((col, rows))
    col, val = col[order], val[order]
    assert np.unique(rows * n + col).size == col.size
    val[col == rows] = 3.0
    return types.SimpleNamespace(n=n, rowptr=torch.from_numpy(rowptr), col=torch.from_numpy(col.astype(np.int32)),
                                 val=torch.from_numpy(val), lengths=lengths, diag_only=int(at[1]), planted=planted)


def near_constant_row(d):
    """5 +- 3 / 2048 alternating (an odd D ends on 5): every partial sum of the row is exact in fp32, so its mean is 5
    and x - mean is exact -- var = 2.1e-6, rstd = 1 / sqrt(1.2e-5) = 287 --, while x^2 is not representable: a one-pass
    variance E[x^2] - mean^2 is off by a tenth of the variance."""
    s = torch.ones(d)
    s[1::2] = -1.0
    if d % 2:
        s[-1] = 0.0
    return (NC_BASE + NC_DELTA * s).float()


def ln_case(d, m, seed=0):
    """(F) LayerNorm: rows with a scale in [0.1, 10] and a mean in [-5, 5] (the training file's), rows 0, m // 2 and m - 1
    near constant from m = 4 on; gamma 1 + 0.1 randn, beta 0.1 randn."""
    g = torch.Generator().manual_seed(100003 * d + m + seed)
    scale = 10.0 ** (2 * torch.rand(m, 1, generator=g) - 1)
    mean = 10 * torch.rand(m, 1, generator=g) - 5
    x = (mean + scale * torch.randn(m, d, generator=g)).float()
    const = torch.zeros(m, dtype=torch.bool)
    if m >= 4:
        const[[0, m // 2, m - 1]] = True
        x[const] = near_constant_row(d)
    classes = {"near-constant rows": const, "other rows": ~const, "second trip": torch.arange(m) >= rowwise_trip_rows()}
    return types.SimpleNamespace(d=d, m=m, x=x, gamma=_randn(g, d, scale=0.1, shift=1.0), beta=_randn(g, d, scale=0.1),
                                 const=const, classes=classes)


GATHER_ROWS = 777
BAD_IDS = (-1, GATHER_ROWS, 2 ** 40)


def gather_case(d, m):
    """(F) endpoint gather: pairs of ids in [0, 777) with -1, 777 and 2^40 planted -- in the first row of ``batch`` at
    pairs 0 .. 2, in the second at the last three (one pair: (-1, 777))."""
    g = torch.Generator().manual_seed(200003 * d + m)
    x = _randn(g, GATHER_ROWS, d)
    batch = torch.randint(0, GATHER_ROWS, (2, m), generator=g)
    bad = torch.tensor(BAD_IDS)
    k = min(3, m)
    batch[0, :k] = bad[:k]
    batch[1, m - k:] = bad[3 - k:] if m >= 3 else bad[1:1 + k]
    out_of_range = ((batch < 0) | (batch >= GATHER_ROWS)).any(0)
    classes = {"ids out of range": out_of_range, "second trip": torch.arange(m) >= gather_trip_rows(d)}
    return types.SimpleNamespace(d=d, m=m, x=x, batch=batch, classes=classes)


def rowdot_case(k, m):
    """(F) dot + sigmoid: rows of randn, w randn, bias 0.3; from m = 5 on row 1 and row m - 3 are 100 w / |w|^2 and
    row 3 and row m - 2 its negative: logits 100.3 and -99.7, whose fp32 sigmoid is exactly 1 and 0."""
    g = torch.Generator().manual_seed(300003 * k + m)
    a, w = _randn(g, m, k), _randn(g, k)
    sat = torch.zeros(m)
    if m >= 5:
        unit = (100.0 * w.double() / (w.double() @ w.double())).float()
        for r, s in ((1, 1.0), (m - 3, 1.0), (3, -1.0), (m - 2, -1.0)):
            a[r], sat[r] = s * unit, s
    classes = {"saturating rows": sat != 0, "other rows": sat == 0, "second trip": torch.arange(m) >= rowwise_trip_rows()}
    return types.SimpleNamespace(k=k, m=m, a=a, w=w, bias=0.3, sat=sat, classes=classes)


# ------------------------------------------------------------------------------------------------ fp64 restatements
def _row_ids(rowptr):
    n = rowptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n, device=rowptr.device), rowptr[1:] - rowptr[:-1])


def gcn_norm64(rowptr, col, w):
    """lpf_gcn_norm_csr in fp64 -> (w_out, dis): a stored diagonal entry counts and is stored as 1 whatever its weight,
    ``w`` None = all ones, deg = the row's sum, dis = deg^-1/2 (0 for an empty row), w_out = (v dis[row]) dis[col]."""
    rows, c = _row_ids(rowptr), col.long()
    v = torch.ones(c.numel(), dtype=torch.float64, device=c.device) if w is None else w.double()
    v = torch.where(c == rows, torch.ones_like(v), v)
    deg = torch.zeros(rowptr.numel() - 1, dtype=torch.float64, device=c.device).index_add_(0, rows, v)
    dis = torch.where(deg > 0, deg.clamp_min(1e-300) ** -0.5, torch.zeros_like(deg))
    return v * dis[rows] * dis[c], dis


def spmm64(rowptr, col, val, h):
    """out[r] = sum over the stored entries e of row r of val[e] h[col[e]], fp64."""
    out = torch.zeros(rowptr.numel() - 1, h.shape[1], dtype=torch.float64, device=h.device)
    return out.index_add_(0, _row_ids(rowptr), h.double()[col.long()] * val.double()[:, None])


def layernorm64(x, gamma=None, beta=None, relu=False):
    """lpf_layernorm_f32 in fp64: biased variance from the centred row, eps 1e-5; gamma None: the rows unchanged."""
    y = x.double()
    if gamma is not None:
        c = y - y.mean(-1, keepdim=True)
        y = c / torch.sqrt((c * c).mean(-1, keepdim=True) + LN_EPS) * gamma.double() + beta.double()
    return y.clamp_min(0) if relu else y


def ln_cond_ratio(got, ref, x, gamma):
    """Worst |got - ref|_ij / (2^-24 max|x_i| rstd_i |gamma_j|) over the rows of a LayerNorm, [M] -> its maximum is what
    ``LN_COND_K`` bounds.  The derivation: fp32 gives the mean of a row with an error of a few 2^-24 max|x_i| however
    close together the row's values lie; x - mean inherits it whole, and the normalisation multiplies it by rstd_i
    gamma_j.  Three values drawn around a mean of up to 5 with a scale down to 0.1 can lie within 1e-3 of each other --
    rstd_i approaches 1 / sqrt(eps) = 316 --, and then 2^-24 x 5 x 316 = 9e-5 is several times 2e-5 max(1, max|ref|): no
    fp32 LayerNorm meets the forward tolerance on such a row (at D = 4 the training file meets the same rows).  From D = 63
    on a row of that many draws is never that close together."""
    x = x.double()
    c = x - x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt((c * c).mean(1, keepdim=True) + LN_EPS)
    unit = U32 * x.abs().amax(1, keepdim=True) * rstd * gamma.double().abs()
    return ((got.double() - ref).abs() / unit).amax(1)


def epilogue64(pre, bias=None, ln=None, relu=False, residual=None, ln2=None):
    """+ bias -> LayerNorm ``ln`` = (gamma, beta) -> ReLU -> + residual -> LayerNorm ``ln2``, fp64."""
    y = pre.double() if bias is None else pre.double() + bias.double()
    if ln is not None:
        y = layernorm64(y, *ln)
    if relu:
        y = y.clamp_min(0)
    if residual is not None:
        y = y + residual.double()
    return layernorm64(y, *ln2) if ln2 is not None else y


def fused_layer64(agg, w, bias=None, ln=None, relu=False, residual=None, ln2=None):
    """epilogue64((A H) W^T) from the aggregated rows ``agg`` = A H."""
    return epilogue64(agg.double() @ w.double().t(), bias, ln, relu, residual, ln2)


def row_parts64(parts, col, val, h):
    """out[p] = sum of val[e] h[col[e]] over e in [parts[p, 0], parts[p, 1]), from a running sum in fp64."""
    run = torch.cumsum(h.double()[col.long()] * val.double()[:, None], 0)
    run = torch.cat([torch.zeros_like(run[:1]), run])
    return run[parts[:, 1]] - run[parts[:, 0]]


def pair_gather64(x, batch, n_rows):
    """(x[a] x[b], x[a] + x[b]) with an id outside [0, n_rows) reading row 0."""
    ids = torch.where((batch < 0) | (batch >= n_rows), torch.zeros_like(batch), batch)
    xa, xb = x.double()[ids[0]], x.double()[ids[1]]
    return xa * xb, xa + xb


def rowdot64(a, w, bias):
    """(logit, sigmoid(logit)) of a w + bias."""
    s = a.double() @ w.double() + bias
    return s, torch.sigmoid(s)


def bf16_bits(x):
    """The bf16 image of an fp32 tensor (finite values), round to nearest even, as int32 in [0, 65536)."""
    u = x.float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).to(torch.int32)


def bf16_rne(x):
    """``x`` rounded to bf16 and back, fp32."""
    return (bf16_bits(x).to(torch.int64) << 16).to(torch.int32).view(torch.float32)


def bf16p_index(d):
    """src[e]: the feature that element e of gcn_fused.hip's permuted row holds: e = 32 i + 8 q + 4 h + u ->
    16 (2 i + h) + 4 q + u."""
    e = np.arange(d)
    i, q, h, u = e // 32, (e % 32) // 8, (e % 8) // 4, e % 4
    return torch.from_numpy(16 * (2 * i + h) + 4 * q + u)


def permute_bf16p(x):
    """Rows in normal feature order -> rows in the permuted order."""
    return x[:, bf16p_index(x.shape[1]).to(x.device)]


def unpermute_bf16p(xp):
    """The inverse of ``permute_bf16p``."""
    out = torch.empty_like(xp)
    out[:, bf16p_index(xp.shape[1]).to(xp.device)] = xp
    return out


# ------------------------------------------------------------------------------------------------ comparison
def compare(got, ref, classes=None, rel=FWD_TOL):
    """Worst |got - ref| / (rel max(1, max|ref|)) over the whole tensor ("all") and over each row class -- a bool mask
    over the rows -- with the class's own max|ref| -> {name: ratio}; an empty class gives 0, a non-finite element of
    ``got`` infinity.  Every element is in "all"."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    g = got.double()
    err = torch.where(torch.isfinite(g), (g - ref.double()).abs(), torch.full_like(g, float("inf")))

    def ratio(e, r):
        return float(e.max()) / (rel * max(1.0, float(r.abs().max()))) if e.numel() else 0.0
    out = {"all": ratio(err, ref)}
    for name, mask in (classes or {}).items():
        mask = mask.to(err.device)
        assert mask.dtype == torch.bool and mask.shape == err.shape[:1], name
        out[name] = ratio(err[mask], ref[mask])
    return out


def worst(ratios):
    name = max(ratios, key=ratios.get)
    return name, ratios[name]


def show(ratios):
    return " ".join(f"{k} {v:.4f}" for k, v in ratios.items() if v > 0 or k == "all")
