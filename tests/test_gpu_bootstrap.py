"""lpf_bootstrap_sums behind lpformer_amd.bootstrap on the MI355X: the kernel against the numpy restatement (integer
sums bit-equal, fp64 sums within P 2^-52 sum_j |x_j| computed from the restatement's own indices), its purity (chunks of
replicates, n_groups, repeats: bitwise), the front ends against the CPU path and the ABI's argument checks.

Sizes: the table lengths around the wavefront (64), the workgroup (256), an unrolled round (1,024) and, because one
segment of LPF_BOOTSTRAP_SEGMENT = 16,384 draws writes its result directly and more go through partial sums and a
second launch, both sides of that threshold; 200,003 rows make 13 segments with a short last one."""
import numpy as np
import pytest
import torch

from lpformer_amd import _lib
from lpformer_amd import bootstrap as B
from tests.bootstrap_cases import EPS, SEEDS, mrr_bound, np_indices, scores, sum_bound, tables

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

PS = (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 10_000)
BS = (1, 3, 64, 257)
COLS = ((1, 0), (0, 1), (3, 1), (8, 4))
# every P with a B, a column shape and a seed that rotate at different rates, then every (B, columns) pair once more on a
# P that walks through the list: 12 + 16 cases of the 576 in the product
CASES = [(p, BS[i % 4], COLS[(i + i // 4) % 4], SEEDS[i % 3]) for i, p in enumerate(PS)]
CASES += [(PS[(5 * i + 3) % 12], b, c, SEEDS[i % 3]) for i, (b, c) in enumerate((b, c) for b in BS for c in COLS)]
# the segment threshold: one segment, exactly one, one draw more, two and a bit; rows of 2 and 4 words too
CASES += [(B.SEGMENT - 1, 3, (3, 1), SEEDS[0]), (B.SEGMENT, 3, (2, 2), SEEDS[1]), (B.SEGMENT + 1, 3, (8, 4), SEEDS[2]),
          (2 * B.SEGMENT + 1, 64, (4, 0), SEEDS[0]), (200_003, 64, (3, 1), SEEDS[1])]


def _device(icols, fcols):
    return (torch.from_numpy(icols).to(DEV) if icols.shape[1] else None,
            torch.from_numpy(fcols).to(DEV) if fcols.shape[1] else None)


def _against_twin(p, b, ci, cf, seed, first=0, **kw):
    icols, fcols = tables(p, ci, cf, rng_seed=p % 1000 + ci)
    di, df = _device(icols, fcols)
    isum, fsum = B.bootstrap_sums(di, df, b, seed, first=first, **kw)
    assert isum.shape == (b, ci) and isum.dtype == torch.int64 and fsum.shape == (b, cf) and fsum.dtype == torch.float64
    isum, fsum = isum.cpu().numpy(), fsum.cpu().numpy()
    step = max(1, (1 << 21) // p)                       # the restatement's own indices, a few replicates at a time
    for r0 in range(0, b, step):
        idx = np_indices(p, min(step, b - r0), seed, first + r0)
        np.testing.assert_array_equal(isum[r0:r0 + step], icols[idx].sum(axis=1))
        if cf:
            err = np.abs(fsum[r0:r0 + step] - fcols[idx].sum(axis=1))
            bound = sum_bound(fcols, idx)
            assert (err <= bound).all(), (float((err / bound).max()), p, b)


@pytest.mark.parametrize("p,b,cols,seed", CASES)
def test_kernel_against_the_restatement(p, b, cols, seed):
    _against_twin(p, b, cols[0], cols[1], seed)


def test_rows_that_are_not_16_byte_aligned():
    p = 1000
    icols, fcols = tables(p, 2, 4)
    flat_i = torch.zeros(2 * p + 1, dtype=torch.int64, device=DEV)
    flat_f = torch.zeros(4 * p + 1, dtype=torch.float64, device=DEV)
    flat_i[1:] = torch.from_numpy(icols).to(DEV).reshape(-1)
    flat_f[1:] = torch.from_numpy(fcols).to(DEV).reshape(-1)
    off_i, off_f = flat_i[1:].view(p, 2), flat_f[1:].view(p, 4)
    assert off_i.data_ptr() % 16 == 8 and off_f.data_ptr() % 16 == 8
    a = B.bootstrap_sums(off_i, off_f, 5, 9)
    b = B.bootstrap_sums(*_device(icols, fcols), 5, 9)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])      # the same order of additions either way


# --------------------------------------------------------------------------------------------------------- purity
@pytest.mark.parametrize("p", (4097, 2 * B.SEGMENT + 1))
def test_chunks_groups_and_repeats_are_bitwise_equal(p):
    icols, fcols = tables(p, 3, 2)
    di, df = _device(icols, fcols)
    seed = SEEDS[1]
    whole = B.bootstrap_sums(di, df, 64, seed)
    again = B.bootstrap_sums(di, df, 64, seed)
    head, tail = B.bootstrap_sums(di, df, 20, seed), B.bootstrap_sums(di, df, 44, seed, first=20)
    for k in (0, 1):
        assert torch.equal(whole[k], again[k])
        assert torch.equal(whole[k], torch.cat([head[k], tail[k]]))
    for n_groups in (1, 3000):
        got = B.bootstrap_sums(di, df, 64, seed, n_groups=n_groups)
        assert torch.equal(whole[0], got[0]) and torch.equal(whole[1], got[1]), n_groups


def test_replicate_chunks_of_the_front_end(monkeypatch):
    p = 2 * B.SEGMENT + 5                               # three segments: the partial sums need a workspace
    icols, fcols = tables(p, 1, 1)
    di, df = _device(icols, fcols)
    whole = B.bootstrap_sums(di, df, 7, 1)
    monkeypatch.setattr(B, "_WORKSPACE_BYTES", 2 * 3 * 2 * 8)     # two replicates per call
    cut = B.bootstrap_sums(di, df, 7, 1)
    assert torch.equal(whole[0], cut[0]) and torch.equal(whole[1], cut[1])


# ------------------------------------------------------------------------------------------------------ front end
def _same(got, want, p, terms=1):
    """Integer-derived metrics exactly; MRR within the bound of a mean of p reciprocal ranks (each <= 1), once per system
    that enters the number (``terms``: 1, or 2 for a difference of two systems).  lo and hi interpolate two replicates,
    so they move by no more than a replicate does; a standard deviation moves by at most sqrt(B / (B - 1)) <= 2 times
    that."""
    assert got.keys() == want.keys()
    for name, w in want.items():
        g = got[name]
        if not isinstance(w, dict):
            assert g == w, name
            continue
        for field, wv in w.items():
            gv = g[field]
            if field == "replicates":
                gv, wv = gv.cpu(), wv.cpu()
                if name == "MRR" and terms == 1:
                    assert bool(((gv - wv).abs() <= p * EPS * wv.abs() + EPS).all())
                elif name == "MRR":
                    assert bool(((gv - wv).abs() <= terms * mrr_bound(p, 1.0)).all())
                else:
                    assert torch.equal(gv, wv), name
            elif isinstance(wv, float) and np.isnan(wv):
                assert np.isnan(gv), (name, field)
            elif name == "MRR" and field == "p":
                pass                                     # a difference that is 0 up to rounding may fall on either side
            elif name == "MRR":
                assert abs(gv - wv) <= (2 if field == "se" else 1) * terms * mrr_bound(p, 1.0), (name, field, gv, wv)
            else:
                assert gv == wv, (name, field, gv, wv)


@pytest.mark.parametrize("layout", ("shared", "rows"))
@pytest.mark.parametrize("with_unit", (False, True))
def test_front_ends_equal_the_cpu_path(layout, with_unit):
    p = 700
    pos, neg = scores(p, layout)
    pos_b = pos + torch.where(torch.arange(p) % 7 == 0, 1.5, 0.0)
    unit = (torch.arange(p) * 31) % 97 if with_unit else None
    dunit = unit.to(DEV) if with_unit else None
    kw = dict(k_list=(1, 5, 20), replicates=40, seed=SEEDS[2], return_replicates=True)
    got = B.bootstrap_metrics(pos.to(DEV), neg.to(DEV), unit=dunit, **kw)
    _same(got, B.bootstrap_metrics(pos, neg, unit=unit, **kw), p)
    got = B.compare_metrics(pos.to(DEV), neg.to(DEV), pos_b.to(DEV), neg.to(DEV), unit=dunit, **kw)
    _same(got, B.compare_metrics(pos, neg, pos_b, neg, unit=unit, **kw), p, terms=2)
    if not with_unit:
        values = torch.arange(p) % 9
        got = B.bootstrap_by_bin(pos.to(DEV), neg.to(DEV), values.to(DEV), **kw)
        want = B.bootstrap_by_bin(pos, neg, values, **kw)
        assert len(got) == len(want) == 4 and got[3]["count"] == 0
        for g, w in zip(got, want):
            assert g["bin"] == w["bin"] and g["count"] == w["count"]
            _same({k: v for k, v in g.items() if k not in ("bin", "count")},
                  {k: v for k, v in w.items() if k not in ("bin", "count")}, p)


# ------------------------------------------------------------------------------------------------------------ ABI
def test_invalid_arguments_return_the_error_code_without_a_launch():
    hip = _lib.hip()
    assert hip.lpf_abi_version() == 16
    p, b = 100, 4
    icols = torch.ones(p, 2, dtype=torch.int64, device=DEV)
    fcols = torch.ones(p, 1, dtype=torch.float64, device=DEV)
    isum = torch.full((b, 2), -7, dtype=torch.int64, device=DEV)
    fsum = torch.full((b, 1), -7.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    ok = dict(P=p, B=b, b0=0, seed=1, icols=icols.data_ptr(), Ci=2, fcols=fcols.data_ptr(), Cf=1, isum=isum.data_ptr(),
              fsum=fsum.data_ptr(), n_groups=0, ws=ws.data_ptr(), ws_bytes=ws.numel())

    def call(**change):
        a = dict(ok, **change)
        return hip.lpf_bootstrap_sums(a["P"], a["B"], a["b0"], a["seed"], a["icols"], a["Ci"], a["fcols"], a["Cf"],
                                      a["isum"], a["fsum"], a["n_groups"], a["ws"], a["ws_bytes"], stream)

    invalid = _lib.CONST["LPF_ERR_INVALID"]
    bad = [dict(P=0), dict(P=2 ** 31), dict(B=0), dict(B=-1), dict(b0=-1), dict(Ci=9), dict(Cf=9), dict(Ci=-1),
           dict(Ci=0, Cf=0), dict(n_groups=-1), dict(n_groups=65536), dict(icols=None), dict(fsum=None),
           dict(P=B.SEGMENT + 1, ws=None), dict(P=B.SEGMENT + 1, ws_bytes=8)]
    for change in bad:
        assert call(**change) == invalid, change
    torch.cuda.synchronize()
    assert bool((isum == -7).all()) and bool((fsum == -7.0).all())   # nothing ran
    for args in ((0, 1, 1, 1, 0), (2 ** 31, 1, 1, 1, 0), (10, 0, 1, 1, 0), (10, 1, 9, 0, 0), (10, 1, 0, 0, 0), (10, 1, 1, 1, -1)):
        assert hip.lpf_bootstrap_workspace_bytes(*args) == -1, args
    assert hip.lpf_bootstrap_workspace_bytes(B.SEGMENT, 1000, 8, 8, 0) == 0
    assert hip.lpf_bootstrap_workspace_bytes(B.SEGMENT + 1, 10, 3, 1, 7) == 10 * 2 * 4 * 8
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((isum == p).all()) and bool((fsum == float(p)).all())
