"""The references of tests/train_kernel_reference.py checked on the CPU, so that the GPU tests compare the training
kernels with something that is itself pinned: the fp64 restatements differentiate correctly (``gradcheck``), the
generalised attention restatement still gives the numbers of the expression it replaced, and the sequential float32
segment sum stays within the textbook bound of an fp64 sum."""
import numpy as np
import torch

from tests import train_kernel_reference as R

KINK_MARGIN = 1e-3      # no ReLU / leaky-ReLU argument this close to 0: gradcheck's central differences (eps 1e-6) stay
                        # on one side of every kink with room to spare


def _attention_case(seed, bs=7, d=8, dh=4, n_t=3, n_nodes=5):
    """A tiny batch in fp64: pair 2 has no entry at all, pair 4 exactly one."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 4, (n_t, bs))
    counts[:, 2] = 0
    counts[:, 4] = 0
    counts[1, 4] = 1
    counts[0, 0] = max(int(counts[0, 0]), 2)
    seg, tbase, n = R.layout(counts)
    g = torch.Generator().manual_seed(seed)
    mk = lambda *shape, s=1.0: s * torch.randn(*shape, dtype=torch.float64, generator=g)
    params = [mk(n_nodes, d), mk(bs, d), mk(d, s=0.3), mk(d, s=0.1), mk(n_t, d, dh, s=dh ** -0.5), mk(n_t, d, s=0.1),
              mk(n_t, dh, 2, s=3.0), mk(n_t, dh, s=0.2), 1 + 0.1 * mk(n_t, dh), mk(n_t, dh, s=0.1)]
    e_node = torch.from_numpy(rng.integers(0, n_nodes, n))
    e_pa, e_pb = (torch.from_numpy(rng.random(n) * 0.05) for _ in range(2))
    return params, (e_node, e_pa, e_pb, R.pair_of_entries(seg), tbase), (seg, counts, n)


def _kink_distance(params, rest):
    """Smallest |argument| over every ReLU of the hidden layer and every leaky ReLU of the score."""
    e_node, e_pa, e_pb, pair, tbase = rest
    w1s, b1s, gams, bets = params[6:]
    worst = float("inf")
    for t in range(w1s.shape[0]):
        lo, hi = tbase[t], tbase[t + 1]
        if hi > lo:
            _, a1, a2 = R.pe_hidden64(w1s[t], b1s[t], gams[t], bets[t], e_pa[lo:hi], e_pb[lo:hi], relu_args=True)
            worst = min(worst, float(a1.abs().min()), float(a2.abs().min()))
    _, _, x = R.attention64(*params, *rest, detail=True)
    return min(worst, float(x.abs().min()))


def _seed_away_from_kinks():
    for seed in range(200):
        params, rest, info = _attention_case(seed)
        if _kink_distance(params, rest) >= KINK_MARGIN:
            return seed, params, rest, info
    raise AssertionError("no seed below 200 keeps every ReLU argument away from 0")


def test_attention_restatement_passes_gradcheck():
    seed, params, rest, (seg, counts, n) = _seed_away_from_kinks()
    assert _kink_distance(params, rest) >= KINK_MARGIN
    assert counts[:, 2].sum() == 0 and counts[:, 4].sum() == 1 and n > 10, (seed, counts)
    params = [p.clone().requires_grad_() for p in params]
    out = R.attention64(*params, *rest)
    assert out.shape == (7, 8) and torch.equal(out[2].detach(), params[3].detach())     # the empty pair: the bias
    assert torch.autograd.gradcheck(lambda *p: R.attention64(*p, *rest), params)


def test_pe_hidden_restatement_passes_gradcheck():
    for seed in range(200):
        g = torch.Generator().manual_seed(seed)
        mk = lambda *shape, s=1.0: s * torch.randn(*shape, dtype=torch.float64, generator=g)
        w1, b1, gam, bet = mk(4, 2, s=3.0), mk(4, s=0.2), 1 + 0.1 * mk(4), mk(4, s=0.1)
        pa = 0.05 * torch.rand(6, dtype=torch.float64, generator=g)
        pb = 0.05 * torch.rand(6, dtype=torch.float64, generator=g)
        pb[3] = pa[3]                                                   # both orders the same row
        _, a1, a2 = R.pe_hidden64(w1, b1, gam, bet, pa, pb, relu_args=True)
        if min(float(a1.abs().min()), float(a2.abs().min())) >= KINK_MARGIN:
            break
    else:
        raise AssertionError("no seed below 200 keeps every ReLU argument away from 0")
    assert min(float(a1.abs().min()), float(a2.abs().min())) >= KINK_MARGIN
    args = [t.clone().requires_grad_() for t in (w1, b1, gam, bet)]
    assert torch.autograd.gradcheck(lambda *p: R.pe_hidden64(*p, pa, pb), args)


def test_attention_restatement_reproduces_the_inline_expression_it_replaced():
    """d == dh: the restatement (one product per type) against the expression test_gpu_train.py carried inline (a
    gathered [n, D, D] weight per entry), same inputs, to 1e-12."""
    params, rest, (seg, counts, n) = _attention_case(11, bs=23, d=8, dh=8, n_nodes=9)
    e_node, e_pa, e_pb, pair_t, tbase = rest
    z_, q_, att_, bias_, wf_, bf_, w1_, b1_, g_, be_ = params
    bs, dim, n_t = 23, 8, 3
    new = R.attention64(*params, *rest)
    # ---- the old inline code, verbatim but for the device
    pair_of = np.zeros(n, np.int64)
    type_of = np.zeros(n, np.int64)
    for t in range(n_t):
        for p in range(bs):
            pair_of[seg[t, p]:seg[t, p + 1]] = p
        type_of[tbase[t]:tbase[t + 1]] = t
    assert np.array_equal(pair_of, pair_t.numpy())
    type_t = torch.from_numpy(type_of)
    pa, pb = e_pa.double(), e_pb.double()

    def hidden(x, y):
        u = x[:, None] * w1_[type_t][:, :, 0] + y[:, None] * w1_[type_t][:, :, 1] + b1_[type_t]
        mu, var = u.mean(1, keepdim=True), u.var(1, unbiased=False, keepdim=True)
        return torch.relu((u - mu) / torch.sqrt(var + 1e-5) * g_[type_t] + be_[type_t])
    h = hidden(pa, pb) + hidden(pb, pa)
    kp = torch.einsum("ed,eod->eo", h, wf_[type_t]) + bf_[type_t]
    k = z_[e_node.long()] + kp
    s = (torch.nn.functional.leaky_relu(k * q_[pair_t], 0.2) * att_).sum(1)
    smax = torch.full((bs,), -float("inf"), dtype=torch.float64).scatter_reduce(0, pair_t, s.detach(), "amax")
    w = torch.exp(s - smax[pair_t])
    den = torch.zeros(bs, dtype=torch.float64).index_add(0, pair_t, w) + 1e-16
    old = torch.zeros(bs, dim, dtype=torch.float64).index_add(0, pair_t, (w / den[pair_t])[:, None] * k) + bias_
    # ----
    assert float(old.abs().max()) > 0.1
    assert float((new - old).abs().max()) <= 1e-12


def test_score_ranges_and_pair_gather():
    s = torch.tensor([1.0, 4.0, -2.0, 7.0], dtype=torch.float64)
    pair = torch.tensor([0, 0, 0, 2])
    assert R.score_ranges(s, pair, 3).tolist() == [6.0, 0.0, 0.0]
    x = torch.arange(12, dtype=torch.float64).reshape(4, 3)
    batch = torch.tensor([[0, 3, 2], [1, 3, 0]])
    assert torch.equal(R.pair_gather64(x, batch, True), x[[0, 3, 2]] * x[[1, 3, 0]])
    assert torch.equal(R.pair_gather64(x, batch, False), x[[0, 3, 2]] + x[[1, 3, 0]])


def test_segment_sum_seq32_within_the_sequential_summation_bound():
    """Runs of 1, 2, 3, 4, 5, 8 and 4001 rows: |seq32 - fp64| <= run length x 2^-24 x sum |rows| per run and column (the
    first-order bound of recursive summation, Higham 4.2: (m - 1) u sum|x_i| with u = 2^-24), on keys that skip rows."""
    rng = np.random.default_rng(5)
    lengths = [1, 2, 3, 4, 5, 8, 4001, 1]
    key_vals = [0, 3, 4, 9, 10, 12, 17, 40]
    keys = np.repeat(np.asarray(key_vals, np.int32), lengths)
    n, d = keys.size, 8
    order = rng.permutation(n).astype(np.int64)
    src = rng.standard_normal((n, d)).astype(np.float32)
    got_keys, got = R.segment_sum_seq32(keys, order, src)
    assert got.dtype == np.float32 and got_keys.tolist() == key_vals
    rows = torch.from_numpy(src[order]).double()
    idx = torch.from_numpy(np.repeat(np.arange(len(lengths)), lengths))
    want = torch.zeros(len(lengths), d, dtype=torch.float64).index_add(0, idx, rows).numpy()
    mag = torch.zeros(len(lengths), d, dtype=torch.float64).index_add(0, idx, rows.abs()).numpy()
    bound = np.asarray(lengths, np.float64)[:, None] * 2.0 ** -24 * mag
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), float((err / bound).max())
    assert np.array_equal(got[0], src[order[0]]) and np.array_equal(got[7], src[order[n - 1]])    # a run of one: the row
    assert float(err[6].max()) > 0          # (the long run does round: the check is not of an exact sum)
    ek, es = R.segment_sum_seq32(np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros((0, d), np.float32))
    assert ek.shape == (0,) and es.shape == (0, d)
