"""The bucket probe of ``select4_kernel`` (GPU box), pinned position by position.  A candidate's 64-byte bucket arrives as
four 16-byte pieces, and any form of the probe that shares a bucket among the four lanes of a quad (EXPERIMENTS.md: tried,
no gain on the collab-like step, not kept) can go wrong in ways the sampled batches of tests/test_gpu_select4.py do not
single out: a key found at some positions of a bucket only, a result kept by the wrong lane of the quad, a quad whose
lanes belong to different pairs, look only in part, or lie past the block's last slot.

The batches are BUILT for that from the model's own walk index, read back to the host: for the walk every pair has (the
shorter adjacency row, looked up in the other endpoint's hashed union row) the test computes bucket, position and
mini-filter verdict of every candidate the way the kernel does, and picks pairs until there is

* a looked-up key at each of the 8 positions of a FULL bucket (8 keys),
* an absent key that passes the mini filter (its bucket is read and says no) and one that does not (no read),
  both inside one walk -- quads in which only some lanes look,
* a union row of one bucket and one of 16 or more,
* a pair that starts at a slot that is no multiple of 4 -- a quad that spans two pairs,
* a block whose last round holds 1, 2 and 3 slots (one filler pair chosen by its slot count),
* a hub pair of more than 2,048 slots: a second batch of the workgroup at 512 threads.

Kept sets, PPR values and the pair table (``sel4_sets`` of tests/test_gpu_select4.py checks the table against the entries)
must be bit-exact against the oracle and against the type-major path (select3.hip), at launch shapes 0, 512 and 256.
"""
import numpy as np
import pytest
import torch

import lpformer_amd
from lpformer_amd import data as D
from lpformer_amd import graph as G
from oracle import lpformer_oracle as O
from tests.test_gpu_select4 import _assert_sets_equal, sel4_sets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = (0, 512, 256)
TAGS = ("cn", "onehop", "non1hop")
EMPTY = 2**31 - 1
N, HUB_A, HUB_B = 3000, 2300, 2200


def _bloom(v):
    h = (int(v) * G.BLOOM_MUL1) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * G.BLOOM_MUL2) & 0xFFFFFFFF
    return h ^ (h >> 13)


class Index:
    """Host copy of the walk index and the kernel's arithmetic on it (csrc/walk_common.h build_desc, bucket_of,
    mini_pass), mask mode "all"."""

    def __init__(self, wi):
        rec = wi.rec.cpu().numpy()
        r64 = rec.view(np.int64)
        self.adj0, self.u0 = r64[:, 0], r64[:, 4]
        self.deg, self.n_a1, self.n_px, self.n_t0, self.unb = (rec[:, 10 + i].astype(np.int64) for i in range(5))
        self.adj = wi.adj_cv.cpu().numpy()[:, 0]
        self.u = wi.u.cv.cpu().numpy()[:, 0]
        self.mini = wi.mini.cpu().numpy().view(np.uint32)
        self.use_px, self.has_t0 = bool(wi.use_px), wi.t0_cv is not None
        assert (self.u0 % G.HASH_BUCKET == 0).all()      # a bucket is an aligned 64-byte run of the index

    def slots(self, a, b):
        """Candidate slots of pair (a, b) -- and the pair owns at least one."""
        e, s, tot = (a, b), (0 if self.deg[a] <= self.deg[b] else 1), 0
        for k in (0, 1):
            me, other = e[k], e[1 - k]
            if k == s:
                tot += self.deg[me]
            elif self.use_px and self.n_px[other] < self.n_a1[me]:
                tot += self.n_px[other]
            else:
                tot += self.n_a1[me]
        if self.has_t0:
            tot += min(self.n_t0[a], self.n_t0[b])
        return max(int(tot), 1)

    def probes(self, a, b):
        """Tags of the look-ups of the pair's full-adjacency walk."""
        w, o = (a, b) if self.deg[a] <= self.deg[b] else (b, a)
        unb, tags, looks = int(self.unb[o]), set(), set()
        if unb == 0 or self.deg[w] == 0:
            return tags
        tags.add("one bucket" if unb == 1 else ("many buckets" if unb >= 16 else "few buckets"))
        for x in self.adj[self.adj0[w]: self.adj0[w] + self.deg[w]]:
            x = int(x)
            mh = _bloom(x ^ G.MINI_SALT)
            mw = int(self.mini[o, mh >> 27])
            look = (mw >> (mh & 31)) & (mw >> ((mh >> 5) & 31)) & 1
            bk = (((x * G.HASH_MUL) & 0xFFFFFFFF) * unb) >> 32
            keys = self.u[self.u0[o] + 8 * bk: self.u0[o] + 8 * bk + 8]
            hit = np.flatnonzero(keys == x)
            assert hit.size <= 1 and (look or hit.size == 0)   # (a key stands once in a row; the filter has no false "no")
            looks.add(bool(look))
            if hit.size:
                if (keys != EMPTY).sum() == 8:
                    tags.add(("full bucket", int(hit[0])))
            else:
                tags.add("absent, read" if look else "absent, not read")
        if looks == {True, False}:
            tags.add("some lanes look")
        return tags


WANTED = {("full bucket", p) for p in range(8)} | {"absent, read", "absent, not read", "some lanes look", "one bucket",
                                                   "many buckets"}


class Case:
    def __init__(self):
        rng = np.random.default_rng(11)
        ei, _ = D.chung_lu_graph(N, 14000, gamma=2.1, seed=11, max_weight=0)
        star = np.concatenate([np.stack([np.zeros(HUB_A, np.int64), rng.choice(np.arange(2, N), HUB_A, replace=False)]),
                               np.stack([np.ones(HUB_B, np.int64), rng.choice(np.arange(2, N), HUB_B, replace=False)])], 1)
        allp = np.concatenate([ei, star, star[::-1]], axis=1)
        _, keep = np.unique(allp[0] * N + allp[1], return_index=True)
        self.ei = ei = allp[:, keep]
        x = rng.standard_normal((N, 16)).astype(np.float32)
        self.ppr = lpformer_amd.calc_ppr(ei, N, 0.15, 1e-4)
        self.cfg = D.train_args_for(dict(thresholds=(0.0, 1e-4, 1e-2), dim=64, gnn_layers=1, residual=False))
        torch.manual_seed(0)
        self.model = lpformer_amd.LinkTransformer(self.cfg, D.build_data(ei, x, N, ppr=self.ppr), device=DEV).to(DEV).eval()
        with torch.cuda.device(self.model.device):
            self.ix = Index(self.model._select_graphs(False, None))
        self.pool = np.concatenate([D.sample_pairs(ei, N, 1500, seed=5), ei[:, rng.choice(ei.shape[1], 500, replace=False)]], 1)
        self.pool = self.pool[:, (self.pool >= 2).all(axis=0)]         # (the hubs have a batch of their own)
        # (union rows of a single bucket are rare among sampled pairs: leaves walked against such a row go in front)
        ones, leaf = np.flatnonzero((self.ix.unb == 1) & (self.ix.deg >= 1))[:4], np.flatnonzero(self.ix.deg == 1)
        front = [(int(w), int(o)) for w, o in zip(leaf[-4:], ones) if w != o]
        self.pool = np.concatenate([np.array(front, dtype=np.int64).reshape(-1, 2).T, self.pool], axis=1)

    def cover(self):
        """Pairs of the pool until every wanted tag has been seen, each pair adding one; then a pair behind one whose
        slots are no multiple of 4."""
        have, batch = set(), []
        for a, b in self.pool.T:
            new = (self.ix.probes(int(a), int(b)) & WANTED) - have
            if new:
                have |= new
                batch.append((int(a), int(b)))
            if have == WANTED:
                break
        assert have == WANTED, f"the pool does not exercise {WANTED - have}"
        starts = np.cumsum([0] + [self.ix.slots(a, b) for a, b in batch])[:-1]
        if not (starts % 4 != 0).any():
            odd = next((int(a), int(b)) for a, b in self.pool.T if self.ix.slots(int(a), int(b)) % 4)
            batch.insert(0, odd)
        assert len(batch) < 60
        return batch

    def with_last_round(self, batch, fill):
        """``batch`` + one pair of the pool whose slots leave ``fill`` slots in the block's last round of 64."""
        have = sum(self.ix.slots(a, b) for a, b in batch)
        for a, b in self.pool.T:
            if (have + self.ix.slots(int(a), int(b))) % 64 == fill:
                return batch + [(int(a), int(b))]
        raise AssertionError(f"no pair of the pool leaves {fill} slots")

    def check(self, batch):
        arr = np.array(batch, dtype=np.int64).T.copy()
        bt = torch.from_numpy(arr)
        ref = O.select_nodes(arr, O.symmetric_mask_csr(self.ei, N), (self.ppr.rowptr, self.ppr.col.astype(np.int64), self.ppr.val),
                             (self.cfg["thresh_cn"], self.cfg["thresh_1hop"], self.cfg["thresh_non1hop"]), n=N)
        self.model.select4_regions = False                             # the type-major path: select3.hip + export
        major = {t: tuple(v.cpu().numpy() for v in i) for t, i in zip(TAGS, self.model.compute_node_mask(bt))}
        _assert_sets_equal(major, ref, TAGS)
        slots = sum(self.ix.slots(a, b) for a, b in batch)
        for threads in SHAPES:
            got, ws = sel4_sets(self.model, bt, threads=threads)
            _assert_sets_equal(got, ref, TAGS)
            _assert_sets_equal(got, major, TAGS)
            if len(batch) <= 64:     # (one block: the kernel reports its candidate slots, rounded to 8 -- the test's count is the kernel's)
                assert int(ws.ctl[1].item()) == (slots + 7) // 8 * 8, (int(ws.ctl[1].item()), slots)
        return ref


@pytest.fixture(scope="module")
def case():
    return Case()


def test_every_position_of_a_bucket_and_partly_looking_quads(case):
    batch = case.cover()
    ref = case.check(batch)
    assert ref["cn"][0].shape[1] > 0 and ref["onehop"][0].shape[1] > 0


@pytest.mark.parametrize("fill", [1, 2, 3])
def test_last_round_of_one_two_three_slots(case, fill):
    batch = case.with_last_round(case.cover(), fill)
    assert sum(case.ix.slots(a, b) for a, b in batch) % 64 == fill and len(batch) <= 64
    case.check(batch)


def test_hub_pair_takes_a_second_batch(case):
    batch = [(0, 1), (5, 9), (1, 0), (0, 0)] + case.cover()[:3]
    assert case.ix.slots(0, 1) > 2048
    ref = case.check(batch)
    assert (ref["cn"][0][0] == 0).sum() > 0
