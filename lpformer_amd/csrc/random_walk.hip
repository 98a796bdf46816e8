// Biased random walks: lpf_random_walks, the node2vec second-order walk by rejection sampling, on a CSR
// with sorted, unique int32 columns and a SYMMETRIC pattern (the typing adjacency; values ignored; a stored self-loop
// is an entry like any other).  The contract is restated in include/lpformer_hip.h and in lpformer_amd/random_walks.py;
// the numpy restatement there equals this kernel integer for integer.
//
// The draw is draw_common.h's: key_w = key(seed, walk id), u(j) = mix64(key_w + G (j + 1)), node(u, d) = (u d) >> 64.
// Walk w (id walk_base + w) starts at starts[w]: walk[0] = start; a start outside [0, n) gives a row of -1 and a forced
// count of 0.  Step t = 1 .. L, cur = walk[t-1], d = stored entries of row cur:
//   d == 0: walk[t] = cur (the walk stays, as PyG pads);
//   else attempt a = 0, 1, ... draws the candidate x = col[rowptr[cur] + node(u(2 ((t-1) T + a)), d)].  It is taken
//   without a test when t == 1, d == 1 or second_order == 0 (p == q == 1).  Otherwise, with prev = walk[t-2], x is of
//   class RETURN (x == prev; this class wins over the next), COMMON (x stored in row prev: a binary search in a sorted
//   row) or OUT, and is accepted iff (u(2 ((t-1) T + a) + 1) >> 1) < thr[class].  After T refused attempts the last
//   candidate is taken and forced[w] is incremented.
// thr[class] = floor(2^63 weight / max weight) comes from the host, exact; the heaviest class has 2^63 and always accepts.
// A walk is a pure function of (seed, walk id, start, graph, L, thresholds, T): no floats, no atomics, no LDS, no lane
// reads another walk's state.  walks is STEP-MAJOR, walks[t * ldw + w]: with a lane per walk a wavefront stores one
// step as one contiguous line.
//
// A step is a chain of dependent gathers -- the candidate, the probes of row prev, then the bounds of the new row --
// and nothing in it can be requested ahead of the previous link, so the kernel lives on wavefronts in flight: no LDS,
// few registers, eight wavefronts per SIMD.  The bounds of rows cur and prev stay in registers across steps (a step
// reads one pair of row pointers, not two), and the probe of row prev is skipped where it cannot change the outcome
// (thr_common == thr_out, that is q == 1).
//
// Form LANE: one lane per walk.  Form GROUP8: eight lanes per walk; all eight make the same draws and read the same
// candidate (one broadcast line), and probe row prev eight keys a round: eight pivots cut the range in nine, a ballot
// over the group counts the pivots below x and picks the ninth that can still hold it -- a row of 600 entries takes 3
// rounds where the binary search takes 10.  Both forms give the same bits (tools/random_walks_time.py times them).
#include "lpf_common.h"
#include "draw_common.h"

namespace {

constexpr int RW_BLOCK = 256;
constexpr int RW_GROUP = 8;                     // lanes per walk of form GROUP8
constexpr uint64_t RW_ALWAYS = 1ull << 63;      // the threshold of the heaviest class

struct WalkArgs {
    int64_t n, nnz;
    const int64_t *rowptr;
    const int32_t *col;
    int64_t W;
    const int64_t *starts;
    uint64_t seed, walk_base;
    int32_t L, T, second_order;
    uint64_t thr_return, thr_common, thr_out;
    int32_t *walks;                             // [L + 1][ldw]
    int64_t ldw;
    int32_t *forced;                            // [W] or NULL
};

// the bounds of row v, clamped to [0, nnz] (a row pointer outside reads as an empty row)
__device__ __forceinline__ void rw_row(const WalkArgs &A, int32_t v, int64_t &r0, int64_t &r1) {
    const int64_t a = A.rowptr[v], b = A.rowptr[v + 1];
    r0 = a < 0 ? 0 : (a > A.nnz ? A.nnz : a);
    r1 = b < r0 ? r0 : (b > A.nnz ? A.nnz : b);
}

// whether the sorted row col[lo, hi) holds x, by the eight lanes of a group together: the same answer in all eight
__device__ __forceinline__ bool rw_group_has(const int32_t *__restrict__ col, int64_t lo, int64_t hi, int32_t x,
                                             int sub, int shift) {
    for (;;) {                                    // uniform over the group: lo, hi and x are
        const int64_t span = hi - lo;
        if (span <= RW_GROUP) {
            const bool eq = sub < span && col[lo + sub] == x;
            return ((__ballot(eq) >> shift) & 0xffull) != 0;
        }
        // pivot i = lo + span (i + 1) / 9, i = 0 .. 7: strictly increasing for span > 8, all inside [lo, hi)
        const int64_t piv = lo + span * (sub + 1) / (RW_GROUP + 1);
        const int32_t v = col[piv];
        const uint32_t eq = (uint32_t)(__ballot(v == x) >> shift) & 0xffu;
        if (eq) return true;
        const int below = __popc((uint32_t)(__ballot(v < x) >> shift) & 0xffu);   // pivots 0 .. below - 1 are < x
        const int64_t nlo = below == 0 ? lo : lo + span * below / (RW_GROUP + 1) + 1;
        const int64_t nhi = below == RW_GROUP ? hi : lo + span * (below + 1) / (RW_GROUP + 1);
        lo = nlo;
        hi = nhi;
        if (lo >= hi) return false;
    }
}

template <bool GROUP>
__global__ __launch_bounds__(RW_BLOCK) void random_walk_kernel(WalkArgs A) {
    const int64_t tid = (int64_t)blockIdx.x * RW_BLOCK + threadIdx.x;
    const int64_t w = GROUP ? tid / RW_GROUP : tid;
    const int sub = GROUP ? (int)(threadIdx.x & (RW_GROUP - 1)) : 0;
    const int shift = GROUP ? (lpf_lane() & ~(RW_GROUP - 1)) : 0;
    if (w >= A.W) return;                         // whole groups leave together
    const bool writer = sub == 0;
    int32_t *out = A.walks + w;
    const int64_t start = A.starts[w];
    if ((uint64_t)start >= (uint64_t)A.n) {
        if (writer) {
            for (int32_t t = 0; t <= A.L; ++t) out[(int64_t)t * A.ldw] = -1;
            if (A.forced) A.forced[w] = 0;
        }
        return;
    }
    const uint64_t key = lpf_draw_key(A.seed, A.walk_base + (uint64_t)w);
    const uint64_t T = (uint64_t)A.T;
    const bool probe = A.thr_common != A.thr_out;
    int32_t cur = (int32_t)start, prev = -1, forced = 0;
    int64_t c0, c1, p0 = 0, p1 = 0;
    rw_row(A, cur, c0, c1);
    if (writer) out[0] = cur;
    // ONE loop over (step, attempt), an attempt per trip: a lane whose candidate was refused tries again while its
    // neighbours move on to their next step, so a wavefront makes as many trips as its longest WALK has attempts, not
    // the sum over the steps of the longest attempt run among its 64 walks (attempts per step are geometric: at
    // (p, q) = (0.25, 4) the mean is about ten and the largest of 64 several times that).  Lanes then store different
    // steps in one trip; with p == q == 1 every trip is a step and the store is one line.
    int32_t t = 1;
    uint64_t a = 0;
    while (t <= A.L) {
        const uint64_t d = (uint64_t)(c1 - c0);
        int32_t x = cur;
        bool taken = true;
        if (d != 0) {
            const uint64_t j = 2ull * ((uint64_t)(t - 1) * T + a);
            x = A.col[c0 + (int64_t)__umul64hi(lpf_mix64(key + LPF_DRAW_G * (j + 1)), d)];
            if (!(t == 1 || d == 1 || !A.second_order)) {
                uint64_t thr = A.thr_return;
                if (x != prev) {
                    thr = A.thr_out;
                    if (probe) {
                        const bool has = GROUP ? rw_group_has(A.col, p0, p1, x, sub, shift)
                                               : lpf_sorted_has(A.col, p0, p1, x);
                        thr = has ? A.thr_common : A.thr_out;
                    }
                }
                taken = thr >= RW_ALWAYS || (lpf_mix64(key + LPF_DRAW_G * (j + 2)) >> 1) < thr;
                if (!taken && a + 1 == T) {
                    ++forced;
                    taken = true;
                }
            }
        }
        if (!taken) {
            ++a;
            continue;
        }
        if (writer) out[(int64_t)t * A.ldw] = x;
        prev = cur;
        p0 = c0;
        p1 = c1;
        if (x != cur) {                           // (a self-loop or an empty row: the bounds in hand are the row's)
            cur = x;
            // a column outside [0, n) is outside the contract; it reads as a node without entries, never out of bounds
            if ((uint64_t)(uint32_t)x < (uint64_t)A.n) rw_row(A, x, c0, c1);
            else c0 = c1 = 0;
        }
        ++t;
        a = 0;
    }
    if (writer && A.forced) A.forced[w] = forced;
}

}  // namespace

extern "C" int lpf_random_walks(int64_t n, int64_t nnz, const int64_t *rowptr, const int32_t *col, int64_t W,
                                const int64_t *starts, int64_t walk_base, int32_t L, uint64_t seed,
                                uint64_t thr_return, uint64_t thr_common, uint64_t thr_out, int32_t second_order,
                                int32_t max_tries, int32_t form, int32_t *walks, int64_t ldw, int32_t *forced,
                                void *stream) {
    LPF_REQUIRE(n >= 0 && n < INT32_MAX && nnz >= 0 && nnz < INT32_MAX && W >= 0 && W < INT32_MAX);
    LPF_REQUIRE(L >= 1 && L <= LPF_WALK_MAX_LENGTH && max_tries >= 1 && max_tries <= LPF_WALK_MAX_TRIES);
    LPF_REQUIRE(form == LPF_WALK_FORM_LANE || form == LPF_WALK_FORM_GROUP8);
    LPF_REQUIRE(second_order == 0 || second_order == 1);
    LPF_REQUIRE(thr_return <= RW_ALWAYS && thr_common <= RW_ALWAYS && thr_out <= RW_ALWAYS);
    if (W == 0 || n == 0) return LPF_OK;
    LPF_REQUIRE(rowptr && (col || nnz == 0) && starts && walks && ldw >= W);
    WalkArgs A{};
    A.n = n;
    A.nnz = nnz;
    A.rowptr = rowptr;
    A.col = col;
    A.W = W;
    A.starts = starts;
    A.seed = seed;
    A.walk_base = (uint64_t)walk_base;
    A.L = L;
    A.T = max_tries;
    A.second_order = second_order;
    A.thr_return = thr_return;
    A.thr_common = thr_common;
    A.thr_out = thr_out;
    A.walks = walks;
    A.ldw = ldw;
    A.forced = forced;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (form == LPF_WALK_FORM_GROUP8) {
        const int64_t grid = (W * RW_GROUP + RW_BLOCK - 1) / RW_BLOCK;      // < 2^31 / 32
        hipLaunchKernelGGL(random_walk_kernel<true>, dim3((unsigned)grid), dim3(RW_BLOCK), 0, s, A);
    } else {
        const int64_t grid = (W + RW_BLOCK - 1) / RW_BLOCK;
        hipLaunchKernelGGL(random_walk_kernel<false>, dim3((unsigned)grid), dim3(RW_BLOCK), 0, s, A);
    }
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}
