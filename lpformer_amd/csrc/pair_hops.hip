// Nodes by distance to both endpoints of a pair, on the typing adjacency (the exact structure counts ELPH / BUDDY
// estimate with sketches: A[d_a, d_b] and B[d]): for each pair (a, b) of a binary CSR with sorted, unique int32 columns
// and a SYMMETRIC pattern (values ignored; a non-symmetric pattern is outside the contract) and hops = k in {1, 2}
//   cls_u(v) = d(u, v) if that is <= k, else k + 1 (farther than k, or unreachable)
//   T[i][j]  = |{v in [0, n) : cls_a(v) = i and cls_b(v) = j}|,   int32 [k + 2][k + 2], far/far included: sum = n.
// a == b is no special case (a diagonal table); stored self-loops change nothing; an id outside [0, n) gives an
// all-zero table.  ignore_direct: for THIS pair the stored entries (a, b) and (b, a) count as absent when distances
// are taken.
//
// pair_walks.hip's skeleton.  The caller hands the pairs over oriented and sorted: row 0 holds a pair's SPREAD endpoint
// s, row 1 its WALK endpoint t, and unit_ptr cuts the list into units, runs of pairs with the same s; the table written
// is T[class of s][class of t] (the caller transposes where it spread b).  Persistent 256-thread workgroups take units
// by an atomic ticket.  Each workgroup owns two dense arrays over all n nodes in the caller's workspace, one 32-bit
// word per node each: the high 30 bits an epoch stamp, the low 2 bits the payload k + 1 - d (1 .. k + 1; 0 never
// occurs in a stamped word).  Nothing is cleared between units or pairs: the S array's epoch grows by one per unit,
// the T array's by one per pair; the entry point zeroes both once per call and epochs start at 1.
// EPOCH WIDTH: 30 bits.  A workgroup takes at most m units and expands at most m pairs, so m < 2^30 keeps every epoch
// below 2^30; the entry point requires it.
//   * spread s, k hops, into the S array: one unsigned atomic max per touch with (epoch << 2) | (k + 1 - d), d the
//     length of the walk that reached the node (s itself: d = 0).  A word of an older epoch is smaller than every word
//     of this one, and within the epoch the larger payload is the smaller distance, so the word ends at the node's
//     smallest distance in whatever order the touches land: the spread has no level barrier.  Class sizes of s: class 0
//     is s; class 1 is the row of s without the self-loop and the skipped entry (columns are unique: counted as read);
//     |B_k(s)| is the number of FIRST touches of the epoch -- the atomic returns the old word, and of the touches of
//     one node exactly one finds a word of an older epoch, whichever it is; class 2 is the rest.
//   * then, per pair of the unit, expand t by k hops into the T array under the pair's own epoch, a wave per w in N(t),
//     its lanes over N(w).  Every touch is one atomic max that returns the old word, and the lane that RAISED the word
//     (old < new) adds 1 to the tally of (class of s, new class of t) and, where the old word was already of this
//     epoch, subtracts 1 from the tally of (class of s, old class of t).
//     ORDER-INDEPENDENCE.  The read-modify-writes on one word are totally ordered, and the raising ones among them form
//     a strictly increasing chain w_1 < w_2 < ... < w_r within the epoch that ends at the largest word any touch of the
//     node carries, i.e. at its smallest distance, whatever the order (which touches are the raising ones does depend
//     on the order; the end of the chain does not).  Raise i adds +1 at class(w_i) and -1 at class(w_{i-1}) (nothing
//     for i = 1), so the node's contributions telescope to exactly +1 at class(w_r), its final class, and every other
//     cell gets 0 from it.  Integer adds commute, so the reduced tallies do not depend on which lane held which part.
//     The class of s of the node is read from the S array, which does not change during the expansion.  No second
//     pass, no claim bit and no barrier inside the expansion.  The class sizes of t are counted like those of s: the
//     row of t, and the first touches of the pair's epoch.
//   * T[i][k + 1] = |class i of s| - sum_j T[i][j], T[k + 1][j] = |class j of t| - sum_i T[i][j] (i, j <= k), and the
//     far/far cell follows from n.  Tallies are per-lane int32 registers, reduced over the workgroup (shuffles, then
//     LDS); one lane stores the (k + 2)^2 cells with plain stores.  Cost per pair: E2(t) touches (deg(t) for k = 1).
// ignore_direct: the kernel skips the transitions {s, t} -- in the spread and in the expansion -- in units of ONE pair
// only; the caller makes every pair that is a stored entry a unit of its own (a pair that is no entry has no such
// transition, so skipping changes nothing for it, and it keeps sharing its spread).
//
// Between the spread and the expansion the lanes of a workgroup exchange GLOBAL data.  The spread writes with atomics
// only, which execute in L2; every wave then drains its own (release fence at agent scope and an explicit wait for its
// outstanding memory operations) before a workgroup barrier, and the expansion reads the S words with relaxed
// agent-scope atomic loads, which are served from L2 and not from a vector L1 line an earlier unit left behind.  The T
// array is only ever touched by returning atomics, and a pair's tallies consume every returned word before the barriers
// of its reduction, as they consume the S loads: neither the next pair's expansion nor the next unit's spread can
// overtake them.
//
// Deterministic: integers only, no floats; a table is a pure function of (graph, pair, options) -- not of the pair's
// position, the units, the number of workgroups or timing; (t, s) gives the transposed table.
#include "lpf_common.h"

namespace {

constexpr int HP_BLOCK = 256;                   // 4 wavefronts
constexpr int HP_WAVES = HP_BLOCK / LPF_WAVE;
constexpr int64_t HP_HEADER = 16;               // bytes in front of the state: the unit ticket
constexpr int HP_BITS = 2;                      // payload bits under the epoch stamp
constexpr int64_t HP_MAX_PAIRS = (int64_t)1 << (32 - HP_BITS);   // epochs stay below 2^30

struct HopArgs {
    int64_t m, n;
    const int64_t *pairs;
    int64_t ld;
    const int64_t *rowptr;
    const int32_t *col;
    int32_t ignore_direct;
    const int32_t *unit_ptr;                    // [m + 1]
    int32_t *ticket;
    uint32_t *state;                            // [n_groups][2][n]: the S array, then the T array
    int32_t *out;                               // [m][(k + 2)^2]
};

__device__ __forceinline__ int32_t hp_wave_sum(int32_t v) {
#pragma unroll
    for (int d = LPF_WAVE >> 1; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

template <int K>
__global__ __launch_bounds__(HP_BLOCK) void pair_hops_kernel(HopArgs A) {
    constexpr int C = K + 1;                    // near classes 0 .. K
    constexpr int NC = C * C;                   // tallied cells
    constexpr int NV = NC + 2;                  // + |class 1 of t|, first touches of t
    constexpr int D = K + 2;
    __shared__ int32_t s_part[HP_WAVES][NV];
    __shared__ int32_t s_spread[HP_WAVES][2];   // per wave: |class 1 of s|, first touches of s
    __shared__ int32_t s_ticket;
    const int tid = threadIdx.x, lane = lpf_lane(), wave = tid >> 6;
    const int64_t n = A.n, m = A.m;
    const int64_t *__restrict__ rowptr = A.rowptr;
    const int32_t *__restrict__ col = A.col;
    uint32_t *ss = A.state + (int64_t)blockIdx.x * 2 * n;
    uint32_t *tt = ss + n;
    uint32_t epoch_s = 0, epoch_t = 0;            // the state is zeroed before the launch
    for (;;) {
        if (tid == 0) s_ticket = atomicAdd(A.ticket, 1);
        __syncthreads();
        const int64_t u = s_ticket;
        __syncthreads();                          // s_ticket is rewritten by the next unit
        if (u < 0 || u >= m) break;               // block-uniform
        const int64_t lo = A.unit_ptr[u], hi = A.unit_ptr[u + 1];
        if (lo < 0 || lo >= m) break;             // past the last unit
        if (hi <= lo || hi > m) continue;         // (a malformed unit: nothing is written for it)
        ++epoch_s;                                // (at most m < 2^30 units per launch)
        const uint32_t stamp_s = epoch_s << HP_BITS;
        const int64_t s = A.pairs[lo];
        const bool s_ok = (uint64_t)s < (uint64_t)n;
        // one-pair units skip the transitions {s, t0}; -1 matches no column
        const int64_t t_only = A.pairs[A.ld + lo];
        const bool own = A.ignore_direct && hi - lo == 1 && s_ok && (uint64_t)t_only < (uint64_t)n;
        const int32_t ks = own ? (int32_t)s : -1, kt = own ? (int32_t)t_only : -1;
#define HP_SKIP(x, y) (own && (((x) == ks && (y) == kt) || ((x) == kt && (y) == ks)))
        int32_t c1s = 0, fts = 0;
        if (s_ok) {
#define HP_SPREAD(v, d)                                                             \
    do {                                                                            \
        const uint32_t old__ = atomicMax(&ss[v], stamp_s | (uint32_t)(C - (d)));    \
        fts += (old__ >> HP_BITS) != epoch_s;                                       \
    } while (0)
            if (tid == 0) HP_SPREAD(s, 0);
            const int64_t s0 = rowptr[s], s1 = rowptr[s + 1];
            if (K == 1) {
                for (int64_t j = s0 + tid; j < s1; j += HP_BLOCK) {
                    const int32_t c = col[j];
                    if ((uint64_t)c >= (uint64_t)n || HP_SKIP((int32_t)s, c)) continue;
                    c1s += c != (int32_t)s;
                    HP_SPREAD(c, 1);
                }
            } else {
                for (int64_t j = s0 + wave; j < s1; j += HP_WAVES) {     // wave-uniform
                    const int32_t w = col[j];
                    if ((uint64_t)w >= (uint64_t)n || HP_SKIP((int32_t)s, w)) continue;
                    if (lane == 0) {
                        c1s += w != (int32_t)s;
                        HP_SPREAD(w, 1);
                    }
                    const int64_t w1 = rowptr[w + 1];
                    for (int64_t k = rowptr[w] + lane; k < w1; k += LPF_WAVE) {
                        const int32_t c = col[k];
                        if ((uint64_t)c < (uint64_t)n && !HP_SKIP(w, c)) HP_SPREAD(c, 2);
                    }
                }
            }
#undef HP_SPREAD
        }
        c1s = hp_wave_sum(c1s);
        fts = hp_wave_sum(fts);
        if (lane == 0) {
            s_spread[wave][0] = c1s;
            s_spread[wave][1] = fts;
        }
        // every wave's atomics have executed before any wave reads the state
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int64_t sz_s[C] = {};                   // class sizes of s (used by thread 0)
        if (tid == 0 && s_ok) {
            int32_t c1 = 0, ft = 0;
#pragma unroll
            for (int q = 0; q < HP_WAVES; ++q) {
                c1 += s_spread[q][0];
                ft += s_spread[q][1];
            }
            sz_s[0] = 1;
            sz_s[1] = c1;
            if (K == 2) sz_s[C - 1] = (int64_t)ft - 1 - c1;
        }
        for (int64_t p = lo; p < hi; ++p) {       // block-uniform
            const int64_t t = A.pairs[A.ld + p];
            const bool ok = s_ok && (uint64_t)t < (uint64_t)n;
            int32_t cnt[NC];
#pragma unroll
            for (int q = 0; q < NC; ++q) cnt[q] = 0;
            int32_t c1t = 0, ftt = 0;
            if (ok) {
                ++epoch_t;                        // (at most m < 2^30 pairs per launch)
                const uint32_t stamp_t = epoch_t << HP_BITS;
                // one touch of the expansion: node v reached by a walk of d entries from t
#define HP_EXPAND(v, d)                                                                                         \
    do {                                                                                                        \
        const uint32_t new__ = stamp_t | (uint32_t)(C - (d));                                                   \
        const uint32_t sw__ = __hip_atomic_load(&ss[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);            \
        const uint32_t old__ = atomicMax(&tt[v], new__);                                                        \
        if (old__ < new__) {                                                                                    \
            const bool in__ = (old__ >> HP_BITS) == epoch_t;                                                    \
            ftt += !in__;                                                                                       \
            if ((sw__ >> HP_BITS) == epoch_s) {                                                                 \
                const int row__ = (C - (int)(sw__ & 3u)) * C;                                                   \
                const int add__ = row__ + (d), sub__ = in__ ? row__ + C - (int)(old__ & 3u) : -1;               \
                _Pragma("unroll") for (int q = 0; q < NC; ++q) cnt[q] += (int)(q == add__) - (int)(q == sub__); \
            }                                                                                                   \
        }                                                                                                       \
    } while (0)
                if (tid == 0) HP_EXPAND(t, 0);
                const int64_t t0 = rowptr[t], t1 = rowptr[t + 1];
                if (K == 1) {
                    for (int64_t j = t0 + tid; j < t1; j += HP_BLOCK) {
                        const int32_t w = col[j];
                        if ((uint64_t)w >= (uint64_t)n || HP_SKIP((int32_t)t, w)) continue;
                        c1t += w != (int32_t)t;
                        HP_EXPAND(w, 1);
                    }
                } else {
                    for (int64_t j = t0 + wave; j < t1; j += HP_WAVES) {  // wave-uniform
                        const int32_t w = col[j];
                        if ((uint64_t)w >= (uint64_t)n || HP_SKIP((int32_t)t, w)) continue;
                        if (lane == 0) {
                            c1t += w != (int32_t)t;
                            HP_EXPAND(w, 1);
                        }
                        const int64_t r1 = rowptr[w + 1];
                        for (int64_t k = rowptr[w] + lane; k < r1; k += LPF_WAVE) {
                            const int32_t c = col[k];
                            if ((uint64_t)c < (uint64_t)n && !HP_SKIP(w, c)) HP_EXPAND(c, 2);
                        }
                    }
                }
#undef HP_EXPAND
            }
#pragma unroll
            for (int q = 0; q < NC; ++q) cnt[q] = hp_wave_sum(cnt[q]);
            c1t = hp_wave_sum(c1t);
            ftt = hp_wave_sum(ftt);
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < NC; ++q) s_part[wave][q] = cnt[q];
                s_part[wave][NC] = c1t;
                s_part[wave][NC + 1] = ftt;
            }
            __syncthreads();
            if (tid == 0) {
                int32_t *o = A.out + p * (D * D);
                if (!ok) {
#pragma unroll
                    for (int q = 0; q < D * D; ++q) o[q] = 0;
                } else {
                    int64_t v[NV];
#pragma unroll
                    for (int q = 0; q < NV; ++q) {
                        v[q] = 0;
#pragma unroll
                        for (int w = 0; w < HP_WAVES; ++w) v[q] += s_part[w][q];
                    }
                    int64_t sz_t[C];
                    sz_t[0] = 1;
                    sz_t[1] = v[NC];
                    if (K == 2) sz_t[C - 1] = v[NC + 1] - 1 - v[NC];
                    int64_t col_sum[C] = {}, far = n;
#pragma unroll
                    for (int i = 0; i < C; ++i) {
                        int64_t row_sum = 0;
#pragma unroll
                        for (int j = 0; j < C; ++j) {
                            o[i * D + j] = (int32_t)v[i * C + j];
                            row_sum += v[i * C + j];
                            col_sum[j] += v[i * C + j];
                        }
                        o[i * D + C] = (int32_t)(sz_s[i] - row_sum);
                        far -= sz_s[i];
                    }
#pragma unroll
                    for (int j = 0; j < C; ++j) {
                        o[C * D + j] = (int32_t)(sz_t[j] - col_sum[j]);
                        far -= sz_t[j] - col_sum[j];
                    }
                    o[C * D + C] = (int32_t)far;
                }
            }
            __syncthreads();                      // s_part is rewritten by the next pair
        }
#undef HP_SKIP
    }
}

}  // namespace

extern "C" int64_t lpf_pair_hop_counts_workspace_bytes(int64_t n, int64_t n_groups) {
    if (n <= 0 || n_groups <= 0) return 0;
    return HP_HEADER + n_groups * 8 * n;        // the unit ticket, then per group two 32-bit words per node
}

extern "C" int lpf_pair_hop_counts(int64_t m, int64_t n, const int64_t *pairs, int64_t pair_stride,
                                   const int64_t *rowptr, const int32_t *col, int32_t hops, int32_t ignore_direct,
                                   const int32_t *unit_ptr, void *workspace, int64_t n_groups, int32_t *table_out,
                                   void *stream) {
    LPF_REQUIRE(hops >= 1 && hops <= 2 && n_groups > 0 && n_groups <= 65535);
    if (m == 0) return LPF_OK;
    LPF_REQUIRE(m > 0 && m < HP_MAX_PAIRS && n > 0 && n < INT32_MAX - 2 && pairs && pair_stride >= m && rowptr &&
                col && unit_ptr && workspace && table_out && lpf_aligned16(workspace));
    HopArgs A{};
    A.m = m;
    A.n = n;
    A.pairs = pairs;
    A.ld = pair_stride;
    A.rowptr = rowptr;
    A.col = col;
    A.ignore_direct = ignore_direct ? 1 : 0;
    A.unit_ptr = unit_ptr;
    A.ticket = static_cast<int32_t *>(workspace);
    A.state = reinterpret_cast<uint32_t *>(static_cast<char *>(workspace) + HP_HEADER);
    A.out = table_out;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t grid = m < n_groups ? m : n_groups;
    if (hipMemsetAsync(workspace, 0, (size_t)(HP_HEADER + grid * n * 8), s) != hipSuccess) {   // ticket and state
        lpf_set_hip_error(hipGetLastError());
        return LPF_ERR_LAUNCH;
    }
    if (hops == 1)
        hipLaunchKernelGGL(pair_hops_kernel<1>, dim3((unsigned)grid), dim3(HP_BLOCK), 0, s, A);
    else
        hipLaunchKernelGGL(pair_hops_kernel<2>, dim3((unsigned)grid), dim3(HP_BLOCK), 0, s, A);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}
