// Walk counts per pair on the typing adjacency (what the Katz index sums: Katz(a, b) = sum_l beta^l (A^l)[a, b], the
// other global structural baseline of HeaRT / OGB link prediction next to the shortest path): for each pair (a, b) of a
// binary CSR with sorted, unique int32 columns and a SYMMETRIC pattern (values ignored; a non-symmetric pattern is
// outside the contract: the two halves of a walk would be counted on different graphs) and l = 1 .. max_len <= 4
//   W_l(a, b) = (A^l)[a, b], the number of walks of l stored entries from a to b.
// Stored self-loops count as the entries they are; a == b is no special case (closed walks: W_2(a, a) = deg(a)); an id
// outside [0, n) gives 0 for every l.  ignore_direct: for THIS pair every transition x -> y with {x, y} = {a, b} is
// skipped at every step, which is counting on a copy of A without the stored entries (a, b) and (b, a).
//
// Meet in the middle: no pair expands more than two hops from either endpoint.  The caller hands the pairs over
// oriented and sorted: row 0 holds a pair's SPREAD endpoint s, row 1 its WALK endpoint t (symmetry makes either choice
// give the same integers), and unit_ptr cuts the list into units, runs of pairs with the same s.  Persistent 256-thread
// workgroups take units by an atomic ticket (the units differ by orders of magnitude in length: a fixed stride would
// leave workgroups idle) and, per unit,
//   * spread s once into the workgroup's dense state over all n nodes, one 64-bit word per node in the caller's
//     workspace: the high half is an epoch stamp, the low half the payload.  The epoch grows by one per unit, so nothing
//     is cleared between units; the entry point zeroes the words once per call.  Payload bit 0 is the indicator of
//     N(s); for max_len = 4 bits 1 .. 31 hold the two-hop count T2_s[c] = |N(s) & N(c)| <= deg(s) < 2^31.  A touch is
//     two integer atomics on the word, both without a return value: an unsigned 64-bit max with (epoch << 32), which
//     resets a word of an older epoch and leaves a current one as it is, then an add of 1 (indicator: the columns of a
//     row are unique, so the bit is added once) or 2 (two-hop count).  Max and add commute with the touches of other
//     lanes in every order that keeps a lane's own max before its own add, and one wave's memory operations on one
//     address stay in order.  A wave takes a row of N(s) at a time for the second hop, its lanes the row's columns;
//   * then walk each pair of the unit two hops from t:  W_1 = ind_s[t];  W_2 = sum_{w in N(t)} ind_s[w];
//     W_3 = sum_{w in N(t)} sum_{c in N(w)} ind_s[c];  W_4 = sum_{w in N(t)} sum_{c in N(w)} T2_s[c]  -- a wave per w,
//     its lanes over N(w); 64-bit unsigned per-lane partial sums, reduced over the workgroup (shuffles, then LDS), one
//     plain store per count.  One walk yields every requested length; max_len < 4 spreads one hop only, max_len < 3
//     walks one hop only, max_len = 1 reads one word.
// ignore_direct: the kernel skips the transitions {s, t} -- in the spread and in the walk -- in units of ONE pair only;
// the caller makes every pair that is a stored entry a unit of its own (a pair that is no entry has no such transition,
// so skipping changes nothing for it, and it keeps sharing its spread).
//
// Between the spread and the walk the lanes of a workgroup exchange GLOBAL data.  The spread writes with atomics only,
// which execute in L2; every wave then drains its own (release fence at agent scope and an explicit wait for its
// outstanding memory operations) before a workgroup barrier, and the walk reads the words with relaxed agent-scope
// atomic loads, which are served from L2 and not from a vector L1 line an earlier unit's walk left behind.  The walk's
// loads are consumed before the barriers of its reduction, so the next unit's spread cannot overtake them.
//
// Deterministic: integer sums only, no floats; a count is a pure function of (graph, pair, options) -- not of the
// pair's position, the orientation, the units, the number of workgroups or timing.
#include "lpf_common.h"

namespace {

constexpr int WK_BLOCK = 256;                   // 4 wavefronts
constexpr int WK_WAVES = WK_BLOCK / LPF_WAVE;
constexpr int64_t WK_HEADER = 16;               // bytes in front of the state: the unit ticket

typedef unsigned long long wk_u64;

struct WalkArgs {
    int64_t m, n;
    const int64_t *pairs;
    int64_t ld;
    const int64_t *rowptr;
    const int32_t *col;
    int32_t max_len;
    int32_t ignore_direct;
    const int32_t *unit_ptr;                    // [m + 1]
    int32_t *ticket;
    wk_u64 *state;                              // [n_groups][n]
    int64_t *out;                               // [m][max_len]
};

__device__ __forceinline__ void wk_touch(wk_u64 *word, wk_u64 stamp, wk_u64 add) {
    atomicMax(word, stamp);
    atomicAdd(word, add);
}

// the payload of a node in the current epoch (0 when its word is of an older one)
__device__ __forceinline__ uint32_t wk_payload(const wk_u64 *word, uint32_t epoch) {
    const wk_u64 v = __hip_atomic_load(const_cast<wk_u64 *>(word), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (uint32_t)(v >> 32) == epoch ? (uint32_t)v : 0u;
}

__device__ __forceinline__ wk_u64 wk_wave_sum(wk_u64 v) {
#pragma unroll
    for (int d = LPF_WAVE >> 1; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(WK_BLOCK) void pair_walks_kernel(WalkArgs A) {
    __shared__ wk_u64 s_part[WK_WAVES][3];
    __shared__ int32_t s_ticket;
    const int tid = threadIdx.x, lane = lpf_lane(), wave = tid >> 6;
    const int64_t n = A.n, m = A.m;
    const int L = A.max_len;
    const int64_t *__restrict__ rowptr = A.rowptr;
    const int32_t *__restrict__ col = A.col;
    wk_u64 *st = A.state + (int64_t)blockIdx.x * n;
    uint32_t epoch = 0;                           // the state is zeroed before the launch
    for (;;) {
        if (tid == 0) s_ticket = atomicAdd(A.ticket, 1);
        __syncthreads();
        const int64_t u = s_ticket;
        __syncthreads();                          // s_ticket is rewritten by the next unit
        if (u < 0 || u >= m) break;               // block-uniform
        const int64_t lo = A.unit_ptr[u], hi = A.unit_ptr[u + 1];
        if (lo < 0 || lo >= m) break;             // past the last unit
        if (hi <= lo || hi > m) continue;         // (a malformed unit: nothing is written for it)
        ++epoch;                                  // (fewer than 2^31 units per launch)
        const wk_u64 stamp = (wk_u64)epoch << 32;
        const int64_t s = A.pairs[lo];
        const bool s_ok = (uint64_t)s < (uint64_t)n;
        // one-pair units skip the transitions {s, t0}; -1 matches no column
        const int64_t t_only = A.pairs[A.ld + lo];
        const bool own = A.ignore_direct && hi - lo == 1 && s_ok && (uint64_t)t_only < (uint64_t)n;
        const int32_t ks = own ? (int32_t)s : -1, kt = own ? (int32_t)t_only : -1;
#define WK_SKIP(x, y) (own && (((x) == ks && (y) == kt) || ((x) == kt && (y) == ks)))
        if (s_ok) {
            const int64_t s0 = rowptr[s], s1 = rowptr[s + 1];
            for (int64_t j = s0 + tid; j < s1; j += WK_BLOCK) {
                const int32_t c = col[j];
                if ((uint64_t)c < (uint64_t)n && !WK_SKIP((int32_t)s, c)) wk_touch(&st[c], stamp, 1ull);
            }
            if (L >= 4) {
                for (int64_t j = s0 + wave; j < s1; j += WK_WAVES) {     // wave-uniform
                    const int32_t w = col[j];
                    if ((uint64_t)w >= (uint64_t)n || WK_SKIP((int32_t)s, w)) continue;
                    const int64_t w1 = rowptr[w + 1];
                    for (int64_t k = rowptr[w] + lane; k < w1; k += LPF_WAVE) {
                        const int32_t c = col[k];
                        if ((uint64_t)c < (uint64_t)n && !WK_SKIP(w, c)) wk_touch(&st[c], stamp, 2ull);
                    }
                }
            }
        }
        // every wave's atomics have executed before any wave reads the state
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int64_t p = lo; p < hi; ++p) {       // block-uniform
            const int64_t t = A.pairs[A.ld + p];
            wk_u64 w1c = 0, w2 = 0, w3 = 0, w4 = 0;
            if (s_ok && (uint64_t)t < (uint64_t)n) {
                if (tid == 0) w1c = wk_payload(&st[t], epoch) & 1u;
                const int64_t t0 = rowptr[t], t1 = rowptr[t + 1];
                if (L == 2) {
                    for (int64_t j = t0 + tid; j < t1; j += WK_BLOCK) {
                        const int32_t w = col[j];
                        if ((uint64_t)w < (uint64_t)n && !WK_SKIP((int32_t)t, w)) w2 += wk_payload(&st[w], epoch) & 1u;
                    }
                } else if (L >= 3) {
                    for (int64_t j = t0 + wave; j < t1; j += WK_WAVES) {  // wave-uniform
                        const int32_t w = col[j];
                        if ((uint64_t)w >= (uint64_t)n || WK_SKIP((int32_t)t, w)) continue;
                        if (lane == 0) w2 += wk_payload(&st[w], epoch) & 1u;
                        const int64_t r1 = rowptr[w + 1];
                        for (int64_t k = rowptr[w] + lane; k < r1; k += LPF_WAVE) {
                            const int32_t c = col[k];
                            if ((uint64_t)c < (uint64_t)n && !WK_SKIP(w, c)) {
                                const uint32_t v = wk_payload(&st[c], epoch);
                                w3 += v & 1u;
                                w4 += v >> 1;
                            }
                        }
                    }
                }
            }
            w2 = wk_wave_sum(w2);
            w3 = wk_wave_sum(w3);
            w4 = wk_wave_sum(w4);
            if (lane == 0) {
                s_part[wave][0] = w2;
                s_part[wave][1] = w3;
                s_part[wave][2] = w4;
            }
            __syncthreads();
            if (tid == 0) {
                int64_t *o = A.out + p * L;
                o[0] = (int64_t)w1c;
                for (int l = 2; l <= L; ++l) {
                    wk_u64 v = 0;
#pragma unroll
                    for (int q = 0; q < WK_WAVES; ++q) v += s_part[q][l - 2];
                    o[l - 1] = (int64_t)v;
                }
            }
            __syncthreads();                      // s_part is rewritten by the next pair
        }
#undef WK_SKIP
    }
}

}  // namespace

extern "C" int64_t lpf_pair_walks_workspace_bytes(int64_t n, int64_t n_groups) {
    if (n <= 0 || n_groups <= 0) return 0;
    return WK_HEADER + n_groups * 8 * n;        // the unit ticket, then per group one 64-bit word per node
}

extern "C" int lpf_pair_walks(int64_t m, int64_t n, const int64_t *pairs, int64_t pair_stride, const int64_t *rowptr,
                              const int32_t *col, int32_t max_len, int32_t ignore_direct, const int32_t *unit_ptr,
                              void *workspace, int64_t n_groups, int64_t *walks_out, void *stream) {
    LPF_REQUIRE(max_len >= 1 && max_len <= 4 && n_groups > 0 && n_groups <= 65535);
    if (m == 0) return LPF_OK;
    LPF_REQUIRE(m > 0 && m < INT32_MAX && n > 0 && n < INT32_MAX - 2 && pairs && pair_stride >= m && rowptr && col &&
                unit_ptr && workspace && walks_out && lpf_aligned16(workspace));
    WalkArgs A{};
    A.m = m;
    A.n = n;
    A.pairs = pairs;
    A.ld = pair_stride;
    A.rowptr = rowptr;
    A.col = col;
    A.max_len = max_len;
    A.ignore_direct = ignore_direct ? 1 : 0;
    A.unit_ptr = unit_ptr;
    A.ticket = static_cast<int32_t *>(workspace);
    A.state = reinterpret_cast<wk_u64 *>(static_cast<char *>(workspace) + WK_HEADER);
    A.out = walks_out;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t grid = m < n_groups ? m : n_groups;
    if (hipMemsetAsync(workspace, 0, (size_t)(WK_HEADER + grid * n * 8), s) != hipSuccess) {   // ticket and state
        lpf_set_hip_error(hipGetLastError());
        return LPF_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(pair_walks_kernel, dim3((unsigned)grid), dim3(WK_BLOCK), 0, s, A);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}
