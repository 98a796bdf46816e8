// Threshold profile: how many nodes of each type every pair of a batch would select at each of T PPR thresholds -- the
// three numbers (thresh_cn, thresh_1hop, thresh_non1hop; src/models/link_transformer.py:241-250, 478) the reference
// tunes by grid search (src/run.py:199-201), answered for a whole grid in one pass over the UNFILTERED graphs.
//
// For pair (a, b), binary typing adjacency A and raw PPR matrix P (CSRs with sorted, unique columns; P reads 0 where
// nothing is stored), a candidate v has a type and two round-tripped values (ra, rb):
//   type 0  v in N(a) & N(b)                                   ra = rt2(P[a,v]), rb = rt2(P[b,v])   (mode "cn": rt1)
//   type 1  v in exactly one of N(a), N(b)                     ra = rt1(P[a,v]), rb = rt1(P[b,v])
//   type 2  v in neither, P[a,v] > 0 and P[b,v] > 0 (stored)   ra = rt1(P[a,v]), rb = rt1(P[b,v])
// (lpf_rt1 / lpf_rt2: the reference's fp32 round trips, op by op) and count[p, t, j] = #{v of type t: ra >= theta_j and
// rb >= theta_j}: exactly what a model built with that threshold selects, boundary values included.  No special case
// for v in {a, b} or a == b.  Mode "cn" has type 0 only.
//
// A pair is a stream of slots: [0, deg a) walks N(a) (search N(b), P_a, P_b), the next deg b slots walk N(b) (search
// N(a): a member is a common neighbour the first walk has counted; else P_a, P_b), the last min(|P_a|, |P_b|) walk the
// shorter PPR row (search the other, then both adjacency rows).  One slot per lane and round.  A lane turns its slot
// into (type, k), k = the number of thresholds it passes -- ascending thresholds: it passes theta_0 .. theta_{k-1} --
// and the round's counts come from one ballot + popcount per type and threshold, stopped at the largest k of the round;
// lane j keeps the three counts of threshold j.  Two classes of work, split by the stream length L:
//   * L <= split_threshold: one wavefront per pair, a grid-stride loop over the pairs;
//   * longer pairs go on a list (an int32 ticket) and a second kernel gives each a 256-thread workgroup; its four waves
//     add their counts into integer LDS counters.
// total / max_per_pair / nonempty: running values in registers across the pairs a wave (workgroup) handles, summed over
// the workgroup in LDS, then ONE integer global atomic per workgroup, type and threshold.  Integers only: the result
// depends on neither the launch shape nor the split path nor timing.
#include "walk_common.h"

namespace {

constexpr int TP_BLOCK = 256;                   // 4 wavefronts
constexpr int TP_WAVES = TP_BLOCK / LPF_WAVE;
constexpr int TP_GRID = 2048;                   // persistent workgroups of either kernel
constexpr int TP_MAX_T = LPF_THRESH_MAX_T;

struct ProfArgs {
    int64_t P, n;
    const int64_t *pairs;
    int64_t ld;
    const int64_t *adj_rowptr;
    const int32_t *adj_col;
    const int64_t *ppr_rowptr;
    const int32_t *ppr_col;
    const float *ppr_val;
    int32_t T, mode_cn;
    int64_t thr;
    int32_t *long_list;
    int32_t *per_pair;                          // [P, 3, T] or NULL
    unsigned long long *total, *nonempty;       // [3, T]
    int32_t *max_per_pair;                      // [3, T]
    float th[TP_MAX_T];
};

struct PairWalk {
    int64_t a0, b0, pa0, pb0;                   // first entries of the adjacency / PPR rows of a and b
    int32_t da, db, la, lb;                     // their lengths
    int32_t w1, w2, w3;                         // slots of the three walks (mode "cn": the first only)
};

// Rows and walks of (a, b); everything empty when an id lies outside [0, n).  Mode "cn" needs the common neighbours
// alone, and they are symmetric in (a, b): the endpoint with the shorter adjacency row takes the place of a.
__device__ __forceinline__ PairWalk pair_walk(const ProfArgs &A, int64_t p) {
    PairWalk w{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int64_t a = A.pairs[p], b = A.pairs[A.ld + p];
    if ((uint64_t)a >= (uint64_t)A.n || (uint64_t)b >= (uint64_t)A.n) return w;
    if (A.mode_cn && A.adj_rowptr[b + 1] - A.adj_rowptr[b] < A.adj_rowptr[a + 1] - A.adj_rowptr[a]) {
        const int64_t t = a;
        a = b;
        b = t;
    }
    w.a0 = A.adj_rowptr[a];
    w.da = (int32_t)(A.adj_rowptr[a + 1] - w.a0);
    w.b0 = A.adj_rowptr[b];
    w.db = (int32_t)(A.adj_rowptr[b + 1] - w.b0);
    w.pa0 = A.ppr_rowptr[a];
    w.la = (int32_t)(A.ppr_rowptr[a + 1] - w.pa0);
    w.pb0 = A.ppr_rowptr[b];
    w.lb = (int32_t)(A.ppr_rowptr[b + 1] - w.pb0);
    w.w1 = w.da;
    w.w2 = A.mode_cn ? 0 : w.db;
    w.w3 = A.mode_cn ? 0 : min(w.la, w.lb);
    return w;
}

__device__ __forceinline__ int64_t walk_len(const PairWalk &w) { return (int64_t)w.w1 + w.w2 + w.w3; }

// P[row, key] (0 where nothing is stored); `found` says whether an entry is stored
__device__ __forceinline__ float row_val(const int32_t *__restrict__ col, const float *__restrict__ val, int64_t r0,
                                         int32_t len, int32_t key, bool &found) {
    const int64_t i = lpf_lower_bound(col, r0, r0 + len, key);
    found = i < r0 + len && col[i] == key;
    return found ? val[i] : 0.f;
}

// Slot f of the pair's stream: its type (-1: no candidate) and k = the number of thresholds both values pass.
__device__ __forceinline__ int slot_type(const ProfArgs &A, const PairWalk &w, int64_t f, const float *th, int &k) {
    k = 0;
    int type;
    float va, vb;
    bool found;
    if (f < w.w1) {                              // N(a)
        const int32_t v = A.adj_col[w.a0 + f];
        const bool cn = lpf_sorted_has(A.adj_col, w.b0, w.b0 + w.db, v);
        if (A.mode_cn && !cn) return -1;
        type = cn ? 0 : 1;
        va = row_val(A.ppr_col, A.ppr_val, w.pa0, w.la, v, found);
        vb = row_val(A.ppr_col, A.ppr_val, w.pb0, w.lb, v, found);
    } else if (f < (int64_t)w.w1 + w.w2) {       // N(b) minus N(a)
        const int32_t v = A.adj_col[w.b0 + (f - w.w1)];
        if (lpf_sorted_has(A.adj_col, w.a0, w.a0 + w.da, v)) return -1;
        type = 1;
        va = row_val(A.ppr_col, A.ppr_val, w.pa0, w.la, v, found);
        vb = row_val(A.ppr_col, A.ppr_val, w.pb0, w.lb, v, found);
    } else {                                     // the shorter PPR row
        const int64_t i = f - w.w1 - w.w2;
        const bool src_a = w.la <= w.lb;
        const int64_t s0 = src_a ? w.pa0 : w.pb0;
        const int32_t v = A.ppr_col[s0 + i];
        const float ws = A.ppr_val[s0 + i];
        const float wo = row_val(A.ppr_col, A.ppr_val, src_a ? w.pb0 : w.pa0, src_a ? w.lb : w.la, v, found);
        if (!(found && ws > 0.f && wo > 0.f)) return -1;
        if (lpf_sorted_has(A.adj_col, w.a0, w.a0 + w.da, v) || lpf_sorted_has(A.adj_col, w.b0, w.b0 + w.db, v)) return -1;
        type = 2;
        va = src_a ? ws : wo;
        vb = src_a ? wo : ws;
    }
    const bool two = type == 0 && !A.mode_cn;
    const float ra = two ? lpf_rt2(va) : lpf_rt1(va);
    const float rb = two ? lpf_rt2(vb) : lpf_rt1(vb);
    for (int j = 0; j < A.T; ++j) k += (ra >= th[j] && rb >= th[j]) ? 1 : 0;   // (LDS broadcast reads)
    return type;
}

// One round of a wavefront: lane j adds to c[t] the slots of type t that pass threshold j.
__device__ __forceinline__ void count_round(int type, int k, int lane, int32_t (&c)[3]) {
    const uint64_t any = __ballot(type >= 0 && k > 0);
    if (!any) return;                            // wave-uniform
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        if (!__ballot(type == t && k > 0)) continue;
        for (int j = 0; j < TP_MAX_T; ++j) {     // ends at the largest k among the round's slots of this type
            const uint64_t m = __ballot(type == t && k > j);
            if (!m) break;
            if (lane == j) c[t] += __popcll(m);
        }
    }
}

// Running reductions of the pairs one thread (lane j of a wave, or thread t * 32 + j of a workgroup) has finished.
struct Running {
    unsigned long long tot, ne;
    int32_t mx;
    __device__ __forceinline__ void add(int32_t c) {
        tot += (unsigned long long)c;
        ne += c > 0 ? 1ull : 0ull;
        mx = max(mx, c);
    }
};

__device__ __forceinline__ void flush(const ProfArgs &A, int slot, const Running &r) {
    if (r.tot) atomicAdd(&A.total[slot], r.tot);
    if (r.ne) atomicAdd(&A.nonempty[slot], r.ne);
    if (r.mx > 0) atomicMax(&A.max_per_pair[slot], r.mx);
}

__global__ __launch_bounds__(TP_BLOCK) void thresh_short_kernel(ProfArgs A) {
    __shared__ float th[TP_MAX_T];
    __shared__ unsigned long long red_tot[3 * TP_MAX_T], red_ne[3 * TP_MAX_T];
    __shared__ int32_t red_mx[3 * TP_MAX_T];
    const int lane = lpf_lane(), wave = threadIdx.x >> 6;
    if (threadIdx.x < A.T) th[threadIdx.x] = A.th[threadIdx.x];
    if (threadIdx.x < 3 * TP_MAX_T) {
        red_tot[threadIdx.x] = 0ull;
        red_ne[threadIdx.x] = 0ull;
        red_mx[threadIdx.x] = 0;
    }
    __syncthreads();

    Running run[3] = {{0ull, 0ull, 0}, {0ull, 0ull, 0}, {0ull, 0ull, 0}};
    const int64_t stride = (int64_t)gridDim.x * TP_WAVES;
    for (int64_t p = (int64_t)blockIdx.x * TP_WAVES + wave; p < A.P; p += stride) {   // wave-uniform
        const PairWalk w = pair_walk(A, p);
        const int64_t L = walk_len(w);
        if (L > A.thr) {
            if (lane == 0) A.long_list[1 + atomicAdd(&A.long_list[0], 1)] = (int32_t)p;
            continue;
        }
        int32_t c[3] = {0, 0, 0};
        for (int64_t base = 0; base < L; base += LPF_WAVE) {
            const int64_t f = base + lane;
            int k = 0;
            const int type = f < L ? slot_type(A, w, f, th, k) : -1;
            count_round(type, k, lane, c);
        }
        if (lane < A.T) {
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                if (A.per_pair) A.per_pair[(p * 3 + t) * A.T + lane] = c[t];
                run[t].add(c[t]);
            }
        }
    }
    if (lane < A.T) {
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int s = t * TP_MAX_T + lane;
            if (run[t].tot) atomicAdd(&red_tot[s], run[t].tot);
            if (run[t].ne) atomicAdd(&red_ne[s], run[t].ne);
            if (run[t].mx > 0) atomicMax(&red_mx[s], run[t].mx);
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 * TP_MAX_T) {
        const int t = threadIdx.x / TP_MAX_T, j = threadIdx.x % TP_MAX_T;
        if (j < A.T) flush(A, t * A.T + j, Running{red_tot[threadIdx.x], red_ne[threadIdx.x], red_mx[threadIdx.x]});
    }
}

__global__ __launch_bounds__(TP_BLOCK) void thresh_long_kernel(ProfArgs A) {
    __shared__ float th[TP_MAX_T];
    __shared__ int32_t cnt[3 * TP_MAX_T];
    const int lane = lpf_lane();
    if (threadIdx.x < A.T) th[threadIdx.x] = A.th[threadIdx.x];
    if (threadIdx.x < 3 * TP_MAX_T) cnt[threadIdx.x] = 0;
    __syncthreads();
    // thread t * 32 + j owns the workgroup's (type t, threshold j)
    const int own_t = threadIdx.x / TP_MAX_T, own_j = threadIdx.x % TP_MAX_T;
    const bool owner = threadIdx.x < 3 * TP_MAX_T && own_j < A.T;
    Running run{0ull, 0ull, 0};
    const int32_t n_long = A.long_list[0];
    for (int32_t li = blockIdx.x; li < n_long; li += gridDim.x) {   // block-uniform
        const int64_t p = A.long_list[1 + li];
        const PairWalk w = pair_walk(A, p);
        const int64_t L = walk_len(w);
        int32_t c[3] = {0, 0, 0};
        for (int64_t base = 0; base < L; base += TP_BLOCK) {        // block-uniform trip count
            const int64_t f = base + threadIdx.x;
            int k = 0;
            const int type = f < L ? slot_type(A, w, f, th, k) : -1;
            count_round(type, k, lane, c);
        }
        if (lane < A.T) {
#pragma unroll
            for (int t = 0; t < 3; ++t)
                if (c[t]) atomicAdd(&cnt[t * TP_MAX_T + lane], c[t]);
        }
        __syncthreads();
        if (owner) {
            const int32_t v = cnt[threadIdx.x];
            if (A.per_pair) A.per_pair[(p * 3 + own_t) * A.T + own_j] = v;
            run.add(v);
            cnt[threadIdx.x] = 0;
        }
        __syncthreads();                         // cnt is added to again by the next pair
    }
    if (owner) flush(A, own_t * A.T + own_j, run);
}

}  // namespace

extern "C" int lpf_threshold_profile(int64_t P, int64_t n, const int64_t *pairs, int64_t pairs_ld,
                                     const int64_t *adj_rowptr, const int32_t *adj_col, const int64_t *ppr_rowptr,
                                     const int32_t *ppr_col, const float *ppr_val, int32_t T, const float *thresholds,
                                     int32_t mode_cn, int32_t split_threshold, int32_t *scratch, int32_t *per_pair,
                                     int64_t *total, int32_t *max_per_pair, int64_t *nonempty, void *stream) {
    LPF_REQUIRE(T >= 1 && T <= TP_MAX_T && thresholds);
    for (int j = 0; j < T; ++j) {
        const float t = thresholds[j];
        LPF_REQUIRE(t >= 0.f && t <= 3.402823466e+38f);               // (false for a NaN)
        LPF_REQUIRE(j == 0 || t > thresholds[j - 1]);
    }
    if (P == 0) return LPF_OK;
    LPF_REQUIRE(P > 0 && P < INT32_MAX && n > 0 && n <= INT32_MAX && pairs && pairs_ld >= P && adj_rowptr && adj_col &&
                ppr_rowptr && ppr_col && ppr_val && scratch && total && max_per_pair && nonempty);
    ProfArgs A;
    A.P = P;
    A.n = n;
    A.pairs = pairs;
    A.ld = pairs_ld;
    A.adj_rowptr = adj_rowptr;
    A.adj_col = adj_col;
    A.ppr_rowptr = ppr_rowptr;
    A.ppr_col = ppr_col;
    A.ppr_val = ppr_val;
    A.T = T;
    A.mode_cn = mode_cn != 0;
    A.thr = split_threshold < 0 ? LPF_THRESH_SPLIT_DEFAULT : split_threshold;
    A.long_list = scratch;
    A.per_pair = per_pair;
    A.total = reinterpret_cast<unsigned long long *>(total);
    A.nonempty = reinterpret_cast<unsigned long long *>(nonempty);
    A.max_per_pair = max_per_pair;
    for (int j = 0; j < TP_MAX_T; ++j) A.th[j] = j < T ? thresholds[j] : 0.f;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (lpf_reset_counter(scratch, s) != LPF_OK) return LPF_ERR_LAUNCH;   // long-pair counter
    const int64_t blocks = (P + TP_WAVES - 1) / TP_WAVES;
    hipLaunchKernelGGL(thresh_short_kernel, dim3((unsigned)(blocks < TP_GRID ? blocks : TP_GRID)), dim3(TP_BLOCK), 0, s,
                       A);
    LPF_CHECK_LAUNCH();
    hipLaunchKernelGGL(thresh_long_kernel, dim3((unsigned)(P < TP_GRID ? P : TP_GRID)), dim3(TP_BLOCK), 0, s, A);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}
