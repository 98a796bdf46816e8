// Ranking counts on the device: for each positive score, how many negatives are >= it and how many are > it.
// Ranks, Hits@K, MRR, AUC and AP all follow from these two integers (lpformer_amd/evaluate.py).
//
// Comparison semantics are IEEE, exactly those of the torch expressions (neg >= pos).sum() and (neg > pos).sum():
// a NaN compares false with everything (a NaN negative is never counted, a NaN positive gets ge = gt = 0),
// -0.0 == +0.0, and +-inf are ordinary values.
//
// 1. Rows (lpf_rank_rows_f32): pos[P] against neg[P, K], each positive with its own negatives (HeaRT, citation2).  One
//    pass over the negatives.  A group of G lanes (G = 1 .. 64, a power of two chosen from K so that every lane has a
//    few 16-byte loads to issue) takes a row: its head up to the first 16-byte boundary and its tail are read as single
//    floats, the body as float4, so rows of any stride and base alignment use wide loads.  Each lane keeps integer
//    counters; a xor butterfly over the group adds them.  No atomics touch ge / gt: they are exact and order-free.
//
// 2. Shared (lpf_rank_shared_f32): pos[P] against ONE set neg[M] (the OGB layout).  The negatives are mapped to uint32
//    keys whose unsigned order is the IEEE order (-0.0 folded onto +0.0, every NaN onto 0xFFFFFFFF, above +inf), sorted
//    once by rocPRIM's radix sort, and each positive is answered by two lower-bound searches: ge = Mv - lb(key),
//    gt = Mv - lb(key + 1), Mv = lb(0xFFFFFFFF) = the negatives that are not NaN.  The top of the search tree is an
//    evenly spaced sample of up to RS_PIVOTS sorted keys that every workgroup stages in LDS; only the last
//    log2(M / RS_PIVOTS) steps read global memory.  The [P, M] comparison matrix never exists; the sorted keys belong
//    to the caller, so a second set of positives against the same negatives skips the sort.
//
// NaN tallies (nan_counts[0]: positives, [1]: negatives) are the only atomics here: integer adds, so still exact.
#include <rocprim/device/device_radix_sort.hpp>

#include "lpf_common.h"

namespace {

constexpr int RR_BLOCK = 256;
constexpr int RS_BLOCK = 256;
constexpr int RS_PIVOTS = 4096;                 // 16 KiB of LDS per workgroup
constexpr uint32_t RS_NAN_KEY = 0xFFFFFFFFu;

__host__ __device__ __forceinline__ int64_t rs_align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

// unsigned order of the keys == IEEE order of the floats; the largest key of a number is +inf -> 0xFF800000
__device__ __forceinline__ uint32_t rs_key(float x) {
    if (x != x) return RS_NAN_KEY;
    const uint32_t b = __float_as_uint(x + 0.0f);    // -0.0 + 0.0 == +0.0 (round to nearest)
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

template <int G>
__device__ __forceinline__ int rr_group_sum(int v) {
#pragma unroll
    for (int m = G >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ void rr_count(float x, float p, int &ge, int &gt, int &nn) {
    ge += (x >= p) ? 1 : 0;
    gt += (x > p) ? 1 : 0;
    nn += (x != x) ? 1 : 0;
}

template <int G>
__global__ __launch_bounds__(RR_BLOCK) void rank_rows_kernel(int64_t P, int64_t K, const float *__restrict__ pos,
                                                             const float *__restrict__ neg, int64_t ld,
                                                             int32_t *__restrict__ ge_out, int32_t *__restrict__ gt_out,
                                                             unsigned long long *__restrict__ nan_counts) {
    constexpr int ROWS = RR_BLOCK / G;          // rows per workgroup
    const int g = threadIdx.x & (G - 1);
    const int64_t r = (int64_t)blockIdx.x * ROWS + (threadIdx.x / G);
    int ge = 0, gt = 0, nn = 0, np = 0;
    if (r < P) {                                // (uniform over the group; the shuffles below are outside)
        const float p = pos[r];
        np = (g == 0 && p != p) ? 1 : 0;
        const float *row = neg + r * ld;
        const int64_t mis = (int64_t)((reinterpret_cast<uintptr_t>(row) >> 2) & 3u);
        int64_t head = (4 - mis) & 3;           // floats before the first 16-byte boundary
        head = head < K ? head : K;
        const int64_t nv = (K - head) >> 2;     // float4 in the body
        const int64_t tail0 = head + 4 * nv;    // first float of the tail
        const int64_t edge = head + (K - tail0);   // head and tail floats: at most 6
        for (int64_t i = g; i < edge; i += G) rr_count(row[i < head ? i : tail0 + (i - head)], p, ge, gt, nn);
        const float4 *body = reinterpret_cast<const float4 *>(row + head);
        for (int64_t v = g; v < nv; v += G) {
            const float4 x = body[v];
            rr_count(x.x, p, ge, gt, nn);
            rr_count(x.y, p, ge, gt, nn);
            rr_count(x.z, p, ge, gt, nn);
            rr_count(x.w, p, ge, gt, nn);
        }
    }
    ge = rr_group_sum<G>(ge);
    gt = rr_group_sum<G>(gt);
    if (r < P && g == 0) {
        ge_out[r] = ge;
        gt_out[r] = gt;
    }
    // NaN tallies of the wavefront (a lane sees fewer than 2^31 values; the sum over 64 lanes is taken in 64 bits)
    long long nn64 = nn, np64 = np;
#pragma unroll
    for (int m = LPF_WAVE >> 1; m > 0; m >>= 1) {
        nn64 += __shfl_xor(nn64, m, 64);
        np64 += __shfl_xor(np64, m, 64);
    }
    if (lpf_lane() == 0) {
        if (np64) atomicAdd(&nan_counts[0], (unsigned long long)np64);
        if (nn64) atomicAdd(&nan_counts[1], (unsigned long long)nn64);
    }
}

__global__ __launch_bounds__(RS_BLOCK) void rank_keys_kernel(int64_t M, const float *__restrict__ neg,
                                                             uint32_t *__restrict__ keys) {
    const int64_t step = (int64_t)gridDim.x * RS_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x; i < M; i += step) keys[i] = rs_key(neg[i]);
}

// first index i in [lo, hi) with a[i] >= key; hi if none
__device__ __forceinline__ int64_t rs_lower_bound(const uint32_t *a, int64_t lo, int64_t hi, uint32_t key) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Lower bound over all M sorted keys.  piv[j] = sorted[s_j], s_j = floor(j * M / npiv) (s_0 = 0, strictly ascending as
// npiv <= M).  With j = the first pivot >= key: sorted[s_(j-1)] < key <= sorted[s_j], so the answer lies in
// (s_(j-1), s_j]; for npiv == M that is one index and nothing is read from global memory.
__device__ __forceinline__ int64_t rs_search(const uint32_t *__restrict__ sorted, int64_t M, const uint32_t *piv,
                                             int npiv, uint32_t key) {
    int lo = 0, hi = npiv;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (piv[mid] < key) lo = mid + 1; else hi = mid;
    }
    const int64_t first = lo == 0 ? 0 : ((int64_t)(lo - 1) * M) / npiv + 1;
    const int64_t last = lo == npiv ? M : ((int64_t)lo * M) / npiv;
    return rs_lower_bound(sorted, first, last, key);
}

__global__ __launch_bounds__(RS_BLOCK) void rank_shared_kernel(int64_t P, const float *__restrict__ pos, int64_t M,
                                                               const uint32_t *__restrict__ sorted,
                                                               int32_t *__restrict__ ge_out, int32_t *__restrict__ gt_out,
                                                               unsigned long long *__restrict__ nan_counts) {
    __shared__ uint32_t piv[RS_PIVOTS];
    __shared__ int64_t mv_sh;
    const int npiv = M < RS_PIVOTS ? (int)M : RS_PIVOTS;
    for (int j = threadIdx.x; j < npiv; j += RS_BLOCK) piv[j] = sorted[((int64_t)j * M) / npiv];
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t mv = rs_search(sorted, M, piv, npiv, RS_NAN_KEY);   // the negatives that are not NaN
        mv_sh = mv;
        if (blockIdx.x == 0) nan_counts[1] = (unsigned long long)(M - mv);
    }
    __syncthreads();
    const int64_t mv = mv_sh;
    const int64_t step = (int64_t)gridDim.x * RS_BLOCK;
    const int64_t rounds = (P + step - 1) / step;              // uniform trip count: the ballot sees whole wavefronts
    for (int64_t it = 0; it < rounds; ++it) {
        const int64_t i = it * step + (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
        bool is_nan = false;
        if (i < P) {
            const uint32_t key = rs_key(pos[i]);
            is_nan = key == RS_NAN_KEY;
            int32_t ge = 0, gt = 0;
            if (!is_nan) {
                ge = (int32_t)(mv - rs_search(sorted, M, piv, npiv, key));
                gt = (int32_t)(mv - rs_search(sorted, M, piv, npiv, key + 1u));   // key <= 0xFF800000: no wrap
            }
            ge_out[i] = ge;
            gt_out[i] = gt;
        }
        const unsigned long long bm = __ballot(is_nan);
        if (bm && lpf_lane() == 0) atomicAdd(&nan_counts[0], (unsigned long long)__popcll(bm));
    }
}

size_t rs_sort_tmp_bytes(int64_t M) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_keys(nullptr, bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)M, 0u, 32u);
    return bytes;
}

template <int G>
void rr_launch(int64_t P, int64_t K, const float *pos, const float *neg, int64_t ld, int32_t *ge, int32_t *gt,
               unsigned long long *nan_counts, hipStream_t s) {
    constexpr int ROWS = RR_BLOCK / G;
    hipLaunchKernelGGL(rank_rows_kernel<G>, dim3((unsigned)((P + ROWS - 1) / ROWS)), dim3(RR_BLOCK), 0, s, P, K, pos,
                       neg, ld, ge, gt, nan_counts);
}

}  // namespace

extern "C" int lpf_rank_rows_f32(int64_t P, int64_t K, const float *pos, const float *neg, int64_t ld_neg, int32_t *ge,
                                 int32_t *gt, int64_t *nan_counts, void *stream) {
    LPF_REQUIRE(P >= 0 && P < INT32_MAX && K >= 0 && K < INT32_MAX && nan_counts);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(nan_counts, 0, 2 * sizeof(int64_t), s) != hipSuccess) {
        lpf_set_hip_error(hipGetLastError());
        return LPF_ERR_LAUNCH;
    }
    if (P == 0) return LPF_OK;
    LPF_REQUIRE(pos && ge && gt && (K == 0 || (neg && ld_neg >= 0)));
    unsigned long long *nc = reinterpret_cast<unsigned long long *>(nan_counts);
    // lanes per row: every lane gets about four 16-byte loads (K = 100 -> 8 lanes, K = 1000 -> 64 lanes)
    const int64_t want = (K + 15) / 16;
    if (want <= 1) rr_launch<1>(P, K, pos, neg, ld_neg, ge, gt, nc, s);
    else if (want <= 2) rr_launch<2>(P, K, pos, neg, ld_neg, ge, gt, nc, s);
    else if (want <= 4) rr_launch<4>(P, K, pos, neg, ld_neg, ge, gt, nc, s);
    else if (want <= 8) rr_launch<8>(P, K, pos, neg, ld_neg, ge, gt, nc, s);
    else if (want <= 16) rr_launch<16>(P, K, pos, neg, ld_neg, ge, gt, nc, s);
    else if (want <= 32) rr_launch<32>(P, K, pos, neg, ld_neg, ge, gt, nc, s);
    else rr_launch<64>(P, K, pos, neg, ld_neg, ge, gt, nc, s);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}

extern "C" int64_t lpf_rank_shared_workspace_bytes(int64_t P, int64_t M) {
    if (P < 0 || M <= 0 || M >= (1ll << 31)) return 0;
    return rs_align256(M * 4) + rs_align256((int64_t)rs_sort_tmp_bytes(M)) + 256;
}

extern "C" int lpf_rank_shared_f32(int64_t P, const float *pos, int64_t M, const float *neg, uint32_t *sorted_keys,
                                   void *workspace, int64_t workspace_bytes, int32_t *ge, int32_t *gt,
                                   int64_t *nan_counts, void *stream) {
    LPF_REQUIRE(P >= 0 && P < INT32_MAX && M >= 0 && M < (1ll << 31) && nan_counts);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(nan_counts, 0, 2 * sizeof(int64_t), s) != hipSuccess) {
        lpf_set_hip_error(hipGetLastError());
        return LPF_ERR_LAUNCH;
    }
    LPF_REQUIRE(P == 0 || (pos && ge && gt));
    LPF_REQUIRE(M == 0 || sorted_keys);
    const int cu = lpf_cu_count();
    if (neg && M > 0) {
        const int64_t keys_bytes = rs_align256(M * 4);
        LPF_REQUIRE(workspace && lpf_aligned16(workspace) && workspace_bytes >= lpf_rank_shared_workspace_bytes(P, M));
        uint32_t *keys = static_cast<uint32_t *>(workspace);
        void *tmp = static_cast<char *>(workspace) + keys_bytes;
        size_t tmp_bytes = (size_t)(workspace_bytes - keys_bytes);
        int64_t grid = (M + RS_BLOCK - 1) / RS_BLOCK;
        const int64_t cap = (int64_t)(cu > 0 ? cu : 256) * 8;
        grid = grid < cap ? grid : cap;
        hipLaunchKernelGGL(rank_keys_kernel, dim3((unsigned)grid), dim3(RS_BLOCK), 0, s, M, neg, keys);
        LPF_CHECK_LAUNCH();
        const hipError_t e = rocprim::radix_sort_keys(tmp, tmp_bytes, static_cast<const uint32_t *>(keys), sorted_keys,
                                                      (size_t)M, 0u, 32u, s);
        if (e != hipSuccess) {
            lpf_set_hip_error(e);
            return LPF_ERR_LAUNCH;
        }
    }
    if (P == 0) return LPF_OK;
    // (M == 0: no pivots, every search returns 0 and nothing is read through sorted_keys)
    // a few workgroups per CU, each staging the pivots once and striding over the positives
    int64_t grid = (P + RS_BLOCK - 1) / RS_BLOCK;
    const int64_t cap = (int64_t)(cu > 0 ? cu : 256) * 4;
    grid = grid < cap ? grid : cap;
    hipLaunchKernelGGL(rank_shared_kernel, dim3((unsigned)grid), dim3(RS_BLOCK), 0, s, P, pos, M,
                       static_cast<const uint32_t *>(sorted_keys), ge, gt,
                       reinterpret_cast<unsigned long long *>(nan_counts));
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}
