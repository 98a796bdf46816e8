// similar_nodes: for each of S query rows, the m table rows with the largest inner product (optionally scaled to a
// cosine), minus an exclusion row and the query's own node -- without ever holding an [S, n] score matrix.
//
// Score.  score(s, v) = sum_k Q[s][k] T[v][k] on v_mfma_f32_16x16x4_f32 (exact fp32 multiply-accumulate): the 16 query
// rows of a workgroup are the A operand (row = lane % 16), 16 table rows the B operand (column = lane % 16), lane
// (j = lane % 16, q = lane / 16) feeds k = 16 g + 4 q + u for the u-th MFMA of k-group g, so every operand fetch is one
// 16-byte load of one row (the layout of gemm_rows_kernel, gemm_f32.hip).  Even and odd MFMAs go to two accumulators
// (the dependent latency of the instruction is longer than its issue interval); their sum is the dot product.  The
// query fragments stay in registers for D <= 256 and are re-read from the cache otherwise.  The K tail is zeroed in
// both operands, so columns D .. ld - 1 may hold anything.  With scales the score is (dot * q_scale[s]) * t_scale[v].
//
// Ranking.  key(s, v) = (ordered uint32 of the score, -0.0 -> +0.0, NaN below -inf) << 32 | ~v: the key of
// lpf_segment_topk_f32 with the node id in place of the position.  Keys of one source are distinct and never 0 (v < 2^31
// keeps bit 31 of ~v set), so 0 is the padding key and the top m keys in descending order ARE the answer: a pure
// function of the inputs whatever the order the tiles are visited in.
//
// Layout.  Grid = (source tiles of `bs` rows) x (n_ranges node ranges).  A workgroup of four wavefronts streams its range
// 64 nodes a round, one 16 x 16 score tile per wavefront.  Per source it keeps in LDS a threshold key (the m-th best so
// far, 0 until there are m), a buffer of `cap` keys and a counter.  A lane whose key beats the threshold tests the
// exclusion row (binary search of v in the source's sorted row: only the few survivors get there) and appends the key
// at a slot taken by an LDS counter add.  cap is the power of two >= m + 64, so a buffer that holds <= cap - 64 keys
// takes any round; a round that leaves some buffer fuller raises a flag, and the workgroup then sorts every buffer
// (bitonic, in LDS), keeps m and raises the thresholds.  bs = 16 sources (8 when cap = 512): 32 KiB of keys.  At the end of
// its range the workgroup writes its m best keys per source, sorted, padded with 0, to workspace[s][range][m].
// The merge kernel (one workgroup per source, same stream) reads a source's ranges 2,048 entries a pass and collects
// the keys above its threshold (0 at first: everything but padding) in a buffer of 4,096; when the next pass might not
// fit it sorts, keeps m and raises the threshold, and once more at the end.  Ids and scores are decoded from the keys:
// padding never leaves the workspace.  A returned -0.0 score reads +0.0 and a NaN the canonical quiet NaN, as the key says.
//
// No workgroup waits on another; every loop is bounded by n, D, m or n_ranges * m; every global index is clamped or
// tested against n / S before use; no float atomics.
#include "lpf_common.h"

namespace {

typedef float f32x4s __attribute__((ext_vector_type(4)));

constexpr int SIM_BLOCK = 256;
constexpr int SIM_ROUND = 64;                   // nodes per round: 16 per wavefront
constexpr int SIM_TILE = 16;                    // query rows of an MFMA tile
constexpr int SIM_KEYS = 4096;                  // keys of a workgroup in LDS (32 KiB)
constexpr int SIM_MERGE_TAKE = 2048;            // workspace entries a merge pass reads
constexpr int SIM_TARGET_GRID = 512;            // default n_ranges: about two workgroups per CU of an MI355X
constexpr int SIM_MAX_RANGES = 65535;
constexpr int SIM_MAX_D = 4096;

struct SimArgs {
    int64_t S, n;
    int32_t D;
    const float *Q; int64_t ldq;
    const float *T; int64_t ldt;
    const float *q_scale, *t_scale;
    const int64_t *src_ids;
    const int64_t *exc_rowptr;
    const int32_t *exc_col;
    int32_t exclude_self, m, R, bs, cap;
    int64_t chunk;                              // nodes per range, a multiple of SIM_ROUND
    uint64_t *ws;
};

inline int sim_cap(int m) {
    int c = 128;
    while (c < m + SIM_ROUND) c <<= 1;
    return c;                                   // 128, 256 or 512
}
inline int sim_bs(int m) { return sim_cap(m) > 256 ? 8 : SIM_TILE; }

inline int64_t sim_ranges(int64_t S, int32_t m, int32_t n_ranges) {
    if (n_ranges > 0 || S < 1) return n_ranges > 0 ? n_ranges : 1;
    const int64_t tiles = (S + sim_bs(m) - 1) / sim_bs(m);
    const int64_t r = (SIM_TARGET_GRID + tiles - 1) / tiles;
    return r < 1 ? 1 : r;
}

__device__ __forceinline__ uint64_t sim_key(float f, uint32_t id) {
    uint32_t u = __float_as_uint(f);
    uint32_t o;
    if ((u & 0x7fffffffu) > 0x7f800000u) {
        o = 0u;                                 // NaN: below -inf (whose key is 0x007fffff)
    } else {
        if (u == 0x80000000u) u = 0u;           // -0.0 == +0.0
        o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return ((uint64_t)o << 32) | (uint64_t)(uint32_t)~id;
}

__device__ __forceinline__ float sim_key_score(uint64_t key) {
    const uint32_t o = (uint32_t)(key >> 32);
    if (o == 0u) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// columns k .. k + 3 of a row, zero from column D on (k a multiple of 4; the row holds pad4(D) readable floats)
__device__ __forceinline__ f32x4s sim_load4(const float *__restrict__ row, int k, int D) {
    f32x4s v = {0.f, 0.f, 0.f, 0.f};
    if (k < D) {
        v = *reinterpret_cast<const f32x4s *>(row + k);
        if (k + 3 >= D) {
            if (k + 1 >= D) v[1] = 0.f;
            if (k + 2 >= D) v[2] = 0.f;
            v[3] = 0.f;
        }
    }
    return v;
}

// Bitonic sort, descending, of every aligned block of `cap` keys of keys[0, total) (cap a power of two, total a multiple
// of cap, total / 2 compare-exchanges per step).  Ends with a barrier.
__device__ void sim_sort_desc(uint64_t *keys, int total, int cap) {
    for (int size = 2; size <= cap; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (total >> 1); t += SIM_BLOCK) {
                const int e = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
                const bool desc = ((e & (cap - 1)) & size) == 0;
                const uint64_t a = keys[e], b = keys[e + stride];
                if (desc ? a < b : a > b) {
                    keys[e] = b;
                    keys[e + stride] = a;
                }
            }
            __syncthreads();
        }
    }
}

template <int NG>
__global__ __launch_bounds__(SIM_BLOCK) void similar_scan_kernel(const SimArgs A) {
    __shared__ uint64_t keys[SIM_KEYS];
    __shared__ uint64_t thr[SIM_TILE];
    __shared__ int64_t sh_self[SIM_TILE], sh_e0[SIM_TILE], sh_e1[SIM_TILE];
    __shared__ int32_t cnt[SIM_TILE];
    __shared__ int32_t sh_full;

    const int lane = lpf_lane(), wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4;
    const int64_t tile = blockIdx.x / A.R;
    const int range = (int)(blockIdx.x % A.R);
    const int64_t s0 = tile * A.bs;
    const int cap = A.cap, m = A.m, D = A.D;
    int lg_cap = 7;
    while ((1 << lg_cap) < cap) ++lg_cap;
    int64_t v_begin = (int64_t)range * A.chunk;
    if (v_begin > A.n) v_begin = A.n;
    const int64_t v_end = v_begin + A.chunk < A.n ? v_begin + A.chunk : A.n;

    if (threadIdx.x < SIM_TILE) {
        const int t = threadIdx.x;
        const int64_t s = s0 + t;
        bool live = t < A.bs && s < A.S;
        int64_t self = -1, e0 = 0, e1 = 0;
        if (live && A.src_ids) {
            const int64_t u = A.src_ids[s];
            live = (uint64_t)u < (uint64_t)A.n;     // an id outside [0, n) has no eligible node
            if (live) {
                if (A.exclude_self) self = u;
                if (A.exc_rowptr) {
                    e0 = A.exc_rowptr[u];
                    e1 = A.exc_rowptr[u + 1];
                }
            }
        }
        thr[t] = live ? 0ull : ~0ull;               // no key beats ~0: a dead row never appends
        sh_self[t] = self;
        sh_e0[t] = e0;
        sh_e1[t] = e1;
        cnt[t] = 0;
    }
    if (threadIdx.x == 0) sh_full = 0;

    // this lane's query row (A operand) and the rows its four results belong to
    const int64_t qrow = s0 + j < A.S ? s0 + j : A.S - 1;
    const float *qp = A.Q + qrow * A.ldq;
    f32x4s qr[NG > 0 ? NG : 1];
    if constexpr (NG > 0) {
#pragma unroll
        for (int g = 0; g < NG; ++g) qr[g] = sim_load4(qp, 16 * g + 4 * q, D);
    }
    float qs[4] = {1.f, 1.f, 1.f, 1.f};
    if (A.q_scale) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t s = s0 + 4 * q + r;
            qs[r] = A.q_scale[s < A.S ? s : A.S - 1];
        }
    }
    __syncthreads();

    auto sort_and_keep = [&]() {                    // workgroup-uniform; ends with a barrier
        const int total = A.bs * cap;
        for (int e = threadIdx.x; e < total; e += SIM_BLOCK)
            if ((e & (cap - 1)) >= cnt[e >> lg_cap]) keys[e] = 0ull;
        __syncthreads();
        sim_sort_desc(keys, total, cap);
        if (threadIdx.x < A.bs) {
            const int t = threadIdx.x;
            const int c = cnt[t] < m ? cnt[t] : m;
            cnt[t] = c;
            if (c >= m) thr[t] = keys[t * cap + m - 1];
        }
        if (threadIdx.x == 0) sh_full = 0;
        __syncthreads();
    };

    for (int64_t r0 = v_begin; r0 < v_end; r0 += SIM_ROUND) {     // workgroup-uniform trip count, bounded by n
        const int64_t v = r0 + 16 * wave + j;
        const int64_t vrow = v < A.n ? v : A.n - 1;
        const float *tp = A.T + vrow * A.ldt;
        f32x4s acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        if constexpr (NG > 0) {
            f32x4s tr[NG];
#pragma unroll
            for (int g = 0; g < NG; ++g) tr[g] = sim_load4(tp, 16 * g + 4 * q, D);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (16 * g < D) {                   // wave-uniform
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(qr[g][0], tr[g][0], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(qr[g][1], tr[g][1], acc1, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(qr[g][2], tr[g][2], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(qr[g][3], tr[g][3], acc1, 0, 0, 0);
                }
            }
        } else {
            for (int k0 = 0; k0 < D; k0 += 64) {    // four k-groups at a time, both operands from memory
                f32x4s qa[4], tr[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    qa[g] = sim_load4(qp, k0 + 16 * g + 4 * q, D);
                    tr[g] = sim_load4(tp, k0 + 16 * g + 4 * q, D);
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[g][0], tr[g][0], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[g][1], tr[g][1], acc1, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[g][2], tr[g][2], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[g][3], tr[g][3], acc1, 0, 0, 0);
                }
            }
        }
        // lane (j, q) holds score(source 4 q + r, node v) in register r
        const float ts = A.t_scale ? A.t_scale[vrow] : 1.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int sl = 4 * q + r;
            float sc = __fadd_rn(acc0[r], acc1[r]);
            if (A.q_scale) sc = __fmul_rn(__fmul_rn(sc, qs[r]), ts);
            const uint64_t key = sim_key(sc, (uint32_t)v);
            if (v < v_end && key > thr[sl]) {
                bool ok = v != sh_self[sl];
                const int64_t e0 = sh_e0[sl], e1 = sh_e1[sl];
                if (ok && e1 > e0) ok = !lpf_sorted_has(A.exc_col, e0, e1, (int32_t)v);
                if (ok) {
                    const int slot = atomicAdd(&cnt[sl], 1);
                    if (slot < cap) keys[sl * cap + slot] = key;     // (always: see the flag below)
                    if (slot + 1 > cap - SIM_ROUND) sh_full = 1;     // the next round might not fit
                }
            }
        }
        __syncthreads();
        const bool full = sh_full != 0;
        __syncthreads();                            // every wavefront has read the flag before the next round sets it
        if (full) sort_and_keep();
    }
    sort_and_keep();

    for (int e = threadIdx.x; e < A.bs * m; e += SIM_BLOCK) {
        const int t = e / m, r = e - t * m;
        const int64_t s = s0 + t;
        if (s < A.S) A.ws[(s * A.R + range) * m + r] = r < cnt[t] ? keys[t * cap + r] : 0ull;
    }
}

__global__ __launch_bounds__(SIM_BLOCK) void similar_merge_kernel(int32_t R, int32_t m, const uint64_t *__restrict__ ws,
                                                                  int64_t *__restrict__ ids, float *__restrict__ scores,
                                                                  int64_t *__restrict__ counts) {
    __shared__ uint64_t keys[SIM_KEYS];
    __shared__ int32_t sh_fill;
    const int64_t s = blockIdx.x;
    const int64_t total = (int64_t)R * m;
    const uint64_t *w = ws + s * total;
    // sort the `fill` collected keys, keep m (workgroup-uniform; ends with a barrier); returns the number kept
    auto sort_and_keep = [&](int fill) {
        int p = 2;
        while (p < fill) p <<= 1;
        for (int i = fill + threadIdx.x; i < p; i += SIM_BLOCK) keys[i] = 0ull;
        __syncthreads();
        sim_sort_desc(keys, p, p);
        const int k = fill < m ? fill : m;
        if (threadIdx.x == 0) sh_fill = k;
        __syncthreads();
        return k;
    };
    int fill = 0;                                   // keys collected so far: the same in every thread
    uint64_t thr = 0ull;                            // the m-th best key at the last sort (0: fewer than m yet)
    if (threadIdx.x == 0) sh_fill = 0;
    __syncthreads();
    for (int64_t pos = 0; pos < total; pos += SIM_MERGE_TAKE) {
        const int take = (int)(total - pos < SIM_MERGE_TAKE ? total - pos : SIM_MERGE_TAKE);
        if (fill + take > SIM_KEYS) {               // the pass might not fit: afterwards fill <= m <= SIM_KEYS - take
            fill = sort_and_keep(fill);
            if (fill >= m) thr = keys[m - 1];
        }
        for (int i = threadIdx.x; i < take; i += SIM_BLOCK) {
            const uint64_t key = w[pos + i];
            if (key > thr) {                        // (padding is 0; a key at or below thr has m better ones already)
                const int slot = atomicAdd(&sh_fill, 1);
                if (slot < SIM_KEYS) keys[slot] = key;   // (always: fill + take <= SIM_KEYS)
            }
        }
        __syncthreads();
        fill = sh_fill < SIM_KEYS ? sh_fill : SIM_KEYS;
        __syncthreads();                            // every wavefront has read the counter before the next pass adds to it
    }
    const int kept = sort_and_keep(fill);
    for (int e = threadIdx.x; e < m; e += SIM_BLOCK) {
        if (e < kept) {
            const uint64_t key = keys[e];
            ids[s * m + e] = (int64_t)(uint32_t)~(uint32_t)key;
            scores[s * m + e] = sim_key_score(key);
        } else {
            ids[s * m + e] = -1;
            scores[s * m + e] = -__builtin_inff();
        }
    }
    if (threadIdx.x == 0) counts[s] = kept;
}

}  // namespace

extern "C" int64_t lpf_similar_workspace_bytes(int64_t S, int32_t m, int32_t n_ranges) {
    if (S < 0 || S >= INT32_MAX || m < 1 || m > LPF_SIMILAR_MAX_M || n_ranges == 0 || n_ranges > SIM_MAX_RANGES)
        return LPF_ERR_INVALID;
    return S * sim_ranges(S, m, n_ranges) * m * (int64_t)sizeof(uint64_t);
}

extern "C" int lpf_similar_topm_f32(int64_t S, int64_t n, int32_t D, const float *Q, int64_t ldq, const float *T,
                                    int64_t ldt, const float *q_scale, const float *t_scale, const int64_t *src_ids,
                                    const int64_t *exc_rowptr, const int32_t *exc_col, int32_t exclude_self, int32_t m,
                                    int32_t n_ranges, void *workspace, int64_t *ids, float *scores, int64_t *counts,
                                    void *stream) {
    if (S == 0) return LPF_OK;
    LPF_REQUIRE(S > 0 && S < INT32_MAX && n >= 1 && n < INT32_MAX && D >= 1 && m >= 1 && m <= LPF_SIMILAR_MAX_M &&
                n_ranges != 0 && n_ranges <= SIM_MAX_RANGES);
    LPF_REQUIRE(Q && T && workspace && ids && scores && counts && ldq >= D && ldt >= D && ldq % 4 == 0 && ldt % 4 == 0 &&
                lpf_aligned16(Q) && lpf_aligned16(T) && (q_scale == nullptr) == (t_scale == nullptr));
    // (exc_col may be NULL beside exc_rowptr: a graph without entries; it is read only inside a non-empty row)
    if (D > SIM_MAX_D) return LPF_ERR_UNSUPPORTED;
    SimArgs A;
    A.S = S; A.n = n; A.D = D;
    A.Q = Q; A.ldq = ldq; A.T = T; A.ldt = ldt;
    A.q_scale = q_scale; A.t_scale = t_scale;
    A.src_ids = src_ids;
    A.exc_rowptr = src_ids ? exc_rowptr : nullptr;
    A.exc_col = exc_col;
    A.exclude_self = exclude_self != 0;
    A.m = m;
    A.R = (int32_t)sim_ranges(S, m, n_ranges);
    A.bs = sim_bs(m);
    A.cap = sim_cap(m);
    const int64_t per = (n + A.R - 1) / A.R;
    A.chunk = (per + SIM_ROUND - 1) / SIM_ROUND * SIM_ROUND;
    A.ws = static_cast<uint64_t *>(workspace);
    const int64_t tiles = (S + A.bs - 1) / A.bs;
    if (tiles * A.R >= INT32_MAX) return LPF_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(tiles * A.R)), block(SIM_BLOCK);
    if (D <= 64) hipLaunchKernelGGL(similar_scan_kernel<4>, grid, block, 0, st, A);
    else if (D <= 128) hipLaunchKernelGGL(similar_scan_kernel<8>, grid, block, 0, st, A);
    else if (D <= 256) hipLaunchKernelGGL(similar_scan_kernel<16>, grid, block, 0, st, A);
    else hipLaunchKernelGGL(similar_scan_kernel<0>, grid, block, 0, st, A);
    LPF_CHECK_LAUNCH();
    hipLaunchKernelGGL(similar_merge_kernel, dim3((unsigned)S), block, 0, st, A.R, m,
                       static_cast<const uint64_t *>(A.ws), ids, scores, counts);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}
