// Shared helpers for the gfx950 kernels (wave = 64 lanes everywhere).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lpformer_hip.h"

#define LPF_WAVE 64

void lpf_set_hip_error(hipError_t e);

// Launch facts are cached PER DEVICE: one process may drive several GPUs, from several host threads.  The guarded
// actions (hipFuncSetAttribute, an occupancy query) are idempotent, so relaxed atomics are enough -- two threads doing
// one of them twice is harmless, launching without it is not (function-local `static bool` caches).
#include <atomic>
constexpr int LPF_MAX_DEVICES = 64;
struct LpfPerDevice {
    std::atomic<int> v[LPF_MAX_DEVICES];
};
int lpf_current_device();                                             // -1: none (or an ordinal beyond the cache)
int lpf_cu_count();                                                   // CUs of the current device; 0: no device
int lpf_set_max_lds(LpfPerDevice &once, const void *kern, int bytes);  // hipFuncAttributeMaxDynamicSharedMemorySize
// resident workgroups per CU of `kern` (occupancy query, cached); `fallback` when the query fails
int lpf_blocks_per_cu(LpfPerDevice &cache, const void *kern, int threads, size_t lds, int fallback);

#define LPF_SET_MAX_LDS(kern, lds)                                                                       \
    do {                                                                                                 \
        static LpfPerDevice once__;                                                                      \
        if ((lds) > 64 * 1024) {                                                                         \
            const int rc__ = lpf_set_max_lds(once__, reinterpret_cast<const void *>(kern), (int)(lds));  \
            if (rc__ != LPF_OK) return rc__;                                                             \
        }                                                                                                \
    } while (0)

#define LPF_CHECK_LAUNCH()                      \
    do {                                        \
        hipError_t e__ = hipGetLastError();     \
        if (e__ != hipSuccess) {                \
            lpf_set_hip_error(e__);             \
            return LPF_ERR_LAUNCH;              \
        }                                       \
    } while (0)

#define LPF_REQUIRE(cond)                 \
    do {                                  \
        if (!(cond)) return LPF_ERR_INVALID; \
    } while (0)

static inline bool lpf_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// zero the counter in front of a long list (scratch[0]) on stream s
static inline int lpf_reset_counter(int32_t *scratch, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(scratch, 0, sizeof(int32_t), s);
    if (e == hipSuccess) return LPF_OK;
    lpf_set_hip_error(e);
    return LPF_ERR_LAUNCH;
}

__device__ __forceinline__ int lpf_lane() { return (int)(threadIdx.x & 63); }

// xor-butterfly reductions over the low `WIDTH` lanes of each aligned group (WIDTH power of two <= 64)
template <int WIDTH>
__device__ __forceinline__ float lpf_group_sum(float v) {
#pragma unroll
    for (int m = WIDTH >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
template <int WIDTH>
__device__ __forceinline__ float lpf_group_max(float v) {
#pragma unroll
    for (int m = WIDTH >> 1; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

// sum over the four lanes {l, l ^ 16, l ^ 32, l ^ 48}: the lanes that share a row / a sample in the MFMA tile layouts
__device__ __forceinline__ float lpf_quad_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// Sum over the G lanes of a group, the same bits in every lane: DPP butterflies inside a row of 16 lanes (quad
// permutes, then the half-row and the row mirrored: after two steps a quad holds one value, so a mirror IS the xor
// partner), one swizzle across the rows, one pair of lane reads across the halves -- no LDS round trip per step
// (__shfl_xor compiles to ds_bpermute_b32: five dependent round trips per entry were a third of the flip kernel).
template <int CTRL>
__device__ __forceinline__ float lpf_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
template <int G>
__device__ __forceinline__ float lpf_dpp_group_sum(float v) {
    v += lpf_dpp<0xB1>(v);                   // quad_perm [1,0,3,2]
    v += lpf_dpp<0x4E>(v);                   // quad_perm [2,3,0,1]
    if constexpr (G >= 8) v += lpf_dpp<0x141>(v);    // row_half_mirror
    if constexpr (G >= 16) v += lpf_dpp<0x140>(v);   // row_mirror
    if constexpr (G >= 32)
        v += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401f));  // lane ^ 16
    if constexpr (G >= 64) {
        const float a = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
        const float b = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32));
        v = a + b;
    }
    return v;
}

// Workgroup barrier that orders LDS ONLY.  __syncthreads() is a workgroup-scope fence + barrier, and the fence makes the
// compiler drain the vector-memory counter -- loads and stores included -- in front of every barrier: in select3's run
// kernel that turned each of the item loop's thirteen barriers into a wait for whatever global reads were in flight
// (in-kernel stamps: ~2 us per dependent round trip, seven of them per item), and behind a loop of global stores every
// barrier waits out a store round trip.
// INVARIANT of every kernel that calls this: no wavefront hands GLOBAL data to another wavefront of its workgroup
// across this barrier.  What a workgroup does pass through global memory carries its own wait (pair_rows' pieces: wait
// + flag) or leaves the workgroup through agent-scope atomics (select3, select4).  So the barrier only has to order
// LDS, and the global loads, stores and atomics requested ahead stay in flight across it.
__device__ __forceinline__ void lpf_lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// The reference's fp32 round trip fl32((fl32(fl32(p*t)+t)-t)/t) for t in {1, 2}: p*1, p*2, x/1 and x/2 are exact, only
// the add and the subtract round -- op by op, never a fused multiply-add
__device__ __forceinline__ float lpf_rt1(float p) {
#pragma clang fp contract(off)
    return __fsub_rn(__fadd_rn(p, 1.0f), 1.0f);
}
__device__ __forceinline__ float lpf_rt2(float p) {
#pragma clang fp contract(off)
    return 0.5f * __fsub_rn(__fadd_rn(p * 2.0f, 2.0f), 2.0f);
}

// 11-bit multiplicative hash of a node id (the 2,048-slot LDS tables of neg_sample.hip and twohop.hip)
__device__ __forceinline__ uint32_t lpf_hash11(int32_t c) { return ((uint32_t)c * 2654435761u) >> 21; }

// first index i in [lo, hi) with a[i] >= key (a sorted ascending); returns hi if none
__device__ __forceinline__ int64_t lpf_lower_bound(const int32_t *__restrict__ a, int64_t lo, int64_t hi, int32_t key) {
    while (lo < hi) {
        int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// whether the sorted row col[lo, hi) holds key
__device__ __forceinline__ bool lpf_sorted_has(const int32_t *__restrict__ col, int64_t lo, int64_t hi, int32_t key) {
    const int64_t i = lpf_lower_bound(col, lo, hi, key);
    return i < hi && col[i] == key;
}

// The sorted-row intersection of a pair (pair_heuristics.hip, node_structure.hip): the pair walks its SHORTER row (on
// equal lengths the row of min(a, b)) and binary-searches each walked column in the other row.
struct LpfPairRows {
    int64_t r0, q0;   // first entry of the walked row / the probed row
    int32_t len, qlen;
};

// The walked and the probed row of (a, b); both empty when an id lies outside [0, n).
__device__ __forceinline__ LpfPairRows lpf_pair_rows(int64_t a, int64_t b, int64_t n,
                                                     const int64_t *__restrict__ rowptr) {
    LpfPairRows r{0, 0, 0, 0};
    if ((uint64_t)a >= (uint64_t)n || (uint64_t)b >= (uint64_t)n) return r;
    const int64_t a0 = rowptr[a], a1 = rowptr[a + 1], b0 = rowptr[b], b1 = rowptr[b + 1];
    const int64_t da = a1 - a0, db = b1 - b0;
    const bool walk_a = da < db || (da == db && a <= b);
    r.r0 = walk_a ? a0 : b0;
    r.len = (int32_t)(walk_a ? da : db);
    r.q0 = walk_a ? b0 : a0;
    r.qlen = (int32_t)(walk_a ? db : da);
    return r;
}

// The flagged lanes of a wave append `item` to list[1 ..]; list[0] counts the entries: one ticket per wave, its lanes
// take consecutive slots.  Call it wave-uniformly.
__device__ __forceinline__ void lpf_wave_list_push(int32_t *__restrict__ list, bool flag, int32_t item) {
    const uint64_t m = __ballot(flag);
    if (!m) return;
    const int lane = lpf_lane();
    int base = 0;
    if (lane == 0) base = atomicAdd(&list[0], __popcll(m));
    base = __shfl(base, 0);
    if (flag) list[1 + base + __popcll(m & ((1ull << lane) - 1ull))] = item;
}

// fp32 <-> bf16 bits (round to nearest even; NaN stays NaN)
__device__ __forceinline__ uint16_t lpf_f32_to_bf16(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__device__ __forceinline__ float lpf_bf16_to_f32(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }

// Dropout inside a kernel (the training forward of the fused GCN layer and its LayerNorm/ReLU backward): element (row,
// col) of a launch with 64-bit seed s is KEPT iff lpf_drop_bits(row key, col, s) >= threshold, threshold =
// lpf_drop_threshold(p) -- a counter-based hash (two lowbias32 rounds), so the backward recomputes the forward's mask
// from (seed, row, col) and no mask tensor exists.  Reference: F.dropout(x, p, training=True) behind every GCN layer
// (src/models/other_models.py:69): Bernoulli(1 - p) keeps scaled by 1 / (1 - p); which elements are kept is random
// there as here (parity is distributional: tests/test_gpu_train.py), p is met to 2^-32.
__host__ __device__ __forceinline__ uint32_t lpf_mix32(uint32_t h) {
    h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
    return h;
}
__host__ __device__ __forceinline__ uint32_t lpf_drop_row_key(int64_t row, uint64_t seed) {
    return lpf_mix32((uint32_t)row * 0x9E3779B1u + (uint32_t)seed) ^ (uint32_t)((uint64_t)row >> 32);
}
__host__ __device__ __forceinline__ uint32_t lpf_drop_bits(uint32_t row_key, int col, uint64_t seed) {
    return lpf_mix32(row_key + (uint32_t)col * 0x85EBCA77u + (uint32_t)(seed >> 32));
}
static inline uint32_t lpf_drop_threshold(float p) {   // keep iff bits >= threshold: P(drop) = threshold / 2^32
    const double t = (double)p * 4294967296.0;
    return t <= 0.0 ? 0u : (t >= 4294967295.0 ? 4294967295u : (uint32_t)t);
}

// Padding draw d of node u (lpf_rank_interleave; restated in include/lpformer_hip.h): plain uint32 arithmetic.
__host__ __device__ __forceinline__ uint32_t lpf_pad_draw(uint64_t seed, int64_t u, uint32_t d, uint32_t n) {
    uint32_t x = lpf_mix32((uint32_t)u * 0x9E3779B1u + (uint32_t)seed);
    x = lpf_mix32(x ^ (uint32_t)(seed >> 32) ^ (d * 0x85EBCA77u));
    return x % n;
}
