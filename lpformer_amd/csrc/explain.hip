// Per-pair attention attribution (lpf_pair_explain_f32; lpformer_amd/explain.py): the segmented reduction
// that turns the attention scores of lpf_pair_scores_f32 into an explanation of every pair.
//
// Input is the reference layout lpf_select_export leaves (type-major: all CN entries sorted by (pair, node), then all
// 1-hop, then all >1-hop; int64 segment pointers relative per type) plus one score per entry.  Per pair, over the UNION
// of its up to three segments (i = 0 .. n-1: its CN entries, then its 1-hop entries, then its >1-hop entries):
//   alpha_i  = exp(s_i - max_j s_j) / (sum_j exp(s_j - max_j s_j) + 1e-16)      PyG segment softmax (layers.py:220)
//   mass[t]  = sum of alpha over the entries of type t ;  entropy = -sum alpha ln alpha  (nats; alpha = 0 adds 0)
//   top-m    = the m entries with the largest alpha, ties to the smaller node id, a NaN alpha last
//   all list = (node, type, alpha) of every entry, pair-major (optional)
//
// Shape.  A wavefront takes a pair (four pairs per 256-thread workgroup, wave-stride loop over the batch); a pair with
// more than EX_HEAVY entries is put on a list instead and taken by a whole workgroup in a second launch, as
// lpf_pair_softmax_gather_f32 does.  The NT = 64 or 256 lanes of a pair stride its entries:
//   1. max of the scores (butterfly), 2. sum of exp (per-lane partial sums, butterfly), 3. alpha per entry: masses and
//   entropy the same way, the all list written on the way, 4. top-m by m rounds of "largest key below the last one":
//   an entry's key is (alpha bits + 1 | NaN -> 0) << 32 | ~node -- unsigned order = (alpha descending, node ascending, NaN
//   last), keys of a pair are distinct (a node occurs once per pair), 0 means "none".  Every lane keeps the keys of its
//   first EX_KEYS entries in registers (a wavefront: pairs up to 256 entries never compute a key twice); the lane that
//   holds the round's winner writes that slot, so no payload travels through the reduction.
// Sums are accumulated in fp64 (full rate on gfx950) and rounded once, so a result does not depend on how many lanes
// shared the pair beyond that rounding; there are no float atomics, and the one integer atomic (appending to the heavy
// list) only decides the ORDER in which heavy pairs are taken.  Nothing is read back; entry counts come from type_ptr.
#include "lpf_common.h"

namespace {

constexpr int EX_BLOCK = 256;    // 4 wavefronts
constexpr int EX_HEAVY = 1024;   // entries of a pair above which a whole workgroup takes it
constexpr int EX_KEYS = 4;       // keys a lane keeps in registers
constexpr int EX_MAX_TOP = 32;

struct ExOut {
    float *mass, *entropy;
    int64_t *top_node;
    float *top_w;
    int8_t *top_type;
    float *top_pa, *top_pb;
    int64_t *all_node;
    int8_t *all_type;
    float *all_w;
};

struct ExSeg {        // a pair's three segments as positions in the type-major arrays
    int64_t beg[3];
    int cnt[3];
    int n;
    int64_t all_off;  // first entry of the pair in the pair-major list
};

// position in the type-major arrays (and the type, 0..2) of entry i of the pair's union
__device__ __forceinline__ int64_t ex_locate(const ExSeg &sg, int i, int &t) {
    const int c0 = sg.cnt[0], c01 = sg.cnt[0] + sg.cnt[1];
    t = (i >= c0 ? 1 : 0) + (i >= c01 ? 1 : 0);
    return t == 0 ? sg.beg[0] + i : (t == 1 ? sg.beg[1] + (i - c0) : sg.beg[2] + (i - c01));   // (static indices)
}

__device__ __forceinline__ float ex_alpha(float s, float m, float den) { return expf(s - m) / den; }

__device__ __forceinline__ unsigned long long ex_key(float alpha, int32_t node) {
    const uint32_t a = (alpha != alpha) ? 0u : __float_as_uint(alpha) + 1u;   // alpha >= +0 when it is a number
    return ((unsigned long long)a << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)node);
}

// Reductions over the NT lanes that share a pair: one wavefront (butterfly alone) or the workgroup (the four wave results
// meet in LDS and are combined in wave order).
template <int NT>
__device__ __forceinline__ float ex_max_f(float v, float *red) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    if constexpr (NT > 64) {
        __syncthreads();   // red[] free: everyone has read its previous use
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    }
    return v;
}
template <int NT>
__device__ __forceinline__ double ex_sum_d(double v, double *red) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    if constexpr (NT > 64) {
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        v = (red[0] + red[1]) + (red[2] + red[3]);
    }
    return v;
}
template <int NT>
__device__ __forceinline__ unsigned long long ex_max_u(unsigned long long v, unsigned long long *red) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m, 64);
        v = o > v ? o : v;
    }
    if constexpr (NT > 64) {
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        const unsigned long long a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
        v = a > b ? a : b;
    }
    return v;
}

__device__ __forceinline__ ExSeg ex_segments(int64_t p, int64_t bs, const int64_t *__restrict__ type_ptr,
                                             int64_t max_entries) {
    const int64_t tot0 = type_ptr[bs], tot1 = type_ptr[(bs + 1) + bs];
    const int64_t tbase[3] = {0, tot0, tot0 + tot1};
    ExSeg sg;
    sg.all_off = 0;
    sg.n = 0;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int64_t lo = type_ptr[t * (bs + 1) + p], hi = type_ptr[t * (bs + 1) + p + 1];
        sg.all_off += lo;
        sg.beg[t] = tbase[t] + lo;
        // (never past the capacity the caller gave, whatever the pointers say)
        int64_t c = hi - lo;
        if (sg.beg[t] < 0 || sg.beg[t] >= max_entries) c = 0;
        else if (c > max_entries - sg.beg[t]) c = max_entries - sg.beg[t];
        sg.cnt[t] = c > 0 ? (int)c : 0;
        sg.n += sg.cnt[t];
    }
    return sg;
}

// One pair by NT lanes (tid = 0 .. NT-1).  Every lane of the group runs this with the same sg.
template <int NT>
__device__ __forceinline__ void ex_pair(int64_t p, const ExSeg &sg, int tid, const int32_t *__restrict__ sel_node,
                                        const float *__restrict__ sel_pa, const float *__restrict__ sel_pb,
                                        const float *__restrict__ score, int64_t max_entries, int top, const ExOut &o,
                                        float *red_f, double *red_d, unsigned long long *red_u) {
    const int n = sg.n;
    int t;
    float m = -INFINITY;
    for (int i = tid; i < n; i += NT) m = fmaxf(m, score[ex_locate(sg, i, t)]);
    m = ex_max_f<NT>(m, red_f);
    double acc = 0.0;
    for (int i = tid; i < n; i += NT) acc += (double)expf(score[ex_locate(sg, i, t)] - m);
    const float den = (float)ex_sum_d<NT>(acc, red_d) + 1e-16f;

    double ms[3] = {0.0, 0.0, 0.0}, ent = 0.0;
    const bool want_all = o.all_w != nullptr;
    for (int i = tid; i < n; i += NT) {
        const int64_t g = ex_locate(sg, i, t);
        const float a = ex_alpha(score[g], m, den);
        ms[0] += t == 0 ? (double)a : 0.0;
        ms[1] += t == 1 ? (double)a : 0.0;
        ms[2] += t == 2 ? (double)a : 0.0;
        ent += (double)(a == 0.f ? 0.f : a * logf(a));
        if (want_all && sg.all_off + i < max_entries) {
            o.all_node[sg.all_off + i] = (int64_t)sel_node[g];
            o.all_type[sg.all_off + i] = (int8_t)(t + 1);
            o.all_w[sg.all_off + i] = a;
        }
    }
    ms[0] = ex_sum_d<NT>(ms[0], red_d);
    ms[1] = ex_sum_d<NT>(ms[1], red_d);
    ms[2] = ex_sum_d<NT>(ms[2], red_d);
    ent = ex_sum_d<NT>(ent, red_d);
    if (tid == 0) {
        o.mass[3 * p + 0] = (float)ms[0];
        o.mass[3 * p + 1] = (float)ms[1];
        o.mass[3 * p + 2] = (float)ms[2];
        o.entropy[p] = (float)(0.0 - ent);
    }

    // top-m: round r finds the largest key below the winner of round r - 1
    unsigned long long kc[EX_KEYS];
#pragma unroll
    for (int c = 0; c < EX_KEYS; ++c) {
        const int i = tid + c * NT;
        kc[c] = 0ull;
        if (i < n) {
            const int64_t g = ex_locate(sg, i, t);
            kc[c] = ex_key(ex_alpha(score[g], m, den), sel_node[g]);
        }
    }
    unsigned long long prev = ~0ull;
    int r = 0;
    for (; r < top; ++r) {
        unsigned long long best = 0ull;
        int bi = -1;
#pragma unroll
        for (int c = 0; c < EX_KEYS; ++c)
            if (kc[c] < prev && kc[c] > best) {
                best = kc[c];
                bi = tid + c * NT;
            }
        for (int i = tid + EX_KEYS * NT; i < n; i += NT) {
            const int64_t g = ex_locate(sg, i, t);
            const unsigned long long k = ex_key(ex_alpha(score[g], m, den), sel_node[g]);
            if (k < prev && k > best) {
                best = k;
                bi = i;
            }
        }
        const unsigned long long win = ex_max_u<NT>(best, red_u);
        if (win == 0ull) break;          // (the same value in every lane of the group)
        if (best == win) {               // keys are distinct: exactly one lane
            const int64_t g = ex_locate(sg, bi, t);
            const int64_t slot = p * top + r;
            o.top_node[slot] = (int64_t)sel_node[g];
            o.top_w[slot] = ex_alpha(score[g], m, den);
            o.top_type[slot] = (int8_t)(t + 1);
            o.top_pa[slot] = sel_pa[g];
            o.top_pb[slot] = sel_pb[g];
        }
        prev = win;
    }
    for (int j = r + tid; j < top; j += NT) {   // padding
        const int64_t slot = p * top + j;
        o.top_node[slot] = -1;
        o.top_w[slot] = 0.f;
        o.top_type[slot] = 0;
        o.top_pa[slot] = 0.f;
        o.top_pb[slot] = 0.f;
    }
}

__global__ __launch_bounds__(EX_BLOCK) void pair_explain_kernel(
    int64_t bs, const int64_t *__restrict__ type_ptr, const int32_t *__restrict__ sel_node,
    const float *__restrict__ sel_pa, const float *__restrict__ sel_pb, const float *__restrict__ score,
    int64_t max_entries, int top, ExOut o, int64_t *__restrict__ all_ptr, int32_t *__restrict__ heavy) {
    const int lane = lpf_lane();
    const int64_t wave_id = (int64_t)blockIdx.x * (EX_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * (EX_BLOCK / 64);
    for (int64_t p = wave_id; p < bs; p += n_waves) {
        const ExSeg sg = ex_segments(p, bs, type_ptr, max_entries);
        if (all_ptr && lane == 0) {
            all_ptr[p] = sg.all_off;
            if (p == bs - 1)
                all_ptr[bs] = type_ptr[bs] + type_ptr[(bs + 1) + bs] + type_ptr[2 * (bs + 1) + bs];
        }
        if (sg.n > EX_HEAVY) {   // left to pair_explain_heavy_kernel
            if (lane == 0) heavy[1 + atomicAdd(&heavy[0], 1)] = (int32_t)p;   // any order: pairs are independent
            continue;
        }
        ex_pair<64>(p, sg, lane, sel_node, sel_pa, sel_pb, score, max_entries, top, o, nullptr, nullptr, nullptr);
    }
}

__global__ __launch_bounds__(EX_BLOCK) void pair_explain_heavy_kernel(
    int64_t bs, const int64_t *__restrict__ type_ptr, const int32_t *__restrict__ sel_node,
    const float *__restrict__ sel_pa, const float *__restrict__ sel_pb, const float *__restrict__ score,
    int64_t max_entries, int top, ExOut o, const int32_t *__restrict__ heavy) {
    __shared__ float red_f[4];
    __shared__ double red_d[4];
    __shared__ unsigned long long red_u[4];
    const int n_heavy = heavy[0];
    for (int h = blockIdx.x; h < n_heavy; h += gridDim.x) {   // list written by the launch in front
        const int64_t p = heavy[1 + h];
        const ExSeg sg = ex_segments(p, bs, type_ptr, max_entries);
        ex_pair<EX_BLOCK>(p, sg, (int)threadIdx.x, sel_node, sel_pa, sel_pb, score, max_entries, top, o, red_f, red_d,
                          red_u);
    }
}

}  // namespace

extern "C" int lpf_pair_explain_f32(int64_t bs, const int64_t *type_ptr, const int32_t *sel_node, const float *sel_pa,
                                    const float *sel_pb, const float *score, int64_t max_entries, int32_t top,
                                    float *mass, float *entropy, int64_t *top_node, float *top_w, int8_t *top_type,
                                    float *top_pa, float *top_pb, int64_t *all_ptr, int64_t *all_node,
                                    int8_t *all_type, float *all_w, int32_t *heavy_scratch, void *stream) {
    LPF_REQUIRE(top >= 1 && top <= EX_MAX_TOP && bs >= 0 && bs < (1ll << 31) && max_entries >= 0 &&
                max_entries < (1ll << 31));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (bs == 0) {
        if (all_ptr) (void)hipMemsetAsync(all_ptr, 0, sizeof(int64_t), s);
        return LPF_OK;
    }
    LPF_REQUIRE(type_ptr && mass && entropy && top_node && top_w && top_type && top_pa && top_pb && heavy_scratch);
    LPF_REQUIRE(max_entries == 0 || (sel_node && sel_pa && sel_pb && score));
    // the pair-major list: wanted iff all_ptr is given, then all four arrays
    LPF_REQUIRE(all_ptr == nullptr || max_entries == 0 || (all_node && all_type && all_w));
    ExOut o{mass, entropy, top_node, top_w, top_type, top_pa, top_pb, all_node, all_type,
            (all_ptr && max_entries > 0) ? all_w : nullptr};
    (void)hipMemsetAsync(heavy_scratch, 0, sizeof(int32_t), s);   // heavy-pair counter
    int64_t blocks = (bs + (EX_BLOCK / 64) - 1) / (EX_BLOCK / 64);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(pair_explain_kernel, dim3((unsigned)blocks), dim3(EX_BLOCK), 0, s, bs, type_ptr, sel_node, sel_pa,
                       sel_pb, score, max_entries, (int)top, o, all_ptr, heavy_scratch);
    const int64_t hblocks = bs < 1024 ? bs : 1024;
    hipLaunchKernelGGL(pair_explain_heavy_kernel, dim3((unsigned)hblocks), dim3(EX_BLOCK), 0, s, bs, type_ptr, sel_node,
                       sel_pa, sel_pb, score, max_entries, (int)top, o, heavy_scratch);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}
