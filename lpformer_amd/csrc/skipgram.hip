// Node2Vec's skip-gram update with negative sampling: lpf_skipgram_coef_f32, lpf_skipgram_grad_rows_f32
// and lpf_sparse_adam_rows_f32.  The contract is restated in include/lpformer_hip.h and in lpformer_amd/skipgram.py,
// whose skipgram_reference is the fp64 restatement the kernels are tested against.
//
// A step is synchronous: every gradient is taken at the table as it stands when the step begins.  The three entries
// split it so that no row is read while another wavefront changes it, and so that every sum has ONE order:
//   coef       per pair the logit l = <E[c], E[x]> (fp32, one fixed order per dim), the coefficient g = dloss/dl with
//              the 1/Mp or 1/Mn scale folded in (evaluated in fp64 from that l, stored as fp32), the two ids, and the
//              loss as fp64: per lane, a fixed tree per workgroup, then one pass over the workgroups' sums.
//   grad_rows  grad[u] = sum over row u's occurrences, in the listed order, of g[pair] E[other]: a segment is cut at
//              multiples of LPF_SKIPGRAM_CHUNK from its own start, a chunk is summed in order by one wavefront, and
//              the partial rows are added in chunk order.  Reads the table, writes grad (and its scratch) only.
//   adam       SparseAdam's formulas on the U listed rows, in place.
// No float atomics, no atomics at all; nothing depends on the launch shape or on timing.  Every id read from a buffer is
// range-checked before it indexes anything: a pair with an id outside [0, n) has coefficient 0, loss 0 and the ids -1;
// an occurrence whose other or pair id is out of range adds nothing; a listed row outside [0, n) is not updated.
#include "lpf_common.h"

namespace {

constexpr int SG_BLOCK = 256;
constexpr int SG_GROUP = 16;                                   // lanes per window of the coef kernel
constexpr int SG_WINDOWS = LPF_SKIPGRAM_BLOCK_WINDOWS;         // windows per workgroup
static_assert(SG_WINDOWS * SG_GROUP == SG_BLOCK, "a workgroup is LPF_SKIPGRAM_BLOCK_WINDOWS groups of 16 lanes");
constexpr int SG_CHUNK = LPF_SKIPGRAM_CHUNK;
constexpr int SG_WAVES = SG_BLOCK / LPF_WAVE;
constexpr double SG_EPS = 1e-15;                               // PyG's Node2Vec.loss

struct CoefArgs {
    int64_t n;
    int32_t dim4;                                              // dim / 4
    const float *table;
    int64_t ldt;
    int32_t nwin, pairs_per_window;                            // L + 2 - context, context - 1
    const int32_t *pos, *neg;
    int64_t ldp, ldn;
    int64_t pos_windows, windows;                              // Wp nwin, (Wp + Wn) nwin
    double inv_mp, inv_mn;
    float *coef;
    int32_t *centre, *other;
    double *partial;
};

// One group of 16 lanes per window: the centre row stays in registers (NV float4 per lane), the partners are read one
// after the other.  The dot product has one order: lane s adds the elements 4 (s + 16 i) .. + 3, i ascending, then the
// butterfly over the 16 lanes, the same bits in every lane.  Lane t of the group keeps the logit of the window's pair
// k0 + t, so sixteen pairs' sigmoids and logarithms (fp64) are evaluated side by side and stored as one line.
template <int NV>
__global__ __launch_bounds__(SG_BLOCK) void skipgram_coef_kernel(CoefArgs A) {
    __shared__ double sums[SG_BLOCK];
    const int group = (int)(threadIdx.x / SG_GROUP), sub = (int)(threadIdx.x % SG_GROUP);
    const int64_t q = (int64_t)blockIdx.x * SG_WINDOWS + group;
    double loss = 0.0;
    if (q < A.windows) {
        const bool isneg = q >= A.pos_windows;
        const int64_t qq = isneg ? q - A.pos_windows : q;
        const int64_t w = qq / A.nwin, o = qq % A.nwin;
        const int32_t *buf = (isneg ? A.neg : A.pos) + w;
        const int64_t ld = isneg ? A.ldn : A.ldp;
        const double scale = isneg ? A.inv_mn : A.inv_mp;
        const int32_t c = buf[o * ld];
        const bool cok = (uint64_t)(uint32_t)c < (uint64_t)A.n;
        float4 cen[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int j = sub + SG_GROUP * i;
            cen[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (cok && j < A.dim4) cen[i] = reinterpret_cast<const float4 *>(A.table + (int64_t)c * A.ldt)[j];
        }
        const int64_t pair0 = q * A.pairs_per_window;          // the negative buffer's ids follow the positive one's
        for (int32_t k0 = 0; k0 < A.pairs_per_window; k0 += SG_GROUP) {
            const int kn = A.pairs_per_window - k0 < SG_GROUP ? A.pairs_per_window - k0 : SG_GROUP;
            // lane t reads the partner of pair k0 + t; an id outside [0, n) (or a bad centre) becomes -1 here
            int32_t my_x = -1;
            if (sub < kn) {
                const int32_t x = buf[(o + k0 + sub + 1) * ld];
                if (cok && (uint64_t)(uint32_t)x < (uint64_t)A.n) my_x = x;
            }
            float my_dot = 0.f;
            for (int t = 0; t < kn; ++t) {
                const int32_t x = __shfl(my_x, t, SG_GROUP);
                float dot = 0.f;
                if (x >= 0) {
                    const float4 *row = reinterpret_cast<const float4 *>(A.table + (int64_t)x * A.ldt);
#pragma unroll
                    for (int i = 0; i < NV; ++i) {
                        const int j = sub + SG_GROUP * i;
                        if (j < A.dim4) {
                            const float4 v = row[j];
                            dot = fmaf(cen[i].x, v.x, dot);
                            dot = fmaf(cen[i].y, v.y, dot);
                            dot = fmaf(cen[i].z, v.z, dot);
                            dot = fmaf(cen[i].w, v.w, dot);
                        }
                    }
                }
                dot = lpf_dpp_group_sum<SG_GROUP>(dot);
                if (sub == t) my_dot = dot;
            }
            if (sub < kn) {
                const int64_t id = pair0 + k0 + sub;
                float g = 0.f;
                if (my_x >= 0) {
                    // s = sigmoid(l) and 1 - s as the contract writes them, in fp64 from the fp32 logit
                    const double s = 1.0 / (1.0 + exp(-(double)my_dot));
                    const double om = 1.0 - s;
                    if (isneg) {
                        loss -= log(om + SG_EPS) * scale;
                        g = (float)(s * om / (om + SG_EPS) * scale);
                    } else {
                        loss -= log(s + SG_EPS) * scale;
                        g = (float)(-(s * om) / (s + SG_EPS) * scale);
                    }
                }
                A.coef[id] = g;
                A.centre[id] = my_x >= 0 ? c : -1;
                A.other[id] = my_x;
            }
        }
    }
    // the workgroup's sum in one order: a fixed tree over its 256 lanes
    sums[threadIdx.x] = loss;
    __syncthreads();
    for (int stride = SG_BLOCK / 2; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) sums[threadIdx.x] += sums[threadIdx.x + stride];
        __syncthreads();
    }
    if (threadIdx.x == 0) A.partial[blockIdx.x] = sums[0];
}

// *loss = the workgroups' sums in ONE order: thread t adds partial[t], partial[t + 256], ..., then a fixed tree.
__global__ __launch_bounds__(SG_BLOCK) void skipgram_loss_kernel(const double *__restrict__ partial, int64_t count,
                                                                 double *__restrict__ loss) {
    __shared__ double sums[SG_BLOCK];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < count; i += SG_BLOCK) s += partial[i];
    sums[threadIdx.x] = s;
    __syncthreads();
    for (int stride = SG_BLOCK / 2; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) sums[threadIdx.x] += sums[threadIdx.x + stride];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = sums[0];
}

struct GradArgs {
    int64_t n;
    int32_t dim4;
    const float *table;
    int64_t ldt;
    int64_t M;
    const float *coef;
    int64_t n_occ;
    const int32_t *occ_other, *occ_pair;
    int64_t U;
    const int64_t *seg;                                        // [U + 1]
    float *grad;
    int64_t ldg;
    float *scratch;                                            // [blocks of LPF_SKIPGRAM_CHUNK occurrences][ldg]
    int64_t items;                                             // ceil(n_occ / LPF_SKIPGRAM_CHUNK)
};

__device__ __forceinline__ int64_t sg_seg(const GradArgs &A, int64_t u) {     // clamped to [0, n_occ]
    const int64_t s = A.seg[u];
    return s < 0 ? 0 : (s > A.n_occ ? A.n_occ : s);
}

// first u in [0, U] with seg[u] >= key (U + 1 if none)
__device__ __forceinline__ int64_t sg_lower_bound(const GradArgs &A, int64_t key) {
    int64_t lo = 0, hi = A.U + 1;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (sg_seg(A, mid) < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// dst[0 .. dim) = the occurrences [a, b) in order, b - a <= LPF_SKIPGRAM_CHUNK: lane l owns the elements 4 l .. 4 l + 3
// (and 4 (l + 64) ..), each occurrence is one fused multiply-add per element.  The wavefront reads 64 occurrences'
// ids and coefficients at once, then requests four rows ahead of their adds.
template <int NV>
__device__ __forceinline__ void sg_sum_chunk(const GradArgs &A, int64_t a, int64_t b, float *__restrict__ dst) {
    const int lane = lpf_lane();
    float4 acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t base = a; base < b; base += LPF_WAVE) {
        const int cnt = (int)((b - base) < LPF_WAVE ? (b - base) : LPF_WAVE);
        int32_t my_o = -1;
        float my_g = 0.f;
        if (lane < cnt) {
            const int32_t o = A.occ_other[base + lane], p = A.occ_pair[base + lane];
            if ((uint64_t)(uint32_t)o < (uint64_t)A.n && (uint64_t)(uint32_t)p < (uint64_t)A.M) {
                my_o = o;
                my_g = A.coef[p];
            }
        }
        for (int e = 0; e < cnt; e += 4) {
            int32_t o[4];
            float g[4];
            float4 v[4][NV];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int src = e + t < cnt ? e + t : cnt - 1;
                o[t] = e + t < cnt ? __shfl(my_o, src) : -1;   // (e, cnt: the same in every lane)
                g[t] = __shfl(my_g, src);
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    const int j = lane + LPF_WAVE * i;
                    v[t][i] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (o[t] >= 0 && j < A.dim4)
                        v[t][i] = reinterpret_cast<const float4 *>(A.table + (int64_t)o[t] * A.ldt)[j];
                }
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (o[t] < 0) continue;                        // adds nothing, not g * 0
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    acc[i].x = fmaf(g[t], v[t][i].x, acc[i].x);
                    acc[i].y = fmaf(g[t], v[t][i].y, acc[i].y);
                    acc[i].z = fmaf(g[t], v[t][i].z, acc[i].z);
                    acc[i].w = fmaf(g[t], v[t][i].w, acc[i].w);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int j = lane + LPF_WAVE * i;
        if (j < A.dim4) reinterpret_cast<float4 *>(dst)[j] = acc[i];
    }
}

// Work item t = the occurrences' block [t CHUNK, (t + 1) CHUNK): its wavefront sums every chunk that STARTS there.
// Those are chunk 0 of every row whose segment starts in the block (into grad[u]) and at most one later chunk, of the
// row that started in front of the block (into scratch[t]: a later chunk starts CHUNK behind the one before it, so no
// two of them start in one block).  Every chunk of every row starts in exactly one block, so the items can be taken in
// any order by any number of wavefronts.
template <int NV>
__global__ __launch_bounds__(SG_BLOCK) void skipgram_grad_chunks_kernel(GradArgs A) {
    const int64_t wave = (int64_t)blockIdx.x * SG_WAVES + threadIdx.x / LPF_WAVE;
    const int64_t waves = (int64_t)gridDim.x * SG_WAVES;
    for (int64_t t = wave; t < A.items; t += waves) {
        const int64_t lo = t * SG_CHUNK, hi = lo + SG_CHUNK;
        const int64_t first = sg_lower_bound(A, lo);           // first row that starts at or behind lo
        if (first >= 1 && first - 1 < A.U) {
            const int64_t s0 = sg_seg(A, first - 1), s1 = sg_seg(A, first);
            const int64_t s = s0 + (lo - s0 + SG_CHUNK - 1) / SG_CHUNK * SG_CHUNK;     // in [lo, hi), behind s0
            if (s < s1) sg_sum_chunk<NV>(A, s, s + SG_CHUNK < s1 ? s + SG_CHUNK : s1, A.scratch + t * A.ldg);
        }
        for (int64_t u = first; u < A.U; ++u) {
            const int64_t s0 = sg_seg(A, u);
            if (s0 >= hi) break;
            int64_t s1 = sg_seg(A, u + 1);
            if (s1 < s0) s1 = s0;
            sg_sum_chunk<NV>(A, s0, s0 + SG_CHUNK < s1 ? s0 + SG_CHUNK : s1, A.grad + u * A.ldg);
        }
    }
}

// grad[u] += its later chunks' partial rows, in chunk order; a row of one chunk is left as it is.
template <int NV>
__global__ __launch_bounds__(SG_BLOCK) void skipgram_grad_combine_kernel(GradArgs A) {
    const int64_t wave = (int64_t)blockIdx.x * SG_WAVES + threadIdx.x / LPF_WAVE;
    const int64_t waves = (int64_t)gridDim.x * SG_WAVES;
    const int lane = lpf_lane();
    for (int64_t u = wave; u < A.U; u += waves) {
        const int64_t s0 = sg_seg(A, u), s1 = sg_seg(A, u + 1);
        if (s0 + SG_CHUNK >= s1) continue;
        float4 acc[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int j = lane + LPF_WAVE * i;
            acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j < A.dim4) acc[i] = reinterpret_cast<const float4 *>(A.grad + u * A.ldg)[j];
        }
        for (int64_t s = s0 + SG_CHUNK; s < s1; s += SG_CHUNK) {
            const float *part = A.scratch + (s / SG_CHUNK) * A.ldg;            // s < n_occ: a block of the list
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int j = lane + LPF_WAVE * i;
                if (j < A.dim4) {
                    const float4 v = reinterpret_cast<const float4 *>(part)[j];
                    acc[i].x += v.x;
                    acc[i].y += v.y;
                    acc[i].z += v.z;
                    acc[i].w += v.w;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int j = lane + LPF_WAVE * i;
            if (j < A.dim4) reinterpret_cast<float4 *>(A.grad + u * A.ldg)[j] = acc[i];
        }
    }
}

struct AdamArgs {
    int64_t n;
    int32_t dim4;
    float *table, *exp_avg, *exp_avg_sq;
    int64_t ldt, lds;
    int64_t U;
    const int32_t *rows;
    const float *grad;
    int64_t ldg;
    float c1, c2, eps, step_size;
};

// torch.optim.SparseAdam on the listed rows, a thread per four elements:  m += (g - m)(1 - beta1),
// v += (g g - v)(1 - beta2), param -= step_size m / (sqrt(v) + eps), step_size = lr sqrt(1 - beta2^t) / (1 - beta1^t).
__global__ __launch_bounds__(SG_BLOCK) void sparse_adam_rows_kernel(AdamArgs A) {
#pragma clang fp contract(off)
    const int64_t tid = (int64_t)blockIdx.x * SG_BLOCK + threadIdx.x;
    const int64_t u = tid / A.dim4;
    const int j = (int)(tid % A.dim4);
    if (u >= A.U) return;
    const int32_t r = A.rows[u];
    if ((uint64_t)(uint32_t)r >= (uint64_t)A.n) return;
    const float4 g = reinterpret_cast<const float4 *>(A.grad + u * A.ldg)[j];
    float4 *pm = reinterpret_cast<float4 *>(A.exp_avg + (int64_t)r * A.lds) + j;
    float4 *pv = reinterpret_cast<float4 *>(A.exp_avg_sq + (int64_t)r * A.lds) + j;
    float4 *pp = reinterpret_cast<float4 *>(A.table + (int64_t)r * A.ldt) + j;
    float4 m = *pm, v = *pv, p = *pp;
    const float c1 = A.c1, c2 = A.c2;
#define SG_ADAM(f)                                           \
    m.f = m.f + (g.f - m.f) * c1;                            \
    v.f = v.f + (g.f * g.f - v.f) * c2;                      \
    p.f = p.f - A.step_size * (m.f / (sqrtf(v.f) + A.eps));
    SG_ADAM(x) SG_ADAM(y) SG_ADAM(z) SG_ADAM(w)
#undef SG_ADAM
    *pm = m;
    *pv = v;
    *pp = p;
}

bool sg_dim_ok(int32_t dim) { return dim >= 4 && dim % 4 == 0 && dim <= LPF_SKIPGRAM_MAX_DIM; }
bool sg_rows_ok(const void *p, int64_t ld, int32_t dim) { return p && lpf_aligned16(p) && ld >= dim && ld % 4 == 0; }

}  // namespace

extern "C" int lpf_skipgram_coef_f32(int64_t n, int32_t dim, const float *table, int64_t ldt, int32_t L,
                                     int32_t context, const int32_t *pos, int64_t Wp, int64_t ldp, const int32_t *neg,
                                     int64_t Wn, int64_t ldn, float *coef, int32_t *centre, int32_t *other,
                                     double *partial, int64_t partial_len, double *loss, void *stream) {
    LPF_REQUIRE(n >= 0 && n < INT32_MAX && sg_dim_ok(dim));
    LPF_REQUIRE(L >= 1 && L <= LPF_WALK_MAX_LENGTH && context >= 2 && context <= L + 1);
    LPF_REQUIRE(Wp >= 0 && Wn >= 0 && Wp < INT32_MAX && Wn < INT32_MAX && ldp >= Wp && ldn >= Wn);
    const int64_t nwin = (int64_t)L + 2 - context, per = context - 1;
    const int64_t windows = (Wp + Wn) * nwin;                  // < 2^32 2^17
    LPF_REQUIRE(windows <= (INT32_MAX - 1) / per);             // pair ids are int32
    if (windows == 0) return LPF_OK;
    LPF_REQUIRE((n == 0 || sg_rows_ok(table, ldt, dim)) && (pos || Wp == 0) && (neg || Wn == 0));
    LPF_REQUIRE(coef && centre && other && partial && loss);
    const int64_t blocks = (windows + SG_WINDOWS - 1) / SG_WINDOWS;
    LPF_REQUIRE(partial_len >= blocks);
    CoefArgs A{};
    A.n = n;
    A.dim4 = dim / 4;
    A.table = table;
    A.ldt = ldt;
    A.nwin = (int32_t)nwin;
    A.pairs_per_window = (int32_t)per;
    A.pos = pos;
    A.neg = neg;
    A.ldp = ldp;
    A.ldn = ldn;
    A.pos_windows = Wp * nwin;
    A.windows = windows;
    A.inv_mp = Wp ? 1.0 / (double)(Wp * nwin * per) : 0.0;
    A.inv_mn = Wn ? 1.0 / (double)(Wn * nwin * per) : 0.0;
    A.coef = coef;
    A.centre = centre;
    A.other = other;
    A.partial = partial;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks), block(SG_BLOCK);
    const int nv = (A.dim4 + SG_GROUP - 1) / SG_GROUP;         // float4 per lane: 1 .. 8
    if (nv <= 1) hipLaunchKernelGGL(skipgram_coef_kernel<1>, grid, block, 0, s, A);
    else if (nv <= 2) hipLaunchKernelGGL(skipgram_coef_kernel<2>, grid, block, 0, s, A);
    else if (nv <= 4) hipLaunchKernelGGL(skipgram_coef_kernel<4>, grid, block, 0, s, A);
    else hipLaunchKernelGGL(skipgram_coef_kernel<8>, grid, block, 0, s, A);
    LPF_CHECK_LAUNCH();
    hipLaunchKernelGGL(skipgram_loss_kernel, dim3(1), block, 0, s, partial, blocks, loss);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}

extern "C" int lpf_skipgram_grad_rows_f32(int64_t n, int32_t dim, const float *table, int64_t ldt, int64_t M,
                                          const float *coef, int64_t n_occ, const int32_t *occ_other,
                                          const int32_t *occ_pair, int64_t U, const int64_t *seg, float *grad,
                                          int64_t ldg, float *scratch, int64_t scratch_rows, int32_t groups,
                                          void *stream) {
    LPF_REQUIRE(n >= 0 && n < INT32_MAX && sg_dim_ok(dim));
    LPF_REQUIRE(M >= 0 && M < INT32_MAX && n_occ >= 0 && n_occ < 2 * (int64_t)INT32_MAX && U >= 0 && U < INT32_MAX);
    LPF_REQUIRE(groups >= 0);
    if (U == 0) return LPF_OK;
    LPF_REQUIRE((n == 0 || sg_rows_ok(table, ldt, dim)) && sg_rows_ok(grad, ldg, dim) && seg);
    LPF_REQUIRE((coef || M == 0) && ((occ_other && occ_pair) || n_occ == 0));
    const int64_t items = (n_occ + SG_CHUNK - 1) / SG_CHUNK;
    LPF_REQUIRE(items == 0 || (scratch && lpf_aligned16(scratch) && scratch_rows >= items));
    GradArgs A{};
    A.n = n;
    A.dim4 = dim / 4;
    A.table = table;
    A.ldt = ldt;
    A.M = M;
    A.coef = coef;
    A.n_occ = n_occ;
    A.occ_other = occ_other;
    A.occ_pair = occ_pair;
    A.U = U;
    A.seg = seg;
    A.grad = grad;
    A.ldg = ldg;
    A.scratch = scratch;
    A.items = items;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 block(SG_BLOCK);
    const bool wide = A.dim4 > LPF_WAVE;
    if (items == 0) {                                          // rows without occurrences: all zero
        const hipError_t e = hipMemset2DAsync(grad, (size_t)ldg * sizeof(float), 0, (size_t)dim * sizeof(float),
                                              (size_t)U, s);
        if (e != hipSuccess) {
            lpf_set_hip_error(e);
            return LPF_ERR_LAUNCH;
        }
        return LPF_OK;
    }
    // groups == 0: a wavefront per item and per row; any other count gives the same bits
    const int64_t want1 = groups ? groups : (items + SG_WAVES - 1) / SG_WAVES;
    const int64_t want2 = groups ? groups : (U + SG_WAVES - 1) / SG_WAVES;
    const dim3 grid1((unsigned)(want1 < (1 << 20) ? want1 : (1 << 20)));
    const dim3 grid2((unsigned)(want2 < (1 << 20) ? want2 : (1 << 20)));
    if (wide) hipLaunchKernelGGL(skipgram_grad_chunks_kernel<2>, grid1, block, 0, s, A);
    else hipLaunchKernelGGL(skipgram_grad_chunks_kernel<1>, grid1, block, 0, s, A);
    LPF_CHECK_LAUNCH();
    if (wide) hipLaunchKernelGGL(skipgram_grad_combine_kernel<2>, grid2, block, 0, s, A);
    else hipLaunchKernelGGL(skipgram_grad_combine_kernel<1>, grid2, block, 0, s, A);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}

extern "C" int lpf_sparse_adam_rows_f32(int64_t n, int32_t dim, float *table, int64_t ldt, float *exp_avg,
                                        float *exp_avg_sq, int64_t lds, int64_t U, const int32_t *rows,
                                        const float *grad, int64_t ldg, double lr, double beta1, double beta2,
                                        double eps, int64_t step, double bias1, double bias2, void *stream) {
    LPF_REQUIRE(n >= 0 && n < INT32_MAX && sg_dim_ok(dim) && U >= 0 && U < INT32_MAX);
    LPF_REQUIRE(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0);
    LPF_REQUIRE(step >= 1 && bias1 > 0.0 && bias1 <= 1.0 && bias2 > 0.0 && bias2 <= 1.0);
    if (U == 0 || n == 0) return LPF_OK;
    LPF_REQUIRE(sg_rows_ok(table, ldt, dim) && sg_rows_ok(exp_avg, lds, dim) && sg_rows_ok(exp_avg_sq, lds, dim));
    LPF_REQUIRE(rows && sg_rows_ok(grad, ldg, dim));
    AdamArgs A{};
    A.n = n;
    A.dim4 = dim / 4;
    A.table = table;
    A.exp_avg = exp_avg;
    A.exp_avg_sq = exp_avg_sq;
    A.ldt = ldt;
    A.lds = lds;
    A.U = U;
    A.rows = rows;
    A.grad = grad;
    A.ldg = ldg;
    A.c1 = (float)(1.0 - beta1);                               // the scalars torch rounds to fp32: 1 - beta, eps, the step size
    A.c2 = (float)(1.0 - beta2);
    A.eps = (float)eps;
    A.step_size = (float)(lr * sqrt(bias2) / bias1);
    const int64_t threads = U * A.dim4;                        // < 2^31 2^7
    const int64_t blocks = (threads + SG_BLOCK - 1) / SG_BLOCK;
    LPF_REQUIRE(blocks <= INT32_MAX);
    hipLaunchKernelGGL(sparse_adam_rows_kernel, dim3((unsigned)blocks), dim3(SG_BLOCK), 0,
                       static_cast<hipStream_t>(stream), A);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}
