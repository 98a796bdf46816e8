// Bootstrap replicates of column sums: for replicate b = b0 + r, r = 0 .. B - 1,
//   isum[r][c] = sum_{j < P} icols[idx(b, j)][c]      (int64, exact)
//   fsum[r][c] = sum_{j < P} fcols[idx(b, j)][c]      (fp64, in the fixed order below)
// with idx(b, j) = node(u(key(seed, b), j), P) -- the draw of draw_common.h, the one the negatives use.  A replicate is
// a pure function of (seed, b, tables): not of b0, B, n_groups, the grid or timing; two runs are bitwise equal.
//
// THE ORDER OF AN fp64 SUM (it is the order of the integer sums as well, where it does not matter):
//   1. j is cut into fixed segments of BS_SEG = 16,384 consecutive draws: segment s holds j in [s BS_SEG, (s + 1) BS_SEG).
//      The cut depends on P alone.
//   2. Inside a segment, thread t of the 256 takes j = s BS_SEG + t, + 256, + 512, ... and adds its rows to its own
//      accumulator in that order, starting from +0.0 (four draws and their gathers are in flight per thread; the adds stay
//      in j order).
//   3. The 64 accumulators of a wavefront are summed by an xor butterfly, partner distances 32, 16, 8, 4, 2, 1 (every
//      lane ends with the same bits: each step adds the same two numbers in both partners).
//   4. The four wavefronts' sums are added in the order ((w0 + w1) + w2) + w3.
//   5. The segments' sums are added in the order s = 0, 1, 2, ..., starting from segment 0's sum (a second launch over
//      the partials in the workspace; with one segment the sum of step 4 is the result and no workspace is used).
// No float atomics and no integer ones either: a (replicate, segment) unit is computed by one workgroup, whichever it is
// (unit u goes to workgroup u mod grid), and written to a place of its own.
//
// What bounds the loop: a draw is two 64-bit multiplies by constants and one 64 x 32 high product built from 32-bit
// multiplies, about 40 vector instructions; a gather is one 16-byte load per pair of columns (rows of 2, 4 or 8 words,
// 16-byte aligned) or one 8-byte load per column from a random row, 64 different cache lines per wave instruction.  Read
// from the code, the gathers set the time once there is more than a column or two, and the unroll by four keeps four
// rows per lane in flight for that reason.  Measured (profiles/bootstrap_timing.json): 1.0e11 draws/s on a
// 1.25 MB table and 2.9e10 on a 114 MB one with the five columns of bootstrap_metrics -- a tenth of what the draw's
// instruction count allows; the split itself (draws without gathers) is not measured.
#include "lpf_common.h"
#include "draw_common.h"

namespace {

constexpr int BS_BLOCK = 256;
constexpr int BS_WAVES = BS_BLOCK / LPF_WAVE;
constexpr int BS_SEG = LPF_BOOTSTRAP_SEGMENT;                   // draws per segment: 64 per thread
constexpr int BS_UNROLL = 4;
constexpr int BS_MAX_COLS = LPF_BOOTSTRAP_MAX_COLS;
constexpr int64_t BS_MAX_GROUPS = 65535;
static_assert(BS_SEG % (BS_BLOCK * BS_UNROLL) == 0, "a full segment is a whole number of unrolled rounds");

struct BsArgs {
    int64_t P, B, nseg;
    uint64_t seed, b0;
    const int64_t *icols;
    const double *fcols;
    int32_t Ci, Cf;
    int32_t ivec, fvec;                         // rows of exactly CI / CF words, 16-byte aligned: 16-byte loads
    int64_t *iout;                              // nseg == 1: isum [B][Ci]; else partials [B][nseg][Ci]
    double *fout;
};

// row `idx` of a [P][C] table into v[0 .. N): N >= C is the padded width the kernel was built for
template <int N, typename T>
__device__ __forceinline__ void bs_load_row(const T *__restrict__ tab, int64_t idx, int32_t C, bool vec, T (&v)[N]) {
    if constexpr (N >= 2) {
        if (vec) {                               // kernel-uniform: C == N
            typedef T T2 __attribute__((ext_vector_type(2)));
            const T2 *p = reinterpret_cast<const T2 *>(tab + idx * N);
#pragma unroll
            for (int c = 0; c < N / 2; ++c) {
                const T2 x = p[c];
                v[2 * c] = x.x;
                v[2 * c + 1] = x.y;
            }
            return;
        }
    }
    const T *p = tab + idx * C;
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] = c < C ? p[c] : T(0);
}

__device__ __forceinline__ int64_t bs_shfl_xor(int64_t v, int m) { return (int64_t)__shfl_xor((long long)v, m, 64); }
__device__ __forceinline__ double bs_shfl_xor(double v, int m) { return __shfl_xor(v, m, 64); }

// steps 3 and 4 of the order; thread c < C then holds column c's segment sum in the return value
template <int N, typename T>
__device__ __forceinline__ T bs_block_sum(T (&acc)[N], T (*lds)[BS_MAX_COLS], int32_t C) {
    const int lane = lpf_lane(), wave = threadIdx.x / LPF_WAVE;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        T v = acc[c];
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) v = v + bs_shfl_xor(v, m);
        if (lane == 0) lds[wave][c] = v;
    }
    __syncthreads();
    T out = T(0);
    if ((int)threadIdx.x < C) {
        out = lds[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < BS_WAVES; ++w) out = out + lds[w][threadIdx.x];
    }
    return out;
}

template <int CI, int CF>
__global__ __launch_bounds__(BS_BLOCK) void bootstrap_segment_kernel(BsArgs A) {
    __shared__ int64_t ilds[BS_WAVES][BS_MAX_COLS];
    __shared__ double flds[BS_WAVES][BS_MAX_COLS];
    const int64_t units = A.B * A.nseg;
    const uint64_t P = (uint64_t)(uint32_t)A.P;     // P < 2^31: the high product needs the low word of P only
    for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {   // workgroup-uniform
        const int64_t r = unit / A.nseg, s = unit - r * A.nseg;
        const uint64_t key = lpf_draw_key(A.seed, A.b0 + (uint64_t)r);
        const int64_t j0 = s * BS_SEG;
        const int64_t j1 = (j0 + BS_SEG < A.P) ? j0 + BS_SEG : A.P;
        int64_t iacc[CI > 0 ? CI : 1];
        double facc[CF > 0 ? CF : 1];
#pragma unroll
        for (int c = 0; c < (CI > 0 ? CI : 1); ++c) iacc[c] = 0;
#pragma unroll
        for (int c = 0; c < (CF > 0 ? CF : 1); ++c) facc[c] = 0.0;
        for (int64_t jb = j0; jb < j1; jb += BS_BLOCK * BS_UNROLL) {   // workgroup-uniform
            int64_t iv[BS_UNROLL][CI > 0 ? CI : 1];
            double fv[BS_UNROLL][CF > 0 ? CF : 1];
            bool live[BS_UNROLL];
#pragma unroll
            for (int k = 0; k < BS_UNROLL; ++k) {
                const int64_t j = jb + k * BS_BLOCK + threadIdx.x;
                live[k] = j < j1;
                // a draw past the end is still a row in [0, P): it is loaded and not added
                const int64_t idx = lpf_draw_node(key, (uint64_t)j, P);
                if constexpr (CI > 0) bs_load_row<CI>(A.icols, idx, A.Ci, A.ivec != 0, iv[k]);
                if constexpr (CF > 0) bs_load_row<CF>(A.fcols, idx, A.Cf, A.fvec != 0, fv[k]);
            }
#pragma unroll
            for (int k = 0; k < BS_UNROLL; ++k) {
                if (live[k]) {
                    if constexpr (CI > 0) {
#pragma unroll
                        for (int c = 0; c < CI; ++c) iacc[c] += iv[k][c];
                    }
                    if constexpr (CF > 0) {
#pragma unroll
                        for (int c = 0; c < CF; ++c) facc[c] = facc[c] + fv[k][c];
                    }
                }
            }
        }
        if constexpr (CI > 0) {
            const int64_t v = bs_block_sum<CI>(iacc, ilds, A.Ci);
            if ((int)threadIdx.x < A.Ci) A.iout[unit * A.Ci + threadIdx.x] = v;
        }
        if constexpr (CF > 0) {
            const double v = bs_block_sum<CF>(facc, flds, A.Cf);
            if ((int)threadIdx.x < A.Cf) A.fout[unit * A.Cf + threadIdx.x] = v;
        }
        __syncthreads();                          // the next unit's lane-0 stores come after these reads
    }
}

// step 5 of the order: one thread per (replicate, column), the segments in ascending order
struct BsFinishArgs {
    int64_t B, nseg;
    int32_t Ci, Cf;
    const int64_t *ipart;
    const double *fpart;
    int64_t *isum;
    double *fsum;
};

__global__ __launch_bounds__(BS_BLOCK) void bootstrap_finish_kernel(BsFinishArgs A) {
    const int32_t C = A.Ci + A.Cf;
    const int64_t e = (int64_t)blockIdx.x * BS_BLOCK + threadIdx.x;
    if (e >= A.B * C) return;
    const int64_t r = e / C;
    const int32_t c = (int32_t)(e - r * C);
    if (c < A.Ci) {
        const int64_t *p = A.ipart + r * A.nseg * A.Ci + c;
        int64_t v = p[0];
        for (int64_t s = 1; s < A.nseg; ++s) v += p[s * A.Ci];
        A.isum[r * A.Ci + c] = v;
    } else {
        const int32_t cf = c - A.Ci;
        const double *p = A.fpart + r * A.nseg * A.Cf + cf;
        double v = p[0];
        for (int64_t s = 1; s < A.nseg; ++s) v = v + p[s * A.Cf];
        A.fsum[r * A.Cf + cf] = v;
    }
}

bool bs_shape_ok(int64_t P, int64_t B, int32_t Ci, int32_t Cf, int64_t n_groups) {
    return P >= 1 && P < ((int64_t)1 << 31) && B >= 1 && B < ((int64_t)1 << 31) && Ci >= 0 && Ci <= BS_MAX_COLS &&
           Cf >= 0 && Cf <= BS_MAX_COLS && Ci + Cf >= 1 && n_groups >= 0 && n_groups <= BS_MAX_GROUPS;
}
int64_t bs_segments(int64_t P) { return (P + BS_SEG - 1) / BS_SEG; }
int bs_pad(int32_t c) { return c == 0 ? 0 : c == 1 ? 1 : c == 2 ? 2 : c <= 4 ? 4 : 8; }

typedef void (*bs_kernel_t)(BsArgs);
template <int CI>
bs_kernel_t bs_pick_f(int cf) {
    switch (cf) {
        case 0: return bootstrap_segment_kernel<CI, 0>;
        case 1: return bootstrap_segment_kernel<CI, 1>;
        case 2: return bootstrap_segment_kernel<CI, 2>;
        case 4: return bootstrap_segment_kernel<CI, 4>;
        default: return bootstrap_segment_kernel<CI, 8>;
    }
}
bs_kernel_t bs_pick(int ci, int cf) {
    switch (ci) {
        case 0: return bs_pick_f<0>(cf);
        case 1: return bs_pick_f<1>(cf);
        case 2: return bs_pick_f<2>(cf);
        case 4: return bs_pick_f<4>(cf);
        default: return bs_pick_f<8>(cf);
    }
}

}  // namespace

extern "C" int64_t lpf_bootstrap_workspace_bytes(int64_t P, int64_t B, int32_t Ci, int32_t Cf, int32_t n_groups) {
    if (!bs_shape_ok(P, B, Ci, Cf, n_groups)) return -1;
    const int64_t nseg = bs_segments(P);
    return nseg == 1 ? 0 : B * nseg * (int64_t)(Ci + Cf) * 8;       // < 2^31 * 2^17 * 16 * 8: no overflow
}

extern "C" int lpf_bootstrap_sums(int64_t P, int64_t B, int64_t b0, uint64_t seed, const int64_t *icols, int32_t Ci,
                                  const double *fcols, int32_t Cf, int64_t *isum, double *fsum, int32_t n_groups,
                                  void *workspace, int64_t workspace_bytes, void *stream) {
    LPF_REQUIRE(bs_shape_ok(P, B, Ci, Cf, n_groups) && b0 >= 0);
    LPF_REQUIRE((Ci == 0 || (icols && isum)) && (Cf == 0 || (fcols && fsum)));
    const int64_t nseg = bs_segments(P);
    const int64_t need = lpf_bootstrap_workspace_bytes(P, B, Ci, Cf, n_groups);
    LPF_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int ci = bs_pad(Ci), cf = bs_pad(Cf);
    BsArgs A{};
    A.P = P;
    A.B = B;
    A.nseg = nseg;
    A.seed = seed;
    A.b0 = (uint64_t)b0;
    A.icols = icols;
    A.fcols = fcols;
    A.Ci = Ci;
    A.Cf = Cf;
    A.ivec = Ci >= 2 && ci == Ci && lpf_aligned16(icols);
    A.fvec = Cf >= 2 && cf == Cf && lpf_aligned16(fcols);
    int64_t *ipart = static_cast<int64_t *>(workspace);
    double *fpart = reinterpret_cast<double *>(ipart + (nseg == 1 ? 0 : B * nseg * Ci));
    A.iout = nseg == 1 ? isum : ipart;
    A.fout = nseg == 1 ? fsum : fpart;
    const int64_t units = B * nseg;
    int64_t grid = n_groups;
    if (grid == 0) {                             // default sizing: eight resident workgroups per CU
        const int cus = lpf_cu_count();
        grid = (int64_t)(cus > 0 ? cus : 256) * 8;
    }
    grid = grid < units ? grid : units;
    hipLaunchKernelGGL(bs_pick(ci, cf), dim3((unsigned)grid), dim3(BS_BLOCK), 0, s, A);
    LPF_CHECK_LAUNCH();
    if (nseg > 1) {
        BsFinishArgs F{};
        F.B = B;
        F.nseg = nseg;
        F.Ci = Ci;
        F.Cf = Cf;
        F.ipart = ipart;
        F.fpart = fpart;
        F.isum = isum;
        F.fsum = fsum;
        const int64_t fgrid = (B * (Ci + Cf) + BS_BLOCK - 1) / BS_BLOCK;
        hipLaunchKernelGGL(bootstrap_finish_kernel, dim3((unsigned)fgrid), dim3(BS_BLOCK), 0, s, F);
        LPF_CHECK_LAUNCH();
    }
    return LPF_OK;
}
