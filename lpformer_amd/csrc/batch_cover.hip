// Batch cover: which undirected training edges does a batch of train_pos ROWS remove from the typing adjacency?
//
// The reference's loop drops the batch's rows of train_pos and builds a symmetric adjacency from the rows that are left
// (src/train/train_model.py:40-45).  An undirected edge {u, v} is therefore ABSENT from that adjacency iff every row
// that holds it -- (u, v) or (v, u), any number of times -- is in the batch.  With the rows grouped by their undirected
// edge once per dataset (gid[e] = group of row e, mult[g] = rows of group g) the answer for one batch is a count:
//
//   count   cnt[gid[perm[i]]] += 1 for every batch position i                     (integer atomics)
//   emit    position i writes (min, max) of its row iff cnt[g] == mult[g], else (-1, -1); stats by ballot + popcount
//   reset   cnt[gid[perm[i]]] = 0                                                 (plain stores)
//
// Three launches in stream order: emit needs the counts of the WHOLE batch -- the twin of a row may be counted by any
// other workgroup -- and a kernel boundary is the one grid-wide phase that needs no spinning; reset needs every emit to
// have read its counter.  The kernels are launch-sized (a batch is a few thousand rows): one thread per position, no
// host synchronisation, a fixed output shape.  perm entries outside [0, E) touch no memory and are counted.
#include "lpf_common.h"

namespace {

constexpr int BC_BLOCK = 256;

struct CoverArgs {
    const int32_t *gid, *mult;
    const int64_t *train_pos, *perm;
    int64_t E, G, B;
    int32_t *cnt;
    int64_t *out;
    int32_t *stats;
};

// Group of batch position i, or -1 when the position names no row (i >= B, perm[i] outside [0, E), or a group id
// outside [0, G): an index that was not built for this train_pos).  `row` receives perm[i].
__device__ __forceinline__ int32_t position_group(const CoverArgs &A, int64_t i, int64_t &row) {
    row = -1;
    if (i >= A.B) return -1;
    row = A.perm[i];
    if ((uint64_t)row >= (uint64_t)A.E) return -1;
    const int32_t g = A.gid[row];
    return (uint64_t)(int64_t)g < (uint64_t)A.G ? g : -1;
}

__global__ __launch_bounds__(BC_BLOCK) void cover_count_kernel(CoverArgs A) {
    int64_t row;
    const int32_t g = position_group(A, (int64_t)blockIdx.x * BC_BLOCK + threadIdx.x, row);
    if (g >= 0) atomicAdd(&A.cnt[g], 1);
}

__global__ __launch_bounds__(BC_BLOCK) void cover_emit_kernel(CoverArgs A) {
    const int64_t i = (int64_t)blockIdx.x * BC_BLOCK + threadIdx.x;
    int64_t row;
    const int32_t g = position_group(A, i, row);
    const bool in_batch = i < A.B;
    const bool emit = g >= 0 && A.cnt[g] == A.mult[g];
    if (in_batch) {
        int64_t lo = -1, hi = -1;
        if (emit) {
            const int64_t u = A.train_pos[2 * row], v = A.train_pos[2 * row + 1];
            lo = u < v ? u : v;
            hi = u < v ? v : u;
        }
        A.out[i] = lo;
        A.out[A.B + i] = hi;
    }
    // one integer atomic per wavefront and word (every lane of the wave reaches the ballots)
    const int n_emit = __popcll(__ballot(emit));
    const int n_held = __popcll(__ballot(g >= 0 && !emit));
    const int n_skip = __popcll(__ballot(in_batch && g < 0));
    if (lpf_lane() == 0) {
        if (n_emit) atomicAdd(&A.stats[0], n_emit);
        if (n_held) atomicAdd(&A.stats[1], n_held);
        if (n_skip) atomicAdd(&A.stats[2], n_skip);
    }
}

__global__ __launch_bounds__(BC_BLOCK) void cover_reset_kernel(CoverArgs A) {
    int64_t row;
    const int32_t g = position_group(A, (int64_t)blockIdx.x * BC_BLOCK + threadIdx.x, row);
    if (g >= 0) A.cnt[g] = 0;
}

}  // namespace

extern "C" int lpf_batch_cover(const int32_t *gid, const int32_t *mult, const int64_t *train_pos, int64_t E, int64_t G,
                               const int64_t *perm, int64_t B, int32_t *cnt, int64_t *out, int32_t *stats, void *stream) {
    LPF_REQUIRE(B >= 0 && E >= 0 && G >= 0);
    if (B == 0) return LPF_OK;
    LPF_REQUIRE(B < INT32_MAX && E < INT32_MAX && G <= E && perm && out && stats);
    LPF_REQUIRE(E == 0 || (gid && train_pos));
    LPF_REQUIRE(G == 0 || (mult && cnt));
    CoverArgs A{gid, mult, train_pos, perm, E, G, B, cnt, out, stats};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((B + BC_BLOCK - 1) / BC_BLOCK)), block(BC_BLOCK);
    hipLaunchKernelGGL(cover_count_kernel, grid, block, 0, s, A);
    LPF_CHECK_LAUNCH();
    hipLaunchKernelGGL(cover_emit_kernel, grid, block, 0, s, A);
    LPF_CHECK_LAUNCH();
    hipLaunchKernelGGL(cover_reset_kernel, grid, block, 0, s, A);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}
