// Incremental refresh of the PPR matrix after a graph edit (lpformer_amd/graph_update.py).
//
// The push of source s (ppr_push.hip) stores EVERY node it popped in row s, and reads a node's neighbour list only when
// it pops it.  So a row that holds none of the "key" nodes of an edit (endpoints of added / removed edges and the old
// neighbours of removal endpoints) replays bit for bit on the edited graph, and only the rows that meet a key are pushed
// again (lpf_ppr_push_f64_sources).  This file holds the two steps around that push:
//   * lpf_ppr_affected_rows: which rows meet a key -- one pass over `col` (4 B per stored entry) with one bit probe per
//     entry; a wavefront per row, four independent loads per lane in flight, ballot-OR of the probes, the row is left at
//     the first hit.  The key bitmap (n / 8 bytes) is staged in LDS when small, probed in global memory (L2) otherwise.
//     The flagged ids are compacted in ascending order by rocPRIM's flagged select.
//   * lpf_ppr_splice_csr: the new CSR = old rows where the flag is clear, freshly pushed rows (sorted by column with the
//     segmented radix sort lpf_ppr_pack_csr uses) where it is set.
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "lpf_common.h"

namespace {

constexpr int PU_BLOCK = 256;                    // four wavefronts
constexpr int64_t PU_LDS_AUTO = 40 * 1024;       // bitmap bytes up to which `auto` stages it: four workgroups per CU
constexpr int64_t PU_LDS_MAX = 64 * 1024;        // ... and up to which the LDS form can be asked for at all

constexpr int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

template <bool LDS>
__global__ __launch_bounds__(PU_BLOCK) void ppr_flag_rows_kernel(int64_t n, const int64_t *__restrict__ rowptr,
                                                                  const int32_t *__restrict__ col,
                                                                  const uint32_t *__restrict__ bitmap, int64_t n_words,
                                                                  int32_t *__restrict__ flag) {
    extern __shared__ uint32_t pu_bits[];
    if (LDS) {
        for (int64_t i = threadIdx.x; i < n_words; i += PU_BLOCK) pu_bits[i] = bitmap[i];
        __syncthreads();
    }
    const uint32_t *__restrict__ bits = LDS ? pu_bits : bitmap;
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * (PU_BLOCK / 64);
    for (int64_t row = (int64_t)blockIdx.x * (PU_BLOCK / 64) + (threadIdx.x >> 6); row < n; row += n_waves) {
        const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
        bool hit = false;
        for (int64_t e = e0 + lane; e - lane < e1 && !hit; e += 256) {
            int32_t c[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] = (e + 64 * k < e1) ? col[e + 64 * k] : -1;
            bool h = false;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((uint32_t)c[k] < (uint32_t)n) h |= (bits[c[k] >> 5] >> (c[k] & 31)) & 1u;   // (-1 and bad ids: no probe)
            hit = __ballot(h) != 0ull;
        }
        if (lane == 0) flag[row] = hit ? 1 : 0;
    }
}

__global__ __launch_bounds__(PU_BLOCK) void splice_len_old_kernel(int64_t n, const int64_t *__restrict__ old_rowptr,
                                                                   int64_t *__restrict__ len64,
                                                                   int32_t *__restrict__ pos) {
    const int64_t i = (int64_t)blockIdx.x * PU_BLOCK + threadIdx.x;
    if (i < n) {
        len64[i] = old_rowptr[i + 1] - old_rowptr[i];
        pos[i] = -1;
    }
}

__global__ __launch_bounds__(PU_BLOCK) void splice_len_new_kernel(int64_t n, int64_t n_src,
                                                                   const int32_t *__restrict__ sources,
                                                                   const int64_t *__restrict__ row_off,
                                                                   const int32_t *__restrict__ row_len,
                                                                   int64_t *__restrict__ len64,
                                                                   int32_t *__restrict__ pos,
                                                                   int64_t *__restrict__ row_end) {
    const int64_t j = (int64_t)blockIdx.x * PU_BLOCK + threadIdx.x;
    if (j < n_src) {
        const int32_t s = sources[j];
        row_end[j] = row_off[j] + row_len[j];
        if ((uint32_t)s < (uint32_t)n) {   // (ids are distinct: no two threads write one slot)
            len64[s] = row_len[j];
            pos[s] = (int32_t)j;
        }
    }
}

// one wavefront per row: the old row, or the sorted re-pushed one
__global__ __launch_bounds__(PU_BLOCK) void splice_copy_kernel(
    int64_t n, const int64_t *__restrict__ old_rowptr, const int32_t *__restrict__ old_col,
    const float *__restrict__ old_val, const int32_t *__restrict__ pos, const int64_t *__restrict__ row_off,
    const int32_t *__restrict__ scol, const float *__restrict__ sval, int64_t nnz_pool,
    const int64_t *__restrict__ out_rowptr, int32_t *__restrict__ out_col, float *__restrict__ out_val,
    int64_t out_capacity) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (PU_BLOCK / 64) + (threadIdx.x >> 6);
    if (row >= n) return;
    const int64_t dst = out_rowptr[row], len = out_rowptr[row + 1] - dst;
    if (dst + len > out_capacity) return;   // (a capacity that does not match the lengths: never write past it)
    const int32_t j = pos[row];
    if (j >= 0) {
        const int64_t src = row_off[j];
        if (src < 0 || src + len > nnz_pool) return;
        for (int64_t i = lane; i < len; i += 64) {
            out_col[dst + i] = scol[src + i];
            out_val[dst + i] = sval[src + i];
        }
    } else {
        const int64_t src = old_rowptr[row];
        for (int64_t i = lane; i < len; i += 64) {
            out_col[dst + i] = old_col[src + i];
            out_val[dst + i] = old_val[src + i];
        }
    }
}

size_t select_tmp_bytes(int64_t n) {
    size_t bytes = 0;
    (void)rocprim::select(nullptr, bytes, rocprim::counting_iterator<int32_t>(0), (const int32_t *)nullptr,
                          (int32_t *)nullptr, (int64_t *)nullptr, (size_t)n);
    return bytes;
}

}  // namespace

extern "C" int64_t lpf_ppr_affected_workspace_bytes(int64_t n) {
    if (n <= 0 || n >= (1ll << 31)) return 0;
    return align256((int64_t)select_tmp_bytes(n)) + 256;
}

extern "C" int lpf_ppr_affected_rows(int64_t n, const int64_t *rowptr, const int32_t *col, const uint32_t *key_bitmap,
                                     int32_t bitmap_mode, int32_t *flag, int32_t *list, int64_t *count,
                                     void *workspace, int64_t workspace_bytes, void *stream) {
    LPF_REQUIRE(n >= 0 && n < (1ll << 31) && count && bitmap_mode >= -1 && bitmap_mode <= 1);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) {
        if (hipMemsetAsync(count, 0, sizeof(int64_t), s) != hipSuccess) return LPF_ERR_LAUNCH;
        return LPF_OK;
    }
    LPF_REQUIRE(rowptr && col && key_bitmap && flag && list && workspace);
    LPF_REQUIRE(workspace_bytes >= lpf_ppr_affected_workspace_bytes(n));
    const int64_t n_words = (n + 31) / 32, lds_bytes = n_words * 4;
    LPF_REQUIRE(bitmap_mode != 1 || lds_bytes <= PU_LDS_MAX);
    const bool lds = bitmap_mode == 1 || (bitmap_mode == -1 && lds_bytes <= PU_LDS_AUTO);
    const int cus = lpf_cu_count() > 0 ? lpf_cu_count() : 256;
    // resident workgroups only: each one stages the bitmap once and then walks rows with a stride
    int64_t per_cu = 8;
    if (lds && (160 * 1024) / lds_bytes < per_cu) per_cu = (160 * 1024) / lds_bytes;
    int64_t grid = (n + PU_BLOCK / 64 - 1) / (PU_BLOCK / 64);
    if (grid > cus * per_cu) grid = cus * per_cu;
    if (lds)
        hipLaunchKernelGGL(ppr_flag_rows_kernel<true>, dim3((unsigned)grid), dim3(PU_BLOCK), (size_t)lds_bytes, s, n,
                           rowptr, col, key_bitmap, n_words, flag);
    else
        hipLaunchKernelGGL(ppr_flag_rows_kernel<false>, dim3((unsigned)grid), dim3(PU_BLOCK), 0, s, n, rowptr, col,
                           key_bitmap, n_words, flag);
    LPF_CHECK_LAUNCH();
    size_t tmp = (size_t)workspace_bytes;
    if (rocprim::select(workspace, tmp, rocprim::counting_iterator<int32_t>(0), static_cast<const int32_t *>(flag), list,
                        count, (size_t)n, s) != hipSuccess)
        return LPF_ERR_LAUNCH;
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}

extern "C" int64_t lpf_ppr_splice_workspace_bytes(int64_t n, int64_t n_src, int64_t nnz_pool) {
    if (n <= 0 || n >= (1ll << 31) || n_src < 0 || n_src > n || nnz_pool < 0 || nnz_pool >= (1ll << 32)) return 0;
    size_t sort_bytes = 0, scan_bytes = 0;
    (void)rocprim::segmented_radix_sort_pairs(nullptr, sort_bytes, (const int32_t *)nullptr, (int32_t *)nullptr,
                                              (const float *)nullptr, (float *)nullptr, (unsigned)nnz_pool,
                                              (unsigned)(n_src > 0 ? n_src : 1), (const int64_t *)nullptr,
                                              (const int64_t *)nullptr, 0, 32);
    (void)rocprim::inclusive_scan(nullptr, scan_bytes, (const int64_t *)nullptr, (int64_t *)nullptr, (size_t)n,
                                  rocprim::plus<int64_t>());
    const int64_t tmp = (int64_t)(sort_bytes > scan_bytes ? sort_bytes : scan_bytes);
    return 2 * align256(nnz_pool * 4) + align256(n_src * 8) + align256(n * 8) + align256(n * 4) + align256(tmp) + 256;
}

extern "C" int lpf_ppr_splice_csr(int64_t n, const int64_t *old_rowptr, const int32_t *old_col, const float *old_val,
                                  int64_t n_src, const int32_t *sources, const int64_t *row_off, const int32_t *row_len,
                                  const int32_t *pool_col, const float *pool_val, int64_t nnz_pool, int64_t *out_rowptr,
                                  int32_t *out_col, float *out_val, int64_t out_capacity, void *workspace,
                                  int64_t workspace_bytes, void *stream) {
    LPF_REQUIRE(n >= 0 && n < (1ll << 31) && out_rowptr);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) {
        if (hipMemsetAsync(out_rowptr, 0, sizeof(int64_t), s) != hipSuccess) return LPF_ERR_LAUNCH;
        return LPF_OK;
    }
    LPF_REQUIRE(old_rowptr && old_col && old_val && n_src >= 0 && n_src <= n && nnz_pool >= 0 &&
                nnz_pool < (1ll << 32) && out_col && out_val && out_capacity >= 0 && workspace);
    LPF_REQUIRE(n_src == 0 || (sources && row_off && row_len && pool_col && pool_val));
    LPF_REQUIRE(workspace_bytes >= lpf_ppr_splice_workspace_bytes(n, n_src, nnz_pool));
    char *w = static_cast<char *>(workspace);
    int32_t *scol = reinterpret_cast<int32_t *>(w);
    w += align256(nnz_pool * 4);
    float *sval = reinterpret_cast<float *>(w);
    w += align256(nnz_pool * 4);
    int64_t *row_end = reinterpret_cast<int64_t *>(w);
    w += align256(n_src * 8);
    int64_t *len64 = reinterpret_cast<int64_t *>(w);
    w += align256(n * 8);
    int32_t *pos = reinterpret_cast<int32_t *>(w);
    w += align256(n * 4);
    const size_t tmp_bytes = (size_t)(workspace_bytes - (w - static_cast<char *>(workspace)));
    hipLaunchKernelGGL(splice_len_old_kernel, dim3((unsigned)((n + PU_BLOCK - 1) / PU_BLOCK)), dim3(PU_BLOCK), 0, s, n,
                       old_rowptr, len64, pos);
    if (n_src > 0)
        hipLaunchKernelGGL(splice_len_new_kernel, dim3((unsigned)((n_src + PU_BLOCK - 1) / PU_BLOCK)), dim3(PU_BLOCK), 0,
                           s, n, n_src, sources, row_off, row_len, len64, pos, row_end);
    LPF_CHECK_LAUNCH();
    // out_rowptr[0] = 0, out_rowptr[1..n] = inclusive scan of the row lengths
    if (hipMemsetAsync(out_rowptr, 0, sizeof(int64_t), s) != hipSuccess) return LPF_ERR_LAUNCH;
    size_t scan_bytes = tmp_bytes;
    if (rocprim::inclusive_scan(w, scan_bytes, len64, out_rowptr + 1, (size_t)n, rocprim::plus<int64_t>(), s) !=
        hipSuccess)
        return LPF_ERR_LAUNCH;
    if (n_src > 0 && nnz_pool > 0) {
        size_t sort_bytes = tmp_bytes;
        if (rocprim::segmented_radix_sort_pairs(w, sort_bytes, pool_col, scol, pool_val, sval, (unsigned)nnz_pool,
                                                (unsigned)n_src, row_off, static_cast<const int64_t *>(row_end), 0, 32,
                                                s) != hipSuccess)
            return LPF_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(splice_copy_kernel, dim3((unsigned)((n + 3) / 4)), dim3(PU_BLOCK), 0, s, n, old_rowptr, old_col,
                       old_val, pos, row_off, scol, sval, nnz_pool, out_rowptr, out_col, out_val, out_capacity);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}
