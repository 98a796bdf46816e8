// Per-node structure of the typing adjacency (structure.py): degree, core number, connected component
// and triangle count of every node of the simple undirected graph G of a binary CSR with sorted, unique int32 columns
// and a SYMMETRIC pattern.  u ~ v iff u != v and v is in row u; values are ignored; every kernel skips col == row, so
// stored self-loops change nothing.  The reference has no such code (its dataset tables come from networkx on the
// host).
//
//   lpf_node_degree        one lane per node: the row length, minus one where the row holds its own id (binary search).
//   lpf_core_sweep         one IN-PLACE sweep of the h-index iteration est[v] <- min(est[v], H_v), H_v the largest h with
//                          at least h neighbours u of est[u] >= h.  Rows of at most LPF_CORE_LONG_ROW entries: eight
//                          lanes per row, the row's estimates loaded ONCE into registers (eight per lane), H_v by
//                          bisection on h with a group count per pass (at most seven passes, no memory in them).  Longer
//                          rows (the caller lists them): one 256-thread workgroup per row, H_v from an LDS histogram of
//                          min(est[u], est[v]) and a suffix scan -- O(deg) -- while est[v] < CORE_BINS, else (or when
//                          the caller asks for it, to measure) by bisection with a workgroup count per pass, O(deg log).
//   lpf_components_hook    one lane per stored entry (u, v): where parent[u] < parent[v], integer atomic min of parent[u]
//   lpf_components_jump    into parent[parent[v]] and parent[v]; then one lane per node follows parent to its root.
//   lpf_node_triangles     one group of eight lanes per stored entry with u < v: c = |N(u) & N(v) \ {u, v}| by the
//                          sorted-row intersection of lpf_common.h (the shorter row walked, the longer binary-searched:
//                          what pair_heuristics.hip counts its common neighbours with); entries that walk more than
//                          split_threshold columns go to a list and get a whole workgroup each.  c is added to BOTH
//                          endpoints with 64-bit integer atomics -- every triangle through a node arrives over two of its
//                          edges -- and a last launch halves: the atomic form, exact in any order.
//
// Estimates and labels are read and written by other workgroups of the same launch: they go through relaxed
// agent-scope atomic loads and stores, and WHICH of a neighbour's values a lane sees changes no result (DESIGN 5.23:
// estimates only fall and stay upper bounds; labels only fall to labels of the same component).  All arithmetic is
// integer; no workgroup waits on another; every loop is bounded by n, a row length or a constant; nothing is read back.
#include "lpf_common.h"

namespace {

constexpr int NS_BLOCK = 256;                       // 4 wavefronts
constexpr int NS_WAVES = NS_BLOCK / LPF_WAVE;
constexpr int NS_GROUP = 8;                         // lanes per short row / per stored entry
constexpr int NS_PER_BLOCK = NS_BLOCK / NS_GROUP;   // short rows / entries per workgroup
constexpr int NS_SLOTS = LPF_CORE_LONG_ROW / NS_GROUP;   // estimates a lane of a short row keeps in registers
constexpr int NS_LONG_GRID = 2048;                  // workgroups over the listed long rows / long entries at most
constexpr int CORE_BINS = 4096;                     // LDS histogram bins of a long row: est[v] < CORE_BINS
static_assert(LPF_CORE_LONG_ROW % NS_GROUP == 0 && NS_SLOTS == 8, "a short row fills eight registers of eight lanes");

__device__ __forceinline__ int32_t ns_load(const int32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ns_store(int32_t *p, int32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Row v as [r0, r0 + len): empty where v or the row pointers lie outside [0, n) / [0, nnz].
__device__ __forceinline__ int32_t ns_row(const int64_t *__restrict__ rowptr, int64_t v, int64_t n, int64_t nnz,
                                          int64_t &r0) {
    r0 = 0;
    if ((uint64_t)v >= (uint64_t)n) return 0;
    const int64_t a = rowptr[v], b = rowptr[v + 1];
    if (a < 0 || b < a || b > nnz || b - a > (int64_t)INT32_MAX) return 0;
    r0 = a;
    return (int32_t)(b - a);
}

// one integer atomic per wavefront at most: the flagged lanes of a wave add their number to *counter
__device__ __forceinline__ void ns_wave_count(int32_t *counter, bool flag) {
    const uint64_t m = __ballot(flag);
    if (m && lpf_lane() == 0) atomicAdd(counter, (int32_t)__popcll(m));
}

// sum / max over the workgroup, the same value in every thread; red: NS_WAVES words of LDS, free again on return
__device__ __forceinline__ int32_t ns_block_sum(int32_t v, int32_t *red) {
#pragma unroll
    for (int m = LPF_WAVE >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m);
    if (lpf_lane() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int32_t t = 0;
#pragma unroll
    for (int w = 0; w < NS_WAVES; ++w) t += red[w];
    __syncthreads();
    return t;
}
__device__ __forceinline__ int32_t ns_block_max(int32_t v, int32_t *red) {
#pragma unroll
    for (int m = LPF_WAVE >> 1; m > 0; m >>= 1) v = max(v, __shfl_xor(v, m));
    if (lpf_lane() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int32_t t = red[0];
#pragma unroll
    for (int w = 1; w < NS_WAVES; ++w) t = max(t, red[w]);
    __syncthreads();
    return t;
}

// ------------------------------------------------------------------------------------------------------------ degree
__global__ __launch_bounds__(NS_BLOCK) void node_degree_kernel(int64_t n, int64_t nnz,
                                                               const int64_t *__restrict__ rowptr,
                                                               const int32_t *__restrict__ col,
                                                               int32_t *__restrict__ degree) {
    const int64_t v = (int64_t)blockIdx.x * NS_BLOCK + threadIdx.x;
    if (v >= n) return;
    int64_t r0;
    const int32_t len = ns_row(rowptr, v, n, nnz, r0);
    degree[v] = len - (lpf_sorted_has(col, r0, r0 + len, (int32_t)v) ? 1 : 0);
}

// -------------------------------------------------------------------------------------------------------- core sweep
// Rows of at most LPF_CORE_LONG_ROW entries, eight lanes each.  Returns through est / changed.
__device__ __forceinline__ void core_short_rows(int64_t block, int64_t n, int64_t nnz,
                                                const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                int32_t *est, int32_t *changed) {
    const int g = threadIdx.x & (NS_GROUP - 1);
    const int64_t v = block * NS_PER_BLOCK + (threadIdx.x / NS_GROUP);
    int64_t r0;
    int32_t len = ns_row(rowptr, v, n, nnz, r0);
    if (len > LPF_CORE_LONG_ROW) len = 0;              // a listed row: its workgroup's
    const int32_t mine = len > 0 ? ns_load(est + v) : 0;   // (this group is the only writer of est[v] in a sweep)
    const int32_t cur = min(mine, len);
    // the row's estimates, once: slot k of lane g is entry g + 8 k (-1: none, the node itself or a column off range)
    int32_t e[NS_SLOTS];
#pragma unroll
    for (int k = 0; k < NS_SLOTS; ++k) {
        const int32_t j = g + k * NS_GROUP;
        e[k] = -1;
        if (cur > 0 && j < len) {
            const int32_t u = col[r0 + j];
            if ((int64_t)u != v && (uint64_t)u < (uint64_t)n) e[k] = ns_load(est + u);
        }
    }
    // the largest h in [0, cur] with |{u : est[u] >= h}| >= h: the count falls as h grows, so bisection finds it
    int32_t lo = 0, hi = cur > 0 ? cur : 0;
    for (int pass = 0; pass < 32; ++pass) {            // (hi - lo halves: at most 7 passes for cur <= 64)
        const bool act = lo < hi;
        if (!__ballot(act)) break;                     // wave-uniform
        const int32_t mid = lo + ((hi - lo + 1) >> 1);
        int32_t c = 0;
#pragma unroll
        for (int k = 0; k < NS_SLOTS; ++k) c += e[k] >= mid ? 1 : 0;
#pragma unroll
        for (int m = NS_GROUP >> 1; m > 0; m >>= 1) c += __shfl_xor(c, m);
        if (act) {
            if (c >= mid) lo = mid; else hi = mid - 1;
        }
    }
    const bool dropped = g == 0 && cur > 0 && lo < mine;
    if (dropped) ns_store(est + v, lo);
    ns_wave_count(changed, dropped);
}

// Listed rows, one workgroup each.  lds: CORE_BINS + 2 * NS_WAVES + 1 words.
__device__ __forceinline__ void core_long_rows(int64_t first, int64_t stride, int64_t n, int64_t nnz,
                                               const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                               const int32_t *__restrict__ long_rows, int64_t n_long, int32_t form,
                                               int32_t *est, int32_t *changed, int32_t *lds) {
    int32_t *hist = lds, *red = lds + CORE_BINS, *wave_tot = red + NS_WAVES, *s_cur = wave_tot + NS_WAVES;
    const int tid = threadIdx.x, lane = lpf_lane(), wave = tid >> 6;
    int32_t drops = 0;                                 // thread 0's
    for (int64_t li = first; li < n_long; li += stride) {   // block-uniform
        const int64_t v = long_rows[li];
        int64_t r0;
        const int32_t len = ns_row(rowptr, v, n, nnz, r0);
        if (tid == 0) *s_cur = len > 0 ? min(ns_load(est + v), len) : 0;   // ONE read: the whole workgroup agrees
        __syncthreads();
        const int32_t cur = *s_cur;
        __syncthreads();
        if (cur <= 0) continue;                        // block-uniform
        int32_t h;
        if (form != LPF_CORE_FORM_BISECT && cur < CORE_BINS) {
            for (int32_t k = tid; k <= cur; k += NS_BLOCK) hist[k] = 0;
            __syncthreads();
            for (int32_t j = tid; j < len; j += NS_BLOCK) {
                const int32_t u = col[r0 + j];
                if ((int64_t)u == v || (uint64_t)u >= (uint64_t)n) continue;
                const int32_t x = ns_load(est + u);
                atomicAdd(&hist[x < 0 ? 0 : min(x, cur)], 1);
            }
            __syncthreads();
            // thread t owns the bins [b0, b1); above = the entries in the bins over b1 (a suffix sum over the threads)
            const int32_t per = (cur + NS_BLOCK) / NS_BLOCK;
            const int32_t b0 = min(tid * per, cur + 1), b1 = min(b0 + per, cur + 1);
            int32_t own = 0;
            for (int32_t k = b0; k < b1; ++k) own += hist[k];
            int32_t incl = own;
#pragma unroll
            for (int d = 1; d < LPF_WAVE; d <<= 1) {
                const int32_t y = __shfl_down(incl, d);
                if (lane + d < LPF_WAVE) incl += y;
            }
            if (lane == 0) wave_tot[wave] = incl;
            __syncthreads();
            int32_t run = incl - own;
            for (int w = wave + 1; w < NS_WAVES; ++w) run += wave_tot[w];
            int32_t best = 0;                          // (h = 0 always holds)
            for (int32_t k = b1 - 1; k >= b0; --k) {
                run += hist[k];
                if (run >= k) {
                    best = k;
                    break;
                }
            }
            h = ns_block_max(best, red);               // (its barriers free hist and wave_tot for the next row)
        } else {
            int32_t lo = 0, hi = cur;
            for (int pass = 0; pass < 32 && lo < hi; ++pass) {   // block-uniform: lo, hi come from workgroup sums
                const int32_t mid = lo + ((hi - lo + 1) >> 1);
                int32_t c = 0;
                for (int32_t j = tid; j < len; j += NS_BLOCK) {
                    const int32_t u = col[r0 + j];
                    if ((int64_t)u != v && (uint64_t)u < (uint64_t)n) c += ns_load(est + u) >= mid ? 1 : 0;
                }
                if (ns_block_sum(c, red) >= mid) lo = mid; else hi = mid - 1;
            }
            h = lo;
        }
        if (tid == 0 && h < ns_load(est + v)) {
            ns_store(est + v, h);
            ++drops;
        }
    }
    if (tid == 0 && drops > 0) atomicAdd(changed, drops);
}

__global__ __launch_bounds__(NS_BLOCK) void core_sweep_kernel(int64_t short_blocks, int64_t n, int64_t nnz,
                                                              const int64_t *__restrict__ rowptr,
                                                              const int32_t *__restrict__ col,
                                                              const int32_t *__restrict__ long_rows, int64_t n_long,
                                                              int32_t form, int32_t *est, int32_t *changed) {
    __shared__ int32_t lds[CORE_BINS + 2 * NS_WAVES + 1];
    if ((int64_t)blockIdx.x < short_blocks)
        core_short_rows(blockIdx.x, n, nnz, rowptr, col, est, changed);
    else
        core_long_rows((int64_t)blockIdx.x - short_blocks, (int64_t)gridDim.x - short_blocks, n, nnz, rowptr, col,
                       long_rows, n_long, form, est, changed, lds);
}

// -------------------------------------------------------------------------------------------------------- components
__global__ __launch_bounds__(NS_BLOCK) void components_hook_kernel(int64_t n, int64_t nnz,
                                                                   const int32_t *__restrict__ row,
                                                                   const int32_t *__restrict__ col, int32_t *parent,
                                                                   int32_t *changed) {
    const int64_t e = (int64_t)blockIdx.x * NS_BLOCK + threadIdx.x;
    bool lowered = false;
    if (e < nnz) {
        const int32_t u = row[e], v = col[e];
        if (u != v && (uint64_t)u < (uint64_t)n && (uint64_t)v < (uint64_t)n) {
            const int32_t pu = ns_load(parent + u), pv = ns_load(parent + v);
            if (pu >= 0 && pu < pv && (uint64_t)pv < (uint64_t)n) {
                lowered = atomicMin(parent + pv, pu) > pu;
                lowered |= atomicMin(parent + v, pu) > pu;
            }
        }
    }
    ns_wave_count(changed, lowered);
}

__global__ __launch_bounds__(NS_BLOCK) void components_jump_kernel(int64_t n, int32_t *parent) {
    const int64_t v = (int64_t)blockIdx.x * NS_BLOCK + threadIdx.x;
    if (v >= n) return;
    const int32_t p0 = ns_load(parent + v);
    int32_t p = p0;
    if ((uint64_t)p >= (uint64_t)n) return;
    for (int64_t i = 0; i < n; ++i) {                 // parent[x] <= x: the chain falls strictly until its root
        const int32_t pp = ns_load(parent + p);
        if (pp < 0 || pp >= p) break;
        p = pp;
    }
    if (p != p0) ns_store(parent + v, p);             // (this lane is the only writer of parent[v] in a jump launch)
}

// --------------------------------------------------------------------------------------------------------- triangles
struct TriEntry {
    int32_t u, v;
    LpfPairRows r;
};

// Entry e as a pair with u < v and its walked / probed rows; r.len == 0 where the entry is not counted.
__device__ __forceinline__ TriEntry tri_entry(int64_t e, int64_t n, int64_t nnz, const int64_t *__restrict__ rowptr,
                                              const int32_t *__restrict__ row, const int32_t *__restrict__ col) {
    TriEntry t{0, 0, {0, 0, 0, 0}};
    if ((uint64_t)e >= (uint64_t)nnz) return t;
    t.u = row[e];
    t.v = col[e];
    if (t.u < 0 || t.u >= t.v || (int64_t)t.v >= n) return t;
    t.r = lpf_pair_rows(t.u, t.v, n, rowptr);
    if (t.r.r0 < 0 || t.r.q0 < 0 || t.r.len < 0 || t.r.qlen < 0 || t.r.r0 + t.r.len > nnz ||
        t.r.q0 + t.r.qlen > nnz)
        t.r = LpfPairRows{0, 0, 0, 0};
    return t;
}

__device__ __forceinline__ void tri_add(int64_t *tri2, int32_t node, int32_t c) {
    atomicAdd(reinterpret_cast<unsigned long long *>(tri2 + node), (unsigned long long)c);
}

__global__ __launch_bounds__(NS_BLOCK) void tri_short_kernel(int64_t n, int64_t nnz,
                                                             const int64_t *__restrict__ rowptr,
                                                             const int32_t *__restrict__ row,
                                                             const int32_t *__restrict__ col, int32_t thr,
                                                             int32_t *__restrict__ long_list, int64_t *tri2) {
    const int g = threadIdx.x & (NS_GROUP - 1);
    const int64_t e = (int64_t)blockIdx.x * NS_PER_BLOCK + (threadIdx.x / NS_GROUP);
    const TriEntry t = tri_entry(e, n, nnz, rowptr, row, col);
    const bool is_long = t.r.len > thr;
    lpf_wave_list_push(long_list, is_long && g == 0, (int32_t)e);
    const int32_t len = is_long ? 0 : t.r.len;
    int32_t c = 0;
    for (int32_t j = g; j < len; j += NS_GROUP) {
        const int32_t key = col[t.r.r0 + j];
        if (key != t.u && key != t.v && lpf_sorted_has(col, t.r.q0, t.r.q0 + t.r.qlen, key)) ++c;
    }
#pragma unroll
    for (int m = NS_GROUP >> 1; m > 0; m >>= 1) c += __shfl_xor(c, m);
    if (g == 0 && c > 0) {
        tri_add(tri2, t.u, c);
        tri_add(tri2, t.v, c);
    }
}

__global__ __launch_bounds__(NS_BLOCK) void tri_long_kernel(int64_t n, int64_t nnz,
                                                            const int64_t *__restrict__ rowptr,
                                                            const int32_t *__restrict__ row,
                                                            const int32_t *__restrict__ col,
                                                            const int32_t *__restrict__ long_list, int64_t list_cap,
                                                            int64_t *tri2) {
    __shared__ int32_t red[NS_WAVES];
    int64_t n_long = long_list[0];
    if (n_long > list_cap) n_long = list_cap;
    for (int64_t li = blockIdx.x; li < n_long; li += gridDim.x) {   // block-uniform
        const TriEntry t = tri_entry(long_list[1 + li], n, nnz, rowptr, row, col);
        const int64_t qend = t.r.q0 + t.r.qlen;
        int64_t lo = t.r.q0;                          // this thread's keys grow: its lower bounds never move back
        int32_t c = 0;
        for (int32_t j = threadIdx.x; j < t.r.len; j += NS_BLOCK) {
            const int32_t key = col[t.r.r0 + j];
            lo = lpf_lower_bound(col, lo, qend, key);
            if (lo < qend && col[lo] == key && key != t.u && key != t.v) ++c;
        }
        c = ns_block_sum(c, red);
        if (threadIdx.x == 0 && c > 0) {
            tri_add(tri2, t.u, c);
            tri_add(tri2, t.v, c);
        }
    }
}

__global__ __launch_bounds__(NS_BLOCK) void tri_halve_kernel(int64_t n, int64_t *tri2) {
    const int64_t v = (int64_t)blockIdx.x * NS_BLOCK + threadIdx.x;
    if (v < n) tri2[v] >>= 1;
}

inline unsigned ns_blocks(int64_t items, int64_t per_block) { return (unsigned)((items + per_block - 1) / per_block); }

}  // namespace

// Limits shared by the entries: n and nnz index int32 columns and int32 list items.
#define NS_REQUIRE_GRAPH(n, nnz) LPF_REQUIRE((n) >= 0 && (n) < INT32_MAX && (nnz) >= 0 && (nnz) < INT32_MAX)

extern "C" int lpf_node_degree(int64_t n, int64_t nnz, const int64_t *rowptr, const int32_t *col, int32_t *degree,
                               void *stream) {
    NS_REQUIRE_GRAPH(n, nnz);
    LPF_REQUIRE(rowptr && degree && (col || nnz == 0));
    if (n == 0) return LPF_OK;
    hipLaunchKernelGGL(node_degree_kernel, dim3(ns_blocks(n, NS_BLOCK)), dim3(NS_BLOCK), 0,
                       static_cast<hipStream_t>(stream), n, nnz, rowptr, col, degree);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}

extern "C" int lpf_core_sweep(int64_t n, int64_t nnz, const int64_t *rowptr, const int32_t *col,
                              const int32_t *long_rows, int64_t n_long, int32_t hv_form, int32_t *est, int32_t *changed,
                              void *stream) {
    NS_REQUIRE_GRAPH(n, nnz);
    LPF_REQUIRE(rowptr && est && changed && (col || nnz == 0));
    LPF_REQUIRE(n_long >= 0 && n_long <= n && (long_rows || n_long == 0));
    LPF_REQUIRE(hv_form == LPF_CORE_FORM_DEFAULT || hv_form == LPF_CORE_FORM_BISECT);
    if (n == 0) return LPF_OK;
    const int64_t short_blocks = (n + NS_PER_BLOCK - 1) / NS_PER_BLOCK;
    const int64_t long_blocks = n_long < NS_LONG_GRID ? n_long : NS_LONG_GRID;
    hipLaunchKernelGGL(core_sweep_kernel, dim3((unsigned)(short_blocks + long_blocks)), dim3(NS_BLOCK), 0,
                       static_cast<hipStream_t>(stream), short_blocks, n, nnz, rowptr, col, long_rows, n_long, hv_form,
                       est, changed);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}

extern "C" int lpf_components_hook(int64_t n, int64_t nnz, const int32_t *row, const int32_t *col, int32_t *parent,
                                   int32_t *changed, void *stream) {
    NS_REQUIRE_GRAPH(n, nnz);
    LPF_REQUIRE(parent && changed && ((row && col) || nnz == 0));
    if (n == 0 || nnz == 0) return LPF_OK;
    hipLaunchKernelGGL(components_hook_kernel, dim3(ns_blocks(nnz, NS_BLOCK)), dim3(NS_BLOCK), 0,
                       static_cast<hipStream_t>(stream), n, nnz, row, col, parent, changed);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}

extern "C" int lpf_components_jump(int64_t n, int32_t *parent, void *stream) {
    LPF_REQUIRE(n >= 0 && n < INT32_MAX && parent);
    if (n == 0) return LPF_OK;
    hipLaunchKernelGGL(components_jump_kernel, dim3(ns_blocks(n, NS_BLOCK)), dim3(NS_BLOCK), 0,
                       static_cast<hipStream_t>(stream), n, parent);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}

extern "C" int lpf_node_triangles(int64_t n, int64_t nnz, const int64_t *rowptr, const int32_t *row,
                                  const int32_t *col, int32_t split_threshold, int32_t *scratch, int64_t *triangles,
                                  void *stream) {
    NS_REQUIRE_GRAPH(n, nnz);
    LPF_REQUIRE(rowptr && triangles && ((row && col && scratch) || nnz == 0));
    if (n == 0) return LPF_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(triangles, 0, (size_t)n * sizeof(int64_t), s);
    if (e != hipSuccess) {
        lpf_set_hip_error(e);
        return LPF_ERR_LAUNCH;
    }
    if (nnz == 0) return LPF_OK;
    const int32_t thr = split_threshold < 0 ? LPF_HEUR_SPLIT_DEFAULT : split_threshold;
    if (lpf_reset_counter(scratch, s) != LPF_OK) return LPF_ERR_LAUNCH;   // long-entry counter
    hipLaunchKernelGGL(tri_short_kernel, dim3(ns_blocks(nnz, NS_PER_BLOCK)), dim3(NS_BLOCK), 0, s, n, nnz, rowptr, row,
                       col, thr, scratch, triangles);
    LPF_CHECK_LAUNCH();
    const int64_t list_cap = nnz;                     // scratch holds 1 + nnz words: no pattern can list more entries
    const int64_t grid = list_cap < NS_LONG_GRID ? list_cap : NS_LONG_GRID;
    hipLaunchKernelGGL(tri_long_kernel, dim3((unsigned)grid), dim3(NS_BLOCK), 0, s, n, nnz, rowptr, row, col, scratch,
                       list_cap, triangles);
    LPF_CHECK_LAUNCH();
    hipLaunchKernelGGL(tri_halve_kernel, dim3(ns_blocks(n, NS_BLOCK)), dim3(NS_BLOCK), 0, s, n, triangles);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}
