// Louvain communities of the typing adjacency (community.py): one ROUND of local moves on a level graph, and
// the inside weight of a labelling.  The level graph is a CSR with sorted, unique int32 columns and a SYMMETRIC pattern,
// int64 weights (NULL: all 1) and a per-node int64 k[v] = sum_{u != v} w(v, u) + s[v]; u ~ v iff u != v and v is in row
// u, so a stored col == row is skipped everywhere.  The reference has no such code (the host baseline is
// networkx.community.louvain_communities).
//
//   lpf_community_move     for every ACTIVE node v (the top bit of lpf_mix64(lpf_draw_key(seed, (level << 32) + round)
//                          + LPF_DRAW_G (v + 1))) the neighbouring community of the best gain
//                              gain(C) = 2m w_C - k_v (tot_C - [C = cur] k_v),   w_C = sum_{u ~ v, comm[u] = C} w(v, u)
//                          among C != cur that two singletons may not swap into (cnt[cur] == 1 && cnt[C] == 1 && C > cur
//                          is dropped), gain descending, id ascending; it wins where its gain exceeds gain(cur), else v
//                          stays.  The round is double-buffered: comm / tot / cnt are read only, new_comm is written, so
//                          the result does not depend on which workgroup runs when.
//                          Rows of at most LPF_COMM_LONG_ROW entries: eight lanes per row, the row's (community, weight)
//                          pairs in registers (eight per lane), equal communities summed by rotating the pairs through
//                          the group, the arg-max by a butterfly over the group.  Every holder of a community evaluates
//                          its gain: holders of one community hold the same (gain, id), which an arg-max does not see.
//                          Longer rows (the caller lists them): persistent 256-thread workgroups stride the list.  A row
//                          of len entries takes an open-addressing table of T = 2^ceil(log2(2 len)) slots -- int32 keys
//                          (community + 1; 0: free) claimed by compare-and-swap, int64 sums by 64-bit integer adds --
//                          in LDS where T <= lds_slots, else in the workgroup's region of `scratch`; one pass over the
//                          T slots evaluates the used ones and frees them, so a table is all zero between rows.
//   lpf_community_quality  entry-parallel: the int64 sum of w over entries with row != col and equal communities; at
//                          most 1,024 workgroups stride the entries, a wavefront and a workgroup reduction, one 64-bit
//                          integer atomic per workgroup (every add lands on one word).
//
// Integers only: 2m < 2^31 bounds every k, tot and w_C by 2^31 and every product by 2^62.  No workgroup waits on
// another; every loop is bounded by a row length, a table size or the list; nothing is read back.  Ids are tested
// before they index: a row pointer outside [0, nnz] gives an empty row, a column or a community outside [0, n) is
// skipped, and a probe loop ends after T slots.
#include "draw_common.h"
#include "lpf_common.h"

namespace {

constexpr int CM_BLOCK = 256;                       // 4 wavefronts
constexpr int CM_WAVES = CM_BLOCK / LPF_WAVE;
constexpr int CM_GROUP = 8;                         // lanes per short row
constexpr int CM_PER_BLOCK = CM_BLOCK / CM_GROUP;   // short rows per workgroup
constexpr int CM_SLOTS = LPF_COMM_LONG_ROW / CM_GROUP;   // pairs a lane of a short row keeps in registers
constexpr int CM_LONG_GRID = 512;                   // persistent workgroups over the listed rows at most
constexpr int CM_BATCH = 4;                         // entries / slots a thread of a listed row requests together
constexpr int CM_QUALITY_GRID = 1024;               // workgroups of the quality kernel at most, striding the entries
constexpr int CM_SLOT_BYTES = 12;                   // an int64 sum and an int32 key
static_assert(LPF_COMM_LONG_ROW % CM_GROUP == 0 && CM_SLOTS == 8, "a short row fills eight registers of eight lanes");

__device__ __forceinline__ int32_t cm_row(const int64_t *__restrict__ rowptr, int64_t v, int64_t n, int64_t nnz,
                                          int64_t &r0) {
    r0 = 0;
    if ((uint64_t)v >= (uint64_t)n) return 0;
    const int64_t a = rowptr[v], b = rowptr[v + 1];
    if (a < 0 || b < a || b > nnz || b - a > (int64_t)INT32_MAX) return 0;
    r0 = a;
    return (int32_t)(b - a);
}

__device__ __forceinline__ bool cm_active(uint64_t round_key, int64_t v) {
    return (lpf_mix64(round_key + LPF_DRAW_G * ((uint64_t)v + 1)) >> 63) != 0;
}

// (gain, id) a beats (gain, id) b: gain descending, id ascending
__device__ __forceinline__ bool cm_better(int64_t ga, int32_t ia, int64_t gb, int32_t ib) {
    return ga > gb || (ga == gb && ia < ib);
}

struct CmArgs {
    int64_t n, nnz;
    const int64_t *rowptr;
    const int32_t *col;
    const int64_t *weight;
    const int64_t *k;
    const int32_t *comm;
    const int64_t *tot;
    const int32_t *cnt;
    int64_t two_m;
    uint64_t round_key;                             // lpf_draw_key(seed, (level << 32) + round): the kernel fills it
    int32_t *new_comm;
    int32_t *moved;
};

// ------------------------------------------------------------------------------------------------------- short rows
__device__ __forceinline__ void move_short_rows(int64_t block, const CmArgs &a) {
    const int lane = lpf_lane(), g = lane & (CM_GROUP - 1), base = lane & ~(CM_GROUP - 1);
    const int64_t v = block * CM_PER_BLOCK + (threadIdx.x / CM_GROUP);
    int64_t r0;
    int32_t len = cm_row(a.rowptr, v, a.n, a.nnz, r0);
    const bool mine = v < a.n && len <= LPF_COMM_LONG_ROW;     // (a longer row is a listed row: its workgroup's)
    const int32_t cur = mine ? a.comm[v] : -1;
    const bool act = mine && (uint64_t)cur < (uint64_t)a.n && cm_active(a.round_key, v);
    if (!act) len = 0;
    // the row's pairs, once: slot s of lane g is entry g + 8 s (-1: none, the node itself, an id off range); w_C <= k_v
    // < 2^31, so 32 bits hold a weight and every sum of a row's weights
    int32_t c[CM_SLOTS];
    uint32_t w[CM_SLOTS], sum[CM_SLOTS];
#pragma unroll
    for (int s = 0; s < CM_SLOTS; ++s) {
        const int32_t j = g + s * CM_GROUP;
        c[s] = -1;
        w[s] = 0;
        if (j < len) {
            const int32_t u = a.col[r0 + j];
            if ((int64_t)u != v && (uint64_t)u < (uint64_t)a.n) {
                const int32_t cu = a.comm[u];
                if ((uint64_t)cu < (uint64_t)a.n) {
                    c[s] = cu;
                    w[s] = a.weight ? (uint32_t)a.weight[r0 + j] : 1u;
                }
            }
        }
        sum[s] = w[s];
    }
    // one tot / cnt gather per entry, requested ahead of the rotation
    int64_t tc[CM_SLOTS];
    bool single[CM_SLOTS];
#pragma unroll
    for (int s = 0; s < CM_SLOTS; ++s) {
        tc[s] = c[s] >= 0 ? a.tot[c[s]] : 0;
        single[s] = c[s] >= 0 && a.cnt[c[s]] == 1;
    }
    const int64_t kv = act ? a.k[v] : 0, tot_cur = act ? a.tot[cur] : 0;
    const bool cur_single = act && a.cnt[cur] == 1;
    // slots in use by the longest row of the wavefront: the loops below stop there (wave-uniform)
    int used = 0;
#pragma unroll
    for (int s = 0; s < CM_SLOTS; ++s)
        if (__ballot(len > s * CM_GROUP)) used = s + 1;
    // sum[s] <- the weight of every pair of the row with c[s]'s community: the other slots of this lane, then the
    // pairs of the seven other lanes, rotated through the group
#pragma unroll
    for (int t = 0; t < CM_SLOTS; ++t) {
        if (t >= used) break;
#pragma unroll
        for (int s = 0; s < CM_SLOTS; ++s)
            if (s != t && c[s] >= 0 && c[s] == c[t]) sum[s] += w[t];
    }
    for (int rot = 1; rot < CM_GROUP; ++rot) {
        const int src = base | ((g + rot) & (CM_GROUP - 1));
#pragma unroll
        for (int t = 0; t < CM_SLOTS; ++t) {
            if (t >= used) break;
            const int32_t oc = __shfl(c[t], src);
            const uint32_t ow = __shfl(w[t], src);
#pragma unroll
            for (int s = 0; s < CM_SLOTS; ++s)
                if (c[s] >= 0 && c[s] == oc) sum[s] += ow;
        }
    }
    uint32_t w_cur = 0;
#pragma unroll
    for (int s = 0; s < CM_SLOTS; ++s) w_cur += c[s] == cur ? w[s] : 0u;
#pragma unroll
    for (int m = CM_GROUP >> 1; m > 0; m >>= 1) w_cur += __shfl_xor(w_cur, m);
    const int64_t stay = a.two_m * (int64_t)w_cur - kv * (tot_cur - kv);
    int64_t best_gain = INT64_MIN;
    int32_t best = INT32_MAX;
#pragma unroll
    for (int s = 0; s < CM_SLOTS; ++s) {
        if (c[s] < 0 || c[s] == cur || (cur_single && single[s] && c[s] > cur)) continue;
        const int64_t gain = a.two_m * (int64_t)sum[s] - kv * tc[s];
        if (cm_better(gain, c[s], best_gain, best)) {
            best_gain = gain;
            best = c[s];
        }
    }
#pragma unroll
    for (int m = CM_GROUP >> 1; m > 0; m >>= 1) {
        const int64_t og = __shfl_xor(best_gain, m);
        const int32_t ob = __shfl_xor(best, m);
        if (cm_better(og, ob, best_gain, best)) {
            best_gain = og;
            best = ob;
        }
    }
    const bool moves = act && best != INT32_MAX && best_gain > stay;
    if (mine && g == 0) a.new_comm[v] = moves ? best : cur;
    const uint64_t mm = __ballot(moves && g == 0);
    if (mm && lane == 0) atomicAdd(a.moved, (int32_t)__popcll(mm));
}

// -------------------------------------------------------------------------------------------------------- long rows
// The table of one row: sums[T], keys[T], all zero on entry and on return.  GLOBAL: the table lies in device memory
// and is read and freed through agent-scope atomics (its adds and claims are served by the L2, so no line of it may be
// read from a cache nearer than that); else in LDS.
template <bool GLOBAL>
__device__ __forceinline__ int32_t cm_key_load(int32_t *p) {
    if constexpr (GLOBAL) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}
template <bool GLOBAL>
__device__ __forceinline__ int64_t cm_sum_load(int64_t *p) {
    if constexpr (GLOBAL) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}
template <bool GLOBAL>
__device__ __forceinline__ void cm_slot_free(int32_t *key, int64_t *sum) {
    if constexpr (GLOBAL) {
        __hip_atomic_store(key, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(sum, (int64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        *key = 0;
        *sum = 0;
    }
}

struct CmRed {                                      // the workgroup's reduction words (LDS)
    int64_t gain[CM_WAVES];
    int32_t id[CM_WAVES];
    uint32_t w_cur;
};

// One listed, active row v with community cur: returns (thread 0 only) whether it moved; writes new_comm[v].
template <bool GLOBAL>
__device__ __forceinline__ bool move_long_row(const CmArgs &a, int64_t v, int32_t cur, int64_t r0, int32_t len,
                                              int64_t T, int bits, int64_t *sums, int32_t *keys, CmRed *red) {
    const int tid = threadIdx.x;
    const int64_t mask = T - 1;
    if (tid == 0) red->w_cur = 0;
    // CM_BATCH entries per thread and step: their columns, then their communities and weights are requested together
    // (an index that fails its test is replaced by one that holds -- entry j0, node v -- so that no load waits for a
    // branch), then each valid pair is inserted
    for (int32_t j0 = tid; j0 < len; j0 += CM_BATCH * CM_BLOCK) {
        int32_t u[CM_BATCH], cu[CM_BATCH];
        int64_t wj[CM_BATCH];
        bool ok[CM_BATCH];
#pragma unroll
        for (int q = 0; q < CM_BATCH; ++q) {
            const int32_t j = j0 + q * CM_BLOCK;
            ok[q] = j < len;
            const int64_t e = r0 + (ok[q] ? j : j0);
            u[q] = a.col[e];
            wj[q] = a.weight ? a.weight[e] : 1;
        }
#pragma unroll
        for (int q = 0; q < CM_BATCH; ++q) {
            ok[q] = ok[q] && (int64_t)u[q] != v && (uint64_t)u[q] < (uint64_t)a.n;
            cu[q] = a.comm[ok[q] ? (int64_t)u[q] : v];
            ok[q] = ok[q] && (uint64_t)cu[q] < (uint64_t)a.n;
        }
#pragma unroll
        for (int q = 0; q < CM_BATCH; ++q) {
            if (!ok[q]) continue;
            int64_t h = (int64_t)(((uint32_t)cu[q] * 2654435761u) >> (32 - bits));
            for (int64_t probe = 0; probe < T; ++probe) {      // (at most len <= T / 2 slots are ever claimed)
                const int32_t old = atomicCAS(keys + h, 0, cu[q] + 1);
                if (old == 0 || old == cu[q] + 1) {
                    atomicAdd(reinterpret_cast<unsigned long long *>(sums + h), (unsigned long long)wj[q]);
                    break;
                }
                h = (h + 1) & mask;
            }
        }
    }
    __syncthreads();
    const int64_t kv = a.k[v];
    const bool cur_single = a.cnt[cur] == 1;
    int64_t best_gain = INT64_MIN;
    int32_t best = INT32_MAX;
    // the pass over the T slots, CM_BATCH per thread and step in the same way: keys and sums, then tot and cnt of the
    // used slots' communities (of cur where a slot is free: an index that holds)
    for (int64_t i0 = tid; i0 < T; i0 += CM_BATCH * CM_BLOCK) {
        int32_t cc[CM_BATCH];
        int64_t wc[CM_BATCH], tc[CM_BATCH];
        bool used[CM_BATCH], single[CM_BATCH];
#pragma unroll
        for (int q = 0; q < CM_BATCH; ++q) {
            const int64_t i = i0 + q * CM_BLOCK;
            const int64_t ic = i < T ? i : i0;
            cc[q] = cm_key_load<GLOBAL>(keys + ic) - 1;
            wc[q] = cm_sum_load<GLOBAL>(sums + ic);
            used[q] = i < T && cc[q] != -1;
        }
#pragma unroll
        for (int q = 0; q < CM_BATCH; ++q) {
            if ((uint64_t)cc[q] >= (uint64_t)a.n) cc[q] = -1;  // (only a scratch that was not zero holds such a key)
            const int32_t ci = used[q] && cc[q] >= 0 ? cc[q] : cur;
            tc[q] = a.tot[ci];
            single[q] = a.cnt[ci] == 1;
        }
#pragma unroll
        for (int q = 0; q < CM_BATCH; ++q) {
            if (!used[q]) continue;
            const int64_t i = i0 + q * CM_BLOCK;
            cm_slot_free<GLOBAL>(keys + i, sums + i);
            if (cc[q] < 0) continue;
            if (cc[q] == cur) {
                red->w_cur = (uint32_t)wc[q];                   // (one slot holds cur: one writer)
                continue;
            }
            if (cur_single && cc[q] > cur && single[q]) continue;
            const int64_t gain = a.two_m * wc[q] - kv * tc[q];
            if (cm_better(gain, cc[q], best_gain, best)) {
                best_gain = gain;
                best = cc[q];
            }
        }
    }
#pragma unroll
    for (int m = LPF_WAVE >> 1; m > 0; m >>= 1) {
        const int64_t og = __shfl_xor(best_gain, m);
        const int32_t ob = __shfl_xor(best, m);
        if (cm_better(og, ob, best_gain, best)) {
            best_gain = og;
            best = ob;
        }
    }
    if (lpf_lane() == 0) {
        red->gain[tid >> 6] = best_gain;
        red->id[tid >> 6] = best;
    }
    __syncthreads();                                            // (also: the table is free before the next row claims)
    bool moves = false;
    if (tid == 0) {
#pragma unroll
        for (int wv = 1; wv < CM_WAVES; ++wv)
            if (cm_better(red->gain[wv], red->id[wv], best_gain, best)) {
                best_gain = red->gain[wv];
                best = red->id[wv];
            }
        const int64_t stay = a.two_m * (int64_t)red->w_cur - kv * (a.tot[cur] - kv);
        moves = best != INT32_MAX && best_gain > stay;
        a.new_comm[v] = moves ? best : cur;
    }
    return moves;
}

__device__ __forceinline__ void move_long_rows(int64_t first, int64_t stride, const CmArgs &a,
                                               const int32_t *__restrict__ long_rows, int64_t n_long,
                                               int32_t lds_slots, char *scratch, int64_t region_slots, char *lds,
                                               CmRed *red) {
    const int tid = threadIdx.x;
    int64_t *lds_sums = reinterpret_cast<int64_t *>(lds);
    int32_t *lds_keys = reinterpret_cast<int32_t *>(lds + (size_t)lds_slots * sizeof(int64_t));
    for (int32_t i = tid; i < lds_slots; i += CM_BLOCK) {
        lds_sums[i] = 0;
        lds_keys[i] = 0;
    }
    __syncthreads();
    char *region = scratch ? scratch + (size_t)first * (size_t)region_slots * CM_SLOT_BYTES : nullptr;
    int64_t *glb_sums = reinterpret_cast<int64_t *>(region);
    int32_t *glb_keys = reinterpret_cast<int32_t *>(region + (size_t)region_slots * sizeof(int64_t));
    int32_t n_moved = 0;                                        // thread 0's
    for (int64_t li = first; li < n_long; li += stride) {       // block-uniform
        const int64_t v = long_rows[li];
        int64_t r0;
        const int32_t len = cm_row(a.rowptr, v, a.n, a.nnz, r0);
        if (len <= LPF_COMM_LONG_ROW) continue;                 // (off range, or a short row: its group's)
        const int32_t cur = a.comm[v];
        int bits = 6;
        while (((int64_t)1 << bits) < 2 * (int64_t)len) ++bits;      // T >= 2 len: at most half of the table fills
        const int64_t T = (int64_t)1 << bits;
        const bool in_lds = T <= lds_slots;
        if ((uint64_t)cur >= (uint64_t)a.n || !cm_active(a.round_key, v) || (!in_lds && T > region_slots)) {
            if (tid == 0) a.new_comm[v] = cur;                  // (a row no table holds stays: the caller sized it)
            continue;
        }
        const bool moves = in_lds ? move_long_row<false>(a, v, cur, r0, len, T, bits, lds_sums, lds_keys, red)
                                  : move_long_row<true>(a, v, cur, r0, len, T, bits, glb_sums, glb_keys, red);
        n_moved += moves ? 1 : 0;
    }
    if (tid == 0 && n_moved > 0) atomicAdd(a.moved, n_moved);
}

__global__ __launch_bounds__(CM_BLOCK) void community_move_kernel(int64_t short_blocks, CmArgs a, uint64_t seed,
                                                                  uint64_t slot,
                                                                  const int32_t *__restrict__ long_rows,
                                                                  int64_t n_long, int32_t lds_slots, char *scratch,
                                                                  int64_t region_slots) {
    extern __shared__ __attribute__((aligned(16))) char cm_lds[];
    __shared__ CmRed red;
    a.round_key = lpf_draw_key(seed, slot);
    if ((int64_t)blockIdx.x < short_blocks)
        move_short_rows(blockIdx.x, a);
    else
        move_long_rows((int64_t)blockIdx.x - short_blocks, (int64_t)gridDim.x - short_blocks, a, long_rows, n_long,
                       lds_slots, scratch, region_slots, cm_lds, &red);
}

// ---------------------------------------------------------------------------------------------------------- quality
__global__ __launch_bounds__(CM_BLOCK) void community_quality_kernel(int64_t n, int64_t nnz,
                                                                     const int32_t *__restrict__ row,
                                                                     const int32_t *__restrict__ col,
                                                                     const int64_t *__restrict__ weight,
                                                                     const int32_t *__restrict__ comm,
                                                                     int64_t *inside) {
    __shared__ int64_t red[CM_WAVES];
    int64_t x = 0;
    for (int64_t e = (int64_t)blockIdx.x * CM_BLOCK + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * CM_BLOCK) {
        const int32_t u = row[e], v = col[e];
        if (u != v && (uint64_t)u < (uint64_t)n && (uint64_t)v < (uint64_t)n && comm[u] == comm[v])
            x += weight ? weight[e] : 1;
    }
#pragma unroll
    for (int m = LPF_WAVE >> 1; m > 0; m >>= 1) x += __shfl_xor(x, m);
    if (lpf_lane() == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    // every add lands on ONE word: the workgroups stride the entries (CM_QUALITY_GRID of them at most) and each adds once
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < CM_WAVES; ++w) x += red[w];
        if (x != 0) atomicAdd(reinterpret_cast<unsigned long long *>(inside), (unsigned long long)x);
    }
}

inline bool cm_slots_ok(int32_t s) { return s >= 64 && s <= LPF_COMM_LDS_SLOTS_MAX && (s & (s - 1)) == 0; }
inline int64_t cm_long_blocks(int64_t n_long) { return n_long < CM_LONG_GRID ? n_long : CM_LONG_GRID; }
// slots of the table of a row of max_row entries
inline int64_t cm_table_slots(int64_t max_row) {
    int64_t t = 64;
    while (t < 2 * max_row) t <<= 1;
    return t;
}

}  // namespace

#define CM_REQUIRE_GRAPH(n, nnz) LPF_REQUIRE((n) >= 0 && (n) < INT32_MAX && (nnz) >= 0 && (nnz) < INT32_MAX)

extern "C" int64_t lpf_community_workspace_bytes(int64_t n_long, int64_t max_row, int32_t lds_slots) {
    if (n_long < 0 || max_row < 0 || max_row >= INT32_MAX || !cm_slots_ok(lds_slots)) return LPF_ERR_INVALID;
    const int64_t t = cm_table_slots(max_row);
    if (n_long == 0 || max_row <= LPF_COMM_LONG_ROW || t <= lds_slots) return 0;
    return cm_long_blocks(n_long) * t * CM_SLOT_BYTES;
}

extern "C" int lpf_community_move(int64_t n, int64_t nnz, const int64_t *rowptr, const int32_t *col,
                                  const int64_t *weight, const int64_t *k, const int32_t *comm, const int64_t *tot,
                                  const int32_t *cnt, int64_t two_m, uint64_t seed, int32_t level, int32_t round,
                                  const int32_t *long_rows, int64_t n_long, int32_t lds_slots, void *scratch,
                                  int64_t scratch_bytes, int32_t *new_comm, int32_t *moved, void *stream) {
    CM_REQUIRE_GRAPH(n, nnz);
    LPF_REQUIRE(rowptr && k && comm && tot && cnt && new_comm && moved && (col || nnz == 0));
    LPF_REQUIRE(two_m >= 0 && two_m < ((int64_t)1 << 31) && level >= 0 && round >= 0);
    LPF_REQUIRE(n_long >= 0 && n_long <= n && (long_rows || n_long == 0));
    LPF_REQUIRE(cm_slots_ok(lds_slots) && scratch_bytes >= 0 && (scratch || scratch_bytes == 0));
    if (n == 0) return LPF_OK;
    const int64_t short_blocks = (n + CM_PER_BLOCK - 1) / CM_PER_BLOCK;
    const int64_t long_blocks = cm_long_blocks(n_long);
    // the largest power of two of slots that every workgroup's region holds
    int64_t region_slots = 0;
    if (long_blocks > 0 && scratch_bytes / (long_blocks * CM_SLOT_BYTES) >= 64) {
        region_slots = 64;
        while (region_slots * 2 <= scratch_bytes / (long_blocks * CM_SLOT_BYTES)) region_slots <<= 1;
    }
    const size_t lds = long_blocks > 0 ? (size_t)lds_slots * CM_SLOT_BYTES : 0;
    LPF_SET_MAX_LDS(community_move_kernel, lds + sizeof(CmRed));
    const uint64_t slot = ((uint64_t)(uint32_t)level << 32) + (uint64_t)(uint32_t)round;
    const CmArgs a{n, nnz, rowptr, col, weight, k, comm, tot, cnt, two_m, 0, new_comm, moved};
    hipLaunchKernelGGL(community_move_kernel, dim3((unsigned)(short_blocks + long_blocks)), dim3(CM_BLOCK), lds,
                       static_cast<hipStream_t>(stream), short_blocks, a, seed, slot, long_rows, n_long, lds_slots,
                       static_cast<char *>(scratch), region_slots);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}

extern "C" int lpf_community_quality(int64_t n, int64_t nnz, const int32_t *row, const int32_t *col,
                                     const int64_t *weight, const int32_t *comm, int64_t *inside, void *stream) {
    CM_REQUIRE_GRAPH(n, nnz);
    LPF_REQUIRE(inside && ((row && col && comm) || nnz == 0));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const hipError_t e = hipMemsetAsync(inside, 0, sizeof(int64_t), s);
    if (e != hipSuccess) {
        lpf_set_hip_error(e);
        return LPF_ERR_LAUNCH;
    }
    if (n == 0 || nnz == 0) return LPF_OK;
    const int64_t blocks = (nnz + CM_BLOCK - 1) / CM_BLOCK;
    hipLaunchKernelGGL(community_quality_kernel, dim3((unsigned)(blocks < CM_QUALITY_GRID ? blocks : CM_QUALITY_GRID)),
                       dim3(CM_BLOCK), 0, s, n, nnz, row, col, weight, comm, inside);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}
