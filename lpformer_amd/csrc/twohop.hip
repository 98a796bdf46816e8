// HeaRT-style hard negatives on the device: two-hop rows, the candidate pool of a node, and the rank interleave.
//
// 1. Two-hop rows (lpf_twohop_count / lpf_twohop_fill).  Row u of A diag(w) A on a binary CSR with sorted, unique int32
//    columns: for each w in N(u) in ascending order, for each c in N(w):  cn[c] += 1, aa[c] += w_aa[w],
//    ra[c] += w_ra[w].  Output: the touched c in ascending id with their sums.  The sums are fp64, added in ascending w
//    and rounded to fp32 once; w is sequential per source and the lanes spread over N(w), whose entries are distinct,
//    so no two lanes touch one accumulator in a step: no float atomics, and the order of the additions depends on the
//    source alone.  Two classes of work, split by the expansion E(u) = sum over w in N(u) of deg(w):
//    * E <= split_threshold (at most TH_WAVE_CAP = 512): one wavefront per source, the accumulators hashed in LDS
//      (1024 slots, open addressing on c with linear probing, at most half full), the live slots compacted by ballot
//      rank and their (id, slot) keys bitonic-sorted in LDS.  28 KiB of LDS per wavefront: five per CU.
//    * larger E: the wave kernel appends the source to a list (an int32 ticket) and a second kernel gives each listed
//      source a 256-thread workgroup with dense state over all n nodes in the caller's workspace (per group: fp64 aa,
//      fp64 ra, int32 cn, int32 stamp; an entry is live when its stamp equals the group's epoch, which grows by one
//      per source, so nothing is cleared between sources).  Up to TH_SORT_CAP = 8192 touched ids are collected in LDS
//      and bitonic-sorted there; a longer row is emitted by an ordered sweep of the stamps (a counting sort by id).
//    flags: bit 0 drops the members of N(u), bit 1 drops u, at output time (the sums are not affected).
//    Both passes classify a source the same way, so the fill pass writes exactly the counted entries.
//
// 2. Pool (lpf_pool_extra_count / lpf_pool_fill).  The pool of u is its two-hop row A' (already without N(u) and u)
//    united with the stored entries of its PPR row B, minus N(u), minus u, ascending id, the values carried along.
//    The entries of B that are kept and not in A' ("extra") are counted, scanned by the caller and written to a
//    temporary row X; A' and X are disjoint and sorted, so the union position of A'[i] is i + lower_bound(X, A'[i]) and
//    that of X[j] is j + lower_bound(A', X[j]).  One wavefront per node, ranks by ballot: no atomics.
//
// 3. Rank interleave (lpf_rank_interleave).  Per node: H ranked lists (segmented top-K outputs), each cut at its first
//    value that is not > 0; walk rank 1 of list 1, rank 1 of list 2, ..., rank 2 of list 1, ... and keep the first
//    `kh` distinct ids; then pad with the draws d = 0, 1, ... of lpf_pad_draw(seed, u, d, n), skipping u, N(u) and ids
//    already kept.  One wavefront per node, 64 sequence elements per round: an element is kept when it is the first
//    holder of its id, decided by an LDS hash (key = id) with an atomicMin on the sequence index; positions come from
//    the round's ballot.  A pure function of (lists, seed, u, N(u)).
#include "lpf_common.h"

namespace {

constexpr int TH_WAVE_CAP = LPF_TWOHOP_SPLIT_DEFAULT;   // largest expansion the wave class takes
constexpr int TH_TABLE = 2 * TH_WAVE_CAP;       // hash slots per wavefront
constexpr int TH_BLOCK = 256;                   // workgroup class: 4 wavefronts
constexpr int TH_WAVES = TH_BLOCK / LPF_WAVE;
constexpr int TH_SORT_CAP = 8192;               // touched ids a workgroup sorts in LDS (32 KiB)
constexpr int POOL_BLOCK = 256;
constexpr int POOL_WAVES = POOL_BLOCK / LPF_WAVE;
constexpr int IL_TABLE = 2048;                  // interleave: hash slots (at most kh + 63 <= 1087 ids are ever inserted)
constexpr int IL_MAX_H = 8;
constexpr int IL_MAX_DRAWS = 1 << 20;           // padding draws before the kernel gives up (the host checks feasibility)

static_assert((TH_TABLE & (TH_TABLE - 1)) == 0, "hash size must be a power of two");

struct THArgs {
    int64_t S, n;
    const int64_t *src;
    const int64_t *rowptr;
    const int32_t *col;
    const float *w_aa, *w_ra;
    int32_t thr, flags;
    int32_t *long_list;
    int64_t *count;                             // count pass
    const int64_t *offset;                      // fill pass: first output slot of each source (NULL in the count pass)
    int64_t T;
    int32_t *out_col, *out_cn;
    float *out_aa, *out_ra;
    double *ws_aa, *ws_ra;                      // [n_groups][n]
    int32_t *ws_stamp, *ws_cn;                  // [n_groups][n]
};

// whether touched id c of source u (row [r0, r1)) is written
__device__ __forceinline__ bool th_keep(const THArgs &A, int64_t u, int64_t r0, int64_t r1, int32_t c) {
    if ((A.flags & 2) && c == u) return false;
    if ((A.flags & 1) && lpf_sorted_has(A.col, r0, r1, c)) return false;
    return true;
}

__device__ __forceinline__ uint32_t th_hash(int32_t c) { return ((uint32_t)c * 2654435761u) >> 22; }   // 10 bits
static_assert(TH_TABLE == 1024, "th_hash yields 10 bits");

// ascending bitonic sort of a[0 .. p2) in LDS by `threads` threads (p2 a power of two, uniform over the workgroup)
template <typename T>
__device__ __forceinline__ void th_bitonic(T *a, int p2, int tid, int threads) {
    for (int size = 2; size <= p2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < (p2 >> 1); i += threads) {
                const int idx = ((i / stride) * (stride << 1)) + (i % stride);
                const int par = idx + stride;
                const bool asc = (idx & size) == 0;
                const T x = a[idx], y = a[par];
                if ((x > y) == asc) {
                    a[idx] = y;
                    a[par] = x;
                }
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ int th_pow2(int m) {
    int p = 2;
    while (p < m) p <<= 1;
    return p;
}

__global__ __launch_bounds__(LPF_WAVE) void twohop_wave_kernel(THArgs A) {
    __shared__ int32_t keys[TH_TABLE];
    __shared__ int32_t cnt[TH_TABLE];
    __shared__ double saa[TH_TABLE], sra[TH_TABLE];
    __shared__ uint64_t srt[TH_WAVE_CAP];
    const int lane = threadIdx.x;
    const int64_t s = blockIdx.x;
    const int64_t u = A.src[s];
    if ((uint64_t)u >= (uint64_t)A.n) {           // (ids outside [0, n): an empty row)
        if (!A.offset && lane == 0) A.count[s] = 0;
        return;
    }
    const int64_t r0 = A.rowptr[u], r1 = A.rowptr[u + 1];
    long long e = 0;
    for (int64_t j = r0 + lane; j < r1; j += LPF_WAVE) {
        const int32_t w = A.col[j];
        if ((uint64_t)w < (uint64_t)A.n) e += (long long)(A.rowptr[w + 1] - A.rowptr[w]);
    }
#pragma unroll
    for (int m = LPF_WAVE >> 1; m > 0; m >>= 1) e += __shfl_xor(e, m);
    if (e > (long long)A.thr) {                   // wave-uniform
        if (lane == 0) A.long_list[1 + atomicAdd(&A.long_list[0], 1)] = (int32_t)s;
        return;
    }
    for (int i = lane; i < TH_TABLE; i += LPF_WAVE) keys[i] = -1;
    __syncthreads();
    const bool fill = A.offset != nullptr;
    for (int64_t j = r0; j < r1; ++j) {           // w ascending, one at a time
        const int32_t w = A.col[j];
        if ((uint64_t)w >= (uint64_t)A.n) continue;
        const int64_t s0 = A.rowptr[w], s1 = A.rowptr[w + 1];
        const double wa = (fill && A.w_aa) ? (double)A.w_aa[w] : 0.0;
        const double wr = (fill && A.w_ra) ? (double)A.w_ra[w] : 0.0;
        for (int64_t i = s0 + lane; i < s1; i += LPF_WAVE) {
            const int32_t c = A.col[i];
            if ((uint64_t)c >= (uint64_t)A.n) continue;
            uint32_t slot = th_hash(c);
            int32_t prev;
            for (;;) {                            // at most 512 of the 1024 slots are ever taken: this ends
                prev = atomicCAS(&keys[slot], -1, c);
                if (prev == -1 || prev == c) break;
                slot = (slot + 1) & (TH_TABLE - 1);
            }
            if (fill) {
                if (prev == -1) {                 // (0.0 + x == x exactly: the same bits as starting from zero)
                    cnt[slot] = 1;
                    saa[slot] = wa;
                    sra[slot] = wr;
                } else {
                    cnt[slot] += 1;
                    saa[slot] += wa;
                    sra[slot] += wr;
                }
            }
        }
        __syncthreads();                          // the next w may touch the same accumulators
    }
    // the live slots that are written, compacted by ballot rank
    int32_t m = 0;
    for (int base = 0; base < TH_TABLE; base += LPF_WAVE) {
        const int32_t k = keys[base + lane];
        const bool keep = k >= 0 && th_keep(A, u, r0, r1, k);
        const uint64_t bm = __ballot(keep);
        if (fill && keep) srt[m + __popcll(bm & ((1ull << lane) - 1ull))] = ((uint64_t)(uint32_t)k << 32) | (uint32_t)(base + lane);
        m += __popcll(bm);
    }
    if (!fill) {
        if (lane == 0) A.count[s] = m;
        return;
    }
    if (m == 0) return;
    const int p2 = th_pow2(m);
    for (int i = m + lane; i < p2; i += LPF_WAVE) srt[i] = ~0ull;
    __syncthreads();
    th_bitonic(srt, p2, lane, LPF_WAVE);
    const int64_t out0 = A.offset[s];
    for (int i = lane; i < m; i += LPF_WAVE) {
        const uint64_t v = srt[i];
        const uint32_t slot = (uint32_t)v;
        const int64_t pos = out0 + i;
        if (pos < A.T) {                          // (always: the fill pass writes the slots the count pass counted)
            A.out_col[pos] = (int32_t)(v >> 32);
            if (A.out_cn) A.out_cn[pos] = cnt[slot];
            if (A.out_aa) A.out_aa[pos] = (float)saa[slot];
            if (A.out_ra) A.out_ra[pos] = (float)sra[slot];
        }
    }
}

__global__ __launch_bounds__(TH_BLOCK) void twohop_group_kernel(THArgs A) {
    __shared__ int32_t lst[TH_SORT_CAP];
    __shared__ int32_t m_sh;
    __shared__ int32_t wave_cnt[TH_WAVES];
    const int tid = threadIdx.x, lane = lpf_lane(), wave = tid >> 6;
    const int64_t g = blockIdx.x;
    double *aa = A.ws_aa + g * A.n, *ra = A.ws_ra + g * A.n;
    int32_t *stamp = A.ws_stamp + g * A.n, *cn = A.ws_cn + g * A.n;
    const bool fill = A.offset != nullptr;
    const int32_t n_long = A.long_list[0];
    int32_t epoch = 0;                            // the stamps are zeroed before the launch
    for (int32_t li = blockIdx.x; li < n_long; li += gridDim.x) {   // block-uniform
        ++epoch;
        const int64_t s = A.long_list[1 + li];
        const int64_t u = A.src[s];
        const int64_t r0 = A.rowptr[u], r1 = A.rowptr[u + 1];
        if (tid == 0) m_sh = 0;
        __syncthreads();
        for (int64_t j = r0; j < r1; ++j) {       // w ascending, one at a time
            const int32_t w = A.col[j];
            if ((uint64_t)w >= (uint64_t)A.n) continue;
            const int64_t s0 = A.rowptr[w], s1 = A.rowptr[w + 1];
            const double wa = (fill && A.w_aa) ? (double)A.w_aa[w] : 0.0;
            const double wr = (fill && A.w_ra) ? (double)A.w_ra[w] : 0.0;
            for (int64_t i = s0 + tid; i < s1; i += TH_BLOCK) {
                const int32_t c = A.col[i];
                if ((uint64_t)c >= (uint64_t)A.n) continue;
                if (stamp[c] != epoch) {
                    stamp[c] = epoch;
                    if (fill) {
                        cn[c] = 1;
                        aa[c] = wa;
                        ra[c] = wr;
                    }
                    const int32_t p = atomicAdd(&m_sh, 1);
                    if (p < TH_SORT_CAP) lst[p] = c;
                } else if (fill) {
                    cn[c] += 1;
                    aa[c] += wa;
                    ra[c] += wr;
                }
            }
            __syncthreads();                      // the next w may touch the same accumulators
        }
        const int32_t m = m_sh;                   // touched ids
        if (!fill) {
            // the count: touched ids minus the dropped ones that were touched
            int32_t drop = 0;
            if (A.flags & 1)
                for (int64_t j = r0 + tid; j < r1; j += TH_BLOCK) {
                    const int32_t x = A.col[j];
                    if ((uint64_t)x < (uint64_t)A.n && stamp[x] == epoch) ++drop;
                }
            if (tid == 0 && (A.flags & 2) && stamp[u] == epoch &&
                !((A.flags & 1) && lpf_sorted_has(A.col, r0, r1, (int32_t)u)))
                ++drop;
            __syncthreads();                      // every thread has read m_sh
            if (drop) atomicSub(&m_sh, drop);
            __syncthreads();
            if (tid == 0) A.count[s] = m_sh;
            __syncthreads();                      // m_sh is rewritten by the next source
            continue;
        }
        const bool sorted = m <= TH_SORT_CAP;
        int64_t M = A.n;                          // sweep: every id of [0, n), live ones kept
        if (sorted) {
            const int p2 = th_pow2(m);
            for (int i = m + tid; i < p2; i += TH_BLOCK) lst[i] = INT32_MAX;
            __syncthreads();
            th_bitonic(lst, p2, tid, TH_BLOCK);
            M = m;
        }
        const int64_t out0 = A.offset[s];
        int64_t base = 0;
        for (int64_t i0 = 0; i0 < M; i0 += TH_BLOCK) {
            const int64_t i = i0 + tid;
            int32_t c = 0;
            bool keep = false;
            if (i < M) {
                c = sorted ? lst[i] : (int32_t)i;
                keep = (sorted || stamp[c] == epoch) && th_keep(A, u, r0, r1, c);
            }
            const uint64_t bm = __ballot(keep);
            if (lane == 0) wave_cnt[wave] = __popcll(bm);
            __syncthreads();
            int64_t before = 0, total = 0;
#pragma unroll
            for (int q = 0; q < TH_WAVES; ++q) {
                before += q < wave ? wave_cnt[q] : 0;
                total += wave_cnt[q];
            }
            if (keep) {
                const int64_t pos = out0 + base + before + __popcll(bm & ((1ull << lane) - 1ull));
                if (pos < A.T) {
                    A.out_col[pos] = c;
                    if (A.out_cn) A.out_cn[pos] = cn[c];
                    if (A.out_aa) A.out_aa[pos] = (float)aa[c];
                    if (A.out_ra) A.out_ra[pos] = (float)ra[c];
                }
            }
            base += total;
            __syncthreads();                      // wave_cnt is rewritten by the next round
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- pool
struct PoolArgs {
    int64_t U, n;
    const int64_t *nodes;
    const int64_t *a_ptr;                       // [U + 1]: two-hop rows (without N(u) and u)
    const int32_t *a_col, *a_cn;
    const float *a_aa, *a_ra;
    const int64_t *b_rowptr;                    // the PPR CSR
    const int32_t *b_col;
    const float *b_val;
    const int64_t *exc_rowptr;                  // the adjacency
    const int32_t *exc_col;
    int64_t *count;                             // extra count pass
    const int64_t *x_ptr;                       // [U + 1]: scan of the extra counts
    int32_t *x_col;
    float *x_val;
    int64_t X, T;
    int64_t *pairs;                             // [2, T]
    float *o_cn, *o_aa, *o_ra, *o_ppr;
};

// mode 0: count the extra entries; mode 1: write them to x_col / x_val
template <int MODE>
__global__ __launch_bounds__(POOL_BLOCK) void pool_extra_kernel(PoolArgs A) {
    const int lane = lpf_lane();
    const int64_t i = (int64_t)blockIdx.x * POOL_WAVES + (threadIdx.x >> 6);
    if (i >= A.U) return;                       // wave-uniform
    const int64_t u = A.nodes[i];
    if ((uint64_t)u >= (uint64_t)A.n) {
        if (MODE == 0 && lane == 0) A.count[i] = 0;
        return;
    }
    const int64_t b0 = A.b_rowptr[u], b1 = A.b_rowptr[u + 1];
    const int64_t e0 = A.exc_rowptr[u], e1 = A.exc_rowptr[u + 1];
    const int64_t a0 = A.a_ptr[i], a1 = A.a_ptr[i + 1];
    const int64_t x0 = MODE ? A.x_ptr[i] : 0;
    int64_t base = 0;
    for (int64_t j0 = b0; j0 < b1; j0 += LPF_WAVE) {   // wave-uniform trip count
        const int64_t j = j0 + lane;
        int32_t c = 0;
        bool keep = false;
        if (j < b1) {
            c = A.b_col[j];
            keep = (uint64_t)c < (uint64_t)A.n && c != u && !lpf_sorted_has(A.exc_col, e0, e1, c) &&
                   !lpf_sorted_has(A.a_col, a0, a1, c);
        }
        const uint64_t bm = __ballot(keep);
        if (MODE && keep) {
            const int64_t pos = x0 + base + __popcll(bm & ((1ull << lane) - 1ull));
            if (pos < A.X) {
                A.x_col[pos] = c;
                A.x_val[pos] = A.b_val[j];
            }
        }
        base += __popcll(bm);
    }
    if (MODE == 0 && lane == 0) A.count[i] = base;
}

__global__ __launch_bounds__(POOL_BLOCK) void pool_merge_kernel(PoolArgs A) {
    const int lane = lpf_lane();
    const int64_t i = (int64_t)blockIdx.x * POOL_WAVES + (threadIdx.x >> 6);
    if (i >= A.U) return;
    const int64_t u = A.nodes[i];
    if ((uint64_t)u >= (uint64_t)A.n) return;
    const int64_t a0 = A.a_ptr[i], a1 = A.a_ptr[i + 1], x0 = A.x_ptr[i], x1 = A.x_ptr[i + 1];
    const int64_t b0 = A.b_rowptr[u], b1 = A.b_rowptr[u + 1];
    const int64_t p0 = a0 + x0;
    for (int64_t j = a0 + lane; j < a1; j += LPF_WAVE) {
        const int32_t c = A.a_col[j];
        const int64_t pos = p0 + (j - a0) + (lpf_lower_bound(A.x_col, x0, x1, c) - x0);
        if (pos >= A.T) continue;
        A.pairs[pos] = u;
        A.pairs[A.T + pos] = c;
        if (A.o_cn) A.o_cn[pos] = (float)A.a_cn[j];
        if (A.o_aa) A.o_aa[pos] = A.a_aa[j];
        if (A.o_ra) A.o_ra[pos] = A.a_ra[j];
        if (A.o_ppr) {
            const int64_t b = lpf_lower_bound(A.b_col, b0, b1, c);
            A.o_ppr[pos] = (b < b1 && A.b_col[b] == c) ? A.b_val[b] : 0.f;
        }
    }
    for (int64_t j = x0 + lane; j < x1; j += LPF_WAVE) {
        const int32_t c = A.x_col[j];
        const int64_t pos = p0 + (j - x0) + (lpf_lower_bound(A.a_col, a0, a1, c) - a0);
        if (pos >= A.T) continue;
        A.pairs[pos] = u;
        A.pairs[A.T + pos] = c;
        if (A.o_cn) A.o_cn[pos] = 0.f;
        if (A.o_aa) A.o_aa[pos] = 0.f;
        if (A.o_ra) A.o_ra[pos] = 0.f;
        if (A.o_ppr) A.o_ppr[pos] = A.x_val[j];
    }
}

// ---------------------------------------------------------------------------------------------------- interleave
struct ILArgs {
    int64_t U, n;
    const int64_t *nodes;
    int32_t H, kh;
    const int64_t *ids;                         // [H][U][kh]
    const float *vals;                          // [H][U][kh]
    const int64_t *counts;                      // [H][U]
    const int64_t *exc_rowptr;
    const int32_t *exc_col;
    uint64_t seed;
    int64_t *lists;                             // [U][kh]
    int32_t *n_ranked;                          // [U]
};

static_assert(IL_TABLE == 2048, "lpf_hash11 yields 11 bits");

// Whether this lane's sequence element (id, index t; `ex`: it exists) is the first holder of its id.  Workgroup-uniform
// call (one wavefront per workgroup).
__device__ __forceinline__ bool il_claim(int32_t *keys, int32_t *tmin, int32_t id, int32_t t, bool ex) {
    uint32_t slot = 0;
    if (ex) {
        slot = lpf_hash11(id);
        for (;;) {
            const int32_t prev = atomicCAS(&keys[slot], -1, id);
            if (prev == -1 || prev == id) break;
            slot = (slot + 1) & (IL_TABLE - 1);
        }
        atomicMin(&tmin[slot], t);
    }
    __syncthreads();
    const bool first = ex && tmin[slot] == t;
    __syncthreads();                            // the next round's atomicMin comes after these reads
    return first;
}

__global__ __launch_bounds__(LPF_WAVE) void rank_interleave_kernel(ILArgs A) {
    __shared__ int32_t keys[IL_TABLE];
    __shared__ int32_t tmin[IL_TABLE];
    __shared__ int32_t ranked[IL_MAX_H];
    const int lane = threadIdx.x;
    const int64_t i = blockIdx.x;
    const int64_t u = A.nodes[i];
    const int32_t kh = A.kh, H = A.H;
    int64_t *out = A.lists + i * kh;
    if ((uint64_t)u >= (uint64_t)A.n) {
        for (int e = lane; e < kh; e += LPF_WAVE) out[e] = -1;
        if (lane == 0) A.n_ranked[i] = 0;
        return;
    }
    for (int e = lane; e < IL_TABLE; e += LPF_WAVE) {
        keys[e] = -1;
        tmin[e] = INT32_MAX;
    }
    // each list is cut at its first value that is not > 0 (it is sorted: the positive values form a prefix)
    int32_t maxr = 0;
    for (int h = 0; h < H; ++h) {
        const int64_t row = ((int64_t)h * A.U + i) * kh;
        int64_t cnt = A.counts[(int64_t)h * A.U + i];
        cnt = cnt < 0 ? 0 : (cnt > kh ? kh : cnt);
        int32_t r = 0;
        for (int64_t e0 = 0; e0 < cnt; e0 += LPF_WAVE) {
            const int64_t e = e0 + lane;
            r += __popcll(__ballot(e < cnt && A.vals[row + e] > 0.f));
        }
        if (lane == 0) ranked[h] = r;
        maxr = r > maxr ? r : maxr;
    }
    __syncthreads();
    const int64_t e0x = A.exc_rowptr[u], e1x = A.exc_rowptr[u + 1];
    int32_t kept = 0;
    const int32_t t_end = maxr * H;
    for (int32_t t0 = 0; t0 < t_end && kept < kh; t0 += LPF_WAVE) {   // wave-uniform
        const int32_t t = t0 + lane;
        const int32_t r = t / H, h = t - r * H;
        bool ex = t < t_end && r < ranked[h];
        int32_t id = -1;
        if (ex) {
            const int64_t v = A.ids[((int64_t)h * A.U + i) * kh + r];
            ex = (uint64_t)v < (uint64_t)A.n;
            id = (int32_t)v;
        }
        const bool first = il_claim(keys, tmin, id, t, ex);
        const uint64_t bm = __ballot(first);
        const int32_t pos = kept + __popcll(bm & ((1ull << lane) - 1ull));
        if (first && pos < kh) out[pos] = id;
        kept += __popcll(bm);
    }
    kept = kept < kh ? kept : kh;
    if (lane == 0) A.n_ranked[i] = kept;
    // padding: the draws of lpf_pad_draw in order, skipping u, N(u) and ids already in the list
    const int32_t t_pad = H * kh;                 // (beyond every ranked sequence index)
    for (int32_t d0 = 0; kept < kh && d0 < IL_MAX_DRAWS; d0 += LPF_WAVE) {
        const int32_t d = d0 + lane;
        const int32_t c = (int32_t)lpf_pad_draw(A.seed, u, (uint32_t)d, (uint32_t)A.n);
        const bool ex = c != u && !lpf_sorted_has(A.exc_col, e0x, e1x, c);
        const bool first = il_claim(keys, tmin, c, t_pad + d, ex);
        const uint64_t bm = __ballot(first);
        const int32_t pos = kept + __popcll(bm & ((1ull << lane) - 1ull));
        if (first && pos < kh) out[pos] = c;
        kept += __popcll(bm);
    }
    kept = kept < kh ? kept : kh;
    for (int e = kept + lane; e < kh; e += LPF_WAVE) out[e] = -1;   // (only when the draws ran out)
}

int th_launch(THArgs &A, int64_t n_groups, void *workspace, hipStream_t s) {
    char *w = static_cast<char *>(workspace);
    A.ws_aa = reinterpret_cast<double *>(w);
    A.ws_ra = A.ws_aa + n_groups * A.n;
    A.ws_stamp = reinterpret_cast<int32_t *>(A.ws_ra + n_groups * A.n);
    A.ws_cn = A.ws_stamp + n_groups * A.n;
    if (hipMemsetAsync(A.long_list, 0, sizeof(int32_t), s) != hipSuccess ||
        hipMemsetAsync(A.ws_stamp, 0, (size_t)(n_groups * A.n) * sizeof(int32_t), s) != hipSuccess) {
        lpf_set_hip_error(hipGetLastError());
        return LPF_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(twohop_wave_kernel, dim3((unsigned)A.S), dim3(LPF_WAVE), 0, s, A);
    LPF_CHECK_LAUNCH();
    const int64_t grid = A.S < n_groups ? A.S : n_groups;
    hipLaunchKernelGGL(twohop_group_kernel, dim3((unsigned)grid), dim3(TH_BLOCK), 0, s, A);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}

}  // namespace

extern "C" int64_t lpf_twohop_workspace_bytes(int64_t n, int64_t n_groups) {
    if (n <= 0 || n_groups <= 0) return 0;
    return n_groups * n * 24;                   // fp64 aa, fp64 ra, int32 stamp, int32 cn per node and group
}

extern "C" int lpf_twohop_count(int64_t S, int64_t n, const int64_t *sources, const int64_t *rowptr,
                                const int32_t *col, int32_t split_threshold, int32_t flags, int32_t *scratch,
                                void *workspace, int64_t n_groups, int64_t *count, void *stream) {
    if (S == 0) return LPF_OK;
    LPF_REQUIRE(S > 0 && S < INT32_MAX && n > 0 && n < INT32_MAX && sources && rowptr && scratch && workspace &&
                n_groups > 0 && n_groups <= 65535 && count && lpf_aligned16(workspace));
    THArgs A{};
    A.S = S;
    A.n = n;
    A.src = sources;
    A.rowptr = rowptr;
    A.col = col;
    A.thr = split_threshold < 0 || split_threshold > TH_WAVE_CAP ? TH_WAVE_CAP : split_threshold;
    A.flags = flags;
    A.long_list = scratch;
    A.count = count;
    return th_launch(A, n_groups, workspace, static_cast<hipStream_t>(stream));
}

extern "C" int lpf_twohop_fill(int64_t S, int64_t n, const int64_t *sources, const int64_t *rowptr, const int32_t *col,
                               const float *w_aa, const float *w_ra, int32_t split_threshold, int32_t flags,
                               int32_t *scratch, void *workspace, int64_t n_groups, const int64_t *offset, int64_t T,
                               int32_t *out_col, int32_t *out_cn, float *out_aa, float *out_ra, void *stream) {
    if (S == 0 || T == 0) return LPF_OK;
    LPF_REQUIRE(S > 0 && S < INT32_MAX && n > 0 && n < INT32_MAX && sources && rowptr && scratch && workspace &&
                n_groups > 0 && n_groups <= 65535 && offset && T > 0 && out_col && lpf_aligned16(workspace));
    LPF_REQUIRE((!out_aa || w_aa) && (!out_ra || w_ra));
    THArgs A{};
    A.S = S;
    A.n = n;
    A.src = sources;
    A.rowptr = rowptr;
    A.col = col;
    A.w_aa = out_aa ? w_aa : nullptr;
    A.w_ra = out_ra ? w_ra : nullptr;
    A.thr = split_threshold < 0 || split_threshold > TH_WAVE_CAP ? TH_WAVE_CAP : split_threshold;
    A.flags = flags;
    A.long_list = scratch;
    A.offset = offset;
    A.T = T;
    A.out_col = out_col;
    A.out_cn = out_cn;
    A.out_aa = out_aa;
    A.out_ra = out_ra;
    return th_launch(A, n_groups, workspace, static_cast<hipStream_t>(stream));
}

extern "C" int lpf_pool_extra_count(int64_t U, int64_t n, const int64_t *nodes, const int64_t *a_ptr,
                                    const int32_t *a_col, const int64_t *b_rowptr, const int32_t *b_col,
                                    const int64_t *exc_rowptr, const int32_t *exc_col, int64_t *count, void *stream) {
    if (U == 0) return LPF_OK;
    LPF_REQUIRE(U > 0 && U < INT32_MAX && n > 0 && n < INT32_MAX && nodes && a_ptr && b_rowptr && exc_rowptr && count);
    PoolArgs A{};
    A.U = U;
    A.n = n;
    A.nodes = nodes;
    A.a_ptr = a_ptr;
    A.a_col = a_col;
    A.b_rowptr = b_rowptr;
    A.b_col = b_col;
    A.exc_rowptr = exc_rowptr;
    A.exc_col = exc_col;
    A.count = count;
    hipLaunchKernelGGL(pool_extra_kernel<0>, dim3((unsigned)((U + POOL_WAVES - 1) / POOL_WAVES)), dim3(POOL_BLOCK), 0,
                       static_cast<hipStream_t>(stream), A);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}

extern "C" int lpf_pool_fill(int64_t U, int64_t n, const int64_t *nodes, const int64_t *a_ptr, const int32_t *a_col,
                             const int32_t *a_cn, const float *a_aa, const float *a_ra, const int64_t *b_rowptr,
                             const int32_t *b_col, const float *b_val, const int64_t *exc_rowptr,
                             const int32_t *exc_col, const int64_t *x_ptr, int32_t *x_col, float *x_val, int64_t X,
                             int64_t T, int64_t *pairs, float *out_cn, float *out_aa, float *out_ra, float *out_ppr,
                             void *stream) {
    if (U == 0 || T == 0) return LPF_OK;
    LPF_REQUIRE(U > 0 && U < INT32_MAX && n > 0 && n < INT32_MAX && nodes && a_ptr && b_rowptr && exc_rowptr && x_ptr &&
                X >= 0 && T > 0 && pairs && (X == 0 || (x_col && x_val && b_col && b_val)));
    LPF_REQUIRE((!out_cn || a_cn || T == X) && (!out_aa || a_aa || T == X) && (!out_ra || a_ra || T == X));
    PoolArgs A{};
    A.U = U;
    A.n = n;
    A.nodes = nodes;
    A.a_ptr = a_ptr;
    A.a_col = a_col;
    A.a_cn = a_cn;
    A.a_aa = a_aa;
    A.a_ra = a_ra;
    A.b_rowptr = b_rowptr;
    A.b_col = b_col;
    A.b_val = b_val;
    A.exc_rowptr = exc_rowptr;
    A.exc_col = exc_col;
    A.x_ptr = x_ptr;
    A.x_col = x_col;
    A.x_val = x_val;
    A.X = X;
    A.T = T;
    A.pairs = pairs;
    A.o_cn = out_cn;
    A.o_aa = out_aa;
    A.o_ra = out_ra;
    A.o_ppr = out_ppr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((U + POOL_WAVES - 1) / POOL_WAVES));
    if (X > 0) {
        hipLaunchKernelGGL(pool_extra_kernel<1>, grid, dim3(POOL_BLOCK), 0, s, A);
        LPF_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(pool_merge_kernel, grid, dim3(POOL_BLOCK), 0, s, A);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}

extern "C" int lpf_rank_interleave(int64_t U, int64_t n, const int64_t *nodes, int32_t H, int32_t kh,
                                   const int64_t *ids, const float *vals, const int64_t *counts,
                                   const int64_t *exc_rowptr, const int32_t *exc_col, uint64_t seed, int64_t *lists,
                                   int32_t *n_ranked, void *stream) {
    if (U == 0) return LPF_OK;
    LPF_REQUIRE(U > 0 && U < INT32_MAX && n > 0 && n < INT32_MAX && nodes && H >= 1 && H <= IL_MAX_H && kh >= 1 &&
                kh <= LPF_INTERLEAVE_MAX_KH && ids && vals && counts && exc_rowptr && lists && n_ranked);
    ILArgs A{};
    A.U = U;
    A.n = n;
    A.nodes = nodes;
    A.H = H;
    A.kh = kh;
    A.ids = ids;
    A.vals = vals;
    A.counts = counts;
    A.exc_rowptr = exc_rowptr;
    A.exc_col = exc_col;
    A.seed = seed;
    A.lists = lists;
    A.n_ranked = n_ranked;
    hipLaunchKernelGGL(rank_interleave_kernel, dim3((unsigned)U), dim3(LPF_WAVE), 0, static_cast<hipStream_t>(stream),
                       A);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}
