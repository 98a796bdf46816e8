// Common-neighbour pooling: lpf_cn_pool_f32 and lpf_cn_entries.  The contract is restated in
// include/lpformer_hip.h and in lpformer_amd/ncn.py, whose cn_pool_reference is the fp64 restatement the kernels are
// tested against.
//
//   pool[p] = sum_j ( sum_{i in chunk j} w[u_i] T[u_i] ),   C(p) = N(a) & N(b) = u_1 < ... < u_k,
// chunk j = the entries [j LPF_CN_POOL_CHUNK, (j + 1) LPF_CN_POOL_CHUNK) of C(p): a chunk is summed from zero in
// ascending order with one fused multiply-add per element and entry, the chunks' rows are added in chunk order to a
// total that starts at zero.  The intersection is pair_heuristics.hip's: the pair walks its SHORTER row (on equal
// lengths the row of min(a, b)) and binary-searches each walked column in the other row; walked order IS ascending id,
// whichever row is walked, so (a, b) and (b, a) give the same entries in the same order.  Two classes of work, split
// by the walked length L against split_threshold:
//   * short: one wavefront takes 64 consecutive pairs and flattens their walked rows into one stream of slots, 64 per
//     round, one probe per lane.  The round's hits are pair-major and in walked order by lane index; the wavefront then
//     walks them with all 64 lanes across the table row (16-byte loads, dim / 4 lanes busy, four rows requested before
//     the first is used), a chunk accumulator and a total in registers, and writes a pair's row when the hits move on
//     to the next pair.
//   * long: the short kernel lists the pair (an int32 ticket) and a second kernel gives each listed pair a 256-thread
//     workgroup: 256 probes per round, the hits compacted in order into LDS behind what the round before left over,
//     every WHOLE chunk of 64 summed by a wavefront of its own into an LDS row, the rows added in chunk order to the
//     total (thread t owns the elements t and t + 256), the remainder moved to the front.  No pair needs more LDS than
//     319 entries and four rows, however many chunks it has.
// Both classes perform the same fp32 operations per element in the same order -- that is what the chunk rule is for --
// so a pair's row does not depend on its class, on its position in the batch, on (a, b) versus (b, a), on the launch
// shape or on timing.  No float atomics; the only atomic is the long list's int32 ticket.  Every id read from memory is
// range-checked before it indexes anything: a pair with an id outside [0, n) has no entries; a common column outside
// [0, n) (a malformed graph) counts in cn, is written by lpf_cn_entries as it stands and takes its place in its chunk,
// but adds nothing to the pool.
#include "lpf_common.h"

namespace {

constexpr int CN_BLOCK = 256;
constexpr int CN_WAVES = CN_BLOCK / LPF_WAVE;
constexpr int CN_LONG_GRID = 2048;              // persistent workgroups of the long-pair kernels
constexpr int CN_CHUNK = LPF_CN_POOL_CHUNK;
constexpr int CN_LIST = CN_CHUNK - 1 + CN_BLOCK;    // LDS entries of a long pair: a remainder + one round's hits
static_assert(CN_CHUNK == LPF_WAVE, "a wavefront holds one chunk's entries, one per lane");
static_assert(LPF_CN_POOL_MAX_DIM == 2 * CN_BLOCK, "a thread of the long kernel owns the elements t and t + 256");

__device__ __forceinline__ uint64_t cn_uniform(uint64_t m) {   // a wave-uniform mask, in scalar registers
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)m), hi = __builtin_amdgcn_readfirstlane((uint32_t)(m >> 32));
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t cn_lanes_below(int l) { return l >= 64 ? ~0ull : ((1ull << l) - 1ull); }

struct CnTable {
    const float *table;
    int64_t ldt;
    int32_t dim4;
};

// The running sums of one pair: lane l owns the elements 4 (l + 64 i) .. + 3.
template <int NV>
struct CnAcc {
    float4 acc[NV], tot[NV];
    int32_t k;                                    // entries taken so far

    __device__ __forceinline__ void reset() {
#pragma unroll
        for (int i = 0; i < NV; ++i) acc[i] = tot[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        k = 0;
    }
    __device__ __forceinline__ void close_chunk() {           // total += the chunk's row; the next chunk starts at zero
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            tot[i].x += acc[i].x;
            tot[i].y += acc[i].y;
            tot[i].z += acc[i].z;
            tot[i].w += acc[i].w;
            acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
};

// Adds the entries held by the lanes of `mask` (wave-uniform), by ascending lane: lane s holds the node my_key (-1:
// adds nothing, but takes its place) and its weight my_w.  Four rows are requested before the first is used.
template <int NV>
__device__ __forceinline__ void cn_add_hits(CnAcc<NV> &A, uint64_t mask, int32_t my_key, float my_w, const CnTable &T) {
    const int lane = lpf_lane();
    while (mask) {
        int32_t key[4];
        float wt[4];
        bool have[4];
        float4 v[4][NV];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            have[t] = mask != 0;
            const int src = have[t] ? __builtin_ctzll(mask) : 0;
            mask &= mask - 1ull;                               // (0 stays 0)
            key[t] = have[t] ? __shfl(my_key, src) : -1;
            wt[t] = __shfl(my_w, src);
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int j = lane + LPF_WAVE * i;
                v[t][i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (key[t] >= 0 && j < T.dim4)
                    v[t][i] = reinterpret_cast<const float4 *>(T.table + (int64_t)key[t] * T.ldt)[j];
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (!have[t]) continue;
            if (A.k > 0 && A.k % CN_CHUNK == 0) A.close_chunk();
            ++A.k;
            if (key[t] < 0) continue;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                A.acc[i].x = fmaf(wt[t], v[t][i].x, A.acc[i].x);
                A.acc[i].y = fmaf(wt[t], v[t][i].y, A.acc[i].y);
                A.acc[i].z = fmaf(wt[t], v[t][i].z, A.acc[i].z);
                A.acc[i].w = fmaf(wt[t], v[t][i].w, A.acc[i].w);
            }
        }
    }
}

template <int NV>
__device__ __forceinline__ void cn_store_row(float *__restrict__ dst, const float4 (&row)[NV], int32_t dim4) {
    const int lane = lpf_lane();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int j = lane + LPF_WAVE * i;
        if (j < dim4) reinterpret_cast<float4 *>(dst)[j] = row[i];
    }
}

struct CnArgs {
    int64_t P, n;
    const int64_t *pairs;
    int64_t ld;
    const int64_t *rowptr;
    const int32_t *col;
    const float *w;                               // or NULL: 1.0
    CnTable T;
    int32_t thr;
    int32_t *long_list;
    float *pool;
    int64_t ldp;
    int32_t *cn;                                  // or NULL
    const int64_t *seg;                           // entries only
    int64_t n_ent;
    int32_t *node;
};

// [lo, hi) of pair p's segment of node[], clamped to [0, n_ent] (a seg that disagrees with the graph writes inside
// its own segments only)
__device__ __forceinline__ void cn_segment(const CnArgs &A, int64_t p, int64_t &lo, int64_t &hi) {
    lo = A.seg[p];
    hi = A.seg[p + 1];
    lo = lo < 0 ? 0 : (lo > A.n_ent ? A.n_ent : lo);
    hi = hi < lo ? lo : (hi > A.n_ent ? A.n_ent : hi);
}

// One probe of the slot stream / of a long pair's round: the walked column, whether the probed row holds it, and (for
// the pool) the node as a table index (-1 where the column lies outside [0, n)) with its weight.
struct CnProbe {
    bool hit;
    int32_t raw, key;
    float wt;
};
__device__ __forceinline__ CnProbe cn_probe(const CnArgs &A, bool active, int64_t at, int64_t q0, int32_t qlen,
                                            bool want_w) {
    CnProbe pr{false, -1, -1, 1.f};
    if (active) {
        pr.raw = A.col[at];
        pr.hit = lpf_sorted_has(A.col, q0, q0 + qlen, pr.raw);
        if (pr.hit && (uint64_t)pr.raw < (uint64_t)A.n) {       // (a column outside [0, n) would index past the tables)
            pr.key = pr.raw;
            if (want_w && A.w) pr.wt = A.w[pr.raw];
        }
    }
    return pr;
}

// ENT: write the entries (lpf_cn_entries); else pool them.  NV: float4 per lane of a table row.
template <int NV, bool ENT>
__global__ __launch_bounds__(CN_BLOCK) void cn_short_kernel(CnArgs A) {
    const int lane = lpf_lane();
    const int64_t wave0 = ((int64_t)blockIdx.x * CN_WAVES + (threadIdx.x >> 6)) * LPF_WAVE;
    if (wave0 >= A.P) return;                     // wave-uniform
    const int64_t p = wave0 + lane;
    const bool live = p < A.P;
    LpfPairRows r{0, 0, 0, 0};
    if (live) r = lpf_pair_rows(A.pairs[p], A.pairs[A.ld + p], A.n, A.rowptr);
    const bool is_long = live && r.len > A.thr;

    lpf_wave_list_push(A.long_list, is_long, (int32_t)p);

    // short pairs: flatten the walked rows of the wave's pairs into one slot stream (inclusive scan of the lengths)
    const int32_t len = is_long ? 0 : r.len;
    int32_t incl = len;
#pragma unroll
    for (int d = 1; d < LPF_WAVE; d <<= 1) {
        const int32_t v = __shfl_up(incl, d);
        if (lane >= d) incl += v;
    }
    const int32_t excl = incl - len;
    const int32_t total = __shfl(incl, LPF_WAVE - 1);

    int64_t seg_lo = 0, seg_hi = 0;
    if (ENT && live) cn_segment(A, p, seg_lo, seg_hi);

    int32_t c = 0;                                // this lane's pair: its hits so far
    int cur = -1;                                 // the pair (lane index) whose sums S holds; wave-uniform
    CnAcc<NV> S;
    S.reset();
    for (int32_t base = 0; base < total; base += LPF_WAVE) {   // wave-uniform trip count
        const int32_t f = base + lane;
        // owner of slot f: the number of lanes whose inclusive end is <= f (incl is non-decreasing), bit by bit
        int q = 0;
#pragma unroll
        for (int bit = LPF_WAVE >> 1; bit > 0; bit >>= 1)
            if (__shfl(incl, q + bit - 1) <= f) q += bit;
        q = q < LPF_WAVE ? q : LPF_WAVE - 1;      // (64 only for f >= total: a lane without a slot)
        const int32_t j = f - __shfl(excl, q);
        const int64_t r0 = __shfl(r.r0, q), q0 = __shfl(r.q0, q);
        const int32_t qlen = __shfl(r.qlen, q);
        const CnProbe pr = cn_probe(A, f < total, r0 + j, q0, qlen, !ENT);
        // this lane's own slots of the round: [s_lo, s_hi) (lane indices)
        const int32_t s_lo = max(excl, base) - base, s_hi = min(incl, base + LPF_WAVE) - base;
        const int32_t mine = s_hi > s_lo ? s_hi - s_lo : 0;
        const uint64_t hm = cn_uniform(__ballot(pr.hit));
        uint64_t own = 0;                         // this lane's hits among them
        if (mine > 0) own = hm & (cn_lanes_below(mine) << s_lo);
        if constexpr (ENT) {
            // the hit's place: its owner's segment + the owner's earlier hits + the owner's hits of this round below it
            const int32_t o_lo = __shfl(s_lo, q), o_hi = __shfl(s_hi, q), o_c = __shfl(c, q);
            const int64_t o_seg = __shfl(seg_lo, q), o_end = __shfl(seg_hi, q);
            if (pr.hit) {
                const uint64_t range = cn_lanes_below(o_hi) & ~cn_lanes_below(o_lo);
                const int64_t at = o_seg + o_c + __popcll(hm & range & cn_lanes_below(lane));
                if (at < o_end) A.node[at] = pr.raw;
            }
        } else {
            // the round's hits by ascending lane are pair-major and in walked order: one owner after the other
            uint64_t rest = hm;
            while (rest) {
                const int s = __builtin_ctzll(rest);
                const int oq = __builtin_amdgcn_readfirstlane(__shfl(q, s));
                const int o_lo = __builtin_amdgcn_readfirstlane(__shfl(s_lo, oq));
                const int o_hi = __builtin_amdgcn_readfirstlane(__shfl(s_hi, oq));
                const uint64_t range = cn_lanes_below(o_hi) & ~cn_lanes_below(o_lo);
                const uint64_t sub = rest & range;
                rest &= ~range;
                if (oq != cur) {
                    if (cur >= 0) {
                        S.close_chunk();
                        cn_store_row<NV>(A.pool + (wave0 + cur) * A.ldp, S.tot, A.T.dim4);
                    }
                    cur = oq;
                    S.reset();
                }
                cn_add_hits<NV>(S, sub, pr.key, pr.wt, A.T);
            }
        }
        c += __popcll(own);
    }
    if constexpr (!ENT) {
        if (cur >= 0) {
            S.close_chunk();
            cn_store_row<NV>(A.pool + (wave0 + cur) * A.ldp, S.tot, A.T.dim4);
        }
        // a short pair without a common neighbour: its row is written all the same
        S.reset();
        uint64_t zero = cn_uniform(__ballot(live && !is_long && c == 0));
        while (zero) {
            const int s = __builtin_ctzll(zero);
            zero &= zero - 1ull;
            cn_store_row<NV>(A.pool + (wave0 + s) * A.ldp, S.tot, A.T.dim4);
        }
        if (A.cn && live && !is_long) A.cn[p] = c;
    }
}

// A listed pair's entries, a 256-thread workgroup per pair: the round's hits keep their walked order through the
// ballot ranks and the four wavefronts' counts.
__global__ __launch_bounds__(CN_BLOCK) void cn_long_entries_kernel(CnArgs A) {
    __shared__ int32_t wcnt[CN_WAVES];
    const int lane = lpf_lane(), wave = threadIdx.x >> 6;
    const int32_t n_long = A.long_list[0];
    for (int32_t li = blockIdx.x; li < n_long; li += gridDim.x) {   // block-uniform
        const int64_t p = A.long_list[1 + li];
        const LpfPairRows r = lpf_pair_rows(A.pairs[p], A.pairs[A.ld + p], A.n, A.rowptr);
        int64_t seg_lo, seg_hi;
        cn_segment(A, p, seg_lo, seg_hi);
        int64_t done = 0;                         // hits of the rounds before
        for (int32_t base = 0; base < r.len; base += CN_BLOCK) {    // block-uniform
            const int32_t j = base + (int32_t)threadIdx.x;
            const CnProbe pr = cn_probe(A, j < r.len, r.r0 + j, r.q0, r.qlen, false);
            const uint64_t hm = __ballot(pr.hit);
            if (lane == 0) wcnt[wave] = __popcll(hm);
            __syncthreads();
            int32_t before = 0, round = 0;
#pragma unroll
            for (int w = 0; w < CN_WAVES; ++w) {
                const int32_t v = wcnt[w];
                if (w < wave) before += v;
                round += v;
            }
            if (pr.hit) {
                const int64_t at = seg_lo + done + before + __popcll(hm & cn_lanes_below(lane));
                if (at < seg_hi) A.node[at] = pr.raw;
            }
            done += round;
            __syncthreads();                      // wcnt is rewritten by the next round
        }
    }
}

// A listed pair's pooled row, a 256-thread workgroup per pair (see the head of this file).
template <int NV>
__global__ __launch_bounds__(CN_BLOCK) void cn_long_pool_kernel(CnArgs A) {
    __shared__ int32_t wcnt[CN_WAVES];
    __shared__ int32_t lkey[CN_LIST];
    __shared__ float lwt[CN_LIST];
    __shared__ __attribute__((aligned(16))) float part[CN_WAVES][LPF_CN_POOL_MAX_DIM];
    const int lane = lpf_lane(), wave = threadIdx.x >> 6;
    const int tid = (int)threadIdx.x;
    const int dim = A.T.dim4 * 4;
    const int32_t n_long = A.long_list[0];
    for (int32_t li = blockIdx.x; li < n_long; li += gridDim.x) {   // block-uniform
        const int64_t p = A.long_list[1 + li];
        const LpfPairRows r = lpf_pair_rows(A.pairs[p], A.pairs[A.ld + p], A.n, A.rowptr);
        int32_t pend = 0, k = 0;                  // entries waiting in LDS (< 64 between rounds); hits so far
        float tot0 = 0.f, tot1 = 0.f;             // the elements tid and tid + 256 of the total
        for (int32_t base = 0; base < r.len; base += CN_BLOCK) {    // block-uniform
            const int32_t j = base + tid;
            const CnProbe pr = cn_probe(A, j < r.len, r.r0 + j, r.q0, r.qlen, true);
            const uint64_t hm = __ballot(pr.hit);
            if (lane == 0) wcnt[wave] = __popcll(hm);
            __syncthreads();
            int32_t before = 0, round = 0;
#pragma unroll
            for (int w = 0; w < CN_WAVES; ++w) {
                const int32_t v = wcnt[w];
                if (w < wave) before += v;
                round += v;
            }
            if (pr.hit) {
                const int at = pend + before + __popcll(hm & cn_lanes_below(lane));   // < 63 + 256
                lkey[at] = pr.key;
                lwt[at] = pr.wt;
            }
            pend += round;
            k += round;
            __syncthreads();
            const int nfull = pend / CN_CHUNK;    // <= 4: a wavefront per whole chunk
            if (nfull > 0) {                      // block-uniform
                if (wave < nfull) {
                    CnAcc<NV> S;
                    S.reset();
                    cn_add_hits<NV>(S, ~0ull, lkey[wave * CN_CHUNK + lane], lwt[wave * CN_CHUNK + lane], A.T);
                    cn_store_row<NV>(part[wave], S.acc, A.T.dim4);
                }
                __syncthreads();
                for (int c = 0; c < nfull; ++c) {             // the chunks' rows in chunk order
                    if (tid < dim) tot0 += part[c][tid];
                    if (tid + CN_BLOCK < dim) tot1 += part[c][tid + CN_BLOCK];
                }
                const int rem = pend - nfull * CN_CHUNK;
                int32_t mk = -1;
                float mw = 0.f;
                if (tid < rem) {
                    mk = lkey[nfull * CN_CHUNK + tid];
                    mw = lwt[nfull * CN_CHUNK + tid];
                }
                __syncthreads();
                if (tid < rem) {                  // the remainder moves to the front
                    lkey[tid] = mk;
                    lwt[tid] = mw;
                }
                pend = rem;
            }
        }
        __syncthreads();
        if (pend > 0) {                           // the last, partial chunk
            if (wave == 0) {
                CnAcc<NV> S;
                S.reset();
                const bool mine = lane < pend;
                cn_add_hits<NV>(S, cn_lanes_below(pend), mine ? lkey[lane] : -1, mine ? lwt[lane] : 0.f, A.T);
                cn_store_row<NV>(part[0], S.acc, A.T.dim4);
            }
            __syncthreads();
            if (tid < dim) tot0 += part[0][tid];
            if (tid + CN_BLOCK < dim) tot1 += part[0][tid + CN_BLOCK];
        }
        float *dst = A.pool + p * A.ldp;
        if (tid < dim) dst[tid] = tot0;
        if (tid + CN_BLOCK < dim) dst[tid + CN_BLOCK] = tot1;
        if (A.cn && tid == 0) A.cn[p] = k;
        __syncthreads();                          // the LDS rows and lists are rewritten by the next pair
    }
}

bool cn_dim_ok(int32_t dim) { return dim >= 4 && dim % 4 == 0 && dim <= LPF_CN_POOL_MAX_DIM; }
bool cn_rows_ok(const void *p, int64_t ld, int32_t dim) { return p && lpf_aligned16(p) && ld >= dim && ld % 4 == 0; }
bool cn_graph_ok(int64_t P, int64_t n, const int64_t *pairs, int64_t pairs_ld, const int64_t *rowptr,
                 const int32_t *col, const int32_t *scratch) {
    return P > 0 && P < INT32_MAX && n > 0 && n <= INT32_MAX && pairs && pairs_ld >= P && rowptr && col && scratch;
}

}  // namespace

extern "C" int lpf_cn_pool_f32(int64_t P, int64_t n, const int64_t *pairs, int64_t pairs_ld, const int64_t *rowptr,
                               const int32_t *col, const float *w, int32_t dim, const float *table, int64_t ldt,
                               int32_t split_threshold, int32_t *scratch, float *pool, int64_t ldp, int32_t *cn,
                               void *stream) {
    LPF_REQUIRE(P >= 0);
    if (P == 0) return LPF_OK;
    LPF_REQUIRE(cn_graph_ok(P, n, pairs, pairs_ld, rowptr, col, scratch));
    LPF_REQUIRE(cn_dim_ok(dim) && cn_rows_ok(table, ldt, dim) && cn_rows_ok(pool, ldp, dim));
    CnArgs A{};
    A.P = P;
    A.n = n;
    A.pairs = pairs;
    A.ld = pairs_ld;
    A.rowptr = rowptr;
    A.col = col;
    A.w = w;
    A.T = CnTable{table, ldt, dim / 4};
    A.thr = split_threshold < 0 ? LPF_HEUR_SPLIT_DEFAULT : split_threshold;
    A.long_list = scratch;
    A.pool = pool;
    A.ldp = ldp;
    A.cn = cn;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (lpf_reset_counter(scratch, s) != LPF_OK) return LPF_ERR_LAUNCH;   // long-pair counter
    const dim3 block(CN_BLOCK), grid1((unsigned)((P + CN_BLOCK - 1) / CN_BLOCK));   // one pair per lane
    const dim3 grid2((unsigned)(P < CN_LONG_GRID ? P : CN_LONG_GRID));
    const bool wide = A.T.dim4 > LPF_WAVE;
    if (wide) hipLaunchKernelGGL((cn_short_kernel<2, false>), grid1, block, 0, s, A);
    else hipLaunchKernelGGL((cn_short_kernel<1, false>), grid1, block, 0, s, A);
    LPF_CHECK_LAUNCH();
    if (wide) hipLaunchKernelGGL(cn_long_pool_kernel<2>, grid2, block, 0, s, A);
    else hipLaunchKernelGGL(cn_long_pool_kernel<1>, grid2, block, 0, s, A);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}

extern "C" int lpf_cn_entries(int64_t P, int64_t n, const int64_t *pairs, int64_t pairs_ld, const int64_t *rowptr,
                              const int32_t *col, int32_t split_threshold, int32_t *scratch, const int64_t *seg,
                              int64_t n_ent, int32_t *node, void *stream) {
    LPF_REQUIRE(P >= 0);
    if (P == 0) return LPF_OK;
    LPF_REQUIRE(cn_graph_ok(P, n, pairs, pairs_ld, rowptr, col, scratch));
    LPF_REQUIRE(seg && n_ent >= 0 && n_ent < INT32_MAX && (node || n_ent == 0));
    if (n_ent == 0) return LPF_OK;                // nothing may be written
    CnArgs A{};
    A.P = P;
    A.n = n;
    A.pairs = pairs;
    A.ld = pairs_ld;
    A.rowptr = rowptr;
    A.col = col;
    A.thr = split_threshold < 0 ? LPF_HEUR_SPLIT_DEFAULT : split_threshold;
    A.long_list = scratch;
    A.seg = seg;
    A.n_ent = n_ent;
    A.node = node;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (lpf_reset_counter(scratch, s) != LPF_OK) return LPF_ERR_LAUNCH;   // long-pair counter
    const dim3 block(CN_BLOCK), grid1((unsigned)((P + CN_BLOCK - 1) / CN_BLOCK));
    const dim3 grid2((unsigned)(P < CN_LONG_GRID ? P : CN_LONG_GRID));
    hipLaunchKernelGGL((cn_short_kernel<1, true>), grid1, block, 0, s, A);
    LPF_CHECK_LAUNCH();
    hipLaunchKernelGGL(cn_long_entries_kernel, grid2, block, 0, s, A);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}
