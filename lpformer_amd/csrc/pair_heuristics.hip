// Pair heuristics on the typing adjacency (the binned-metric analysis of src/train/eval.py:21-77, which counts common
// neighbours with dense adj[edge[0]].to_dense() rows per batch, and the CN / Adamic-Adar / Resource-Allocation baselines
// of HeaRT-style comparisons): for each pair (a, b) of a binary CSR with sorted, unique int32 columns
//   cn[p] = |N(a) & N(b)|,   aa[p] = sum_{w in N(a) & N(b)} w_aa[w],   ra[p] = sum_{w in N(a) & N(b)} w_ra[w]
// (w_aa = 1 / ln deg, 0 where deg <= 1; w_ra = 1 / deg: per-node fp32 tables the caller builds once per graph).
//
// Work: the pair walks its SHORTER row (on equal lengths the row of min(a, b)) and binary-searches each walked column
// in the other row: min(deg) * log2(max deg) probes.  Two classes of work, split by the walked length L:
//   * L <= split_threshold (short): one wavefront takes 64 consecutive pairs and flattens their walked rows into one
//     stream of slots, 64 slots per round, one probe per lane -- a wave of leaf pairs needs a round or two, not one
//     round per pair.  A pair's hits are counted from the round's ballot; the weights of its hits are added by its
//     owner lane, in walked-row order, in fp64.
//   * L > split_threshold (long: hub x hub pairs of a ppa-like graph walk thousands of entries): the short kernel
//     appends the pair to a list (an int32 ticket), and a second kernel gives each listed pair a whole 256-thread
//     workgroup: thread t probes entries t, t + 256, ... (its search window narrows as its keys grow), fp64 partials
//     summed over the workgroup by a fixed tree (butterfly inside each wave, then the four waves in order).
// Deterministic and symmetric: which row is walked, which class a pair falls in and the order of its additions depend on
// the pair (and the threshold) alone -- not on its position in the batch, not on (a, b) versus (b, a), not on timing;
// no float atomics anywhere.  So h(a, b) and h(b, a) are bitwise equal, and so are two runs.  The fp64 sums are rounded
// to fp32 once.  cn is exact in both classes; aa / ra of one pair may differ in the last bit between the two classes.
#include "lpf_common.h"

namespace {

constexpr int HEUR_BLOCK = 256;                 // 4 wavefronts
constexpr int HEUR_WAVES = HEUR_BLOCK / LPF_WAVE;
constexpr int HEUR_LONG_GRID = 2048;            // persistent workgroups of the long-pair kernel

__device__ __forceinline__ void write_out(int64_t p, int32_t c, double sa, double sr, int32_t *__restrict__ cn,
                                          float *__restrict__ aa, float *__restrict__ ra) {
    if (cn) cn[p] = c;
    if (aa) aa[p] = (float)sa;
    if (ra) ra[p] = (float)sr;
}

__global__ __launch_bounds__(HEUR_BLOCK) void heur_short_kernel(
    int64_t P, int64_t n, const int64_t *__restrict__ pairs, int64_t ld, const int64_t *__restrict__ rowptr,
    const int32_t *__restrict__ col, const float *__restrict__ w_aa, const float *__restrict__ w_ra, int32_t thr,
    int32_t *__restrict__ long_list, int32_t *__restrict__ cn, float *__restrict__ aa, float *__restrict__ ra) {
    const int lane = lpf_lane();
    const int64_t wave0 = ((int64_t)blockIdx.x * HEUR_WAVES + (threadIdx.x >> 6)) * LPF_WAVE;
    if (wave0 >= P) return;                        // wave-uniform
    const int64_t p = wave0 + lane;
    const bool live = p < P;
    LpfPairRows r{0, 0, 0, 0};
    if (live) r = lpf_pair_rows(pairs[p], pairs[ld + p], n, rowptr);
    const bool is_long = live && r.len > thr;

    lpf_wave_list_push(long_list, is_long, (int32_t)p);

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
    const bool want_w = aa || ra;

    int32_t c = 0;
    double sa = 0.0, sr = 0.0;
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
        bool hit = false;
        float ta = 0.f, tr = 0.f;
        if (f < total) {
            const int32_t key = col[r0 + j];
            hit = lpf_sorted_has(col, q0, q0 + qlen, key);
            if (hit && (uint64_t)key < (uint64_t)n) {   // (a column outside [0, n) would index past the tables)
                if (aa) ta = w_aa[key];
                if (ra) tr = w_ra[key];
            }
        }
        // this lane's own slots of the round: [s_lo, s_hi) (lane indices)
        const int32_t s_lo = max(excl, base) - base, s_hi = min(incl, base + LPF_WAVE) - base;
        const int32_t mine = s_hi > s_lo ? s_hi - s_lo : 0;
        const uint64_t hm = __ballot(hit);
        uint64_t own = 0;                         // this lane's hits among them
        if (mine > 0) own = hm & ((mine == 64 ? ~0ull : ((1ull << mine) - 1ull)) << s_lo);
        c += __popcll(own);
        if (want_w) {
            // the owner adds the weights of its hits in walked-row order (a miss adds +0.0: skipping it changes no
            // bit); trip count = the most hits any lane owns in this round, usually 0 - 3
            while (__ballot(own != 0)) {
                const int src = own ? __builtin_ctzll(own) : 0;
                const float va = __shfl(ta, src), vr = __shfl(tr, src);
                if (own) {
                    sa += (double)va;
                    sr += (double)vr;
                    own &= own - 1ull;
                }
            }
        }
    }
    if (live && !is_long) write_out(p, c, sa, sr, cn, aa, ra);
}

__global__ __launch_bounds__(HEUR_BLOCK) void heur_long_kernel(
    int64_t n, const int64_t *__restrict__ pairs, int64_t ld, const int64_t *__restrict__ rowptr,
    const int32_t *__restrict__ col, const float *__restrict__ w_aa, const float *__restrict__ w_ra,
    const int32_t *__restrict__ long_list, int32_t *__restrict__ cn, float *__restrict__ aa, float *__restrict__ ra) {
    __shared__ double red_a[HEUR_WAVES], red_r[HEUR_WAVES];
    __shared__ int32_t red_c[HEUR_WAVES];
    const int lane = lpf_lane(), wave = threadIdx.x >> 6;
    const int32_t n_long = long_list[0];
    for (int32_t li = blockIdx.x; li < n_long; li += gridDim.x) {   // block-uniform
        const int64_t p = long_list[1 + li];
        const LpfPairRows r = lpf_pair_rows(pairs[p], pairs[ld + p], n, rowptr);
        const int64_t qend = r.q0 + r.qlen;
        int64_t lo = r.q0;                        // this thread's keys grow: its lower bounds never move back
        int32_t c = 0;
        double sa = 0.0, sr = 0.0;
        for (int32_t j = threadIdx.x; j < r.len; j += HEUR_BLOCK) {
            const int32_t key = col[r.r0 + j];
            lo = lpf_lower_bound(col, lo, qend, key);
            if (lo < qend && col[lo] == key) {
                ++c;
                if ((uint64_t)key < (uint64_t)n) {
                    if (aa) sa += (double)w_aa[key];
                    if (ra) sr += (double)w_ra[key];
                }
            }
        }
#pragma unroll
        for (int m = LPF_WAVE >> 1; m > 0; m >>= 1) {
            c += __shfl_xor(c, m);
            sa += __shfl_xor(sa, m);
            sr += __shfl_xor(sr, m);
        }
        if (lane == 0) {
            red_c[wave] = c;
            red_a[wave] = sa;
            red_r[wave] = sr;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int32_t ct = 0;
            double ta = 0.0, tr = 0.0;
#pragma unroll
            for (int w = 0; w < HEUR_WAVES; ++w) {
                ct += red_c[w];
                ta += red_a[w];
                tr += red_r[w];
            }
            write_out(p, ct, ta, tr, cn, aa, ra);
        }
        __syncthreads();                          // red_* are rewritten by the next pair
    }
}

}  // namespace

extern "C" int lpf_pair_heuristics_f32(int64_t P, int64_t n, const int64_t *pairs, int64_t pairs_ld,
                                       const int64_t *rowptr, const int32_t *col, const float *w_aa, const float *w_ra,
                                       int32_t split_threshold, int32_t *scratch, int32_t *cn, float *aa, float *ra,
                                       void *stream) {
    if (P == 0) return LPF_OK;
    LPF_REQUIRE(P > 0 && P < INT32_MAX && n > 0 && n <= INT32_MAX && pairs && pairs_ld >= P && rowptr && col &&
                scratch);
    LPF_REQUIRE((!aa || w_aa) && (!ra || w_ra));
    if (!cn && !aa && !ra) return LPF_OK;
    const int32_t thr = split_threshold < 0 ? LPF_HEUR_SPLIT_DEFAULT : split_threshold;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (lpf_reset_counter(scratch, s) != LPF_OK) return LPF_ERR_LAUNCH;   // long-pair counter
    const int64_t pairs_per_block = (int64_t)HEUR_BLOCK;   // one pair per lane
    hipLaunchKernelGGL(heur_short_kernel, dim3((unsigned)((P + pairs_per_block - 1) / pairs_per_block)),
                       dim3(HEUR_BLOCK), 0, s, P, n, pairs, pairs_ld, rowptr, col, w_aa, w_ra, thr, scratch, cn, aa,
                       ra);
    LPF_CHECK_LAUNCH();
    const int64_t grid = P < HEUR_LONG_GRID ? P : HEUR_LONG_GRID;
    hipLaunchKernelGGL(heur_long_kernel, dim3((unsigned)grid), dim3(HEUR_BLOCK), 0, s, n, pairs, pairs_ld, rowptr, col,
                       w_aa, w_ra, scratch, cn, aa, ra);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}
