// Top-K link recommendation: the candidate pairs of a batch of sources, and the segmented top-K of their scores.
//
// 1. Candidates (lpf_rec_candidate_count / lpf_rec_candidate_fill).  For source u, C(u) is the include row of u -- the
//    stored entries of u's PPR row whose fp32 value is > 0 and >= min_val, or every id of [0, n) when no include CSR
//    is given -- minus the exclusion row of u (sorted int32 columns) and, with exclude_self, minus u itself; ascending
//    v.  The count pass writes |C(u)|; the caller scans the counts and the fill pass writes (u, v) straight into the
//    [2, P] int64 layout score_edges takes.  Two classes of work, split by the include-row length L:
//    * L <= split_threshold (short): one wavefront per source, four sources per workgroup.  Each lane tests one v per
//      round against the exclusion row by binary search, the row staged in LDS when it holds <= REC_EXC_LDS entries.
//      Output ranks come from the round's ballot and popcount: no atomics on the output.
//    * L > split_threshold, and every "all" row (long): the short kernel appends the source to a list (an int32
//      ticket) and a second kernel gives each listed source a 256-thread workgroup.  A PPR row goes 256 entries per
//      round, ranked by ballot plus the four wave totals.  An "all" row is never searched entry by entry: output
//      position r maps to v = r' + i, with i the first exclusion index whose c_i - i > r' (r' = r, or r + 1 past u's
//      own slot when u is dropped and not excluded already), so the workgroup walks the gaps between excluded ids.
//    Both passes classify a source the same way, so the fill pass writes exactly the counted entries.
//
// 2. Segmented top-K (lpf_segment_topk_f32).  Segment s = [seg_ptr[s], seg_ptr[s + 1]) of score / cand.  The key of
//    position p of a segment is (ordered uint32 of the score) << 32 | ~p, where the ordered uint32 maps -0.0 to +0.0
//    and every NaN below -inf.  Keys are unique inside a segment; the top min(k, len) keys in descending order are the
//    result, so ties go to the earlier position and the output is a pure function of the input (no float atomics).
//    * len <= REC_WAVE_SORT (256): one wavefront per segment, 4 keys per lane, a bitonic network in registers
//      (cross-lane steps by __shfl_xor).
//    * longer segments are ticketed to a persistent kernel, one 512-thread workgroup per segment.  len <= REC_SORT_CAP
//      (4096 keys, 32 KiB of LDS): load the keys into LDS and bitonic-sort them.  Longer: an MSB-first radix select
//      on the 64-bit key, 8 bits per pass with a 256-bin LDS histogram, narrowed until the keys at or above the
//      current bucket number <= REC_SORT_CAP (at the latest after 8 passes, when the bucket is the exact k-th key and
//      at most k - 1 <= 1023 keys lie above it).  Those keys are compacted into LDS and sorted as above.
//    LDS per workgroup: 32 KiB of keys + 1 KiB of histogram, so four workgroups fit in the 160 KiB of a CU.
#include "lpf_common.h"

namespace {

constexpr int REC_BLOCK = 256;                  // candidate kernels: 4 wavefronts
constexpr int REC_WAVES = REC_BLOCK / LPF_WAVE;
constexpr int REC_EXC_LDS = 1024;               // exclusion entries staged per wavefront (4 KiB; 16 KiB per workgroup)
constexpr int REC_LONG_GRID = 2048;             // persistent workgroups of the long-row kernel
constexpr int REC_WAVE_SORT = 256;              // segments up to this length: one wavefront, 4 keys per lane
constexpr int REC_WAVE_KEYS = REC_WAVE_SORT / LPF_WAVE;
constexpr int REC_SORT_CAP = 4096;              // keys a top-K workgroup sorts in LDS
constexpr int REC_TOPK_BLOCK = 512;
constexpr int REC_TOPK_GRID = 1024;

struct CandArgs {
    int64_t S, n;
    const int64_t *src;
    const int64_t *inc_rowptr;                  // NULL: every id of [0, n)
    const int32_t *inc_col;
    const float *inc_val;
    float min_val;
    const int64_t *exc_rowptr;                  // NULL: no exclusion row
    const int32_t *exc_col;
    int32_t exclude_self, thr;
    int32_t *long_list;
    int64_t *count;                             // count pass: |C(u)|
    const int64_t *offset;                      // fill pass: first output slot of each source (NULL in the count pass)
    int64_t P;
    int64_t *pairs;                             // fill pass: [2, P]
};

__device__ __forceinline__ void exc_row(const CandArgs &A, int64_t u, int64_t &e0, int64_t &e1) {
    e0 = e1 = 0;
    if (A.exc_rowptr) {
        e0 = A.exc_rowptr[u];
        e1 = A.exc_rowptr[u + 1];
    }
}

// the include-row test of entry j (absolute index) of u's PPR row, exclusion aside
__device__ __forceinline__ bool inc_keep(const CandArgs &A, int64_t u, int64_t j, int32_t &v) {
    v = A.inc_col[j];
    const float val = A.inc_val[j];
    return val > 0.f && val >= A.min_val && (uint64_t)v < (uint64_t)A.n && !(A.exclude_self && v == u);
}

__global__ __launch_bounds__(REC_BLOCK) void rec_short_kernel(CandArgs A) {
    __shared__ int32_t exc_lds[REC_WAVES][REC_EXC_LDS];
    const int lane = lpf_lane(), wave = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * REC_WAVES + wave;
    const int64_t u = w < A.S ? A.src[w] : -1;
    const bool valid = w < A.S && (uint64_t)u < (uint64_t)A.n;
    int64_t r0 = 0, len = 0, e0 = 0, e1 = 0;
    bool is_long = false;
    if (valid) {
        if (A.inc_rowptr) {
            r0 = A.inc_rowptr[u];
            len = A.inc_rowptr[u + 1] - r0;
        }
        is_long = !A.inc_rowptr || len > A.thr;
        exc_row(A, u, e0, e1);
    }
    if (is_long && lane == 0) A.long_list[1 + atomicAdd(&A.long_list[0], 1)] = (int32_t)w;
    const bool run = valid && !is_long;         // wave-uniform
    const bool staged = run && e1 - e0 <= REC_EXC_LDS;
    if (staged)
        for (int64_t i = lane; i < e1 - e0; i += LPF_WAVE) exc_lds[wave][i] = A.exc_col[e0 + i];
    __syncthreads();
    if (w < A.S && !valid && !A.offset && lane == 0) A.count[w] = 0;   // (ids outside [0, n): nothing)
    if (!run) return;

    const int32_t *ex = staged ? exc_lds[wave] : A.exc_col;
    const int64_t x0 = staged ? 0 : e0, x1 = staged ? e1 - e0 : e1;
    const int64_t out0 = A.offset ? A.offset[w] : 0;
    int64_t base = 0;
    for (int64_t j0 = 0; j0 < len; j0 += LPF_WAVE) {   // wave-uniform trip count
        const int64_t j = j0 + lane;
        int32_t v = 0;
        bool keep = false;
        if (j < len) {
            keep = inc_keep(A, u, r0 + j, v);
            if (keep && x1 > x0) keep = !lpf_sorted_has(ex, x0, x1, v);
        }
        const uint64_t m = __ballot(keep);
        if (A.offset && keep) {
            const int64_t pos = out0 + base + __popcll(m & ((1ull << lane) - 1ull));
            if (pos < A.P) {                    // (always: the fill pass writes the slots the count pass counted)
                A.pairs[pos] = u;
                A.pairs[A.P + pos] = v;
            }
        }
        base += __popcll(m);
    }
    if (!A.offset && lane == 0) A.count[w] = base;
}

__global__ __launch_bounds__(REC_BLOCK) void rec_long_kernel(CandArgs A) {
    __shared__ int32_t wave_cnt[REC_WAVES];
    const int lane = lpf_lane(), wave = threadIdx.x >> 6;
    const int32_t n_long = A.long_list[0];
    for (int32_t li = blockIdx.x; li < n_long; li += gridDim.x) {   // block-uniform
        const int64_t w = A.long_list[1 + li];
        const int64_t u = A.src[w];
        int64_t e0, e1;
        exc_row(A, u, e0, e1);
        const int64_t out0 = A.offset ? A.offset[w] : 0;
        if (A.inc_rowptr) {
            const int64_t r0 = A.inc_rowptr[u], len = A.inc_rowptr[u + 1] - r0;
            int64_t lo = e0;                    // this thread's v grow: its lower bound never moves back
            int64_t base = 0;
            for (int64_t j0 = 0; j0 < len; j0 += REC_BLOCK) {
                const int64_t j = j0 + threadIdx.x;
                int32_t v = 0;
                bool keep = false;
                if (j < len) {
                    keep = inc_keep(A, u, r0 + j, v);
                    if (keep && e1 > e0) {
                        lo = lpf_lower_bound(A.exc_col, lo, e1, v);
                        keep = !(lo < e1 && A.exc_col[lo] == v);
                    }
                }
                const uint64_t m = __ballot(keep);
                if (lane == 0) wave_cnt[wave] = __popcll(m);
                __syncthreads();
                int64_t before = 0, total = 0;
#pragma unroll
                for (int q = 0; q < REC_WAVES; ++q) {
                    before += q < wave ? wave_cnt[q] : 0;
                    total += wave_cnt[q];
                }
                if (A.offset && keep) {
                    const int64_t pos = out0 + base + before + __popcll(m & ((1ull << lane) - 1ull));
                    if (pos < A.P) {
                        A.pairs[pos] = u;
                        A.pairs[A.P + pos] = v;
                    }
                }
                base += total;
                __syncthreads();                // wave_cnt is rewritten by the next round
            }
            if (!A.offset && threadIdx.x == 0) A.count[w] = base;
        } else {
            // "all": the non-excluded ids in ascending order.  Excluded columns outside [0, n) are ignored.
            const int64_t eb = lpf_lower_bound(A.exc_col, e0, e1, 0);
            const int64_t ee = lpf_lower_bound(A.exc_col, eb, e1, (int32_t)A.n);
            const int64_t m = ee - eb;
            const int64_t iu = lpf_lower_bound(A.exc_col, eb, ee, (int32_t)u);
            const bool drop_u = A.exclude_self && !(iu < ee && A.exc_col[iu] == u);
            const int64_t cnt = A.n - m - (drop_u ? 1 : 0);
            if (!A.offset) {
                if (threadIdx.x == 0) A.count[w] = cnt;
                continue;
            }
            const int64_t pu = u - (iu - eb);   // u's position among the non-excluded ids
            int64_t lo = 0;                     // first exclusion index i with c_i - i > r' (r' grows per thread)
            for (int64_t r = threadIdx.x; r < cnt; r += REC_BLOCK) {
                const int64_t rr = r + (drop_u && r >= pu ? 1 : 0);
                int64_t hi = m;
                while (lo < hi) {
                    const int64_t mid = lo + ((hi - lo) >> 1);
                    if ((int64_t)A.exc_col[eb + mid] - mid > rr) hi = mid; else lo = mid + 1;
                }
                const int64_t pos = out0 + r;
                if (pos >= A.P) break;
                A.pairs[pos] = u;
                A.pairs[A.P + pos] = rr + lo;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- segmented top-K
__device__ __forceinline__ uint64_t topk_key(float f, uint32_t pos) {
    uint32_t u = __float_as_uint(f);
    uint32_t o;
    if ((u & 0x7fffffffu) > 0x7f800000u) {
        o = 0u;                                 // NaN: below -inf (whose key is 0x007fffff)
    } else {
        if (u == 0x80000000u) u = 0u;           // -0.0 == +0.0
        o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return ((uint64_t)o << 32) | (uint64_t)(uint32_t)~pos;
}

__device__ __forceinline__ void topk_write(int64_t s, int32_t k, int64_t seg0, uint64_t key, int64_t e,
                                           const float *__restrict__ score, const int64_t *__restrict__ cand,
                                           int64_t *__restrict__ ids, float *__restrict__ out) {
    const uint32_t pos = ~(uint32_t)key;
    ids[s * k + e] = cand[seg0 + pos];
    out[s * k + e] = score[seg0 + pos];
}

__device__ __forceinline__ void topk_pad(int64_t s, int32_t k, int64_t e, int64_t *__restrict__ ids,
                                         float *__restrict__ out) {
    ids[s * k + e] = -1;
    out[s * k + e] = -__builtin_inff();
}

__global__ __launch_bounds__(REC_BLOCK) void topk_wave_kernel(int64_t S, const int64_t *__restrict__ seg_ptr,
                                                              const float *__restrict__ score,
                                                              const int64_t *__restrict__ cand, int32_t k,
                                                              int32_t *__restrict__ long_list,
                                                              int64_t *__restrict__ ids, float *__restrict__ out,
                                                              int64_t *__restrict__ counts) {
    const int lane = lpf_lane();
    const int64_t s = (int64_t)blockIdx.x * REC_WAVES + (threadIdx.x >> 6);
    if (s >= S) return;                         // wave-uniform
    const int64_t seg0 = seg_ptr[s], len = seg_ptr[s + 1] - seg0;
    if (len > REC_WAVE_SORT) {
        if (lane == 0) long_list[1 + atomicAdd(&long_list[0], 1)] = (int32_t)s;
        return;
    }
    // element e = lane + 64 * i of the network lives in K[i]; padding keys are 0, below every real key
    uint64_t K[REC_WAVE_KEYS];
#pragma unroll
    for (int i = 0; i < REC_WAVE_KEYS; ++i) {
        const int64_t e = lane + LPF_WAVE * i;
        K[i] = e < len ? topk_key(score[seg0 + e], (uint32_t)e) : 0ull;
    }
#pragma unroll
    for (int size = 2; size <= REC_WAVE_SORT; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (stride >= LPF_WAVE) {           // partner in another register of this lane
                const int rs = stride / LPF_WAVE;
#pragma unroll
                for (int i = 0; i < REC_WAVE_KEYS; ++i) {
                    if (i & rs) continue;
                    const int j = i | rs;
                    const bool desc = ((lane + LPF_WAVE * i) & size) == 0;
                    const uint64_t a = K[i], b = K[j];
                    const bool sw = desc ? a < b : a > b;
                    K[i] = sw ? b : a;
                    K[j] = sw ? a : b;
                }
            } else {                            // partner in lane ^ stride, same register
                const bool lower = (lane & stride) == 0;
#pragma unroll
                for (int i = 0; i < REC_WAVE_KEYS; ++i) {
                    const bool desc = ((lane + LPF_WAVE * i) & size) == 0;
                    const uint64_t a = K[i], b = __shfl_xor(K[i], stride);
                    const uint64_t hi = a > b ? a : b, lo = a > b ? b : a;
                    K[i] = lower == desc ? hi : lo;
                }
            }
        }
    }
    const int64_t cnt = len < k ? len : k;
#pragma unroll
    for (int i = 0; i < REC_WAVE_KEYS; ++i) {
        const int64_t e = lane + LPF_WAVE * i;
        if (e < cnt) topk_write(s, k, seg0, K[i], e, score, cand, ids, out);
    }
    for (int64_t e = cnt + lane; e < k; e += LPF_WAVE) topk_pad(s, k, e, ids, out);
    if (lane == 0) counts[s] = cnt;
}

// bitonic sort of keys[0, p) in LDS, descending (p a power of two, entries past the live ones set to 0)
__device__ void lds_sort_desc(uint64_t *keys, int p) {
    for (int size = 2; size <= p; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (p >> 1); t += REC_TOPK_BLOCK) {
                const int e = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
                const bool desc = (e & size) == 0;
                const uint64_t a = keys[e], b = keys[e + stride];
                if (desc ? a < b : a > b) {
                    keys[e] = b;
                    keys[e + stride] = a;
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(REC_TOPK_BLOCK) void topk_block_kernel(const int64_t *__restrict__ seg_ptr,
                                                                    const float *__restrict__ score,
                                                                    const int64_t *__restrict__ cand, int32_t k,
                                                                    const int32_t *__restrict__ long_list,
                                                                    int64_t *__restrict__ ids,
                                                                    float *__restrict__ out,
                                                                    int64_t *__restrict__ counts) {
    __shared__ uint64_t keys[REC_SORT_CAP];
    __shared__ int32_t hist[256];
    __shared__ uint64_t sh_prefix, sh_mask;
    __shared__ int64_t sh_need, sh_above, sh_stop;
    __shared__ int32_t sh_fill;
    const int32_t n_long = long_list[0];
    for (int32_t li = blockIdx.x; li < n_long; li += gridDim.x) {   // block-uniform
        const int64_t s = long_list[1 + li];
        const int64_t seg0 = seg_ptr[s], len = seg_ptr[s + 1] - seg0;
        const int64_t cnt = len < k ? len : k;
        int n_sel;
        if (len <= REC_SORT_CAP) {
            for (int64_t i = threadIdx.x; i < len; i += REC_TOPK_BLOCK)
                keys[i] = topk_key(score[seg0 + i], (uint32_t)i);
            n_sel = (int)len;
        } else {
            if (threadIdx.x == 0) {
                sh_prefix = 0ull;
                sh_mask = 0ull;
                sh_need = cnt;
                sh_above = 0;
                sh_stop = 0;
                sh_fill = 0;
            }
            __syncthreads();
            for (int shift = 56; shift >= 0; shift -= 8) {
                for (int b = threadIdx.x; b < 256; b += REC_TOPK_BLOCK) hist[b] = 0;
                __syncthreads();
                const uint64_t prefix = sh_prefix, mask = sh_mask;
                for (int64_t i = threadIdx.x; i < len; i += REC_TOPK_BLOCK) {
                    const uint64_t key = topk_key(score[seg0 + i], (uint32_t)i);
                    if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
                }
                __syncthreads();
                if (threadIdx.x == 0) {
                    // the bucket holding the need-th largest key of those matching the prefix
                    int64_t acc = 0;
                    int b = 255;
                    for (; b > 0; --b) {
                        if (acc + hist[b] >= sh_need) break;
                        acc += hist[b];
                    }
                    sh_prefix = prefix | ((uint64_t)b << shift);
                    sh_mask = mask | (0xffull << shift);
                    sh_need -= acc;
                    sh_above += acc;
                    sh_stop = sh_above + hist[b] <= REC_SORT_CAP;
                }
                __syncthreads();
                if (sh_stop) break;
            }
            // every key at or above the bucket: the sh_above keys of higher buckets and the bucket itself
            const uint64_t prefix = sh_prefix, mask = sh_mask;
            for (int64_t i = threadIdx.x; i < len; i += REC_TOPK_BLOCK) {
                const uint64_t key = topk_key(score[seg0 + i], (uint32_t)i);
                if ((key & mask) >= prefix) {
                    const int slot = atomicAdd(&sh_fill, 1);
                    if (slot < REC_SORT_CAP) keys[slot] = key;   // (always: the select stops at <= REC_SORT_CAP keys)
                }
            }
            __syncthreads();
            n_sel = sh_fill < REC_SORT_CAP ? sh_fill : REC_SORT_CAP;
        }
        int p = 2;
        while (p < n_sel) p <<= 1;
        for (int i = n_sel + threadIdx.x; i < p; i += REC_TOPK_BLOCK) keys[i] = 0ull;
        __syncthreads();
        lds_sort_desc(keys, p);
        for (int64_t e = threadIdx.x; e < k; e += REC_TOPK_BLOCK) {
            if (e < cnt) topk_write(s, k, seg0, keys[e], e, score, cand, ids, out);
            else topk_pad(s, k, e, ids, out);
        }
        if (threadIdx.x == 0) counts[s] = cnt;
        __syncthreads();                        // keys / sh_* are rewritten by the next segment
    }
}

int rec_candidates(const CandArgs &A, void *stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (lpf_reset_counter(A.long_list, s) != LPF_OK) return LPF_ERR_LAUNCH;   // long-row counter
    hipLaunchKernelGGL(rec_short_kernel, dim3((unsigned)((A.S + REC_WAVES - 1) / REC_WAVES)), dim3(REC_BLOCK), 0, s,
                       A);
    LPF_CHECK_LAUNCH();
    const int64_t grid = A.S < REC_LONG_GRID ? A.S : REC_LONG_GRID;
    hipLaunchKernelGGL(rec_long_kernel, dim3((unsigned)grid), dim3(REC_BLOCK), 0, s, A);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}

CandArgs cand_args(int64_t S, int64_t n, const int64_t *sources, const int64_t *inc_rowptr, const int32_t *inc_col,
                   const float *inc_val, float min_val, const int64_t *exc_rowptr, const int32_t *exc_col,
                   int32_t exclude_self, int32_t split_threshold, int32_t *scratch) {
    CandArgs A;
    A.S = S;
    A.n = n;
    A.src = sources;
    A.inc_rowptr = inc_rowptr;
    A.inc_col = inc_col;
    A.inc_val = inc_val;
    A.min_val = min_val;
    A.exc_rowptr = exc_rowptr;
    A.exc_col = exc_col;
    A.exclude_self = exclude_self != 0;
    A.thr = split_threshold < 0 ? LPF_REC_SPLIT_DEFAULT : split_threshold;
    A.long_list = scratch;
    A.count = nullptr;
    A.offset = nullptr;
    A.P = 0;
    A.pairs = nullptr;
    return A;
}

bool cand_valid(int64_t S, int64_t n, const int64_t *sources, const int64_t *inc_rowptr, const int32_t *inc_col,
                const float *inc_val, const int64_t *exc_rowptr, const int32_t *exc_col, int32_t *scratch) {
    return S > 0 && S < INT32_MAX && n > 0 && n <= INT32_MAX && sources && scratch &&
           (!inc_rowptr || (inc_col && inc_val)) && (!exc_rowptr || exc_col);
}

}  // namespace

extern "C" int lpf_rec_candidate_count(int64_t S, int64_t n, const int64_t *sources, const int64_t *inc_rowptr,
                                       const int32_t *inc_col, const float *inc_val, float min_val,
                                       const int64_t *exc_rowptr, const int32_t *exc_col, int32_t exclude_self,
                                       int32_t split_threshold, int32_t *scratch, int64_t *count, void *stream) {
    if (S == 0) return LPF_OK;
    LPF_REQUIRE(cand_valid(S, n, sources, inc_rowptr, inc_col, inc_val, exc_rowptr, exc_col, scratch) && count);
    CandArgs A = cand_args(S, n, sources, inc_rowptr, inc_col, inc_val, min_val, exc_rowptr, exc_col, exclude_self,
                           split_threshold, scratch);
    A.count = count;
    return rec_candidates(A, stream);
}

extern "C" int lpf_rec_candidate_fill(int64_t S, int64_t n, const int64_t *sources, const int64_t *inc_rowptr,
                                      const int32_t *inc_col, const float *inc_val, float min_val,
                                      const int64_t *exc_rowptr, const int32_t *exc_col, int32_t exclude_self,
                                      int32_t split_threshold, int32_t *scratch, const int64_t *offset, int64_t P,
                                      int64_t *pairs, void *stream) {
    if (S == 0 || P == 0) return LPF_OK;
    LPF_REQUIRE(cand_valid(S, n, sources, inc_rowptr, inc_col, inc_val, exc_rowptr, exc_col, scratch) && offset &&
                pairs && P > 0);
    CandArgs A = cand_args(S, n, sources, inc_rowptr, inc_col, inc_val, min_val, exc_rowptr, exc_col, exclude_self,
                           split_threshold, scratch);
    A.offset = offset;
    A.P = P;
    A.pairs = pairs;
    return rec_candidates(A, stream);
}

extern "C" int lpf_segment_topk_f32(int64_t S, const int64_t *seg_ptr, const float *score, const int64_t *cand,
                                    int32_t k, int32_t *scratch, int64_t *ids, float *scores, int64_t *counts,
                                    void *stream) {
    if (S == 0) return LPF_OK;
    LPF_REQUIRE(S > 0 && S < INT32_MAX && k >= 1 && k <= LPF_TOPK_MAX_K && seg_ptr && score && cand && scratch && ids &&
                scores && counts);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (lpf_reset_counter(scratch, s) != LPF_OK) return LPF_ERR_LAUNCH;   // long-segment counter
    hipLaunchKernelGGL(topk_wave_kernel, dim3((unsigned)((S + REC_WAVES - 1) / REC_WAVES)), dim3(REC_BLOCK), 0, s, S,
                       seg_ptr, score, cand, k, scratch, ids, scores, counts);
    LPF_CHECK_LAUNCH();
    const int64_t grid = S < REC_TOPK_GRID ? S : REC_TOPK_GRID;
    hipLaunchKernelGGL(topk_block_kernel, dim3((unsigned)grid), dim3(REC_TOPK_BLOCK), 0, s, seg_ptr, score, cand, k,
                       scratch, ids, scores, counts);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}
