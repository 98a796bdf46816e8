// Uniform negatives that avoid known edges: targets per source (lpf_negative_rows) and node pairs
// (lpf_negative_pairs) drawn on the device against a "known" CSR with sorted, unique int32 columns.  Fixed output
// shapes, one integer counter per call, nothing for the host to read in between.
//
// The draw (draw_common.h; restated in include/lpformer_hip.h and in lpformer_amd/negatives.py), all in uint64:
//   mix64(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
//   G = 0x9E3779B97F4A7C15;  key(seed, i) = mix64(seed + G (i + 1));  u(seed, i, j) = mix64(key(seed, i) + G (j + 1))
//   node(u, n) = (u * n) >> 64
// -- splitmix64 started at the slot's key.  Every output is a pure function of (seed, slot, graph, options): a slot
// reads its own stream only, and which draws it accepts depends on the graph and on its own earlier draws.
//
// Rows: one wavefront (one 64-thread workgroup) per row; lane l of round t takes draw j = 64 t + l.  A draw is valid
// when it is not the source and not in the source's row (binary search).  Repeats go through an LDS hash set of 2,048
// slots: a valid draw claims the slot of its node id by compare-and-swap (linear probing) and leaves its draw index
// there by an integer atomic min; after a barrier the lane whose index the slot holds is the FIRST draw of that id --
// within the round and against every earlier round -- and only it is accepted.  The set never holds more than
// K - 1 + 64 <= 1,087 ids.  Accepted lanes are ranked by ballot, which is draw order; positions >= K are dropped.
//
// Pairs: one lane per slot walks its stream until a pair (a, b) with a != b that is stored in neither direction.
//
// Integers only, no float atomics; the two counters are integer atomics, one per wavefront that has something to add.
#include "lpf_common.h"
#include "draw_common.h"

namespace {

constexpr int NS_TABLE = 2048;                  // hash-set slots per row (a power of two)
constexpr int NS_PAIR_BLOCK = 256;

typedef unsigned long long ns_u64;
static_assert(NS_TABLE == 2048, "lpf_hash11 yields 11 bits");

struct RowArgs {
    int64_t R, n;
    const int64_t *sources;
    int32_t K, max_draws;
    const int64_t *rowptr;
    const int32_t *col;
    uint64_t seed, row_base;
    int64_t *out;                               // [R][K]
    ns_u64 *short_rows;
};

__global__ __launch_bounds__(LPF_WAVE) void negative_rows_kernel(RowArgs A) {
    __shared__ int32_t keys[NS_TABLE];
    __shared__ uint32_t first[NS_TABLE];
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int32_t K = A.K;
    int64_t *out = A.out + r * K;
    const int64_t s = A.sources[r];
    if ((uint64_t)s >= (uint64_t)A.n) {           // workgroup-uniform
        for (int e = lane; e < K; e += LPF_WAVE) out[e] = -1;
        if (lane == 0) atomicAdd(A.short_rows, 1ull);
        return;
    }
    for (int e = lane; e < NS_TABLE; e += LPF_WAVE) {
        keys[e] = -1;
        first[e] = 0xFFFFFFFFu;
    }
    __syncthreads();
    const int64_t r0 = A.rowptr[s], r1 = A.rowptr[s + 1];
    // what the row can hold at all: every node but the source and the row's members
    int64_t avail = A.n - (r1 - r0) - (lpf_sorted_has(A.col, r0, r1, (int32_t)s) ? 0 : 1);
    avail = avail < 0 ? 0 : avail;
    const int32_t want = avail < K ? (int32_t)avail : K;
    const uint64_t key = lpf_draw_key(A.seed, A.row_base + (uint64_t)r);
    const uint32_t max_draws = (uint32_t)A.max_draws;
    int32_t kept = 0;
    for (uint32_t j0 = 0; kept < want && j0 < max_draws; j0 += LPF_WAVE) {   // workgroup-uniform
        const uint32_t j = j0 + lane;
        const int32_t c = lpf_draw_node(key, j, (uint64_t)A.n);
        const bool valid = j < max_draws && c != (int32_t)s && !lpf_sorted_has(A.col, r0, r1, c);
        uint32_t slot = 0;
        if (valid) {
            slot = lpf_hash11(c);
            for (;;) {
                const int32_t prev = atomicCAS(&keys[slot], -1, c);
                if (prev == -1 || prev == c) break;
                slot = (slot + 1) & (NS_TABLE - 1);
            }
            atomicMin(&first[slot], j);
        }
        __syncthreads();
        const bool acc = valid && first[slot] == j;
        __syncthreads();                          // the next round's atomicMin comes after these reads
        const uint64_t bm = __ballot(acc);
        const int32_t pos = kept + __popcll(bm & ((1ull << lane) - 1ull));
        if (acc && pos < K) out[pos] = c;
        kept += __popcll(bm);
    }
    kept = kept < K ? kept : K;
    for (int e = kept + lane; e < K; e += LPF_WAVE) out[e] = -1;
    if (lane == 0 && kept < K) atomicAdd(A.short_rows, 1ull);
}

struct PairArgs {
    int64_t M, n;
    const int64_t *rowptr;
    const int32_t *col;
    uint64_t seed, slot_base;
    int32_t max_draws;
    const uint8_t *active;
    int32_t *next;
    int64_t *pairs;
    int64_t ld;
    ns_u64 *unresolved;
};

__global__ __launch_bounds__(NS_PAIR_BLOCK) void negative_pairs_kernel(PairArgs A) {
    const int64_t i = (int64_t)blockIdx.x * NS_PAIR_BLOCK + threadIdx.x;
    bool lost = false;
    if (i < A.M && (!A.active || A.active[i])) {
        const uint64_t key = lpf_draw_key(A.seed, A.slot_base + (uint64_t)i);
        const uint64_t n = (uint64_t)A.n;
        int32_t j = A.next[i];
        j = j < 0 ? 0 : j;
        int64_t a = -1, b = -1;
        for (; j < A.max_draws; ++j) {
            const int32_t ca = lpf_draw_node(key, 2ull * (uint64_t)j, n), cb = lpf_draw_node(key, 2ull * (uint64_t)j + 1, n);
            if (ca == cb) continue;
            if (lpf_sorted_has(A.col, A.rowptr[ca], A.rowptr[ca + 1], cb)) continue;
            if (lpf_sorted_has(A.col, A.rowptr[cb], A.rowptr[cb + 1], ca)) continue;
            a = ca;
            b = cb;
            ++j;                                  // the draw index after the accepted one
            break;
        }
        A.pairs[i] = a;
        A.pairs[A.ld + i] = b;
        A.next[i] = j;
        lost = a < 0;
    }
    const uint64_t bm = __ballot(lost);
    if (bm && lpf_lane() == 0) atomicAdd(A.unresolved, (ns_u64)__popcll(bm));
}

int ns_zero_counter(int64_t *counter, hipStream_t s) {
    if (hipMemsetAsync(counter, 0, sizeof(int64_t), s) == hipSuccess) return LPF_OK;
    lpf_set_hip_error(hipGetLastError());
    return LPF_ERR_LAUNCH;
}

}  // namespace

extern "C" int lpf_negative_rows(int64_t R, int64_t n, const int64_t *sources, int32_t K, const int64_t *rowptr,
                                 const int32_t *col, uint64_t seed, int64_t row_base, int32_t max_draws, int64_t *out,
                                 int64_t *short_rows, void *stream) {
    LPF_REQUIRE(K >= 1 && K <= LPF_NEGATIVE_MAX_K && max_draws >= 1 && max_draws <= LPF_NEGATIVE_MAX_DRAWS &&
                short_rows && R >= 0 && R < INT32_MAX);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = ns_zero_counter(short_rows, s);
    if (rc != LPF_OK || R == 0) return rc;
    LPF_REQUIRE(n > 0 && n < INT32_MAX && sources && rowptr && col && out);
    RowArgs A{};
    A.R = R;
    A.n = n;
    A.sources = sources;
    A.K = K;
    A.max_draws = max_draws;
    A.rowptr = rowptr;
    A.col = col;
    A.seed = seed;
    A.row_base = (uint64_t)row_base;
    A.out = out;
    A.short_rows = reinterpret_cast<ns_u64 *>(short_rows);
    hipLaunchKernelGGL(negative_rows_kernel, dim3((unsigned)R), dim3(LPF_WAVE), 0, s, A);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}

extern "C" int lpf_negative_pairs(int64_t M, int64_t n, const int64_t *rowptr, const int32_t *col, uint64_t seed,
                                  int64_t slot_base, int32_t max_draws, const uint8_t *active, int32_t *next,
                                  int64_t *pairs, int64_t pair_stride, int64_t *unresolved, void *stream) {
    LPF_REQUIRE(max_draws >= 1 && max_draws <= LPF_NEGATIVE_MAX_DRAWS && unresolved && M >= 0 && M < INT32_MAX);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = ns_zero_counter(unresolved, s);
    if (rc != LPF_OK || M == 0) return rc;
    LPF_REQUIRE(n > 0 && n < INT32_MAX && rowptr && col && next && pairs && pair_stride >= M);
    PairArgs A{};
    A.M = M;
    A.n = n;
    A.rowptr = rowptr;
    A.col = col;
    A.seed = seed;
    A.slot_base = (uint64_t)slot_base;
    A.max_draws = max_draws;
    A.active = active;
    A.next = next;
    A.pairs = pairs;
    A.ld = pair_stride;
    A.unresolved = reinterpret_cast<ns_u64 *>(unresolved);
    const int64_t grid = (M + NS_PAIR_BLOCK - 1) / NS_PAIR_BLOCK;
    hipLaunchKernelGGL(negative_pairs_kernel, dim3((unsigned)grid), dim3(NS_PAIR_BLOCK), 0, s, A);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}
