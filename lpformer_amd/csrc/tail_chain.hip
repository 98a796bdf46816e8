// The dense tail of the scoring path in ONE launch (LinkTransformer.score_pairs):
//
//   A  o   = LayerNorm_post( G[:, D:] Wcat^T + G[:, :D] )                attention output (layers.py:78)
//   B  r_p = ReLU(LayerNorm( W_p0 [o | counts] + b_p0 ))                 first layer of pairwise_lin
//   C  s   = w_s1 . ReLU( A_e r_e + A_p r_p + c ) + b_s1 ; sigmoid       score head with the boundary Linears folded
//
// Same machinery as dense_chain.hip (samples on the MFMA columns, a pair of wavefronts per 16 samples splitting the
// feature tiles, weights host-packed in A-operand order and staged global -> registers -> LDS ahead of the MFMAs,
// double-buffered, one barrier per stage -- here as one stream through all stages, see TC_PIN), with three stages
// chained through LDS: a stage's accumulators, written in accumulator layout, are the next stage's B operands.  What the stage boundaries read besides -- biases, LayerNorm
// weights, w_dot -- is requested once at the start of the workgroup and waits in LDS.  Stage B appends one k-group read from global memory (the
// count features), stage C starts with k-groups read from global memory (r_e, produced on the side stream by the
// elementwise branch).  Against three separate launches this removes two launch ramps and the round trips of the
// attention output and of r_p through HBM.
//
// Stage E (rows + perm form, fp32, D = 128: lpf_tail_chain_rows_perm_ew_f32) puts the elementwise branch in front:
//   E  r_e = ReLU(LayerNorm( W_e0 (x_a * x_b) + b_e0 ))                  first layer of elementwise_lin
// with the arithmetic of dense_chain.hip (in_mode 1), operation for operation; the rows are gathered whole (8 adjacent
// lanes per 128-byte line, every row once per workgroup) and the products reach the k-loop through the hidden tiles.
// r_e goes to the hidden tiles and stage C's r_e half runs directly behind it -- the tiles are free again before stage A writes
// them, so LDS does not grow --; its accumulators then live across stages A and B.  Order inside a workgroup:
// E -> C over r_e -> (64 pairs without selected nodes: epilogue, done) -> A -> B -> C over r_p -> epilogue.  Stage C
// sums in the order it always did (r_e k-groups first), so the scores are bitwise those of the separate launches.
#include <type_traits>
#include <utility>

#include "lpf_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

#ifndef LPF_TC_GROUPS
#define LPF_TC_GROUPS 4
#endif
constexpr int TC_GROUPS = LPF_TC_GROUPS;   // 16-sample groups per workgroup
constexpr int TC_WAVES = 2 * TC_GROUPS;    // a wave pair per group
constexpr int TC_THREADS = 64 * TC_WAVES;

struct TailArgs {
    int64_t M;
    const float *x; int64_t ldx; int KA;               // stage A input rows [M, KA]
    const float *addend; int64_t ldadd;                // [M, NA]
    const float *wA, *lnA_g, *lnA_b; int NA;
    const float *tail; int64_t ldtail;                 // [M, 4] appended to stage B's input (count features)
    const float *wB, *bB, *lnB_g, *lnB_b; int NB;
    const float *re; int64_t ldre;                     // [M, 16 * NGE] leading input of stage C
    const float *wC, *bC; int NC;
    const float *wdot, *bdot;
    float *logit, *prob;
    // merge mode (part != nullptr): stage A is not a GEMM but the merge of the per-type attention records written by
    // lpf_pair_attention_fused_f32 -- out = sum_t e^{m_t - M} acc_t / (sum_t e^{m_t - M} l_t + 1e-16) + bias -- and the
    // count features come from the int32 segment pointers of the selection
    const float *part;              // [3][M][NA + 4]: acc[NA], m, l, -, -
    const float *bnd;               // [3][units_cap][2][NA + 4]: boundary records of segments that cross 16-entry units
    int64_t units_cap;
    const int32_t *type_ptr;        // [3][M + 1]
    const float *att_bias;          // [NA]
    const int64_t *sel_ctl;         // selection control block: word 3 != 0 => the batch did not fit, scores = NaN
    int n_counts;
    // rows mode (rows != nullptr): stage A is already done -- lpf_pair_attention_rows_* left one finished row per pair,
    // [post_att_norm(attention output) (NA) | count features (4, zero padded)] -- and is a plain read
    const float *rows; int64_t ldrows;
    // rows mode, optional: the pairs are taken in the order perm[] (lpf_pair_attention_rows_perm_*: those with selected
    // nodes first, *n_full of them, the others behind).  A workgroup whose 64 pairs all lie behind *n_full skips stage
    // A, stage B and the r_p half of stage C: the pairwise branch of a pair without selected nodes is a constant, folded
    // into bC_empty on the host (fold.empty_pair_head_bias).
    const int32_t *perm;
    const int64_t *n_full;
    const float *bC_empty;
    // ... and a pair without selected nodes in a MIXED workgroup takes its (constant) row from here and zero counts: the
    // attention kernel that leaves the order does not write rows for such pairs
    const float *row_empty;         // [NA]
    // stage E (EW instantiation, wE != nullptr): r_e is not read from `re` but computed from the node table, X[a] * X[b]
    // gathered through batch[0][m], batch[1][m] (ids outside [0, n_rows) read row 0, as in dense_chain.hip)
    const float *X; int64_t ldX;
    const int64_t *batch; int64_t batch_ld, n_rows;
    const float *wE, *bE, *lnE_g, *lnE_b;
};

constexpr int tc_per_thread(int ntp) { return (ntp * 64 + TC_THREADS - 1) / TC_THREADS; }
// elements between two stages of a packed weight image (lpformer_amd/fold.py pack_dense: padded to 512 per stage)
constexpr int tc_stage_stride(int ntp) { return (ntp * 64 + 511) / 512 * 512; }

// weight elements: one per (tile, lane) and k-group -- four fp32 (f32x4) or, in the bf16 variant, four bf16 (uint2) of
// W[16 c + i][16 ks + 4 q .. + 3]
typedef short bf16x4_bits __attribute__((ext_vector_type(4)));
// (one register stage serves every weight stream of the kernel: PM elements, a stream uses the first P)
template <int P, int NTP, int PM, typename T>
__device__ __forceinline__ void tc_load(T (&r)[PM], const float *packed, int stage, int tid) {
    static_assert(P <= PM, "the register stage holds a weight stage");
    const T *src = reinterpret_cast<const T *>(packed) + (int64_t)stage * tc_stage_stride(NTP);
#pragma unroll
    for (int e = 0; e < P; ++e) {
        const int i = e * TC_THREADS + tid;
#ifdef TC_NOWLOAD      /* (tuning builds: how much of the kernel is waiting for the weight stream?) */
        r[e] = T{};
        (void)src; (void)i;
#else
        r[e] = src[i < tc_stage_stride(NTP) ? i : 0];   // (the last strip of a thread may lie past the stage's padding)
#endif
    }
}
template <int P, int PM, typename T>
__device__ __forceinline__ void tc_store(const T (&r)[PM], T *slab, int tid) {
    static_assert(P <= PM, "the register stage holds a weight stage");
#pragma unroll
    for (int e = 0; e < P; ++e) slab[e * TC_THREADS + tid] = r[e];
}

// The weights are ONE stream through the kernel, two stages ahead of the MFMAs: while k-group kg runs out of one slab,
// stage kg + 1 -- requested a k-group earlier -- goes from the registers to the other slab, and stage kg + 2 is
// requested into the same registers.  A k-group is
//     operand reads | its first MFMAs | wait for kg + 1, store it, request kg + 2 | the other MFMAs | barrier
// so nothing but the wait for the store's completion stands between a k-group's last MFMA and the barrier, and nothing
// but the operand reads between the barrier and the next k-group's first MFMA: the store, its wait for the weights and
// the request's address arithmetic run under the matrix pipe.  The other slab is free by then -- every wavefront read
// its operands of kg - 1 before the MFMAs it issued in front of the barrier that ended kg - 1.  The stream runs across
// the stage boundaries: a stage's last two k-groups store and request the next stage's first two weight stages, so a
// stage starts with its weights published and no round trip of its own.  A stage's last k-group has no barrier where
// the boundary behind it (a LayerNorm exchange, the publication of the hidden tiles) brings one anyway.
// Nothing is scheduled across a TC_PIN(); the scheduler, left alone, sinks the request to the end of the k-group and
// pulls the store and the barrier into the MFMA stream (tools/tail_isa.py reads the order back from the assembly).
#define TC_PIN() __builtin_amdgcn_sched_barrier(0)
struct TcNoStep { __device__ __forceinline__ void operator()() const {} };
// the barrier between two k-groups of a stage (tools/tail_isa.py knows the k-groups by it)
__device__ __forceinline__ void tc_kgroup_barrier() { __syncthreads(); }
// f(kg) for kg = 0, STEP, .. < N with kg a constant expression: which stream a k-group's weight step serves is decided
// per k-group at compile time (as run-time branches of an unrolled loop the two requests are merged into one with a
// selected address, and the assembly no longer says which call made a load)
template <int STEP, typename F, int... I>
__device__ __forceinline__ void tc_each_impl(F &f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I * STEP>()), ...);
}
template <int N, int STEP = 1, typename F>
__device__ __forceinline__ void tc_each(F f) {
    tc_each_impl<STEP>(f, std::make_integer_sequence<int, (N + STEP - 1) / STEP>());
}

// acc[c] += W[16 (c0 + c) + i][k-group] * bv for this wave's TPW tiles; lw = slab + c0 * 64 + lane.  last = false (the
// same for the whole wavefront): the wave's last tile is padding -- all-zero weight rows -- and is left out.
// step(): the weight stream's store and request of this k-group, run behind the k-group's first MFMAs.
template <int TPW, typename Step = TcNoStep>
__device__ __forceinline__ void tc_mfma(f32x4 (&acc)[TPW], const f32x4 *lw, const f32x4 bv, bool last = true,
                                        Step step = Step()) {
    // (eight tiles and more go four at a time: with all their operands read at once the D = 128 forms no longer fit
    //  128 registers beside the weight stage that now stays in flight through the whole k-group; an accumulator still
    //  takes its four MFMAs in ascending k)
    constexpr int H = TPW >= 8 ? 4 : TPW;
#pragma unroll
    for (int h = 0; h < TPW; h += H) {
        f32x4 a[H];
#pragma unroll
        for (int c = 0; c < H; ++c) a[c] = lw[(h + c < TPW ? h + c : TPW - 1) * 64];
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // consecutive MFMAs go to different accumulators
            // (the tile that may be padding goes first: what a wavefront that leaves it out has to restore then stands
            //  in front of the other MFMAs, not between the k-group's last one and the barrier)
            if (h + H >= TPW && last)
                acc[TPW - 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[TPW - 1 - h][u], bv[u], acc[TPW - 1], 0, 0, 0);
#pragma unroll
            for (int c = 0; c < H; ++c)
                if (h + c < TPW - 1) acc[h + c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c][u], bv[u], acc[h + c], 0, 0, 0);
            if constexpr (!std::is_same<Step, TcNoStep>::value) {
                if (u == 0 && h == 0) {
                    TC_PIN();
                    step();
                    TC_PIN();
                }
            }
        }
    }
}
// bf16 variant: the four fp32 MFMAs of a k-group become ONE v_mfma_f32_16x16x16_bf16 -- a lane's four A values and
// four B values (k = 4 q .. 4 q + 3 of the group) are exactly that instruction's operands; the activations are rounded
// to bf16 here, the accumulation stays fp32.
template <int TPW, typename Step = TcNoStep>
__device__ __forceinline__ void tc_mfma(f32x4 (&acc)[TPW], const uint2 *lw, const f32x4 bv, bool last = true,
                                        Step step = Step()) {
    bf16x4_bits b;
#pragma unroll
    for (int u = 0; u < 4; ++u) b[u] = (short)lpf_f32_to_bf16(bv[u]);
    uint2 w[TPW];
#pragma unroll
    for (int c = 0; c < TPW; ++c) w[c] = lw[c * 64];
#pragma unroll
    for (int c = 0; c < TPW; ++c) {
        if (c == TPW - 1 && !last) break;
        const bf16x4_bits a = {(short)(w[c].x & 0xffffu), (short)(w[c].x >> 16), (short)(w[c].y & 0xffffu),
                               (short)(w[c].y >> 16)};
        acc[c] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, acc[c], 0, 0, 0);
        if constexpr (!std::is_same<Step, TcNoStep>::value) {
            if (c == 0) {
                TC_PIN();
                step();
                TC_PIN();
            }
        }
    }
}

// LayerNorm over the n real features held by the wave pair (this wave: TPW tiles from feature fbase), in place.
// my_x / peer_x: this wave's and its peer's word of the exchange slot of s1; those of s2 lie TC_XCH_SLOT floats behind.
// Every exchange of the kernel has a slot of its own (TcShape) and a workgroup runs the kernel's stages once, so a slot
// is written once in a workgroup's life: there is no earlier value somebody could still be reading, and the only barrier
// an exchange needs is the one between its write and its read.
constexpr int TC_XCH_SLOT = TC_WAVES * 16;
template <int TPW>
__device__ __forceinline__ void tc_layernorm(f32x4 (&acc)[TPW], int fbase, int n, const float *g, const float *b, int half,
                                             int q, float *my_x, const float *peer_x, bool relu) {
    float s1 = 0.f;
#pragma unroll
    for (int c = 0; c < TPW; ++c) s1 += acc[c][0] + acc[c][1] + acc[c][2] + acc[c][3];
    s1 = lpf_quad_sum(s1);  // padded features are exactly 0 and add nothing
    if (q == 0) *my_x = s1;
    __syncthreads();
    const float mean = (half == 0 ? s1 + *peer_x : *peer_x + s1) / (float)n;  // same order in both waves
    float s2 = 0.f;
#pragma unroll
    for (int c = 0; c < TPW; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float d = (fbase + 16 * c + r < n) ? acc[c][r] - mean : 0.f;
            s2 += d * d;
        }
    s2 = lpf_quad_sum(s2);
    if (q == 0) my_x[TC_XCH_SLOT] = s2;
    __syncthreads();
    const float p2 = peer_x[TC_XCH_SLOT];
    const float rstd = 1.0f / sqrtf((half == 0 ? s2 + p2 : p2 + s2) / (float)n + 1e-5f);
#pragma unroll
    for (int c = 0; c < TPW; ++c) {
        const f32x4 gg = *reinterpret_cast<const f32x4 *>(g + fbase + 16 * c);  // zero-padded: pads come out 0
        const f32x4 bb = *reinterpret_cast<const f32x4 *>(b + fbase + 16 * c);
        acc[c] = (acc[c] - mean) * rstd * gg + bb;
        if (relu) {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[c][r] = fmaxf(acc[c][r], 0.f);
        }
    }
}

// (tuning builds, -DTC_STAMPS: wall-clock marks -- 100 MHz -- of lane 0 of every wavefront; tools/tail_stamps.py)
#ifdef TC_STAMPS
__device__ uint64_t *tc_stamp_buf = nullptr;
#define TC_STAMP(k) do { if (lane == 0) st_t[k] = wall_clock64(); } while (0)
#define TC_STAMPS_OUT(kind) do { if (lane == 0 && tc_stamp_buf) { uint64_t *o__ = tc_stamp_buf + ((int64_t)blockIdx.x * TC_WAVES + wave) * 16; \
        for (int k__ = 0; k__ < 10; ++k__) o__[k__] = st_t[k__]; o__[15] = (kind); } } while (0)
// (16 words per wavefront: marks 0-6 as they always were, 7 = stage E done -- with it mark 4, C's r_e k-groups, comes
//  BEFORE mark 1 --, 8 = stage E's gathered rows have arrived (the stamped build waits for them there, vmcnt(0);
//  the product build waits where the first use is), 9 = stage E's k-loop done, word 15 = the kind)
#define TC_STAMP_ROWS() do { __builtin_amdgcn_s_waitcnt(0x0f70); TC_STAMP(8); } while (0)
#else
#define TC_STAMP_ROWS() do { } while (0)
#define TC_STAMP(k) do { } while (0)
#define TC_STAMPS_OUT(kind) do { } while (0)
#endif

// NTA / NTB / NTC: 16-feature tiles of the three stages' outputs (NTA = NGE = D/16)
template <int NTA, int NTB, int NTC>
struct TcShape {
    static constexpr int NTPA = (NTA + 1) & ~1, NTPB = (NTB + 1) & ~1, NTPC = (NTC + 1) & ~1;
    static constexpr int PA = tc_per_thread(NTPA), PB = tc_per_thread(NTPB), PC = tc_per_thread(NTPC);
    static constexpr int PM = PA > PB ? (PA > PC ? PA : PC) : (PB > PC ? PB : PC);
    static constexpr int SLAB = PM * TC_THREADS;
    static constexpr int HT = NTPA > NTPB ? NTPA : NTPB;  // hidden tiles kept per sample group
    static constexpr int HID = TC_GROUPS * HT * 64;
    // exchange slots: s1, s2 of the first LayerNorm (E, or A in the forms that have one), s1, s2 of LayerNorm B, the score dot
    static constexpr int XCH = 5 * TC_WAVES * 16;
    // the boundary vectors, staged in LDS once per workgroup (floats): bE, lnE_g, lnE_b | bB, lnB_g, lnB_b | bC (or
    // bC_empty), w_dot -- each zero-padded by the host to its stage's padded tiles
    static constexpr int VEC_B = 3 * 16 * NTPA, VEC_C = VEC_B + 3 * 16 * NTPB, VEC_N = VEC_C + 2 * 16 * NTPC;
    static constexpr size_t BYTES = (size_t)(2 * SLAB + HID) * sizeof(f32x4) + (XCH + VEC_N) * sizeof(float);
    static_assert(NTC >= 32 || BYTES <= 81920, "two workgroups share a CU's 160 KB of LDS");
};

// (D = 256: 32 output tiles of the score head -- 16 accumulators per lane in stage C alone --, one workgroup per CU with
//  twice the registers)
// WM: how the two GEMMs run -- 0 fp32 weights and MFMAs, 1 bf16 weights and activations (throughput mode)
// EW: stage E in front (rows + perm form, fp32)
template <int NTA, int NTB, int NTC, int WM = 0, bool ROWS = false, bool EW = false>
__global__ __launch_bounds__(TC_THREADS, NTC >= 32 ? 2 : (TC_THREADS >= 512 ? 4 : 3)) void tail_chain_kernel(const TailArgs A) {
    using S = TcShape<NTA, NTB, NTC>;
    constexpr bool WB = WM != 0;
    // weight element: four fp32 or four bf16
    using WT = typename std::conditional<WM == 1, uint2, f32x4>::type;
    constexpr int NTPA = S::NTPA, NTPB = S::NTPB, NTPC = S::NTPC;
    constexpr int TPWA = NTPA / 2, TPWB = NTPB / 2, TPWC = NTPC / 2;
    constexpr int NGE = NTA;  // k-groups of r_e
    extern __shared__ __attribute__((aligned(16))) f32x4 lds[];
    f32x4 *hid = lds + 2 * S::SLAB;
    float *xch = reinterpret_cast<float *>(hid + S::HID);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = wave >> 1, half = wave & 1, q = lane >> 4, j = lane & 15;
    float *my_x = xch + wave * 16 + j;                  // (slot 0; slot k lies k * TC_XCH_SLOT floats behind)
    const float *peer_x = xch + (wave ^ 1) * 16 + j;
    float *vec = xch + S::XCH;
    f32x4 *my_hid = hid + (grp * S::HT) * 64 + lane;
    int buf = 0;                // the slab the current k-group reads; the stream's next stage goes to the other one
    WT wr[S::PM];               // the weight stream's register stage
    WT *const slabs = reinterpret_cast<WT *>(lds);
#ifdef TC_STAMPS
    uint64_t st_t[10] = {0};
    TC_STAMP(0);
#endif

    // (With an order the short workgroups are the LAST ones of the grid.  Dealing the tiles from both ends instead, a short
    // workgroup next to every full one on a CU, measured worse: collab-like 0.205 against 0.186 ms per pipelined step, the
    // launch alone unchanged at 55 us -- what the short workgroups buy is a grid that drains early for the next kernel.)
    const int64_t tile = blockIdx.x;
    const int64_t pos = tile * (16 * TC_GROUPS) + grp * 16 + j;
    const bool live = pos < A.M;
    bool lite = false;          // (rows mode with an order: every pair of this workgroup is one without selected nodes)
    int64_t m = pos;
    if constexpr (ROWS) {
        if (A.perm) {
            m = A.perm[live ? pos : A.M - 1];
            lite = tile * (16 * TC_GROUPS) >= *A.n_full;
        }
    }
    const int64_t mm = live ? m : (ROWS && A.perm ? m : A.M - 1);  // dead lanes compute on a valid row and store nothing
    bool no_sel = false;        // (rows mode with an order: this pair has no selected nodes)
    if constexpr (ROWS) no_sel = A.perm && A.row_empty && (live ? pos : A.M - 1) >= *A.n_full;

    // The boundary vectors (about 1.4 k floats at D = 128) go through LDS: requested here, one 16-byte piece per thread,
    // written (tc_vec_publish) in front of the first barrier of whichever path the workgroup takes -- by then the wait
    // for the first weight stage, requested behind them, has covered them -- and read where the LayerNorms and the
    // epilogue used to wait for a global round trip each.  Threads past the last piece request and write the last piece
    // again (the same value to the same place): with a guard around the write the request is sunk into the guard, to
    // the far end of everything requested in between.
    constexpr int VP0 = EW ? 0 : S::VEC_B / 4, VPN = S::VEC_N / 4 - VP0, VPT = (VPN + TC_THREADS - 1) / TC_THREADS;
    f32x4 vecr[VPT];
#pragma unroll
    for (int e = 0; e < VPT; ++e) {
        int p = VP0 + e * TC_THREADS + tid;
        p = p < S::VEC_N / 4 ? p : S::VEC_N / 4 - 1;
        const float *src;
        if (p >= S::VEC_C / 4) {
            const int o = p - S::VEC_C / 4;
            src = o < 4 * NTPC ? (lite ? A.bC_empty : A.bC) + 4 * o : A.wdot + 4 * (o - 4 * NTPC);
        } else if (!EW || p >= S::VEC_B / 4) {
            const int o = p - S::VEC_B / 4;
            src = o < 4 * NTPB ? A.bB + 4 * o : (o < 8 * NTPB ? A.lnB_g + 4 * (o - 4 * NTPB) : A.lnB_b + 4 * (o - 8 * NTPB));
        } else {
            src = p < 4 * NTPA ? A.bE + 4 * p : (p < 8 * NTPA ? A.lnE_g + 4 * (p - 4 * NTPA) : A.lnE_b + 4 * (p - 8 * NTPA));
        }
        vecr[e] = *reinterpret_cast<const f32x4 *>(src);
    }
    TC_PIN();   // (the requests stay here, in front of whatever the first stage gathers)
    auto tc_vec_publish = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < VPT; ++e) {
            int p = VP0 + e * TC_THREADS + tid;
            p = p < S::VEC_N / 4 ? p : S::VEC_N / 4 - 1;
            reinterpret_cast<f32x4 *>(vec)[p] = vecr[e];
        }
    };
    const float *v_bE = vec, *v_lnE_g = vec + 16 * NTPA, *v_lnE_b = vec + 32 * NTPA;
    const float *v_bB = vec + S::VEC_B, *v_lnB_g = v_bB + 16 * NTPB, *v_lnB_b = v_bB + 32 * NTPB;
    const float *v_bC = vec + S::VEC_C, *v_wdot = v_bC + 16 * NTPC;

    // rows mode: a pair's finished row and its count features, all pieces requested together -- addresses clamped into
    // the row, the values selected where stage A and stage B take them.  The counts are read from the
    // pair's own row even where the pair takes the constant row: row_empty has no counts, and the value is dropped.
    f32x4 rowv[ROWS ? TPWA : 1], rowt = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < (ROWS ? TPWA : 1); ++c) rowv[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto tc_rows_request = [&]() __attribute__((always_inline)) {
        if constexpr (ROWS) {
            const int fbase = 16 * half * TPWA + 4 * q;
            // (stage E form: a workgroup without selected nodes requests too -- every lane the first row, whose values
            //  nobody takes -- so that the counted waits of the weight stream behind the request are the same on both
            //  paths; with the request under a branch they become waits for everything)
            const float *own = A.rows + (EW && lite ? 0 : mm * A.ldrows), *row = no_sel ? A.row_empty : own;
#pragma unroll
            for (int c = 0; c < TPWA; ++c) {
                const int f0 = fbase + 16 * c;
                rowv[c] = *reinterpret_cast<const f32x4 *>(row + (f0 < A.NA ? f0 : 0));
            }
            rowt = *reinterpret_cast<const f32x4 *>(own + A.NA);
        }
    };

    f32x4 accC[TPWC];           // stage C's accumulators (with stage E they are filled first and live across A and B)
    if constexpr (EW) {
        static_assert(ROWS && WM == 0 && S::PA == 1 && NTPA == NTA && NGE % 2 == 0 && 2 * tc_stage_stride(NTPA) <= S::SLAB &&
                          tc_stage_stride(2 * NTPA) == 2 * tc_stage_stride(NTPA), "stage E: the fp32 rows form at D = 128");
        // ------------------------------------------------------------------ stage E: first layer of elementwise_lin
        // dense_chain.hip's layer 1 with in_mode 1: the B operand of k-group kg is X[a][16 kg + 4 q ..] * X[b][..].  The
        // rows are gathered whole, not in operand shape: a wavefront takes 8 of its group's 16 pairs (the wave pair splits
        // them), 8 adjacent lanes per pair, and lane 8 jj + p reads the 16-byte piece p of each 128-byte line of the
        // pair's two rows -- a load instruction touches 8 whole lines, and the wave pair no longer fetches every row
        // twice: 8 loads per lane, all requested at once in front of the first k-group.  The products go to the
        // (still free) hidden tiles in B-operand order and the k-loop reads them back: (kg, q, j) lies at
        // kg TE_KG + (q >> 1) TE_Q2 + (q & 1) 16 + j.  The two strides are what keeps the banks apart: ds_read_b128
        // serves lanes {0-3, 12-15, 20-27} .. together (j and 16 + j must differ mod 16: the (q & 1) 16), ds_write_b128
        // 8 adjacent lanes -- here the 8 pieces (2 k-groups x 4 q) of one pair -- over 8 slots of 16 bytes: TE_KG = 4,
        // TE_Q2 = 2 (mod 8) leave q and q ^ 1 on one slot, a 2-way conflict (16 LDS cycles against the 13 the store
        // takes to hand over its registers), where the plain tiles would be 8-way.
        constexpr int TE_KG = 68, TE_Q2 = 34;
        static_assert((NGE - 1) * TE_KG + TE_Q2 + 32 <= S::HT * 64, "stage E's product tiles fit a group's hidden tiles");
        const int gj = 8 * half + (lane >> 3), gp = lane & 7;       // pair of the group and piece of a line this lane gathers
        const int64_t gpos = tile * (16 * TC_GROUPS) + grp * 16 + gj;
        const int64_t gm = gpos < A.M ? gpos : A.M - 1;             // (a dead lane gathers what it would compute on)
        const int64_t gmm = A.perm ? A.perm[gm] : gm;
        int64_t ra = A.batch[gmm], rb = A.batch[A.batch_ld + gmm];
        static_assert(S::PM >= 2 && S::PC <= S::PM && NGE >= 4, "stage E's weight stages fit the register stage");
        tc_load<2, 2 * NTPA>(wr, A.wE, 0, tid);
        TC_PIN();   // (the first weights are requested next to the ids, not behind the eight pieces of the rows)
        if ((uint64_t)ra >= (uint64_t)A.n_rows) ra = 0;
        if ((uint64_t)rb >= (uint64_t)A.n_rows) rb = 0;
        const float *xa = A.X + ra * A.ldX + 4 * gp, *xb = A.X + rb * A.ldX + 4 * gp;
        f32x4 accE[TPWA];
#pragma unroll
        for (int c = 0; c < TPWA; ++c) accE[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
        f32x4 xra[NGE / 2], xrb[NGE / 2];
#pragma unroll
        for (int i = 0; i < NGE / 2; ++i) {                         // line i of a row: k-groups 2 i and 2 i + 1
            xra[i] = *reinterpret_cast<const f32x4 *>(xa + 32 * i);
            xrb[i] = *reinterpret_cast<const f32x4 *>(xb + 32 * i);
        }
        // the stream's start: stage 0 waits for nothing but itself (the eight pieces stay in flight), stage 1 flies
        // while the pieces arrive
        tc_store<2>(wr, slabs + buf * S::SLAB, tid);
        tc_load<2, 2 * NTPA>(wr, A.wE, 1, tid);
        TC_PIN();
        tc_vec_publish();
        TC_STAMP_ROWS();
        {
            f32x4 *pe = hid + (grp * S::HT) * 64 + (gp >> 2) * TE_KG + ((gp >> 1) & 1) * TE_Q2 + (gp & 1) * 16 + gj;
#pragma unroll
            for (int i = 0; i < NGE / 2; ++i) pe[2 * i * TE_KG] = xra[i] * xrb[i];
        }
        const f32x4 *my_pe = hid + (grp * S::HT) * 64 + (q >> 1) * TE_Q2 + (q & 1) * 16 + j;
        __syncthreads();   // publishes the products, the boundary vectors and the first weight stage
        // (two k-groups per weight stage and barrier: a k-group of this layer is 512 float4, a slab holds 1,024; the
        //  k-groups still reach an accumulator in ascending order.  The last two weight steps are stage C's first two.)
        tc_each<NGE, 2>([&](auto KG) __attribute__((always_inline)) {
            constexpr int kg = decltype(KG)::value;
            const WT *lw = slabs + buf * S::SLAB;
            WT *nw = slabs + (buf ^ 1) * S::SLAB;
            const f32x4 bv0 = my_pe[kg * TE_KG], bv1 = my_pe[(kg + 1) * TE_KG];
            tc_mfma<TPWA>(accE, lw + (half * TPWA) * 64 + lane, bv0, true, [&]() __attribute__((always_inline)) {
                if constexpr (kg + 2 < NGE) tc_store<2>(wr, nw, tid);
                else tc_store<S::PC>(wr, nw, tid);
                if constexpr (kg + 4 < NGE) tc_load<2, 2 * NTPA>(wr, A.wE, kg / 2 + 2, tid);
                else tc_load<S::PC, NTPC>(wr, A.wC, (kg + 4 - NGE) / 2, tid);
            });
            tc_mfma<TPWA>(accE, lw + tc_stage_stride(NTPA) + (half * TPWA) * 64 + lane, bv1);
            TC_PIN();
            buf ^= 1;
            if constexpr (kg + 2 < NGE) tc_kgroup_barrier();   // (behind the last k-group the LayerNorm's barriers follow)
        });
        TC_STAMP(9);
        // stage A's rows: requested here, a LayerNorm and eight k-groups ahead of their use (the registers of the gathered
        // rows are free from here on), instead of one more round trip in front of stage B.  Stage C's first weights are
        // in their slab already, the second stage was requested in front of the rows: its wait leaves them in flight.
        tc_rows_request();
        TC_PIN();
        {   // bias -> LayerNorm -> ReLU: dense_chain.hip's epilogue 1, same operations in the same order
            const int fbase = 16 * half * TPWA + 4 * q;
#pragma unroll
            for (int c = 0; c < TPWA; ++c) accE[c] += *reinterpret_cast<const f32x4 *>(v_bE + fbase + 16 * c);
            tc_layernorm<TPWA>(accE, fbase, A.NA, v_lnE_g, v_lnE_b, half, q, my_x, peer_x, true);
#pragma unroll
            for (int c = 0; c < TPWA; ++c) my_hid[(half * TPWA + c) * 64] = accE[c];
        }
        TC_STAMP(7);
        // ---- stage C over the r_e k-groups, r_e straight from LDS
#pragma unroll
        for (int c = 0; c < TPWC; ++c) accC[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
        __syncthreads();   // publishes r_e (and the weight stage stored under stage E's last k-groups)
        // (unrolled: the wait of k-group 0 leaves the rows in flight, which a loop's one wait for all trips cannot; the
        //  last two weight steps of a workgroup that goes on are stage B's first two)
        tc_each<NGE>([&](auto KG) __attribute__((always_inline)) {
            constexpr int kg = decltype(KG)::value;
            const WT *lw = slabs + buf * S::SLAB;
            WT *nw = slabs + (buf ^ 1) * S::SLAB;
            tc_mfma<TPWC>(accC, lw + (half * TPWC) * 64 + lane, my_hid[kg * 64], true, [&]() __attribute__((always_inline)) {
                if constexpr (kg + 2 < NGE) {
                    tc_store<S::PC>(wr, nw, tid);
                    tc_load<S::PC, NTPC>(wr, A.wC, kg + 2, tid);
                } else if (!lite) {
                    if constexpr (kg + 1 < NGE) tc_store<S::PC>(wr, nw, tid);
                    else tc_store<S::PB>(wr, nw, tid);
                    if constexpr (kg + 2 == NGE) tc_load<S::PB, NTPB>(wr, A.wB, 0, tid);
                    else tc_load<S::PB, NTPB>(wr, A.wB, 1, tid);
                } else if constexpr (kg + 1 < NGE) {
                    tc_store<S::PC>(wr, nw, tid);
                }
            });
            TC_PIN();
            buf ^= 1;
            // (behind the last k-group: every wave has read r_e, stage A may write the hidden tiles -- workgroup-uniform)
            if constexpr (kg + 1 < NGE) tc_kgroup_barrier();
            else if (!lite) __syncthreads();
        });
        TC_STAMP(4);
    }

    if constexpr (ROWS) {
        if (lite) {
            // ---- 64 pairs without selected nodes: score = w_dot . ReLU(A_e r_e + bC_empty) + b_dot -- stage C over the
            //      r_e k-groups alone (35 % of the matrix work of a full workgroup), nothing else
            f32x4 (&acc)[TPWC] = accC;
            if constexpr (!EW) {
#pragma unroll
            for (int c = 0; c < TPWC; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
            static_assert(NGE >= 2, "the stream's start requests two stages");
            const float *rer = A.re + mm * A.ldre + 4 * q;
            tc_load<S::PC, NTPC>(wr, A.wC, 0, tid);
            // r_e runs one k-group ahead: a group is requested in front of the weight stage of its step, so its wait at
            // the head of the next k-group leaves that step's weights in flight.  Two registers take turns (k-groups
            // in pairs): a loop that carries one copies it, and the copy waits for everything in front of the barrier.
            f32x4 x0 = *reinterpret_cast<const f32x4 *>(rer), x1 = (f32x4){0.f, 0.f, 0.f, 0.f};
            tc_vec_publish();
            tc_store<S::PC>(wr, slabs + buf * S::SLAB, tid);
            tc_load<S::PC, NTPC>(wr, A.wC, 1, tid);
            TC_PIN();
            __syncthreads();
            // (the last two steps store and request the last stage again: a step without a branch keeps the counted
            //  waits, and nobody reads what it leaves)
            auto group = [&](int kg, const f32x4 &xc, f32x4 &xn) __attribute__((always_inline)) {
                const WT *lw = slabs + buf * S::SLAB;
                WT *nw = slabs + (buf ^ 1) * S::SLAB;
                tc_mfma<TPWC>(acc, lw + (half * TPWC) * 64 + lane, xc, true, [&]() __attribute__((always_inline)) {
                    tc_store<S::PC>(wr, nw, tid);
                    xn = *reinterpret_cast<const f32x4 *>(rer + 16 * (kg + 1 < NGE ? kg + 1 : NGE - 1));
                    tc_load<S::PC, NTPC>(wr, A.wC, kg + 2 < NGE ? kg + 2 : NGE - 1, tid);
                });
                TC_PIN();
                buf ^= 1;
                if (kg + 1 < NGE) tc_kgroup_barrier();
            };
            static_assert(NGE % 2 == 0, "k-groups in pairs");
            if constexpr (NGE == 8) {   // (D = 128: unrolled, every wait is counted for its own k-group)
#pragma unroll
                for (int kg = 0; kg < NGE; kg += 2) {
                    group(kg, x0, x1);
                    group(kg + 1, x1, x0);
                }
            } else {
#pragma unroll 1
                for (int kg = 0; kg < NGE; kg += 2) {
                    group(kg, x0, x1);
                    group(kg + 1, x1, x0);
                }
            }
            }   // (!EW)
            const int fbase = 16 * half * TPWC + 4 * q;
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < TPWC; ++c) {
                const f32x4 b = *reinterpret_cast<const f32x4 *>(v_bC + fbase + 16 * c);   // (bC_empty: lite)
                const f32x4 w = *reinterpret_cast<const f32x4 *>(v_wdot + fbase + 16 * c);
#pragma unroll
                for (int r = 0; r < 4; ++r) d = fmaf(fmaxf(acc[c][r] + b[r], 0.f), w[r], d);
            }
            d = lpf_quad_sum(d);
            if (q == 0) my_x[4 * TC_XCH_SLOT] = d;
            __syncthreads();
            if (live && q == 0 && half == 0) {
                d = d + peer_x[4 * TC_XCH_SLOT] + A.bdot[0];
                if (A.sel_ctl && A.sel_ctl[3] != 0) d = __builtin_nanf("");
                if (A.logit) A.logit[m] = d;
                if (A.prob) A.prob[m] = 1.0f / (1.0f + expf(-d));
            }
            TC_STAMP(6);
            TC_STAMPS_OUT(1);
            return;
        }
    }
    if constexpr (!EW) tc_vec_publish();   // (in front of this path's first barrier: stage A's, or stage B's first k-group)
    // ------------------------------------------------------------------ stage A: attention output + post-norm
    f32x4 accA[TPWA];
#pragma unroll
    for (int c = 0; c < TPWA; ++c) accA[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int seg_cnt[3] = {0, 0, 0};
    const bool gemmA = !WB && !ROWS && A.part == nullptr;
    if constexpr (!WB && !ROWS) {
    if (gemmA) {   // (the GEMM form of stage A exists in fp32 only)
        const float *xa = A.x + mm * A.ldx;
        const int ngA = (A.KA + 15) >> 4;
        tc_load<S::PA, NTPA>(wr, A.wA, 0, tid);
        int kk = 4 * q < A.KA ? 4 * q : A.KA - 4;  // clamped into the row; out-of-range groups are zeroed below
        f32x4 xr = *reinterpret_cast<const f32x4 *>(xa + kk);
        tc_store<S::PA>(wr, slabs + buf * S::SLAB, tid);
        if (ngA > 1) tc_load<S::PA, NTPA>(wr, A.wA, 1, tid);
        else tc_load<S::PB, NTPB>(wr, A.wB, 0, tid);
        TC_PIN();
        __syncthreads();
        // (the last two weight steps are stage B's first two; the input group of the next k-group is requested in
        //  front of the step's weights, so its wait leaves them in flight)
        f32x4 x1 = (f32x4){0.f, 0.f, 0.f, 0.f};   // (two registers take turns: see the r_e loops)
        auto group = [&](int kg, const f32x4 &xc, f32x4 &xn) __attribute__((always_inline)) {
            const f32x4 bv = (16 * kg + 4 * q < A.KA) ? xc : (f32x4){0.f, 0.f, 0.f, 0.f};
            const f32x4 *lw = slabs + buf * S::SLAB;
            f32x4 *nw = slabs + (buf ^ 1) * S::SLAB;
            tc_mfma<TPWA>(accA, lw + (half * TPWA) * 64 + lane, bv, true, [&]() __attribute__((always_inline)) {
                if (kg + 1 < ngA) tc_store<S::PA>(wr, nw, tid);
                else tc_store<S::PB>(wr, nw, tid);
                kk = 16 * (kg + 1) + 4 * q;
                kk = kk < A.KA ? kk : A.KA - 4;
                xn = *reinterpret_cast<const f32x4 *>(xa + kk);
                if (kg + 2 < ngA) tc_load<S::PA, NTPA>(wr, A.wA, kg + 2, tid);
                else tc_load<S::PB, NTPB>(wr, A.wB, kg + 2 - ngA, tid);
            });
            TC_PIN();
            buf ^= 1;
            tc_kgroup_barrier();
        };
        int kg = 0;
#pragma unroll 1
        for (; kg + 1 < ngA; kg += 2) {
            group(kg, xr, x1);
            group(kg + 1, x1, xr);
        }
        if (kg < ngA) group(kg, xr, x1);
    }
    }
    // stage B's first weights: behind stage E and behind the GEMM form of stage A the stream has brought them; the
    // other forms request them here, to fly during whatever stage A is, and store them (tc_b_start) where stage A is
    // done -- the second stage then flies during the LayerNorm, or while the rows arrive
    if constexpr (!EW) {
        if (!gemmA) tc_load<S::PB, NTPB>(wr, A.wB, 0, tid);
    }
    auto tc_b_start = [&]() __attribute__((always_inline)) {
        tc_store<S::PB>(wr, slabs + buf * S::SLAB, tid);
        tc_load<S::PB, NTPB>(wr, A.wB, 1, tid);
        TC_PIN();
    };
    if constexpr (ROWS) {
        const int fbase = 16 * half * TPWA + 4 * q;
        if constexpr (!EW) {
            tc_rows_request();
            TC_PIN();
            tc_b_start();   // (waits for the weights alone: the rows stay in flight)
        }
#pragma unroll
        for (int c = 0; c < TPWA; ++c) accA[c] = fbase + 16 * c < A.NA ? rowv[c] : (f32x4){0.f, 0.f, 0.f, 0.f};
    } else if (A.part == nullptr) {
        const int fbase = 16 * half * TPWA + 4 * q;
        f32x4 ad[TPWA];
#pragma unroll
        for (int c = 0; c < TPWA; ++c) {
            const int f0 = fbase + 16 * c;
            ad[c] = *reinterpret_cast<const f32x4 *>(A.addend + mm * A.ldadd + (f0 < A.NA ? f0 : 0));
        }
#pragma unroll
        for (int c = 0; c < TPWA; ++c) accA[c] += (fbase + 16 * c < A.NA) ? ad[c] : (f32x4){0.f, 0.f, 0.f, 0.f};
    } else {
        // Merge of this pair's attention records (online-softmax states {acc, m, l}).  A (pair, type) segment
        // [lo, hi) of the type's entry region that lies inside one 16-entry unit left ONE record in part[t][pair];
        // one that crosses units left a boundary record per unit it touches -- the head in slot 1 of its first unit,
        // then slot 0 of every following unit (pair_fused.hip) -- whose addresses follow from lo and hi alone.
        // All addresses are known before the first record arrives, so the reads go out in batches (the three segment
        // pointers, the three first records, then the remaining boundary records two or four at a time): the record region is
        // hundreds of MB touched sparsely, every read is a long-latency miss, and there are only two wavefronts per
        // SIMD here to hide it.
        const int fbase = 16 * half * TPWA + 4 * q;
        const int64_t rs = A.NA + 4;
        float mx = -INFINITY, den = 0.f;
        f32x4 v[TPWA];
#pragma unroll
        for (int c = 0; c < TPWA; ++c) v[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
        auto fetch = [&](const float *rec, f32x4 &h, f32x4 *b) __attribute__((always_inline)) {
            h = *reinterpret_cast<const f32x4 *>(rec + A.NA);
#pragma unroll
            for (int c = 0; c < TPWA; ++c) {
                const int f0 = fbase + 16 * c;
                b[c] = *reinterpret_cast<const f32x4 *>(rec + (f0 < A.NA ? f0 : 0));
            }
        };
        auto merge = [&](const f32x4 &h, const f32x4 *b) __attribute__((always_inline)) {
            const float mn = fmaxf(mx, h[0]);
            const float sa = __expf(mx - mn), sb = __expf(h[0] - mn);
            den = fmaf(den, sa, h[1] * sb);
#pragma unroll
            for (int c = 0; c < TPWA; ++c) v[c] = v[c] * sa + b[c] * sb;
            mx = mn;
        };
        int lo[3], hi[3], n_p[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int32_t *tp = A.type_ptr + (int64_t)t * (A.M + 1) + mm;
            lo[t] = tp[0];
            hi[t] = tp[1];
        }
        {
            f32x4 h0[3], b0[3][TPWA];
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                seg_cnt[t] = hi[t] - lo[t];
                // (a segment past the region: sel_ctl[3] is set and the row becomes NaN below)
                const bool some = hi[t] > lo[t] && ((hi[t] - 1) >> 4) < A.units_cap;
                n_p[t] = some ? ((hi[t] - 1) >> 4) - (lo[t] >> 4) + 1 : 0;
                const float *rec = n_p[t] > 1 ? A.bnd + ((((int64_t)t * A.units_cap + (lo[t] >> 4)) * 2) + 1) * rs
                                              : A.part + ((int64_t)t * A.M + mm) * rs;
                h0[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < TPWA; ++c) b0[t][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (n_p[t] > 0) fetch(rec, h0[t], b0[t]);  // (most pairs have no entry of some type: nothing to read)
            }
#pragma unroll
            for (int t = 0; t < 3; ++t)
                if (n_p[t] > 0) merge(h0[t], b0[t]);
        }
        const int r0 = n_p[0] > 1 ? n_p[0] - 1 : 0, r1 = n_p[1] > 1 ? n_p[1] - 1 : 0, r2 = n_p[2] > 1 ? n_p[2] - 1 : 0;
        const int n_rest = r0 + r1 + r2;
        constexpr int NB = TPWA >= 4 ? 2 : 4;  // (registers: the kernel is held to 128)
#pragma unroll 1
        for (int k0 = 0; k0 < n_rest; k0 += NB) {
            f32x4 hh[NB], bb[NB][TPWA];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int k = k0 + i < n_rest ? k0 + i : n_rest - 1;
                const int t = k < r0 ? 0 : (k < r0 + r1 ? 1 : 2);
                const int jj = k - (t == 0 ? 0 : (t == 1 ? r0 : r0 + r1));
                const int ut = t == 0 ? lo[0] >> 4 : (t == 1 ? lo[1] >> 4 : lo[2] >> 4);
                fetch(A.bnd + (((int64_t)t * A.units_cap + ut + 1 + jj) * 2) * rs, hh[i], bb[i]);
            }
#pragma unroll
            for (int i = 0; i < NB; ++i)
                if (k0 + i < n_rest) merge(hh[i], bb[i]);
        }
        const float inv = 1.0f / (den + 1e-16f);
#pragma unroll
        for (int c = 0; c < TPWA; ++c) {
            const int f0 = fbase + 16 * c;
            if (f0 < A.NA) accA[c] = v[c] * inv + *reinterpret_cast<const f32x4 *>(A.att_bias + f0);
        }
    }
    {
        const int fbase = 16 * half * TPWA + 4 * q;
        if constexpr (!ROWS) {
            if (!gemmA) tc_b_start();
            tc_layernorm<TPWA>(accA, fbase, A.NA, A.lnA_g, A.lnA_b, half, q, my_x, peer_x, false);
        }
#pragma unroll
        for (int c = 0; c < TPWA; ++c) my_hid[(half * TPWA + c) * 64] = accA[c];
    }

    TC_STAMP(1);
    // ------------------------------------------------------------------ stage B: first layer of pairwise_lin
    f32x4 accB[TPWB];
#pragma unroll
    for (int c = 0; c < TPWB; ++c) accB[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float *rer = EW ? nullptr : A.re + mm * A.ldre + 4 * q;
    f32x4 xr = (f32x4){0.f, 0.f, 0.f, 0.f};     // stage C's input group (the form that reads r_e), one k-group ahead
    {
        // the appended k-group: the count features (4 floats per sample) in lane quarter 0, zeros elsewhere
        f32x4 tailv = (f32x4){0.f, 0.f, 0.f, 0.f};
        if constexpr (ROWS) {
            if (q == 0 && !no_sel) tailv = rowt;
        } else if (q == 0) {
            if (A.part == nullptr) {
                tailv = *reinterpret_cast<const f32x4 *>(A.tail + mm * A.ldtail);
            } else {  // get_structure_cnts (link_transformer.py:340-356): n_cn, n_1hop, [n_non1hop,] n_cn + n_1hop
                const float n0 = (float)seg_cnt[0], n1 = (float)seg_cnt[1], n2 = (float)seg_cnt[2];
                tailv = A.n_counts == 4 ? (f32x4){n0, n1, n2, n0 + n1}
                                         : (A.n_counts == 3 ? (f32x4){n0, n1, n0 + n1, 0.f} : (f32x4){n0, 0.f, 0.f, 0.f});
            }
        }
        constexpr int NKB = NTPA + 1;   // stage B's k-groups
        constexpr int C0 = EW ? NGE : 0;   // (stage E form: C's r_e k-groups are done, the r_p groups follow)
        static_assert(NKB >= 2 && NTB >= 2, "a stage's last two weight steps are the next stage's first two");
        __syncthreads();  // publishes stage A's hidden tiles and stage B's first weights
        // (the last two weight steps are stage C's first two)
        tc_each<NKB>([&](auto KG) __attribute__((always_inline)) {
            constexpr int kg = decltype(KG)::value;
            const WT *lw = slabs + buf * S::SLAB;
            WT *nw = slabs + (buf ^ 1) * S::SLAB;
            const f32x4 bv = kg < NTPA ? my_hid[(kg < NTPA ? kg : 0) * 64] : tailv;
            // (NTB odd: tile NTPB - 1, the second wave's last one, is padding -- its accumulators stay 0)
            tc_mfma<TPWB>(accB, lw + (half * TPWB) * 64 + lane, bv, !((NTB & 1) && half == 1),
                          [&]() __attribute__((always_inline)) {
                if constexpr (kg + 1 < NKB) tc_store<S::PB>(wr, nw, tid);
                else tc_store<S::PC>(wr, nw, tid);
                if constexpr (kg + 2 < NKB) tc_load<S::PB, NTPB>(wr, A.wB, kg + 2, tid);
                else {
                    if constexpr (kg + 2 == NKB) tc_load<S::PC, NTPC>(wr, A.wC, C0, tid);
                    else tc_load<S::PC, NTPC>(wr, A.wC, C0 + 1, tid);
                }
            });
            TC_PIN();
            buf ^= 1;
            if constexpr (kg + 1 < NKB) tc_kgroup_barrier();   // (behind the last k-group the LayerNorm's barriers follow)
        });
    }
    TC_STAMP(2);
    if constexpr (!EW) xr = *reinterpret_cast<const f32x4 *>(rer);  // stage C's first input group
    {
        const int fbase = 16 * half * TPWB + 4 * q;
#pragma unroll
        for (int c = 0; c < TPWB; ++c) accB[c] += *reinterpret_cast<const f32x4 *>(v_bB + fbase + 16 * c);
        tc_layernorm<TPWB>(accB, fbase, A.NB, v_lnB_g, v_lnB_b, half, q, my_x + 2 * TC_XCH_SLOT, peer_x + 2 * TC_XCH_SLOT, true);
        // (the barriers inside the LayerNorm exchange come after every wave's last read of stage A's tiles)
#pragma unroll
        for (int c = 0; c < TPWB; ++c) my_hid[(half * TPWB + c) * 64] = accB[c];
    }

    TC_STAMP(3);
    // ------------------------------------------------------------------ stage C: folded score head
    __syncthreads();  // publishes stage B's hidden tiles and the weight stage stored under stage B's last k-group
    if constexpr (!EW) {
#pragma unroll
    for (int c = 0; c < TPWC; ++c) accC[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // r_e, read from global memory one k-group ahead, in front of the step's weights; two registers take turns.
    // (What was requested in front of the LayerNorm has long arrived: said once here, the waits of a loop that stays
    //  rolled are counted for what the loop itself requests -- not for everything, as its entry would have it.)
    __builtin_amdgcn_s_waitcnt(0x0f70);
    f32x4 x1 = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto group = [&](int kg, const f32x4 &xc, f32x4 &xn) __attribute__((always_inline)) {
        const WT *lw = slabs + buf * S::SLAB;
        WT *nw = slabs + (buf ^ 1) * S::SLAB;
        tc_mfma<TPWC>(accC, lw + (half * TPWC) * 64 + lane, xc, true, [&]() __attribute__((always_inline)) {
            tc_store<S::PC>(wr, nw, tid);
            xn = *reinterpret_cast<const f32x4 *>(rer + 16 * (kg + 1 < NGE ? kg + 1 : NGE - 1));
            tc_load<S::PC, NTPC>(wr, A.wC, kg + 2, tid);  // (stages NGE and NGE + 1 exist: the r_p groups follow)
        });
        TC_PIN();
        buf ^= 1;
        tc_kgroup_barrier();
    };
    static_assert(NGE % 2 == 0, "k-groups in pairs");
    if constexpr (NGE == 8) {   // (D = 128: unrolled, every wait is counted for its own k-group)
#pragma unroll
        for (int kg = 0; kg < NGE; kg += 2) {
            group(kg, xr, x1);
            group(kg + 1, x1, xr);
        }
    } else {
#pragma unroll 1
        for (int kg = 0; kg < NGE; kg += 2) {
            group(kg, xr, x1);
            group(kg + 1, x1, xr);
        }
    }
    TC_STAMP(4);
    }
    // r_p, straight from LDS (its padding tile, all zeros, is no k-group worth running)
    tc_each<NTB>([&](auto KG) __attribute__((always_inline)) {
        constexpr int kg = decltype(KG)::value;
        const WT *lw = slabs + buf * S::SLAB;
        WT *nw = slabs + (buf ^ 1) * S::SLAB;
        tc_mfma<TPWC>(accC, lw + (half * TPWC) * 64 + lane, my_hid[kg * 64], true, [&]() __attribute__((always_inline)) {
            if constexpr (kg + 1 < NTB) tc_store<S::PC>(wr, nw, tid);
            if constexpr (kg + 2 < NTB) tc_load<S::PC, NTPC>(wr, A.wC, NGE + kg + 2, tid);
        });
        TC_PIN();
        buf ^= 1;
        if constexpr (kg + 1 < NTB) tc_kgroup_barrier();
    });
    TC_STAMP(5);
    {
        const int fbase = 16 * half * TPWC + 4 * q;
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < TPWC; ++c) {
            const f32x4 b = *reinterpret_cast<const f32x4 *>(v_bC + fbase + 16 * c);
            const f32x4 w = *reinterpret_cast<const f32x4 *>(v_wdot + fbase + 16 * c);  // zero-padded
#pragma unroll
            for (int r = 0; r < 4; ++r) d = fmaf(fmaxf(accC[c][r] + b[r], 0.f), w[r], d);
        }
        d = lpf_quad_sum(d);
        if (q == 0) my_x[4 * TC_XCH_SLOT] = d;
        __syncthreads();
        if (live && q == 0 && half == 0) {
            d = d + peer_x[4 * TC_XCH_SLOT] + A.bdot[0];
            if (A.sel_ctl && A.sel_ctl[3] != 0) d = __builtin_nanf("");  // the batch did not fit the selection workspace
            if (A.logit) A.logit[m] = d;
            if (A.prob) A.prob[m] = 1.0f / (1.0f + expf(-d));
        }
    }
    TC_STAMP(6);
    TC_STAMPS_OUT(0);
}

template <int NTA, int NTB, int NTC, int WM = 0, bool ROWS = false, bool EW = false>
int tc_launch(const TailArgs &a, hipStream_t s) {
    constexpr size_t lds = TcShape<NTA, NTB, NTC>::BYTES;
    auto kern = tail_chain_kernel<NTA, NTB, NTC, WM, ROWS, EW>;
    LPF_SET_MAX_LDS(kern, lds);  // (per instantiation and device; the attribute is sticky)
    const int64_t blocks = (a.M + 16 * TC_GROUPS - 1) / (16 * TC_GROUPS);
    if (blocks > 0x7fffffff) return LPF_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(TC_THREADS), lds, s, a);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}

}  // namespace

#ifdef TC_STAMPS
extern "C" int lpf_tail_chain_set_stamps(void *buf) {
    return hipMemcpyToSymbol(HIP_SYMBOL(tc_stamp_buf), &buf, sizeof(buf)) == hipSuccess ? LPF_OK : LPF_ERR_LAUNCH;
}
#endif


extern "C" int lpf_tail_chain_f32(int64_t M, int32_t D, int32_t n_counts, const float *G, int64_t ldg,
                                  const float *wA_packed, const float *lnA_g, const float *lnA_b, const float *counts,
                                  int64_t ldc, const float *wB_packed, const float *bB, const float *lnB_g,
                                  const float *lnB_b, const float *r_e, int64_t ldre, const float *wC_packed,
                                  const float *bC, const float *w_dot, const float *b_dot, float *logit, float *prob,
                                  void *stream) {
    if (M == 0) return LPF_OK;
    LPF_REQUIRE(M > 0 && G && wA_packed && lnA_g && lnA_b && counts && wB_packed && bB && lnB_g && lnB_b && r_e &&
                wC_packed && bC && w_dot && b_dot && (logit || prob));
    LPF_REQUIRE(n_counts >= 1 && n_counts <= 4 && (ldg & 3) == 0 && ldg >= 4 * D + 4 && (ldc & 3) == 0 && ldc >= 4 &&
                (ldre & 3) == 0 && ldre >= D);
    LPF_REQUIRE(lpf_aligned16(G) && lpf_aligned16(counts) && lpf_aligned16(r_e) && lpf_aligned16(wA_packed) &&
                lpf_aligned16(wB_packed) && lpf_aligned16(wC_packed) && lpf_aligned16(lnA_g) && lpf_aligned16(lnA_b) &&
                lpf_aligned16(bB) && lpf_aligned16(lnB_g) && lpf_aligned16(lnB_b) && lpf_aligned16(bC) &&
                lpf_aligned16(w_dot));
    TailArgs a{M, G + D, ldg, 3 * D + 4, G, ldg, wA_packed, lnA_g, lnA_b, D, counts, ldc, wB_packed, bB, lnB_g,
               lnB_b, D + n_counts, r_e, ldre, wC_packed, bC, 2 * D, w_dot, b_dot, logit, prob,
               nullptr, nullptr, 0, nullptr, nullptr, nullptr, n_counts, nullptr, 0, nullptr, nullptr, nullptr, nullptr};
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (D) {
        case 32: return tc_launch<2, 3, 4>(a, s);
        case 64: return tc_launch<4, 5, 8>(a, s);
        case 128: return tc_launch<8, 9, 16>(a, s);
        default: return LPF_ERR_UNSUPPORTED;  // D = 256: 32-tile score head, the per-layer chains are used instead
    }
}

extern "C" int lpf_tail_chain_merge_f32(int64_t M, int32_t D, int32_t n_counts, const float *part, const float *bnd,
                                        int64_t units_cap, const int32_t *type_ptr, const float *att_bias, const float *lnA_g,
                                        const float *lnA_b, const float *wB_packed, const float *bB, const float *lnB_g,
                                        const float *lnB_b, const float *r_e, int64_t ldre, const float *wC_packed,
                                        const float *bC, const float *w_dot, const float *b_dot,
                                        const int64_t *sel_ctl, float *logit, float *prob, void *stream) {
    if (M == 0) return LPF_OK;
    LPF_REQUIRE(M > 0 && part && bnd && units_cap > 0 && lpf_aligned16(bnd) && type_ptr && att_bias && lnA_g && lnA_b && wB_packed && bB && lnB_g && lnB_b && r_e &&
                wC_packed && bC && w_dot && b_dot && (logit || prob));
    LPF_REQUIRE((n_counts == 1 || n_counts == 3 || n_counts == 4) && (ldre & 3) == 0 && ldre >= D);
    LPF_REQUIRE(lpf_aligned16(part) && lpf_aligned16(att_bias) && lpf_aligned16(r_e) && lpf_aligned16(wB_packed) &&
                lpf_aligned16(wC_packed) && lpf_aligned16(lnA_g) && lpf_aligned16(lnA_b) && lpf_aligned16(bB) &&
                lpf_aligned16(lnB_g) && lpf_aligned16(lnB_b) && lpf_aligned16(bC) && lpf_aligned16(w_dot));
    TailArgs a{M, nullptr, 0, 0, nullptr, 0, nullptr, lnA_g, lnA_b, D, nullptr, 0, wB_packed, bB, lnB_g,
               lnB_b, D + n_counts, r_e, ldre, wC_packed, bC, 2 * D, w_dot, b_dot, logit, prob,
               part, bnd, units_cap, type_ptr, att_bias, sel_ctl, n_counts, nullptr, 0, nullptr, nullptr, nullptr, nullptr};
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (D) {
        case 32: return tc_launch<2, 3, 4>(a, s);
        case 64: return tc_launch<4, 5, 8>(a, s);
        case 128: return tc_launch<8, 9, 16>(a, s);
        default: return LPF_ERR_UNSUPPORTED;
    }
}

extern "C" int lpf_tail_chain_merge_bf16(int64_t M, int32_t D, int32_t n_counts, const float *part, const float *bnd,
                                         int64_t units_cap, const int32_t *type_ptr, const float *att_bias,
                                         const float *lnA_g, const float *lnA_b, const void *wB_packed_bf16,
                                         const float *bB, const float *lnB_g, const float *lnB_b, const float *r_e,
                                         int64_t ldre, const void *wC_packed_bf16, const float *bC, const float *w_dot,
                                         const float *b_dot, const int64_t *sel_ctl, float *logit, float *prob,
                                         void *stream) {
    if (M == 0) return LPF_OK;
    LPF_REQUIRE(M > 0 && part && bnd && units_cap > 0 && lpf_aligned16(bnd) && type_ptr && att_bias && lnA_g && lnA_b &&
                wB_packed_bf16 && bB && lnB_g && lnB_b && r_e && wC_packed_bf16 && bC && w_dot && b_dot &&
                (logit || prob));
    LPF_REQUIRE((n_counts == 1 || n_counts == 3 || n_counts == 4) && (ldre & 3) == 0 && ldre >= D);
    LPF_REQUIRE(lpf_aligned16(part) && lpf_aligned16(att_bias) && lpf_aligned16(r_e) && lpf_aligned16(wB_packed_bf16) &&
                lpf_aligned16(wC_packed_bf16) && lpf_aligned16(lnA_g) && lpf_aligned16(lnA_b) && lpf_aligned16(bB) &&
                lpf_aligned16(lnB_g) && lpf_aligned16(lnB_b) && lpf_aligned16(bC) && lpf_aligned16(w_dot));
    TailArgs a{M, nullptr, 0, 0, nullptr, 0, nullptr, lnA_g, lnA_b, D, nullptr, 0,
               static_cast<const float *>(wB_packed_bf16), bB, lnB_g, lnB_b, D + n_counts, r_e, ldre,
               static_cast<const float *>(wC_packed_bf16), bC, 2 * D, w_dot, b_dot, logit, prob,
               part, bnd, units_cap, type_ptr, att_bias, sel_ctl, n_counts, nullptr, 0, nullptr, nullptr, nullptr, nullptr};
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (D) {
        case 32: return tc_launch<2, 3, 4, 1>(a, s);
        case 64: return tc_launch<4, 5, 8, 1>(a, s);
        case 128: return tc_launch<8, 9, 16, 1>(a, s);
        default: return LPF_ERR_UNSUPPORTED;
    }
}

// Rows mode: stage A was done by lpf_pair_attention_rows_* (one finished row per pair: post_att_norm(attention output)
// followed by the count features, zero padded to 4); the tail is the two GEMMs, their LayerNorm and the score.
namespace {
template <int WM>
int tc_rows(int64_t M, int32_t D, int32_t n_counts, const float *rows, int64_t ldrows, const void *wB, const float *bB,
            const float *lnB_g, const float *lnB_b, const float *r_e, int64_t ldre, const void *wC, const float *bC,
            const float *w_dot, const float *b_dot, const int64_t *sel_ctl, float *logit, float *prob, void *stream,
            const int32_t *perm = nullptr, const int64_t *n_full = nullptr, const float *bC_empty = nullptr,
            const float *row_empty = nullptr) {
    if (M == 0) return LPF_OK;
    LPF_REQUIRE(!perm || (n_full && bC_empty && lpf_aligned16(bC_empty)));
    LPF_REQUIRE(!row_empty || (perm && lpf_aligned16(row_empty)));
    LPF_REQUIRE(M > 0 && rows && wB && bB && lnB_g && lnB_b && r_e && wC && bC && w_dot && b_dot && (logit || prob));
    LPF_REQUIRE((n_counts == 1 || n_counts == 3 || n_counts == 4) && (ldre & 3) == 0 && ldre >= D && (ldrows & 3) == 0 &&
                ldrows >= D + 4);
    LPF_REQUIRE(lpf_aligned16(rows) && lpf_aligned16(r_e) && lpf_aligned16(wB) && lpf_aligned16(wC) && lpf_aligned16(bB) &&
                lpf_aligned16(lnB_g) && lpf_aligned16(lnB_b) && lpf_aligned16(bC) && lpf_aligned16(w_dot));
    TailArgs a{M, nullptr, 0, 0, nullptr, 0, nullptr, nullptr, nullptr, D, nullptr, 0, static_cast<const float *>(wB), bB,
               lnB_g, lnB_b, D + n_counts, r_e, ldre, static_cast<const float *>(wC), bC, 2 * D, w_dot, b_dot, logit, prob,
               nullptr, nullptr, 0, nullptr, nullptr, sel_ctl, n_counts, rows, ldrows, perm, n_full, bC_empty, row_empty};
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (D) {
        case 32: return tc_launch<2, 3, 4, WM, true>(a, s);
        case 64: return tc_launch<4, 5, 8, WM, true>(a, s);
        case 128: return tc_launch<8, 9, 16, WM, true>(a, s);
        case 256: return tc_launch<16, 17, 32, WM, true>(a, s);
        default: return LPF_ERR_UNSUPPORTED;
    }
}
}  // namespace

extern "C" int lpf_tail_chain_rows_f32(int64_t M, int32_t D, int32_t n_counts, const float *rows, int64_t ldrows,
                                       const float *wB_packed, const float *bB, const float *lnB_g, const float *lnB_b,
                                       const float *r_e, int64_t ldre, const float *wC_packed, const float *bC,
                                       const float *w_dot, const float *b_dot, const int64_t *sel_ctl, float *logit,
                                       float *prob, void *stream) {
    return tc_rows<0>(M, D, n_counts, rows, ldrows, wB_packed, bB, lnB_g, lnB_b, r_e, ldre, wC_packed, bC, w_dot, b_dot,
                          sel_ctl, logit, prob, stream);
}

extern "C" int lpf_tail_chain_rows_bf16(int64_t M, int32_t D, int32_t n_counts, const float *rows, int64_t ldrows,
                                        const void *wB_packed_bf16, const float *bB, const float *lnB_g, const float *lnB_b,
                                        const float *r_e, int64_t ldre, const void *wC_packed_bf16, const float *bC,
                                        const float *w_dot, const float *b_dot, const int64_t *sel_ctl, float *logit,
                                        float *prob, void *stream) {
    return tc_rows<1>(M, D, n_counts, rows, ldrows, wB_packed_bf16, bB, lnB_g, lnB_b, r_e, ldre, wC_packed_bf16, bC, w_dot,
                         b_dot, sel_ctl, logit, prob, stream);
}

/* lpf_tail_chain_rows_* taking the pairs in the order lpf_pair_attention_rows_perm_* left: perm int32[M], *n_full = how
 * many of them (the first ones) have selected nodes.  Workgroups whose 64 pairs all lie behind *n_full compute
 * score = w_dot . ReLU(A_e r_e + bC_empty) + b_dot only -- bC_empty [2D] = bC + A_p r_p0 with r_p0 the (constant) hidden
 * activation of pairwise_lin for a pair without selected nodes (lpformer_amd/fold.py empty_pair_head_bias). */
extern "C" int lpf_tail_chain_rows_perm_f32(int64_t M, int32_t D, int32_t n_counts, const float *rows, int64_t ldrows,
                                            const float *wB_packed, const float *bB, const float *lnB_g,
                                            const float *lnB_b, const float *r_e, int64_t ldre, const float *wC_packed,
                                            const float *bC, const float *w_dot, const float *b_dot,
                                            const int64_t *sel_ctl, const int32_t *perm, const int64_t *n_full,
                                            const float *bC_empty, const float *row_empty, float *logit, float *prob,
                                            void *stream) {
    LPF_REQUIRE(perm && n_full && bC_empty);
    return tc_rows<0>(M, D, n_counts, rows, ldrows, wB_packed, bB, lnB_g, lnB_b, r_e, ldre, wC_packed, bC, w_dot, b_dot,
                          sel_ctl, logit, prob, stream, perm, n_full, bC_empty, row_empty);
}

extern "C" int lpf_tail_chain_rows_perm_bf16(int64_t M, int32_t D, int32_t n_counts, const float *rows, int64_t ldrows,
                                             const void *wB_packed_bf16, const float *bB, const float *lnB_g,
                                             const float *lnB_b, const float *r_e, int64_t ldre,
                                             const void *wC_packed_bf16, const float *bC, const float *w_dot,
                                             const float *b_dot, const int64_t *sel_ctl, const int32_t *perm,
                                             const int64_t *n_full, const float *bC_empty, const float *row_empty,
                                             float *logit, float *prob, void *stream) {
    LPF_REQUIRE(perm && n_full && bC_empty);
    return tc_rows<1>(M, D, n_counts, rows, ldrows, wB_packed_bf16, bB, lnB_g, lnB_b, r_e, ldre, wC_packed_bf16, bC, w_dot,
                         b_dot, sel_ctl, logit, prob, stream, perm, n_full, bC_empty, row_empty);
}

/* lpf_tail_chain_rows_perm_f32 with stage E in front (the header has the contract): r_e is computed by the tail's own
 * workgroups from the node table instead of being read. */
extern "C" int lpf_tail_chain_rows_perm_ew_f32(int64_t M, int32_t D, int32_t n_counts, const float *rows, int64_t ldrows,
                                               const float *wB_packed, const float *bB, const float *lnB_g,
                                               const float *lnB_b, const float *r_e, int64_t ldre, const float *wC_packed,
                                               const float *bC, const float *w_dot, const float *b_dot,
                                               const int64_t *sel_ctl, const int32_t *perm, const int64_t *n_full,
                                               const float *bC_empty, const float *row_empty, const float *X, int64_t ldx,
                                               const int64_t *batch, int64_t batch_ld, int64_t n_rows,
                                               const float *wE_packed, const float *bE, const float *lnE_g,
                                               const float *lnE_b, float *logit, float *prob, void *stream) {
    if (!wE_packed)
        return lpf_tail_chain_rows_perm_f32(M, D, n_counts, rows, ldrows, wB_packed, bB, lnB_g, lnB_b, r_e, ldre, wC_packed, bC,
                                            w_dot, b_dot, sel_ctl, perm, n_full, bC_empty, row_empty, logit, prob, stream);
    if (M == 0) return LPF_OK;
    if (D != 128) return LPF_ERR_UNSUPPORTED;
    LPF_REQUIRE(perm && n_full && bC_empty && lpf_aligned16(bC_empty) && (!row_empty || lpf_aligned16(row_empty)));
    LPF_REQUIRE(M > 0 && rows && wB_packed && bB && lnB_g && lnB_b && wC_packed && bC && w_dot && b_dot && (logit || prob));
    LPF_REQUIRE((n_counts == 1 || n_counts == 3 || n_counts == 4) && (ldrows & 3) == 0 && ldrows >= D + 4);
    LPF_REQUIRE(X && batch && bE && lnE_g && lnE_b && n_rows > 0 && batch_ld >= M && (ldx & 3) == 0 && ldx >= D);
    LPF_REQUIRE(lpf_aligned16(rows) && lpf_aligned16(wB_packed) && lpf_aligned16(wC_packed) && lpf_aligned16(bB) &&
                lpf_aligned16(lnB_g) && lpf_aligned16(lnB_b) && lpf_aligned16(bC) && lpf_aligned16(w_dot) &&
                lpf_aligned16(X) && lpf_aligned16(wE_packed) && lpf_aligned16(bE) && lpf_aligned16(lnE_g) &&
                lpf_aligned16(lnE_b));
    TailArgs a{M, nullptr, 0, 0, nullptr, 0, nullptr, nullptr, nullptr, D, nullptr, 0, wB_packed, bB,
               lnB_g, lnB_b, D + n_counts, nullptr, 0, wC_packed, bC, 2 * D, w_dot, b_dot, logit, prob,
               nullptr, nullptr, 0, nullptr, nullptr, sel_ctl, n_counts, rows, ldrows, perm, n_full, bC_empty, row_empty,
               X, ldx, batch, batch_ld, n_rows, wE_packed, bE, lnE_g, lnE_b};
    return tc_launch<8, 9, 16, 0, true, true>(a, static_cast<hipStream_t>(stream));
}
