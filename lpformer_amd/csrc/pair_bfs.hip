// Shortest-path hops per pair on the typing adjacency (the "shortest path" baseline of HeaRT / OGB link prediction and
// the axis "how far apart are the endpoints" of the binned analyses): for each pair (a, b) of a binary CSR with sorted,
// unique int32 columns and a SYMMETRIC pattern (values ignored; a non-symmetric pattern is outside the contract: the
// two sides of the search would walk different graphs)
//   dist[p] = 0 when a == b;  -1 when an id lies outside [0, n);  else the number of edges of a shortest a-b path,
//             -1 when there is none;  with ignore_direct the stored entries (a, b) and (b, a) of THIS pair are absent;
//             with max_dist = m > 0 a distance above m reads -1.  Stored self-loops change nothing.
//
// Two classes of work; nothing is read back to the host between them.
//   * Front kernel, one lane per pair: everything that needs no search -- a == b, bad ids, an endpoint without a usable
//     entry (degree 0, or 0 once the direct entry is ignored), distance 1 (binary search of b in row a and of a in row
//     b), the max_dist = 1 cut-off, and distance 2 when the shorter row (equal lengths: the row of min(a, b)) holds at
//     most split_threshold entries: its columns other than a and b are probed in the other row, stopping at the first
//     hit; no hit and max_dist = 2 is -1.  Every other pair is appended to a list by ballot rank (one int32 ticket
//     per wave).
//   * Search kernel, persistent 256-thread workgroups: a workgroup takes listed pairs by counting the list's own counter
//     down (an atomic ticket: the searches differ by orders of magnitude in length, a fixed stride would leave
//     workgroups idle) and runs a bidirectional level-synchronous BFS per pair.  Per workgroup, in the caller's
//     workspace: a dense stamp array of n 32-bit words -- a word holds (epoch << 1 | side); the epoch grows by one per
//     pair, so nothing is cleared between pairs; the entry point zeroes the array once per call -- and one visit list of
//     n + 2 int32: side a's visited nodes grow from the front, side b's from the back; the two sets are disjoint until
//     the search ends, so together they never exceed the list.  A side's frontier is the last slice it appended.
//     Each round expands, over one COMPLETE level, the side whose frontier has the smaller sum of degrees.  The
//     frontier's rows are flattened into one stream of slots, 256 frontier nodes at a time (an inclusive scan of their
//     degrees over the workgroup, kept in LDS: 4 KiB per workgroup, so the registers -- 7 workgroups per CU -- and not
//     LDS set the occupancy; what a search waits for is the latency of its scattered stamp words), 256 slots per step,
//     one column per thread: a hub row of hundreds of entries is spread over the whole workgroup.  A column is claimed
//     by an integer compare-and-swap on its stamp word; the claimed columns of a step are appended by ballot rank plus
//     one LDS counter add per wave, their degrees summed the same way.  The plain loads of stamp words and list entries
//     that follow another wave's stores rely on the four waves of a workgroup sharing one CU's vector L1 (workgroups
//     are not split over CUs: the default, non-tgsplit mode), as the dense state of twohop.hip does; a stale stamp load
//     could in any case only show an old epoch, which the compare-and-swap then corrects.
//
// Why the first contact is decisive.  Invariant: side a holds exactly the nodes within dA hops of a, side b those within
// dB hops of b, and the sets are disjoint -- so dist >= dA + dB + 1.  When expanding side S from depth dS, let c be a
// neighbour of a frontier node u (depth dS on S) that the other side T already holds, at depth k <= dT.  Were k < dT, u
// would lie within k + 1 <= dT hops of T's endpoint and, the levels being complete, T would hold u: but S holds u and
// the sets are disjoint.  So k = dT, the path through u and c has dS + 1 + dT edges, which is the lower bound: the kernel
// stops at the first contact it sees.  The same bound gives the cut-off: dA + dB + 1 > max_dist means dist > max_dist,
// and an empty frontier means the component of that side is exhausted: both end with -1.
//
// Deterministic: a stamp word changes once per epoch (old epoch -> this side), so whichever lane wins a claim, the set a
// level claims, the levels, and hence the distance depend on (graph, pair, options) alone -- not on the position in the
// batch, (a, b) versus (b, a), the threshold, the number of workgroups or timing (only the ORDER inside a frontier
// slice varies).  Integer arithmetic only: no floats, no float atomics.
#include "lpf_common.h"

namespace {

constexpr int BFS_BLOCK = 256;                  // 4 wavefronts
constexpr int BFS_WAVES = BFS_BLOCK / LPF_WAVE;

struct BfsArgs {
    int64_t P, n;
    const int64_t *pairs;
    int64_t ld;
    const int64_t *rowptr;
    const int32_t *col;
    int32_t max_dist;                           // 0: unlimited
    int32_t ignore_direct;
    int32_t thr;
    int32_t *list;                              // [0]: counter, [1 ..]: listed pairs
    uint32_t *stamps;                           // [n_groups][n]
    int32_t *visits;                            // [n_groups][n + 2]
    int32_t *dist;
};

__global__ __launch_bounds__(BFS_BLOCK) void bfs_front_kernel(BfsArgs A) {
    const int64_t p = (int64_t)blockIdx.x * BFS_BLOCK + threadIdx.x;
    const int32_t *__restrict__ col = A.col;
    int32_t d = -1;
    bool listed = false;
    if (p < A.P) {
        const int64_t a = A.pairs[p], b = A.pairs[A.ld + p];
        if (a == b) {
            d = 0;
        } else if ((uint64_t)a < (uint64_t)A.n && (uint64_t)b < (uint64_t)A.n) {
            const int64_t a0 = A.rowptr[a], a1 = A.rowptr[a + 1], b0 = A.rowptr[b], b1 = A.rowptr[b + 1];
            const bool e_ab = lpf_sorted_has(col, a0, a1, (int32_t)b), e_ba = lpf_sorted_has(col, b0, b1, (int32_t)a);
            const int64_t da = a1 - a0 - (A.ignore_direct && e_ab ? 1 : 0);
            const int64_t db = b1 - b0 - (A.ignore_direct && e_ba ? 1 : 0);
            if (da <= 0 || db <= 0) {
                d = -1;
            } else if (!A.ignore_direct && (e_ab || e_ba)) {
                d = 1;
            } else if (A.max_dist == 1) {
                d = -1;
            } else {
                const bool walk_a = a1 - a0 < b1 - b0 || (a1 - a0 == b1 - b0 && a < b);
                const int64_t w0 = walk_a ? a0 : b0, w1 = walk_a ? a1 : b1, q0 = walk_a ? b0 : a0, q1 = walk_a ? b1 : a1;
                if (w1 - w0 > (int64_t)A.thr) {
                    listed = true;
                } else {
                    bool hit = false;
                    for (int64_t j = w0; j < w1 && !hit; ++j) {
                        const int32_t w = col[j];     // (a column equal to a or b is a self-loop or the direct entry)
                        hit = w != (int32_t)a && w != (int32_t)b && lpf_sorted_has(col, q0, q1, w);
                    }
                    if (hit) d = 2;
                    else if (A.max_dist == 2) d = -1;
                    else listed = true;
                }
            }
        }
    }
    lpf_wave_list_push(A.list, listed, (int32_t)p);
    if (p < A.P && !listed) A.dist[p] = d;
}

__global__ __launch_bounds__(BFS_BLOCK) void bfs_search_kernel(BfsArgs A) {
    __shared__ int64_t s_incl[BFS_BLOCK];       // inclusive scan of the chunk's degrees
    __shared__ int64_t s_row[BFS_BLOCK];        // first entry of the chunk's rows
    __shared__ int64_t s_wave[BFS_WAVES];
    __shared__ unsigned long long s_deg;        // sum of the degrees of the round's claimed nodes
    __shared__ int32_t s_cnt, s_found, s_ticket;
    const int tid = threadIdx.x, lane = lpf_lane(), wave = tid >> 6;
    const int64_t n = A.n;
    const int64_t *__restrict__ rowptr = A.rowptr;
    const int32_t *__restrict__ col = A.col;
    uint32_t *stamp = A.stamps + (int64_t)blockIdx.x * n;
    int32_t *vis = A.visits + (int64_t)blockIdx.x * (n + 2);
    uint32_t epoch = 0;                           // the stamps are zeroed before the launch
    for (;;) {
        if (tid == 0) s_ticket = atomicSub(&A.list[0], 1) - 1;   // the list is taken from its end
        __syncthreads();
        const int32_t ticket = s_ticket;
        if (ticket < 0) break;                    // block-uniform
        ++epoch;                                  // (at most P < 2^31 - 1 pairs: epoch << 1 fits)
        const int64_t p = A.list[1 + ticket];
        const int64_t a = A.pairs[p], b = A.pairs[A.ld + p];
        // side a: visited = vis[0, a_end), frontier = vis[a_lo, a_end);  side b: vis[b_lo, n + 2), frontier [b_lo, b_hi)
        int64_t a_lo = 0, a_end = 1, b_lo = n + 1, b_hi = n + 2;
        int32_t depth_a = 0, depth_b = 0;
        unsigned long long deg_a = (unsigned long long)(rowptr[a + 1] - rowptr[a]);
        unsigned long long deg_b = (unsigned long long)(rowptr[b + 1] - rowptr[b]);
        if (tid == 0) {
            vis[0] = (int32_t)a;
            vis[n + 1] = (int32_t)b;
            stamp[a] = epoch << 1;
            stamp[b] = (epoch << 1) | 1u;
        }
        int32_t result = -1;
        for (;;) {
            const bool side_b = deg_b < deg_a;
            const int64_t f_lo = side_b ? b_lo : a_lo, f_hi = side_b ? b_hi : a_end;
            if (f_hi == f_lo) break;              // this side's component is exhausted
            if (A.max_dist > 0 && depth_a + depth_b + 1 > A.max_dist) break;
            if (tid == 0) {
                s_cnt = 0;
                s_deg = 0ull;
                s_found = 0;
            }
            __syncthreads();                      // also: the previous round's stamps and list entries are visible
            const uint32_t mine = (epoch << 1) | (side_b ? 1u : 0u);
            // ignore_direct: the entry of the other endpoint in the row of this side's endpoint (depth 0 only)
            const int32_t skip = (A.ignore_direct && (side_b ? depth_b : depth_a) == 0) ? (int32_t)(side_b ? a : b) : -1;
            for (int64_t c0 = f_lo; c0 < f_hi; c0 += BFS_BLOCK) {   // block-uniform
                int64_t deg = 0, r0 = 0;
                if (c0 + tid < f_hi) {
                    const int64_t u = vis[c0 + tid];
                    r0 = rowptr[u];
                    deg = rowptr[u + 1] - r0;
                }
                int64_t incl = deg;
#pragma unroll
                for (int d = 1; d < LPF_WAVE; d <<= 1) {
                    const int64_t v = __shfl_up(incl, d);
                    if (lane >= d) incl += v;
                }
                if (lane == LPF_WAVE - 1) s_wave[wave] = incl;
                __syncthreads();
#pragma unroll
                for (int q = 0; q < BFS_WAVES; ++q) incl += q < wave ? s_wave[q] : 0;
                s_incl[tid] = incl;
                s_row[tid] = r0;
                __syncthreads();
                const int64_t total = s_incl[BFS_BLOCK - 1];
                for (int64_t base = 0; base < total; base += BFS_BLOCK) {   // block-uniform bounds, no barrier inside
                    if (*(volatile int32_t *)&s_found) break;   // (one LDS word: wave-uniform)
                    const int64_t f = base + tid;
                    bool claimed = false;
                    int32_t c = 0;
                    if (f < total) {
                        // owner of slot f: the number of chunk rows whose inclusive end is <= f, bit by bit
                        int q = 0;
#pragma unroll
                        for (int bit = BFS_BLOCK >> 1; bit > 0; bit >>= 1)
                            if (s_incl[q + bit - 1] <= f) q += bit;
                        c = col[s_row[q] + (f - (q ? s_incl[q - 1] : 0))];
                        if ((uint64_t)c < (uint64_t)n && c != skip) {
                            uint32_t w = stamp[c];
                            if ((w >> 1) != epoch) {          // not seen in this search (as far as this load tells)
                                const uint32_t old = atomicCAS(&stamp[c], w, mine);
                                claimed = old == w;
                                w = old;                      // lost: the word holds this epoch, whoever wrote it
                            }
                            if (!claimed && w == (mine ^ 1u)) s_found = 1;   // the other side holds c: contact
                        }
                    }
                    const uint64_t cm = __ballot(claimed);
                    if (cm) {                                 // wave-uniform
                        int64_t dg = claimed ? rowptr[c + 1] - rowptr[c] : 0;
#pragma unroll
                        for (int m = LPF_WAVE >> 1; m > 0; m >>= 1) dg += __shfl_xor(dg, m);
                        int32_t at = 0;
                        if (lane == 0) {
                            at = atomicAdd(&s_cnt, __popcll(cm));
                            atomicAdd(&s_deg, (unsigned long long)dg);
                        }
                        at = __shfl(at, 0) + __popcll(cm & ((1ull << lane) - 1ull));
                        if (claimed) vis[side_b ? f_lo - 1 - at : a_end + at] = c;
                    }
                }
                __syncthreads();                  // s_incl / s_row are rewritten by the next chunk
                if (s_found) break;               // block-uniform: read after the barrier
            }
            const int32_t found = s_found, cnt = s_cnt;
            const unsigned long long dsum = s_deg;
            __syncthreads();                      // the counters are reset by the next round
            if (found) {
                result = depth_a + depth_b + 1;
                break;
            }
            if (side_b) {
                b_hi = b_lo;
                b_lo -= cnt;
                ++depth_b;
                deg_b = dsum;
            } else {
                a_lo = a_end;
                a_end += cnt;
                ++depth_a;
                deg_a = dsum;
            }
        }
        if (tid == 0) A.dist[p] = result;
        __syncthreads();                          // s_ticket is rewritten by the next pair
    }
}

}  // namespace

extern "C" int64_t lpf_pair_bfs_workspace_bytes(int64_t n, int64_t n_groups) {
    if (n <= 0 || n_groups <= 0) return 0;
    return n_groups * (8 * n + 8);              // per group: n stamp words and a visit list of n + 2 int32
}

extern "C" int lpf_pair_bfs(int64_t P, int64_t n, const int64_t *pairs, int64_t pairs_ld, const int64_t *rowptr,
                            const int32_t *col, int32_t max_dist, int32_t flags, int32_t split_threshold,
                            int32_t *scratch, void *workspace, int64_t n_groups, int32_t *dist, void *stream) {
    if (P == 0) return LPF_OK;
    LPF_REQUIRE(P > 0 && P < INT32_MAX && n > 0 && n < INT32_MAX - 2 && pairs && pairs_ld >= P && rowptr && col &&
                scratch && workspace && n_groups > 0 && n_groups <= 65535 && dist && lpf_aligned16(workspace));
    BfsArgs A{};
    A.P = P;
    A.n = n;
    A.pairs = pairs;
    A.ld = pairs_ld;
    A.rowptr = rowptr;
    A.col = col;
    A.max_dist = max_dist > 0 ? max_dist : 0;
    A.ignore_direct = flags & 1;
    A.thr = split_threshold < 0 ? LPF_BFS_SPLIT_DEFAULT : split_threshold;
    A.list = scratch;
    A.stamps = static_cast<uint32_t *>(workspace);
    A.visits = reinterpret_cast<int32_t *>(A.stamps + n_groups * n);
    A.dist = dist;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t grid = P < n_groups ? P : n_groups;
    if (hipMemsetAsync(scratch, 0, sizeof(int32_t), s) != hipSuccess ||   // listed-pair counter
        hipMemsetAsync(A.stamps, 0, (size_t)(grid * n) * sizeof(uint32_t), s) != hipSuccess) {
        lpf_set_hip_error(hipGetLastError());
        return LPF_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(bfs_front_kernel, dim3((unsigned)((P + BFS_BLOCK - 1) / BFS_BLOCK)), dim3(BFS_BLOCK), 0, s, A);
    LPF_CHECK_LAUNCH();
    hipLaunchKernelGGL(bfs_search_kernel, dim3((unsigned)grid), dim3(BFS_BLOCK), 0, s, A);
    LPF_CHECK_LAUNCH();
    return LPF_OK;
}
