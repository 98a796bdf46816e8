// First layer of the PPR positional MLP with its LayerNorm in closed form (shared by the attention kernels).
// Reference: get_pos_encodings (src/models/link_transformer.py:182-211) -> MLP (src/models/other_models.py:125-138).
#pragma once
#include "lpf_common.h"

// pe_stat float[6][8] (fold.pe_tables).  Rows 0-2 state the 3 x 3 centred second-moment matrix M of (w0, w1, b) over the
// hidden units by its six entries and are not read on the device; rows 3-5 hold its factor L, M = L L^T, lower triangular,
// as (l00, l10, l20, l11, l21, l22, 0, no-flip radius): the kernels read these, from float PE_STAT_FACTOR on.
constexpr int PE_STAT_FACTOR = 24;

struct PeStat {
    float l00, l10, l20, l11, l21, l22;
};

__device__ __forceinline__ PeStat pe_load_stat(const float *__restrict__ pe_stat, int t) {
    const float *__restrict__ f = pe_stat + PE_STAT_FACTOR + 8 * t;
    PeStat s;
    s.l00 = f[0]; s.l10 = f[1]; s.l20 = f[2];
    s.l11 = f[3]; s.l21 = f[4]; s.l22 = f[5];
    return s;
}

// Variance of u_k = w0_k*x + w1_k*y + b_k over k: (x, y, 1) M (x, y, 1)^T = |L^T (x, y, 1)|^2, a sum of squares.  Written
// out as the quadratic form of M it is a difference of large terms where w1 ~ -w0 and x ~ y, and loses
// u * (sum of |terms|) / var; as a sum of squares it loses the root of that, at the same instruction count.
__device__ __forceinline__ float pe_var(float l00, float l10, float l20, float l11, float l21, float l22, float x, float y) {
    const float a = fmaf(l00, x, fmaf(l10, y, l20));
    const float b = fmaf(l11, y, l21);
    return fmaf(a, a, fmaf(b, b, l22 * l22));
}

// LayerNorm statistics of u_k: mean-free by construction (pe_tab already holds centred, gamma-scaled coefficients), so
// only 1/std is needed.
__device__ __forceinline__ float pe_rstd(const PeStat &s, float x, float y) {
    return 1.0f / sqrtf(pe_var(s.l00, s.l10, s.l20, s.l11, s.l21, s.l22, x, y) + 1e-5f);
}

// h_k = ReLU(LN(W1 [pa,pb] + b1))_k + ReLU(LN(W1 [pb,pa] + b1))_k ; k = (g (w0 - mean), g (w1 - mean), g (b - mean), beta)
__device__ __forceinline__ float pe_hidden(const float4 k, float pa, float pb, float r_ab, float r_ba) {
    const float u_ab = fmaf(k.x, pa, fmaf(k.y, pb, k.z));
    const float u_ba = fmaf(k.x, pb, fmaf(k.y, pa, k.z));
    return fmaxf(fmaf(r_ab, u_ab, k.w), 0.0f) + fmaxf(fmaf(r_ba, u_ba, k.w), 0.0f);
}
