// The row arithmetic of the moments mode of the all-candidate loop (txe.h: txe_score_moments_block), shared by the three score
// kernels' epilogues (txe_gemm.h gemm_tile_epilogue, txe_mlp_score.hip, and through the former txe_ntn_score.hip and the bf16 pipe)
// so that they cannot drift apart: on the same scores all of them leave the same quadruples.
#pragma once
#include "txe_common.h"

namespace txe {

// A set of scaled scores t is carried as the quadruple (m, s0, s1, s2): m = max t (NaN kept, lse_max), and with d = t - m <= 0
//   s0 = sum exp(d),  s1 = sum d exp(d),  s2 = sum d^2 exp(d)
// -- the sums centred at the set's own maximum: nothing overflows, and no variance is ever formed as a difference of large numbers.
// The sums count only while m is finite (lse_term's rule); a t = -Inf adds nothing to any of them (no -Inf * 0).
//
// mom_scaled: t = fl32(beta * z), ONE multiply rounded on its own (never contracted into the subtraction of the maximum); z = the
// score when larger is better, else its negative.  beta = 1 gives z back bit for bit.
__device__ __forceinline__ float mom_scaled(float x, bool larger, float beta) {
#pragma clang fp contract(off)                       // (the product carries no contract flag: no later pass can fold it into an fma)
    const float t = beta * (larger ? x : -x);
    return t;
}

// the maximum pass over one value: `bad` collects a NaN among the values that count, mx the hardware maximum of the others
__device__ __forceinline__ void mom_max_step(float t, bool in, float& mx, bool& bad) {
    bad |= in & (t != t);
    mx = in ? fmaxf(mx, t) : mx;
}

// the sum pass over one value of a set whose maximum is m: s0 takes lse_term's very value (at beta = 1 the lse mode's sum, bit for bit)
__device__ __forceinline__ void mom_sum_step(float t, bool in, float m, float& s0, float& s1, float& s2) {
    const float d = t - m;
    const float e = in ? lse_term(t, m) : 0.f;
    const float dz = (e > 0.f) ? d : 0.f;            // (t = -Inf, m not finite, a column past N: e is 0 and d may be -Inf or NaN)
    const float de = dz * e;
    s0 += e;
    s1 += de;
    s2 = __builtin_fmaf(dz, de, s2);
}

// A row's merged quadruple -> (lse, mean, var, entropy) in float64 (txe.h states the formulas).  M: the largest part maximum (NaN kept);
// S0 / S1 / S2: the parts' sums re-centred at M.  Where lse is not finite the other three are NaN.
__device__ __forceinline__ void mom_finish(float M, double S0, double S1, double S2, double* out) {
    const double nan = __builtin_nan("");
    if (!(fabsf(M) < INFINITY)) {                    // NaN in the row; a +Inf term; no term above -Inf
        out[0] = (double)M; out[1] = nan; out[2] = nan; out[3] = nan;
        return;
    }
    const double ls = (S0 != 1.0) ? log(S0) : 0.0, r1 = S1 / S0, v = S2 / S0 - r1 * r1, h = ls - r1;
    out[0] = (double)M + ls;
    out[1] = (double)M + r1;
    out[2] = v > 0.0 ? v : 0.0;
    out[3] = h > 0.0 ? h : 0.0;
}

}  // namespace txe
