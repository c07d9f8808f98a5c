// The per-element Adam / AMSGrad update, shared by the dense launch (txe_optim.hip: every element of every parameter tensor) and the
// row-sparse one (txe_rowgrad.hip: the touched rows of the feature table).  ONE copy: optim.host_guarded_adam restates it operation for
// operation and the Adam tests pin its bits.
#pragma once
#include <math.h>

#include "txe_common.h"

namespace txe {

struct AdamScalars {
    float one_minus_b1, b2, one_minus_b2, eps, wd, step_size, bc2_sqrt;
};

// the scalars of update number `step` (>= 1), rounded to fp32 once, on the host
static inline AdamScalars adam_scalars(double lr, double beta1, double beta2, double eps, double weight_decay, long long step) {
    AdamScalars c;
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    c.one_minus_b1 = (float)(1.0 - beta1);
    c.b2 = (float)beta2;
    c.one_minus_b2 = (float)(1.0 - beta2);
    c.eps = (float)eps;
    c.wd = (float)weight_decay;
    c.step_size = (float)(lr / bc1);
    c.bc2_sqrt = (float)sqrt(bc2);
    return c;
}

// The products that hipcc contracts under its default -ffp-contract=fast are spelled as fmaf here, so that the arithmetic is a property
// of the source (optim.host_guarded_adam restates it operation for operation): m = fma(1-b1, g - m, m), v = fma(g, (1-b2) g, b2 v).
template <bool GUARD>
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float& vm, bool ams, const AdamScalars& c, float coef) {
    if (GUARD) g *= coef;                                   // coef == 1: g unchanged, bit for bit
    g = fmaf(c.wd, p, g);                                   // wd == 0: g unchanged
    m = fmaf(c.one_minus_b1, g - m, m);                     // lerp(m, g, 1 - beta1)
    v = fmaf(g, c.one_minus_b2 * g, c.b2 * v);
    float d;
    if (ams) { vm = fmaxf(vm, v); d = sqrtf(vm) / c.bc2_sqrt + c.eps; }
    else d = sqrtf(v) / c.bc2_sqrt + c.eps;
    p -= c.step_size * m / d;
}

}  // namespace txe
