// The row arithmetic of the InfoNCE losses, shared by txe_loss.hip (txe_info_nce) and txe_taxoloss.hip (txe_info_nce_taxo) so that
// the two cannot drift apart: on the same row values both leave the same bytes in d_x.
#pragma once
#include "txe_common.h"

namespace txe {

// One row of Cc values on a group of GW lanes (GW = 32 or 64, lane gl of the group; longer rows loop, lane gl takes c = gl, gl + GW, ...).
// val(c) gives the row's value at column c.  A lane asks it for the columns it owns, three times -- the maximum, the sum of
// __expf(v - max) and the gradient, each combined over the group by __shfl_xor from GW / 2 down -- and lane 0 for column t besides.
// With `live` the lane writes drow[c] = __expf(v - max) / sum - [c == t] for its columns; the group's lane 0 gets the row's loss
// (max + __logf(sum)) - val(t) back, every other lane (and a row that is not live) 0.  val(t) is taken BEFORE the first store to drow, and
// a column is stored by its owner after the owner's last read of it: val may read drow itself at columns of the asking lane
// (txe_taxoloss.hip keeps the shifted values of long rows there, with t = 0, lane 0's own).  All lanes of a wave call this together.
template <int GW, class Val>
__device__ __forceinline__ float nce_row(Val val, int Cc, int gl, int t, bool live, float* drow) {
    float m = -INFINITY;
    for (int c = gl; c < Cc; c += GW) m = fmaxf(m, val(c));
#pragma unroll
    for (int o = GW / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float s = 0.f;
    for (int c = gl; c < Cc; c += GW) s += __expf(val(c) - m);
#pragma unroll
    for (int o = GW / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float inv = 1.f / s;
    float out = 0.f;
    if (live) {
        const float xt = gl == 0 ? val(t) : 0.f;
        for (int c = gl; c < Cc; c += GW) drow[c] = __expf(val(c) - m) * inv - (c == t ? 1.f : 0.f);
        if (gl == 0) out = m + __logf(s) - xt;
    }
    return out;
}

}  // namespace txe
