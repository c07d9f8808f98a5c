// One element of an aggregated row of a node with one or two in-edges, as the egonet walks form it.  The forward walk
// (gat_aggregate_ego_kernel) writes it; the fused backward walk (gat_fused_bwd_ego_kernel<.., REFORM>) forms it again from the same Y rows
// and the same coefficients instead of reading it back.  ONE expression for both, so that the two stay bit-identical: the order of the
// FMAs and the explicit + 0 of the first one (-0 products become +0) are part of the result.
//   parent  (in-list [self])      : r = act(fmaf(cs, y, 0))
//   sibling (in-list [hub, self]) : r = act(fmaf(cs, y, fmaf(ch, hub, 0)))        (a run of two: the base is the run's accumulator)
// One wave per node (gat_fwd_node: acc = fmaf(coef_e, row_e, acc) over the in-list, from 0) gives the same bits; for an in-list
// [self, hub] it gives the sibling form with the two (coefficient, row) pairs swapped.
#pragma once
#include "txe_common.h"

namespace txe {

// a run's accumulator behind row y: fl = 2 starts a run here, 1 continues it, 0 leaves acc alone
__device__ __forceinline__ float ego_run_acc(const float cr, const float y, const int fl, const float acc) {
    const float tmp = fmaf(cr, y, (fl == 2) ? 0.f : acc);
    return fl ? tmp : acc;
}

// hubref: the base is the hub's row times ch; otherwise the run's accumulator (hasrun) or nothing
__device__ __forceinline__ float ego_row_elem(const float cs, const float y, const bool hubref, const float ch, const float hub,
                                              const bool hasrun, const float acc, const bool act, const float act_slope) {
    const float base = hubref ? fmaf(ch, hub, 0.f) : (hasrun ? acc : 0.f);
    float r = fmaf(cs, y, base);
    if (act) r = leaky(r, act_slope);
    return r;
}

}  // namespace txe
