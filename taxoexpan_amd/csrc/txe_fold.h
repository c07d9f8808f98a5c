// What the fused backward sweep (txe_fold_bwd.hip) shares with the folded output layers (txe_fold.hip): the workspace plan of the
// folded GAT layer's backward and the launchers of its sweep-3 and edge-level kernels.
#pragma once
#include "txe_common.h"

namespace txe {

// the folded matcher's backward in the prologue of cl_attn_bwd_kernel<true> (txe_fold.hip)
struct FoldDcArgs {
    const float* e_part; int ntile; const float *m_ds, *m_s; int m_exp; float scale; const float *wsum, *coef; float *dc, *cn, *dS;
    const int* zrow; int* zgid;
};

struct CollapseWs {
    float *dZ, *part, *dwa_part, *dwa, *dc, *cn, *dS, *dz, *da1, *da2, *dwv, *ppart, *ppart2;
    void* tail;
    size_t tail_bytes, total;
    int splits, seg_blocks, seg_rows, chunks;
};

CollapseWs plan_collapse_ws(void* ws, int n, int e, int G, int Kp, int D, int Pd, int vocab, int max_splits = 0);
int cl_bwd_dot_launch(int n_nodes, const int* gid, const float* X, int Kp, const unsigned* mk, const unsigned* dummy_mask, int mask_ld, float fs,
                      const float* dZ, const float* wsum, const float* coef, float* dc, float* cn, int nb_ds, int G, int D, const float* d_hg,
                      long long ld_dhg, const float* hg, long long ld_hg, float* dS, double bytes, hipStream_t s);
// cl_attn_bwd_kernel<fold> (no launch check of its own: the caller's next TXE_CHECK_LAUNCH covers it)
void cl_attn_bwd_launch(bool fold, const int* rowptr_in, const int* col_src, const int* rowptr_out, const int* pos_out, const int* goff, int G,
                        const float* a12, float slope, const float* alpha, float drop_p, float drop_scale, unsigned long long seed, const int* pos,
                        const float* pw, const float* dc, const float* dS, float* dz, float* da1, float* da2, float* dwv, const FoldDcArgs& fd,
                        hipStream_t s);

}  // namespace txe
