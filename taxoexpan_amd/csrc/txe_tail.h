// The reductions that end a layer's backward (position sums, folded attention rows, unfold), shared by the dense projections
// (txe_project.hip), the folded output layers (txe_fold.hip) and the fused backward sweep (txe_fold_bwd.hip): the jobs more than one
// unit's kernels inline, their argument structs, and the launchers of the kernels txe_project.hip defines.
#pragma once
#include "txe_common.h"
#include "txe_dxpos.h"

namespace txe {

constexpr int MAX_VOCAB = 8;

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// dwa[r][k] = sum_s part[s][F + r][k]     r < 2H
__device__ __forceinline__ void ext_rows_job(const int r, const int k, const float* __restrict__ part, int S, long long split_stride, int F,
                                             int ldp, float* __restrict__ dwa) {
    if (k >= ldp) return;
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc += part[(long long)s * split_stride + (long long)(F + r) * ldp + k];
    dwa[(long long)r * ldp + k] = acc;
}

// arguments of unfold_job (txe_project.hip)
struct UnfoldArgs {
    const float* part; int S; long long split_stride; const float* dwa; long long ldp; const float* W; long long ldw;
    const float *attn_l, *attn_r; int H, D, Kt; float* dW; long long ld_dw; float *d_attn_l, *d_attn_r;
};

// Deterministic two-stage "sum rows by position class":  dP[c][j] = sum_{m : pos[m]==c} x[m][j]
// stage 1: block b owns rows [b*rows_per_block, ...): 64 column lanes x 4 row groups, fixed-order LDS combine.
struct Seg1Args { const float* x; long long ldx; int cols; float* part; };
__device__ __forceinline__ void segsum1_job(const int bid, const Seg1Args& a, const int* __restrict__ pos, int n_rows, int vocab,
                                            int rows_per_block) {
    __shared__ float red[4][MAX_VOCAB][64];
    const int r0 = bid * rows_per_block, r1 = min(n_rows, r0 + rows_per_block);
    const int jl = threadIdx.x & 63, rg = threadIdx.x >> 6;
    for (int j0 = 0; j0 < a.cols; j0 += 64) {
        const int j = j0 + jl;
        const int jc = (j < a.cols) ? j : 0;
        float acc[MAX_VOCAB];
#pragma unroll
        for (int c = 0; c < MAX_VOCAB; ++c) acc[c] = 0.f;
#pragma unroll 4
        for (int m = r0 + rg; m < r1; m += 4) {
            const int pc = pos[m];
            const float v = a.x[(long long)m * a.ldx + jc];
#pragma unroll
            for (int c = 0; c < MAX_VOCAB; ++c) acc[c] += (pc == c) ? v : 0.f;
        }
#pragma unroll
        for (int c = 0; c < MAX_VOCAB; ++c) red[rg][c][jl] = acc[c];
        __syncthreads();
        if (rg == 0 && j < a.cols)
            for (int c = 0; c < vocab; ++c)
                a.part[((long long)bid * vocab + c) * a.cols + j] = red[0][c][jl] + red[1][c][jl] + red[2][c][jl] + red[3][c][jl];
        __syncthreads();
    }
}
struct Seg2Args { const float* part; int nb; int n /* vocab * cols */; float* out; };
__device__ __forceinline__ void segsum2_job(const int bid, const Seg2Args& a) {
    __shared__ float red[4][64];
    const int il = threadIdx.x & 63, bg = threadIdx.x >> 6;
    const int i = bid * 64 + il;
    const int ic = (i < a.n) ? i : 0;
    float acc = 0.f;
    for (int b0 = bg; b0 < a.nb; b0 += 64) {          // 16 partial rows of this row group per step: clamped loads issued together
        float v[16];                                   // (the fused sweeps leave ~1,100 partial rows: one load in flight per thread
#pragma unroll                                         //  made this walk 280 dependent round trips)
        for (int q = 0; q < 16; ++q) v[q] = a.part[(long long)min(b0 + 4 * q, a.nb - 1) * a.n + ic];
#pragma unroll
        for (int q = 0; q < 16; ++q) acc += (b0 + 4 * q < a.nb) ? v[q] : 0.f;
    }
    red[bg][il] = acc;
    __syncthreads();
    if (bg == 0 && i < a.n) a.out[i] = red[0][il] + red[1][il] + red[2][il] + red[3][il];
}

// The reductions that end a GATLayer's backward, as TWO launches of independent jobs on disjoint workgroup ranges:
//   phase A: per-block partial position sums (embedding gradient; readout position-weight gradient) and the folded attention rows'
//            gradient d_wa (split-K slices of the extension rows, or the per-block partials of the folded output layer);
//   phase B: dW / d_attn from d_wa (unfold) and the second stage of the position sums.
struct TailA {
    int nb_dx; DxPosArgs dx;                    // leading jobs: the streaming d_X kernel's row blocks (dxpos_finish_job)
    int nb_s1a, nb_s1b, nb_r, r_kind;           // r_kind 1: extension rows of the split-K weight gradient, 2: stage 2 over dwa_part
    Seg1Args s1a, s1b;
    const int* pos; int n_rows, vocab, rows_per_block;
    const float* rpart; int S; long long split_stride; int F, ldp, nbx; float* dwa;
    Seg2Args r2;
};
__device__ __forceinline__ void reduce_a_job(int b, const TailA& a) {
    if (b < a.nb_dx) { dxpos_finish_job(b, a.dx); return; }
    b -= a.nb_dx;
    if (b < a.nb_s1a) { segsum1_job(b, a.s1a, a.pos, a.n_rows, a.vocab, a.rows_per_block); return; }
    b -= a.nb_s1a;
    if (b < a.nb_s1b) { segsum1_job(b, a.s1b, a.pos, a.n_rows, a.vocab, a.rows_per_block); return; }
    b -= a.nb_s1b;
    if (a.r_kind == 1) ext_rows_job(b / a.nbx, (b % a.nbx) * 256 + threadIdx.x, a.rpart, a.S, a.split_stride, a.F, a.ldp, a.dwa);
    else segsum2_job(b, a.r2);
}
struct TailB {
    int nb_u, nb_2a, nb_2b;
    UnfoldArgs u;
    Seg2Args s2a, s2b;
};

// launchers of txe_project.hip's kernels: gat_bwd_reduce_a_kernel; gat_bwd_reduce_b(_multi)_kernel; pos_segsum_stage1 + stage2;
// reduce_splits_sub_kernel
int tail_a_launch(const TailA& a, hipStream_t s);
int tail_b_submit(const TailB* own, void* chain_, bool defer, hipStream_t s);
int pos_segsum_launch(const float* x, long long ldx, const int* pos, int n_rows, int cols, int vocab, int nb, int rows_per_block, float* part,
                      float* out, hipStream_t s);
int reduce_splits_sub_launch(const float* part, int S, long long stride, int rows, int cols, int ldp, float* out, hipStream_t s);

}  // namespace txe
