// Dense feature projections of the propagation layers, forward and backward, on the fp32 MFMA GEMM.
//
//   GATLayer (model_zoo.py:82-85):   h = feat_drop(cat(x, P[pos]));  ft = h W^T;  a1 = <ft, attn_l>;  a2 = <ft, attn_r>
//   GCNLayer (model_zoo.py:35-37):   h = dropout(cat(x, P[pos]));    hw = h W
//
// MI355X-first restructuring (identical math, different association):
//  * the concat with the position embedding and the dropout are synthesised by the GEMM's operand loader
//    (txe_gemm.h VMat) -- cat(x, P[pos]) and the dropped copy never exist in HBM;
//  * the attention projections are folded into the same GEMM: a1 = h (W^T attn_l) -> 2H extra output
//    columns computed from 2H folded weight rows wa = [attn_l; attn_r] (x) W.  That removes the two
//    N x H x D passes of model_zoo.py:84-85 in forward AND their two passes in backward: the gradients
//    d a1, d a2 ride as 2H extra columns of the incoming gradient through the dX and dW GEMMs and are
//    unfolded on the (tiny) weight side:  dW += attn (x) d wa,  d attn = <d wa, W>.
#include <string.h>

#include "txe_gemm.h"
#include "txe_gather.h"
#include "txe_dxpos.h"
#include "txe_gemm_split.h"
#include "txe_tail.h"

namespace txe {

// wa[h][k]   = sum_d attn_l[h*D+d] * W[(h*D+d)*ldw + k]
// wa[H+h][k] = sum_d attn_r[h*D+d] * W[(h*D+d)*ldw + k]            (k < Kt)
// One workgroup per (row r, 64-column chunk): 64 columns x 16 d-groups, LDS tree over the d-groups.
constexpr int FOLD_DG = 16;
__device__ __forceinline__ void fold_attn_job(const int bx, const int r /* 0 .. 2H-1 */, const float* __restrict__ W, long long ldw, int Kt,
                                              const float* __restrict__ attn_l, const float* __restrict__ attn_r, int H, int D,
                                              float* __restrict__ wa, long long ld_wa) {
    __shared__ float red[FOLD_DG][64];
    const int h = r % H;
    const float* attn = ((r < H) ? attn_l : attn_r) + (long long)h * D;
    const float* Wh = W + (long long)h * D * ldw;
    const int kl = threadIdx.x & 63, dg = threadIdx.x >> 6;
    const int k = bx * 64 + kl;
    const int kc = (k < Kt) ? k : 0;
    float acc = 0.f;
#pragma unroll 4
    for (int d = dg; d < D; d += FOLD_DG) acc = fmaf(attn[d], Wh[(long long)d * ldw + kc], acc);
    red[dg][kl] = acc;
    __syncthreads();
    if (dg == 0 && k < Kt) {
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < FOLD_DG; ++g) s += red[g][kl];
        wa[(long long)r * ld_wa + k] = s;
    }
}
__global__ __launch_bounds__(64 * FOLD_DG) void fold_attn_kernel(const float* __restrict__ W, long long ldw, int Kt,
                                                                 const float* __restrict__ attn_l, const float* __restrict__ attn_r,
                                                                 int H, int D, float* __restrict__ wa, long long ld_wa) {
    fold_attn_job(blockIdx.x, blockIdx.y, W, ldw, Kt, attn_l, attn_r, H, D, wa, ld_wa);
}

__global__ void reduce_ext_rows_kernel(const float* __restrict__ part, int S, long long split_stride, int F, int H2, int ldp,
                                       float* __restrict__ dwa) {
    ext_rows_job(blockIdx.y, blockIdx.x * blockDim.x + threadIdx.x, part, S, split_stride, F, ldp, dwa);
}

// One workgroup per weight row f = h*D + d:
//   dW[f][k]    = sum_s part[s][f][k] + attn_l[f] * dwa[h][k] + attn_r[f] * dwa[H+h][k]
//   d_attn_l[f] = sum_k dwa[h][k]   * W[f][k]
//   d_attn_r[f] = sum_k dwa[H+h][k] * W[f][k]
__device__ __forceinline__ void unfold_job(const int f, const UnfoldArgs& a) {
    __shared__ float red[2][4];
    const int h = f / a.D;
    const float al = a.attn_l[f], ar = a.attn_r[f];
    float dl = 0.f, dr = 0.f;
    for (int k = threadIdx.x; k < a.Kt; k += blockDim.x) {
        // the split-K partials are summed in slice order, eight (unconditional, clamped) loads in flight at a time
        const float* pp = a.part + (long long)f * a.ldp + k;
        const float gl = a.dwa[(long long)h * a.ldp + k], gr = a.dwa[(long long)(a.H + h) * a.ldp + k];
        const float wv = a.W[(long long)f * a.ldw + k];
        float acc = 0.f;
        for (int s0 = 0; s0 < a.S; s0 += 8) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = pp[(long long)min(s0 + j, a.S - 1) * a.split_stride];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc += (s0 + j < a.S) ? v[j] : 0.f;
        }
        a.dW[(long long)f * a.ld_dw + k] = acc + al * gl + ar * gr;
        dl = fmaf(gl, wv, dl);
        dr = fmaf(gr, wv, dr);
    }
    dl = wave_sum(dl);
    dr = wave_sum(dr);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][w] = dl; red[1][w] = dr; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.d_attn_l[f] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        a.d_attn_r[f] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    }
}

// out[i] = sum_s part[s*stride + i]
__global__ void reduce_splits_kernel(const float* __restrict__ part, int S, long long stride, long long n, float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float acc = 0.f;
        for (int s = 0; s < S; ++s) acc += part[(long long)s * stride + i];
        out[i] = acc;
    }
}

// "sum rows by position class" (segsum1_job / segsum2_job, txe_tail.h) as two launches of their own
__global__ __launch_bounds__(256) void pos_segsum_stage1(const float* __restrict__ x, long long ldx, const int* __restrict__ pos,
                                                         int n_rows, int cols, int vocab, int rows_per_block,
                                                         float* __restrict__ part /*[nb][vocab][cols]*/) {
    Seg1Args a{x, ldx, cols, part};
    segsum1_job(blockIdx.x, a, pos, n_rows, vocab, rows_per_block);
}
__global__ __launch_bounds__(256) void pos_segsum_stage2(const float* __restrict__ part, int nb, int vocab, int cols,
                                                         float* __restrict__ out) {
    Seg2Args a{part, nb, vocab * cols, out};
    segsum2_job(blockIdx.x, a);
}
// both stages: out[c][j] = sum_{m : pos[m]==c} x[m][j] through part [nb][vocab][cols]
int pos_segsum_launch(const float* x, long long ldx, const int* pos, int n_rows, int cols, int vocab, int nb, int rows_per_block, float* part,
                      float* out, hipStream_t s) {
    if (n_rows > 0) {
        hipLaunchKernelGGL(pos_segsum_stage1, dim3(nb), dim3(256), 0, s, x, ldx, pos, n_rows, cols, vocab, rows_per_block, part);
        TXE_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(pos_segsum_stage2, dim3((vocab * cols + 63) / 64), dim3(256), 0, s, (const float*)part, n_rows > 0 ? nb : 0, vocab, cols, out);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

// the two launches that end a GATLayer's backward (TailA / TailB and phase A's jobs: txe_tail.h)
__global__ __launch_bounds__(256) void gat_bwd_reduce_a_kernel(const TailA a) { reduce_a_job(blockIdx.x, a); }
int tail_a_launch(const TailA& a, hipStream_t s) {
    hipLaunchKernelGGL(gat_bwd_reduce_a_kernel, dim3(a.nb_dx + a.nb_s1a + a.nb_s1b + a.nb_r), dim3(256), 0, s, a);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}
__device__ __forceinline__ void tail_b_job(int b, const TailB& a) {
    if (b < a.nb_u) { unfold_job(b, a.u); return; }
    b -= a.nb_u;
    if (b < a.nb_2a) { segsum2_job(b, a.s2a); return; }
    segsum2_job(b - a.nb_2a, a.s2b);
}
__global__ __launch_bounds__(256) void gat_bwd_reduce_b_kernel(const TailB a) { tail_b_job(blockIdx.x, a); }

// Phase B of SEVERAL layers in one launch.  A layer's phase B only finishes parameter gradients (nothing downstream in the backward
// pass reads them), so a caller may DEFER it (phases | TXE_PH_DEFER) into a host-side chain and let the last layer's call launch them all:
// one ~17 us dispatch per stack instead of one per layer.
constexpr int TAIL_CHAIN_MAX = 3;                       // deferred layers a chain holds (a fourth deferral flushes)
struct TailChain { int n; int pad; TailB tb[TAIL_CHAIN_MAX]; };
struct TailMulti { int n; int nb_end[TAIL_CHAIN_MAX + 1]; TailB tb[TAIL_CHAIN_MAX + 1]; };
__global__ __launch_bounds__(256) void gat_bwd_reduce_b_multi_kernel(const TailMulti m) {
    int b = blockIdx.x, i = 0;
    while (i + 1 < m.n && b >= m.nb_end[i]) ++i;                    // (block-uniform)
    tail_b_job(b - ((i > 0) ? m.nb_end[i - 1] : 0), m.tb[i]);
}
static inline int tail_b_blocks(const TailB& t) { return t.nb_u + t.nb_2a + t.nb_2b; }
// launch `own` (if given) together with everything the chain holds, or -- defer -- append `own` to the chain
int tail_b_submit(const TailB* own, void* chain_, bool defer, hipStream_t s) {
    TailChain* c = reinterpret_cast<TailChain*>(chain_);
    if (c && (c->n < 0 || c->n > TAIL_CHAIN_MAX)) return TXE_ERR_ARG;
    if (defer && c && own && c->n < TAIL_CHAIN_MAX) { c->tb[c->n++] = *own; return TXE_OK; }
    TailMulti m;
    memset(&m, 0, sizeof(m));
    int total = 0;
    auto add = [&](const TailB& t) { if (tail_b_blocks(t) > 0) { m.tb[m.n] = t; total += tail_b_blocks(t); m.nb_end[m.n++] = total; } };
    if (own) add(*own);
    if (c) { for (int i = 0; i < c->n; ++i) add(c->tb[i]); c->n = 0; }
    if (m.n == 0) return TXE_OK;
    if (m.n == 1) hipLaunchKernelGGL(gat_bwd_reduce_b_kernel, dim3(total), dim3(256), 0, s, m.tb[0]);
    else hipLaunchKernelGGL(gat_bwd_reduce_b_multi_kernel, dim3(total), dim3(256), 0, s, m);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}


__device__ __forceinline__ void dropout_mask_job(const int bid, const int nb, long long n_words, unsigned long long seed, unsigned thr16,
                                                 unsigned* __restrict__ mask) {
    for (long long w = (long long)bid * blockDim.x + threadIdx.x; w < n_words; w += (long long)nb * blockDim.x)
        mask[w] = drop_mask_word(seed, (unsigned long long)w, thr16);
}
__global__ void dropout_mask_kernel(long long n_words, unsigned long long seed, unsigned thr16, unsigned* __restrict__ mask) {
    dropout_mask_job(blockIdx.x, gridDim.x, n_words, seed, thr16, mask);
}

}  // namespace txe

using namespace txe;

extern "C" {

// Feature-dropout keep mask for an [n_rows][n_cols] operand: bit (r, c) = word[r*ceil(n_cols/32) + c/32] >> (c%32) & 1.
// nn.Dropout(p) of model_zoo.py:36,82 -- generated once per layer per step, reused by forward, dX and dW.
size_t txe_dropout_mask_bytes(long long n_rows, int n_cols) { return (size_t)n_rows * ((n_cols + 31) / 32) * 4; }

int txe_dropout_mask(long long n_rows, int n_cols, float p, unsigned long long seed, unsigned* mask, void* stream) {
    if (n_rows < 0 || n_cols < 1 || p < 0.f || p >= 1.f || !mask) return TXE_ERR_ARG;
    const long long n_words = n_rows * ((n_cols + 31) / 32);
    if (n_words == 0) return TXE_OK;
    const unsigned thr16 = (unsigned)(p * 65536.0f + 0.5f);
    const int nb = (int)((n_words + 255) / 256 < 4096 ? (n_words + 255) / 256 : 4096);
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, n_words, seed, thr16, mask);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

}  // extern "C"

namespace txe {

// ---------------------------------------------------------------------------------------------
// GATLayer dense part on PADDED operands.
//   X  [N][Kp]   layer input:  [h (Kh) | Emb[pos] (Pd) | 0 ...],  Kp = roundup(Kh+Pd, 32).  The producer of h (the previous
//                layer's aggregation kernel, or txe_gat_build_x for the raw features) writes straight into it.
//   Wp [Fp][Kp]  packed weights: rows < F = fc.weight, rows F..F+2H = folded attention rows, rest 0; Fp = roundup(F+2H,128)
//   Y  [N][Fp]   projection output: [ft (F) | a1 (H) | a2 (H) | unused];  d_Y has the same layout with ZERO padding.
// Every GEMM operand is then a plain, 16-byte aligned, tile-padded matrix (all tiles take the hoisted fast path); the only
// loader-side extra left is the dropout bit mask on X.
// ---------------------------------------------------------------------------------------------

// Wp[f][k] = W[f][k] (f < F, k < Kt) else 0   (rows F..Fe are written by fold_attn_kernel)
// One thread per 4 consecutive packed columns (Kp % 4 == 0), two such quads in flight per thread: every load is issued before the
// first store, the packed row leaves as 16-byte stores.  (One wave per row with a scalar column loop made the 2,080-column rows of
// the output layer a 33-deep load -> store chain per wave.)
constexpr int PREP_U = 2;
// extra (or NULL): row F of Wp = extra[0 .. Kt) -- a folded GCN layer's bias rides as one more weight row (txe_gcn_layer_prepare)
__device__ __forceinline__ void pack_w_job(const int bid, const int nb, const float* __restrict__ W, int F, int Fe, int Fp, int Kt, int Kp,
                                           float* __restrict__ Wp, const float* __restrict__ extra = nullptr) {
    const unsigned qpr = (unsigned)Kp >> 2, total = (unsigned)Fp * qpr;          // (a weight matrix: far below 2^32 quads)
    const bool v2 = ((Kt & 1) == 0) && (((uintptr_t)W & 7) == 0);                // rows 8-byte aligned: float2 loads
    for (unsigned base = (unsigned)bid * blockDim.x * PREP_U; base < total; base += (unsigned)nb * blockDim.x * PREP_U) {
        float v[PREP_U][4];
        unsigned fi[PREP_U], ki[PREP_U];
#pragma unroll
        for (int u = 0; u < PREP_U; ++u) {
            const unsigned i = base + u * blockDim.x + threadIdx.x;
            const unsigned f = i / qpr, k = (i - f * qpr) * 4;
            fi[u] = f; ki[u] = k;
            const bool isx = extra != nullptr && i < total && f == (unsigned)F;
            const bool live = (i < total && f < (unsigned)F) || isx;
            const float* src = isx ? extra : W + (long long)(live ? f : 0) * Kt;
            if (live && k + 3 < (unsigned)Kt && v2) {
                const float2 a = *reinterpret_cast<const float2*>(src + k), b = *reinterpret_cast<const float2*>(src + k + 2);
                v[u][0] = a.x; v[u][1] = a.y; v[u][2] = b.x; v[u][3] = b.y;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[u][e] = (live && k + e < (unsigned)Kt) ? src[k + e] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < PREP_U; ++u) {
            const unsigned i = base + u * blockDim.x + threadIdx.x;
            if (i >= total) continue;
            float* dst = Wp + (long long)fi[u] * Kp + ki[u];
            if (fi[u] >= (unsigned)F && fi[u] < (unsigned)Fe) {                   // folded rows: the other job writes [0, Kt); zero the padding
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (ki[u] + e >= (unsigned)Kt) dst[e] = 0.f;
            } else {
                *reinterpret_cast<float4*>(dst) = make_float4(v[u][0], v[u][1], v[u][2], v[u][3]);
            }
        }
    }
}
__global__ void pack_w_kernel(const float* __restrict__ W, int F, int Fe, int Fp, int Kt, int Kp, float* __restrict__ Wp) {
    pack_w_job(blockIdx.x, gridDim.x, W, F, Fe, Fp, Kt, Kp, Wp);
}

// X[r][c] = h[r][c] (c < Kh, only when h != NULL) | P[pos[r]][c-Kh] (Kh <= c < Kt) | 0 (Kt <= c < Kp)
// drop_thr16 != 0: the feature dropout is applied HERE (X[r][c] *= keep(r, c) ? drop_scale : 0, the very bits of drop_mask_word over
// ceil(Kt/32) words per row): the layer's GEMMs then read X as a plain operand -- no mask words, no selects in their loaders (the
// first-layer projection and its weight gradient: 226 -> 213 us, 282 -> 269 us).  With `mask` given (only when h != NULL: every
// word of a row is then needed here anyway) the job also WRITES the keep mask, and the launch needs no mask job for this layer.
//
// A workgroup owns a block of consecutive rows; one thread per 4 consecutive columns (a "quad", Kp % 32 == 0), PREP_UX quads in
// flight per thread, 16-byte stores.  Branch-free: every quad issues its pos[] load and its (column-clamped) feature loads, the
// workgroup then hashes the rows' mask words ONCE each into LDS (under those loads' latency), and -- pos[] being the oldest load in
// flight -- the (clamped) position-embedding loads follow; selects afterwards: two memory latencies per thread whatever mix of
// feature / embedding / padding quads a wave holds.  (One wave per row with a scalar column loop ran 5 dependent load -> hash ->
// store rounds per wave; divergent quad kinds with the dependent pos -> P chain inside a branch were slower still.)
constexpr int PREP_UX = 4;
constexpr int PREP_LDSW = 4096;                         // mask words a row block may hold in LDS
__device__ __forceinline__ void build_x_job(const int bid, const int nb, const float* __restrict__ h, long long ld_h, const int* __restrict__ pos,
                                            const float* __restrict__ P, int n_rows, int Kh, int Pd, int Kp, float* __restrict__ X,
                                            const unsigned long long drop_seed = 0, const unsigned drop_thr16 = 0, const float drop_scale = 1.f,
                                            unsigned* __restrict__ mask = nullptr) {
    __shared__ unsigned s_words[PREP_LDSW];
    const int T = blockDim.x;
    const int Kt = Kh + Pd, wpr = (Kt + 31) >> 5;
    const int q0 = h ? 0 : (Kh >> 2);                   // h == NULL: columns [0, Kh) are in place already
    const int qn = (Kp >> 2) - q0;                      // quads per row handled here
    const int w_lo = (q0 * 4) >> 5, nw = (Kp >> 5) - w_lo;   // mask words of a row that cover those quads (Kp/32 >= wpr; words >= wpr: no bits)
    const bool drop = drop_thr16 != 0u;
    const bool lds_words = drop && nw <= PREP_LDSW;
    int RB = (T * PREP_UX) / qn;                        // rows per block: one pass of PREP_UX quads per thread
    if (RB < 1) RB = 1;
    if (lds_words && RB * nw > PREP_LDSW) RB = PREP_LDSW / nw;
    const bool v2 = h && Kh >= 2 && ((Kh & 1) == 0) && ((ld_h & 1) == 0) && (((uintptr_t)h & 7) == 0);   // whole 8-byte pairs inside a row
    for (long long r0l = (long long)bid * RB; r0l < n_rows; r0l += (long long)nb * RB) {
        const int r0 = (int)r0l, nr = min(RB, n_rows - r0), nq = nr * qn;
        for (int pb = 0; pb < nq; pb += T * PREP_UX) {  // (one pass unless a single row has more than T * PREP_UX quads)
            float hv[PREP_UX][4], pv[PREP_UX][4];
            int li[PREP_UX], ci[PREP_UX], pr[PREP_UX];  // local row (-1: no quad), first column, pos[]
#pragma unroll
            for (int u = 0; u < PREP_UX; ++u) {
                const int i = pb + u * T + (int)threadIdx.x;
                const bool live = i < nq;
                const int lr = live ? i / qn : 0;
                li[u] = live ? lr : -1;
                ci[u] = (q0 + (live ? i - lr * qn : 0)) * 4;
                pr[u] = (Pd > 0) ? pos[r0 + lr] : 0;
            }
            if (h) {
#pragma unroll
                for (int u = 0; u < PREP_UX; ++u) {
                    const float* hrow = h + (long long)(r0 + max(li[u], 0)) * ld_h;
                    const int c = ci[u];
                    if (v2) {
                        const float2 a = *reinterpret_cast<const float2*>(hrow + min(c, Kh - 2));
                        const float2 b = *reinterpret_cast<const float2*>(hrow + min(c + 2, Kh - 2));
                        hv[u][0] = a.x; hv[u][1] = a.y; hv[u][2] = b.x; hv[u][3] = b.y;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) hv[u][e] = hrow[min(c + e, Kh - 1)];
                    }
                }
            }
            if (lds_words && pb == 0) {                 // the block's mask words, once each (under the loads above)
                for (int wi = threadIdx.x; wi < nr * nw; wi += T) {
                    const int lr = wi / nw, wl = w_lo + (wi - lr * nw);
                    const unsigned long long w = (unsigned long long)(r0 + lr) * wpr + wl;
                    const unsigned word = (wl < wpr) ? drop_mask_word(drop_seed, w, drop_thr16) : 0u;
                    s_words[wi] = word;
                    if (mask && wl < wpr) mask[w] = word;
                }
                __syncthreads();
            }
            if (Pd > 0) {
#pragma unroll
                for (int u = 0; u < PREP_UX; ++u) {
                    const float* prow = P + (long long)pr[u] * Pd;
#pragma unroll
                    for (int e = 0; e < 4; ++e) pv[u][e] = prow[min(max(ci[u] + e - Kh, 0), Pd - 1)];
                }
            }
#pragma unroll
            for (int u = 0; u < PREP_UX; ++u) {
                if (li[u] < 0) continue;
                const int r = r0 + li[u], c = ci[u];
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (c + e < Kh) ? (h ? hv[u][e] : 0.f) : ((c + e < Kt) ? pv[u][e] : 0.f);
                if (drop && c < Kt) {                   // bits (c & 31) .. +3 of the row's mask word c / 32
                    const unsigned word = lds_words ? s_words[li[u] * nw + (c >> 5) - w_lo]
                                                    : drop_mask_word(drop_seed, (unsigned long long)r * wpr + (c >> 5), drop_thr16);
#pragma unroll
                    for (int e = 0; e < 4; ++e)         // (columns in [Kt, Kp) hold zeros: scaling them is harmless)
                        v[e] = ((word >> ((c & 31) + e)) & 1u) ? v[e] * drop_scale : 0.f;
                }
                float* dst = X + (long long)r * Kp + c;
                if (!h && c < Kh) {                     // the quad straddling Kh: its feature columns belong to the layer below
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e >= Kh) dst[e] = v[e];
                } else {
                    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
                }
            }
        }
        if (lds_words) __syncthreads();                 // (the next row block overwrites the words)
    }
}
__global__ void build_x_kernel(const float* __restrict__ h, long long ld_h, const int* __restrict__ pos, const float* __restrict__ P,
                               int n_rows, int Kh, int Pd, int Kp, float* __restrict__ X) {
    build_x_job(blockIdx.x, gridDim.x, h, ld_h, pos, P, n_rows, Kh, Pd, Kp, X);
}

// Everything a GATLayer needs before its projection GEMM, in ONE launch (four independent jobs on disjoint ranges of workgroups):
// layer input X (build_x), packed weights Wp (pack_w), folded attention rows (fold_attn), feature-dropout keep mask.
// workgroups of build_x_job: one per block of rows (the device code's RB)
static inline int build_x_blocks(int T, int n_rows, int Kh, int Pd, int Kp, bool has_h, bool drop, int cap) {
    const int q0 = has_h ? 0 : (Kh >> 2), qn = (Kp >> 2) - q0, nw = (Kp >> 5) - ((q0 * 4) >> 5);
    if (qn <= 0 || n_rows <= 0) return 0;
    int RB = (T * PREP_UX) / qn;
    if (RB < 1) RB = 1;
    if (drop && nw <= PREP_LDSW && RB * nw > PREP_LDSW) RB = PREP_LDSW / nw;
    const long long b = ((long long)n_rows + RB - 1) / RB;
    return (int)(b < cap ? b : cap);
}
struct PrepArgs {
    int nb_x, nb_w, nb_f, nb_m, fold_bx;
    const float* h; long long ld_h; const int* pos; const float* P; int n_rows, Kh, Pd, Kp; float* X;
    const float *W, *attn_l, *attn_r; int H, D, F, Fe, Fp, Kt; float* Wp;
    int pk_rows, pk_ext, pk_prows, pk_cols, pk_pcols;       // packing job: W [pk_rows][pk_cols] -> Wp [pk_prows][pk_pcols], rows [pk_rows, pk_ext) left to fold
    const float* pk_extra;                                  // ... or NULL / one more row (row pk_rows) to pack behind W
    long long n_words; unsigned long long seed; unsigned thr16; unsigned* mask;
    int x_dropped; float drop_scale;                        // build_x applies the dropout itself (the mask is still written:
    int x_mask;                                             //  by build_x too when x_mask, else by the mask job)
};
__device__ __forceinline__ void prepare_jobs(const PrepArgs& a, int b) {
    // the latency-bound job (a strided reduction per folded row) is dispatched first, the streaming jobs fill in behind it
    if (b < a.nb_f) {
        fold_attn_job(b % a.fold_bx, b / a.fold_bx, a.W, (long long)a.Kt, a.Kt, a.attn_l, a.attn_r, a.H, a.D, a.Wp + (long long)a.F * a.Kp,
                      (long long)a.Kp);
        return;
    }
    b -= a.nb_f;
    if (b < a.nb_w) { pack_w_job(b, a.nb_w, a.W, a.pk_rows, a.pk_ext, a.pk_prows, a.pk_cols, a.pk_pcols, a.Wp, a.pk_extra); return; }
    b -= a.nb_w;
    if (b < a.nb_m) { dropout_mask_job(b, a.nb_m, a.n_words, a.seed, a.thr16, a.mask); return; }
    b -= a.nb_m;
    build_x_job(b, a.nb_x, a.h, a.ld_h, a.pos, a.P, a.n_rows, a.Kh, a.Pd, a.Kp, a.X, a.seed, a.x_dropped ? a.thr16 : 0u, a.drop_scale,
                a.x_mask ? a.mask : nullptr);
}
__global__ __launch_bounds__(64 * FOLD_DG) void gat_prepare_kernel(const PrepArgs a) { prepare_jobs(a, blockIdx.x); }

// zero columns [c0, c1) of a row-major [n_rows][ld] matrix
__global__ void zero_cols_kernel(float* __restrict__ x, long long ld, int n_rows, int c0, int c1) {
    const int wdt = c1 - c0;
    const long long n = (long long)n_rows * wdt;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        x[(i / wdt) * ld + c0 + (i % wdt)] = 0.f;
}

// Y[v][c] = T[row[v]][c] + T2[row2[v]][c]   (16-byte columns): the layer-0 projection of a batch whose node features are rows of a
// taxonomy table -- T = table W^T computed once per DISTINCT taxonomy node, T2 = the 3 position-embedding rows' projections.
__global__ __launch_bounds__(256) void gather_add_rows_kernel(const float* __restrict__ T, long long ld_t, const int* __restrict__ row,
                                                              const float* __restrict__ T2, long long ld_t2, const int* __restrict__ row2,
                                                              long long n_rows, int nvec, float* __restrict__ Y, long long ld_y) {
    const long long total = n_rows * nvec;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long v = i / nvec;
        const int j = (int)(i % nvec);
        float4 a = *reinterpret_cast<const float4*>(T + (long long)row[v] * ld_t + 4 * j);
        if (T2) {
            const float4 b = *reinterpret_cast<const float4*>(T2 + (long long)row2[v] * ld_t2 + 4 * j);
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
        *reinterpret_cast<float4*>(Y + v * ld_y + 4 * j) = a;
    }
}

struct DenseWs {
    float* dwa;     // [2H][Kp]
    float* dxpart;  // the streaming d_X kernel's k-slice partial products
    float* ppart;   // [nb][vocab][Pd]
    float* part;    // [S][Fp][Kp]
    void* tail;
    size_t tail_bytes;
    int splits, seg_blocks, seg_rows;
    size_t total;
};

static DenseWs plan_dense_ws(void* ws, int n, int Fp, int H2, int Kp, int Pd, int vocab, bool dx_stream = true, int min_splits = 0) {
    DenseWs p;
    char* b = (char*)ws;
    size_t off = 0;
    auto take = [&](size_t bytes) { float* r = (float*)(b + off); off += align_up(bytes, 256); return r; };
    p.dwa = take((size_t)H2 * Kp * 4);
    p.seg_rows = 64;
    p.seg_blocks = (n + p.seg_rows - 1) / p.seg_rows;
    if (p.seg_blocks < 1) p.seg_blocks = 1;
    // (sized for the streaming d_X kernel's 16-row workgroups, which write these partial sums themselves)
    const int ppart_blocks = dxpos_blocks(n) > p.seg_blocks ? dxpos_blocks(n) : p.seg_blocks;
    p.ppart = take((size_t)ppart_blocks * (vocab > 0 ? vocab : 1) * (Pd > 0 ? Pd : 1) * 4);
    p.dxpart = take((Pd > 0 && dx_stream) ? dxpos_part_bytes(n, Fp) : 0);
    p.splits = choose_splits(Fp, Kp, n);
    p.part = take((size_t)(p.splits > min_splits ? p.splits : min_splits) * Fp * Kp * 4);
    p.tail_bytes = gemm_tail_ws_bytes();
    p.tail = take(p.tail_bytes);
    p.total = off;
    return p;
}

// A GCNLayer's weight gradient dW [Kp][Fop] = X^T d_hw has its SHORT side first (Kp = 320 rows of 128-row tiles: 3 row panels, one of them
// half empty, x 64-wide column tiles: 96 us for 5.7 GFLOP on the training batch, 0.38 of the MFMA roof).  Its transpose
// dW^T [Fop][Kp] = d_hw^T X is the GAT layers' shape -- 128 x 160 tiles with LDS-direct operand copies (gemm_tn_lds_kernel) -- whenever Kp
// splits into 160-column tiles without more padding than 64-column ones; the slice reduction writes it back transposed.
// Returns the number of k-slices of that route, 0 = not eligible.
static int gcn_dwt_splits(int n, int Kp, int Fop) {
    if (n < 4096 || ((Kp + 159) / 160) * 160 > ((Kp + 63) / 64) * 64) return 0;
    const int tiles = ((Fop + 127) / 128) * ((Kp + 159) / 160);
    const int slots = 2 * device_cu_count();
    int S = slots / tiles;
    const int nkt = (n + GEMM_BK - 1) / GEMM_BK;
    if (S > nkt / 8) S = nkt / 8;                                   // >= 8 k-tiles per slice
    if (S > 64) S = 64;
    return S >= 2 ? S : 0;
}
// out[k][f] = sum_s part[s][f][k]   (k < rows, f < cols; part slices [Fop][ldp]; slices added in order).  A workgroup owns 8 f x 32 k
// elements, one per thread, sixteen slices' loads in flight (the first version -- 32 x 32 tiles, one load in flight -- took 72 us for 42 MB).
__global__ __launch_bounds__(256) void reduce_splits_transposed_kernel(const float* __restrict__ part, int S, long long stride, int rows, int cols,
                                                                        int ldp, float* __restrict__ out) {
    __shared__ float tile[8][33];
    const int f0 = blockIdx.x * 8, k0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int f = min(f0 + ty, cols - 1), k = min(k0 + tx, rows - 1);
    const float* p = part + (long long)f * ldp + k;
    float acc = 0.f;
    for (int s0 = 0; s0 < S; s0 += 16) {
        float v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = p[(long long)min(s0 + q, S - 1) * stride];
#pragma unroll
        for (int q = 0; q < 16; ++q) acc += (s0 + q < S) ? v[q] : 0.f;
    }
    tile[ty][tx] = acc;
    __syncthreads();
    const int kk = threadIdx.x >> 3, ff = threadIdx.x & 7;          // 32 k rows x 8 f: a row's 8 floats are consecutive in `out`
    if (k0 + kk < rows && f0 + ff < cols) out[(long long)(k0 + kk) * cols + f0 + ff] = tile[ff][kk];
}

}  // namespace txe
using namespace txe;
extern "C" {

int txe_gat_padded_k(int Kh, int Pd) { return round_up(Kh + Pd, 32); }
int txe_gat_padded_f(int H, int D) { return round_up(H * D + 2 * H, 128); }

// Wp [Fp][Kp] from fc.weight W [H*D][Kt], attn_l / attn_r [H*D]   (model_zoo.py:56,65-66)
int txe_gat_pack_weights(const float* W, const float* attn_l, const float* attn_r, int H, int D, int Kt, float* Wp, void* stream) {
    if (!W || !attn_l || !attn_r || !Wp || H < 1 || D < 1 || Kt < 1) return TXE_ERR_ARG;
    const int F = H * D, Fe = F + 2 * H, Fp = round_up(Fe, 128), Kp = round_up(Kt, 32);
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)Fp * Kp;
    hipLaunchKernelGGL(pack_w_kernel, dim3((int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048)), dim3(256), 0, s, W, F, Fe, Fp, Kt, Kp, Wp);
    hipLaunchKernelGGL(fold_attn_kernel, dim3((Kt + 63) / 64, 2 * H), dim3(64 * FOLD_DG), 0, s, W, (long long)Kt, Kt, attn_l, attn_r, H, D,
                       Wp + (long long)F * Kp, (long long)Kp);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

// Layer input in padded layout (model_zoo.py:214-215 `cat(h, Emb[pos])`).  h == NULL: the feature part [0, Kh) is already in
// place (written by the previous layer's aggregation), only the position-embedding and padding columns are filled.
int txe_gat_build_x(const float* h, long long ld_h, int n_nodes, int Kh, const int* pos, const float* P, int Pd, float* X, void* stream) {
    if (n_nodes < 0 || Kh < 1 || Pd < 0 || !X || (Pd > 0 && (!pos || !P))) return TXE_ERR_ARG;
    if (n_nodes == 0) return TXE_OK;
    const int Kp = round_up(Kh + Pd, 32);
    const long long n = (long long)n_nodes * (Kp - (h ? 0 : Kh));
    if (n == 0) return TXE_OK;
    hipLaunchKernelGGL(build_x_kernel, dim3((int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096)), dim3(256), 0, (hipStream_t)stream, h,
                       ld_h, pos, P, n_nodes, Kh, Pd, Kp, X);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

// txe_gat_build_x + txe_gat_pack_weights + txe_dropout_mask (over the [n_nodes][Kh+Pd] layer input; feat_drop_p == 0: mask may be NULL)
// as ONE launch -- the per-layer preparation of GATLayer.forward (model_zoo.py:80-85) costs one dispatch instead of four.
int txe_gat_layer_prepare(const float* h, long long ld_h, int n_nodes, int Kh, const int* pos, const float* P, int Pd, float* X,
                          const float* W, const float* attn_l, const float* attn_r, int H, int D, float* Wp, float feat_drop_p,
                          unsigned long long seed, unsigned* mask, void* stream) {
    if (n_nodes < 0 || Kh < 1 || Pd < 0 || !X || (Pd > 0 && (!pos || !P)) || !W || !attn_l || !attn_r || !Wp || H < 1 || D < 1)
        return TXE_ERR_ARG;
    if (feat_drop_p < 0.f || feat_drop_p >= 1.f || (feat_drop_p > 0.f && !mask)) return TXE_ERR_ARG;
    const int T = 64 * FOLD_DG;
    PrepArgs a;
    memset(&a, 0, sizeof(a));
    a.Kt = Kh + Pd; a.Kp = round_up(a.Kt, 32);
    a.F = H * D; a.Fe = a.F + 2 * H; a.Fp = round_up(a.Fe, 128);
    auto blocks = [&](long long n, int cap) { const long long b = (n + T - 1) / T; return (int)(b < cap ? b : cap); };
    const long long nx = (long long)n_nodes * (a.Kp - (h ? 0 : Kh));
    a.nb_x = nx > 0 ? build_x_blocks(T, n_nodes, Kh, Pd, a.Kp, h != nullptr, false, 2048) : 0;
    a.n_words = (feat_drop_p > 0.f) ? (long long)n_nodes * ((a.Kt + 31) / 32) : 0;
    a.nb_m = blocks(a.n_words, 1024);
    a.nb_w = blocks(((long long)a.Fp * a.Kp / 4 + PREP_U - 1) / PREP_U, 512);   // PREP_U quads per thread
    a.fold_bx = (a.Kt + 63) / 64;
    a.nb_f = a.fold_bx * 2 * H;
    a.h = h; a.ld_h = ld_h; a.pos = pos; a.P = P; a.n_rows = n_nodes; a.Kh = Kh; a.Pd = Pd; a.X = X;
    a.W = W; a.attn_l = attn_l; a.attn_r = attn_r; a.H = H; a.D = D; a.Wp = Wp;
    a.pk_rows = a.F; a.pk_ext = a.Fe; a.pk_prows = a.Fp; a.pk_cols = a.Kt; a.pk_pcols = a.Kp;
    a.seed = seed; a.thr16 = (unsigned)(feat_drop_p * 65536.0f + 0.5f); a.mask = mask;
    a.x_dropped = 0; a.drop_scale = 1.f;                                  // (this entry leaves the dropout to the GEMM loaders)
    hipLaunchKernelGGL(gat_prepare_kernel, dim3(a.nb_x + a.nb_m + a.nb_w + a.nb_f), dim3(T), 0, (hipStream_t)stream, a);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

// txe_gat_layer_prepare for ALL GATLayers of a stack in ONE launch: everything a layer needs before its projection -- packed weights,
// folded attention rows, keep mask, the position-embedding / padding columns of its input -- depends on the parameters and on `pos`
// only, never on the layer below's output, so the whole stack can be prepared before the first GEMM (one dispatch instead of one per
// layer; the feature columns of the deeper layers' inputs are written later by the aggregation below them).
}  // extern "C"
namespace txe {
constexpr int PREP_MAXL = 4;
struct PrepMulti {
    int n; int nb_end[PREP_MAXL]; PrepArgs a[PREP_MAXL];
    int nb_norm; const int* norm_rowptr; int norm_n; float* norm;   // GCN stacks: norm = in_degree^-1/2 (model_zoo.py:157-161) by leading workgroups
};
__global__ __launch_bounds__(64 * FOLD_DG) void gat_prepare_multi_kernel(const PrepMulti m) {
    int b = blockIdx.x, i = 0;
    if (b < m.nb_norm) {
        const int v = b * (64 * FOLD_DG) + threadIdx.x;
        if (v < m.norm_n) { const int deg = m.norm_rowptr[v + 1] - m.norm_rowptr[v]; m.norm[v] = deg > 0 ? 1.0f / sqrtf((float)deg) : 0.f; }
        return;
    }
    b -= m.nb_norm;
    while (i + 1 < m.n && b >= m.nb_end[i]) ++i;                    // (block-uniform)
    prepare_jobs(m.a[i], b - ((i > 0) ? m.nb_end[i - 1] : 0));
}
// (measured on the 18 k-node training batch, 35 us layer after layer: the VALU-bound mask jobs and the streaming jobs dealt
//  alternately, one of each per CU: 40.5 us; JOB-major order over the layers -- folds, build_x, packs, masks: 35.9 us, and 150
//  against 138 us on the 1.1 M-node inference batch; the deeper layers' preparation on the second stream under the first
//  projection GEMM: the step unchanged -- its workgroups crawl beside the persistent GEMM's and that GEMM loses what was gained)
static int fill_prep(PrepArgs& a, const txe_gat_prepare_desc& d) {
    // (X == NULL: the layer's input is not stored -- txe_gat_dense_fwd_split_src forms it from h; mask and weights are still written)
    if (d.n_nodes < 0 || d.Kh < 1 || d.Pd < 0 || (!d.X && !d.h) || (d.Pd > 0 && (!d.pos || !d.P)) || !d.W || !d.attn_l || !d.attn_r || !d.Wp || d.H < 1 ||
        d.D < 1 || d.feat_drop_p < 0.f || d.feat_drop_p >= 1.f || (d.feat_drop_p > 0.f && !d.mask))
        return TXE_ERR_ARG;
    const int T = 64 * FOLD_DG;
    a.Kt = d.Kh + d.Pd; a.Kp = round_up(a.Kt, 32);
    a.F = d.H * d.D; a.Fe = a.F + 2 * d.H; a.Fp = round_up(a.Fe, 128);
    auto blocks = [&](long long n, int cap) { const long long b = (n + T - 1) / T; return (int)(b < cap ? b : cap); };
    const long long nx = d.X ? (long long)d.n_nodes * (a.Kp - (d.h ? 0 : d.Kh)) : 0;
    a.seed = d.seed; a.thr16 = (unsigned)(d.feat_drop_p * 65536.0f + 0.5f); a.mask = d.mask;
    a.x_dropped = (d.x_dropped && d.feat_drop_p > 0.f && a.thr16 != 0u) ? 1 : 0;
    a.x_mask = (a.x_dropped && d.h != nullptr && nx > 0) ? 1 : 0;     // build_x hashes every word of its rows anyway: it writes the mask
    a.drop_scale = 1.f / (1.f - d.feat_drop_p);
    a.nb_x = nx > 0 ? build_x_blocks(T, d.n_nodes, d.Kh, d.Pd, a.Kp, d.h != nullptr, a.x_dropped != 0, 2048) : 0;
    a.n_words = (d.feat_drop_p > 0.f) ? (long long)d.n_nodes * ((a.Kt + 31) / 32) : 0;
    a.nb_m = a.x_mask ? 0 : blocks(a.n_words, 1024);
    a.nb_w = blocks(((long long)a.Fp * a.Kp / 4 + PREP_U - 1) / PREP_U, 512);
    a.fold_bx = (a.Kt + 63) / 64;
    a.nb_f = a.fold_bx * 2 * d.H;
    a.h = d.h; a.ld_h = d.ld_h; a.pos = d.pos; a.P = d.P; a.n_rows = d.n_nodes; a.Kh = d.Kh; a.Pd = d.Pd; a.X = d.X;
    a.W = d.W; a.attn_l = d.attn_l; a.attn_r = d.attn_r; a.H = d.H; a.D = d.D; a.Wp = d.Wp;
    a.pk_rows = a.F; a.pk_ext = a.Fe; a.pk_prows = a.Fp; a.pk_cols = a.Kt; a.pk_pcols = a.Kp;
    return TXE_OK;
}
}  // namespace txe
extern "C" {
int txe_gat_layers_prepare(const struct txe_gat_prepare_desc* descs, int n_layers, void* stream) {
    if (!descs || n_layers < 1) return TXE_ERR_ARG;
    for (int i0 = 0; i0 < n_layers; i0 += PREP_MAXL) {              // (more than PREP_MAXL layers: several launches)
        PrepMulti m;
        memset(&m, 0, sizeof(m));
        m.n = n_layers - i0 < PREP_MAXL ? n_layers - i0 : PREP_MAXL;
        int total = 0;
        for (int i = 0; i < m.n; ++i) {
            const int rc = fill_prep(m.a[i], descs[i0 + i]);
            if (rc) return rc;
            total += m.a[i].nb_x + m.a[i].nb_m + m.a[i].nb_w + m.a[i].nb_f;
            m.nb_end[i] = total;
        }
        if (total == 0) continue;
        hipLaunchKernelGGL(gat_prepare_multi_kernel, dim3(total), dim3(64 * FOLD_DG), 0, (hipStream_t)stream, m);
        TXE_CHECK_LAUNCH();
    }
    return TXE_OK;
}

// The same for a GCNLayer (model_zoo.py:35-37): txe_gat_build_x + txe_gcn_pack_weights + txe_dropout_mask in one launch.
// W [Kh+Pd][Fo] -> Wp [roundup(roundup(Kh+Pd,32),128)][roundup(Fo,32)]; mask may be NULL when drop_p == 0.
}  // extern "C"
namespace txe {
static int fill_prep_gcn(PrepArgs& a, const txe_gcn_prepare_desc& d) {
    // bias_row (or NULL): packed as row Kh + Pd of Wp (needs a padding row: (Kh + Pd) % 32 != 0) -- the folded output layer then carries
    // its bias as the weight row of a column of Z that counts as 1 (txe_bilinear_folded_*: one_col)
    if (d.n_nodes < 0 || d.Kh < 1 || d.Pd < 0 || !d.X || (d.Pd > 0 && (!d.pos || !d.P)) || !d.W || !d.Wp || d.Fo < 1) return TXE_ERR_ARG;
    if (d.bias_row && ((d.Kh + d.Pd) % 32) == 0) return TXE_ERR_ARG;
    if (d.drop_p < 0.f || d.drop_p >= 1.f || (d.drop_p > 0.f && !d.mask)) return TXE_ERR_ARG;
    const int T = 64 * FOLD_DG;
    memset(&a, 0, sizeof(a));
    a.Kt = d.Kh + d.Pd; a.Kp = round_up(a.Kt, 32);
    auto blocks = [&](long long n, int cap) { const long long b = (n + T - 1) / T; return (int)(b < cap ? b : cap); };
    const long long nx = (long long)d.n_nodes * (a.Kp - (d.h ? 0 : d.Kh));
    a.seed = d.seed; a.thr16 = (unsigned)(d.drop_p * 65536.0f + 0.5f); a.mask = d.mask;
    a.x_dropped = (d.x_dropped && d.drop_p > 0.f && a.thr16 != 0u) ? 1 : 0;      // (as txe_gat_prepare_desc.x_dropped)
    a.x_mask = (a.x_dropped && d.h != nullptr && nx > 0) ? 1 : 0;
    a.drop_scale = 1.f / (1.f - d.drop_p);
    a.nb_x = nx > 0 ? build_x_blocks(T, d.n_nodes, d.Kh, d.Pd, a.Kp, d.h != nullptr, a.x_dropped != 0, 2048) : 0;
    a.n_words = (d.drop_p > 0.f) ? (long long)d.n_nodes * ((a.Kt + 31) / 32) : 0;
    a.nb_m = a.x_mask ? 0 : blocks(a.n_words, 1024);
    a.pk_rows = a.Kt; a.pk_ext = a.Kt; a.pk_prows = round_up(a.Kp, 128); a.pk_cols = d.Fo; a.pk_pcols = round_up(d.Fo, 32);
    a.nb_w = blocks(((long long)a.pk_prows * a.pk_pcols / 4 + PREP_U - 1) / PREP_U, 512);
    a.nb_f = 0; a.fold_bx = 1;
    a.h = d.h; a.ld_h = d.ld_h; a.pos = d.pos; a.P = d.P; a.n_rows = d.n_nodes; a.Kh = d.Kh; a.Pd = d.Pd; a.X = d.X;
    a.W = d.W; a.Wp = d.Wp; a.pk_extra = d.bias_row;
    return TXE_OK;
}
}  // namespace txe
extern "C" {
int txe_gcn_layer_prepare(const float* h, long long ld_h, int n_nodes, int Kh, const int* pos, const float* P, int Pd, float* X,
                          const float* W, int Fo, float* Wp, float drop_p, unsigned long long seed, unsigned* mask, int x_dropped,
                          const float* bias_row, void* stream) {
    const txe_gcn_prepare_desc d{h, ld_h, n_nodes, Kh, pos, P, Pd, X, W, Fo, Wp, drop_p, seed, mask, x_dropped, bias_row};
    PrepArgs a;
    const int rc = fill_prep_gcn(a, d);
    if (rc) return rc;
    hipLaunchKernelGGL(gat_prepare_kernel, dim3(a.nb_x + a.nb_m + a.nb_w), dim3(64 * FOLD_DG), 0, (hipStream_t)stream, a);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

// ... for every GCNLayer of a stack in ONE launch (a layer's preparation never depends on the layer below's output), together with the
// stack's degree normalisation norm[v] = in_degree(v)^-1/2 (txe_gcn_norm; rowptr_in == NULL: without it)
int txe_gcn_layers_prepare(const struct txe_gcn_prepare_desc* descs, int n_layers, const int* rowptr_in, int n_nodes, float* norm, void* stream) {
    if (!descs || n_layers < 1 || (rowptr_in && (n_nodes < 0 || !norm))) return TXE_ERR_ARG;
    for (int i0 = 0; i0 < n_layers; i0 += PREP_MAXL) {
        PrepMulti m;
        memset(&m, 0, sizeof(m));
        m.n = n_layers - i0 < PREP_MAXL ? n_layers - i0 : PREP_MAXL;
        if (i0 == 0 && rowptr_in && n_nodes > 0) {
            m.nb_norm = (n_nodes + 64 * FOLD_DG - 1) / (64 * FOLD_DG); m.norm_rowptr = rowptr_in; m.norm_n = n_nodes; m.norm = norm;
        }
        int total = 0;
        for (int i = 0; i < m.n; ++i) {
            const int rc = fill_prep_gcn(m.a[i], descs[i0 + i]);
            if (rc) return rc;
            total += m.a[i].nb_x + m.a[i].nb_m + m.a[i].nb_w;
            m.nb_end[i] = total;
        }
        if (total + m.nb_norm == 0) continue;
        hipLaunchKernelGGL(gat_prepare_multi_kernel, dim3(total + m.nb_norm), dim3(64 * FOLD_DG), 0, (hipStream_t)stream, m);
        TXE_CHECK_LAUNCH();
    }
    return TXE_OK;
}

// Eval-mode layer-0 projection of a batch drawn from a feature table (SURVEY 8f-2 "dedup by _id"): Y[v] = T[row[v]] + T2[row2[v]],
// n_cols a multiple of 4, 16-byte aligned rows.  T2 / row2 may be NULL.
int txe_gather_add_rows(const float* T, long long ld_t, const int* row, const float* T2, long long ld_t2, const int* row2, long long n_rows,
                        int n_cols, float* Y, long long ld_y, void* stream) {
    if (n_rows < 0 || n_cols < 4 || (n_cols & 3) || !T || !row || !Y || (T2 && !row2) || (ld_t & 3) || (ld_y & 3) || (T2 && (ld_t2 & 3)))
        return TXE_ERR_ARG;
    if ((((uintptr_t)T | (uintptr_t)Y | (uintptr_t)T2) & 15) != 0) return TXE_ERR_ARG;
    if (n_rows == 0) return TXE_OK;
    const int nvec = n_cols / 4;
    const long long total = n_rows * nvec;
    const int nb = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    ProfScope prof("gather_add_rows_kernel", (hipStream_t)stream, 4.0 * 2.0 * n_rows * (double)n_cols, 1);     // read a row, write a row
    hipLaunchKernelGGL(gather_add_rows_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, T, ld_t, row, T2, ld_t2, row2, n_rows, nvec, Y, ld_y);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

// 1: txe_gat_dense_bwd forms this layer's d_X with the streaming position-column kernel (phase 1 is then an HBM stream that belongs
// IN LINE on the caller's stream, not beside the weight-gradient product on a second one)
int txe_gat_dx_streams(int Kh, int Pd, int need_dh) {
    if (need_dh || Pd < 1 || Kh < 1) return 0;
    const int c0 = (Kh / 4) * 4;
    return (Kh + Pd - c0 <= DXPOS_MAXC && Kh - c0 + Pd <= DXPOS_MAXC) ? 1 : 0;
}

// extra workspace (behind txe_gat_dense_ws_bytes) with which txe_gat_dense_bwd forms a need_dh layer's d_X on the bf16 pipe
static inline size_t dense_bwd_split_bytes(int n_nodes, int Fp, int Kt) {
    return align_up(split_packed_bytes(n_nodes, Fp), 256) + align_up(split_packed_bytes(Kt, Fp), 256);
}
size_t txe_gat_dense_bwd_split_ws_bytes(int n_nodes, int Kh, int Pd, int H, int D) {
    if (n_nodes < 1 || Kh < 1 || Pd < 0 || H < 1 || D < 1) return 0;
    return dense_bwd_split_bytes(n_nodes, round_up(H * D + 2 * H, 128), Kh + Pd);
}
size_t txe_gat_dense_ws_bytes(int n_nodes, int Kh, int Pd, int H, int D, int vocab) {
    return plan_dense_ws(nullptr, n_nodes, round_up(H * D + 2 * H, 128), 2 * H, round_up(Kh + Pd, 32), Pd, vocab).total;
}

// Y [N][Fp] = dropout(X) [N][Kp] * Wp^T      (model_zoo.py:82-85: feat_drop, fc, a1, a2 in one product)
int txe_gat_dense_fwd(const float* X, int n_nodes, int Kh, int Pd, const float* Wp, int H, int D, float feat_drop_p,
                      const unsigned* mask, float* Y, void* ws, size_t ws_bytes, void* stream) {
    if (n_nodes < 0 || Kh < 1 || Pd < 0 || H < 1 || D < 1 || !X || !Wp || !Y) return TXE_ERR_ARG;
    if (feat_drop_p < 0.f || feat_drop_p >= 1.f) return TXE_ERR_ARG;
    if (n_nodes == 0) return TXE_OK;
    const int Fe = H * D + 2 * H, Fp = round_up(Fe, 128), Kp = round_up(Kh + Pd, 32);
    VMat A = vmat_plain(X, Kp, n_nodes, Kp);
    vmat_set_mask(A, mask, feat_drop_p);
    VMat B = vmat_plain(Wp, Kp, Fp, Kp);
    Epi E = epi_plain(Y, Fp, Fe);
    E.alg_flops = 2.0 * n_nodes * (double)Fe * (Kh + Pd);           // without the k-tile padding of X / Wp
    E.k_valid = Kh + Pd;                                             // (X and Wp carry zeros behind it: txe_gat_layers_prepare / pack_w)
    const bool tail_ok = ws && ws_bytes >= gemm_tail_ws_bytes();
    return gemm_nt(A, B, E, n_nodes, Fe, Kp, 1, (hipStream_t)stream, tail_ok ? ws : nullptr, tail_ok ? ws_bytes : 0);
}

// The same product on the bf16 matrix pipe (txe_gemm_split.h: three bf16 planes per fp32 operand, six plane products, fp32
// accumulation -- fp32 accuracy at 6/16 of the fp32 MFMA's time).  X is a PLAIN operand here: dropout(X) already applied
// (txe_gat_prepare_desc.x_dropped) or no dropout.  Xs / Ws: the packed planes of X (side 0) / Wp (side 1) when the preparation launch
// wrote them, else NULL -- they are then packed here, into ws.  Xt_out (or NULL): txe_gat_dense_split_xt_bytes for X packed
// contraction-major, what txe_gat_dense_bwd's weight gradient takes on the same pipe.
size_t txe_gat_dense_split_ws_bytes(int n_nodes, int Kh, int Pd, int H, int D) {
    if (n_nodes < 1 || Kh < 1 || Pd < 0 || H < 1 || D < 1) return 0;
    const int Fp = round_up(H * D + 2 * H, 128), Kp = round_up(Kh + Pd, 32);
    return align_up(split_packed_bytes(n_nodes, Kp), 256) + align_up(split_packed_bytes(Fp, Kp), 256);
}
size_t txe_gat_dense_split_xt_bytes(int n_nodes, int Kh, int Pd, int H, int D) {       // 0: this layer's weight gradient keeps the fp32 route
    if (n_nodes < 1 || Kh < 1 || Pd < 0 || H < 1 || D < 1) return 0;
    const int Fp = round_up(H * D + 2 * H, 128), Kp = round_up(Kh + Pd, 32);
    return (split_tn_eligible(Fp, Kp) && split_tn_fits(n_nodes, Fp)) ? split_packed_t_bytes(n_nodes, Kp) : 0;
}
int txe_gat_dense_fwd_split(const float* X, int n_nodes, int Kh, int Pd, const float* Wp, int H, int D, const void* Xs, const void* Ws,
                            void* Xt_out, float* Y, void* ws, size_t ws_bytes, void* stream) {
    if (n_nodes < 0 || Kh < 1 || Pd < 0 || H < 1 || D < 1 || !Y || (!Xs && !X) || (!Ws && !Wp)) return TXE_ERR_ARG;
    if (n_nodes == 0) return TXE_OK;
    const int Fe = H * D + 2 * H, Fp = round_up(Fe, 128), Kp = round_up(Kh + Pd, 32);
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    size_t off = 0;
    int rc;
    if (Xt_out && (!X || !split_tn_eligible(Fp, Kp))) return TXE_ERR_ARG;
    bool xt_done = false;
    // the contraction runs over whole k-tiles of 16: Kc columns (X and Wp hold zeros in [Kh + Pd, Kp))
    const int Kc = round_up(Kh + Pd, 16);
    if (!Xs && !Ws) {                                   // the usual case: all three packs in one launch
        const size_t ba = align_up(split_packed_bytes(n_nodes, Kp), 256), bb = align_up(split_packed_bytes(Fp, Kp), 256);
        if (!ws || ws_bytes < ba + bb) return TXE_ERR_WORKSPACE;
        rc = split_pack_layer_launch(X, Kp, n_nodes, Wp, Kp, Fp, Kc, Kp, w, w + ba, Xt_out, s);
        if (rc) return rc;
        Xs = w; Ws = w + ba; xt_done = true;
    }
    if (!Xs) {
        const size_t b = align_up(split_packed_bytes(n_nodes, Kp), 256);
        if (!ws || ws_bytes < off + b) return TXE_ERR_WORKSPACE;
        rc = split_pack_launch(X, Kp, n_nodes, Kc, 0, w + off, s);
        if (rc) return rc;
        Xs = w + off; off += b;
    }
    if (!Ws) {
        const size_t b = align_up(split_packed_bytes(Fp, Kp), 256);
        if (!ws || ws_bytes < off + b) return TXE_ERR_WORKSPACE;
        rc = split_pack_launch(Wp, Kp, Fp, Kc, 1, w + off, s);
        if (rc) return rc;
        Ws = w + off; off += b;
    }
    rc = gemm_nt_split_launch(Xs, Ws, n_nodes, Fe, Kc, Y, Fp, 2.0 * n_nodes * (double)Fe * (Kh + Pd), s);
    if (rc) return rc;
    // (X packed contraction-major for the backward pass's weight gradient, txe_gat_dense_bwd: Xt)
    if (Xt_out && !xt_done) return split_pack_t_launch(X, Kp, n_nodes, Kp, Xt_out, s);
    return TXE_OK;
}

// The same product for a FIRST layer whose input X = dropout([h | Emb[pos]]) is never stored: the packs form its elements from h, the
// position table and the keep mask (txe_gat_layers_prepare with X == NULL writes mask and weights only) -- one 23-MB write and two reads
// of it less per step on the training batch.  mask == NULL or feat_drop_p == 0: no dropout.
int txe_gat_dense_fwd_split_src(const float* h, long long ld_h, const int* pos, const float* P, const unsigned* mask, float feat_drop_p,
                                int n_nodes, int Kh, int Pd, const float* Wp, int H, int D, void* Xt_out, float* Y, void* ws, size_t ws_bytes,
                                void* stream) {
    if (n_nodes < 0 || Kh < 1 || Pd < 0 || H < 1 || D < 1 || !Y || !h || !Wp || ld_h < Kh || (Pd > 0 && (!pos || !P)) || feat_drop_p < 0.f ||
        feat_drop_p >= 1.f || (feat_drop_p > 0.f && !mask))
        return TXE_ERR_ARG;
    if (n_nodes == 0) return TXE_OK;
    const int Fe = H * D + 2 * H, Fp = round_up(Fe, 128), Kp = round_up(Kh + Pd, 32);
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    if (Xt_out && !split_tn_eligible(Fp, Kp)) return TXE_ERR_ARG;
    const int Kc = round_up(Kh + Pd, 16);
    const size_t ba = align_up(split_packed_bytes(n_nodes, Kp), 256), bb = align_up(split_packed_bytes(Fp, Kp), 256);
    if (!ws || ws_bytes < ba + bb) return TXE_ERR_WORKSPACE;
    SplitVSrc vs{h, ld_h, pos, P, Kh, Pd, feat_drop_p > 0.f ? mask : nullptr, (Kh + Pd + 31) / 32, 1.f / (1.f - feat_drop_p)};
    int rc = split_pack_layer_launch(nullptr, Kp, n_nodes, Wp, Kp, Fp, Kc, Kp, w, w + ba, Xt_out, s, &vs);
    if (rc) return rc;
    return gemm_nt_split_launch(w, w + ba, n_nodes, Fe, Kc, Y, Fp, 2.0 * n_nodes * (double)Fe * (Kh + Pd), s);
}

// Backward of txe_gat_dense_fwd.  d_Y [N][Fp] must have ZERO padding columns [F+2H, Fp).
//   d_X [N][Kp]: columns [c0, Kt) are written, c0 = 0 if need_dh else the 32-aligned start of the position columns;
//                columns < Kh are multiplied by leaky'(X) when act_slope_on (X[:, :Kh] is then the activated output of the
//                previous layer), all by the dropout factor.
//   dW [F][Kt], d_attn_l / d_attn_r [F], dP [vocab][Pd].
// phases: TXE_DENSE_ALL = everything; _DX = d_X, _DW = the dW GEMM (independent of each other), _REDUCE = the reductions that need both -- separate calls
// share the workspace.  phases | TXE_DENSE_DX_SPLIT: the full d_X product (need_dh) runs on the bf16 matrix pipe, its packed operands behind the workspace
// (ws_bytes >= txe_gat_dense_ws_bytes + txe_gat_dense_bwd_split_ws_bytes, else TXE_ERR_WORKSPACE); without the bit: the fp32 MFMA.
int txe_gat_dense_bwd(const float* X, int n_nodes, int Kh, int Pd, const int* pos, int vocab, const float* Wp, const float* W,
                      const float* attn_l, const float* attn_r, int H, int D, float feat_drop_p, const unsigned* mask, const float* d_Y,
                      int need_dh, int act_on, float act_slope, float* d_X, float* dW, float* d_attn_l, float* d_attn_r, float* dP,
                      int x_dropped, const void* Xt, int phases, void* chain, void* ws, size_t ws_bytes, void* stream) {
    // (X == NULL: a first layer whose input was never stored, txe_gat_dense_fwd_split_src -- its weight gradient needs Xt then)
    if (n_nodes < 0 || Kh < 1 || Pd < 0 || H < 1 || D < 1 || (!X && (!Xt || act_on)) || !Wp || !W || !attn_l || !attn_r || !d_Y || !dW || !d_attn_l || !d_attn_r || !ws)
        return TXE_ERR_ARG;
    static_assert(sizeof(TailChain) <= TXE_TAIL_CHAIN_BYTES, "txe.h: TXE_TAIL_CHAIN_BYTES");
    if ((need_dh || Pd > 0) && !d_X) return TXE_ERR_ARG;
    if (Pd > 0 && (!pos || !dP || vocab < 1 || vocab > MAX_VOCAB)) return TXE_ERR_ARG;
    if (feat_drop_p < 0.f || feat_drop_p >= 1.f) return TXE_ERR_ARG;
    const int F = H * D, H2 = 2 * H, Fe = F + H2, Fp = round_up(Fe, 128), Kt = Kh + Pd, Kp = round_up(Kt, 32);
    DenseWs p = plan_dense_ws(ws, n_nodes, Fp, H2, Kp, Pd, vocab);
    if (ws_bytes < p.total) return TXE_ERR_WORKSPACE;
    // (every rejection in front of the first launch: the bf16 d_X route's workspace, and a weight gradient that would take the fp32
    //  product without a stored X)
    if ((phases & TXE_DENSE_DX) && (phases & TXE_DENSE_DX_SPLIT) && need_dh && n_nodes > 0 && ws_bytes < p.total + dense_bwd_split_bytes(n_nodes, Fp, Kt))
        return TXE_ERR_WORKSPACE;                                   // (the route is the caller's choice, not the buffer's size)
    const bool dw_split = Xt && x_dropped + (feat_drop_p == 0.f) > 0 && split_tn_eligible(Fp, Kp) && split_tn_fits(n_nodes, Fp) && n_nodes > 0;
    if ((phases & TXE_DENSE_DW) && !dw_split && !X) return TXE_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    // ---- d_X[:, c0:Kt] = d_Y * Wp[:, c0:Kt] ----
    const int c0 = need_dh ? 0 : (Kh / 4) * 4;      // 16-byte aligned start of the position columns
    // position columns only: one stream over d_Y (txe_dxpos.hip) that also leaves the per-class partial sums of dP
    const bool stream_dx = txe_gat_dx_streams(Kh, Pd, need_dh) == 1 && n_nodes > 0;
    DxPosArgs da;
    memset(&da, 0, sizeof(da));
    if (stream_dx) {
        da.dY = d_Y; da.ld_dy = Fp; da.n_rows = n_nodes; da.K = Fp;
        da.Wp = Wp; da.ld_w = Kp; da.Kp = Kp; da.c0 = c0; da.NC = Kt - c0;
        da.mask = mask; da.mask_ld = (Kt + 31) / 32; da.mask_on = (mask && feat_drop_p > 0.f) ? 1 : 0;
        da.drop_scale = da.mask_on ? 1.f / (1.f - feat_drop_p) : 1.f;
        da.dX = d_X; da.ld_dx = Kp;
        da.pos = pos; da.vocab = vocab; da.Pd = Pd; da.pcol0 = Kh - c0; da.ppart = p.ppart; da.part = p.dxpart;
        rc = dxpos_prepare(da);
        if (rc) return rc;
    }
    if ((phases & TXE_DENSE_DX) && stream_dx) {
        rc = dxpos_launch(da, s);
        if (rc) return rc;
    } else if ((phases & TXE_DENSE_DX) && (phases & TXE_DENSE_DX_SPLIT) && need_dh && n_nodes > 0) {
        // the whole d_X = d_Y Wp on the bf16 pipe (txe_gemm_split.h): d_Y packed as the row operand, Wp -- given as the transpose of
        // the column operand -- packed from its columns; dropout mask and leaky' factor in the store loop (epi_store_one's arithmetic)
        char* sw = (char*)ws + p.total;
        const size_t ba = align_up(split_packed_bytes(n_nodes, Fp), 256);
        const int Fc = round_up(Fe, 16);                 // whole k-tiles of 16 over the contraction (d_Y's columns past Fe are zeros)
        rc = split_pack_launch(d_Y, Fp, n_nodes, Fc, 0, sw, s);
        if (rc) return rc;
        rc = split_pack_launch(Wp, Kp, Kt, Fc, 3, sw + ba, s);
        if (rc) return rc;
        SplitEpi e;
        memset(&e, 0, sizeof(e));
        e.drop_scale = 1.f;
        if (mask && feat_drop_p > 0.f) { e.mask = mask; e.mask_ld = (Kt + 31) / 32; e.mask_col0 = 0; e.drop_scale = 1.f / (1.f - feat_drop_p); }
        if (act_on) { e.act_src = X; e.ld_act = Kp; e.act_slope = act_slope; e.cols_act = Kh; }
        rc = gemm_nt_split_launch(sw, sw + ba, n_nodes, Kt, Fc, d_X, Kp, 2.0 * n_nodes * (double)Kt * Fe, s, &e);
        if (rc) return rc;
    } else if ((phases & TXE_DENSE_DX) && Kt - c0 > 0 && n_nodes > 0 && (need_dh || Pd > 0)) {
        VMat A = vmat_plain(d_Y, Fp, n_nodes, Fp);
        VMat B = vmat_plain(Wp + c0, Kp, Fp, Kp - c0);
        Epi E = epi_plain(d_X + c0, Kp, Kh > c0 ? Kh - c0 : 0);
        E.c2 = d_X + c0 + E.cols_main; E.ldc2 = Kp;                 // same buffer: the split only scopes the activation factor
        epi_set_mask(E, mask, Kt, c0, feat_drop_p);
        if (act_on && need_dh) epi_set_act(E, X + c0, Kp, act_slope);
        E.alg_flops = 2.0 * n_nodes * (double)(need_dh ? Kt : Pd) * Fe;
        rc = gemm_nn(A, B, E, n_nodes, Kt - c0, Fp, 1, s, p.tail, p.tail_bytes);
        if (rc) return rc;
    }
    // ---- dWp = d_Y^T * dropout(X)  (split-K over the node dimension) ----
    VMat A = vmat_plain(d_Y, Fp, n_nodes, Fp);
    VMat B = vmat_plain(X, Kp, n_nodes, Kp);
    if (!x_dropped) vmat_set_mask(B, mask, feat_drop_p);            // (x_dropped: X already holds dropout(X), txe_gat_layers_prepare)
    Epi E = epi_plain(p.part, Kp, Kp);
    E.split_stride = (long long)Fp * Kp;
    E.alg_flops = 2.0 * Fe * (double)Kt * n_nodes;
    const int splits = p.splits;
    if ((phases & TXE_DENSE_DW) && dw_split) {
        // the same slices on the bf16 pipe (txe_gemm_split.h): X packed contraction-major by the forward pass, d_Y split in the loader
        const int ks = round_up((n_nodes + splits - 1) / splits, 16);
        rc = gemm_tn_split_launch(d_Y, Fp, Fp, Xt, Kp, n_nodes, splits, ks, p.part, Kp, E.split_stride, E.alg_flops, s);
        if (rc) return rc;
    } else if (phases & TXE_DENSE_DW) {
        rc = gemm_tn(A, B, E, Fp, Kp, n_nodes, splits, s);
        if (rc) return rc;
    }
    if (!(phases & TXE_DENSE_REDUCE)) return TXE_OK;
    const int S = n_nodes > 0 ? splits : 0;
    // ---- phase A: dP partials (dP[c][j] = sum_{pos[m]==c} d_X[m][Kh+j]) and d_wa = the extension rows of dWp ----
    const int nseg = (Pd > 0 && n_nodes > 0) ? (stream_dx ? dxpos_blocks(n_nodes) : p.seg_blocks) : 0;
    TailA ta;
    memset(&ta, 0, sizeof(ta));
    ta.nb_dx = stream_dx ? nseg : 0; ta.dx = da;
    ta.nb_s1a = stream_dx ? 0 : nseg; ta.s1a = Seg1Args{d_X ? d_X + Kh : nullptr, (long long)Kp, Pd, p.ppart};
    ta.pos = pos; ta.n_rows = n_nodes; ta.vocab = vocab; ta.rows_per_block = p.seg_rows;
    ta.r_kind = 1; ta.nbx = (Kp + 255) / 256; ta.nb_r = ta.nbx * H2;
    ta.rpart = p.part; ta.S = S; ta.split_stride = E.split_stride; ta.F = F; ta.ldp = Kp; ta.dwa = p.dwa;
    rc = tail_a_launch(ta, s);
    if (rc) return rc;
    // ---- phase B: dW / d_attn (unfold) and dP ----
    TailB tb;
    memset(&tb, 0, sizeof(tb));
    tb.nb_u = F;
    tb.u = UnfoldArgs{p.part, S, E.split_stride, p.dwa, (long long)Kp, W, (long long)Kt, attn_l, attn_r, H, D, Kt, dW, (long long)Kt,
                      d_attn_l, d_attn_r};
    tb.nb_2a = Pd > 0 ? (vocab * Pd + 63) / 64 : 0;
    tb.s2a = Seg2Args{p.ppart, nseg, vocab * Pd, dP};
    return tail_b_submit(&tb, chain, (phases & TXE_PH_DEFER) != 0, s);
}

// launches whatever a chain of deferred phase-B jobs still holds (a stack whose last call deferred too); chain == NULL: nothing
int txe_gat_tail_flush(void* chain, void* stream) {
    if (!chain) return TXE_OK;
    return tail_b_submit(nullptr, chain, false, (hipStream_t)stream);
}

// zero columns [c0, c1) of a row-major fp32 matrix (padding columns of d_Y)
int txe_zero_cols(float* x, long long ld, int n_rows, int c0, int c1, void* stream) {
    if (!x || n_rows < 0 || c0 < 0 || c1 < c0) return TXE_ERR_ARG;
    const long long n = (long long)n_rows * (c1 - c0);
    if (n == 0) return TXE_OK;
    hipLaunchKernelGGL(zero_cols_kernel, dim3((int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048)), dim3(256), 0, (hipStream_t)stream, x, ld,
                       n_rows, c0, c1);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}


// ---------------------------------------------------------------------------------------------
// GCNLayer dense part (model_zoo.py:35-37) on padded operands:  hw = dropout(X) Wp,
//   X  [N][Kp]       as for GAT (txe_gat_build_x),
//   Wp [Kp128][Fop]  = weight [Kt][Fo] zero-padded, Kp128 = roundup(Kp,128), Fop = roundup(Fo,32),
//   hw / d_hw [N][Fop]  (d_hw with ZERO padding columns).
// ---------------------------------------------------------------------------------------------
int txe_gcn_padded_f(int Fo) { return round_up(Fo, 32); }

int txe_gcn_pack_weights(const float* W, int Kt, int Fo, float* Wp, void* stream) {
    if (!W || !Wp || Kt < 1 || Fo < 1) return TXE_ERR_ARG;
    const int Kp128 = round_up(round_up(Kt, 32), 128), Fop = round_up(Fo, 32);
    const long long n = (long long)Kp128 * Fop;
    // pack_w_kernel(W, F=rows, Fe=rows, Fp=padded rows, Kt=cols, Kp=padded cols)
    hipLaunchKernelGGL(pack_w_kernel, dim3((int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048)), dim3(256), 0, (hipStream_t)stream, W, Kt,
                       Kt, Kp128, Fo, Fop, Wp);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

size_t txe_gcn_dense_ws_bytes(int n_nodes, int Kh, int Pd, int Fo, int vocab) {
    const int Kp = round_up(Kh + Pd, 32), Fop = round_up(Fo, 32);
    return plan_dense_ws(nullptr, n_nodes, Kp, 0, Fop, Pd, vocab, false, gcn_dwt_splits(n_nodes, Kp, Fop)).total;
}

int txe_gcn_dense_fwd(const float* X, int n_nodes, int Kh, int Pd, const float* Wp, int Fo, float drop_p, const unsigned* mask,
                      float* hw, void* ws, size_t ws_bytes, void* stream) {
    if (n_nodes < 0 || Kh < 1 || Pd < 0 || Fo < 1 || !X || !Wp || !hw) return TXE_ERR_ARG;
    if (drop_p < 0.f || drop_p >= 1.f) return TXE_ERR_ARG;
    if (n_nodes == 0) return TXE_OK;
    const int Kp = round_up(Kh + Pd, 32), Fop = round_up(Fo, 32);
    VMat A = vmat_plain(X, Kp, n_nodes, Kp);
    vmat_set_mask(A, mask, drop_p);
    VMat B = vmat_plain(Wp, Fop, Kp, Fop);
    Epi E = epi_plain(hw, Fop, Fo);
    E.alg_flops = 2.0 * n_nodes * (double)Fo * (Kh + Pd);
    const bool tail_ok = ws && ws_bytes >= gemm_tail_ws_bytes();
    return gemm_nn(A, B, E, n_nodes, Fo, Kp, 1, (hipStream_t)stream, tail_ok ? ws : nullptr, tail_ok ? ws_bytes : 0);
}

// dW[k][f] = sum_s part[s][k][f]  (k < Kt, f < Fo; part rows have stride ldp)
__global__ void reduce_splits_sub_kernel(const float* __restrict__ part, int S, long long stride, int rows, int cols, int ldp,
                                         float* __restrict__ out) {
    const long long n = (long long)rows * cols;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / cols;
        const int c = (int)(i % cols);
        float acc = 0.f;
        for (int s = 0; s < S; ++s) acc += part[(long long)s * stride + r * ldp + c];
        out[i] = acc;
    }
}
}  // extern "C"
namespace txe {
int reduce_splits_sub_launch(const float* part, int S, long long stride, int rows, int cols, int ldp, float* out, hipStream_t s) {
    const long long n = (long long)rows * cols;
    hipLaunchKernelGGL(reduce_splits_sub_kernel, dim3((int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048)), dim3(256), 0, s, part, S, stride,
                       rows, cols, ldp, out);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}
}  // namespace txe
extern "C" {

// d_hw [N][Fop] with zero padding columns.  Writes d_X columns [c0, Kt) (as txe_gat_dense_bwd), dW [Kt][Fo], dP.
int txe_gcn_dense_bwd(const float* X, int n_nodes, int Kh, int Pd, const int* pos, int vocab, const float* Wp, int Fo, float drop_p,
                      const unsigned* mask, const float* d_hw, int need_dh, int act_on, float act_slope, float* d_X, float* dW,
                      float* dP, int x_dropped, void* ws, size_t ws_bytes, void* stream) {
    if (n_nodes < 0 || Kh < 1 || Pd < 0 || Fo < 1 || !X || !Wp || !d_hw || !dW || !ws) return TXE_ERR_ARG;
    if ((need_dh || Pd > 0) && !d_X) return TXE_ERR_ARG;
    if (Pd > 0 && (!pos || !dP || vocab < 1 || vocab > MAX_VOCAB)) return TXE_ERR_ARG;
    if (drop_p < 0.f || drop_p >= 1.f) return TXE_ERR_ARG;
    const int Kt = Kh + Pd, Kp = round_up(Kt, 32), Fop = round_up(Fo, 32);
    const int St = gcn_dwt_splits(n_nodes, Kp, Fop);
    DenseWs p = plan_dense_ws(ws, n_nodes, Kp, 0, Fop, Pd, vocab, false, St);   // part: [S][Kp][Fop] (or transposed: [St][Fop][Kp])
    if (ws_bytes < p.total) return TXE_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    const int c0 = need_dh ? 0 : (Kh / 4) * 4;
    if (Kt - c0 > 0 && n_nodes > 0 && (need_dh || Pd > 0)) {
        // d_X[m][c] = sum_f d_hw[m][f] * Wp[c][f]     (NT; Wp rows are padded to a multiple of 128, so every tile is plain)
        VMat A = vmat_plain(d_hw, Fop, n_nodes, Fop);
        VMat B = vmat_plain(Wp + (long long)c0 * Fop, Fop, round_up(Kp, 128) - c0, Fop);
        Epi E = epi_plain(d_X + c0, Kp, Kh > c0 ? Kh - c0 : 0);
        E.c2 = d_X + c0 + E.cols_main; E.ldc2 = Kp;
        epi_set_mask(E, mask, Kt, c0, drop_p);
        if (act_on && need_dh) epi_set_act(E, X + c0, Kp, act_slope);
        E.alg_flops = 2.0 * n_nodes * (double)(need_dh ? Kt : Pd) * Fo;
        rc = gemm_nt(A, B, E, n_nodes, Kt - c0, Fop, 1, s, p.tail, p.tail_bytes);
        if (rc) return rc;
    }
    if (Pd > 0) {
        rc = pos_segsum_launch(d_X + Kh, (long long)Kp, pos, n_nodes, Pd, vocab, p.seg_blocks, p.seg_rows, p.ppart, dP, s);
        if (rc) return rc;
    }
    if (St > 0 && (x_dropped || !mask || drop_p <= 0.f)) {
        // dW^T [Fop][Kp] = d_hw^T X on 128 x 160 tiles (gcn_dwt_splits), written back transposed by the slice reduction
        VMat A = vmat_plain(d_hw, Fop, n_nodes, Fop);
        VMat B = vmat_plain(X, Kp, n_nodes, Kp);
        Epi E = epi_plain(p.part, Kp, Kp);
        E.split_stride = (long long)Fop * Kp;
        E.alg_flops = 2.0 * Kt * (double)Fo * n_nodes;
        E.route |= GEMM_ROUTE_FORCE_BN160;
        rc = gemm_tn(A, B, E, Fop, Kp, n_nodes, St, s);
        if (rc) return rc;
        hipLaunchKernelGGL(reduce_splits_transposed_kernel, dim3((Fo + 7) / 8, (Kt + 31) / 32), dim3(256), 0, s, (const float*)p.part, St,
                           E.split_stride, Kt, Fo, Kp, dW);
        TXE_CHECK_LAUNCH();
    } else {   // dWp[k][f] = sum_m dropout(X)[m][k] * d_hw[m][f]
        VMat A = vmat_plain(X, Kp, n_nodes, Kp);
        if (!x_dropped) vmat_set_mask(A, mask, drop_p);             // (x_dropped: X already holds dropout(X), txe_gcn_layer_prepare)
        VMat B = vmat_plain(d_hw, Fop, n_nodes, Fop);
        Epi E = epi_plain(p.part, Fop, Fop);
        E.split_stride = (long long)Kp * Fop;
        E.alg_flops = 2.0 * Kt * (double)Fo * n_nodes;
        rc = gemm_tn(A, B, E, Kp, Fop, n_nodes, p.splits, s);
        if (rc) return rc;
        rc = reduce_splits_sub_launch(p.part, n_nodes > 0 ? p.splits : 0, E.split_stride, Kt, Fo, Fop, dW, s);
        if (rc) return rc;
    }
    return TXE_OK;
}

}  // extern "C"
