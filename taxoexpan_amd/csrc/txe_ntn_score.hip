// All-candidate scoring of the NTN matcher (model_zoo.py:331-346 under test_fast.py:121-123 / infer.py:97-99) on the fp32 MFMA.
// Split V.weight [k][l + r] as [V1 | V2].  For candidate g and query q, slice j < k:
//     U_j[g] = hg[g] W_j                  (once per candidate set: txe_bilinear_project per slice, or on the stacked weight)
//     a_j[g] = V1_j . hg[g] + b_j          (once per candidate set: txe_ntn_project)
//     c_j[q] = V2_j . q                    (once per query block: txe_ntn_query_project)
//     S[q][g] = sum_j u_j tanh((<q, U_j[g]> + a_j[g]) + c_j[q])
// The pair work is the bilinear score GEMM k times with a reducing epilogue: one workgroup owns a 128 x 128 score tile (queries along
// M, candidates along N, the tile geometry, operand loaders and fragment maps of gemm_kernel) and runs gemm_kernel's k-loop once per
// slice over U_j; after slice j every accumulator goes through  s = fma(u_j, tanh((acc + a_j[n]) + c_j[m]), s)  and is cleared.  After
// the last slice s IS the tile the GEMM's epilogue receives: gemm_tile_epilogue stores it, picks the positives' pairs out of it
// (EPI_PICK), counts (EPI_COUNT_*), keeps its best k (EPI_TOPK_*) or reduces its rows to (max, sum exp) pairs (EPI_LSE_*).  No [Q x G x k] pre-activation is ever written, and nothing is split
// along the reduction: a score is a function of its two rows' values only (an MFMA accumulator is a k-ordered fmaf chain over its own
// row and column), so the four modes see bit-identical scores wherever a pair lands -- in another tile, another launch, or among the
// gathered rows of the positives.
#include "txe_gemm.h"

namespace txe {

constexpr int NTN_MAX_K = 16;

// tanh, the one function every mode calls.  |x| < 0.625: x + x^3 P(x^2), the odd minimax polynomial of the Cephes single-precision
// tanh (relative error ~1e-7 down to zero, where 1 - 2 / (exp(2x) + 1) cancels).  Above: 1 - 2 / (exp(2|x|) + 1) with the sign put
// back; exp overflows to +inf from |x| ~ 44, 2 / inf = 0 and the result is exactly 1 (it already rounds to 1 from |x| ~ 9).  No clamp
// (fminf / fmaxf would swallow a NaN): NaN fails the range test, goes through exp and the division, and comes out NaN.
__device__ __forceinline__ float ntn_tanh(float x) {
    const float ax = fabsf(x), z = x * x;
    float p = -5.70498872745e-3f;
    p = __builtin_fmaf(p, z, 2.06390887954e-2f);
    p = __builtin_fmaf(p, z, -5.37397155531e-2f);
    p = __builtin_fmaf(p, z, 1.33314422036e-1f);
    p = __builtin_fmaf(p, z, -3.33332819422e-1f);
    const float small = __builtin_fmaf(p * z, x, x);
    const float e = __expf(2.f * ax);
    const float big = copysignf(1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f), x);
    return ax < 0.625f ? small : big;
}

struct NtnArgs {
    const float* U;            // slice j of the candidate side: U + j * slice_u, rows [N][K] on pitch ld_u (the VMat B describes slice 0)
    long long slice_u;
    const float* a;            // a [k][N] on pitch ld_a
    long long ld_a;
    const float* c;            // c [k][M] on pitch ld_c
    long long ld_c;
    const float* u;            // u_R.weight [k]
    int k;
};

// One 128 x 128 score tile per workgroup (2 x 2 waves of 64 x 64, 32x32x2 fp32 MFMA, operands global -> registers -> LDS, double
// buffered, one barrier per k-tile).  The k * nk k-tiles of the k slices form one software-pipelined stream: the first k-tile of slice
// j + 1 is fetched under the last MFMA block of slice j.  A k-tile that lies wholly inside K takes the 16-byte row loader, a ragged
// last one the element loader (both zero what lies past M / N / K).  V: the operands' common vector width (4, or 1 on odd pitches).
// LSE: the tile ends in the epilogue's lse mode (Epi: EPI_LSE_MAX / EPI_LSE_MIN) -- an instantiation of its own
// VX: the vector width V, or -V -- the tile ends in the epilogue's moments mode (EPI_MOM_MAX / EPI_MOM_MIN), an instantiation of its own
// (gemm_kernel's BNX pattern: the existing instantiations keep their names)
template <int VX, bool LSE = false>
__global__ __launch_bounds__(GEMM_THREADS, 2) void ntn_score_kernel(const VMat A, VMat B, const NtnArgs P, const Epi E, const int M, const int N,
                                                                    const int K) {
    constexpr int V = VX < 0 ? -VX : VX;
    constexpr int RED = VX < 0 ? RED_MOM : (LSE ? RED_LSE : RED_NONE);
    constexpr int BN = 128, MI = 2, NJ = 2, CLD = BN + 4;
    using GA = StageGeom<true, V, GEMM_BM>;
    using GB = StageGeom<true, V, BN>;
    constexpr int ASZ = GA::LDS, BSZ = GB::LDS;
    constexpr int SMEM = 2 * (ASZ + BSZ);
    static_assert(SMEM >= GEMM_BM * CLD + 10 * GEMM_BM, "the C tile and the count mode's staged thresholds fit the operand stages");
    __shared__ __attribute__((aligned(16))) float smem[SMEM];
    __shared__ float cs[2][GEMM_BM];                  // c_j of the tile's rows, for the slice that has just ended (by slice parity)
    float* As = smem;
    float* Bs = smem + 2 * ASZ;

    const int nbn = (N + BN - 1) / BN, nbm = (M + GEMM_BM - 1) / GEMM_BM;
    const int row_fast = (nbn > nbm) ? 1 : 0;        // gemm_kernel's tile order: the long operand is streamed once
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int tm = row_fast ? lb % nbm : lb / nbn, tn = row_fast ? lb / nbm : lb % nbn;
    const int m0 = tm * GEMM_BM, n0 = tn * BN;

    if (E.cnt_mode == EPI_PICK) {                    // pick mode: a tile without a (row, own column) pair has nothing to do (block-uniform)
        const int lo = E.cnt_off[m0], hi = E.cnt_off[min(m0 + GEMM_BM, M)];
        if (n0 >= hi || n0 + BN <= lo) return;
    }
    int cnt_pb = 0, cnt_np = 0;
    float cnt_th[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if ((E.cnt_mode == EPI_COUNT_GT || E.cnt_mode == EPI_COUNT_LT) && threadIdx.x < GEMM_BM && m0 + (int)threadIdx.x < M) {
        cnt_pb = E.cnt_off[m0 + threadIdx.x];
        cnt_np = E.cnt_off[m0 + threadIdx.x + 1] - cnt_pb;
#pragma unroll
        for (int t = 0; t < 8; ++t) cnt_th[t] = E.cnt_thr[(t < cnt_np) ? cnt_pb + t : 0];
    }

    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int wm0 = (w >> 1) * 64, wn0 = (w & 1) * 64;
    // rows of a and c past N / M are never read: the lanes of an edge tile re-read the last valid one (their scores are never used)
    const int crow = min(m0 + (int)(threadIdx.x & (GEMM_BM - 1)), M - 1);
    int acol[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acol[j] = min(n0 + wn0 + j * 32 + (l & 31), N - 1);

    f32x16 acc[MI][NJ], sc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc[i][j][e] = 0.f; sc[i][j][e] = 0.f; }

    float ra[GA::NREG], rb[GB::NREG];
    unsigned ma[GA::PASSES], mb[GB::PASSES];
    const int nk = (K + GEMM_BK - 1) / GEMM_BK;       // k-tiles per slice (K >= 1)
    const int nkf = K / GEMM_BK;                      // ... of which the leading nkf lie wholly inside K
    const float* const U0 = B.p;

#define NTN_COMPUTE_TILE(cur_)                                                                                       \
    {                                                                                                                \
        const float* a_l = As + (cur_) * ASZ;                                                                        \
        const float* b_l = Bs + (cur_) * BSZ;                                                                        \
        _Pragma("unroll") for (int kb = 0; kb < GEMM_BK / 8; ++kb) {                                                 \
            float fa[MI][4], fb[NJ][4];                                                                              \
            _Pragma("unroll") for (int i = 0; i < MI; ++i) frag_load<true, GEMM_BM>(a_l, wm0 + i * 32, kb, fa[i]);   \
            _Pragma("unroll") for (int j = 0; j < NJ; ++j) frag_load<true, BN>(b_l, wn0 + j * 32, kb, fb[j]);        \
            _Pragma("unroll") for (int s = 0; s < 4; ++s)                                                            \
                _Pragma("unroll") for (int i = 0; i < MI; ++i)                                                       \
                    _Pragma("unroll") for (int j = 0; j < NJ; ++j)                                                   \
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][s], fb[j][s], acc[i][j], 0, 0, 0);    \
        }                                                                                                            \
    }
#define NTN_NOTHING
    // fetch k-tile k0_ of the slice B points at into stage buf_ while COMPUTE_ runs (loads first, selects after the MFMA block; no
    // branch between a load and its first use)
#define NTN_STAGE(FAST_, k0_, buf_, COMPUTE_)                                                                        \
    {                                                                                                                \
        stage_issue<true, V, GEMM_BM, FAST_>(A, m0, (k0_), ra, ma);                                                  \
        stage_issue<true, V, BN, FAST_>(B, n0, (k0_), rb, mb);                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                           \
        COMPUTE_                                                                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                           \
        stage_finish<true, V, GEMM_BM, FAST_>(A, m0, (k0_), ra, ma);                                                 \
        stage_finish<true, V, BN, FAST_>(B, n0, (k0_), rb, mb);                                                      \
        stage_store<true, V, GEMM_BM>(As + (buf_) * ASZ, ra);                                                        \
        stage_store<true, V, BN>(Bs + (buf_) * BSZ, rb);                                                             \
    }

    if (nkf > 0) NTN_STAGE(true, 0, 0, NTN_NOTHING)
    else NTN_STAGE(false, 0, 0, NTN_NOTHING)
    __syncthreads();
    int it = 0;                                       // k-tile of the stream being multiplied; it lies in stage it & 1
    for (int j = 0; j < P.k; ++j) {
        // this slice's share of the epilogue's operands: in flight over the whole k-loop
        const float cj = P.c[(long long)j * P.ld_c + crow];
        float aj[NJ];
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) aj[jj] = P.a[(long long)j * P.ld_a + acol[jj]];
        const float uj = P.u[j];
        // the loop is split by the kind of k-tile being FETCHED (gemm_kernel's rule): whole k-tiles, then the ragged last one, then --
        // under the slice's last MFMA block -- the first k-tile of the next slice
        int t = 0;
        for (; t + 1 < nkf; ++t, ++it) {
            NTN_STAGE(true, (t + 1) * GEMM_BK, (it + 1) & 1, NTN_COMPUTE_TILE(it & 1))
            __syncthreads();
        }
        for (; t + 1 < nk; ++t, ++it) {
            NTN_STAGE(false, (t + 1) * GEMM_BK, (it + 1) & 1, NTN_COMPUTE_TILE(it & 1))
            __syncthreads();
        }
        if (j + 1 == P.k) {
            NTN_COMPUTE_TILE(it & 1)
        } else {
            B.p = U0 + (long long)(j + 1) * P.slice_u;
            if (nkf > 0) NTN_STAGE(true, 0, (it + 1) & 1, NTN_COMPUTE_TILE(it & 1))
            else NTN_STAGE(false, 0, (it + 1) & 1, NTN_COMPUTE_TILE(it & 1))
        }
        ++it;
        // slice j is complete in acc.  (cs[j & 1] is written before this barrier and read behind it; the wave that writes it next, two
        // slices on, has passed the next slice's barrier by then -- which every wave reaches only after the reads below)
        cs[j & 1][threadIdx.x & (GEMM_BM - 1)] = cj;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float cm = cs[j & 1][wm0 + i * 32 + 4 * (l >> 5) + (e & 3) + 8 * (e >> 2)];
#pragma unroll
                for (int jj = 0; jj < NJ; ++jj) {
                    sc[i][jj][e] = __builtin_fmaf(uj, ntn_tanh((acc[i][jj][e] + aj[jj]) + cm), sc[i][jj][e]);
                    acc[i][jj][e] = 0.f;
                }
                __builtin_amdgcn_sched_barrier(0);   // (64 tanh chains scheduled side by side do not fit the register file)
            }
    }
#undef NTN_STAGE
#undef NTN_NOTHING
#undef NTN_COMPUTE_TILE

    // the tile goes through the operand stages to the GEMM's epilogue (C/D layout of the 32x32 MFMA: column = lane & 31,
    // row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)); every wave is past its last read of the stages (the barrier above)
    float* Cs = smem;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = wm0 + i * 32 + 4 * (l >> 5) + (e & 3) + 8 * (e >> 2);
                Cs[row * CLD + wn0 + j * 32 + (l & 31)] = sc[i][j][e];
            }
    __syncthreads();
    gemm_tile_epilogue<BN, SMEM, RED>(E, smem, m0, n0, M, N, tn, nbn, 0, cnt_pb, cnt_np, cnt_th);
}

// out[j][i] = <Wv[j], X[i]> (+ bias[j]) for i < n, j < k: the candidate side's a (X = hg, Wv = V1, bias = W.bias) and the query side's c
// (X = the queries, Wv = V2, no bias).  One wave per row of X; per j the lanes' partial sums (columns d = lane, lane + 64, ... in
// ascending order) meet in a fixed butterfly: a row's values depend on the row alone, not on the block it is in.
__global__ __launch_bounds__(256) void ntn_rowdot_kernel(const float* __restrict__ X, long long ld_x, int n, int d, const float* __restrict__ Wv,
                                                         long long ld_w, const float* __restrict__ bias, int k, float* __restrict__ out,
                                                         long long ld_o) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (i >= n) return;                              // (whole waves leave: the shuffles below stay uniform)
    const float* x = X + (long long)i * ld_x;
    for (int j = 0; j < k; ++j) {
        const float* wv = Wv + (long long)j * ld_w;
        float s = 0.f;
        for (int c = l; c < d; c += 64) s = __builtin_fmaf(wv[c], x[c], s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (l == 0) out[(long long)j * ld_o + i] = bias ? s + bias[j] : s;
    }
}

static int ntn_rowdot(const float* X, long long ld_x, int n, int d, const float* Wv, long long ld_w, const float* bias, int k, float* out,
                      long long ld_o, hipStream_t s, const char* name) {
    ProfScope prof(name, s, 2.0 * n * (double)d * k, 0);
    hipLaunchKernelGGL(ntn_rowdot_kernel, dim3((n + 3) / 4), dim3(256), 0, s, X, ld_x, n, d, Wv, ld_w, bias, k, out, ld_o);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

// the arguments the four scoring entry points share
struct NtnCall {
    const float* Q; long long ld_q; int nq;
    const float* U; long long ld_u, slice_u; int G, r;
    const float* a; long long ld_a;
    const float* c; long long ld_c;
    const float* u; int k;
};

static bool ntn_call_ok(const NtnCall& n) {
    if (n.nq < 0 || n.G < 0 || n.r < 1 || n.k < 1 || n.k > NTN_MAX_K) return false;
    if (!n.Q || !n.U || !n.a || !n.c || !n.u) return false;
    if (n.ld_u < n.r || (n.nq > 1 && n.ld_q < n.r)) return false;
    // (slices side by side in one [G][k * rp] matrix -- slice_u = rp, ld_u = k * rp -- or one after the other: both are fine)
    if (n.k > 1 && (n.ld_a < n.G || n.ld_c < n.nq || n.slice_u < n.r)) return false;
    return true;
}

static int ntn_launch(const NtnCall& n, int N, Epi E, hipStream_t s, const char* name) {
    VMat A = vmat_plain(n.Q, n.ld_q, n.nq, n.r);
    VMat B = vmat_plain(n.U, n.ld_u, N, n.r);
    NtnArgs P;
    P.U = n.U; P.slice_u = n.slice_u; P.a = n.a; P.ld_a = n.ld_a; P.c = n.c; P.ld_c = n.ld_c; P.u = n.u; P.k = n.k;
    {   // the epilogue's unused extras: a readable address, as gemm_launch_layout gives them
        E.act_src = E.c;
        E.mask = reinterpret_cast<const unsigned*>(E.c);
    }
    const int tiles = ((n.nq + GEMM_BM - 1) / GEMM_BM) * ((N + 127) / 128);
    // 16-byte loaders when every row of both operands starts on a 16-byte boundary -- every slice's too
    const bool v4 = vmat_vec(A) == 4 && vmat_vec(B) == 4 && (n.k == 1 || n.slice_u % 4 == 0);
    ProfScope prof(name, s, 2.0 * n.nq * (double)N * n.r * n.k, 0);
    if (epi_is_lse(E.cnt_mode)) {
        if (v4) hipLaunchKernelGGL((ntn_score_kernel<4, true>), dim3(tiles), dim3(GEMM_THREADS), 0, s, A, B, P, E, n.nq, N, n.r);
        else hipLaunchKernelGGL((ntn_score_kernel<1, true>), dim3(tiles), dim3(GEMM_THREADS), 0, s, A, B, P, E, n.nq, N, n.r);
    } else if (epi_is_mom(E.cnt_mode)) {
        if (v4) hipLaunchKernelGGL((ntn_score_kernel<-4>), dim3(tiles), dim3(GEMM_THREADS), 0, s, A, B, P, E, n.nq, N, n.r);
        else hipLaunchKernelGGL((ntn_score_kernel<-1>), dim3(tiles), dim3(GEMM_THREADS), 0, s, A, B, P, E, n.nq, N, n.r);
    } else if (v4) hipLaunchKernelGGL((ntn_score_kernel<4>), dim3(tiles), dim3(GEMM_THREADS), 0, s, A, B, P, E, n.nq, N, n.r);
    else hipLaunchKernelGGL((ntn_score_kernel<1>), dim3(tiles), dim3(GEMM_THREADS), 0, s, A, B, P, E, n.nq, N, n.r);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

}  // namespace txe

using namespace txe;

extern "C" {

int txe_ntn_project(const float* hg, long long ld_hg, int G, int l, const float* V1, long long ld_v, const float* b, int k, float* a,
                    long long ld_a, void* stream) {
    if (G < 0 || l < 1 || k < 1 || k > NTN_MAX_K || ld_hg < l || ld_v < l || ld_a < G || !hg || !V1 || !b || !a) return TXE_ERR_ARG;
    if (G == 0) return TXE_OK;
    return ntn_rowdot(hg, ld_hg, G, l, V1, ld_v, b, k, a, ld_a, (hipStream_t)stream, "ntn_rowdot_kernel[a]");
}

int txe_ntn_query_project(const float* Q, long long ld_q, int nq, int r, const float* V2, long long ld_v, int k, float* c, long long ld_c,
                          void* stream) {
    if (nq < 0 || r < 1 || k < 1 || k > NTN_MAX_K || ld_q < r || ld_v < r || ld_c < nq || !Q || !V2 || !c) return TXE_ERR_ARG;
    if (nq == 0) return TXE_OK;
    return ntn_rowdot(Q, ld_q, nq, r, V2, ld_v, nullptr, k, c, ld_c, (hipStream_t)stream, "ntn_rowdot_kernel[c]");
}

#define TXE_NTN_CALL NtnCall n{Q, ld_q, nq, U, ld_u, slice_u, G, r, a, ld_a, c, ld_c, u, k}

int txe_ntn_score_block(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, long long slice_u, int G, int r,
                        const float* a, long long ld_a, const float* c, long long ld_c, const float* u, int k, float* S, long long ld_s,
                        void* stream) {
    TXE_NTN_CALL;
    if (!ntn_call_ok(n) || !S || (nq > 1 && ld_s < G)) return TXE_ERR_ARG;
    if (nq == 0 || G == 0) return TXE_OK;
    Epi E = epi_plain(S, ld_s, G);
    return ntn_launch(n, G, E, (hipStream_t)stream, "ntn_score_kernel[store]");
}

int txe_ntn_score_positives(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, long long slice_u, int G, int r,
                            const float* a, long long ld_a, const float* c, long long ld_c, const float* u, int k, const int* pos_off,
                            float* thr, void* stream) {
    TXE_NTN_CALL;
    if (!ntn_call_ok(n) || !pos_off || !thr) return TXE_ERR_ARG;
    if (nq == 0 || G == 0) return TXE_OK;
    Epi E = epi_plain(thr, 0, G);
    E.cnt_mode = EPI_PICK;
    E.cnt_off = pos_off;
    return ntn_launch(n, G, E, (hipStream_t)stream, "ntn_score_kernel[positives]");
}

int txe_ntn_score_count_block(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, long long slice_u, int G, int r,
                              const float* a, long long ld_a, const float* c, long long ld_c, const float* u, int k, const int* pos_off,
                              const float* thr, int larger_is_better, int* counts, void* stream) {
    TXE_NTN_CALL;
    if (!ntn_call_ok(n) || !pos_off || !thr || !counts) return TXE_ERR_ARG;
    if (nq == 0 || G == 0) return TXE_OK;
    Epi E = epi_plain(reinterpret_cast<float*>(counts), 0, G);     // c is never written in count mode
    E.cnt_mode = larger_is_better ? EPI_COUNT_GT : EPI_COUNT_LT;
    E.cnt_off = pos_off; E.cnt_thr = thr; E.cnt_out = counts;
    return ntn_launch(n, G, E, (hipStream_t)stream, "ntn_score_kernel[count]");
}

int txe_ntn_score_topk_block(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, long long slice_u, int G, int r,
                             const float* a, long long ld_a, const float* c, long long ld_c, const float* u, int k, int larger_is_better,
                             int topk, int idx_base, float* part_key, int* part_idx, int* floor_ws, int* out_idx, float* out_key,
                             void* stream) {
    TXE_NTN_CALL;
    if (!ntn_call_ok(n) || G < 1 || topk < 1 || topk > TOPK_MAX || !part_key || !part_idx || !floor_ws || !out_idx) return TXE_ERR_ARG;
    if (nq == 0) return TXE_OK;
    hipStream_t s = (hipStream_t)stream;
    Epi E = epi_plain(part_key, 0, G);                              // c is never written in top-k mode
    E.cnt_mode = larger_is_better ? EPI_TOPK_MAX : EPI_TOPK_MIN;
    E.topk_k = topk; E.topk_key = part_key; E.topk_idx = part_idx; E.topk_floor = floor_ws;
    return topk_one_pass(nq, txe_score_topk_tiles(G), topk, {part_key, part_idx, floor_ws, out_idx, out_key, idx_base}, s,
                         [&] { return ntn_launch(n, G, E, s, "ntn_score_kernel[topk]"); });
}

// model_zoo.py:331-346 under infer.py:100-106 with a longer list -- txe_ntn_score_topk_block for 1 <= topk <= 64, txe_score_topk_wide_block's
// rounds, scratch (part_key / part_idx [nq][tiles][min(topk, 8)], ceil_ws 8 * nq bytes) and conventions
int txe_ntn_score_topk_wide_block(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, long long slice_u, int G, int r,
                                  const float* a, long long ld_a, const float* c, long long ld_c, const float* u, int k,
                                  int larger_is_better, int topk, int idx_base, float* part_key, int* part_idx, int* floor_ws, int* out_idx,
                                  float* out_key, void* ceil_ws, void* stream) {
    TXE_NTN_CALL;
    if (!ntn_call_ok(n) || G < 1 || topk < 1 || topk > TOPK_WIDE_MAX || !part_key || !part_idx || !floor_ws || !out_idx || !ceil_ws)
        return TXE_ERR_ARG;
    if (nq == 0) return TXE_OK;
    hipStream_t s = (hipStream_t)stream;
    Epi E = epi_plain(part_key, 0, G);                              // c is never written in top-k mode
    E.cnt_mode = larger_is_better ? EPI_TOPK_MAX : EPI_TOPK_MIN;
    E.topk_key = part_key; E.topk_idx = part_idx; E.topk_floor = floor_ws;
    return topk_rounds(nq, txe_score_topk_tiles(G), topk, {part_key, part_idx, floor_ws, out_idx, out_key, idx_base}, ceil_ws, s,
                       [&](int kr, const float* ceil_key, const int* ceil_idx) {
                           E.topk_k = kr; E.topk_ceil_key = ceil_key; E.topk_ceil_idx = ceil_idx;
                           return ntn_launch(n, G, E, s, "ntn_score_kernel[topk]");
                       });
}

// model_zoo.py:331-346 under model/loss.py:52-57 over test_fast.py:121-123 / infer.py:97-99 -- the log-partition of every query over all
// candidates, txe_score_lse_block's conventions: the finished tile's rows leave (max z, sum exp(z - max)), txe_lse_merge combines them
int txe_ntn_score_lse_block(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, long long slice_u, int G, int r,
                            const float* a, long long ld_a, const float* c, long long ld_c, const float* u, int k, int larger_is_better,
                            float* part_max, float* part_sum, float* lse, void* stream) {
    TXE_NTN_CALL;
    if (!ntn_call_ok(n) || G < 1 || !part_max || !part_sum || !lse) return TXE_ERR_ARG;
    if (nq == 0) return TXE_OK;
    Epi E = epi_plain(part_max, 0, G);                              // c is never written in lse mode
    E.cnt_mode = larger_is_better ? EPI_LSE_MAX : EPI_LSE_MIN;
    E.lse_m = part_max; E.lse_s = part_sum;
    hipStream_t s = (hipStream_t)stream;
    return lse_one_pass(nq, txe_score_topk_tiles(G), part_max, part_sum, lse, s, [&] { return ntn_launch(n, G, E, s, "ntn_score_kernel[lse]"); });
}

// model_zoo.py:331-346 under a score scale -- the moments of every query's predictive distribution over all candidates,
// txe_score_moments_block's definition, scratch and merge
int txe_ntn_score_moments_block(const float* Q, long long ld_q, int nq, const float* U, long long ld_u, long long slice_u, int G, int r,
                                const float* a, long long ld_a, const float* c, long long ld_c, const float* u, int k, int larger_is_better,
                                float beta, float* part_max, float* part_s0, float* part_s1, float* part_s2, double* out, void* stream) {
    TXE_NTN_CALL;
    if (!ntn_call_ok(n) || G < 1 || !moments_args_ok(beta, part_max, part_s0, part_s1, part_s2, out)) return TXE_ERR_ARG;
    if (nq == 0) return TXE_OK;
    Epi E = epi_plain(part_max, 0, G);                              // c is never written in moments mode
    E.cnt_mode = larger_is_better ? EPI_MOM_MAX : EPI_MOM_MIN;
    E.mom_beta = beta; E.lse_m = part_max; E.lse_s = part_s0; E.mom_s1 = part_s1; E.mom_s2 = part_s2;
    hipStream_t s = (hipStream_t)stream;
    return moments_one_pass(nq, txe_score_topk_tiles(G), {part_max, part_s0, part_s1, part_s2, out}, s,
                            [&] { return ntn_launch(n, G, E, s, "ntn_score_kernel[moments]"); });
}

#undef TXE_NTN_CALL

}  // extern "C"
