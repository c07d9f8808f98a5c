// All-candidate scoring of the MLP matcher (model_zoo.py:285-298 under test_fast.py:121-123 / infer.py:97-99), on the VALU.
// Split ffn[0].weight W1 [H][l+r] as [W1a | W1b].  For candidate g and query q:
//     A[g] = hg[g] W1a^T + b1          (once per candidate set: txe_linear_fwd, then txe_mlp_project pads it and flags its rows)
//     B[q] = q W1b^T                   (once per query block: txe_mlp_query_project, stored negated)
//     S[q][g] = b2 + sum_h w2[h] relu(A[g][h] + B[q][h])
//             = c[q] + sum_h w2[h] max(A[g][h], -B[q][h]),    c[q] = b2 + sum_h w2[h] B[q][h]      (relu(a + b) = max(a, -b) + b)
// The pair term is not a product: one v_max_f32 and one FMA per (pair, h), no matrix pipe.  Every pair's score is a pure function of
// its A row, its -B row, w2 and c[q], summed over h = 0 .. Hp-1 in ascending order by one FMA chain -- never split over h -- so the
// store, positives, count, top-k and lse modes see bit-identical scores wherever a pair lands.  H is zero-padded to Hp (a multiple of the
// 16-wide k-step) in A, -B and w2: a padded step is fma(0, max(0, 0), acc) = acc.
// The identity is exact only in the finite domain: the hardware max returns the non-NaN operand, and max(a, -b) + b hides an overflow
// of a + b.  Rows of A and of B that hold NaN, +-Inf or a magnitude above lim = 2^120 / max(1, sum_h |w2[h]|) are flagged, and every
// pair that touches a flagged row is recomputed with the literal per-pair formula (relu propagates NaN, as torch's does).  Below lim
// no partial sum of either form comes near FLT_MAX (|w2| * |a + b| summed over h stays under 2^121), so the two forms then produce the
// same non-finite pattern: none.
#include "txe_common.h"
#include "txe_moments.h"

namespace txe {

constexpr int MLP_KC = 16;      // k-step: H is padded to a multiple of it
constexpr int MLP_BG = 128;     // candidates per workgroup (= the 128-wide column tiles of txe_score_topk_tiles)
constexpr int MLP_BQ = 64;      // queries per workgroup
constexpr int MLP_QP = 8;       // queries per workgroup of the query-side projection

__host__ __device__ __forceinline__ int mlp_padded(int H) { return (H + MLP_KC - 1) / MLP_KC * MLP_KC; }

// the hardware max as one instruction: the compiler's fmaxf canonicalises operands it cannot prove canonical (an extra v_max each)
// and NaN never reaches it here (flagged rows take the literal path)
__device__ __forceinline__ float vmax(float a, float b) {
    float d;
    asm("v_max_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ float relu_nan(float x) { return x > 0.f ? x : (x == x ? 0.f : x); }

__device__ __forceinline__ bool mlp_bad(float x, float lim) { return !(fabsf(x) <= lim); }

// The literal per-pair formula (the fallback of flagged rows): b2 + sum_h w2[h] relu(A[g][h] + B[q][h]), h ascending
__device__ __forceinline__ float mlp_literal(const float* __restrict__ ar, const float* __restrict__ nbr, const float* __restrict__ mw, int Hp) {
    float acc = 0.f;
    for (int h = 0; h < Hp; ++h) acc = __builtin_fmaf(mw[h], relu_nan(ar[h] - nbr[h]), acc);
    return mw[Hp] + acc;
}

// The two-op formula of one pair, h ascending: the chain every mode's tiles run, restated for single pairs (positives)
__device__ __forceinline__ float mlp_pair(const float* __restrict__ ar, const float* __restrict__ nbr, const float* __restrict__ mw, int Hp, float c) {
    float acc = 0.f;
    for (int h = 0; h < Hp; ++h) acc = __builtin_fmaf(mw[h], vmax(ar[h], nbr[h]), acc);
    return c + acc;
}

// mw [Hp + 2] = w2 zero-padded to Hp, then b2, then lim.  One workgroup; sum |w2| in a fixed order.
__global__ __launch_bounds__(256) void mlp_weights_kernel(const float* __restrict__ w2, const float* __restrict__ b2, int H, int Hp,
                                                          float* __restrict__ mw) {
    __shared__ float part[256];
    float s = 0.f;
    for (int h = threadIdx.x; h < Hp; h += 256) {
        const float w = h < H ? w2[h] : 0.f;
        mw[h] = w;
        s += fabsf(w);
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        mw[Hp] = b2[0];
        mw[Hp + 1] = ldexpf(1.f, 120) / fmaxf(1.f, part[0]);
    }
}

// Ap [G][Hp] = A zero-padded, flags[g] = the row holds NaN / +-Inf / a magnitude above lim.  One wave per row.
__global__ __launch_bounds__(256) void mlp_pad_rows_kernel(const float* __restrict__ A, long long ld_a, int G, int H, int Hp,
                                                           const float* __restrict__ mw, float* __restrict__ Ap, int* __restrict__ flags) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (g >= G) return;
    const float lim = mw[Hp + 1];
    bool bad = false;
    for (int h = l; h < Hp; h += 64) {
        const float v = h < H ? A[(long long)g * ld_a + h] : 0.f;
        Ap[(long long)g * Hp + h] = v;
        bad |= mlp_bad(v, lim);
    }
    const bool any = __ballot(bad) != 0;
    if (l == 0) flags[g] = any ? 1 : 0;
}

// Query side of one block: nB[q][h] = -(Qf[q] W1b^T)[h] (j ascending, one FMA chain per element: a row's values do not depend on the
// block it is in), zero-padded to Hp; c[q] = b2 + sum_h w2[h] B[q][h] accumulated in double (products of two floats are exact there)
// and reduced in a fixed tree; flags[q] as for the candidates.  W1bT [r][H] = W1b transposed.  MLP_QP queries per workgroup.
__global__ __launch_bounds__(256) void mlp_query_kernel(const float* __restrict__ Qf, long long ld_q, int nq, int r,
                                                        const float* __restrict__ W1bT, int H, int Hp, const float* __restrict__ mw,
                                                        float* __restrict__ nB, float* __restrict__ c, int* __restrict__ flags) {
    constexpr int RC = 256;
    __shared__ float qs[MLP_QP][RC];
    __shared__ double red[MLP_QP][256];
    __shared__ int sbad[MLP_QP];
    const int q0 = blockIdx.x * MLP_QP, t = threadIdx.x;
    const float lim = mw[Hp + 1];
    if (t < MLP_QP) sbad[t] = 0;
    double pd[MLP_QP];
#pragma unroll
    for (int i = 0; i < MLP_QP; ++i) pd[i] = 0.0;
    for (int h0 = 0; h0 < Hp; h0 += 256) {
        const int h = h0 + t;
        float acc[MLP_QP];
#pragma unroll
        for (int i = 0; i < MLP_QP; ++i) acc[i] = 0.f;
        for (int j0 = 0; j0 < r; j0 += RC) {
            const int nj = min(RC, r - j0);
            __syncthreads();
            for (int e = t; e < MLP_QP * RC; e += 256) {
                const int i = e / RC, j = e % RC;
                qs[i][j] = (q0 + i < nq && j < nj) ? Qf[(long long)(q0 + i) * ld_q + j0 + j] : 0.f;
            }
            __syncthreads();
            if (h < H) {
                const float* wp = W1bT + (long long)j0 * H + h;
                for (int j = 0; j < nj; ++j) {
                    const float w = wp[(long long)j * H];
#pragma unroll
                    for (int i = 0; i < MLP_QP; ++i) acc[i] = __builtin_fmaf(qs[i][j], w, acc[i]);
                }
            }
        }
        if (h < Hp) {
            const float w2 = mw[h];
#pragma unroll
            for (int i = 0; i < MLP_QP; ++i) {
                const float b = h < H ? acc[i] : 0.f;
                if (q0 + i < nq) {
                    nB[(long long)(q0 + i) * Hp + h] = -b;
                    if (mlp_bad(b, lim)) atomicOr(&sbad[i], 1);
                }
                pd[i] += (double)w2 * (double)b;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MLP_QP; ++i) red[i][t] = pd[i];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int i = 0; i < MLP_QP; ++i) red[i][t] += red[i][t + o];
        }
        __syncthreads();
    }
    if (t < MLP_QP && q0 + t < nq) {
        c[q0 + t] = (float)((double)mw[Hp] + red[t][0]);
        flags[q0 + t] = sbad[t];
    }
}

struct MlpArgs {
    const float* Ap; const int* fa; int G;          // candidates: padded A, row flags
    const float* nB; const float* c; const int* fb; int nq;   // query block: padded -B, c, row flags
    const float* mw; int Hp;                        // w2 (padded), b2, lim
    float* S; long long ld_s;                       // store
    const int* pos_off; const float* thr; int* counts; int larger;   // count
    // (moments: the score scale and the two further sums ride in top-k's slots, which a moments launch never reads)
    union { int k; float beta; }; union { float* part_key; float* part_s1; }; int* part_idx; int* floor_ws;   // top-k
    union { const float* ceil_key; float* part_s2; }; const int* ceil_idx;   // top-k: the rows' ceilings of a wide best-k's later rounds (NULL: none)
    float* part_max; float* part_sum;                                // lse; moments: (max, s0)
};

static_assert(sizeof(MlpArgs) == 176, "MlpArgs grew: the moments mode's fields are meant to ride in top-k's slots");

// (MLP_TOPK_CEIL: MLP_TOPK under the rows' ceilings, a later round of a wide best-k -- an instantiation of its own, so that the k <= 8
//  path's kernel keeps its registers and its occupancy)
enum { MLP_STORE = 0, MLP_COUNT = 1, MLP_TOPK = 2, MLP_LSE = 3, MLP_TOPK_CEIL = 4, MLP_MOM = 5 };

// One 128-candidate x 64-query tile per workgroup of 256 threads; thread (tg, tq) = (tid & 15, tid >> 4) owns candidates
// g0 + {tg*4 .. tg*4+3, 64 + tg*4 .. 64 + tg*4+3} and queries q0 + tq*4 .. tq*4+3: 32 pairs.  A and -B go through LDS in 16-step
// chunks, transposed (h-major), double-buffered: the next chunk's global loads are in flight while the current one is consumed.
template <int MODE>
__global__ __launch_bounds__(256) void mlp_pair_kernel(const MlpArgs a) {
    __shared__ float As[2][MLP_KC][MLP_BG];
    __shared__ float Bs[2][MLP_KC][MLP_BQ];
    const int tid = threadIdx.x, tg = tid & 15, tq = tid >> 4;
    const int g0 = blockIdx.x * MLP_BG, q0 = blockIdx.y * MLP_BQ;
    const int Hp = a.Hp;
    // loaders: A rows g0 + tid/2 (8 steps each half), -B rows q0 + tid/4 (4 steps each quarter); rows past the end read the last row
    const int la_r = tid >> 1, la_h = (tid & 1) * 8, lb_r = tid >> 2, lb_h = (tid & 3) * 4;
    const float* pa = a.Ap + (long long)min(g0 + la_r, a.G - 1) * Hp + la_h;
    const float* pb = a.nB + (long long)min(q0 + lb_r, a.nq - 1) * Hp + lb_h;
    float4 ra0 = *reinterpret_cast<const float4*>(pa), ra1 = *reinterpret_cast<const float4*>(pa + 4);
    float4 rb = *reinterpret_cast<const float4*>(pb);
    auto stage = [&](int buf) {
        const float va[8] = {ra0.x, ra0.y, ra0.z, ra0.w, ra1.x, ra1.y, ra1.z, ra1.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) As[buf][la_h + i][la_r] = va[i];
        const float vb[4] = {rb.x, rb.y, rb.z, rb.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) Bs[buf][lb_h + i][lb_r] = vb[i];
    };
    stage(0);
    __syncthreads();
    float acc[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    const int nk = Hp / MLP_KC;
    for (int kc = 0; kc < nk; ++kc) {
        const int cur = kc & 1;
        if (kc + 1 < nk) {
            const int o = (kc + 1) * MLP_KC;
            ra0 = *reinterpret_cast<const float4*>(pa + o); ra1 = *reinterpret_cast<const float4*>(pa + o + 4);
            rb = *reinterpret_cast<const float4*>(pb + o);
        }
        const float* w2c = a.mw + kc * MLP_KC;
#pragma unroll 8
        for (int h = 0; h < MLP_KC; ++h) {
            const float w = w2c[h];
            const float4 x0 = *reinterpret_cast<const float4*>(&As[cur][h][tg * 4]);
            const float4 x1 = *reinterpret_cast<const float4*>(&As[cur][h][64 + tg * 4]);
            const float4 y = *reinterpret_cast<const float4*>(&Bs[cur][h][tq * 4]);
            const float xv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
            const float yv[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][j] = __builtin_fmaf(w, vmax(xv[j], yv[i]), acc[i][j]);
        }
        if (kc + 1 < nk) stage(cur ^ 1);
        __syncthreads();
    }
    // scores: c[q] + acc; a pair that touches a flagged row is recomputed with the literal formula (rare: one copy of the loop, the
    // pair picked out of a bit mask so that the accumulators stay in registers)
    int gcol[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) gcol[j] = g0 + (j < 4 ? tg * 4 + j : 64 + tg * 4 + (j - 4));
    unsigned need = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = q0 + tq * 4 + i, qc = min(q, a.nq - 1);
        const float cq = a.c[qc];
        const int fq = a.fb[qc];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            acc[i][j] = cq + acc[i][j];
            if ((fq | a.fa[min(gcol[j], a.G - 1)]) && q < a.nq && gcol[j] < a.G) need |= 1u << (i * 8 + j);
        }
    }
    while (need) {
        const int p = __builtin_ctz(need), i = p >> 3, j = p & 7;
        need &= need - 1u;
        const int q = q0 + tq * 4 + i, g = g0 + (j < 4 ? tg * 4 + j : 64 + tg * 4 + (j - 4));
        const float v = mlp_literal(a.Ap + (long long)g * Hp, a.nB + (long long)q * Hp, a.mw, Hp);
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) acc[ii][jj] = (ii * 8 + jj == p) ? v : acc[ii][jj];
    }
    if constexpr (MODE == MLP_STORE) {
        const bool vec = ((a.ld_s & 3) == 0) && ((reinterpret_cast<uintptr_t>(a.S) & 15) == 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = q0 + tq * 4 + i;
            if (q >= a.nq) continue;
            float* row = a.S + (long long)q * a.ld_s;
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int gb = gcol[hf * 4];
                if (vec && gb + 3 < a.G) {
                    *reinterpret_cast<float4*>(row + gb) = make_float4(acc[i][hf * 4], acc[i][hf * 4 + 1], acc[i][hf * 4 + 2], acc[i][hf * 4 + 3]);
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (gb + u < a.G) row[gb + u] = acc[i][hf * 4 + u];
                }
            }
        }
    } else if constexpr (MODE == MLP_COUNT) {
        // counts[j] += #{g : S[q][g] strictly better than thr[j]}: the 16 threads of a query row (lanes tq*16 .. +15 of the wave, one
        // trip count) reduce their counts by butterfly, then one integer atomic per (tile, positive) -- exact and order independent
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = q0 + tq * 4 + i;
            if (q >= a.nq) continue;
            const int pb = a.pos_off[q], pe = a.pos_off[q + 1];
            for (int p = pb; p < pe; ++p) {
                const float th = a.thr[p];
                int cnt = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) cnt += (gcol[j] < a.G && (a.larger ? acc[i][j] > th : acc[i][j] < th)) ? 1 : 0;
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) cnt += __shfl_xor(cnt, o, 64);
                if (tg == 0 && cnt) atomicAdd(a.counts + p, cnt);
            }
        }
    } else if constexpr (MODE == MLP_LSE) {
        // log-partition: (max z, sum exp(z - max)) of every query row over this tile's candidates, z = the score or its negative.  Each
        // thread's 8 columns, then a butterfly over the 16 threads of the row, once for the maximum (NaN kept) and once for the sum --
        // a fixed order: a row's pair depends on the row's scores alone
        const int nbn = (a.G + MLP_BG - 1) / MLP_BG;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = q0 + tq * 4 + i;
            float mx = -INFINITY;
            bool bad = false;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float z = a.larger ? acc[i][j] : -acc[i][j];
                const bool in = gcol[j] < a.G;
                bad |= in & (z != z);
                mx = in ? fmaxf(mx, z) : mx;
            }
            mx = bad ? __builtin_nanf("") : mx;
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) mx = lse_max(mx, __shfl_xor(mx, o, 64));
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) s += (gcol[j] < a.G) ? lse_term(a.larger ? acc[i][j] : -acc[i][j], mx) : 0.f;
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o, 64);
            if (tg == 0 && q < a.nq) {
                const long long o = (long long)q * nbn + blockIdx.x;
                a.part_max[o] = mx;
                a.part_sum[o] = s;
            }
        }
    } else if constexpr (MODE == MLP_MOM) {
        // moments: the lse mode above over t = fl32(beta * z) (txe_moments.h) -- each thread's 8 columns, then a butterfly over the 16
        // threads of the row, once for the maximum (NaN kept) and once for the three sums: a fixed order
        const int nbn = (a.G + MLP_BG - 1) / MLP_BG;
        const bool larger = a.larger != 0;
        const float beta = a.beta;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = q0 + tq * 4 + i;
            float mx = -INFINITY;
            bool bad = false;
#pragma unroll
            for (int j = 0; j < 8; ++j) mom_max_step(mom_scaled(acc[i][j], larger, beta), gcol[j] < a.G, mx, bad);
            mx = bad ? __builtin_nanf("") : mx;
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) mx = lse_max(mx, __shfl_xor(mx, o, 64));
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) mom_sum_step(mom_scaled(acc[i][j], larger, beta), gcol[j] < a.G, mx, s0, s1, s2);
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                s0 += __shfl_xor(s0, o, 64);
                s1 += __shfl_xor(s1, o, 64);
                s2 += __shfl_xor(s2, o, 64);
            }
            if (tg == 0 && q < a.nq) {
                const long long o = (long long)q * nbn + blockIdx.x;
                a.part_max[o] = mx;
                a.part_sum[o] = s0;
                a.part_s1[o] = s1;
                a.part_s2[o] = s2;
            }
        }
    } else {
        // best-k of this tile per query row: each thread's 8 columns, then a butterfly over the 16 threads of the row (all lanes
        // take part: the shuffles stay uniform); the row's rising floor skips values another tile has already beaten k times
        const int nbn = (a.G + MLP_BG - 1) / MLP_BG, kk = a.k;
        const bool larger = a.larger != 0;
#pragma unroll 1
        for (int i = 0; i < 4; ++i) {
            const int q = q0 + tq * 4 + i;
            const bool qok = q < a.nq;
            const float floor_key = qok ? topk_unord(__hip_atomic_load(a.floor_ws + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) : -INFINITY;
            float bk[TOPK_MAX];
            int bi[TOPK_MAX];
            topk_init(bk, bi);
            float wk = -INFINITY;
            int wi = 0x7fffffff;
            // the row's ceiling (Epi::topk_ceil_key's rule: only entries strictly worse than it are eligible)
            float ck = INFINITY;
            int ci = -1;
            if constexpr (MODE == MLP_TOPK_CEIL) {
                ck = qok ? a.ceil_key[q] : INFINITY;
                ci = qok ? a.ceil_idx[q] : -1;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int n = gcol[j];
                const float key = topk_key_of(acc[i][j], larger);
                bool take = n < a.G && !(key < floor_key) && topk_better(key, n, wk, wi);
                if constexpr (MODE == MLP_TOPK_CEIL) take = take && topk_better(ck, ci, key, n);
                if (take) {
                    topk_insert(bk, bi, key, n);
                    topk_kth(bk, bi, kk, wk, wi);
                }
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                float ok[TOPK_MAX];
                int oi[TOPK_MAX];
#pragma unroll
                for (int t = 0; t < TOPK_MAX; ++t) { ok[t] = __shfl_xor(bk[t], o, 64); oi[t] = __shfl_xor(bi[t], o, 64); }
#pragma unroll
                for (int t = 0; t < TOPK_MAX; ++t)
                    if (t < kk && topk_better(ok[t], oi[t], wk, wi)) {
                        topk_insert(bk, bi, ok[t], oi[t]);
                        topk_kth(bk, bi, kk, wk, wi);
                    }
            }
            if (tg == 0 && qok) {
                const long long o = ((long long)q * nbn + blockIdx.x) * kk;
                float kth = -INFINITY;
                int kth_i = 0x7fffffff;
#pragma unroll
                for (int t = 0; t < TOPK_MAX; ++t)
                    if (t < kk) { a.part_key[o + t] = bk[t]; a.part_idx[o + t] = bi[t]; kth = bk[t]; kth_i = bi[t]; }
                if (kth_i != 0x7fffffff && kth > floor_key) atomicMax(a.floor_ws + q, topk_ord(kth));
            }
        }
    }
}

// thr[j] = S[q][pos_idx[j]] for j in [pos_off[q], pos_off[q+1]) (0 where pos_idx[j] is not a row of this candidate set: a positive
// that lives in another shard) -- one thread per positive, the tiles' own chain
__global__ __launch_bounds__(256) void mlp_positives_kernel(const MlpArgs a, const int* __restrict__ pos_idx, int n_pos) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_pos) return;
    int lo = 0, hi = a.nq;                           // the query of positive j: pos_off[q] <= j < pos_off[q+1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.pos_off[mid] <= j) lo = mid; else hi = mid;
    }
    const int q = lo, g = pos_idx[j];
    if (g < 0 || g >= a.G) { a.S[j] = 0.f; return; }
    const float* ar = a.Ap + (long long)g * a.Hp;
    const float* nbr = a.nB + (long long)q * a.Hp;
    a.S[j] = (a.fa[g] | a.fb[q]) ? mlp_literal(ar, nbr, a.mw, a.Hp) : mlp_pair(ar, nbr, a.mw, a.Hp, a.c[q]);
}

static MlpArgs mlp_args(const float* Ap, const int* fa, int G, const float* nB, const float* c, const int* fb, int nq, int H, const float* mw) {
    MlpArgs a{};
    a.Ap = Ap; a.fa = fa; a.G = G; a.nB = nB; a.c = c; a.fb = fb; a.nq = nq; a.mw = mw; a.Hp = mlp_padded(H);
    return a;
}

template <int MODE>
static int mlp_launch(const MlpArgs& a, hipStream_t s, const char* name) {
    ProfScope prof(name, s, 2.0 * a.G * (double)a.nq * a.Hp, 0);
    hipLaunchKernelGGL(mlp_pair_kernel<MODE>, dim3((a.G + MLP_BG - 1) / MLP_BG, (a.nq + MLP_BQ - 1) / MLP_BQ), dim3(256), 0, s, a);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

}  // namespace txe

using namespace txe;

extern "C" {

int txe_mlp_padded_h(int H) { return H < 1 ? 0 : mlp_padded(H); }

int txe_mlp_project(const float* A, long long ld_a, int G, int H, const float* w2, const float* b2, float* Ap, float* mw, int* flags,
                    void* stream) {
    if (G < 0 || H < 1 || (G > 0 && (ld_a < H || !A || !Ap || !flags)) || !w2 || !b2 || !mw) return TXE_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int Hp = mlp_padded(H);
    hipLaunchKernelGGL(mlp_weights_kernel, dim3(1), dim3(256), 0, s, w2, b2, H, Hp, mw);
    TXE_CHECK_LAUNCH();
    if (G == 0) return TXE_OK;
    hipLaunchKernelGGL(mlp_pad_rows_kernel, dim3((G + 3) / 4), dim3(256), 0, s, A, ld_a, G, H, Hp, (const float*)mw, Ap, flags);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

int txe_mlp_query_project(const float* Qf, long long ld_q, int nq, int r, const float* W1bT, int H, const float* mw, float* nB, float* c,
                          int* flags, void* stream) {
    if (nq < 0 || r < 1 || H < 1 || ld_q < r || !Qf || !W1bT || !mw || !nB || !c || !flags) return TXE_ERR_ARG;
    if (nq == 0) return TXE_OK;
    hipLaunchKernelGGL(mlp_query_kernel, dim3((nq + MLP_QP - 1) / MLP_QP), dim3(256), 0, (hipStream_t)stream, Qf, ld_q, nq, r, W1bT, H,
                       mlp_padded(H), mw, nB, c, flags);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

#define TXE_MLP_ARGS_OK (G >= 0 && nq >= 0 && H >= 1 && Ap && flag_a && nB && c && flag_b && mw)

int txe_mlp_score_block(const float* Ap, const int* flag_a, int G, const float* nB, const float* c, const int* flag_b, int nq, int H,
                        const float* mw, float* S, long long ld_s, void* stream) {
    if (!TXE_MLP_ARGS_OK || !S || (nq > 1 && ld_s < G)) return TXE_ERR_ARG;
    if (nq == 0 || G == 0) return TXE_OK;
    MlpArgs a = mlp_args(Ap, flag_a, G, nB, c, flag_b, nq, H, mw);
    a.S = S; a.ld_s = ld_s;
    return mlp_launch<MLP_STORE>(a, (hipStream_t)stream, "mlp_pair_kernel[store]");
}

int txe_mlp_score_positives(const float* Ap, const int* flag_a, int G, const float* nB, const float* c, const int* flag_b, int nq, int H,
                            const float* mw, const int* pos_off, const int* pos_idx, int n_pos, float* thr, void* stream) {
    if (!TXE_MLP_ARGS_OK || n_pos < 0 || !pos_off || !pos_idx || !thr) return TXE_ERR_ARG;
    if (nq == 0 || n_pos == 0) return TXE_OK;
    MlpArgs a = mlp_args(Ap, flag_a, G, nB, c, flag_b, nq, H, mw);
    a.S = thr; a.pos_off = pos_off;
    hipLaunchKernelGGL(mlp_positives_kernel, dim3((n_pos + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, pos_idx, n_pos);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

int txe_mlp_score_count_block(const float* Ap, const int* flag_a, int G, const float* nB, const float* c, const int* flag_b, int nq, int H,
                              const float* mw, const int* pos_off, const float* thr, int larger_is_better, int* counts, void* stream) {
    if (!TXE_MLP_ARGS_OK || !pos_off || !thr || !counts) return TXE_ERR_ARG;
    if (nq == 0 || G == 0) return TXE_OK;
    MlpArgs a = mlp_args(Ap, flag_a, G, nB, c, flag_b, nq, H, mw);
    a.pos_off = pos_off; a.thr = thr; a.counts = counts; a.larger = larger_is_better ? 1 : 0;
    return mlp_launch<MLP_COUNT>(a, (hipStream_t)stream, "mlp_pair_kernel[count]");
}

int txe_mlp_score_topk_block(const float* Ap, const int* flag_a, int G, const float* nB, const float* c, const int* flag_b, int nq, int H,
                             const float* mw, int larger_is_better, int k, int idx_base, float* part_key, int* part_idx, int* floor_ws,
                             int* out_idx, float* out_key, void* stream) {
    if (!TXE_MLP_ARGS_OK || G < 1 || k < 1 || k > TOPK_MAX || !part_key || !part_idx || !floor_ws || !out_idx) return TXE_ERR_ARG;
    if (nq == 0) return TXE_OK;
    hipStream_t s = (hipStream_t)stream;
    MlpArgs a = mlp_args(Ap, flag_a, G, nB, c, flag_b, nq, H, mw);
    a.larger = larger_is_better ? 1 : 0; a.k = k; a.part_key = part_key; a.part_idx = part_idx; a.floor_ws = floor_ws;
    return topk_one_pass(nq, (G + MLP_BG - 1) / MLP_BG, k, {part_key, part_idx, floor_ws, out_idx, out_key, idx_base}, s,
                         [&] { return mlp_launch<MLP_TOPK>(a, s, "mlp_pair_kernel[topk]"); });
}

// model_zoo.py:285-298 under infer.py:100-106 with a longer list -- txe_mlp_score_topk_block for 1 <= k <= 64, txe_score_topk_wide_block's
// rounds, scratch (part_key / part_idx [nq][tiles][min(k, 8)], ceil_ws 8 * nq bytes) and conventions
int txe_mlp_score_topk_wide_block(const float* Ap, const int* flag_a, int G, const float* nB, const float* c, const int* flag_b, int nq, int H,
                                  const float* mw, int larger_is_better, int k, int idx_base, float* part_key, int* part_idx,
                                  int* floor_ws, int* out_idx, float* out_key, void* ceil_ws, void* stream) {
    if (!TXE_MLP_ARGS_OK || G < 1 || k < 1 || k > TOPK_WIDE_MAX || !part_key || !part_idx || !floor_ws || !out_idx || !ceil_ws) return TXE_ERR_ARG;
    if (nq == 0) return TXE_OK;
    hipStream_t s = (hipStream_t)stream;
    MlpArgs a = mlp_args(Ap, flag_a, G, nB, c, flag_b, nq, H, mw);
    a.larger = larger_is_better ? 1 : 0; a.part_key = part_key; a.part_idx = part_idx; a.floor_ws = floor_ws;
    return topk_rounds(nq, (G + MLP_BG - 1) / MLP_BG, k, {part_key, part_idx, floor_ws, out_idx, out_key, idx_base}, ceil_ws, s,
                       [&](int kr, const float* ceil_key, const int* ceil_idx) {
                           a.k = kr; a.ceil_key = ceil_key; a.ceil_idx = ceil_idx;
                           return ceil_key ? mlp_launch<MLP_TOPK_CEIL>(a, s, "mlp_pair_kernel[topk]") : mlp_launch<MLP_TOPK>(a, s, "mlp_pair_kernel[topk]");
                       });
}

// model_zoo.py:285-298 under model/loss.py:52-57 over test_fast.py:121-123 / infer.py:97-99 -- the log-partition of every query over all
// candidates, txe_score_lse_block's conventions: part_max / part_sum [nq][txe_score_topk_tiles(G)] scratch, lse [nq]
int txe_mlp_score_lse_block(const float* Ap, const int* flag_a, int G, const float* nB, const float* c, const int* flag_b, int nq, int H,
                            const float* mw, int larger_is_better, float* part_max, float* part_sum, float* lse, void* stream) {
    if (!TXE_MLP_ARGS_OK || G < 1 || !part_max || !part_sum || !lse) return TXE_ERR_ARG;
    if (nq == 0) return TXE_OK;
    hipStream_t s = (hipStream_t)stream;
    MlpArgs a = mlp_args(Ap, flag_a, G, nB, c, flag_b, nq, H, mw);
    a.larger = larger_is_better ? 1 : 0; a.part_max = part_max; a.part_sum = part_sum;
    return lse_one_pass(nq, (G + MLP_BG - 1) / MLP_BG, part_max, part_sum, lse, s, [&] { return mlp_launch<MLP_LSE>(a, s, "mlp_pair_kernel[lse]"); });
}

// model_zoo.py:285-298 under a score scale -- the moments of every query's predictive distribution over all candidates,
// txe_score_moments_block's definition, scratch and merge (the pair kernel's tiles are 128 candidates wide too)
int txe_mlp_score_moments_block(const float* Ap, const int* flag_a, int G, const float* nB, const float* c, const int* flag_b, int nq, int H,
                                const float* mw, int larger_is_better, float beta, float* part_max, float* part_s0, float* part_s1,
                                float* part_s2, double* out, void* stream) {
    if (!TXE_MLP_ARGS_OK || G < 1 || !moments_args_ok(beta, part_max, part_s0, part_s1, part_s2, out)) return TXE_ERR_ARG;
    if (nq == 0) return TXE_OK;
    hipStream_t s = (hipStream_t)stream;
    MlpArgs a = mlp_args(Ap, flag_a, G, nB, c, flag_b, nq, H, mw);
    a.larger = larger_is_better ? 1 : 0; a.beta = beta; a.part_max = part_max; a.part_sum = part_s0; a.part_s1 = part_s1; a.part_s2 = part_s2;
    return moments_one_pass(nq, (G + MLP_BG - 1) / MLP_BG, {part_max, part_s0, part_s1, part_s2, out}, s,
                            [&] { return mlp_launch<MLP_MOM>(a, s, "mlp_pair_kernel[moments]"); });
}

}  // extern "C"
