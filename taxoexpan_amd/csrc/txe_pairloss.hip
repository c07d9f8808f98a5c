// The pointwise and pairwise training losses of model/loss.py -- bce_loss (:21-29), square_exp_loss (:12-19) and margin_rank_loss
// (:31-50) -- each with its gradient, sum-reduced, on a labelled score vector x [B] with labels [B] (int32 or int64).  An entry is a
// positive iff its label is 1.
//
//   bce          loss = sum over positives of softplus(x_i) + sum over the others of softplus(-x_i)   (the score is an energy)
//                     = binary_cross_entropy_with_logits(x, 1 - label, reduction="sum"); softplus(z) = max(z, 0) + log1p(exp(-|z|))
//                d_x[i] = sigmoid(x_i) - [i is no positive]
//   square_exp   loss = sum over positives of x_i^2 + beta * sum over label == 0 of exp(-x_i);  d_x[i] = 2 x_i | -beta exp(-x_i) | 0
//   margin_rank  groups as in txe_groups.h; loss = sum over every (positive p, negative n) pair of one group of
//                max(0, (x_p - x_n) + margin), evaluated in fp32 as written (one subtraction, one addition);
//                d_x[p] = +(the group's negatives with (x_p - x_n) + margin > 0), d_x[n] = -(the group's positives with the same):
//                integers.  NaN never compares true (no gradient), and a NaN term makes the loss NaN, as torch's clamp does.
//
// bce and square_exp are ONE launch of one workgroup each (the training path has B <= 2^18 scores): every lane adds its own terms in
// index order, the lanes of a wave are combined by the fixed DPP tree of wave_sum, the 16 wave sums in wave order.  margin_rank is FIVE
// enqueued steps on one stream (flags, the 64-bit scan, index, pairs, finish), no host synchronisation, nothing sized by device data:
//   pairs:  one wave per 64 consecutive entries.  For every group that meets the tile and every positive of that group the wave forms the
//           hinge terms of its own negatives, counts the active lanes by ballot and adds the count to the positive's INTEGER counter
//           (order-independent, exact); every lane keeps its own negative's count and its own sum of terms.  The negatives' gradients
//           are written here, the tile's loss partial goes to the workspace.  Work = sum over groups of P_g x (tiles of the group).
//   finish: the positives' counters become fp32 gradients; the first workgroup adds the tile partials in a fixed order (256 consecutive
//           runs, each in index order, then the 256 run sums in index order).
// No floating-point atomics anywhere: two calls on the same input give the same bits.
#include <cmath>

#include "txe_groups.h"

namespace txe {

constexpr int PL_WAVES = 16;

// lanes -> wave (fixed DPP tree) -> workgroup (wave order); every thread of the workgroup must arrive.  The total is valid in thread 0.
__device__ __forceinline__ float block_sum_fixed(float v, float* s_part) {
    const float w = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = w;
    __syncthreads();
    float tot = 0.f;
    if (threadIdx.x == 0) {
        const int nw = (int)(blockDim.x >> 6);
        for (int i = 0; i < nw; ++i) tot += s_part[i];
    }
    __syncthreads();
    return tot;
}

// KIND 0: bce, 1: square_exp.  One workgroup.
template <typename L, int KIND>
__global__ __launch_bounds__(PL_WAVES * 64) void pointwise_loss_kernel(const float* __restrict__ x, const L* __restrict__ lab, int B, float beta,
                                                                      float* __restrict__ loss, float* __restrict__ d_x) {
    __shared__ float s_part[PL_WAVES];
    float a0 = 0.f, a1 = 0.f;                         // bce: all terms in a0; square_exp: squares in a0, exponentials in a1
#pragma unroll 4
    for (int i = threadIdx.x; i < B; i += PL_WAVES * 64) {
        const float xi = x[i];
        const L t = lab[i];
        if (KIND == 0) {
            // One workgroup does all B scores, so the per-score arithmetic is the launch's time: the hardware exp2 / log2 / reciprocal
            // (1 ulp each), not the library's expf / log1pf and correctly rounded divisions (DESIGN 4.11 has both times).
            const float e = __expf(-fabsf(xi));       // in [0, 1]: nothing overflows, +-1e4 gives 0
            const float u = 1.f + e;
            const float r = __builtin_amdgcn_rcpf(u);  // v_rcp_f32 (a `/` is a ten-instruction correctly rounded division)
            const float big = xi >= 0.f ? r : e * r;  // sigmoid(x)
            const float small = xi >= 0.f ? e * r : r;   // sigmoid(-x) = 1 - sigmoid(x), without the cancellation
            const float z = (t == 1) ? xi : -xi;
            // log1p(e) = log(u) * e / (u - 1): u - 1 is exact, and the quotient undoes the rounding of 1 + e, so a small term keeps its
            // relative accuracy; u == 1: log1p(e) = e to fp32
            const float um1 = u - 1.f;
            const float l1p = um1 == 0.f ? e : __logf(u) * (e * __builtin_amdgcn_rcpf(um1));
            a0 += fmaxf(z, 0.f) + l1p;                // a NaN score: fmaxf gives 0, l1p carries the NaN
            d_x[i] = (t == 1) ? big : -small;
        } else {
            float d = 0.f;
            if (t == 1) {
                a0 += xi * xi;
                d = 2.f * xi;
            } else if (t == 0) {
                const float e = expf(-xi);            // fp32 overflow gives +Inf, as the torch expression does
                a1 += e;
                d = -beta * e;
            }
            d_x[i] = d;
        }
    }
    const float t0 = block_sum_fixed(a0, s_part);
    const float t1 = KIND == 1 ? block_sum_fixed(a1, s_part) : 0.f;
    if (threadIdx.x == 0) loss[0] = KIND == 1 ? t0 + beta * t1 : t0;
}

__global__ __launch_bounds__(256) void margin_pairs_kernel(const float* __restrict__ score, const u64* __restrict__ v, const u64* __restrict__ e, int B,
                                                           float margin, const int* __restrict__ pos_off, const int* __restrict__ pos_elem,
                                                           int* __restrict__ cnt, float* __restrict__ d_x, float* __restrict__ partial) {
    const int l = threadIdx.x & 63;
    const long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long t0 = tile * 64;
    if (t0 >= B) return;                                           // (wave-uniform)
    const long long i = t0 + l;
    const bool valid = i < B;
    int g = -1;
    float s = 0.f;
    bool neg = false;
    if (valid) {
        const u64 vi = v[i];
        g = (int)(e[i] >> 32) + (int)(vi >> 32) - 1;
        s = score[i];
        neg = (vi & 1ull) == 0ull;
    }
    const int last = (int)((B - 1 - t0) < 63 ? (B - 1 - t0) : 63);
    const int g0 = __builtin_amdgcn_readfirstlane(__shfl(g, 0)), g1 = __builtin_amdgcn_readfirstlane(__shfl(g, last));   // (uniform: scalar loop)
    int mine = 0;                                                  // this negative's active positives
    float acc = 0.f;                                               // this negative's hinge terms, in positive order
    for (int gg = g0; gg <= g1; ++gg) {
        const int p1 = pos_off[gg + 1];
        for (int p = pos_off[gg]; p < p1; ++p) {
            const float sp = score[pos_elem[p]];
            const float d = sp - s;
            const float t = d + margin;                            // (no multiply: nothing contracts to an FMA)
            const bool pair = neg && g == gg;
            const bool active = pair && t > 0.f;
            const u64 m = __ballot(active);
            if (active) ++mine;
            if (pair && !(t <= 0.f)) acc += t;                     // t > 0, or NaN (torch's clamp_min keeps a NaN)
            if (l == 0 && m) atomicAdd(cnt + p, (int)__popcll(m));
        }
    }
    if (valid && neg) d_x[i] = mine ? -(float)mine : 0.f;
    const float tot = wave_sum(acc);                               // all 64 lanes are here: the early return above is wave-uniform
    if (l == 0) partial[tile] = tot;
}

__global__ __launch_bounds__(256) void margin_finish_kernel(const u64* __restrict__ v, const u64* __restrict__ e, int B, const int* __restrict__ cnt,
                                                            const float* __restrict__ partial, int tiles, float* __restrict__ d_x,
                                                            float* __restrict__ loss) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < B; i += (long long)gridDim.x * 256)
        if (v[i] & 1ull) d_x[i] = (float)cnt[(int)(e[i] & 0xffffffffull)];
    if (blockIdx.x == 0) {
        __shared__ float s_run[256];
        const int per = (tiles + 255) / 256;
        const int a = (int)threadIdx.x * per, b = (a + per < tiles) ? a + per : tiles;
        float r = 0.f;
        for (int t = a; t < b; ++t) r += partial[t];
        s_run[threadIdx.x] = r;
        __syncthreads();
        if (threadIdx.x == 0) {
            float tot = 0.f;
            for (int k = 0; k < 256; ++k) tot += s_run[k];
            loss[0] = tot;
        }
    }
}

// the workspace of txe_margin_rank_loss, a function of B alone: byte offsets of its parts
struct MarginWs {
    size_t v, e, pos_elem, pos_off, cnt, partial, temp, total;
};

static MarginWs margin_ws(int B) {
    MarginWs w;
    size_t o = 0;
    const size_t tiles = ((size_t)B + 63) / 64;
    w.v = o;        o += align256((size_t)B * 8);            // u64 [B]: the flags
    w.e = o;        o += align256((size_t)B * 8);            // u64 [B]: their exclusive scan
    w.pos_elem = o; o += align256((size_t)B * 4);            // int [B]
    w.pos_off = o;  o += align256(((size_t)B + 1) * 4);      // int [B + 1]
    w.cnt = o;      o += align256((size_t)B * 4);            // int [B]: active negatives per positive
    w.partial = o;  o += align256(tiles * 4);                // float [tiles]
    w.temp = o;     o += align256(group_scan_temp_bytes(B));
    w.total = o;
    return w;
}

template <typename L, int KIND>
static int pointwise_impl(const char* name, const float* x, const L* lab, int B, float beta, float* loss, float* d_x, hipStream_t s) {
    ProfScope prof(name, s, (double)B * (8.0 + sizeof(L)) + 4.0, 1);
    hipLaunchKernelGGL((pointwise_loss_kernel<L, KIND>), dim3(1), dim3(PL_WAVES * 64), 0, s, x, lab, B, beta, loss, d_x);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

template <typename L>
static int margin_impl(const float* x, const L* lab, int B, float margin, float* loss, float* d_x, char* ws, size_t ws_bytes, hipStream_t s) {
    const MarginWs o = margin_ws(B);
    struct { u64 *v, *e; int *pos_elem, *pos_off, *cnt; float* partial; char* temp; } w = {
        (u64*)(ws + o.v), (u64*)(ws + o.e), (int*)(ws + o.pos_elem), (int*)(ws + o.pos_off), (int*)(ws + o.cnt), (float*)(ws + o.partial), ws + o.temp};
    const size_t temp_bytes = ws_bytes - o.temp;
    const int blocks = group_blocks(B);
    const int tiles = (int)((B + 63LL) / 64);
    {
        ProfScope prof("group_flags_kernel", s, (double)B * (8.0 + sizeof(L)), 1);
        hipLaunchKernelGGL(group_flags_kernel<L>, dim3(blocks), dim3(256), 0, s, lab, B, w.v);
        TXE_CHECK_LAUNCH();
    }
    {
        ProfScope prof("group_scan", s, 16.0 * B, 1);
        if (!group_scan(w.v, w.e, B, w.temp, temp_bytes, s)) return TXE_ERR_LAUNCH;
    }
    {
        ProfScope prof("group_index_kernel<0>", s, 24.0 * B, 1);
        hipLaunchKernelGGL(group_index_kernel<0>, dim3(blocks), dim3(256), 0, s, w.v, w.e, B, w.pos_off, w.pos_elem, w.cnt, (int*)nullptr);
        TXE_CHECK_LAUNCH();
    }
    {
        ProfScope prof("margin_pairs_kernel", s, 24.0 * B + 4.0 * tiles, 1);
        hipLaunchKernelGGL(margin_pairs_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, s, x, w.v, w.e, B, margin, w.pos_off, w.pos_elem,
                           w.cnt, d_x, w.partial);
        TXE_CHECK_LAUNCH();
    }
    {
        ProfScope prof("margin_finish_kernel", s, 24.0 * B + 4.0 * tiles + 4.0, 1);
        hipLaunchKernelGGL(margin_finish_kernel, dim3(blocks), dim3(256), 0, s, w.v, w.e, B, w.cnt, w.partial, tiles, d_x, loss);
        TXE_CHECK_LAUNCH();
    }
    return TXE_OK;
}

}  // namespace txe

using namespace txe;

extern "C" {

int txe_bce_loss(const float* x, const void* labels, int label_bytes, int B, float* loss, float* d_x, void* stream) {
    if (!x || !labels || !loss || !d_x) return TXE_ERR_ARG;
    if (B < 1 || (label_bytes != 4 && label_bytes != 8)) return TXE_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (label_bytes == 4) return pointwise_impl<int, 0>("bce_loss_kernel", x, (const int*)labels, B, 0.f, loss, d_x, s);
    return pointwise_impl<long long, 0>("bce_loss_kernel", x, (const long long*)labels, B, 0.f, loss, d_x, s);
}

int txe_square_exp_loss(const float* x, const void* labels, int label_bytes, int B, float beta, float* loss, float* d_x, void* stream) {
    if (!x || !labels || !loss || !d_x) return TXE_ERR_ARG;
    if (B < 1 || (label_bytes != 4 && label_bytes != 8) || !std::isfinite(beta)) return TXE_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (label_bytes == 4) return pointwise_impl<int, 1>("square_exp_loss_kernel", x, (const int*)labels, B, beta, loss, d_x, s);
    return pointwise_impl<long long, 1>("square_exp_loss_kernel", x, (const long long*)labels, B, beta, loss, d_x, s);
}

size_t txe_margin_rank_loss_ws_bytes(int B) {
    if (B < 1) return 0;
    return margin_ws(B).total;
}

int txe_margin_rank_loss(const float* x, const void* labels, int label_bytes, int B, float margin, float* loss, float* d_x, void* ws,
                         size_t ws_bytes, void* stream) {
    if (!x || !labels || !loss || !d_x || !ws) return TXE_ERR_ARG;
    if (B < 1 || (label_bytes != 4 && label_bytes != 8) || !std::isfinite(margin)) return TXE_ERR_ARG;
    if (ws_bytes < txe_margin_rank_loss_ws_bytes(B)) return TXE_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (label_bytes == 4) return margin_impl(x, (const int*)labels, B, margin, loss, d_x, (char*)ws, ws_bytes, s);
    return margin_impl(x, (const long long*)labels, B, margin, loss, d_x, (char*)ws, ws_bytes, s);
}

}  // extern "C"
