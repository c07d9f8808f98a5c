// In-batch negatives: the masked all-pairs InfoNCE of a training batch.  Every query row i of the score matrix S [Q][G] is a
// cross entropy over the batch's G egonet columns, without the columns whose anchor lies in node2masks[qnode[i]] -- the query's other
// parents, its siblings' positives, its descendants -- and with its own positive pos_col[i] always in:
//     valid(i, g) = (g == pos_col[i]) or anchor[g] not in mask row of qnode[i]
//     loss = sum_i (log sum_{g valid} exp S[i][g] - S[i][pos_col[i]]),   dS[i][g] = softmax over the valid g - [g == pos_col[i]], 0 where not valid
// Two launches: one workgroup per row (validity, max, sum, gradient, the row's loss), then one workgroup that adds the row losses in a
// fixed order in float64.  No floating-point atomics anywhere: two calls on the same inputs give the same bytes.
#include "txe_common.h"

namespace txe {

constexpr int IB_THREADS = 256, IB_WAVES = IB_THREADS / 64;
constexpr int IB_BIT_WORDS = 1024;                       // validity bits kept in LDS: 64 columns per word
constexpr long long IB_BIT_COLS = 64ll * IB_BIT_WORDS;   // rows up to 65,536 columns search every column once; longer rows once per pass

// is `a` in the ascending mask row mask_idx[lo .. hi)?  The row stays in global memory (10^5 entries on the big taxonomies): 17 probes.
__device__ __forceinline__ bool in_mask_row(const int* __restrict__ mask_idx, int lo, int hi, int a) {
    const int end = hi;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (mask_idx[mid] < a) lo = mid + 1; else hi = mid;
    }
    return lo < end && mask_idx[lo] == a;
}

// One workgroup per query row; a wave takes 64 consecutive columns per pass, so a pass's validity is one ballot word: lane 0 keeps it in
// LDS and the two later passes of the SAME wave read it back (a broadcast read).  S and d_out may be the same buffer: an element is
// overwritten by the thread that read it, in the last pass, and the positive's score is read before the first barrier.
__global__ __launch_bounds__(IB_THREADS) void inbatch_nce_kernel(const float* S, long long ld_s, int G, const int* __restrict__ pos_col,
                                                                 const int* __restrict__ anchor, const int* __restrict__ qnode,
                                                                 const int* __restrict__ mask_ptr, const int* __restrict__ mask_idx,
                                                                 int chain_exp, float* d_out, long long ld_d, int* __restrict__ n_valid,
                                                                 float* __restrict__ row_loss, int* __restrict__ row_cnt) {
    __shared__ unsigned long long s_bits[IB_BIT_WORDS];
    __shared__ float s_max[IB_WAVES], s_sum[IB_WAVES];
    __shared__ int s_cnt[IB_WAVES];
    const int i = blockIdx.x, w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const float* row = S + (long long)i * ld_s;
    float* drow = d_out + (long long)i * ld_d;
    const int t = pos_col[i];
    const float xt = row[t];
    int lo = 0, hi = 0;                                  // the query's mask row; empty when nothing is masked
    if (mask_ptr) { const int q = qnode[i]; lo = mask_ptr[q]; hi = mask_ptr[q + 1]; }
    const bool keep_bits = G <= IB_BIT_COLS;

    // pass 1: validity (the one search per column), the count, the maximum over the valid columns
    float m = -INFINITY;
    int cnt = 0;
    for (long long g0 = w * 64; g0 < G; g0 += IB_THREADS) {          // (wave-uniform bounds: every lane reaches the ballot)
        const long long g = g0 + l;
        bool v = false;
        if (g < G) v = (g == t) || !in_mask_row(mask_idx, lo, hi, anchor[g]);
        const unsigned long long b = __ballot(v);
        if (keep_bits && l == 0) s_bits[g0 >> 6] = b;
        cnt += __popcll(b);
        if (v) m = fmaxf(m, row[g]);                                 // (a NaN is dropped here and poisons the sum below)
    }
    m = wave_max(m);
    if (l == 0) { s_max[w] = m; s_cnt[w] = cnt; }
    __syncthreads();
    m = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    auto valid = [&](long long g0, long long g) -> bool {
        if (keep_bits) return (s_bits[g0 >> 6] >> l) & 1ull;
        return g < G && ((g == t) || !in_mask_row(mask_idx, lo, hi, anchor[g]));
    };

    // pass 2: the sum of exp(S - max) over the valid columns
    float s = 0.f;
    for (long long g0 = w * 64; g0 < G; g0 += IB_THREADS) {
        const long long g = g0 + l;
        if (valid(g0, g)) s += expf(row[g] - m);
    }
    s = wave_sum(s);
    if (l == 0) s_sum[w] = s;
    __syncthreads();
    s = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);

    // pass 3: the gradient, exactly 0 where the column is masked (whatever its score holds)
    const float inv = 1.f / s;
    for (long long g0 = w * 64; g0 < G; g0 += IB_THREADS) {
        const long long g = g0 + l;
        if (g >= G) continue;
        float d = 0.f;
        if (valid(g0, g)) {
            const float x = row[g];
            d = expf(x - m) * inv - (g == t ? 1.f : 0.f);
            if (chain_exp) d *= x;
        }
        drow[g] = d;
    }
    if (threadIdx.x == 0) {
        const int n = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        row_loss[i] = (m + logf(s)) - xt;
        row_cnt[i] = n;
        if (n_valid) n_valid[i] = n;
    }
}

// the row losses in a fixed order, in float64: thread t adds rows t, t + 256, ..., then a tree over the threads
__global__ __launch_bounds__(IB_THREADS) void inbatch_nce_finish_kernel(const float* __restrict__ row_loss, const int* __restrict__ row_cnt,
                                                                        int Q, float* __restrict__ loss, unsigned long long* valid_total) {
    __shared__ double s_l[IB_THREADS];
    __shared__ unsigned long long s_c[IB_THREADS];
    double a = 0.0;
    unsigned long long c = 0;
    for (int i = threadIdx.x; i < Q; i += IB_THREADS) { a += (double)row_loss[i]; c += (unsigned long long)row_cnt[i]; }
    s_l[threadIdx.x] = a; s_c[threadIdx.x] = c;
    __syncthreads();
    for (int o = IB_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { s_l[threadIdx.x] += s_l[threadIdx.x + o]; s_c[threadIdx.x] += s_c[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss[0] = (float)s_l[0];
        if (valid_total) atomicAdd(valid_total, s_c[0]);             // (an integer: exact in any order)
    }
}

__global__ __launch_bounds__(IB_THREADS) void inbatch_exp_kernel(float* B, long long ld_b, int G, long long n) {
    for (long long e = (long long)blockIdx.x * IB_THREADS + threadIdx.x; e < n; e += (long long)gridDim.x * IB_THREADS) {
        float* p = B + (e / G) * ld_b + (e % G);
        *p = expf(*p);
    }
}

static inline size_t ib_align16(size_t n) { return (n + 15) / 16 * 16; }

}  // namespace txe

using namespace txe;

extern "C" {

// ws: [Q] float row losses, then [Q] int row counts
size_t txe_inbatch_nce_ws_bytes(int Q) { return 2 * ib_align16((size_t)(Q > 0 ? Q : 1) * 4); }

int txe_inbatch_nce(const float* S, long long ld_s, int Q, int G, const int* pos_col, const int* anchor, const int* qnode,
                    const int* mask_ptr, const int* mask_idx, int chain_exp, float* loss, float* d_out, long long ld_d, int* n_valid,
                    long long* valid_total, void* ws, size_t ws_bytes, void* stream) {
    if (Q < 0 || G < 1 || (long long)Q * G >= (1ll << 31) || ld_s < G || ld_d < G) return TXE_ERR_ARG;
    if (!S || !pos_col || !anchor || !qnode || !loss || !d_out || ((mask_ptr == nullptr) != (mask_idx == nullptr))) return TXE_ERR_ARG;
    if (!ws || ws_bytes < txe_inbatch_nce_ws_bytes(Q)) return TXE_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (Q == 0) return hipMemsetAsync(loss, 0, sizeof(float), s) == hipSuccess ? TXE_OK : TXE_ERR_LAUNCH;
    float* row_loss = (float*)ws;
    int* row_cnt = (int*)((char*)ws + ib_align16((size_t)Q * 4));
    {
        ProfScope prof("inbatch_nce_kernel", s, 16.0 * Q * (double)G, 1);        // (bytes: three reads of S, one write of d_out)
        hipLaunchKernelGGL(inbatch_nce_kernel, dim3(Q), dim3(IB_THREADS), 0, s, S, ld_s, G, pos_col, anchor, qnode, mask_ptr, mask_idx, chain_exp,
                           d_out, ld_d, n_valid, row_loss, row_cnt);
        TXE_CHECK_LAUNCH();
    }
    {
        ProfScope prof("inbatch_nce_finish_kernel", s, 8.0 * Q + 4.0, 1);
        hipLaunchKernelGGL(inbatch_nce_finish_kernel, dim3(1), dim3(IB_THREADS), 0, s, row_loss, row_cnt, Q, loss, (unsigned long long*)valid_total);
        TXE_CHECK_LAUNCH();
    }
    return TXE_OK;
}

int txe_inbatch_exp(float* B, long long ld_b, int Q, int G, void* stream) {
    if (Q < 0 || G < 1 || ld_b < G || (Q > 0 && !B)) return TXE_ERR_ARG;
    if (Q == 0) return TXE_OK;
    const long long n = (long long)Q * G, blocks = (n + IB_THREADS - 1) / IB_THREADS;
    ProfScope prof("inbatch_exp_kernel", (hipStream_t)stream, 8.0 * (double)n, 1);
    hipLaunchKernelGGL(inbatch_exp_kernel, dim3((int)(blocks < 2048 ? blocks : 2048)), dim3(IB_THREADS), 0, (hipStream_t)stream, B, ld_b, G, n);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

}  // extern "C"
