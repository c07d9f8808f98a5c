// The retrieval stage of the two-stage test protocol (data_loader/dataset.py:316-330): per query the k unmasked candidates nearest by
// cosine distance.  Rows are normalised once (row_normalize_kernel), the similarity block S = Qn Cn^T comes from txe_score_block, and
// this unit selects: per row of S the k unmasked columns with the largest value, best first, equal values by ascending column, NaN
// last (NaN takes the key of -inf; -0.0 and +0.0 tie) -- the order of topk_parents / txe_topk_merge.
//
// select_k_kernel, one workgroup of 1,024 threads per row, no write into S:
//   keys    ord(x): the float's bits as an unsigned of the same order (larger float = larger ord).
//   masks   a bitmap [nq][ceil(G / 32)] in the caller's workspace, zeroed and marked (atomicOr: the result does not depend on order)
//           by mask_mark_kernel ahead of the selection; no masks at all: no bitmap, no extra read.
//   radix   three histogram passes over the row (12 + 12 + 8 bits of ord, LDS integer counters) find T = the k-th largest key, the
//           number n_gt of keys above it and the number of keys equal to it.
//   emit    a fourth pass collects every key above T into LDS (slot from an LDS counter: the slots' order varies from run to run, the
//           SET does not, and the sort below orders it by a total order).  Keys equal to T: all of them when exactly as many are
//           needed; otherwise (ties straddle the k-th place) the lowest columns, found in column order -- every wave walks one
//           contiguous stretch of the row, counts its ties, and a fifth pass places them behind the waves before it.
//   sort    bitonic sort of the <= 4,096 survivors in LDS on (ord, ~column), descending; unused output slots get -1.
// Every step is integer counting or a sort on distinct 64-bit keys: the output is a pure function of the row.
#include "txe_common.h"

namespace txe {

typedef unsigned long long u64;

constexpr int SEL_THREADS = 1024;
constexpr int SEL_WAVES = SEL_THREADS / TXE_WAVE;
constexpr int SEL_KMAX = 4096;
constexpr int SEL_BINS = 4096;

__global__ __launch_bounds__(256) void row_normalize_kernel(const float* __restrict__ x, long long ld_x, int n, int d, float* __restrict__ y,
                                                            long long ld_y) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;                                          // (wave-uniform)
    const float* xr = x + row * ld_x;
    float* yr = y + row * ld_y;
    float s = 0.f;
    for (int c = lane; c < d; c += 64) {
        const float v = xr[c];
        s += v * v;
    }
    const float nrm = sqrtf(wave_sum(s));                          // a zero row: 0 / 0 = NaN; an infinite entry: inf / inf = NaN
    for (int c = lane; c < d; c += 64) yr[c] = xr[c] / nrm;
}

__global__ __launch_bounds__(256) void mask_mark_kernel(const int* __restrict__ mask_off, const int* __restrict__ mask_idx, int G, int W,
                                                        unsigned* __restrict__ bits) {
    const long long row = blockIdx.x;
    const long long a = mask_off[row], b = mask_off[row + 1];
    for (long long j = a + threadIdx.x; j < b; j += 256) {
        const int c = mask_idx[j];
        if ((unsigned)c < (unsigned)G) atomicOr(bits + row * W + (c >> 5), 1u << (c & 31));      // a column outside the row masks nothing
    }
}

__device__ __forceinline__ unsigned sel_ord(float x) {
    unsigned u = __float_as_uint(x);
    if (x != x) u = 0xFF800000u;                                   // NaN ranks with -inf
    if (u == 0x80000000u) u = 0u;                                  // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct SelRow {
    const float* s;
    const unsigned* mb;
    __device__ __forceinline__ bool get(int c, unsigned& o) const {
        if (mb && ((mb[c >> 5] >> (c & 31)) & 1u)) return false;
        o = sel_ord(s[c]);
        return true;
    }
};

// the bin of the 4,096-entry histogram that holds the `need`-th largest key: *bin, *above = keys in higher bins, *in_bin = keys in it,
// returns the histogram's total (need is clamped to it).  Every thread gets the same answers; ends with the LDS free for re-use.
__device__ __forceinline__ int sel_find_bin(const unsigned* hist, int* wsum, int* res, int need, int& bin, int& above, int& in_bin) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = (int)hist[4 * tid], c1 = (int)hist[4 * tid + 1], c2 = (int)hist[4 * tid + 2], c3 = (int)hist[4 * tid + 3];
    const int v = c0 + c1 + c2 + c3;
    int x = v;                                                     // -> the sum over this wave's lanes >= lane
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_down(x, d);
        if (lane + d < 64) x += t;
    }
    if (lane == 0) wsum[wave] = x;
    __syncthreads();
    int higher = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SEL_WAVES; ++w) {
        const int t = wsum[w];
        total += t;
        higher += (w > wave) ? t : 0;
    }
    need = need < total ? need : total;
    int ab = higher + x - v;                                       // keys in the bins above this thread's four
    const int cs[4] = {c3, c2, c1, c0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (ab < need && ab + cs[j] >= need) {                     // (exactly one bin of one thread when need >= 1)
            res[0] = 4 * tid + 3 - j;
            res[1] = ab;
            res[2] = cs[j];
        }
        ab += cs[j];
    }
    __syncthreads();
    bin = res[0];
    above = res[1];
    in_bin = res[2];
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(SEL_THREADS) void select_k_kernel(const float* __restrict__ S, long long ld_s, int G, const unsigned* __restrict__ bits,
                                                               int W, int k, int* __restrict__ out_idx, float* __restrict__ out_key) {
    __shared__ unsigned hist[SEL_BINS];
    __shared__ u64 buf[SEL_KMAX];
    __shared__ int wsum[SEL_WAVES];
    __shared__ int res[3];
    __shared__ int n_emit;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row = blockIdx.x;
    SelRow r;
    r.s = S + row * ld_s;
    r.mb = bits ? bits + row * W : nullptr;
    int* oi = out_idx + row * k;
    float* ok = out_key ? out_key + row * k : nullptr;

    // ---- radix passes: bits [31:20], [19:8], [7:0] of ord --------------------------------------------------------------------------
    int need = k, n_gt = 0, n_eq = 0, k_eff = 0;
    unsigned T = 0;
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
        for (int i = tid; i < SEL_BINS; i += SEL_THREADS) hist[i] = 0u;
        __syncthreads();
        const int shift = pass == 0 ? 20 : (pass == 1 ? 8 : 0);
        const unsigned bmask = pass == 2 ? 0xFFu : 0xFFFu;
        const int pshift = pass == 1 ? 20 : 8;                     // the bits above `shift + width` must equal T's (pass 0: none)
#pragma unroll 4
        for (int c = tid; c < G; c += SEL_THREADS) {
            unsigned o;
            if (r.get(c, o) && (pass == 0 || (o >> pshift) == (T >> pshift))) atomicAdd(&hist[(o >> shift) & bmask], 1u);
        }
        __syncthreads();
        int bin, above, in_bin;
        const int total = sel_find_bin(hist, wsum, res, need, bin, above, in_bin);
        if (pass == 0) {
            k_eff = k < total ? k : total;                         // fewer than k unmasked columns: all of them
            need = k_eff;
            if (total == 0) {                                      // (block-uniform)
                for (int i = tid; i < k; i += SEL_THREADS) {
                    oi[i] = -1;
                    if (ok) ok[i] = -INFINITY;
                }
                return;
            }
        }
        T |= (unsigned)bin << shift;
        n_gt += above;
        need -= above;
        n_eq = in_bin;
    }
    const int need_eq = need;                                      // 1 <= need_eq <= n_eq, n_gt + need_eq = k_eff
    const bool all_eq = n_eq == need_eq;

    // ---- emit: every wave walks one contiguous stretch of the row ------------------------------------------------------------------
    if (tid == 0) n_emit = 0;
    __syncthreads();
    const int seg = (((G + SEL_WAVES - 1) / SEL_WAVES) + 63) / 64 * 64;
    const long long b0 = (long long)wave * seg;
    const int beg = (int)(b0 < G ? b0 : G), end = (int)(b0 + seg < G ? b0 + seg : G);
    int weq = 0;
    for (int base = beg; base < end; base += 64) {                 // (wave-uniform bounds)
        const int c = base + lane;
        unsigned o = 0u;
        const bool valid = c < end && r.get(c, o);
        const bool eq = valid && o == T;
        if (valid && (o > T || (eq && all_eq))) {
            const int slot = atomicAdd(&n_emit, 1);
            if (slot < SEL_KMAX) buf[slot] = ((u64)o << 32) | (u64)(0xFFFFFFFFu - (unsigned)c);
        }
        if (!all_eq) weq += (int)__popcll(__ballot(eq));
    }
    if (!all_eq) {                                                 // (block-uniform) ties straddle the k-th place: the lowest columns
        if (lane == 0) wsum[wave] = weq;
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        for (int base = beg; base < end && before < need_eq; base += 64) {
            const int c = base + lane;
            unsigned o = 0u;
            const bool eq = c < end && r.get(c, o) && o == T;
            const u64 m = __ballot(eq);
            const int rank = before + (int)__popcll(m & ((1ull << lane) - 1ull));
            if (eq && rank < need_eq && n_gt + rank < SEL_KMAX) buf[n_gt + rank] = ((u64)o << 32) | (u64)(0xFFFFFFFFu - (unsigned)c);
            before += (int)__popcll(m);
        }
    }
    __syncthreads();

    // ---- sort the k_eff survivors: (ord, ~column) descending = best first, equal keys by ascending column --------------------------
    int P = 1;
    while (P < k_eff) P <<= 1;
    for (int i = k_eff + tid; i < P; i += SEL_THREADS) buf[i] = 0ull;       // below every real entry (ord >= 0x007FFFFF)
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (P >> 1); t += SEL_THREADS) {
                const int j = t & (stride - 1);
                const int a = ((t - j) << 1) + j, b = a + stride;
                const u64 va = buf[a], vb = buf[b];
                const bool desc = (a & size) == 0;
                if ((va < vb) == desc) {
                    buf[a] = vb;
                    buf[b] = va;
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < k; i += SEL_THREADS) {
        if (i < k_eff) {
            const int c = (int)(0xFFFFFFFFu - (unsigned)(buf[i] & 0xFFFFFFFFull));
            oi[i] = c;
            if (ok) {
                const float v = r.s[(unsigned)c < (unsigned)G ? c : 0];
                ok[i] = (v != v) ? -INFINITY : v;
            }
        } else {
            oi[i] = -1;
            if (ok) ok[i] = -INFINITY;
        }
    }
}

}  // namespace txe

using namespace txe;

extern "C" {

int txe_row_normalize(const float* x, long long ld_x, int n, int d, float* y, long long ld_y, void* stream) {
    if (!x || !y || n < 0 || d < 1 || ld_x < d || ld_y < d) return TXE_ERR_ARG;
    if (n == 0) return TXE_OK;
    ProfScope prof("row_normalize", (hipStream_t)stream, 8.0 * n * d, 1);
    hipLaunchKernelGGL(row_normalize_kernel, dim3((unsigned)((n + 3LL) / 4)), dim3(256), 0, (hipStream_t)stream, x, ld_x, n, d, y, ld_y);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

size_t txe_select_k_ws_bytes(int nq, int G) {
    if (nq < 1 || G < 1) return 0;
    return (size_t)nq * (size_t)((G + 31) / 32) * 4;
}

int txe_select_k(const float* S, long long ld_s, int nq, int G, const int* mask_off, const int* mask_idx, int k, int* out_idx, float* out_key,
                 void* ws, size_t ws_bytes, void* stream) {
    if (k < 1 || k > SEL_KMAX) return TXE_ERR_ARG;
    if (!S || !out_idx || nq < 0 || G < 1 || G > 0x7fffffff - SEL_WAVES * 64 - 64 || ld_s < G) return TXE_ERR_ARG;
    if ((mask_off == nullptr) != (mask_idx == nullptr)) return TXE_ERR_ARG;
    if (nq == 0) return TXE_OK;
    hipStream_t s = (hipStream_t)stream;
    unsigned* bits = nullptr;
    const int W = (G + 31) / 32;
    if (mask_off) {
        const size_t need = txe_select_k_ws_bytes(nq, G);
        if (!ws) return TXE_ERR_ARG;
        if (ws_bytes < need) return TXE_ERR_WORKSPACE;
        bits = (unsigned*)ws;
        if (hipMemsetAsync(bits, 0, need, s) != hipSuccess) return TXE_ERR_LAUNCH;
        hipLaunchKernelGGL(mask_mark_kernel, dim3((unsigned)nq), dim3(256), 0, s, mask_off, mask_idx, G, W, bits);
        TXE_CHECK_LAUNCH();
    }
    ProfScope prof("select_k", s, 16.0 * nq * G, 1);
    hipLaunchKernelGGL(select_k_kernel, dim3((unsigned)nq), dim3(SEL_THREADS), 0, s, S, ld_s, G, bits, W, k, out_idx, out_key);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

}  // extern "C"
