// Grouped ranking of a labelled score vector (model/metric.py:33-60 obtain_ranks) and the per-batch metric reduction
// (model/metric.py:62-96) on the device.
//
// Groups start at index 0 and at every i with label[i-1] == 0 and label[i] == 1 (the reference splits at every [0, 1] pair of the
// label bytes).  Positives are the entries with label 1; every other entry of the group is a negative.  The rank of a positive is
// 1 + the number of negatives of its group that are strictly better in fp32 (mode 0: smaller, mode 1: larger): NaN never compares true,
// ties never count.  A group without negatives ranks its positives 1 (the reference's numpy gives masked values there).
//
// Steps (one stream, no host synchronisation):
//   flags: v[i] = (group start) << 32 | (positive) -- a single 64-bit exclusive scan (hipcub) gives both the group index (high half) and
//          the positive index (low half) of every entry; B < 2^31 keeps the low half from carrying.
//   index: pos_off[g] = positives before group g, pos_elem[p] = the entry of positive p, ranks[p] = 1, counts = {n_groups, n_pos}.
//   rank:  one wave per 64 consecutive entries; for every group that meets the tile and every positive of that group, the wave counts
//          its own better negatives (ballot) and adds them to the positive's rank.  Work = sum over groups of P_g x (tiles of the group).
#include "txe_groups.h"      // group_flags_kernel, the scan, group_index_kernel: shared with txe_pairloss.hip

namespace txe {

template <typename L, int MODE>
__global__ __launch_bounds__(256) void group_rank_kernel(const float* __restrict__ score, const L* __restrict__ lab, const u64* __restrict__ v,
                                                         const u64* __restrict__ e, int B, const int* __restrict__ pos_off,
                                                         const int* __restrict__ pos_elem, int* __restrict__ ranks) {
    const int l = threadIdx.x & 63;
    const long long t0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (t0 >= B) return;                                           // (wave-uniform)
    const long long i = t0 + l;
    const bool valid = i < B;
    int g = -1;
    float s = 0.f;
    bool neg = false;
    if (valid) {
        g = (int)(e[i] >> 32) + (int)(v[i] >> 32) - 1;
        s = score[i];
        neg = lab[i] != 1;
    }
    const int last = (int)((B - 1 - t0) < 63 ? (B - 1 - t0) : 63);
    const int g0 = __shfl(g, 0), g1 = __shfl(g, last);
    for (int gg = g0; gg <= g1; ++gg) {
        const int p1 = pos_off[gg + 1];
        for (int p = pos_off[gg]; p < p1; ++p) {
            const float sp = score[pos_elem[p]];
            const bool better = MODE == 0 ? (s < sp) : (s > sp);
            const u64 m = __ballot(neg && g == gg && better);
            if (l == 0 && m) atomicAdd(ranks + p, (int)__popcll(m));
        }
    }
}

// metric ids (taxoexpan_amd/metric.py METRIC_IDS): 0 macro_mr, 1 micro_mr, 2 hit_at_1, 3 hit_at_3, 4 hit_at_5, 5 mrr_scaled_10,
// 6 combined_metrics.  One workgroup; the integer sums are exact, the two fp64 sums are tree-reduced.
__global__ __launch_bounds__(256) void group_metrics_kernel(const int* __restrict__ ranks, const int* __restrict__ pos_off, const int* __restrict__ counts,
                                                            u64 which, int n_which, double* __restrict__ acc) {
    __shared__ long long si[4][256];
    __shared__ double sd[2][256];
    const int tid = threadIdx.x;
    const int ng = counts[0], np_ = counts[1];
    long long sr = 0, h1 = 0, h3 = 0, h5 = 0;
    double mrr = 0.0, mac = 0.0;
    for (int p = tid; p < np_; p += 256) {
        const long long r = ranks[p];
        sr += r;
        h1 += r <= 1;
        h3 += r <= 3;
        h5 += r <= 5;
        mrr += 1.0 / (double)((r + 9) / 10);                      // = 1 / ceil(r / 10) for r >= 1
    }
    for (int g = tid; g < ng; g += 256) {
        const int a = pos_off[g], b = pos_off[g + 1];
        long long s = 0;
        for (int p = a; p < b; ++p) s += ranks[p];
        mac += (double)s / (double)(b - a);                       // an empty group: 0 / 0 = NaN, as the reference's mean of []
    }
    si[0][tid] = sr; si[1][tid] = h1; si[2][tid] = h3; si[3][tid] = h5;
    sd[0][tid] = mrr; sd[1][tid] = mac;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (tid < d) {
            for (int u = 0; u < 4; ++u) si[u][tid] += si[u][tid + d];
            for (int u = 0; u < 2; ++u) sd[u][tid] += sd[u][tid + d];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double n = (double)np_;
        double val[7];
        val[0] = sd[1][0] / (double)ng;
        val[1] = (double)si[0][0] / n;
        val[2] = (double)si[1][0] / n;
        val[3] = (double)si[2][0] / n;
        val[4] = (double)si[3][0] / n;
        val[5] = sd[0][0] / n;
        // Python's max(x, 1e-4) returns x when x is NaN
        const double c_mrr = (1e-4 > val[5]) ? 1e-4 : val[5], c_h3 = (1e-4 > val[3]) ? 1e-4 : val[3], c_h1 = (1e-4 > val[2]) ? 1e-4 : val[2];
        val[6] = val[0] * (1.0 / c_mrr) * (1.0 / c_h3) * (1.0 / c_h1);
        for (int m = 0; m < n_which; ++m) acc[m] += val[(which >> (4 * m)) & 15ull];
        acc[n_which] += (double)ng;
        acc[n_which + 1] += (double)np_;
    }
}

template <typename L>
static int group_rank_impl(const float* score, const L* lab, int B, int mode, int* ranks, int* pos_off, int* counts, char* ws, size_t ws_bytes,
                           hipStream_t s) {
    u64* v = (u64*)ws;
    u64* e = (u64*)(ws + align256((size_t)B * 8));
    int* pos_elem = (int*)(ws + 2 * align256((size_t)B * 8));
    char* temp = ws + 2 * align256((size_t)B * 8) + align256((size_t)B * 4);
    size_t temp_bytes = ws_bytes - (size_t)(temp - ws);
    const int blocks = group_blocks(B);
    hipLaunchKernelGGL(group_flags_kernel<L>, dim3(blocks), dim3(256), 0, s, lab, B, v);
    TXE_CHECK_LAUNCH();
    if (!group_scan(v, e, B, temp, temp_bytes, s)) return TXE_ERR_LAUNCH;
    hipLaunchKernelGGL(group_index_kernel<1>, dim3(blocks), dim3(256), 0, s, v, e, B, pos_off, pos_elem, ranks, counts);
    TXE_CHECK_LAUNCH();
    const long long tiles = (B + 63LL) / 64;
    const dim3 grid((unsigned)((tiles + 3) / 4));
    if (mode == 0)
        hipLaunchKernelGGL((group_rank_kernel<L, 0>), grid, dim3(256), 0, s, score, lab, v, e, B, pos_off, pos_elem, ranks);
    else
        hipLaunchKernelGGL((group_rank_kernel<L, 1>), grid, dim3(256), 0, s, score, lab, v, e, B, pos_off, pos_elem, ranks);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

}  // namespace txe

using namespace txe;

extern "C" {

size_t txe_group_rank_ws_bytes(int B) {
    if (B < 1) return 0;
    return 2 * align256((size_t)B * 8) + align256((size_t)B * 4) + align256(group_scan_temp_bytes(B));
}

int txe_group_rank(const float* score, const void* labels, int label_bytes, int B, int mode, int* ranks, int* pos_off, int* counts, void* ws,
                   size_t ws_bytes, void* stream) {
    if (!score || !labels || !ranks || !pos_off || !counts || !ws) return TXE_ERR_ARG;
    if (B < 1 || (label_bytes != 4 && label_bytes != 8) || (mode != 0 && mode != 1)) return TXE_ERR_ARG;
    if (ws_bytes < txe_group_rank_ws_bytes(B)) return TXE_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (label_bytes == 4) return group_rank_impl(score, (const int*)labels, B, mode, ranks, pos_off, counts, (char*)ws, ws_bytes, s);
    return group_rank_impl(score, (const long long*)labels, B, mode, ranks, pos_off, counts, (char*)ws, ws_bytes, s);
}

int txe_group_metrics(const int* ranks, const int* pos_off, const int* counts, unsigned long long which, int n_which, double* acc, void* stream) {
    if (!ranks || !pos_off || !counts || !acc) return TXE_ERR_ARG;
    if (n_which < 1 || n_which > 16) return TXE_ERR_ARG;
    for (int m = 0; m < n_which; ++m)
        if (((which >> (4 * m)) & 15ull) > 6) return TXE_ERR_ARG;
    hipLaunchKernelGGL(group_metrics_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ranks, pos_off, counts, which, n_which, acc);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

}  // extern "C"
