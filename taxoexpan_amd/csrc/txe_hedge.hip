// Hedged placement ON DEVICE (taxoexpan_amd/hedge.py): the probability mass of every candidate's subtree and, per query
// and threshold, the deepest candidate whose subtree mass reaches the threshold.
//
// Everything is in candidate-column space.  The index (sub_ptr / sub_idx: row a = the columns of a and of its descendants, ascending;
// depth; the work list) is built and validated on the host (HedgeIndex.build) and is read-only here.
//
// txe_hedge_probs   p = fl32(exp(float64(fl32(beta z)) - lse[q])) of a score block [nq, G], written CANDIDATE-MAJOR PT [G, ldq]
//                   through a padded 64 x 64 LDS tile: the reads are coalesced along candidates, the writes along queries.
// txe_hedge_sweep   lanes run across queries.  A wave owns one work item -- a row of at most TXE_HEDGE_SLICE entries, or one slice of
//                   a longer row -- for a tile of 64 consecutive queries: every closure entry is one wave-uniform index load and one
//                   coalesced 256-byte read of PT's row.  The float64 sum is taken strictly left to right from 0.0 (eight loads are
//                   issued before their eight adds), so a mass depends on the list alone: not on the wave, the workgroup, the grid, the
//                   query's lane or the block it came in.  Long rows leave one partial per slice in the workspace and a second launch
//                   adds them in slice order.  Store mode writes mass [G, ldm]; hedge mode keeps per lane and threshold the running best
//                   (depth, mass, column), merges a workgroup's four waves through LDS, writes one partial key per workgroup, and a
//                   small finish launch merges the partial keys per query in slot order.  The best of a total order over distinct
//                   columns does not depend on the merge order; there are no atomics, and every output element has one writer.
//
// Bounds: every work item's row, every closure entry, every workspace slice and every offset is compared against its range BEFORE it
// addresses anything (a bad entry contributes nothing); lanes whose query lies beyond nq neither load nor store.
#include "txe_common.h"

#include <math.h>

#define HEDGE_TILE 64
#define HEDGE_WAVES 4
#define HEDGE_UNROLL 8
#define HEDGE_MAX_SWEEP_WG 1024
#define HEDGE_MAX_LONG_WG 256
#define HEDGE_ITEMS_PER_WAVE 16
#define HEDGE_TP_PITCH 65          // the transposition tile's row pitch in floats: 64 + 1, conflict-free both ways

namespace txe {

struct HedgeTaus {
    double tau[TXE_HEDGE_MAX_THRESHOLDS];
};

// the running best of one (lane, threshold): a strictly better candidate is deeper; at equal depth heavier; at equal mass the smaller column
struct HedgeKey {
    int d;
    int c;
    double m;
};
__device__ __forceinline__ bool hedge_better(int d, double m, int c, const HedgeKey& b) {
    return d > b.d || (d == b.d && (m > b.m || (m == b.m && c < b.c)));
}
__device__ __forceinline__ void hedge_offer(HedgeKey* best, const HedgeTaus& taus, int nt, int d, double m, int c) {
#pragma unroll
    for (int t = 0; t < TXE_HEDGE_MAX_THRESHOLDS; ++t) {
        if (t < nt && m >= taus.tau[t] && hedge_better(d, m, c, best[t])) {
            best[t].d = d;
            best[t].c = c;
            best[t].m = m;
        }
    }
}
__device__ __forceinline__ void hedge_init(HedgeKey* best) {
#pragma unroll
    for (int t = 0; t < TXE_HEDGE_MAX_THRESHOLDS; ++t) {
        best[t].d = -1;                 // (a depth is >= 1: the first qualifying column always wins)
        best[t].c = -1;
        best[t].m = 0.0;
    }
}

// the four waves' keys through LDS, merged by wave 0 in wave order, to the workgroup's slot of the partial keys [slot][nt][ldk]
__device__ __forceinline__ void hedge_write_slot(HedgeKey* best, int nt, int wv, int lane, long long q, int nq, int slot, long long ldk,
                                                 int* __restrict__ kd, int* __restrict__ kc, double* __restrict__ km) {
    __shared__ int s_d[HEDGE_WAVES][TXE_HEDGE_MAX_THRESHOLDS][HEDGE_TILE];
    __shared__ int s_c[HEDGE_WAVES][TXE_HEDGE_MAX_THRESHOLDS][HEDGE_TILE];
    __shared__ double s_m[HEDGE_WAVES][TXE_HEDGE_MAX_THRESHOLDS][HEDGE_TILE];
    if (wv > 0) {
#pragma unroll
        for (int t = 0; t < TXE_HEDGE_MAX_THRESHOLDS; ++t) {
            s_d[wv][t][lane] = best[t].d;
            s_c[wv][t][lane] = best[t].c;
            s_m[wv][t][lane] = best[t].m;
        }
    }
    __syncthreads();
    if (wv == 0 && q < nq) {
#pragma unroll
        for (int t = 0; t < TXE_HEDGE_MAX_THRESHOLDS; ++t) {
            if (t < nt) {
                HedgeKey b = best[t];
                for (int w = 1; w < HEDGE_WAVES; ++w) {
                    const int d = s_d[w][t][lane], c = s_c[w][t][lane];
                    const double m = s_m[w][t][lane];
                    if (c >= 0 && hedge_better(d, m, c, b)) { b.d = d; b.c = c; b.m = m; }
                }
                const size_t at = ((size_t)slot * nt + t) * (size_t)ldk + (size_t)q;
                kd[at] = b.d;
                kc[at] = b.c;
                km[at] = b.m;
            }
        }
    }
}

__global__ __launch_bounds__(256) void hedge_probs_kernel(const float* __restrict__ S, long long ldS, int nq, int G,
                                                          const double* __restrict__ lse, float beta, int negate,
                                                          float* __restrict__ PT, long long ldq) {
    __shared__ float tile[HEDGE_TILE * HEDGE_TP_PITCH];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const long long g0 = (long long)blockIdx.x * HEDGE_TILE, q0 = (long long)blockIdx.y * HEDGE_TILE;
    const long long g = g0 + tx;
    for (int r = ty; r < HEDGE_TILE; r += HEDGE_WAVES) {
        const long long q = q0 + r;
        float p = 0.f;
        if (q < nq && g < G) {
            const double l = lse[q];
            if (fabs(l) < (double)INFINITY) {                       // (false for a NaN too: the row is zeros)
                const float s = S[(size_t)q * (size_t)ldS + (size_t)g];
                const float t = beta * (negate ? -s : s);           // one fp32 product, rounded on its own
                p = (float)exp((double)t - l);
            }
        }
        tile[r * HEDGE_TP_PITCH + tx] = p;
    }
    __syncthreads();
    const long long q = q0 + tx;
    for (int c = ty; c < HEDGE_TILE; c += HEDGE_WAVES) {
        const long long gg = g0 + c;
        if (gg < G && q < ldq) PT[(size_t)gg * (size_t)ldq + (size_t)q] = tile[tx * HEDGE_TP_PITCH + c];
    }
}

template <bool HEDGE>
__global__ __launch_bounds__(256) void hedge_sweep_kernel(const int* __restrict__ sub_ptr, const int* __restrict__ sub_idx,
                                                          const int* __restrict__ depth, int G, int nnz,
                                                          const int* __restrict__ item_row, const int* __restrict__ item_slice,
                                                          const int* __restrict__ item_part, int n_items, int n_part,
                                                          const float* __restrict__ PT, long long ldq, int nq, HedgeTaus taus, int nt,
                                                          double* __restrict__ mass, long long ldm, double* __restrict__ part,
                                                          long long ldk, int* __restrict__ kd, int* __restrict__ kc,
                                                          double* __restrict__ km) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long q = (long long)blockIdx.y * HEDGE_TILE + lane;
    const bool live = q < nq;
    const float* __restrict__ col = PT + (live ? q : 0);
    const int n_waves = gridDim.x * HEDGE_WAVES;
    HedgeKey best[TXE_HEDGE_MAX_THRESHOLDS];
    if (HEDGE) hedge_init(best);
    for (int it = blockIdx.x * HEDGE_WAVES + wv; it < n_items; it += n_waves) {
        const int a = item_row[it], s = item_slice[it], pt = item_part[it];
        if ((unsigned)a >= (unsigned)G || s < 0) continue;                   // (wave-uniform)
        const int lo = min(max(sub_ptr[a], 0), nnz), hi = min(max(sub_ptr[a + 1], lo), nnz);
        const long long b = (long long)lo + (long long)s * TXE_HEDGE_SLICE;
        const int e0 = (int)(b < hi ? b : hi), e1 = (int)(b + TXE_HEDGE_SLICE < hi ? b + TXE_HEDGE_SLICE : hi);
        double acc = 0.0;
        int i = e0;
        for (; i + HEDGE_UNROLL <= e1; i += HEDGE_UNROLL) {
            float v[HEDGE_UNROLL];
#pragma unroll
            for (int u = 0; u < HEDGE_UNROLL; ++u) {
                const int dcol = sub_idx[i + u];
                v[u] = (live && (unsigned)dcol < (unsigned)G) ? col[(size_t)dcol * (size_t)ldq] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < HEDGE_UNROLL; ++u) acc += (double)v[u];
        }
        for (; i < e1; ++i) {
            const int dcol = sub_idx[i];
            acc += (double)((live && (unsigned)dcol < (unsigned)G) ? col[(size_t)dcol * (size_t)ldq] : 0.f);
        }
        if (pt >= 0) {
            if (pt < n_part && live) part[(size_t)pt * (size_t)ldk + (size_t)q] = acc;
        } else if (!HEDGE) {
            if (live) mass[(size_t)a * (size_t)ldm + (size_t)q] = acc;
        } else {
            hedge_offer(best, taus, nt, depth[a], acc, a);
        }
    }
    if (HEDGE) hedge_write_slot(best, nt, wv, lane, q, nq, blockIdx.x, ldk, kd, kc, km);
}

// the long rows: their slices' partial sums added in slice order
template <bool HEDGE>
__global__ __launch_bounds__(256) void hedge_long_kernel(const int* __restrict__ long_row, const int* __restrict__ long_ptr, int n_long,
                                                         int n_part, const int* __restrict__ depth, int G,
                                                         const double* __restrict__ part, long long ldk, int nq, HedgeTaus taus, int nt,
                                                         double* __restrict__ mass, long long ldm, int slot_base, int* __restrict__ kd,
                                                         int* __restrict__ kc, double* __restrict__ km) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long q = (long long)blockIdx.y * HEDGE_TILE + lane;
    const bool live = q < nq;
    const int n_waves = gridDim.x * HEDGE_WAVES;
    HedgeKey best[TXE_HEDGE_MAX_THRESHOLDS];
    if (HEDGE) hedge_init(best);
    for (int k = blockIdx.x * HEDGE_WAVES + wv; k < n_long; k += n_waves) {
        const int a = long_row[k];
        if ((unsigned)a >= (unsigned)G) continue;
        const int p0 = min(max(long_ptr[k], 0), n_part), p1 = min(max(long_ptr[k + 1], p0), n_part);
        double tot = 0.0;
        if (live && p1 > p0) {
            tot = part[(size_t)p0 * (size_t)ldk + (size_t)q];
            for (int j = p0 + 1; j < p1; ++j) tot += part[(size_t)j * (size_t)ldk + (size_t)q];
        }
        if (!HEDGE) {
            if (live) mass[(size_t)a * (size_t)ldm + (size_t)q] = tot;
        } else {
            hedge_offer(best, taus, nt, depth[a], tot, a);
        }
    }
    if (HEDGE) hedge_write_slot(best, nt, wv, lane, q, nq, slot_base + blockIdx.x, ldk, kd, kc, km);
}

// per query and threshold: the partial keys merged in slot order; the three outputs [nq][nt]
__global__ __launch_bounds__(256) void hedge_finish_kernel(const int* __restrict__ kd, const int* __restrict__ kc,
                                                           const double* __restrict__ km, int n_slots, long long ldk, int nq, int nt,
                                                           int* __restrict__ out_col, double* __restrict__ out_mass,
                                                           int* __restrict__ out_depth) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    for (int t = 0; t < nt; ++t) {
        HedgeKey b;
        b.d = -1; b.c = -1; b.m = 0.0;
        for (int s = 0; s < n_slots; ++s) {
            const size_t at = ((size_t)s * nt + t) * (size_t)ldk + (size_t)q;
            const int d = kd[at], c = kc[at];
            const double m = km[at];
            if (c >= 0 && hedge_better(d, m, c, b)) { b.d = d; b.c = c; b.m = m; }
        }
        const size_t o = (size_t)q * nt + t;
        out_col[o] = b.c;
        out_mass[o] = b.c >= 0 ? b.m : (double)NAN;
        out_depth[o] = b.c >= 0 ? b.d : 0;
    }
}

static inline int hedge_sweep_wgs(int n_items) {
    const long long per = (long long)HEDGE_WAVES * HEDGE_ITEMS_PER_WAVE;
    const long long w = ((long long)n_items + per - 1) / per;
    return (int)(w < 1 ? 1 : (w > HEDGE_MAX_SWEEP_WG ? HEDGE_MAX_SWEEP_WG : w));
}
static inline int hedge_long_wgs(int n_long) {
    if (n_long <= 0) return 0;
    const int w = (n_long + HEDGE_WAVES - 1) / HEDGE_WAVES;
    return w > HEDGE_MAX_LONG_WG ? HEDGE_MAX_LONG_WG : w;
}
static inline long long hedge_ldk(int nq) { return ((long long)nq + HEDGE_TILE - 1) / HEDGE_TILE * HEDGE_TILE; }
static inline size_t hedge_part_bytes(int n_part, int nq) { return ((size_t)n_part * (size_t)hedge_ldk(nq) * sizeof(double) + 255) / 256 * 256; }

}  // namespace txe

using namespace txe;

extern "C" {

int txe_hedge_probs(const float* S, long long ldS, int nq, int G, const double* lse, float beta, int negate, float* PT, long long ldq,
                    void* stream) {
    if (nq < 0 || G < 0 || !(beta > 0.f) || !(beta < INFINITY)) return TXE_ERR_ARG;
    if (nq == 0 || G == 0) return TXE_OK;
    if (!S || !lse || !PT || ldS < G || ldq < nq) return TXE_ERR_ARG;
    const long long gt = ((long long)G + HEDGE_TILE - 1) / HEDGE_TILE, qt = (ldq + HEDGE_TILE - 1) / HEDGE_TILE;
    if (gt > 0x7fffffffLL || qt > 65535) return TXE_ERR_ARG;
    ProfScope prof("hedge_probs", (hipStream_t)stream, 8.0 * (double)nq * (double)G, 1);
    hipLaunchKernelGGL(hedge_probs_kernel, dim3((unsigned)gt, (unsigned)qt), dim3(256), 0, (hipStream_t)stream, S, ldS, nq, G, lse, beta,
                       negate, PT, ldq);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

size_t txe_hedge_sweep_ws_bytes(int n_items, int n_long, int n_part, int nq, int n_thr) {
    if (n_items < 0 || n_long < 0 || n_part < 0 || nq < 0 || n_thr < 0 || n_thr > TXE_HEDGE_MAX_THRESHOLDS) return 0;
    size_t b = hedge_part_bytes(n_part, nq);
    if (n_thr > 0) {
        const size_t slots = (size_t)hedge_sweep_wgs(n_items) + (size_t)hedge_long_wgs(n_long);
        b += slots * (size_t)n_thr * (size_t)hedge_ldk(nq) * (2 * sizeof(int) + sizeof(double));
    }
    return b + 256;
}

int txe_hedge_sweep(const int* sub_ptr, const int* sub_idx, const int* depth, int G, int nnz, const int* item_row, const int* item_slice,
                    const int* item_part, int n_items, const int* long_row, const int* long_ptr, int n_long, int n_part, const float* PT,
                    long long ldq, int nq, const double* thresholds, int n_thr, double* mass, long long ldm, int* out_col,
                    double* out_mass, int* out_depth, void* ws, size_t ws_bytes, void* stream) {
    if (nq < 0 || G < 0 || nnz < 0 || n_items < 0 || n_long < 0 || n_part < 0 || n_thr < 0 || n_thr > TXE_HEDGE_MAX_THRESHOLDS)
        return TXE_ERR_ARG;
    HedgeTaus taus;
    for (int t = 0; t < TXE_HEDGE_MAX_THRESHOLDS; ++t) taus.tau[t] = 2.0;
    if (n_thr > 0) {
        if (!thresholds) return TXE_ERR_ARG;
        for (int t = 0; t < n_thr; ++t) {
            if (!(thresholds[t] > 0.0) || !(thresholds[t] <= 1.0)) return TXE_ERR_ARG;     // (a NaN fails both)
            taus.tau[t] = thresholds[t];
        }
    }
    if (nq == 0 || G == 0) return TXE_OK;
    if (!sub_ptr || !sub_idx || !depth || !item_row || !item_slice || !item_part || !long_row || !long_ptr || !PT) return TXE_ERR_ARG;
    if (ldq < nq) return TXE_ERR_ARG;
    if (n_thr == 0 && (!mass || ldm < nq)) return TXE_ERR_ARG;
    if (n_thr > 0 && (!out_col || !out_mass || !out_depth)) return TXE_ERR_ARG;
    const long long tiles = hedge_ldk(nq) / HEDGE_TILE;
    if (tiles > 65535) return TXE_ERR_ARG;
    if (!ws || ws_bytes < txe_hedge_sweep_ws_bytes(n_items, n_long, n_part, nq, n_thr)) return TXE_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long long ldk = hedge_ldk(nq);
    char* w = (char*)(((uintptr_t)ws + 255) / 256 * 256);
    double* part = (double*)w;
    w += hedge_part_bytes(n_part, nq);
    const int wg_sweep = hedge_sweep_wgs(n_items), wg_long = hedge_long_wgs(n_long);
    const size_t key_elems = (size_t)(wg_sweep + wg_long) * (size_t)n_thr * (size_t)ldk;
    double* km = (double*)w;
    int* kd = (int*)(w + key_elems * sizeof(double));
    int* kc = kd + key_elems;
    ProfScope prof(n_thr ? "hedge_sweep" : "hedge_mass", s, 4.0 * (double)nnz * (double)nq, 1);
    const dim3 grid((unsigned)wg_sweep, (unsigned)tiles), grid_long((unsigned)(wg_long ? wg_long : 1), (unsigned)tiles);
    if (n_thr == 0) {
        hipLaunchKernelGGL(hedge_sweep_kernel<false>, grid, dim3(256), 0, s, sub_ptr, sub_idx, depth, G, nnz, item_row, item_slice,
                           item_part, n_items, n_part, PT, ldq, nq, taus, 0, mass, ldm, part, ldk, kd, kc, km);
        TXE_CHECK_LAUNCH();
        if (wg_long) {
            hipLaunchKernelGGL(hedge_long_kernel<false>, grid_long, dim3(256), 0, s, long_row, long_ptr, n_long, n_part, depth, G,
                               (const double*)part, ldk, nq, taus, 0, mass, ldm, 0, kd, kc, km);
            TXE_CHECK_LAUNCH();
        }
        return TXE_OK;
    }
    hipLaunchKernelGGL(hedge_sweep_kernel<true>, grid, dim3(256), 0, s, sub_ptr, sub_idx, depth, G, nnz, item_row, item_slice, item_part,
                       n_items, n_part, PT, ldq, nq, taus, n_thr, (double*)nullptr, 0LL, part, ldk, kd, kc, km);
    TXE_CHECK_LAUNCH();
    if (wg_long) {
        hipLaunchKernelGGL(hedge_long_kernel<true>, grid_long, dim3(256), 0, s, long_row, long_ptr, n_long, n_part, depth, G,
                           (const double*)part, ldk, nq, taus, n_thr, (double*)nullptr, 0LL, wg_sweep, kd, kc, km);
        TXE_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(hedge_finish_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, (const int*)kd, (const int*)kc,
                       (const double*)km, wg_sweep + wg_long, ldk, nq, n_thr, out_col, out_mass, out_depth);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

}  // extern "C"
