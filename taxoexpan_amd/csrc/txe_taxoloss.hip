// Taxonomy-aware InfoNCE: the training-side counterpart of txe_taxometric.hip's Wu & Palmer similarity.  A batch has Q
// groups of C = 1 + k columns; x[i][c] is the model's output for group i, column c, a[i][c] the taxonomy node the column's egonet is
// anchored at, column 0 the positive, p_i = a[i][0].  With depth, anc and lca_depth as in txe_taxometric.hip (an index of n nodes):
//     d[i][0] = 0
//     d[i][c] = 0                                          if a[i][c] or p_i lies outside [0, n)   (compared BEFORE it addresses anything)
//     d[i][c] = 1.0 - 2.0 * lca_depth(a[i][c], p_i) / (depth[a[i][c]] + depth[p_i])     float64; in [0, 1]; 0 iff a[i][c] == p_i; 1 in a forest
//     m[i][c] = (float)((double)gamma * d[i][c])           one rounding to fp32
//     y[i][c] = x[i][c] + m[i][c]                          one fp32 add
//     row_i   = logsumexp_c y[i][c] - x[i][0]
//     loss    = sum_i row_i                                (row losses merged in a fixed order, in float64, then one rounding)
//     d_x[i][c] = softmax_c(y[i])[c] - [c == 0]            (d is a constant of the batch: no gradient flows into it)
// A negative far from the true parent must be beaten by more.  Margins are integers until one quotient: 2 l is an exact product, the
// quotient is one correctly rounded fp64 division, then one subtraction, one product with gamma and one cast -- no expression here has
// a product feeding a sum, so fp contraction has nothing to fuse and the numpy restatement (loss.host_taxo_margins) gives the same bits.
//
// Lane mapping = txe_info_nce's: a row occupies GW lanes (32 when C <= 32, else 64; longer rows loop), a wave holds 64 / GW rows, a
// workgroup TL_WAVES waves, the grid ceil(Q / rows per workgroup) workgroups.  EVERY LANE OWNS ONE COLUMN (per loop pass) and
// intersects its own negative's closure row with the positive's, so the group's C intersections run side by side and need no
// cross-lane step; the row arithmetic afterwards is nce_row (txe_nce_row.h), the function txe_info_nce calls: at gamma = 0, y = x + 0
// and d_x has txe_info_nce's bytes.
// Dependent global round trips per group (all lanes of the group take them together):
//     1  a[i][0] (every lane of the group reads it: one broadcast), the lane's own a[i][c] and x[i][c]
//     2  anc_ptr[p], anc_ptr[p + 1], depth[p]  |  anc_ptr[a], anc_ptr[a + 1], depth[a]
//     3  the positive's row anc(p), GW entries per lane pass  |  the first TL_CHUNK entries of anc(a), issued together
//     4  depth[] of the positive's entries -> LDS, once per group: every common ancestor is in that row, so a hit costs no gather
// then the searches run in LDS.  A negative's list beyond TL_CHUNK entries (mean 4.8, longest 24 on the masked synthetic MAG-CS) adds one
// trip per further entry.  A positive whose row exceeds TXE_TAXO_STAGE_CAP entries is not staged: its group binary-searches the row in
// global memory and gathers depth[v] per hit (txe_taxometric.hip's taxo_lower_bound route), ~log2(row) + 1 trips per entry.
// Then one launch that adds the row losses in row order in float64.  No floating-point atomics; dist_total is an integer atomic.
#include "txe_common.h"
#include "txe_nce_row.h"
#include "../../include/txe.h"

namespace txe {

constexpr int TL_WAVES = 4, TL_THREADS = TL_WAVES * 64;
constexpr int TL_CAP = TXE_TAXO_STAGE_CAP;
constexpr int TL_CHUNK = 8;                            // entries of a negative's closure row loaded before the first is searched
constexpr int TL_FIN_THREADS = 256;

// first position of the sorted row r[0..n) whose value is >= v (LDS or global)
__device__ __forceinline__ int tl_lower_bound(const int* r, int n, int v) {
    int lo = 0;
    while (n > 0) {
        const int half = n >> 1;
        if (r[lo + half] < v) { lo += half + 1; n -= half + 1; } else { n = half; }
    }
    return lo;
}

// a column's node: the bounds of its closure row, its depth and the row's first entries.  a outside [0, n): an empty row.
struct TlNode {
    int ab, na, da;
    int v[TL_CHUNK];
};
__device__ __forceinline__ TlNode tl_load_node(int a, int n_nodes, const int* __restrict__ anc_ptr, const int* __restrict__ anc_idx,
                                               const int* __restrict__ depth) {
    TlNode nd;
    nd.ab = 0; nd.na = 0; nd.da = 0;
    if (a >= 0 && a < n_nodes) { nd.ab = anc_ptr[a]; nd.na = anc_ptr[a + 1] - nd.ab; nd.da = depth[a]; }
#pragma unroll
    for (int u = 0; u < TL_CHUNK; ++u) nd.v[u] = u < nd.na ? anc_idx[nd.ab + u] : -1;
    return nd;
}

template <int GW>
__global__ __launch_bounds__(TL_THREADS) void info_nce_taxo_kernel(const float* __restrict__ x, long long ld_x, int Q, int Cc,
                                                                   const int* __restrict__ anchors, long long ld_a,
                                                                   const int* __restrict__ anc_ptr, const int* __restrict__ anc_idx,
                                                                   const int* __restrict__ depth, int n_nodes, double gamma, float* d_x,
                                                                   long long ld_dx, float* __restrict__ margin,
                                                                   unsigned long long* dist_total, float* __restrict__ row_loss) {
    constexpr int RPW = 64 / GW, RPB = TL_WAVES * RPW;     // rows per wave, rows per workgroup
    __shared__ int s_id[RPB][TL_CAP], s_dp[RPB][TL_CAP];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int sub = l / GW, gl = l % GW, slot = w * RPW + sub;
    const long long b = (long long)blockIdx.x * RPB + slot;
    const bool live = b < Q;                               // (a row that is not live does row 0's reads and writes nothing)
    const long long bb = live ? b : 0;
    const int* __restrict__ arow = anchors + bb * ld_a;
    const float* __restrict__ xrow = x + bb * ld_x;
    float* drow = d_x + bb * ld_dx;

    // trips 1 - 3 of the positive and of the lane's first column, side by side
    const int p = arow[0];
    const bool own = gl < Cc;
    const int a0 = own ? arow[gl] : -1;
    const float x0 = own ? xrow[gl] : 0.f;
    const bool p_ok = p >= 0 && p < n_nodes;
    int pb = 0, np = 0, dp = 0;
    if (p_ok) { pb = anc_ptr[p]; np = anc_ptr[p + 1] - pb; dp = depth[p]; }
    const bool staged = np <= TL_CAP;
    TlNode nd = tl_load_node(a0, n_nodes, anc_ptr, anc_idx, depth);
    if (staged) {
        for (int i = gl; i < np; i += GW) {                // trip 3 and 4 of the positive
            const int v = anc_idx[pb + i];
            s_id[slot][i] = v;
            s_dp[slot][i] = depth[v];
        }
    }
    __syncthreads();
    const int* __restrict__ prow = anc_idx + pb;           // the global route's row

    auto hit_depth = [&](int v) -> int {                   // depth[v] if v is in anc(p), else 0 (depths are >= 1)
        if (staged) {
            const int at = tl_lower_bound(s_id[slot], np, v);
            return (at < np && s_id[slot][at] == v) ? s_dp[slot][at] : 0;
        }
        const int at = tl_lower_bound(prow, np, v);
        return (at < np && prow[at] == v) ? depth[v] : 0;
    };

    float y0 = 0.f;                                        // the lane's first column stays in a register; later ones wait in d_x
    long long dist = 0;
    for (int c = gl; c < Cc; c += GW) {
        float xc = x0;
        if (c != gl) {
            xc = xrow[c];
            nd = tl_load_node(arow[c], n_nodes, anc_ptr, anc_idx, depth);
        }
        double d = 0.0;
        if (c > 0 && p_ok && nd.na > 0) {
            int lca = 0;
#pragma unroll
            for (int u = 0; u < TL_CHUNK; ++u)
                if (u < nd.na) lca = max(lca, hit_depth(nd.v[u]));
            for (int j = TL_CHUNK; j < nd.na; ++j) lca = max(lca, hit_depth(anc_idx[nd.ab + j]));
            d = 1.0 - (2.0 * (double)lca) / (double)(nd.da + dp);
        }
        const float m = (float)(gamma * d);
        const float y = xc + m;
        if (c == gl) y0 = y;
        else if (live) drow[c] = y;
        if (live) {
            if (margin) margin[b * Cc + c] = m;
            dist += (long long)(d * 1048576.0);            // floor: d >= 0, and the product by 2^20 is exact
        }
    }

    const float r = nce_row<GW>([&](int c) { return c == gl ? y0 : (live ? drow[c] : xrow[c]); }, Cc, gl, 0, live, drow);
    // row[0] of the loss is the SCORE x[i][0], not y[i][0]: they are the same number (d[i][0] = 0, m = +0, x + 0 = x)
    if (live && gl == 0) row_loss[b] = r;
    if (dist_total) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dist += __shfl_xor(dist, o, 64);
        if (l == 0 && dist != 0) atomicAdd(dist_total, (unsigned long long)dist);     // (an integer: exact in any order)
    }
}

// the row losses in a fixed order, in float64: thread t adds rows t, t + 256, ..., then a tree over the threads
__global__ __launch_bounds__(TL_FIN_THREADS) void info_nce_taxo_finish_kernel(const float* __restrict__ row_loss, int Q,
                                                                              float* __restrict__ loss) {
    __shared__ double s_l[TL_FIN_THREADS];
    double a = 0.0;
    for (int i = threadIdx.x; i < Q; i += TL_FIN_THREADS) a += (double)row_loss[i];
    s_l[threadIdx.x] = a;
    __syncthreads();
    for (int o = TL_FIN_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_l[threadIdx.x] += s_l[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)s_l[0];
}

}  // namespace txe

using namespace txe;

extern "C" {

// ws: [Q] float row losses
size_t txe_info_nce_taxo_ws_bytes(int Q) { return ((size_t)(Q > 0 ? Q : 1) * 4 + 15) / 16 * 16; }

// the definition at the top of this file; include/txe.h has the contract
int txe_info_nce_taxo(const float* x, long long ld_x, int Q, int C, const int* anchors, long long ld_a, const int* anc_ptr,
                      const int* anc_idx, const int* depth, int n_nodes, double gamma, float* loss, float* d_x, long long ld_dx,
                      float* margin, long long* dist_total, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !anchors || !anc_ptr || !anc_idx || !depth || !loss || !d_x) return TXE_ERR_ARG;
    if (Q < 0 || C < 1 || ld_x < C || ld_dx < C || ld_a < C || (long long)Q * C >= (1ll << 31) || n_nodes < 0) return TXE_ERR_ARG;
    if (!(gamma >= 0.0) || !(gamma <= 1.7976931348623157e308)) return TXE_ERR_ARG;       // NaN, negative, Inf
    if (!ws || ws_bytes < txe_info_nce_taxo_ws_bytes(Q)) return TXE_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (Q == 0) return hipMemsetAsync(loss, 0, sizeof(float), s) == hipSuccess ? TXE_OK : TXE_ERR_LAUNCH;
    float* row_loss = (float*)ws;
    {
        ProfScope prof("info_nce_taxo_kernel", s, 16.0 * Q * (double)C, 1);
        if (C <= 32) {
            const int rpb = TL_WAVES * 2;
            hipLaunchKernelGGL(info_nce_taxo_kernel<32>, dim3((Q + rpb - 1) / rpb), dim3(TL_THREADS), 0, s, x, ld_x, Q, C, anchors, ld_a, anc_ptr,
                               anc_idx, depth, n_nodes, gamma, d_x, ld_dx, margin, (unsigned long long*)dist_total, row_loss);
        } else {
            const int rpb = TL_WAVES;
            hipLaunchKernelGGL(info_nce_taxo_kernel<64>, dim3((Q + rpb - 1) / rpb), dim3(TL_THREADS), 0, s, x, ld_x, Q, C, anchors, ld_a, anc_ptr,
                               anc_idx, depth, n_nodes, gamma, d_x, ld_dx, margin, (unsigned long long*)dist_total, row_loss);
        }
        TXE_CHECK_LAUNCH();
    }
    {
        ProfScope prof("info_nce_taxo_finish_kernel", s, 4.0 * Q + 4.0, 1);
        hipLaunchKernelGGL(info_nce_taxo_finish_kernel, dim3(1), dim3(TL_FIN_THREADS), 0, s, row_loss, Q, loss);
        TXE_CHECK_LAUNCH();
    }
    return TXE_OK;
}

}  // extern "C"
