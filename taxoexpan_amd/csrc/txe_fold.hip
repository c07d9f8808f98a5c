// =====================================================================================================================
// Last GATLayer folded behind a linear readout (PGAT / GAT output layer with ONE head + MeanReadout / WeightedMeanReadout;
// model_zoo.py:80-104,219,227-242).  The output layer has no activation, its head mean is the identity, and the readout is
// a weighted mean, so   hg[g] = sum_v w_v/S_g * sum_u alpha'_uv * (Xd[u] W^T)  =  ( sum_{u in g} c_u Xd[u] ) W^T,
//     c_u = sum_{v : u->v} w_v alpha'_uv / S_g,   Xd = feat-dropped layer input,  alpha' = attention-dropped softmax,
// and the attention logits need only two columns:  a1 = Xd wa1, a2 = Xd wa2 (the folded rows F, F+1 of Wp).
// Same arithmetic, different association: the projection (and its dX / dW products) shrink from N node rows to G graph
// rows (4.4x fewer flops on the MAG batch); everything else is two HBM sweeps over X in forward and two in backward.
//   forward : logits (sweep 1) -> alpha [E] -> c~ [N] -> Z[g] = sum c~_u Xd[u] / S_g (sweep 2) -> hg = Z W^T (GEMM, G rows)
//   backward: dZ = d_hg W, dW = d_hg^T Z (GEMMs, G rows) -> dc~_u = <dZ[g], Xd[u]>/S_g, dS_g (sweep 3) -> edge-level softmax /
//             readout-weight backward -> d_X[u] = keep*s*(c_u dZ[g] + da1_u wa1 + da2_u wa2) * leaky'(X), d_wa (sweep 4) -> unfold.
// The backward's sweep 4 fused with the layer below is txe_fold_bwd.hip; the folded GCN output layer, which reuses these sweeps, ends
// this file.
// =====================================================================================================================
#include <string.h>

#include "txe_gemm.h"
#include "txe_gather.h"
#include "txe_colsum.h"
#include "txe_gemm_split.h"
#include "txe_tail.h"
#include "txe_fold.h"

namespace txe {

constexpr int CL_NI = 4;                      // 16-byte vectors per lane per column tile (256 vectors = 1024 columns per tile)

__device__ __forceinline__ float cl_softplus(float x) { return x > 20.f ? x : log1pf(__expf(x)); }
__device__ __forceinline__ float cl_sigmoid(float x) { return x > 20.f ? 1.f : 1.f / (1.f + __expf(-x)); }

// keep factors (0 / 1) of the 4 columns of vector j from the row's mask words (mask == nullptr: all kept)
template <bool MASK>
__device__ __forceinline__ void cl_keep4(const unsigned* __restrict__ mrow, int mask_ld, int j, float* k4) {
    if constexpr (!MASK) { k4[0] = k4[1] = k4[2] = k4[3] = 1.f; return; }
    // vector j < Kp / 4 and the mask row has Kp / 32 = mask_ld words: the word always exists.  (A bounds select here makes hipcc sink
    // the load into the conditional and wait vmcnt(0) behind it -- one load in flight per wave.)
    const int c = j * 4;
    const unsigned b = mrow[c >> 5] >> (c & 31);
    k4[0] = (b & 1u) ? 1.f : 0.f; k4[1] = (b & 2u) ? 1.f : 0.f; k4[2] = (b & 4u) ? 1.f : 0.f; k4[3] = (b & 8u) ? 1.f : 0.f;
}

// sweep 1 -- one wave per node (persistent waves keep the two folded rows in registers per column tile):
//   a12[u][0] = <Xd[u], wa1>,  a12[u][1] = <Xd[u], wa2>
template <bool MASK>
__global__ __launch_bounds__(256) void cl_logits_kernel(const float* __restrict__ X, int Kp, int n_nodes, const unsigned* __restrict__ mask,
                                                        int mask_ld, float scale, const float* __restrict__ wa /*[2][Kp]*/,
                                                        float* __restrict__ a12) {
    const int l = threadIdx.x & 63;
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
    const int nvec = Kp >> 2;
    for (int u = wave; u < n_nodes; u += nwaves) {
        const float* row = X + (long long)u * Kp;
        const unsigned* mrow = mask + (MASK ? (long long)u * mask_ld : 0);
        float s1 = 0.f, s2 = 0.f;
        for (int t0 = 0; t0 < nvec; t0 += 64 * CL_NI) {
            float x[CL_NI][4], w1[CL_NI][4], w2[CL_NI][4], k4[CL_NI][4];
#pragma unroll
            for (int i = 0; i < CL_NI; ++i) {
                const int j = t0 + l + 64 * i;
                const int jc = (j < nvec) ? j : t0;
                vload<4>(row + jc * 4, x[i]);
                vload<4>(wa + jc * 4, w1[i]);
                vload<4>(wa + Kp + jc * 4, w2[i]);
                cl_keep4<MASK>(mrow, mask_ld, jc, k4[i]);
                const float live = (j < nvec) ? 1.f : 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) k4[i][k] *= live;
            }
#pragma unroll
            for (int i = 0; i < CL_NI; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float xd = x[i][k] * k4[i][k];
                    s1 = fmaf(xd, w1[i][k], s1);
                    s2 = fmaf(xd, w2[i][k], s2);
                }
        }
        s1 = wave_sum(s1) * scale;
        s2 = wave_sum(s2) * scale;
        if (l == 0) { a12[2 * (long long)u] = s1; a12[2 * (long long)u + 1] = s2; }
    }
}

// per graph: S_g = sum_v w_v -> wsum[g];  gid[v] = g for its nodes
__device__ __forceinline__ void cl_wsum_job(const int bid, const int* __restrict__ goff, int G, const int* __restrict__ pos,
                                            const float* __restrict__ pw, float* __restrict__ wsum, int* __restrict__ gid) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int g = bid * 4 + w;
    if (g >= G) return;
    const int beg = goff[g], end = goff[g + 1];
    float S = 0.f;
    for (int v = beg + l; v < end; v += 64) {
        S += pw ? cl_softplus(pw[pos[v]]) : 1.f;
        gid[v] = g;
    }
    S = wave_sum(S);
    if (l == 0) wsum[g] = S;
}
__global__ __launch_bounds__(256) void cl_wsum_kernel(const int* __restrict__ goff, int G, const int* __restrict__ pos,
                                                      const float* __restrict__ pw, float* __restrict__ wsum, int* __restrict__ gid) {
    cl_wsum_job(blockIdx.x, goff, G, pos, pw, wsum, gid);
}
// sweep 2 -- one wave per (graph, 256-column tile):  Z[g][tile] = (scale / S_g) sum_{u in g} c~_u (X[u] * keep)[tile]
template <bool MASK>
__global__ __launch_bounds__(256) void cl_zsum_kernel(const int* __restrict__ goff, int G, int ntile, const float* __restrict__ X, int Kp,
                                                      const unsigned* __restrict__ mask, int mask_ld, float scale,
                                                      const float* __restrict__ coef, const float* __restrict__ wsum,
                                                      float* __restrict__ Z) {
    const int l = threadIdx.x & 63;
    const long long wid = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int g = (int)(wid / ntile), t = (int)(wid % ntile);
    if (g >= G) return;
    const int beg = goff[g], end = goff[g + 1];
    const int nvec = Kp >> 2;
    const int j = t * 64 + l;
    const int jc = (j < nvec) ? j : t * 64;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int u0 = beg; u0 < end; u0 += 4) {                          // four nodes per step: independent loads in flight
        float x[4][4], k4[4][4], cu[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int u = min(u0 + e, end - 1);
            cu[e] = coef[u] * ((u0 + e < end) ? 1.f : 0.f);
            vload<4>(X + (long long)u * Kp + jc * 4, x[e]);
            cl_keep4<MASK>(mask + (MASK ? (long long)u * mask_ld : 0), mask_ld, jc, k4[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = fmaf(cu[e] * k4[e][k], x[e][k], acc[k]);
    }
    if (j < nvec) {
        const float S = wsum[g];
        const float zs = S > 0.f ? scale / S : 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] *= zs;
        vstore<4>(Z + (long long)g * Kp + j * 4, acc);
    }
}

// The same sweep with one wave per (chunk of ZS_GPW consecutive graphs, column tile): an egonet has ~4 nodes, so a (graph, tile) wave
// asks for 4 KB and is gone -- 36,864 waves of two dependent round trips each on the training batch.  A chunk's nodes are one
// contiguous range: the wave streams it eight nodes (8 KB) per step and writes a graph's row of Z whenever the range crosses into
// the next graph (offsets and weight sums of the chunk sit in lanes, read back as scalars: uniform control flow).  Per graph the same
// nodes in the same order: bit-identical to cl_zsum_kernel.
#ifndef TXE_ZS_GPW
#define TXE_ZS_GPW 4
#endif
constexpr int ZS_GPW = TXE_ZS_GPW;
// EDOT (the graph vector folded into a bilinear matcher): the gradient of Z will be dZ[g] = dsl_g Tf[zrow[g]] with Tf known NOW, so
// the backward's <dZ[g], keep X[u]> sweep is this sweep's <Tf[zrow[g]], keep X[u]> times a scalar: the wave adds its tile's share of that
// dot product per node to e_part[u][tile] (summed over the tiles, in tile order, by cl_fold_dc_kernel).
template <bool MASK, bool EDOT = false>
__global__ __launch_bounds__(256) void cl_zsum_chunk_kernel(const int* __restrict__ goff, int G, int ntile, int nmap, const float* __restrict__ X, int Kp,
                                                            const unsigned* __restrict__ mask, int mask_ld, float scale,
                                                            const float* __restrict__ coef, const float* __restrict__ wsum,
                                                            float* __restrict__ Z, const float* __restrict__ Tf = nullptr,
                                                            const int* __restrict__ zrow = nullptr, float* __restrict__ e_part = nullptr) {
    constexpr int NU = 8;
    const int l = threadIdx.x & 63;
    const long long wid = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
    // waves are numbered over (chunk, nmap slots): nmap = ntile, or ntile + 1 with an idle slot when ntile is a multiple of 4 -- the four
    // waves of a workgroup (and the two workgroups of an 8-tile row) would otherwise always sit on the SAME chunk's rows, which costs a
    // quarter of the sweep's rate (8 tiles: 67 against 51 us; 4: 35 / 25; 16: 118 / 90 -- with or without the e_part stores)
    const int ch = (int)(wid / nmap), t = (int)(wid % nmap);
    const int g0 = ch * ZS_GPW;
    if (g0 >= G || t >= ntile) return;
    const int ng = min(ZS_GPW, G - g0);
    const int my_off = goff[g0 + min(l, ng)];                       // lanes 0..ng: the chunk's graph offsets
    const float my_ws = wsum[g0 + min(l, ng - 1)];                  // lanes 0..ng-1: their weight sums
    const int nvec = Kp >> 2;
    const int j = t * 64 + l;
    const int jc = (j < nvec) ? j : t * 64;
    const int beg = __builtin_amdgcn_readlane(my_off, 0), end = __builtin_amdgcn_readlane(my_off, ng);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int gi = 0;                                                     // current graph of the chunk (uniform)
    int next = __builtin_amdgcn_readlane(my_off, 1);               // first node past it
    float tt[4] = {0.f, 0.f, 0.f, 0.f};                             // EDOT: this lane's piece of Tf[zrow[current graph]]
    int my_zr = 0;
    if constexpr (EDOT) {
        my_zr = zrow[g0 + min(l, ng - 1)];                          // lanes 0..ng-1: the chunk's rows of Tf
        vload<4>(Tf + (long long)__builtin_amdgcn_readlane(my_zr, 0) * Kp + jc * 4, tt);
    }
    auto flush = [&]() {                                            // graph gi is complete: scale, store, start the next one
        const float S = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_ws), gi));
        const float zs = S > 0.f ? scale / S : 0.f;
        if (j < nvec) {
            float o[4] = {acc[0] * zs, acc[1] * zs, acc[2] * zs, acc[3] * zs};
            vstore<4>(Z + (long long)(g0 + gi) * Kp + j * 4, o);
        }
        acc[0] = acc[1] = acc[2] = acc[3] = 0.f;
        ++gi;
        next = __builtin_amdgcn_readlane(my_off, min(gi + 1, ng));
        if constexpr (EDOT) vload<4>(Tf + (long long)__builtin_amdgcn_readlane(my_zr, min(gi, ng - 1)) * Kp + jc * 4, tt);
    };
    for (int u0 = beg; u0 < end; u0 += NU) {                        // NU nodes per step: independent loads in flight
        float x[NU][4], k4[NU][4], cu[NU];
#pragma unroll
        for (int e = 0; e < NU; ++e) {
            const int u = min(u0 + e, end - 1);
            cu[e] = coef[u];
            vload<4>(X + (long long)u * Kp + jc * 4, x[e]);
            cl_keep4<MASK>(mask + (MASK ? (long long)u * mask_ld : 0), mask_ld, jc, k4[e]);
        }
        float pe[NU];                                               // EDOT: this lane's share of the NU nodes' dot products with Tf
#pragma unroll
        for (int e = 0; e < NU; ++e) pe[e] = 0.f;
#pragma unroll
        for (int e = 0; e < NU; ++e) {
            const int u = u0 + e;
            if (u < end) {                                          // (uniform)
                while (u >= next) flush();                          // graphs that ended before u (empty ones included)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = fmaf(cu[e] * k4[e][k], x[e][k], acc[k]);
                if constexpr (EDOT) {
                    float q = 0.f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) q = fmaf(tt[k] * k4[e][k], x[e][k], q);
                    pe[e] = (j < nvec) ? q : 0.f;
                }
            }
        }
        if constexpr (EDOT) {
            // eight sums over the wave in 10 exchanges instead of 8 x 6: halve the set of values a lane carries with every exchange
            // (lane bit 5 picks nodes 0-3 / 4-7, bit 4 pairs, bit 3 one), then three plain butterflies; lane 8 n holds node n's sum
            static_assert(NU == 8, "the reduction below is written for eight nodes per step");
            // (all on the VALU: v_permlane32_swap / v_permlane16_swap hand the half a lane does not keep to its partner 32 / 16 lanes away,
            //  DPP row rotations and quad permutes do the rest -- __shfl_xor is ds_bpermute, a trip through the LDS pipeline per exchange;
            //  same pairs added in the same order)
            float a4[4], b2[2];
            const bool h5 = (l & 32) != 0, h4 = (l & 16) != 0, h3 = (l & 8) != 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(pe[k]), __float_as_uint(pe[k + 4]), false, false);
                a4[k] = h5 ? __uint_as_float(r[1]) + __uint_as_float(r[0]) : __uint_as_float(r[0]) + __uint_as_float(r[1]);
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a4[k]), __float_as_uint(a4[k + 2]), false, false);
                b2[k] = h4 ? __uint_as_float(r[1]) + __uint_as_float(r[0]) : __uint_as_float(r[0]) + __uint_as_float(r[1]);
            }
            float c1 = (h3 ? b2[1] : b2[0]) + dpp_f<0x128>(h3 ? b2[0] : b2[1]);          // row_ror:8 = lane ^ 8
            {   // lane ^ 4: row_shl:4 for the lanes with bit 2 clear (banks 0, 2), row_shr:4 for the others
                int o = __builtin_amdgcn_update_dpp(0, __float_as_int(c1), 0x104, 0xF, 0x5, false);
                o = __builtin_amdgcn_update_dpp(o, __float_as_int(c1), 0x114, 0xF, 0xA, false);
                c1 += __int_as_float(o);
            }
            c1 += dpp_f<0x4E>(c1);                                                       // quad_perm [2,3,0,1] = lane ^ 2
            c1 += dpp_f<0xB1>(c1);                                                       // quad_perm [1,0,3,2] = lane ^ 1
            const int en = (h5 ? 4 : 0) + (h4 ? 2 : 0) + (h3 ? 1 : 0);
            if ((l & 7) == 0 && u0 + en < end) e_part[(long long)(u0 + en) * ntile + t] = c1;
        }
    }
    while (gi < ng) flush();                                        // the last graph, and empty graphs at the chunk's end
}

// launch of the Z sweep: small graphs (egonets: ~4 nodes) on the chunked kernel, large ones one wave per graph and tile
static bool cl_zsum_chunked(int n_nodes, int G) { return (long long)n_nodes <= 16LL * G && G >= 16; }
static int cl_zsum_launch(const int* graph_off, int G, int n_nodes, const float* X, int Kp, const unsigned* mk, const unsigned* dummy_mask,
                          int mask_ld, float fs, const float* coef, const float* wsum, float* Z, hipStream_t s, const float* Tf = nullptr,
                          const int* zrow = nullptr, float* e_part = nullptr) {
    const int ntile = (Kp / 4 + 63) / 64;
    const int nmap = (ntile % 4 == 0) ? ntile + 1 : ntile;          // (slots per chunk in the chunked kernel's wave numbering: see there)
    const bool chunked = cl_zsum_chunked(n_nodes, G);
    if (e_part) {                                   // (only the chunked kernel forms the dot products: the entry point checks cl_zsum_chunked)
        if (!chunked || !Tf || !zrow) return TXE_ERR_ARG;
        const long long nw = (long long)((G + ZS_GPW - 1) / ZS_GPW) * nmap;
        ProfScope prof(mk ? "cl_zsum_chunk_kernel<true, true>" : "cl_zsum_chunk_kernel<false, true>", s, 4.0 * (n_nodes + (double)G) * Kp, 1);
        const dim3 grid((unsigned)((nw + 3) / 4));
        if (mk) hipLaunchKernelGGL((cl_zsum_chunk_kernel<true, true>), grid, dim3(256), 0, s, graph_off, G, ntile, nmap, X, Kp, mk, mask_ld, fs, coef, wsum, Z, Tf, zrow, e_part);
        else hipLaunchKernelGGL((cl_zsum_chunk_kernel<false, true>), grid, dim3(256), 0, s, graph_off, G, ntile, nmap, X, Kp, dummy_mask, mask_ld, fs, coef, wsum, Z, Tf,
                                zrow, e_part);
        TXE_CHECK_LAUNCH();
        return TXE_OK;
    }
    const long long nwaves = chunked ? (long long)((G + ZS_GPW - 1) / ZS_GPW) * nmap : (long long)G * ntile;
    ProfScope prof(chunked ? (mk ? "cl_zsum_chunk_kernel<true, false>" : "cl_zsum_chunk_kernel<false, false>") : (mk ? "cl_zsum_kernel<true>" : "cl_zsum_kernel<false>"), s,
                   4.0 * (n_nodes + (double)G) * Kp, 1);
    const dim3 grid((unsigned)((nwaves + 3) / 4));
    if (chunked && mk) hipLaunchKernelGGL((cl_zsum_chunk_kernel<true, false>), grid, dim3(256), 0, s, graph_off, G, ntile, nmap, X, Kp, mk, mask_ld, fs, coef, wsum, Z,
                                          (const float*)nullptr, (const int*)nullptr, (float*)nullptr);
    else if (chunked) hipLaunchKernelGGL((cl_zsum_chunk_kernel<false, false>), grid, dim3(256), 0, s, graph_off, G, ntile, nmap, X, Kp, dummy_mask, mask_ld, fs, coef, wsum,
                                         Z, (const float*)nullptr, (const int*)nullptr, (float*)nullptr);
    else if (mk) hipLaunchKernelGGL(cl_zsum_kernel<true>, grid, dim3(256), 0, s, graph_off, G, ntile, X, Kp, mk, mask_ld, fs, coef, wsum, Z);
    else hipLaunchKernelGGL(cl_zsum_kernel<false>, grid, dim3(256), 0, s, graph_off, G, ntile, X, Kp, dummy_mask, mask_ld, fs, coef, wsum, Z);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

// per graph: dS[g] = -<dZ[g], Z[g]> / S_g
__global__ __launch_bounds__(256) void cl_bwd_ds_kernel(int G, int Kp, const float* __restrict__ dZ, const float* __restrict__ Z,
                                                        const float* __restrict__ wsum, float* __restrict__ dS) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + w;
    if (g >= G) return;
    const int nvec = Kp >> 2;
    float s = 0.f;
    for (int j = l; j < nvec; j += 64) {
        float d[4], z[4];
        vload<4>(dZ + (long long)g * Kp + j * 4, d);
        vload<4>(Z + (long long)g * Kp + j * 4, z);
#pragma unroll
        for (int k = 0; k < 4; ++k) s = fmaf(d[k], z[k], s);
    }
    s = wave_sum(s);
    if (l == 0) dS[g] = wsum[g] > 0.f ? -s / wsum[g] : 0.f;
}

// sweep 3 -- one wave per node:  dc~_u = (scale / S_g) <dZ[g], X[u] * keep>
template <bool MASK>
__global__ __launch_bounds__(256) void cl_bwd_dot_kernel(int n_nodes, const int* __restrict__ gid, const float* __restrict__ X, int Kp,
                                                         const unsigned* __restrict__ mask, int mask_ld, float scale,
                                                         const float* __restrict__ dZ, const float* __restrict__ wsum,
                                                         const float* __restrict__ coef, float* __restrict__ dc, float* __restrict__ cn,
                                                         const int nb_ds, const int G, const int D, const float* __restrict__ d_hg,
                                                         const long long ld_dhg, const float* __restrict__ hg, const long long ld_hg,
                                                         float* __restrict__ dS) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    if ((int)blockIdx.x < nb_ds) {
        // independent job on the first workgroups, one wave per graph: dS[g] = -<dZ[g], Z[g]> / S_g, and since dZ = d_hg W and
        // hg = Z W^T the product is <d_hg[g], hg[g]> -- D columns instead of Kp, and no dependence on the dZ GEMM
        const int g = blockIdx.x * 4 + w;
        if (g >= G) return;
        float s = 0.f;
        for (int j = l; j < D; j += 64) s = fmaf(d_hg[(long long)g * ld_dhg + j], hg[(long long)g * ld_hg + j], s);
        s = wave_sum(s);
        if (l == 0) dS[g] = wsum[g] > 0.f ? -s / wsum[g] : 0.f;
        return;
    }
    const int u = ((int)blockIdx.x - nb_ds) * 4 + w;
    if (u >= n_nodes) return;
    const int g = gid[u];
    const int nvec = Kp >> 2;
    const float* row = X + (long long)u * Kp;
    const float* dzrow = dZ + (long long)g * Kp;
    const unsigned* mrow = mask + (MASK ? (long long)u * mask_ld : 0);
    float part = 0.f;
    for (int t0 = 0; t0 < nvec; t0 += 64 * CL_NI) {
        float x[CL_NI][4], d[CL_NI][4], k4[CL_NI][4];
#pragma unroll
        for (int i = 0; i < CL_NI; ++i) {
            const int j = t0 + l + 64 * i;
            const int jc = (j < nvec) ? j : t0;
            vload<4>(row + jc * 4, x[i]);
            vload<4>(dzrow + jc * 4, d[i]);
            cl_keep4<MASK>(mrow, mask_ld, jc, k4[i]);
            const float live = (j < nvec) ? 1.f : 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) k4[i][k] *= live;
        }
#pragma unroll
        for (int i = 0; i < CL_NI; ++i)
#pragma unroll
            for (int k = 0; k < 4; ++k) part = fmaf(d[i][k] * k4[i][k], x[i][k], part);
    }
    part = wave_sum(part);
    if (l == 0) {
        const float S = wsum[g];
        const float inv = S > 0.f ? 1.f / S : 0.f;
        dc[u] = part * scale * inv;
        cn[u] = coef[u] * inv;                        // normalised coefficient for the d_X sweep
    }
}

// The same sweep with the node's WHOLE row in one round trip: NT tiles of 64 vectors per lane issued together (the tile loop above is
// three dependent round trips for a 2,080-column row, behind the gid one).  Lanes past the row re-read its first tile (L1 hits) with a
// zero factor; per lane the vectors are summed in the same ascending order: bit-identical.
template <bool MASK, int NT>
__global__ __launch_bounds__(256) void cl_bwd_dot_row_kernel(int n_nodes, const int* __restrict__ gid, const float* __restrict__ X, int Kp,
                                                             const unsigned* __restrict__ mask, int mask_ld, float scale,
                                                             const float* __restrict__ dZ, const float* __restrict__ wsum,
                                                             const float* __restrict__ coef, float* __restrict__ dc, float* __restrict__ cn,
                                                             const int nb_ds, const int G, const int D, const float* __restrict__ d_hg,
                                                             const long long ld_dhg, const float* __restrict__ hg, const long long ld_hg,
                                                             float* __restrict__ dS) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    if ((int)blockIdx.x < nb_ds) {                      // (the dS job of cl_bwd_dot_kernel)
        const int g = blockIdx.x * 4 + w;
        if (g >= G) return;
        float s = 0.f;
        for (int j = l; j < D; j += 64) s = fmaf(d_hg[(long long)g * ld_dhg + j], hg[(long long)g * ld_hg + j], s);
        s = wave_sum(s);
        if (l == 0) dS[g] = wsum[g] > 0.f ? -s / wsum[g] : 0.f;
        return;
    }
    const int u = ((int)blockIdx.x - nb_ds) * 4 + w;
    if (u >= n_nodes) return;
    const int g = gid[u];
    const float S = wsum[g];
    const float cu = coef[u];
    const int nvec = Kp >> 2;                           // (> 64: the launcher sends narrower rows to cl_bwd_dot_kernel)
    const float* row = X + (long long)u * Kp;
    const float* dzrow = dZ + (long long)g * Kp;
    const unsigned* mrow = mask + (MASK ? (long long)u * mask_ld : 0);
    float x[NT][4], d[NT][4], k4[NT][4];
    // (the node's own row first and the gid-dependent dZ row behind it, in two loops: 61 against 55 us)
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int j = l + 64 * i;
        const int jc = (j < nvec) ? j : l;
        vload<4>(row + jc * 4, x[i]);
        vload<4>(dzrow + jc * 4, d[i]);
        cl_keep4<MASK>(mrow, mask_ld, jc, k4[i]);
        const float live = (j < nvec) ? 1.f : 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) k4[i][k] *= live;
    }
    float part = 0.f;
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) part = fmaf(d[i][k] * k4[i][k], x[i][k], part);
    part = wave_sum(part);
    if (l == 0) {
        const float inv = S > 0.f ? 1.f / S : 0.f;
        dc[u] = part * scale * inv;
        cn[u] = cu * inv;
    }
}

// launch of sweep 3: rows of 65..640 vectors go out in one round trip of 5, 9 or 10 tiles (cl_bwd_dot_row_kernel), anything else tile by tile
int cl_bwd_dot_launch(int n_nodes, const int* gid, const float* X, int Kp, const unsigned* mk, const unsigned* dummy_mask, int mask_ld, float fs,
                             const float* dZ, const float* wsum, const float* coef, float* dc, float* cn, int nb_ds, int G, int D, const float* d_hg,
                             long long ld_dhg, const float* hg, long long ld_hg, float* dS, double bytes, hipStream_t s) {
    const int nb = (n_nodes + 3) / 4, nvec = Kp >> 2;
    const int nt = (nvec > 64 && nvec <= 320) ? 5 : ((nvec > 320 && nvec <= 576) ? 9 : ((nvec > 576 && nvec <= 640) ? 10 : 0));
    const unsigned* m = mk ? mk : dummy_mask;
    const dim3 grid(nb_ds + nb);
#define TXE_BD_ARGS n_nodes, gid, X, Kp, m, mask_ld, fs, dZ, wsum, coef, dc, cn, nb_ds, G, D, d_hg, ld_dhg, hg, ld_hg, dS
    if (nt == 0) {
        ProfScope prof(mk ? "cl_bwd_dot_kernel<true>" : "cl_bwd_dot_kernel<false>", s, bytes, 1);
        if (mk) hipLaunchKernelGGL(cl_bwd_dot_kernel<true>, grid, dim3(256), 0, s, TXE_BD_ARGS);
        else hipLaunchKernelGGL(cl_bwd_dot_kernel<false>, grid, dim3(256), 0, s, TXE_BD_ARGS);
    } else {
        static const char* names[6] = {"cl_bwd_dot_row_kernel<false, 5>", "cl_bwd_dot_row_kernel<true, 5>", "cl_bwd_dot_row_kernel<false, 9>",
                                       "cl_bwd_dot_row_kernel<true, 9>", "cl_bwd_dot_row_kernel<false, 10>", "cl_bwd_dot_row_kernel<true, 10>"};
        ProfScope prof(names[(mk ? 1 : 0) + (nt == 9 ? 2 : (nt == 10 ? 4 : 0))], s, bytes, 1);
        if (nt == 5 && mk) hipLaunchKernelGGL((cl_bwd_dot_row_kernel<true, 5>), grid, dim3(256), 0, s, TXE_BD_ARGS);
        else if (nt == 5) hipLaunchKernelGGL((cl_bwd_dot_row_kernel<false, 5>), grid, dim3(256), 0, s, TXE_BD_ARGS);
        else if (nt == 9 && mk) hipLaunchKernelGGL((cl_bwd_dot_row_kernel<true, 9>), grid, dim3(256), 0, s, TXE_BD_ARGS);
        else if (nt == 9) hipLaunchKernelGGL((cl_bwd_dot_row_kernel<false, 9>), grid, dim3(256), 0, s, TXE_BD_ARGS);
        else if (mk) hipLaunchKernelGGL((cl_bwd_dot_row_kernel<true, 10>), grid, dim3(256), 0, s, TXE_BD_ARGS);
        else hipLaunchKernelGGL((cl_bwd_dot_row_kernel<false, 10>), grid, dim3(256), 0, s, TXE_BD_ARGS);
    }
#undef TXE_BD_ARGS
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The folded layer's edge-level work as ONE launch each way.  Everything here is tiny (a few bytes per edge) and stays inside a graph,
// so a workgroup that owns CG_GRAPHS whole graphs can run the destination-side and the source-side halves back to back behind a
// workgroup barrier (they were two ~10 us launches each).  Degrees up to CG_LIGHT are walked by one thread per node with every load
// unrolled and clamped (no branch between a load and its use); heavier nodes (an egonet's anchor feeds up to 50 siblings; hubs of
// generic graphs) are collected and handled by a whole wave each.
//   forward : alpha[p] = softmax_in(leaky(a1[u] + a2[v])), gid, w_v;  S_g = sum w_v;  c~_u = sum_out w_v f alpha
//   backward: dz[p], da2[v], dwv[v] (destination side, cl_bwd_edge_kernel's math);  da1[u] = sum_out dz (source side)
// ---------------------------------------------------------------------------------------------------------------------
constexpr int CG_GRAPHS = 8;
constexpr int CG_LIGHT = 8;
constexpr int CG_MAXN = 512;        // nodes of a workgroup whose readout weights are staged in LDS (beyond: recomputed)

__device__ __forceinline__ int cg_graph_of(const int* s_goff, int ng, int v) {
    int g = 0;
#pragma unroll
    for (int q = 1; q < CG_GRAPHS; ++q) g += (q < ng && v >= s_goff[q]) ? 1 : 0;
    return g;
}

__global__ __launch_bounds__(256) void cl_attn_coef_kernel(const int* __restrict__ rowptr_in, const int* __restrict__ col_src,
                                                           const int* __restrict__ rowptr_out, const int* __restrict__ col_dst,
                                                           const int* __restrict__ pos_out, const int* __restrict__ goff, const int G,
                                                           const float* __restrict__ a12, const float slope, const float drop_p,
                                                           const float drop_scale, const unsigned long long seed,
                                                           const int* __restrict__ pos, const float* __restrict__ pw,
                                                           float* __restrict__ alpha, float* __restrict__ coef, float* __restrict__ wsum,
                                                           int* __restrict__ gid) {
    __shared__ int s_goff[CG_GRAPHS + 1], s_heavy[2][256], s_nh[2];
    __shared__ float s_wv[CG_MAXN];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int g0 = blockIdx.x * CG_GRAPHS, g1 = min(G, g0 + CG_GRAPHS), ng = g1 - g0;
    if (threadIdx.x <= ng) s_goff[threadIdx.x] = goff[g0 + threadIdx.x];
    if (threadIdx.x < 2) s_nh[threadIdx.x] = 0;
    __syncthreads();
    const int n0 = s_goff[0], nn = s_goff[ng] - n0;
    // ---- destination side: alpha, graph ids, readout weights ----
    for (int t = threadIdx.x; t < nn; t += 256) {
        const int v = n0 + t;
        gid[v] = g0 + cg_graph_of(s_goff, ng, v);
        if (t < CG_MAXN) s_wv[t] = pw ? cl_softplus(pw[pos[v]]) : 1.f;
        const int beg = rowptr_in[v], end = rowptr_in[v + 1];
        if (end - beg > CG_LIGHT) { const int k = atomicAdd(&s_nh[0], 1); if (k < 256) s_heavy[0][k] = v; continue; }
        const float a2v = a12[2 * (long long)v + 1];
        float z[CG_LIGHT];
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < CG_LIGHT; ++i) {
            const int p = min(beg + i, max(end - 1, beg));
            const float zz = leaky(a12[2 * (long long)col_src[p]] + a2v, slope);
            z[i] = (beg + i < end) ? zz : -INFINITY;
            m = fmaxf(m, z[i]);
        }
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < CG_LIGHT; ++i) { z[i] = (beg + i < end) ? __expf(z[i] - m) : 0.f; sum += z[i]; }
        const float inv = 1.f / sum;
#pragma unroll
        for (int i = 0; i < CG_LIGHT; ++i)
            if (beg + i < end) alpha[beg + i] = z[i] * inv;
    }
    __syncthreads();
    {
        const bool listed = s_nh[0] <= 256;
        for (int i = w; i < (listed ? s_nh[0] : nn); i += 4) {
            const int v = listed ? s_heavy[0][i] : n0 + i;
            const int beg = rowptr_in[v], end = rowptr_in[v + 1];
            if (end - beg <= CG_LIGHT) continue;
            const float a2v = a12[2 * (long long)v + 1];
            float m = -INFINITY;
            for (int p = beg + l; p < end; p += 64) m = fmaxf(m, leaky(a12[2 * (long long)col_src[p]] + a2v, slope));
            m = wave_max(m);
            float sum = 0.f;
            for (int p = beg + l; p < end; p += 64) sum += __expf(leaky(a12[2 * (long long)col_src[p]] + a2v, slope) - m);
            sum = wave_sum(sum);
            const float inv = 1.f / sum;
            for (int p = beg + l; p < end; p += 64) alpha[p] = __expf(leaky(a12[2 * (long long)col_src[p]] + a2v, slope) - m) * inv;
        }
    }
    if (threadIdx.x < ng) {                            // S_g: a serial walk in fixed order (deterministic)
        float S = 0.f;
        for (int v = s_goff[threadIdx.x]; v < s_goff[threadIdx.x + 1]; ++v)
            S += (v - n0 < CG_MAXN) ? s_wv[v - n0] : (pw ? cl_softplus(pw[pos[v]]) : 1.f);
        wsum[g0 + threadIdx.x] = S;
    }
    __syncthreads();                                   // alpha of these graphs' edges is complete (first touched below)
    // ---- source side: coefficients ----
    for (int t = threadIdx.x; t < nn; t += 256) {
        const int u = n0 + t;
        const int beg = rowptr_out[u], end = rowptr_out[u + 1];
        if (end - beg > CG_LIGHT) { const int k = atomicAdd(&s_nh[1], 1); if (k < 256) s_heavy[1][k] = u; continue; }
        float cu = 0.f;
#pragma unroll
        for (int i = 0; i < CG_LIGHT; ++i) {
            const int j = min(beg + i, max(end - 1, beg));
            const int p = pos_out[j], v = col_dst[j];
            const int tv = min(max(v - n0, 0), CG_MAXN - 1);
            const float wv = (v - n0 < CG_MAXN && v >= n0) ? s_wv[tv] : (pw ? cl_softplus(pw[pos[v]]) : 1.f);
            const float f = (drop_p > 0.f) ? drop_factor(seed, (unsigned long long)p, drop_p, drop_scale) : 1.f;
            cu += (beg + i < end) ? wv * f * alpha[p] : 0.f;
        }
        coef[u] = cu;
    }
    __syncthreads();
    {
        const bool listed = s_nh[1] <= 256;
        for (int i = w; i < (listed ? s_nh[1] : nn); i += 4) {
            const int u = listed ? s_heavy[1][i] : n0 + i;
            const int beg = rowptr_out[u], end = rowptr_out[u + 1];
            if (end - beg <= CG_LIGHT) continue;
            float cu = 0.f;
            for (int j = beg + l; j < end; j += 64) {
                const int p = pos_out[j], v = col_dst[j];
                const float wv = pw ? cl_softplus(pw[pos[v]]) : 1.f;
                const float f = (drop_p > 0.f) ? drop_factor(seed, (unsigned long long)p, drop_p, drop_scale) : 1.f;
                cu = fmaf(wv * f, alpha[p], cu);
            }
            cu = wave_sum(cu);
            if (l == 0) coef[u] = cu;
        }
    }
}

// The folded matcher's backward in place of the <dZ, X> sweep: dZ[g] = dsl_g Tf[zrow[g]], so
//   dc~_u = dsl_g (scale / S_g) sum_tiles e_part[u][tile],   cn_u = dsl_g c~_u / S_g (the sweep's dZ row is Tf's),   dS_g = -dsl_g raw_g / S_g
// with dsl = ds (* s for the exp matcher) and raw_g = <Z_g, Tf[zrow[g]]> = the score before exp -- per node / per graph scalars of the
// graphs a workgroup of cl_attn_bwd_kernel<true> owns, formed in its prologue (they were a launch of their own, cl_fold_dc_kernel).
// (struct FoldDcArgs: txe_fold.h)

template <bool FOLD>
__global__ __launch_bounds__(256) void cl_attn_bwd_kernel(const int* __restrict__ rowptr_in, const int* __restrict__ col_src,
                                                          const int* __restrict__ rowptr_out, const int* __restrict__ pos_out,
                                                          const int* __restrict__ goff, const int G, const float* __restrict__ a12,
                                                          const float slope, const float* __restrict__ alpha, const float drop_p,
                                                          const float drop_scale, const unsigned long long seed,
                                                          const int* __restrict__ pos, const float* __restrict__ pw,
                                                          const float* __restrict__ dc, const float* __restrict__ dS,
                                                          float* __restrict__ dz, float* __restrict__ da1, float* __restrict__ da2,
                                                          float* __restrict__ dwv, const FoldDcArgs fd_) {
    __shared__ int s_goff[CG_GRAPHS + 1], s_heavy[2][256], s_nh[2];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int g0 = blockIdx.x * CG_GRAPHS, g1 = min(G, g0 + CG_GRAPHS), ng = g1 - g0;
    if (threadIdx.x <= ng) s_goff[threadIdx.x] = goff[g0 + threadIdx.x];
    if (threadIdx.x < 2) s_nh[threadIdx.x] = 0;
    __syncthreads();
    const int n0 = s_goff[0], nn = s_goff[ng] - n0;
    // (FOLD: dc / dS are written by this workgroup's prologue -- read them back through the same, unrestricted pointers)
    const float* dcp = FOLD ? (const float*)fd_.dc : dc;
    const float* dSp = FOLD ? (const float*)fd_.dS : dS;
    if constexpr (FOLD) {
        if ((int)threadIdx.x < ng) {
            const int g = g0 + threadIdx.x;
            const float sv = fd_.m_s[g], dsl = fd_.m_exp ? fd_.m_ds[g] * sv : fd_.m_ds[g];
            const float raw = fd_.m_exp ? logf(sv) : sv;
            const float S = fd_.wsum[g];
            fd_.dS[g] = (S > 0.f && dsl != 0.f) ? -dsl * raw / S : 0.f;
        }
        for (int t = threadIdx.x; t < nn; t += 256) {
            const int u = n0 + t;
            const int g = g0 + cg_graph_of(s_goff, ng, u);
            const float dsl = fd_.m_exp ? fd_.m_ds[g] * fd_.m_s[g] : fd_.m_ds[g];
            const float S = fd_.wsum[g];
            const float inv = S > 0.f ? 1.f / S : 0.f;
            float e = 0.f;
            for (int q = 0; q < fd_.ntile; ++q) e += fd_.e_part[(long long)u * fd_.ntile + q];
            fd_.dc[u] = dsl * e * fd_.scale * inv;
            // the fused sweep reads "dZ[g]" as Tf[zrow[g]] with dsl_g folded into the node's coefficient: dZ itself is never formed
            fd_.cn[u] = fd_.coef[u] * inv * dsl;
            fd_.zgid[u] = fd_.zrow[g];
        }
        __syncthreads();                               // dc / dS of these graphs: read below by other threads of this workgroup
    }
    // ---- destination side ----
    for (int t = threadIdx.x; t < nn; t += 256) {
        const int v = n0 + t;
        const int beg = rowptr_in[v], end = rowptr_in[v + 1];
        if (end - beg > CG_LIGHT) { const int k = atomicAdd(&s_nh[0], 1); if (k < 256) s_heavy[0][k] = v; continue; }
        const float pwv = pw ? pw[pos[v]] : 0.f;
        const float wv = pw ? cl_softplus(pwv) : 1.f;
        const float a2v = a12[2 * (long long)v + 1];
        float al[CG_LIGHT], fd[CG_LIGHT], zs[CG_LIGHT];
        float T = 0.f, dw = 0.f;
#pragma unroll
        for (int i = 0; i < CG_LIGHT; ++i) {
            const int p = min(beg + i, max(end - 1, beg));
            const int u = col_src[p];
            const float f = (drop_p > 0.f) ? drop_factor(seed, (unsigned long long)p, drop_p, drop_scale) : 1.f;
            const bool ok = beg + i < end;
            al[i] = ok ? alpha[p] : 0.f;
            fd[i] = f * dcp[u];                               // f dc~_u
            zs[i] = a12[2 * (long long)u] + a2v;
            dw += al[i] * fd[i];
            T = fmaf(al[i], wv * fd[i], T);
        }
        float s2 = 0.f;
#pragma unroll
        for (int i = 0; i < CG_LIGHT; ++i) {
            const float gz = al[i] * (wv * fd[i] - T) * (zs[i] > 0.f ? 1.f : slope);
            if (beg + i < end) dz[beg + i] = gz;
            s2 += (beg + i < end) ? gz : 0.f;
        }
        da2[v] = s2;
        dwv[v] = pw ? (dSp[g0 + cg_graph_of(s_goff, ng, v)] + dw) * cl_sigmoid(pwv) : 0.f;
    }
    __syncthreads();
    {
        const bool listed = s_nh[0] <= 256;
        for (int i = w; i < (listed ? s_nh[0] : nn); i += 4) {
            const int v = listed ? s_heavy[0][i] : n0 + i;
            const int beg = rowptr_in[v], end = rowptr_in[v + 1];
            if (end - beg <= CG_LIGHT) continue;
            const float pwv = pw ? pw[pos[v]] : 0.f;
            const float wv = pw ? cl_softplus(pwv) : 1.f;
            const float a2v = a12[2 * (long long)v + 1];
            float T = 0.f, dw = 0.f;
            for (int p = beg + l; p < end; p += 64) {
                const float f = (drop_p > 0.f) ? drop_factor(seed, (unsigned long long)p, drop_p, drop_scale) : 1.f;
                const float gq = alpha[p] * f * dcp[col_src[p]];
                dw += gq;
                T = fmaf(alpha[p], wv * f * dcp[col_src[p]], T);
            }
            T = wave_sum(T);
            dw = wave_sum(dw);
            float s2 = 0.f;
            for (int p = beg + l; p < end; p += 64) {
                const float f = (drop_p > 0.f) ? drop_factor(seed, (unsigned long long)p, drop_p, drop_scale) : 1.f;
                const float de = alpha[p] * (wv * f * dcp[col_src[p]] - T);
                const float zq = a12[2 * (long long)col_src[p]] + a2v;
                const float gz = de * (zq > 0.f ? 1.f : slope);
                dz[p] = gz;
                s2 += gz;
            }
            s2 = wave_sum(s2);
            if (l == 0) {
                da2[v] = s2;
                dwv[v] = pw ? (dSp[g0 + cg_graph_of(s_goff, ng, v)] + dw) * cl_sigmoid(pwv) : 0.f;
            }
        }
    }
    __syncthreads();                                   // dz of these graphs' edges is complete (first touched below)
    // ---- source side ----
    for (int t = threadIdx.x; t < nn; t += 256) {
        const int u = n0 + t;
        const int beg = rowptr_out[u], end = rowptr_out[u + 1];
        if (end - beg > CG_LIGHT) { const int k = atomicAdd(&s_nh[1], 1); if (k < 256) s_heavy[1][k] = u; continue; }
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < CG_LIGHT; ++i) {
            const int j = min(beg + i, max(end - 1, beg));
            a += (beg + i < end) ? dz[pos_out[j]] : 0.f;
        }
        da1[u] = a;
    }
    __syncthreads();
    {
        const bool listed = s_nh[1] <= 256;
        for (int i = w; i < (listed ? s_nh[1] : nn); i += 4) {
            const int u = listed ? s_heavy[1][i] : n0 + i;
            const int beg = rowptr_out[u], end = rowptr_out[u + 1];
            if (end - beg <= CG_LIGHT) continue;
            float a = 0.f;
            for (int j = beg + l; j < end; j += 64) a += dz[pos_out[j]];
            a = wave_sum(a);
            if (l == 0) da1[u] = a;
        }
    }
}
void cl_attn_bwd_launch(bool fold, const int* rowptr_in, const int* col_src, const int* rowptr_out, const int* pos_out, const int* goff, int G,
                        const float* a12, float slope, const float* alpha, float drop_p, float drop_scale, unsigned long long seed, const int* pos,
                        const float* pw, const float* dc, const float* dS, float* dz, float* da1, float* da2, float* dwv, const FoldDcArgs& fd,
                        hipStream_t s) {
    const dim3 grid((G + CG_GRAPHS - 1) / CG_GRAPHS);
    if (fold) hipLaunchKernelGGL(cl_attn_bwd_kernel<true>, grid, dim3(256), 0, s, rowptr_in, col_src, rowptr_out, pos_out, goff, G, a12, slope, alpha, drop_p,
                                 drop_scale, seed, pos, pw, dc, dS, dz, da1, da2, dwv, fd);
    else hipLaunchKernelGGL(cl_attn_bwd_kernel<false>, grid, dim3(256), 0, s, rowptr_in, col_src, rowptr_out, pos_out, goff, G, a12, slope, alpha, drop_p,
                            drop_scale, seed, pos, pw, dc, dS, dz, da1, da2, dwv, fd);
}

// sweep 4 -- one wave per (chunk of CL_CHUNK nodes, 256-column tile):
//   d_X[u][j] = keep * scale * (c~_u / S_g * dZ[g][j] + da1[u] wa1[j] + da2[u] wa2[j]) * (act_on && j < Kh ? leaky'(X[u][j]) : 1)
//   dwa_part[chunk][0/1][j] = sum over the chunk's nodes of da1/da2[u] * scale * keep * X[u][j]     (fixed order: deterministic)
constexpr int CL_CHUNK = 32;
template <bool MASK, bool ATT>
__global__ __launch_bounds__(256) void cl_bwd_dx_kernel(int n_nodes, int ntile, const int* __restrict__ gid, const float* __restrict__ X, int Kp,
                                                        int Kh, const unsigned* __restrict__ mask, int mask_ld, float scale,
                                                        const float* __restrict__ dZ, const float* __restrict__ cn,
                                                        const float* __restrict__ da1, const float* __restrict__ da2,
                                                        const float* __restrict__ wa, int act_on, float act_slope,
                                                        float* __restrict__ d_X, float* __restrict__ dwa_part) {
    const int l = threadIdx.x & 63;
    const long long wid = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int chunk = (int)(wid / ntile), t = (int)(wid % ntile);
    const int u_beg = chunk * CL_CHUNK;
    if (u_beg >= n_nodes) return;
    const int u_end = min(n_nodes, u_beg + CL_CHUNK);
    const int nvec = Kp >> 2;
    const int j = t * 64 + l;
    const bool jok = j < nvec;
    const int jc = jok ? j : t * 64;
    // leaky' applies to the first Kh columns (the previous layer's activated output); slope 1 elsewhere / when off
    float sl[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) sl[k] = (act_on && (jc * 4 + k) < Kh) ? act_slope : 1.f;
    float w1[4] = {0.f, 0.f, 0.f, 0.f}, w2[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (ATT) {
        vload<4>(wa + jc * 4, w1);
        vload<4>(wa + Kp + jc * 4, w2);
    }
    constexpr int NU = 8;                            // nodes per step: all their loads are unconditional and issued together
    for (int u0 = u_beg; u0 < u_end; u0 += NU) {
        float x[NU][4], d[NU][4], k4[NU][4], cu[NU], g1[NU], g2[NU];
#pragma unroll
        for (int e = 0; e < NU; ++e) {
            const int u = min(u0 + e, u_end - 1);
            const float ok = (u0 + e < u_end) ? 1.f : 0.f;
            const int g = gid[u];
            cu[e] = cn[u] * ok;
            g1[e] = ATT ? da1[u] * ok : 0.f;
            g2[e] = ATT ? da2[u] * ok : 0.f;
            vload<4>(X + (long long)u * Kp + jc * 4, x[e]);
            vload<4>(dZ + (long long)g * Kp + jc * 4, d[e]);
            cl_keep4<MASK>(mask + (MASK ? (long long)u * mask_ld : 0), mask_ld, jc, k4[e]);
        }
#pragma unroll
        for (int e = 0; e < NU; ++e) {
            float o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float ks = k4[e][k] * scale;
                o[k] = ks * (cu[e] * d[e][k] + g1[e] * w1[k] + g2[e] * w2[k]) * ((x[e][k] > 0.f) ? 1.f : sl[k]);
                const float xd = x[e][k] * ks;
                s1[k] = fmaf(g1[e], xd, s1[k]);
                s2[k] = fmaf(g2[e], xd, s2[k]);
            }
            if (jok && u0 + e < u_end) vstore<4>(d_X + (long long)(u0 + e) * Kp + j * 4, o);
        }
    }
    if (ATT && jok) {
        vstore<4>(dwa_part + ((long long)chunk * 2 + 0) * Kp + j * 4, s1);
        vstore<4>(dwa_part + ((long long)chunk * 2 + 1) * Kp + j * 4, s2);
    }
}

// ... and the folded matcher's FORWARD score from the same dot products: <Z_g, Tf[zrow[g]]> = (scale / S_g) sum_{u in g} c~_u e_u -- a sum
// over the graph's few nodes instead of a sweep over Z.
__global__ __launch_bounds__(256) void cl_fold_score_kernel(const int* __restrict__ goff, int G, const float* __restrict__ coef,
                                                            const float* __restrict__ wsum, const float* __restrict__ e_part, int ntile, float scale,
                                                            int apply_exp, float* __restrict__ sc) {
    // one wave per graph: its nodes' tiles are ONE contiguous range of e_part, a lane takes every 64th value (fixed order: deterministic)
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (g >= G) return;
    const int u0 = goff[g], n = (goff[g + 1] - u0) * ntile;
    const float* base = e_part + (long long)u0 * ntile;
    float acc = 0.f;
    for (int i = l; i < n; i += 64) acc = fmaf(coef[u0 + i / ntile], base[i], acc);
    acc = wave_sum(acc);
    if (l == 0) {
        const float S = wsum[g];
        const float raw = S > 0.f ? acc * scale / S : 0.f;
        sc[g] = apply_exp ? __expf(raw) : raw;
    }
}

CollapseWs plan_collapse_ws(void* ws, int n, int e, int G, int Kp, int D, int Pd, int vocab, int max_splits) {
    CollapseWs p;
    char* b = (char*)ws;
    size_t off = 0;
    auto take = [&](size_t bytes) { float* r = (float*)(b + off); off += align_up(bytes > 0 ? bytes : 4, 256); return r; };
    const int n1 = n > 0 ? n : 1, v1 = vocab > 0 ? vocab : 1;
    p.dZ = take((size_t)(G > 0 ? G : 1) * Kp * 4);
    p.splits = choose_splits(D, Kp, G);
    if (max_splits > 0 && p.splits > max_splits) p.splits = max_splits;
    p.part = take((size_t)p.splits * D * Kp * 4);
    p.chunks = (n + CL_CHUNK - 1) / CL_CHUNK;
    p.dwa_part = take((size_t)(p.chunks > 0 ? p.chunks : 1) * 2 * Kp * 4);
    p.dwa = take((size_t)2 * Kp * 4);
    p.dc = take((size_t)n1 * 4);
    p.cn = take((size_t)n1 * 4);
    p.dS = take((size_t)(G > 0 ? G : 1) * 4);
    p.dz = take((size_t)(e > 0 ? e : 1) * 4);
    p.da1 = take((size_t)n1 * 4);
    p.da2 = take((size_t)n1 * 4);
    p.dwv = take((size_t)n1 * 4);
    p.seg_rows = 64;
    p.seg_blocks = (n + p.seg_rows - 1) / p.seg_rows;
    if (p.seg_blocks < 1) p.seg_blocks = 1;
    p.ppart = take((size_t)p.seg_blocks * v1 * (Pd > 0 ? Pd : 1) * 4);
    p.ppart2 = take((size_t)p.seg_blocks * v1 * 4);
    p.tail_bytes = gemm_tail_ws_bytes();
    p.tail = take(p.tail_bytes);
    p.total = off;
    return p;
}

}  // namespace txe
using namespace txe;
extern "C" {

// extra workspace (behind txe_gat_collapse_ws_bytes) with which txe_gat_collapse_fwd forms hg = Z W^T on the bf16 pipe
static inline size_t collapse_split_bytes(int G, int D, int Kt) {
    const int Kc = round_up(Kt, 16);
    return align_up(split_packed_bytes(G, Kc), 256) + align_up(split_packed_bytes(D, Kc), 256);
}
size_t txe_gat_collapse_split_ws_bytes(int G, int Kh, int Pd, int D) {
    return (G < 1 || Kh < 1 || Pd < 0 || D < 1) ? 0 : collapse_split_bytes(G, D, Kh + Pd);
}
size_t txe_gat_collapse_ws_bytes(int n_nodes, int n_edges, int G, int Kh, int Pd, int D, int vocab) {
    return plan_collapse_ws(nullptr, n_nodes, n_edges, G, round_up(Kh + Pd, 32), D, Pd, vocab).total;
}

// X [N][Kp], Wp [Fp][Kp] (rows < D the weight, rows D / D+1 the folded attention rows), mask: feature-dropout keep bits of X
// or NULL.  pos / pw: WeightedMeanReadout (pw == NULL: MeanReadout).  Saved for backward: a12 [N][2], alpha [E], coef [N],
// wsum [G], gid [N] (graph of each node), Z [G][Kp].  hg [G][D] (row stride ld_hg).
// column tiles per node of txe_gat_collapse_fwd's e_part output; 0 when the batch does not take the chunked Z sweep that forms it
int txe_gat_collapse_e_tiles(int n_nodes, int G, int Kh, int Pd) {
    if (n_nodes <= 0 || G <= 0 || !cl_zsum_chunked(n_nodes, G)) return 0;
    return (round_up(Kh + Pd, 32) / 4 + 63) / 64;
}

// scores of the folded bilinear matcher from txe_gat_collapse_fwd's e_part (the same Tf / zrow): s_g = [exp] <Z_g, Tf[zrow[g]]>
int txe_gat_collapse_fold_scores(const int* graph_off, int n_nodes, int G, int Kh, int Pd, const float* coef, const float* wsum, const float* e_part,
                                 float feat_drop_p, int masked, int apply_exp, float* s, void* stream) {
    if (G < 0 || !graph_off || !coef || !wsum || !e_part || !s || feat_drop_p < 0.f || feat_drop_p >= 1.f) return TXE_ERR_ARG;
    const int nt = txe_gat_collapse_e_tiles(n_nodes, G, Kh, Pd);
    if (nt <= 0) return TXE_ERR_ARG;
    const float fs = (masked && feat_drop_p > 0.f) ? 1.f / (1.f - feat_drop_p) : 1.f;
    ProfScope prof("cl_fold_score_kernel", (hipStream_t)stream, 4.0 * (n_nodes * (nt + 1.0) + 2.0 * G), 1);
    hipLaunchKernelGGL(cl_fold_score_kernel, dim3((G + 3) / 4), dim3(256), 0, (hipStream_t)stream, graph_off, G, coef, wsum, e_part, nt, fs, apply_exp, s);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

int txe_gat_collapse_fwd(const struct txe_graph_batch* batch, const struct txe_gat_fold_layer* layer, const struct txe_fold_match* match,
                         int flags, void* ws, size_t ws_bytes, void* stream) {
    if (!batch || !layer) return TXE_ERR_ARG;
    const int *rowptr_in = batch->rowptr_in, *col_src = batch->col_src, *rowptr_out = batch->rowptr_out, *col_dst = batch->col_dst,
              *pos_out = batch->pos_out, *graph_off = batch->graph_off, *pos = layer->pos;
    const int n_nodes = batch->n_nodes, n_edges = batch->n_edges, G = batch->G, Kh = layer->Kh, Pd = layer->Pd, D = layer->D;
    const float *X = layer->X, *Wp = layer->Wp, *pw = layer->pw, *Tf = match ? match->Tf : nullptr;
    const unsigned* mask = layer->mask;
    const float feat_drop_p = layer->feat_drop_p, attn_slope = layer->attn_slope, attn_drop_p = layer->attn_drop_p;
    const unsigned long long seed = layer->seed;
    float *a12 = layer->a12, *alpha = layer->alpha, *coef = layer->coef, *wsum = layer->wsum, *Z = layer->Z, *hg = layer->hg,
          *e_part = match ? match->e_part : nullptr;
    int* gid = layer->gid;
    const int* zrow = match ? match->zrow : nullptr;
    const long long ld_hg = layer->ld_hg;
    if (n_nodes < 0 || n_edges < 0 || G < 0 || Kh < 1 || Pd < 0 || D < 1 || !rowptr_in || !rowptr_out || !graph_off || !X || !Wp || !a12 ||
        !alpha || !coef || !wsum || !gid || !Z || !ws || (pw && !pos))
        return TXE_ERR_ARG;
    if (feat_drop_p < 0.f || feat_drop_p >= 1.f || attn_drop_p < 0.f || attn_drop_p >= 1.f) return TXE_ERR_ARG;
    // e_part rides in the chunked Z sweep only (txe_gat_collapse_e_tiles == 0 otherwise) and needs Tf and zrow: said before any launch
    if (e_part && (!cl_zsum_chunked(n_nodes, G) || !Tf || !zrow)) return TXE_ERR_ARG;
    const int Kt = Kh + Pd, Kp = round_up(Kt, 32);
    CollapseWs p = plan_collapse_ws(ws, n_nodes, n_edges, G, Kp, D, Pd, 0);
    if (ws_bytes < p.total) return TXE_ERR_WORKSPACE;
    if (G == 0) return TXE_OK;
    // (the bf16 route for hg is the caller's choice, not the buffer's size: a buffer too small for it is an error, before any launch)
    if (hg && (flags & TXE_FOLD_HG_SPLIT) && ws_bytes < p.total + collapse_split_bytes(G, D, Kt)) return TXE_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const unsigned* mk = (mask && feat_drop_p > 0.f) ? mask : nullptr;
    const int mask_ld = (Kt + 31) / 32;
    const float fs = mk ? 1.f / (1.f - feat_drop_p) : 1.f, as = 1.f / (1.f - attn_drop_p);
    const float* wa = Wp + (long long)D * Kp;
    const unsigned* dummy_mask = reinterpret_cast<const unsigned*>(X);     // never dereferenced by the <false> instantiations
    if (n_nodes > 0) {
        const int nb = (n_nodes + 3) / 4;
        if (!(flags & TXE_FOLD_A12_READY)) {    // (the producer of X may already have formed them: txe_gat_aggregate_fwd's fused epilogue)
            ProfScope prof(mk ? "cl_logits_kernel<true>" : "cl_logits_kernel<false>", s, 4.0 * n_nodes * (double)Kp, 1);
            if (mk) hipLaunchKernelGGL(cl_logits_kernel<true>, dim3(nb < 2048 ? nb : 2048), dim3(256), 0, s, X, Kp, n_nodes, mk, mask_ld, fs, wa, a12);
            else hipLaunchKernelGGL(cl_logits_kernel<false>, dim3(nb < 2048 ? nb : 2048), dim3(256), 0, s, X, Kp, n_nodes, dummy_mask, mask_ld, fs, wa, a12);
        }
        hipLaunchKernelGGL(cl_attn_coef_kernel, dim3((G + CG_GRAPHS - 1) / CG_GRAPHS), dim3(256), 0, s, rowptr_in, col_src, rowptr_out, col_dst, pos_out,
                           graph_off, G, (const float*)a12, attn_slope, attn_drop_p, as, seed, pos, pw, alpha, coef, wsum, gid);
        TXE_CHECK_LAUNCH();
    } else if (G > 0) {
        hipLaunchKernelGGL(cl_wsum_kernel, dim3((G + 3) / 4), dim3(256), 0, s, graph_off, G, pos, pw, wsum, gid);
    }
    // e_part != NULL (with hg == NULL: the folded matcher already has Tf [runs][Kp] and zrow [G], graph -> its row of Tf): the sweep also
    // leaves <Tf[zrow[g]], keep X[u]> per node and column tile at e_part [N][txe_gat_collapse_e_tiles] -- backward's <dZ, X> sweep, ahead of time
    const int rc_z = cl_zsum_launch(graph_off, G, n_nodes, X, Kp, mk, dummy_mask, mask_ld, fs, (const float*)coef, (const float*)wsum, Z, s, Tf, zrow,
                                    e_part);
    if (rc_z) return rc_z;
    if (!hg) return TXE_OK;          // (the caller folds hg = Z W^T into what consumes it: txe_bilinear_folded_*)
    if (G > 0 && (flags & TXE_FOLD_HG_SPLIT)) {
        // hg = Z W^T on the bf16 matrix pipe (txe_gemm_split.h): Z and the weight rows packed behind the workspace's own regions
        char* sw = (char*)ws + p.total;
        const int Kc = round_up(Kt, 16);
        const size_t ba = align_up(split_packed_bytes(G, Kc), 256);
        int rc = split_pack_launch(Z, Kp, G, Kc, 0, sw, s);
        if (rc) return rc;
        rc = split_pack_launch(Wp, Kp, D, Kc, 1, sw + ba, s);
        if (rc) return rc;
        return gemm_nt_split_launch(sw, sw + ba, G, D, Kc, hg, ld_hg, 2.0 * G * (double)D * Kt, s);
    }
    VMat A = vmat_plain(Z, Kp, G, Kp);
    VMat B = vmat_plain(Wp, Kp, round_up(D + 2, 128), Kp);       // all Fp packed rows are readable: every tile stays on the plain loader
    Epi E = epi_plain(hg, ld_hg, D);
    E.alg_flops = 2.0 * G * (double)D * Kt;
    return gemm_nt(A, B, E, G, D, Kp, 1, s, p.tail, p.tail_bytes);
}

// d_hg [G][D] -> d_X [N][Kp] (first Kh columns through leaky' of X when act_on: they are d(pre-activation) of the previous
// layer), dW [D][Kt], d_attn_l / d_attn_r [D], dP [vocab][Pd] (Pd > 0), d_pw [vocab] (pw != NULL).
int txe_gat_collapse_bwd(const struct txe_graph_batch* batch, const struct txe_gat_fold_layer* layer, const float* d_hg, long long ld_dhg,
                         int act_on, float act_slope, float* d_X, const struct txe_gat_fold_grads* grads, void* ws, size_t ws_bytes, void* stream) {
    if (!batch || !layer || !grads) return TXE_ERR_ARG;
    const int *rowptr_in = batch->rowptr_in, *col_src = batch->col_src, *rowptr_out = batch->rowptr_out, *pos_out = batch->pos_out,
              *graph_off = batch->graph_off, *pos = layer->pos, *gid = layer->gid;
    const int n_nodes = batch->n_nodes, n_edges = batch->n_edges, G = batch->G, Kh = layer->Kh, Pd = layer->Pd, D = layer->D, vocab = layer->vocab;
    const float *X = layer->X, *Wp = layer->Wp, *W = layer->W, *attn_l = layer->attn_l, *attn_r = layer->attn_r, *pw = layer->pw, *a12 = layer->a12,
                *alpha = layer->alpha, *coef = layer->coef, *wsum = layer->wsum, *Z = layer->Z, *hg = layer->hg;
    const unsigned* mask = layer->mask;
    const float feat_drop_p = layer->feat_drop_p, attn_slope = layer->attn_slope, attn_drop_p = layer->attn_drop_p;
    const unsigned long long seed = layer->seed;
    const long long ld_hg = layer->ld_hg;
    float *dW = grads->dW, *d_attn_l = grads->d_attn_l, *d_attn_r = grads->d_attn_r, *dP = grads->dP, *d_pw = grads->d_pw;
    if (n_nodes < 0 || n_edges < 0 || G < 0 || Kh < 1 || Pd < 0 || D < 1 || !rowptr_in || !rowptr_out || !graph_off || !X || !Wp || !W ||
        !attn_l || !attn_r || !a12 || !alpha || !coef || !wsum || !gid || !Z || !hg || !d_hg || !d_X || !dW || !d_attn_l || !d_attn_r || !ws)
        return TXE_ERR_ARG;
    if ((Pd > 0 || pw) && (!pos || vocab < 1 || vocab > MAX_VOCAB)) return TXE_ERR_ARG;
    if ((Pd > 0 && !dP) || (pw && !d_pw)) return TXE_ERR_ARG;
    if (feat_drop_p < 0.f || feat_drop_p >= 1.f || attn_drop_p < 0.f || attn_drop_p >= 1.f) return TXE_ERR_ARG;
    const int Kt = Kh + Pd, Kp = round_up(Kt, 32);
    CollapseWs p = plan_collapse_ws(ws, n_nodes, n_edges, G, Kp, D, Pd, vocab);
    if (ws_bytes < p.total) return TXE_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const unsigned* mk = (mask && feat_drop_p > 0.f) ? mask : nullptr;
    const int mask_ld = (Kt + 31) / 32;
    const float fs = mk ? 1.f / (1.f - feat_drop_p) : 1.f, as = 1.f / (1.f - attn_drop_p);
    const float* wa = Wp + (long long)D * Kp;
    const unsigned* dummy_mask = reinterpret_cast<const unsigned*>(X);
    int rc;
    // ---- dZ = d_hg W ;  dW (main part, split-K partial slices) = d_hg^T Z ----
    {
        VMat A = vmat_plain(d_hg, ld_dhg, G, D);
        VMat B = vmat_plain(Wp, Kp, D, Kp);
        Epi E = epi_plain(p.dZ, Kp, Kp);
        E.alg_flops = 2.0 * G * (double)Kt * D;
        rc = gemm_nn(A, B, E, G, Kp, D, 1, s, p.tail, p.tail_bytes);
        if (rc) return rc;
    }
    const long long split_stride = (long long)D * Kp;
    {
        VMat A = vmat_plain(d_hg, ld_dhg, G, D);
        VMat B = vmat_plain(Z, Kp, G, Kp);
        Epi E = epi_plain(p.part, Kp, Kp);
        E.split_stride = split_stride;
        E.alg_flops = 2.0 * D * (double)Kt * G;
        rc = gemm_tn(A, B, E, D, Kp, G, p.splits, s);
        if (rc) return rc;
    }
    const int S = G > 0 ? p.splits : 0;
    const int nblk = (G > 0 && n_nodes > 0) ? p.chunks : 0;
    if (G > 0 && n_nodes > 0) {
        const int ntile = (Kp / 4 + 63) / 64;
        rc = cl_bwd_dot_launch(n_nodes, gid, X, Kp, mk, dummy_mask, mask_ld, fs, (const float*)p.dZ, wsum, coef, p.dc, p.cn, (G + 3) / 4, G, D, d_hg, ld_dhg,
                               hg, ld_hg, p.dS, 4.0 * ((n_nodes + (double)G) * Kp + 2.0 * G * D), s);
        if (rc) return rc;
        cl_attn_bwd_launch(false, rowptr_in, col_src, rowptr_out, pos_out, graph_off, G, a12, attn_slope, alpha, attn_drop_p, as, seed, pos, pw, p.dc,
                           p.dS, p.dz, p.da1, p.da2, p.dwv, FoldDcArgs{}, s);
        {
            const long long nwaves = (long long)p.chunks * ntile;
            ProfScope prof(mk ? "cl_bwd_dx_kernel<true, true>" : "cl_bwd_dx_kernel<false, true>", s, 4.0 * (2.0 * n_nodes + G) * Kp, 1);
            if (mk) hipLaunchKernelGGL((cl_bwd_dx_kernel<true, true>), dim3((unsigned)((nwaves + 3) / 4)), dim3(256), 0, s, n_nodes, ntile, gid, X, Kp, Kh, mk,
                                       mask_ld, fs, (const float*)p.dZ, (const float*)p.cn, (const float*)p.da1, (const float*)p.da2, wa, act_on,
                                       act_slope, d_X, p.dwa_part);
            else hipLaunchKernelGGL((cl_bwd_dx_kernel<false, true>), dim3((unsigned)((nwaves + 3) / 4)), dim3(256), 0, s, n_nodes, ntile, gid, X, Kp, Kh,
                                    dummy_mask, mask_ld, fs, (const float*)p.dZ, (const float*)p.cn, (const float*)p.da1, (const float*)p.da2, wa,
                                    act_on, act_slope, d_X, p.dwa_part);
        }
        TXE_CHECK_LAUNCH();
    }
    // ---- phase A: d_wa = sum of the per-block partials; partial position sums (embedding / readout position-weight gradients) ----
    const int nseg = n_nodes > 0 ? p.seg_blocks : 0;
    TailA ta;
    memset(&ta, 0, sizeof(ta));
    ta.nb_s1a = Pd > 0 ? nseg : 0; ta.s1a = Seg1Args{d_X + Kh, (long long)Kp, Pd, p.ppart};
    ta.nb_s1b = pw ? nseg : 0; ta.s1b = Seg1Args{p.dwv, 1, 1, p.ppart2};
    ta.pos = pos; ta.n_rows = n_nodes; ta.vocab = vocab; ta.rows_per_block = p.seg_rows;
    ta.r_kind = 2; ta.nb_r = (2 * Kp + 63) / 64; ta.r2 = Seg2Args{p.dwa_part, nblk, 2 * Kp, p.dwa};
    rc = tail_a_launch(ta, s);
    if (rc) return rc;
    // ---- phase B: dW = main + attn (x) d_wa, d_attn = <d_wa, W> (unfold);  dP, d_pw ----
    TailB tb;
    memset(&tb, 0, sizeof(tb));
    tb.nb_u = D;
    tb.u = UnfoldArgs{p.part, S, split_stride, p.dwa, (long long)Kp, W, (long long)Kt, attn_l, attn_r, 1, D, Kt, dW, (long long)Kt, d_attn_l,
                      d_attn_r};
    tb.nb_2a = Pd > 0 ? (vocab * Pd + 63) / 64 : 0;
    tb.s2a = Seg2Args{p.ppart, nseg, vocab * Pd, dP};
    tb.nb_2b = pw ? (vocab + 63) / 64 : 0;
    tb.s2b = Seg2Args{p.ppart2, nseg, vocab, d_pw};
    return tail_b_submit(&tb, nullptr, false, s);
}

}  // extern "C"

// =====================================================================================================================
// Last GCNLayer folded behind MeanReadout / WeightedMeanReadout (PGCN / GCN output layer: no activation; model_zoo.py:35-47,
// 139-167, 227-242):  hg[g] = sum_v w_v/S_g (norm_v sum_{u->v} norm_u Xd[u] W + b) = (sum_{u in g} c_u Xd[u]) W + b,
//     c_u = norm_u sum_{v : u->v} w_v norm_v / S_g      -- graph constants (no attention): one sweep forward, one backward
// (two with learnable readout weights).  Reuses the sweep kernels of the GAT fold above.
// =====================================================================================================================
namespace txe {

// one wave per source: c~_u = norm_u * sum_{j in out(u)} w_{dst(j)} norm_{dst(j)}
__global__ __launch_bounds__(256) void gcl_coef_kernel(const int* __restrict__ rowptr_out, const int* __restrict__ col_dst, int n_nodes,
                                                       const float* __restrict__ norm, const int* __restrict__ pos,
                                                       const float* __restrict__ pw, float* __restrict__ coef) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int u = blockIdx.x * 4 + w;
    if (u >= n_nodes) return;
    float c = 0.f;
    for (int j = rowptr_out[u] + l; j < rowptr_out[u + 1]; j += 64) {
        const int v = col_dst[j];
        c = fmaf(pw ? cl_softplus(pw[pos[v]]) : 1.f, norm[v], c);
    }
    c = wave_sum(c);
    if (l == 0) coef[u] = c * norm[u];
}

// one wave per destination: dwv[v] = (dS_g(v) + norm_v sum_{p in in(v)} norm_u dc~_u) * sigmoid(pw[pos_v])
__global__ __launch_bounds__(256) void gcl_bwd_w_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, int n_nodes,
                                                        const float* __restrict__ norm, const int* __restrict__ pos,
                                                        const float* __restrict__ pw, const float* __restrict__ dc,
                                                        const float* __restrict__ dS, const int* __restrict__ gid,
                                                        float* __restrict__ dwv) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int v = blockIdx.x * 4 + w;
    if (v >= n_nodes) return;
    float a = 0.f;
    for (int p = rowptr[v] + l; p < rowptr[v + 1]; p += 64) a = fmaf(norm[col[p]], dc[col[p]], a);
    a = wave_sum(a);
    if (l == 0) dwv[v] = (dS[gid[v]] + norm[v] * a) * cl_sigmoid(pw[pos[v]]);
}

// y[g][f] += b[f]
__global__ void gcl_add_bias_kernel(float* __restrict__ y, long long ld, int rows, int cols, const float* __restrict__ b) {
    const long long n = (long long)rows * cols;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        y[(i / cols) * ld + (i % cols)] += b[i % cols];
}

struct GclWs {
    float *dZ, *part, *dc, *cn, *dS, *dwv, *ppart, *ppart2, *cpart;
    void* tail;
    size_t tail_bytes, total;
    int splits, seg_blocks, seg_rows;
};

static GclWs plan_gcl_ws(void* ws, int n, int G, int Kp, int Fop, int Pd, int vocab) {
    GclWs p;
    char* b = (char*)ws;
    size_t off = 0;
    auto take = [&](size_t bytes) { float* r = (float*)(b + off); off += align_up(bytes > 0 ? bytes : 4, 256); return r; };
    const int n1 = n > 0 ? n : 1, g1 = G > 0 ? G : 1, v1 = vocab > 0 ? vocab : 1;
    p.dZ = take((size_t)g1 * Kp * 4);
    p.splits = choose_splits(Kp, Fop, G);
    p.part = take((size_t)p.splits * Kp * Fop * 4);
    p.dc = take((size_t)n1 * 4);
    p.cn = take((size_t)n1 * 4);
    p.dS = take((size_t)g1 * 4);
    p.dwv = take((size_t)n1 * 4);
    p.seg_rows = 64;
    p.seg_blocks = (n + p.seg_rows - 1) / p.seg_rows;
    if (p.seg_blocks < 1) p.seg_blocks = 1;
    p.ppart = take((size_t)p.seg_blocks * v1 * (Pd > 0 ? Pd : 1) * 4);
    p.ppart2 = take((size_t)p.seg_blocks * v1 * 4);
    p.cpart = take(colsum_ws_bytes(G, Fop));
    p.tail_bytes = gemm_tail_ws_bytes();
    p.tail = take(p.tail_bytes);
    p.total = off;
    return p;
}

// cn[u] = coef[u] / S_g(u)   (MeanReadout path: no dot sweep to piggy-back on)
__global__ void gcl_cn_kernel(int n_nodes, const int* __restrict__ gid, const float* __restrict__ coef, const float* __restrict__ wsum,
                              float* __restrict__ cn) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_nodes) return;
    const float S = wsum[gid[u]];
    cn[u] = S > 0.f ? coef[u] / S : 0.f;
}

}  // namespace txe
using namespace txe;
extern "C" {

size_t txe_gcn_collapse_ws_bytes(int n_nodes, int G, int Kh, int Pd, int Fo, int vocab) {
    return plan_gcl_ws(nullptr, n_nodes, G, round_up(Kh + Pd, 32), round_up(Fo, 32), Pd, vocab).total;
}

// X [N][Kp], Wp [Kp128][Fop], mask as for txe_gcn_dense_*; norm [N] (txe_gcn_norm); bias [Fo] or NULL; pw == NULL: MeanReadout.
// Saved for backward: coef [N], wsum [G], gid [N], Z [G][Kp].  hg [G][Fo] (row stride ld_hg).
int txe_gcn_collapse_fwd(const struct txe_graph_batch* batch, const struct txe_gcn_fold_layer* layer, void* ws, size_t ws_bytes, void* stream) {
    if (!batch || !layer) return TXE_ERR_ARG;
    const int *rowptr_out = batch->rowptr_out, *col_dst = batch->col_dst, *graph_off = batch->graph_off, *pos = layer->pos;
    const int n_nodes = batch->n_nodes, G = batch->G, Kh = layer->Kh, Pd = layer->Pd, Fo = layer->Fo;
    const float *X = layer->X, *Wp = layer->Wp, *bias = layer->bias, *norm = layer->norm, *pw = layer->pw;
    const unsigned* mask = layer->mask;
    const float drop_p = layer->drop_p;
    float *coef = layer->coef, *wsum = layer->wsum, *Z = layer->Z, *hg = layer->hg;
    int* gid = layer->gid;
    const long long ld_hg = layer->ld_hg;
    if (n_nodes < 0 || G < 0 || Kh < 1 || Pd < 0 || Fo < 1 || !rowptr_out || !graph_off || !X || !Wp || !norm || !coef || !wsum || !gid || !Z ||
        !ws || (pw && !pos))
        return TXE_ERR_ARG;
    if (drop_p < 0.f || drop_p >= 1.f) return TXE_ERR_ARG;
    const int Kt = Kh + Pd, Kp = round_up(Kt, 32), Fop = round_up(Fo, 32);
    GclWs p = plan_gcl_ws(ws, n_nodes, G, Kp, Fop, Pd, 0);
    if (ws_bytes < p.total) return TXE_ERR_WORKSPACE;
    if (G == 0) return TXE_OK;
    hipStream_t s = (hipStream_t)stream;
    const unsigned* mk = (mask && drop_p > 0.f) ? mask : nullptr;
    const unsigned* dummy_mask = reinterpret_cast<const unsigned*>(X);
    const int mask_ld = (Kt + 31) / 32;
    const float fs = mk ? 1.f / (1.f - drop_p) : 1.f;
    if (n_nodes > 0)
        hipLaunchKernelGGL(gcl_coef_kernel, dim3((n_nodes + 3) / 4), dim3(256), 0, s, rowptr_out, col_dst, n_nodes, norm, pos, pw, coef);
    hipLaunchKernelGGL(cl_wsum_kernel, dim3((G + 3) / 4), dim3(256), 0, s, graph_off, G, pos, pw, wsum, gid);
    const int rc_z = cl_zsum_launch(graph_off, G, n_nodes, X, Kp, mk, dummy_mask, mask_ld, fs, (const float*)coef, (const float*)wsum, Z, s);
    if (rc_z) return rc_z;
    if (!hg) return TXE_OK;          // (the caller folds hg = Z W + b into what consumes it: txe_bilinear_folded_*, wf_by_k)
    VMat A = vmat_plain(Z, Kp, G, Kp);
    VMat B = vmat_plain(Wp, Fop, Kp, Fop);
    Epi E = epi_plain(hg, ld_hg, Fo);
    E.alg_flops = 2.0 * G * (double)Fo * Kt;
    int rc = gemm_nn(A, B, E, G, Fo, Kp, 1, s, p.tail, p.tail_bytes);
    if (rc) return rc;
    if (bias) {
        const long long n = (long long)G * Fo;
        hipLaunchKernelGGL(gcl_add_bias_kernel, dim3((int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048)), dim3(256), 0, s, hg, ld_hg, G, Fo,
                           bias);
        TXE_CHECK_LAUNCH();
    }
    return TXE_OK;
}

// d_hg [G][Fo] -> d_X [N][Kp] (layout of txe_gcn_dense_bwd), dW [Kt][Fo], d_b [Fo] (or NULL), dP, d_pw.
int txe_gcn_collapse_bwd(const struct txe_graph_batch* batch, const struct txe_gcn_fold_layer* layer, const float* d_hg, long long ld_dhg,
                         int act_on, float act_slope, float* d_X, const struct txe_gcn_fold_grads* grads, int dz_given, void* ws, size_t ws_bytes,
                         void* stream) {
    if (!batch || !layer || !grads) return TXE_ERR_ARG;
    const int *rowptr_in = batch->rowptr_in, *col_src = batch->col_src, *graph_off = batch->graph_off, *pos = layer->pos, *gid = layer->gid;
    const int n_nodes = batch->n_nodes, G = batch->G, Kh = layer->Kh, Pd = layer->Pd, Fo = layer->Fo, vocab = layer->vocab;
    const float *X = layer->X, *Wp = layer->Wp, *norm = layer->norm, *pw = layer->pw, *coef = layer->coef, *wsum = layer->wsum, *Z = layer->Z;
    const unsigned* mask = layer->mask;
    const float drop_p = layer->drop_p;
    float *dW = grads->dW, *d_b = grads->d_b, *dP = grads->dP, *d_pw = grads->d_pw;
    // dz_given: `d_hg` IS dZ [G][Kp] (ld_dhg == Kp) -- whoever consumed Z folded hg = Z W + b into its own products (txe_bilinear_folded_*,
    // wf_by_k) and formed dW / d_b itself: no product here, dW / d_b are not written
    if (n_nodes < 0 || G < 0 || Kh < 1 || Pd < 0 || Fo < 1 || !rowptr_in || !graph_off || !X || !Wp || !norm || !coef || !wsum || !gid || !Z ||
        !d_hg || !d_X || (!dW && !dz_given) || !ws)
        return TXE_ERR_ARG;
    if (dz_given && ld_dhg != round_up(Kh + Pd, 32)) return TXE_ERR_ARG;
    if ((Pd > 0 || pw) && (!pos || vocab < 1 || vocab > MAX_VOCAB)) return TXE_ERR_ARG;
    if ((Pd > 0 && !dP) || (pw && !d_pw)) return TXE_ERR_ARG;
    if (drop_p < 0.f || drop_p >= 1.f) return TXE_ERR_ARG;
    const int Kt = Kh + Pd, Kp = round_up(Kt, 32), Fop = round_up(Fo, 32);
    GclWs p = plan_gcl_ws(ws, n_nodes, G, Kp, Fop, Pd, vocab);
    if (ws_bytes < p.total) return TXE_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const unsigned* mk = (mask && drop_p > 0.f) ? mask : nullptr;
    const unsigned* dummy_mask = reinterpret_cast<const unsigned*>(X);
    const int mask_ld = (Kt + 31) / 32;
    const float fs = mk ? 1.f / (1.f - drop_p) : 1.f;
    int rc;
    if (dz_given) p.dZ = const_cast<float*>(d_hg);
    if (!dz_given) {   // dZ[g][k] = sum_f d_hg[g][f] Wp[k][f]
        VMat A = vmat_plain(d_hg, ld_dhg, G, Fo);
        VMat B = vmat_plain(Wp, Fop, round_up(Kp, 128), Fop);
        Epi E = epi_plain(p.dZ, Kp, Kp);
        E.alg_flops = 2.0 * G * (double)Kt * Fo;
        rc = gemm_nt(A, B, E, G, Kp, Fo, 1, s, p.tail, p.tail_bytes);
        if (rc) return rc;
    }
    if (!dz_given) {   // dW[k][f] = sum_g Z[g][k] d_hg[g][f]
        VMat A = vmat_plain(Z, Kp, G, Kp);
        VMat B = vmat_plain(d_hg, ld_dhg, G, Fo);
        Epi E = epi_plain(p.part, Fop, Fo);
        E.split_stride = (long long)Kp * Fop;
        E.alg_flops = 2.0 * Kt * (double)Fo * G;
        rc = gemm_tn(A, B, E, Kp, Fo, G, p.splits, s);
        if (rc) return rc;
        rc = reduce_splits_sub_launch(p.part, G > 0 ? p.splits : 0, E.split_stride, Kt, Fo, Fop, dW, s);
        if (rc) return rc;
    }
    if (d_b && !dz_given) {
        rc = colsum_launch(d_hg, ld_dhg, G, Fo, p.cpart, d_b, s);
        if (rc) return rc;
    }
    if (G > 0 && n_nodes > 0) {
        const int nb = (n_nodes + 3) / 4;
        const int ntile = (Kp / 4 + 63) / 64;
        if (pw) {
            hipLaunchKernelGGL(cl_bwd_ds_kernel, dim3((G + 3) / 4), dim3(256), 0, s, G, Kp, (const float*)p.dZ, Z, wsum, p.dS);
            // (the bias makes hg != Z W here, so dS keeps its own kernel: no leading dS workgroups)
            rc = cl_bwd_dot_launch(n_nodes, gid, X, Kp, mk, dummy_mask, mask_ld, fs, (const float*)p.dZ, wsum, coef, p.dc, p.cn, 0, 0, 0, nullptr, 0LL, nullptr,
                                   0LL, nullptr, 4.0 * (n_nodes + (double)G) * Kp, s);
            if (rc) return rc;
            hipLaunchKernelGGL(gcl_bwd_w_kernel, dim3(nb), dim3(256), 0, s, rowptr_in, col_src, n_nodes, norm, pos, pw, (const float*)p.dc,
                               (const float*)p.dS, gid, p.dwv);
        } else {
            hipLaunchKernelGGL(gcl_cn_kernel, dim3((n_nodes + 255) / 256), dim3(256), 0, s, n_nodes, gid, coef, wsum, p.cn);
        }
        {
            const long long nwaves = (long long)((n_nodes + CL_CHUNK - 1) / CL_CHUNK) * ntile;
            ProfScope prof(mk ? "cl_bwd_dx_kernel<true, false>" : "cl_bwd_dx_kernel<false, false>", s, 4.0 * (2.0 * n_nodes + G) * Kp, 1);
            if (mk) hipLaunchKernelGGL((cl_bwd_dx_kernel<true, false>), dim3((unsigned)((nwaves + 3) / 4)), dim3(256), 0, s, n_nodes, ntile, gid, X, Kp,
                                       Kh, mk, mask_ld, fs, (const float*)p.dZ, (const float*)p.cn, (const float*)nullptr,
                                       (const float*)nullptr, (const float*)nullptr, act_on, act_slope, d_X, (float*)nullptr);
            else hipLaunchKernelGGL((cl_bwd_dx_kernel<false, false>), dim3((unsigned)((nwaves + 3) / 4)), dim3(256), 0, s, n_nodes, ntile, gid, X,
                                    Kp, Kh, dummy_mask, mask_ld, fs, (const float*)p.dZ, (const float*)p.cn, (const float*)nullptr,
                                    (const float*)nullptr, (const float*)nullptr, act_on, act_slope, d_X, (float*)nullptr);
        }
        TXE_CHECK_LAUNCH();
    }
    if (Pd > 0) {
        rc = pos_segsum_launch(d_X + Kh, (long long)Kp, pos, n_nodes, Pd, vocab, p.seg_blocks, p.seg_rows, p.ppart, dP, s);
        if (rc) return rc;
    }
    if (pw) {
        rc = pos_segsum_launch(p.dwv, 1, pos, n_nodes, 1, vocab, p.seg_blocks, p.seg_rows, p.ppart2, d_pw, s);
        if (rc) return rc;
    }
    return TXE_OK;
}

}  // extern "C"
