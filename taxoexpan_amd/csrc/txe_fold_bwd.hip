// ---------------------------------------------------------------------------------------------------------------------
// Folded layer's d_X sweep FUSED with the previous GATLayer's message/reduce backward (one row sweep instead of three).
// The unfused chain writes d_X' = d(folded layer's input) [N][Kp] (cl_bwd_dx), then reads it twice more: gat_bwd_edge
// (d alpha_e = <d_pre[v], ft[u]>) and gat_bwd_node (d_ft[u] = sum alpha'_e d_pre[v]) -- ~920 MB of HBM traffic on the 18 k-node
// training batch.  But a row of d_pre is an ELEMENTWISE function of rows that are read anyway:
//     d_pre[v][j] = keep[v][j] s (cn_v dZ[g(v)][j] + da1_v wa1[j] + da2_v wa2[j]) leaky'(X'[v][j])          (j < H*D)
// so the source-side sweep can form it on the fly: for source node u, with ft[u] in registers, every out-edge (u -> v) loads X'[v]
// (the row cl_bwd_dx would have read), forms d_pre[v], and uses it twice -- the dot product with ft[u] (d alpha_e) and the
// alpha'-weighted accumulation (d_ft[u]).  d_X' never exists; X', dZ and Y are each read once (+ L2 hits for shared rows), d_Y is
// written once: ~475 MB.  The four waves of a workgroup own a quarter of the H*D row each (for H = 4: one head per wave, so the
// per-head dot products are wave-local); a workgroup walks FB_NODES consecutive source nodes, whose out-edge scalars
// (destination, CSR position, cn, da1, da2) are staged in LDS once, so that the row loads depend on nothing but LDS.
// The per-node leftovers of cl_bwd_dx ride along: the folded attention rows' gradient partials (sum_u da_u Xd'[u]) per workgroup,
// and the position-embedding gradient partials from the (never stored) position columns of d_X'.
// What is left per edge -- softmax / leaky-relu backward of the previous layer's attention from the raw d alpha -- is
// gat_attn_bwd_job (edge-level, a few microseconds; launched together with stage 1 of the reductions).
// ---------------------------------------------------------------------------------------------------------------------
#include <string.h>

#include "txe_gemm.h"
#include "txe_gather.h"
#include "txe_tail.h"
#include "txe_fold.h"
#include "txe_ego_row.h"

namespace txe {

constexpr int FB_NODES = 32;        // most source nodes a workgroup walks (fb_nodes_per_wg picks the number for a batch)
constexpr int FB_MAXE = 192;        // out-edges of a workgroup whose scalars are staged in LDS (beyond: read from global)
#ifndef TXE_FB_EU
#define TXE_FB_EU 4
#endif
#ifndef TXE_FB_OCC
#define TXE_FB_OCC 3
#endif
constexpr int FB_EU = TXE_FB_EU;      // out-edges per round trip behind a node's first two
constexpr int FB_MAXPD = 128;       // position columns (Kp - Kh <= 128 is a precondition of the fused path)

struct FusedBwdArgs {
    const int *rowptr_out, *col_dst, *pos_out, *gid, *pos;
    int n_nodes;
    const float* X; int Kp, Kh, Pd; const unsigned* mask; int mask_ld; float fscale;
    const float *dZ, *cn, *da1, *da2, *wa; float act_slope; int vocab;
    const float* Y; long long ld_y; int H, D; const float* alpha; float drop_p, drop_scale; unsigned long long seed;
    float* d_Y; long long ld_dy; float* dal; float* dwa_part; float* ppart;
    int npw;                            // source nodes per workgroup
    // (the egonet-walking variant) the graphs themselves: destination CSR, graph offsets, node -> graph
    const int *rowptr_in, *col_src, *goff, *ggid; int G;
    float* hpart;                       // [workgroups][H*D]: a workgroup's share of d_ft[hub] for a graph whose hub lives in an earlier window
    const int* plan;                    // [n_nodes][8] or NULL: the batch's walk plan (egonet_walk_plan_kernel): the shape checks done once
};

// Source nodes per workgroup of the fused sweep.  The kernel holds 3 workgroups per CU; its workgroups cost about (nodes + 6) each (LDS
// staging of the folded rows, the partial rows written at the end), and a last partial round costs a whole one: on the 18 k-node
// training batch 24 nodes make 745 workgroups = one round of 768 (141 us), 16 make 1.46 rounds (153 us), 32 three quarters of one (154 us).
static inline int fb_nodes_per_wg(int n_nodes, int occupancy = 3) {
#ifdef TXE_FB_NPW
    return TXE_FB_NPW;                  // (a build for measurements: the window forced, 12..FB_NODES)
#endif
    const int slots = occupancy * device_cu_count();
    int best = 16;
    double best_cost = 1e30;
    for (int npw = 12; npw <= FB_NODES; npw += 2) {
        const long long blocks = ((long long)n_nodes + npw - 1) / npw;
        const double cost = (double)((blocks + slots - 1) / slots) * (npw + 6.0);
        if (cost <= best_cost) { best_cost = cost; best = npw; }     // (ties: fewer, larger workgroups)
    }
    return best;
}

// keep bits (low 4) of the 4 columns starting at c (multiple of 4) of row r; all ones without a mask
template <bool MASK>
__device__ __forceinline__ unsigned fb_keep(const unsigned* __restrict__ mask, int mask_ld, long long r, int c) {
    if constexpr (!MASK) return 0xFu;
    // c < Kp = 32 * mask_ld always (the mask has one word per 32 columns of the PADDED row), so the word exists: no bounds select
    // here -- with one, hipcc sinks the load into the conditional and waits vmcnt(0) right behind it, serialising every row load
    return (mask[r * mask_ld + (c >> 5)] >> (c & 31)) & 0xFu;
}

// One workgroup's share of the fused sweep.  STAGED: the out-edge scalars of its FB_NODES source nodes sit in LDS (the usual case);
// otherwise (more than FB_MAXE out-edges) they are read from global memory with dependent loads -- correct, slow, rare.
// There is NO branch between a load and its first use (hipcc waits vmcnt(0) at every control-flow merge behind a pending load):
// every address is clamped to something readable, conditions become weights of 0.
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ float uni(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

template <int NI, int EU> struct FbGroup {
    int p[EU];
    float cnv[EU], g1v[EU], g2v[EU], al[EU];
    float xv[EU][NI][4];
    unsigned mv[EU][NI];
};

template <bool MASK, int NI, int NWH, bool STAGED>
__device__ __forceinline__ void fb_body(const FusedBwdArgs& a, const int b, const int u0, const int u1, const int e0, const int ne,
                                        const int* s_v, const int* s_p, const float* s_cn, const float* s_g1, const float* s_g2,
                                        const int* s_ni, const float* s_nf, float (*s_dot)[4], float* s_dp, const float* s_wa,
                                        float* s_acc) {
    const int w = uni((int)(threadIdx.x >> 6)), l = threadIdx.x & 63;   // w is wave-uniform: say so (SGPRs, scalar ALU)
    const int F = a.H * a.D, SL = F >> 2, nvec = SL >> 2;
    const int c0 = w * SL, hw = c0 / a.D;
    const int Kp = a.Kp;
    int off[NI];
    float live[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int j = l + 64 * i;
        off[i] = c0 + 4 * ((j < nvec) ? j : 0);
        live[i] = (j < nvec) ? 1.f : 0.f;
    }
    // tail columns [F, Kp) (position embedding + padding) of the folded layer's input: lanes of wave 0 (the loads are issued by
    // every lane with clamped addresses; only the tail lanes use them)
    const int tvec = (Kp - F) >> 2;
    const bool tail = (w == 0) && (l < tvec);
    const int tc = min(F + 4 * (tail ? l : 0), Kp - 4);
    const int elast = max(ne - 1, 0);

    // the rows of EU consecutive out-edges, all loads issued together; edge scalars are wave-uniform (SGPRs)
    auto load_group = [&](auto& q, const int j, const int je) {
        constexpr int EU = sizeof(q.p) / sizeof(int);
#pragma unroll
        for (int t = 0; t < EU; ++t) {
            const int idx = min(max(min(j + t, je - 1) - e0, 0), elast);
            int v;
            if constexpr (STAGED) { v = uni(s_v[idx]); q.p[t] = uni(s_p[idx]); q.cnv[t] = uni(s_cn[idx]); q.g1v[t] = uni(s_g1[idx]); q.g2v[t] = uni(s_g2[idx]); }
            else { v = a.col_dst[e0 + idx]; q.p[t] = a.pos_out[e0 + idx]; q.cnv[t] = a.cn[v]; q.g1v[t] = a.da1[v]; q.g2v[t] = a.da2[v]; }
            q.al[t] = a.alpha[(long long)q.p[t] * a.H + hw];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                vload<4>(a.X + (long long)v * Kp + off[i], q.xv[t][i]);
                q.mv[t][i] = fb_keep<MASK>(a.mask, a.mask_ld, v, off[i]);
            }
        }
    };
    // d alpha_e (raw) and the alpha'-weighted accumulation for the EU edges of a group
    auto use_group = [&](auto& q, const int j, const int je, const float (&ft)[NI][4], const float (&dz)[NI][4], float (&acc)[NI][4]) {
        constexpr int EU = sizeof(q.p) / sizeof(int);
        float fd[EU];
#pragma unroll
        for (int t = 0; t < EU; ++t) {
            fd[t] = 1.f;
            if (j + t < je) {                                      // wave-uniform (and behind every load of the group): the clamped
                                                                   // duplicates that pad a short group cost no arithmetic
                fd[t] = (a.drop_p > 0.f) ? drop_factor(a.seed, (unsigned long long)q.p[t] * a.H + hw, a.drop_p, a.drop_scale) : 1.f;
                const float coef = q.al[t] * fd[t];
                const float sc = q.cnv[t] * a.fscale, s1 = q.g1v[t] * a.fscale, s2 = q.g2v[t] * a.fscale;     // (uniform: scalar ALU)
                float part = 0.f;
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    float w1[4], w2[4];
                    vload<4>(s_wa + off[i], w1);
                    vload<4>(s_wa + Kp + off[i], w2);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float tv = sc * dz[i][k] + s1 * w1[k] + s2 * w2[k];
                        const float lk = (q.xv[t][i][k] > 0.f) ? live[i] : a.act_slope * live[i];
                        const float dp = ((q.mv[t][i] >> k) & 1u) ? tv * lk : 0.f;
                        part = fmaf(dp, ft[i][k], part);
                        acc[i][k] = fmaf(coef, dp, acc[i][k]);
                    }
                }
                part = wave_sum(part);
                if constexpr (NWH > 1) {                           // a head spans NWH waves: combine their partial dot products
                    if (l == 0) s_dot[t][w] = part;
                } else {
                    if (l == 0) a.dal[(long long)q.p[t] * a.H + hw] = part * fd[t];
                }
            }
        }
        if constexpr (NWH > 1) {
            __syncthreads();
            if (l == 0 && (w % NWH) == 0) {
#pragma unroll
                for (int t = 0; t < EU; ++t) {
                    float tot = 0.f;
#pragma unroll
                    for (int x = 0; x < NWH; ++x) tot += s_dot[t][w + x];
                    if (j + t < je) a.dal[(long long)q.p[t] * a.H + hw] = tot * fd[t];
                }
            }
            __syncthreads();
        }
    };

    for (int u = u0; u < u1; ++u) {
        const int un = u - u0;                                      // per-node scalars were staged with the edge scalars
        const int g = uni(s_ni[4 * un]), jb = uni(s_ni[4 * un + 1]), je = uni(s_ni[4 * un + 2]), pu = s_ni[4 * un + 3];
        const float g1u = uni(s_nf[4 * un]), g2u = uni(s_nf[4 * un + 1]), cnu = s_nf[4 * un + 2];
        float ft[NI][4], dz[NI][4], acc[NI][4];
        float xu[NI][4], xt[4], dzt[4];
        unsigned mu[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {                              // this node's own rows ...
            vload<4>(a.Y + (long long)u * a.ld_y + off[i], ft[i]);
            vload<4>(a.dZ + (long long)g * Kp + off[i], dz[i]);
            vload<4>(a.X + (long long)u * Kp + off[i], xu[i]);
            mu[i] = fb_keep<MASK>(a.mask, a.mask_ld, u, off[i]);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[i][k] = 0.f;
        }
        vload<4>(a.X + (long long)u * Kp + tc, xt);
        vload<4>(a.dZ + (long long)g * Kp + tc, dzt);
        const unsigned mt = fb_keep<MASK>(a.mask, a.mask_ld, u, tc);
        FbGroup<NI, 2> q;
        load_group(q, jb, je);                                      // ... and its first two out-edges' rows: one round trip
        // own-row leftovers of cl_bwd_dx: d_wa partials (per workgroup, in LDS), position columns of d_X'
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            float a1[4], a2[4];
            vload<4>(s_acc + off[i], a1);
            vload<4>(s_acc + Kp + off[i], a2);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float xd = ((mu[i] >> k) & 1u) ? xu[i][k] * a.fscale * live[i] : 0.f;
                a1[k] = fmaf(g1u, xd, a1[k]);
                a2[k] = fmaf(g2u, xd, a2[k]);
            }
            if (l + 64 * i < nvec) { vstore<4>(s_acc + off[i], a1); vstore<4>(s_acc + Kp + off[i], a2); }
        }
        if (tail) {
            float a1[4], a2[4], wt1[4], wt2[4];
            vload<4>(s_acc + tc, a1);
            vload<4>(s_acc + Kp + tc, a2);
            vload<4>(s_wa + tc, wt1);
            vload<4>(s_wa + Kp + tc, wt2);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool keep = ((mt >> k) & 1u) != 0u;
                const float xd = keep ? xt[k] * a.fscale : 0.f;
                a1[k] = fmaf(g1u, xd, a1[k]);
                a2[k] = fmaf(g2u, xd, a2[k]);
                const int pc = tc + k - a.Kh;                      // position column (d_X' there has no activation factor)
                if (pc >= 0 && pc < a.Pd) s_dp[pu * a.Pd + pc] += keep ? a.fscale * (cnu * dzt[k] + g1u * wt1[k] + g2u * wt2[k]) : 0.f;
            }
            vstore<4>(s_acc + tc, a1);
            vstore<4>(s_acc + Kp + tc, a2);
        }
        if (jb < je) use_group(q, jb, je, ft, dz, acc);
        for (int j = jb + 2; j < je; j += FB_EU) {                  // a hub's further out-edges, FB_EU rows per round trip
            FbGroup<NI, FB_EU> q4;
            load_group(q4, j, je);
            use_group(q4, j, je, ft, dz, acc);
        }
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (l + 64 * i < nvec) vstore<4>(a.d_Y + (long long)u * a.ld_dy + off[i], acc[i]);
    }
}

template <bool MASK, int NI, int NWH /* waves per head = 4 / H */>
// (three workgroups per CU = 168 VGPRs hold the sweep up to NI = 2 -- rows of up to 2,048 columns, the MAG shape; wider rows (SemEval:
//  2,400) spilled 77 registers per lane there: two workgroups per CU, 256 VGPRs)
__global__ __launch_bounds__(256, (NI >= 3) ? 2 : TXE_FB_OCC) void gat_fused_bwd_kernel(const FusedBwdArgs a) {
    __shared__ int s_v[FB_MAXE], s_p[FB_MAXE], s_ni[4 * FB_NODES];
    __shared__ float s_cn[FB_MAXE], s_g1[FB_MAXE], s_g2[FB_MAXE], s_nf[4 * FB_NODES];
    __shared__ float s_dot[4][4];
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];   // [2][Kp] folded attention rows | [2][Kp] their gradient partials |
    const int b = xcd_remap(blockIdx.x, gridDim.x);                 // [vocab][Pd] position-embedding gradient partials
    const int u0 = b * a.npw, u1 = min(a.n_nodes, u0 + a.npw);
    const int Kp = a.Kp;
    float* s_wa = s_dyn;
    float* s_acc = s_dyn + 2 * Kp;
    float* s_dp = s_dyn + 4 * Kp;
    const int e0 = a.rowptr_out[u0], ne = a.rowptr_out[u1] - e0;
    if (threadIdx.x == 0) { s_v[0] = u0; s_p[0] = 0; s_cn[0] = 0.f; s_g1[0] = 0.f; s_g2[0] = 0.f; }   // (a workgroup without out-edges)
    __syncthreads();
    for (int i = threadIdx.x; i < min(ne, FB_MAXE); i += 256) {
        const int v = a.col_dst[e0 + i];
        s_v[i] = v; s_p[i] = a.pos_out[e0 + i];
        s_cn[i] = a.cn[v]; s_g1[i] = a.da1[v]; s_g2[i] = a.da2[v];
    }
    if (threadIdx.x < u1 - u0) {
        const int u = u0 + threadIdx.x;
        s_ni[4 * threadIdx.x] = a.gid[u]; s_ni[4 * threadIdx.x + 1] = a.rowptr_out[u]; s_ni[4 * threadIdx.x + 2] = a.rowptr_out[u + 1];
        s_ni[4 * threadIdx.x + 3] = a.pos[u];                       // (a readable dummy when there are no position columns)
        s_nf[4 * threadIdx.x] = a.da1[u]; s_nf[4 * threadIdx.x + 1] = a.da2[u]; s_nf[4 * threadIdx.x + 2] = a.cn[u];
    }
    for (int i = threadIdx.x; i < a.vocab * a.Pd; i += 256) s_dp[i] = 0.f;
    for (int i = threadIdx.x * 4; i < 2 * Kp; i += 1024) {
        *reinterpret_cast<float4*>(s_wa + i) = *reinterpret_cast<const float4*>(a.wa + i);
        *reinterpret_cast<float4*>(s_acc + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    if (ne <= FB_MAXE) fb_body<MASK, NI, NWH, true>(a, b, u0, u1, e0, ne, s_v, s_p, s_cn, s_g1, s_g2, s_ni, s_nf, s_dot, s_dp, s_wa, s_acc);
    else fb_body<MASK, NI, NWH, false>(a, b, u0, u1, e0, ne, s_v, s_p, s_cn, s_g1, s_g2, s_ni, s_nf, s_dot, s_dp, s_wa, s_acc);
    // per-workgroup partials: folded attention rows' gradient [2][Kp], position-embedding gradient [vocab][Pd]
    __syncthreads();
    float* dw = a.dwa_part + (long long)b * 2 * Kp;
    for (int i = threadIdx.x * 4; i < 2 * Kp; i += 1024) *reinterpret_cast<float4*>(dw + i) = *reinterpret_cast<const float4*>(s_acc + i);
    for (int i = threadIdx.x; i < a.vocab * a.Pd; i += 256) a.ppart[(long long)b * a.vocab * a.Pd + i] = s_dp[i];
}

// ---- the same sweep, WALKING EGONETS (dataset.py:404-437: parents -> anchor, anchor -> siblings, self loops) -----------------------
// The sweep above fetches X'[v] once per out-edge (u -> v): an anchor's row once per parent, a sibling's row once for the anchor and
// once as its own -- 64 MB of re-fetched rows on the training batch (FETCH_SIZE 374 MB against 326 MB algorithmic).  In an egonet every
// edge that is not a self loop touches ONE node, the hub h (the anchor): parents u have out-edges {u, h}, siblings s have {s} and the
// in-edge h -> s.  With the hub's three row slices in registers -- ft[h], d_pre[h] and the accumulating d_ft[h] -- every other node's rows
// are read exactly once:
//     hub h        : d_pre[h], self edge
//     parent u     : d_pre[u], self edge;  edge u -> h: d alpha = <d_pre[h], ft[u]>, d_ft[u] += alpha' d_pre[h]
//     sibling s    : d_pre[s], self edge;  edge h -> s: d alpha = <d_pre[s], ft[h]>, d_ft[h] += alpha' d_pre[s]
// X', Y are streamed once, d_Y written once: the algorithmic bytes.
// Work list: the nodes of a hub-shaped graph in the order hub, parents, siblings (list position = node index except inside a graph);
// a workgroup walks npw consecutive LIST POSITIONS, two per round trip -- every workgroup the same amount of work, whatever the graph
// sizes (a 54-node egonet beside 2-node ones).  A graph cut by a workgroup boundary: the later workgroup first loads the hub's rows
// again (d_pre[h], ft[h]; nothing written), and leaves ITS share of d_ft[h] in hpart[workgroup]; gat_attn_bwd_reduce_a_kernel -- the next
// launch -- adds those rows to d_Y[h] in workgroup order (fused_hub_fixup_job: deterministic, no atomics).
// The shape is CHECKED per graph from the CSR arrays (out-degrees, out-lists of the small nodes, in-lists of the siblings -- never the
// position labels), by every workgroup that touches the graph: a graph that is not hub-shaped -- or has more than EGO_MAXN nodes -- is
// walked by the generic body above (fb_body, edge scalars from global memory) for the source nodes in the workgroup's window.
// One head per wave (H = 4: the per-head dot products are wave-local); other head counts keep the kernel above.
constexpr int EGO_MAXN = 64;                             // largest hub-shaped graph walked from registers
constexpr int EGO_TAB = FB_NODES + 2 * EGO_MAXN;         // nodes of the graphs that intersect a window of <= FB_NODES positions
enum { EGO_SKIP = 0, EGO_HUB = 1, EGO_PRE = 2, EGO_POST = 3, EGO_FOREIGN = 4 };

// list position (local index t inside a hub-shaped graph with hub h) -> local node index
__device__ __forceinline__ int ego_node_of(int t, int h) { return t == 0 ? h : (t <= h ? t - 1 : t); }

// The walk plan of a batch: what the staging phases (1)-(3) of the kernel below work out per workgroup and step -- hub, roles, CSR
// positions, the list order -- depends on the graphs alone, so it can be done ONCE per batch (it is a view of the graph like the two CSR
// orders).  8 ints per LIST POSITION p: the node walked there, flags (role | walkable << 4 | at most EGO_MAXN nodes << 5), the destination
// CSR positions of its self loop and of its edge with the hub, the graph's hub (node id), the graph's first position.  With a plan the
// sweep's staging is two trips (plan; then the per-node scalars and the edge coefficients) instead of eight.  One wave per graph.
constexpr int EGO_PLAN_W = 8;
__global__ __launch_bounds__(256) void egonet_walk_plan_kernel(const int* __restrict__ rowptr_in, const int* __restrict__ col_src,
                                                               const int* __restrict__ rowptr_out, const int* __restrict__ col_dst,
                                                               const int* __restrict__ pos_out, const int* __restrict__ goff, const int G,
                                                               int* __restrict__ plan) {
    const int g = (int)(((long long)blockIdx.x * 256 + threadIdx.x) >> 6), l = threadIdx.x & 63;
    if (g >= G) return;
    const int o = goff[g], n = goff[g + 1] - o;
    auto put = [&](int p, int node, int flags, int ps, int ph, int hub) {
        int4* q = reinterpret_cast<int4*>(plan + (long long)p * EGO_PLAN_W);
        q[0] = make_int4(node, flags, ps, ph);
        q[1] = make_int4(hub, o, 0, 0);
    };
    if (n > EGO_MAXN) {                                             // never walked from registers: list position = node
        for (int i = l; i < n; i += 64) put(o + i, o + i, EGO_SKIP, 0, 0, -1);
        return;
    }
    if (n == 0) return;
    const bool act = l < n;
    const int v = o + (act ? l : 0);
    const int e0 = rowptr_out[v], d = act ? rowptr_out[v + 1] - e0 : 0;
    int tgt = -1;
    if (d == 2) { const int d0 = col_dst[e0], d1 = col_dst[e0 + 1]; tgt = ((d0 == v) ? d1 : d0) - o; }
    // the hub: THE node of out-degree >= 3, else the target of the first node of out-degree 2, else node 0 of a single-node graph
    const unsigned long long mbig = __ballot(d >= 3), m2 = __ballot(d == 2);
    int h = -1;
    if (mbig != 0ull) h = __ffsll((long long)mbig) - 1;
    else if (m2 != 0ull) h = __shfl(tgt, __ffsll((long long)m2) - 1, 64);
    else if (n == 1) h = 0;
    bool gok = __popcll(mbig) <= 1 && h >= 0 && h < n;
    int role = EGO_SKIP, pself = -1, phub = -1;
    if (gok) {
        const int vh = o + h;
        const int n_post = __popcll(__ballot(act && l != h && d == 1));
        bool ok = true;
        if (act) {
            const int pi0 = rowptr_in[v], din = rowptr_in[v + 1] - pi0;
            if (l == h) {                          // hub: itself in its in-list; out-degree = 1 + #siblings (the siblings check their side)
                role = EGO_HUB;
                for (int q = 0; q < din; ++q) if (col_src[pi0 + q] == v) pself = pi0 + q;
                ok = pself >= 0 && d == 1 + n_post;
                phub = pself;
            } else if (d == 2) {                   // parent: out-list {self, hub}
                role = EGO_PRE;
                const int d0 = col_dst[e0], d1 = col_dst[e0 + 1];
                if (d0 == v && d1 == vh) { pself = pos_out[e0]; phub = pos_out[e0 + 1]; }
                else if (d1 == v && d0 == vh) { pself = pos_out[e0 + 1]; phub = pos_out[e0]; }
                else ok = false;
            } else if (d == 1) {                   // sibling: in-list {hub, self}; its one out-edge is then the self loop
                role = EGO_POST;
                if (din == 2) {
                    const int s0 = col_src[pi0], s1 = col_src[pi0 + 1];
                    if (s0 == v && s1 == vh) { pself = pi0; phub = pi0 + 1; }
                    else if (s1 == v && s0 == vh) { pself = pi0 + 1; phub = pi0; }
                    else ok = false;
                } else ok = false;
            } else ok = false;
        }
        gok = __ballot(act && !ok) == 0ull;
    }
    if (!act) return;
    if (gok) put(o + ((l == h) ? 0 : (l < h ? l + 1 : l)), v, role | 16 | 32, max(pself, 0), max(phub, 0), o + h);
    else put(o + l, v, EGO_SKIP | 32, 0, 0, -1);
}

#ifndef TXE_EGO_OCC
#define TXE_EGO_OCC 3
#endif
#ifndef TXE_EGO_SLOTS
#define TXE_EGO_SLOTS 1
#endif
// REFORM: the X' columns [0, F) of a parent or sibling entry are not loaded but formed again from rows the walk holds anyway -- the node's
// own ft row, the hub's ft row (fth) and the staged coefficients alpha * dropout factor, which are the forward's, bit for bit
// (ego_row_elem, txe_ego_row.h: the expression the forward walk wrote the row with).  Only a hub's row carries information the walk
// does not hold.  Hub and foreign-hub entries, the tail columns [F, Kp) and everything the generic body walks load X' as before.
// The caller vouches that X' columns [0, F) ARE leaky(aggregate(Y), act_slope), stored un-dropped (act_slope 1: no activation).
template <bool MASK, int NI, bool REFORM = false>
__global__ __launch_bounds__(256, (NI >= 3) ? 2 : TXE_EGO_OCC) void gat_fused_bwd_ego_kernel(const FusedBwdArgs a) {
    __shared__ int s_v[4], s_p[4], s_ni[4 * FB_NODES];                         // (the generic body's per-node table; its edge tables are not used)
    __shared__ float s_cn[4], s_g1[4], s_g2[4], s_nf[4 * FB_NODES];
    __shared__ float s_dot[4][4];
    // per list position of the window (+ one entry for a foreign hub, + one skip entry that pads an odd count)
    __shared__ int t_node[FB_NODES + 2], t_role[FB_NODES + 2], t_self[FB_NODES + 2], t_hub[FB_NODES + 2], t_dz[FB_NODES + 2], t_pos[FB_NODES + 2];
    __shared__ float t_cn[FB_NODES + 2], t_g1[FB_NODES + 2], t_g2[FB_NODES + 2];
    // per position and head: alpha' = alpha * dropout factor and the factor itself, of the self loop [0..3] and of the edge with the hub [4..7]
    __shared__ float t_coef[FB_NODES + 2][8], t_fd[FB_NODES + 2][8];
    // per node of the intersecting graphs (staging)
    __shared__ int n_deg[EGO_TAB], n_tgt[EGO_TAB], n_role[EGO_TAB], n_self[EGO_TAB], n_hubp[EGO_TAB];
    __shared__ int g_hub[FB_NODES], g_ok[FB_NODES];
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int Kp = a.Kp;
    float* s_wa = s_dyn;
    float* s_acc = s_dyn + 2 * Kp;
    float* s_dp = s_dyn + 4 * Kp;
    const int tid = threadIdx.x;
    // ---- the window of list positions and the graphs that intersect it ----
    const int u0 = b * a.npw, u1 = min(a.n_nodes, u0 + a.npw), nw = u1 - u0;   // (nw >= 1: the grid has ceil(n / npw) workgroups)
    __shared__ int t_ok[FB_NODES + 2], t_gs[FB_NODES + 2];                     // (with a plan) the position's graph is walked; its first position
    const bool planned = a.plan != nullptr;
    int gF = 0, gL = 0, ng = 0, offF = 0, endL = 0, tb = 0, te = 0;
    if (!planned) {
        gF = a.ggid[u0]; gL = a.ggid[u1 - 1]; ng = gL - gF + 1;                // <= npw <= FB_NODES graphs
        offF = a.goff[gF]; endL = a.goff[gL + 1];
        tb = (a.goff[gF + 1] - offF <= EGO_MAXN) ? offF : u0;                 // first / one-past-last node with a staging entry
        te = (endL - a.goff[gL] <= EGO_MAXN) ? endL : u1;                      // (only the first and the last graph reach outside the window)
    }
    // (with a plan the entries 0..nw are written whole by the staging loop below: no barrier between defaults and values)
    for (int i = tid; i < FB_NODES + 2; i += 256)
        if (!planned || i > nw) { t_node[i] = u0; t_role[i] = EGO_SKIP; t_self[i] = 0; t_hub[i] = 0; t_dz[i] = 0; t_pos[i] = 0; t_cn[i] = 0.f; t_g1[i] = 0.f; t_g2[i] = 0.f; }
    for (int i = tid; i < (FB_NODES + 2) * 8; i += 256)
        if (!planned || (i >> 3) > nw) { t_coef[i >> 3][i & 7] = 0.f; t_fd[i >> 3][i & 7] = 0.f; }
    for (int i = tid; i < a.vocab * a.Pd; i += 256) s_dp[i] = 0.f;
    for (int i = tid * 4; i < 2 * Kp; i += 1024) {
        *reinterpret_cast<float4*>(s_wa + i) = *reinterpret_cast<const float4*>(a.wa + i);
        *reinterpret_cast<float4*>(s_acc + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    bool owes_hpart = false;
    if (planned) {
        // ---- staging from the batch's walk plan: trip 1 = the plan entries (the window's first one with them: does the window start
        //      inside a graph?), trip 2 = the nodes' scalars and the edge coefficients; one barrier ----
        const int4 p0 = *reinterpret_cast<const int4*>(a.plan + (long long)u0 * EGO_PLAN_W);
        const int4 p0b = *reinterpret_cast<const int4*>(a.plan + (long long)u0 * EGO_PLAN_W + 4);
        for (int i = tid; i < (nw + 1) * 8; i += 256) {
            const int t = i >> 3, e = (i >> 2) & 1, hd = i & 3;
            const long long pp = (long long)(u0 + (t < nw ? t : 0)) * EGO_PLAN_W;
            const int4 q = *reinterpret_cast<const int4*>(a.plan + pp);
            const int4 qb = *reinterpret_cast<const int4*>(a.plan + pp + 4);
            const bool foreign = p0b.y < u0 && (p0.y & 16) != 0;               // the window starts inside a graph that is walked
            const int role = (t < nw) ? (q.y & 15) : (foreign ? EGO_FOREIGN : EGO_SKIP);
            const int v = (role == EGO_SKIP) ? u0 : ((t < nw) ? q.x : qb.x);
            float fd = 0.f, cf = 0.f;
            if (role != EGO_SKIP) {
                const long long idx = (long long)(e ? q.w : q.z) * a.H + hd;   // (a foreign hub's coefficients are never used)
                fd = (a.drop_p > 0.f) ? drop_factor(a.seed, (unsigned long long)idx, a.drop_p, a.drop_scale) : 1.f;
                cf = (t < nw) ? a.alpha[idx] * fd : 0.f;
            }
            t_fd[t][i & 7] = fd;
            t_coef[t][i & 7] = cf;
            if ((i & 7) == 0) {
                const bool live = role != EGO_SKIP;
                t_ok[t] = (q.y >> 4) & 1; t_gs[t] = qb.y;
                t_node[t] = v; t_role[t] = role; t_self[t] = live ? q.z : 0; t_hub[t] = live ? q.w : 0;
                t_dz[t] = live ? a.gid[v] : 0; t_pos[t] = live ? a.pos[v] : 0;
                t_cn[t] = live ? a.cn[v] : 0.f; t_g1[t] = live ? a.da1[v] : 0.f; t_g2[t] = live ? a.da2[v] : 0.f;
            }
        }
        owes_hpart = p0b.y < u0 && (p0.y & 32) != 0;                           // (a graph of at most EGO_MAXN nodes, walked or not)
        __syncthreads();
    } else {
    if (ng > FB_NODES) {
        // more graphs than positions in the window: it holds EMPTY graphs (an egonet has at least its anchor) -- not a batch of egonets;
        // every source node of the window through the generic body, and the row a fix-up pass may read cleared
        __syncthreads();
        if (tid < nw) {
            const int u = u0 + tid;
            s_ni[4 * tid] = a.gid[u]; s_ni[4 * tid + 1] = a.rowptr_out[u]; s_ni[4 * tid + 2] = a.rowptr_out[u + 1];
            s_ni[4 * tid + 3] = a.pos[u];
            s_nf[4 * tid] = a.da1[u]; s_nf[4 * tid + 1] = a.da2[u]; s_nf[4 * tid + 2] = a.cn[u];
        }
        __syncthreads();
        const int e0 = a.rowptr_out[u0], ne = a.rowptr_out[u1] - e0;
        fb_body<MASK, NI, 1, false>(a, b, u0, u1, e0, ne, s_v, s_p, s_cn, s_g1, s_g2, s_ni, s_nf, s_dot, s_dp, s_wa, s_acc);
        if (u0 > offF && a.goff[gF + 1] - offF <= EGO_MAXN)
            for (int c = tid; c < a.H * a.D; c += 256) a.hpart[(long long)b * a.H * a.D + c] = 0.f;
        __syncthreads();
        float* dwg = a.dwa_part + (long long)b * 2 * Kp;
        for (int i = tid * 4; i < 2 * Kp; i += 1024) *reinterpret_cast<float4*>(dwg + i) = *reinterpret_cast<const float4*>(s_acc + i);
        for (int i = tid; i < a.vocab * a.Pd; i += 256) a.ppart[(long long)b * a.vocab * a.Pd + i] = s_dp[i];
        return;
    }
    if (tid < ng) { g_ok[tid] = (a.goff[gF + tid + 1] - a.goff[gF + tid] <= EGO_MAXN) ? 1 : 0; g_hub[tid] = 0; }
    __syncthreads();
    // (1) out-degree, and the non-self target of a node of out-degree 2 -- one thread per node of the graphs that fit
    int my_g = -1, my_i = 0, my_n = 0, my_v = 0, my_base = 0;
    if (tid < te - tb) {
        const int v = tb + tid, g = a.ggid[v];
        if (g_ok[g - gF]) { my_g = g - gF; my_base = a.goff[g] - tb; my_i = v - a.goff[g]; my_n = a.goff[g + 1] - a.goff[g]; my_v = v; }
    }
    if (my_g >= 0) {
        const int e0 = a.rowptr_out[my_v], d = a.rowptr_out[my_v + 1] - e0;
        n_deg[tid] = d;
        int tgt = -1;
        if (d == 2) { const int d0 = a.col_dst[e0], d1 = a.col_dst[e0 + 1]; tgt = (d0 == my_v) ? d1 : d0; }
        n_tgt[tid] = tgt - (tb + my_base);                                 // local index inside the graph (or out of range)
    }
    __syncthreads();
    // (2) the hub of every graph: THE node of out-degree >= 3, else the target of the first node of out-degree 2, else node 0 of a
    //     single-node graph
    if (tid < ng && g_ok[tid]) {
        const int base = a.goff[gF + tid] - tb, n = a.goff[gF + tid + 1] - a.goff[gF + tid];
        int h = -1, big = 0;
        for (int i = 0; i < n; ++i) if (n_deg[base + i] >= 3) { h = i; ++big; }
        if (big == 0) {
            for (int i = 0; i < n && h < 0; ++i) if (n_deg[base + i] == 2) h = n_tgt[base + i];
            if (h < 0) h = (n == 1) ? 0 : -1;
        }
        if (big > 1 || h < 0 || h >= n) g_ok[tid] = 0; else g_hub[tid] = h;
    }
    __syncthreads();
    // (3) every node against the hub shape; its role and the destination-CSR positions of its self loop and of its edge with the hub
    if (my_g >= 0 && g_ok[my_g]) {
        const int h = g_hub[my_g], vh = tb + my_base + h, d = n_deg[tid];
        const int pi0 = a.rowptr_in[my_v], din = a.rowptr_in[my_v + 1] - pi0;
        int role = EGO_SKIP, pself = -1, phub = -1;
        bool ok = true;
        if (my_i == h) {                       // hub: itself in its in-list; out-degree = 1 + #siblings (the siblings check their side)
            role = EGO_HUB;
            for (int q = 0; q < din; ++q) if (a.col_src[pi0 + q] == my_v) pself = pi0 + q;
            int n_post = 0;
            for (int i = 0; i < my_n; ++i) n_post += (i != h && n_deg[my_base + i] == 1) ? 1 : 0;
            ok = pself >= 0 && d == 1 + n_post;
            phub = pself;
        } else if (d == 2) {                   // parent: out-list {self, hub}
            role = EGO_PRE;
            const int e0 = a.rowptr_out[my_v];
            const int d0 = a.col_dst[e0], d1 = a.col_dst[e0 + 1];
            if (d0 == my_v && d1 == vh) { pself = a.pos_out[e0]; phub = a.pos_out[e0 + 1]; }
            else if (d1 == my_v && d0 == vh) { pself = a.pos_out[e0 + 1]; phub = a.pos_out[e0]; }
            else ok = false;
        } else if (d == 1) {                   // sibling: in-list {hub, self}; its one out-edge is then the self loop
            role = EGO_POST;
            if (din == 2) {
                const int s0 = a.col_src[pi0], s1 = a.col_src[pi0 + 1];
                if (s0 == my_v && s1 == vh) { pself = pi0; phub = pi0 + 1; }
                else if (s1 == my_v && s0 == vh) { pself = pi0 + 1; phub = pi0; }
                else ok = false;
            } else ok = false;
        } else ok = false;
        if (!ok) g_ok[my_g] = 0;                 // (benign race: every writer stores 0)
        n_role[tid] = role; n_self[tid] = max(pself, 0); n_hubp[tid] = max(phub, 0);
    }
    __syncthreads();
    // (4) the window's list positions -> table entries; entry nw: the hub of a graph whose list the window enters in the middle
    if (tid <= nw) {
        int v = -1, role = EGO_SKIP, idx = 0;
        if (tid < nw) {
            const int p = u0 + tid, g = a.ggid[p];
            if (g_ok[g - gF]) { v = a.goff[g] + ego_node_of(p - a.goff[g], g_hub[g - gF]); idx = v - tb; role = n_role[idx]; }
        } else if (g_ok[0] && u0 > offF) { v = offF + g_hub[0]; idx = v - tb; role = EGO_FOREIGN; }
        if (v >= 0) {
            t_node[tid] = v; t_role[tid] = role; t_self[tid] = n_self[idx]; t_hub[tid] = n_hubp[idx];
            t_dz[tid] = a.gid[v]; t_pos[tid] = a.pos[v];
            t_cn[tid] = a.cn[v]; t_g1[tid] = a.da1[v]; t_g2[tid] = a.da2[v];
        }
    }
    __syncthreads();
    // (5) the edge scalars of every (position, edge, head): one thread each -- the walk reads them from LDS
    for (int i = tid; i < (nw + 1) * 8; i += 256) {
        const int t = i >> 3, e = (i >> 2) & 1, hd = i & 3;
        if (t_role[t] != EGO_SKIP) {
            const long long idx = (long long)(e ? t_hub[t] : t_self[t]) * a.H + hd;
            const float fd = (a.drop_p > 0.f) ? drop_factor(a.seed, (unsigned long long)idx, a.drop_p, a.drop_scale) : 1.f;
            t_fd[t][i & 7] = fd;
            t_coef[t][i & 7] = a.alpha[idx] * fd;
        }
    }
    __syncthreads();

    }   // (!planned)

    const int w = uni((int)(tid >> 6)), l = tid & 63;
    const int F = a.H * a.D, SL = F >> 2, nvec = SL >> 2;
    const int c0 = w * SL, hw = c0 / a.D;
    int off[NI];
    float live[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int j = l + 64 * i;
        off[i] = c0 + 4 * ((j < nvec) ? j : 0);
        live[i] = (j < nvec) ? 1.f : 0.f;
    }
    const int tvec = (Kp - F) >> 2;
    const bool tail = (w == 0) && (l < tvec);
    const int tc = min(F + 4 * (tail ? l : 0), Kp - 4);
    float fth[NI][4], pph[NI][4], acch[NI][4];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) { fth[i][k] = 0.f; pph[i][k] = 0.f; acch[i][k] = 0.f; }
    int hub_node = -1;                           // the hub whose slices are in registers; hub_home: its d_ft goes to d_Y (else to hpart[b])
    bool hub_home = true;
    // a window that starts inside a graph of <= EGO_MAXN nodes owes the fix-up pass a row hpart[b]: its share of the hub's d_ft, or
    // zeros if the graph turned out not to be hub-shaped (fused_hub_fixup_job repeats only the cheap half of the shape check)
    if (!planned) owes_hpart = u0 > offF && (a.goff[gF + 1] - offF <= EGO_MAXN);
    bool paid_hpart = false;
    auto flush_hub = [&]() {
        if (hub_node >= 0) {
            if (!hub_home) paid_hpart = true;
            float* dst = hub_home ? a.d_Y + (long long)hub_node * a.ld_dy : a.hpart + (long long)b * F;
#pragma unroll
            for (int i = 0; i < NI; ++i)
                if (l + 64 * i < nvec) vstore<4>(dst + off[i], acch[i]);
        }
    };

    // the walk, NS entries per round trip: entry nw first if it is a foreign hub, then the positions
    // (REFORM: two entries per trip pay once most entries ask for two rows instead of three -- rows of 2,048 columns 101 -> 94 us with
    //  168 VGPRs and 4 of them spilled; loading walk: two entries spilled 10-37 and lost, DESIGN 4.3.  NI >= 3 not measured: one entry)
    constexpr int NS = (REFORM && NI <= 2) ? 2 : TXE_EGO_SLOTS;
    for (int t0 = (t_role[nw] == EGO_FOREIGN) ? -1 : 0; t0 < nw; t0 += NS) {
        // ---- every load of the two entries first (rows, masks, edge scalars), nothing in between ----
        int vv[NS], role[NS], ps[NS], ph[NS], pv[NS];
        float cnv[NS], g1v[NS], g2v[NS], cfs[NS], fds[NS], cfh[NS], fdh2[NS];
        float ft[NS][NI][4], xv[NS][NI][4], dz[NS][NI][4], xt[NS][4], dzt[NS][4];
        unsigned mv[NS][NI], mt[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            const int t = (t0 + q < 0) ? nw : ((t0 + q < nw) ? t0 + q : FB_NODES + 1);     // (FB_NODES + 1: an entry that stays EGO_SKIP)
            vv[q] = uni(t_node[t]); role[q] = uni(t_role[t]); ps[q] = uni(t_self[t]); ph[q] = uni(t_hub[t]); pv[q] = t_pos[t];
            cnv[q] = uni(t_cn[t]); g1v[q] = uni(t_g1[t]); g2v[q] = uni(t_g2[t]);
            const int dzr = uni(t_dz[t]);
            cfs[q] = uni(t_coef[t][hw]); fds[q] = uni(t_fd[t][hw]); cfh[q] = uni(t_coef[t][4 + hw]); fdh2[q] = uni(t_fd[t][4 + hw]);
            if constexpr (REFORM) {
                // a hub's X' row only (wave-uniform branch, and the FIRST load of the entry: every load behind the merge is counted
                // alike on both sides, so the waits for them stay exact)
                if (role[q] == EGO_HUB || role[q] == EGO_FOREIGN) {
#pragma unroll
                    for (int i = 0; i < NI; ++i) vload<4>(a.X + (long long)vv[q] * Kp + off[i], xv[q][i]);
                } else {
#pragma unroll
                    for (int i = 0; i < NI; ++i)
#pragma unroll
                        for (int k = 0; k < 4; ++k) xv[q][i][k] = 0.f;
                }
            }
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                vload<4>(a.Y + (long long)vv[q] * a.ld_y + off[i], ft[q][i]);
                if constexpr (!REFORM) vload<4>(a.X + (long long)vv[q] * Kp + off[i], xv[q][i]);
                vload<4>(a.dZ + (long long)dzr * Kp + off[i], dz[q][i]);
                mv[q][i] = fb_keep<MASK>(a.mask, a.mask_ld, vv[q], off[i]);
            }
            vload<4>(a.X + (long long)vv[q] * Kp + tc, xt[q]);
            vload<4>(a.dZ + (long long)dzr * Kp + tc, dzt[q]);
            mt[q] = fb_keep<MASK>(a.mask, a.mask_ld, vv[q], tc);
        }
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            if (role[q] == EGO_SKIP) continue;                        // (wave-uniform)
            const int v = vv[q];
            const bool own = role[q] != EGO_FOREIGN;                  // a foreign hub: d_pre and ft only -- its own-row work belongs to its home
            const float sc = cnv[q] * a.fscale, s1 = g1v[q] * a.fscale, s2 = g2v[q] * a.fscale;
            float dp[NI][4], acc[NI][4];
            const float fd = fds[q], coef = cfs[q];
            const float go1 = own ? g1v[q] : 0.f, go2 = own ? g2v[q] : 0.f;
            float part = 0.f;
            if constexpr (REFORM) {
                if (role[q] == EGO_PRE || role[q] == EGO_POST) {          // (wave-uniform) the row the forward stored, formed again
                    const bool sib = role[q] == EGO_POST;
                    // a sibling's in-list is [hub, self] -- or [self, hub]: one wave per node summed it in that order
                    const bool swp = sib && ps[q] < ph[q];
                    const float ca = swp ? cfh[q] : cfs[q], cb = swp ? cfs[q] : cfh[q];
#pragma unroll
                    for (int i = 0; i < NI; ++i)
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const float ya = swp ? fth[i][k] : ft[q][i][k], yb = swp ? ft[q][i][k] : fth[i][k];
                            xv[q][i][k] = ego_row_elem(ca, ya, sib, cb, yb, false, 0.f, true, a.act_slope);
                        }
                }
            }
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                float w1[4], w2[4], a1[4], a2[4];
                vload<4>(s_wa + off[i], w1);
                vload<4>(s_wa + Kp + off[i], w2);
                vload<4>(s_acc + off[i], a1);
                vload<4>(s_acc + Kp + off[i], a2);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool keep = ((mv[q][i] >> k) & 1u) != 0u;
                    const float tv = sc * dz[q][i][k] + s1 * w1[k] + s2 * w2[k];
                    const float lk = (xv[q][i][k] > 0.f) ? live[i] : a.act_slope * live[i];
                    dp[i][k] = keep ? tv * lk : 0.f;
                    part = fmaf(dp[i][k], ft[q][i][k], part);
                    acc[i][k] = coef * dp[i][k];
                    const float xd = keep ? xv[q][i][k] * a.fscale * live[i] : 0.f;       // own-row leftovers of cl_bwd_dx: d_wa partials
                    a1[k] = fmaf(go1, xd, a1[k]);
                    a2[k] = fmaf(go2, xd, a2[k]);
                }
                if (l + 64 * i < nvec) { vstore<4>(s_acc + off[i], a1); vstore<4>(s_acc + Kp + off[i], a2); }
            }
            if (tail && own) {
                float a1[4], a2[4], wt1[4], wt2[4];
                vload<4>(s_acc + tc, a1);
                vload<4>(s_acc + Kp + tc, a2);
                vload<4>(s_wa + tc, wt1);
                vload<4>(s_wa + Kp + tc, wt2);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool keep = ((mt[q] >> k) & 1u) != 0u;
                    const float xd = keep ? xt[q][k] * a.fscale : 0.f;
                    a1[k] = fmaf(g1v[q], xd, a1[k]);
                    a2[k] = fmaf(g2v[q], xd, a2[k]);
                    const int pc = tc + k - a.Kh;                      // position column (d_X' there has no activation factor)
                    if (pc >= 0 && pc < a.Pd) s_dp[pv[q] * a.Pd + pc] += keep ? a.fscale * (cnv[q] * dzt[q][k] + g1v[q] * wt1[k] + g2v[q] * wt2[k]) : 0.f;
                }
                vstore<4>(s_acc + tc, a1);
                vstore<4>(s_acc + Kp + tc, a2);
            }
            if (own) {
                part = wave_sum(part);
                if (l == 0) a.dal[(long long)ps[q] * a.H + hw] = part * fd;           // the self loop's raw d alpha
            }
            if (role[q] == EGO_HUB || role[q] == EGO_FOREIGN) {
                flush_hub();
                hub_node = v; hub_home = own;
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int k = 0; k < 4; ++k) { fth[i][k] = ft[q][i][k]; pph[i][k] = dp[i][k]; acch[i][k] = own ? acc[i][k] : 0.f; }
            } else {
                const float fdh = fdh2[q], coefh = cfh[q];
                float part2 = 0.f;
                if (role[q] == EGO_PRE) {          // edge v -> hub: d_pre[hub] against this node's ft, accumulated into this node's d_ft
#pragma unroll
                    for (int i = 0; i < NI; ++i)
#pragma unroll
                        for (int k = 0; k < 4; ++k) { part2 = fmaf(pph[i][k], ft[q][i][k], part2); acc[i][k] = fmaf(coefh, pph[i][k], acc[i][k]); }
                } else {                           // edge hub -> v: this node's d_pre against the hub's ft, accumulated into the hub's d_ft
#pragma unroll
                    for (int i = 0; i < NI; ++i)
#pragma unroll
                        for (int k = 0; k < 4; ++k) { part2 = fmaf(dp[i][k], fth[i][k], part2); acch[i][k] = fmaf(coefh, dp[i][k], acch[i][k]); }
                }
                part2 = wave_sum(part2);
                if (l == 0) a.dal[(long long)ph[q] * a.H + hw] = part2 * fdh;
#pragma unroll
                for (int i = 0; i < NI; ++i)
                    if (l + 64 * i < nvec) vstore<4>(a.d_Y + (long long)v * a.ld_dy + off[i], acc[i]);
            }
        }
    }
    flush_hub();
    if (owes_hpart && !paid_hpart) {
        const float z[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (l + 64 * i < nvec) vstore<4>(a.hpart + (long long)b * F + off[i], z);
    }
    // ---- graphs that are not hub-shaped (or too large): the generic body over their source nodes inside the window ----
    for (int gi = 0, tp = 0; planned ? tp < nw : gi < ng; ++gi) {
        int c, cu1;
        if (planned) {                                               // the next stretch of positions of ONE graph that is not walked
            if (t_ok[tp]) { ++tp; continue; }                        // (LDS values: the same for every thread)
            const int gs = t_gs[tp];
            c = u0 + tp;
            while (tp < nw && !t_ok[tp] && t_gs[tp] == gs) ++tp;
            cu1 = u0 + tp;
        } else {
        if (g_ok[gi]) continue;                                      // (LDS value: the same for every thread)
        c = max(u0, a.goff[gF + gi]); cu1 = min(u1, a.goff[gF + gi + 1]);
        }
        __syncthreads();
        if (tid < cu1 - c) {
            const int u = c + tid;
            s_ni[4 * tid] = a.gid[u]; s_ni[4 * tid + 1] = a.rowptr_out[u]; s_ni[4 * tid + 2] = a.rowptr_out[u + 1];
            s_ni[4 * tid + 3] = a.pos[u];
            s_nf[4 * tid] = a.da1[u]; s_nf[4 * tid + 1] = a.da2[u]; s_nf[4 * tid + 2] = a.cn[u];
        }
        __syncthreads();
        const int e0 = a.rowptr_out[c], ne = a.rowptr_out[cu1] - e0;
        fb_body<MASK, NI, 1, false>(a, b, c, cu1, e0, ne, s_v, s_p, s_cn, s_g1, s_g2, s_ni, s_nf, s_dot, s_dp, s_wa, s_acc);
    }
    __syncthreads();
    float* dw = a.dwa_part + (long long)b * 2 * Kp;
    for (int i = tid * 4; i < 2 * Kp; i += 1024) *reinterpret_cast<float4*>(dw + i) = *reinterpret_cast<const float4*>(s_acc + i);
    for (int i = tid; i < a.vocab * a.Pd; i += 256) a.ppart[(long long)b * a.vocab * a.Pd + i] = s_dp[i];
}

// A hub-shaped graph cut by workgroup boundaries of the walk above: d_Y[hub] (written by the hub's home workgroup) += the later
// workgroups' shares, in workgroup order.  Block j stands for the boundary in front of window j; it acts only if that boundary cuts a
// graph whose hub lives in window j - 1... or earlier but this is the FIRST boundary inside the graph -- every cut graph is fixed once.
struct HubFixArgs { const int *goff, *ggid, *rowptr_out, *col_dst; int n_nodes, npw, nblocks, F; const float* hpart; float* d_Y; long long ld_dy; };
__device__ __forceinline__ void fused_hub_fixup_job(const int j, const HubFixArgs& a) {
    const int p = j * a.npw;                                         // first list position of window j (1 <= j < nblocks)
    const int g = a.ggid[p], o = a.goff[g], n = a.goff[g + 1] - o;
    if (o == p || n > EGO_MAXN) return;                              // no graph is cut here / never hub-walked
    const int bh = o / a.npw;                                        // home window of the hub (list position o)
    if (j != bh + 1) return;                                         // (the first boundary inside the graph does the whole job)
    // the graph's hub and whether it was hub-walked at all: the same rule as the sweep (out-degrees; the full shape check is repeated
    // cheaply: a graph that failed there wrote no hpart rows and must not be touched -- recompute the verdict)
    __shared__ int s_h, s_ok;
    if (threadIdx.x == 0) {
        int h = -1, big = 0;
        for (int i = 0; i < n; ++i) if (a.rowptr_out[o + i + 1] - a.rowptr_out[o + i] >= 3) { h = i; ++big; }
        if (big == 0) {
            for (int i = 0; i < n && h < 0; ++i) {
                const int e0 = a.rowptr_out[o + i];
                if (a.rowptr_out[o + i + 1] - e0 == 2) { const int d0 = a.col_dst[e0], d1 = a.col_dst[e0 + 1]; h = ((d0 == o + i) ? d1 : d0) - o; }
            }
            if (h < 0) h = (n == 1) ? 0 : -1;
        }
        s_h = h; s_ok = (big <= 1 && h >= 0 && h < n) ? 1 : 0;
    }
    __syncthreads();
    if (!s_ok) return;
    const int bl = (o + n - 1) / a.npw;
    float* dst = a.d_Y + (long long)(o + s_h) * a.ld_dy;
    for (int c = threadIdx.x; c < a.F; c += 256) {
        float v = dst[c];
        for (int bb = bh + 1; bb <= bl; ++bb) v += a.hpart[(long long)bb * a.F + c];
        dst[c] = v;
    }
}

// Softmax + leaky-relu backward of a GATLayer's attention from the raw d alpha of the fused sweep, edge level:
//   dz_p = alpha_p (dal_p - sum_q alpha_q dal_q) leaky'(a_src[u_p] + a_dst[v]);  d a_dst[v] = sum_in dz;  d a_src[u] = sum_out dz
// written into the a1 / a2 columns of d_Y (and zeros into its padding columns).  A workgroup owns FA_GRAPHS consecutive graphs:
// the edges of a batched graph stay inside it, so the destination-side and source-side halves only need a workgroup barrier.
constexpr int FA_GRAPHS = 8;
constexpr int FA_LIGHT = 8;         // degrees up to this are walked by one thread per (node, head); heavier nodes by a whole wave
struct AttnBwdArgs {
    const int *rowptr_in, *col_src, *rowptr_out, *pos_out, *graph_off;
    int G;
    const float* Y; long long ld_y; int H, F; float slope;
    const float *alpha, *dal;
    float *dz, *d_Y; long long ld_dy; int n_pad;
};
__device__ __forceinline__ void gat_attn_bwd_job(const int bid, const AttnBwdArgs& a) {
    const int* __restrict__ rowptr_in = a.rowptr_in; const int* __restrict__ col_src = a.col_src;
    const int* __restrict__ rowptr_out = a.rowptr_out; const int* __restrict__ pos_out = a.pos_out;
    const int* __restrict__ graph_off = a.graph_off; const int G = a.G;
    const float* __restrict__ Y = a.Y; const long long ld_y = a.ld_y; const int H = a.H, F = a.F; const float slope = a.slope;
    const float* __restrict__ alpha = a.alpha; const float* __restrict__ dal = a.dal;
    float* __restrict__ dz = a.dz; float* __restrict__ d_Y = a.d_Y; const long long ld_dy = a.ld_dy; const int n_pad = a.n_pad;
    __shared__ int s_heavy[2][256], s_nh[2];                        // heavy destinations / sources found by the light passes
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int g0 = bid * FA_GRAPHS, g1 = min(G, g0 + FA_GRAPHS);
    const int n0 = graph_off[g0], n1 = graph_off[g1];
    const int nn = n1 - n0;
    if (threadIdx.x < 2) s_nh[threadIdx.x] = 0;
    __syncthreads();
    // ---- destination side ----
    for (int t = threadIdx.x; t < nn * H; t += 256) {               // light nodes: one thread per (node, head)
        const int v = n0 + t / H, h = t % H;
        const int beg = rowptr_in[v], end = rowptr_in[v + 1];
        if (end - beg > FA_LIGHT) {
            if (h == 0) { const int k = atomicAdd(&s_nh[0], 1); if (k < 256) s_heavy[0][k] = v; }
            continue;
        }
        const float ad = Y[(long long)v * ld_y + F + H + h];
        float al[FA_LIGHT], dl[FA_LIGHT], zs[FA_LIGHT];
#pragma unroll
        for (int i = 0; i < FA_LIGHT; ++i) {                        // clamped, unconditional: all loads of the node go out together
            const int p = min(beg + i, max(end - 1, beg));
            const bool ok = beg + i < end;
            al[i] = ok ? alpha[(long long)p * H + h] : 0.f;
            dl[i] = ok ? dal[(long long)p * H + h] : 0.f;
            zs[i] = ok ? Y[(long long)col_src[p] * ld_y + F + h] : 0.f;
        }
        float S = 0.f, accv = 0.f;
#pragma unroll
        for (int i = 0; i < FA_LIGHT; ++i) S = fmaf(al[i], dl[i], S);
#pragma unroll
        for (int i = 0; i < FA_LIGHT; ++i) {
            const float gz = al[i] * (dl[i] - S) * ((zs[i] + ad > 0.f) ? 1.f : slope);
            if (beg + i < end) dz[(long long)(beg + i) * H + h] = gz;
            accv += (beg + i < end) ? gz : 0.f;
        }
        d_Y[(long long)v * ld_dy + F + H + h] = accv;
    }
    for (int t = threadIdx.x; t < nn * n_pad; t += 256) d_Y[(long long)(n0 + t / n_pad) * ld_dy + F + 2 * H + t % n_pad] = 0.f;
    __syncthreads();
    const bool list_a = s_nh[0] <= 256;                             // (more heavy nodes than the list holds: scan the node range)
    for (int i = w; i < (list_a ? s_nh[0] : nn); i += 4) {          // heavy nodes: one wave each, lanes over the in-edges
        const int v = list_a ? s_heavy[0][i] : n0 + i;
        const int beg = rowptr_in[v], end = rowptr_in[v + 1];
        if (end - beg <= FA_LIGHT) continue;                        // (wave-uniform)
        for (int h = 0; h < H; ++h) {
            const float ad = Y[(long long)v * ld_y + F + H + h];
            float S = 0.f;
            for (int p = beg + l; p < end; p += 64) S = fmaf(alpha[(long long)p * H + h], dal[(long long)p * H + h], S);
            S = wave_sum(S);
            float accv = 0.f;
            for (int p = beg + l; p < end; p += 64) {
                const float de = alpha[(long long)p * H + h] * (dal[(long long)p * H + h] - S);
                const float z = Y[(long long)col_src[p] * ld_y + F + h] + ad;
                const float gz = de * (z > 0.f ? 1.f : slope);
                dz[(long long)p * H + h] = gz;
                accv += gz;
            }
            accv = wave_sum(accv);
            if (l == 0) d_Y[(long long)v * ld_dy + F + H + h] = accv;
        }
    }
    __syncthreads();                                               // dz of this workgroup's edges is complete (first touched below)
    // ---- source side ----
    for (int t = threadIdx.x; t < nn * H; t += 256) {
        const int u = n0 + t / H, h = t % H;
        const int beg = rowptr_out[u], end = rowptr_out[u + 1];
        if (end - beg > FA_LIGHT) {
            if (h == 0) { const int k = atomicAdd(&s_nh[1], 1); if (k < 256) s_heavy[1][k] = u; }
            continue;
        }
        float accu = 0.f;
#pragma unroll
        for (int i = 0; i < FA_LIGHT; ++i) {
            const int j = min(beg + i, max(end - 1, beg));
            accu += (beg + i < end) ? dz[(long long)pos_out[j] * H + h] : 0.f;
        }
        d_Y[(long long)u * ld_dy + F + h] = accu;
    }
    __syncthreads();
    const bool list_b = s_nh[1] <= 256;
    for (int i = w; i < (list_b ? s_nh[1] : nn); i += 4) {
        const int u = list_b ? s_heavy[1][i] : n0 + i;
        const int beg = rowptr_out[u], end = rowptr_out[u + 1];
        if (end - beg <= FA_LIGHT) continue;
        for (int h = 0; h < H; ++h) {
            float accu = 0.f;
            for (int j = beg + l; j < end; j += 64) accu += dz[(long long)pos_out[j] * H + h];
            accu = wave_sum(accu);
            if (l == 0) d_Y[(long long)u * ld_dy + F + h] = accu;
        }
    }
}
// The attention backward of the layer below and stage 1 of the folded layer's reductions depend on the fused sweep only, not on each
// other: one launch, the first nb_attn workgroups do the former.
// ... and (after the egonet-walking sweep) the hubs of graphs cut by its window boundaries: nb_fix = windows - 1 more workgroups.
__global__ __launch_bounds__(256) void gat_attn_bwd_reduce_a_kernel(const AttnBwdArgs aa, const int nb_attn, const TailA a, const HubFixArgs hf,
                                                                    const int nb_fix) {
    // (the fix-up workgroups LAST: almost all of them return after two loads, and in front of the grid they delayed the real jobs by a
    //  dispatch round: 27.9 -> 22.1 us by HIP events)
    const int bid = (int)blockIdx.x, nb_main = (int)gridDim.x - nb_fix;
    if (bid >= nb_main) { fused_hub_fixup_job(bid - nb_main + 1, hf); return; }
    if (bid < nb_attn) { gat_attn_bwd_job(bid, aa); return; }
    reduce_a_job(bid - nb_attn, a);
}

// phases | TXE_FUSED_DW_BESIDE of the folded layer's backward entries: the weight-gradient product runs on a second stream BESIDE the caller's dZ product
// and sweeps (every call of one backward pass carries the bit: the workspace layout depends on it).  Few fat k-slices then -- 2 instead
// of the 7 that fill the machine: ~140 workgroups leave the kernels on the caller's stream their wave slots (cl_bwd_dot 73 -> 61 us,
// step -11 us on the 4,096-egonet batch) and the product still ends under the fused sweep (one slice: it does not -- sweep 139 -> 204 us)
constexpr int DW_BESIDE_SPLITS = 2;
struct FusedWs {
    CollapseWs c;
    float *dal, *dwa_part, *ppart, *hpart;
    int nblocks, npw;
    size_t total;
};
static FusedWs plan_fused_ws(void* ws, int n, int e, int G, int Kh, int Kp, int D, int Pd, int vocab, int Hp, int max_splits = 0) {
    FusedWs f;
    f.c = plan_collapse_ws(ws, n, e, G, Kp, D, Pd, vocab, max_splits);
    char* b = (char*)ws;
    size_t off = f.c.total;
    auto take = [&](size_t bytes) { float* r = (float*)(b + off); off += align_up(bytes > 0 ? bytes : 4, 256); return r; };
    f.npw = fb_nodes_per_wg(n, (Kh > 2048) ? 2 : 3);                // (rows of more than 2,048 feature columns: NI >= 3, two workgroups per CU)
    f.nblocks = (n + f.npw - 1) / f.npw;
    const int nb1 = f.nblocks > 0 ? f.nblocks : 1;
    f.dal = take((size_t)(e > 0 ? e : 1) * Hp * 4);
    f.dwa_part = take((size_t)nb1 * 2 * Kp * 4);
    f.ppart = take((size_t)nb1 * (vocab > 0 ? vocab : 1) * (Pd > 0 ? Pd : 1) * 4);
    f.hpart = take(Hp == 4 ? (size_t)nb1 * Kp * 4 : 4);             // (the egonet walk: H*D = Kh <= Kp floats per window)
    f.total = off;
    return f;
}
}  // namespace txe
using namespace txe;

extern "C" {

// The walk plan of a batch of graphs for the egonet-walking sweeps (egonet_walk_plan_kernel): 8 ints per node.
size_t txe_egonet_walk_plan_bytes(int n_nodes) { return (size_t)(n_nodes > 0 ? n_nodes : 1) * EGO_PLAN_W * sizeof(int); }
int txe_egonet_walk_plan(const int* rowptr_in, const int* col_src, const int* rowptr_out, const int* col_dst, const int* pos_out,
                         const int* graph_off, int n_nodes, int G, int* plan, void* stream) {
    if (n_nodes < 0 || G < 0 || !plan || (n_nodes > 0 && (!rowptr_in || !col_src || !rowptr_out || !col_dst || !pos_out || !graph_off))) return TXE_ERR_ARG;
    if (((uintptr_t)plan & 15) != 0) return TXE_ERR_ARG;
    if (n_nodes == 0 || G == 0) return TXE_OK;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("egonet_walk_plan_kernel", s, 4.0 * (6.0 * n_nodes + EGO_PLAN_W * (double)n_nodes), 1);
    hipLaunchKernelGGL(egonet_walk_plan_kernel, dim3((G + 3) / 4), dim3(256), 0, s, rowptr_in, col_src, rowptr_out, col_dst, pos_out, graph_off, G, plan);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

// 1 when txe_gat_collapse_bwd_fused supports the shape: the previous layer has 1, 2 or 4 heads, its H*D columns are a multiple of 16
// and at most 4096, and the folded layer's input has at most 128 columns behind them.
int txe_gat_fused_bwd_supported(int Kh, int Pd, int Hp, int Dp) {
    const int F = Hp * Dp, Kp = round_up(Kh + Pd, 32);
    return (Hp == 1 || Hp == 2 || Hp == 4) && F == Kh && (F % 16) == 0 && F <= 4096 && Kp - F <= FB_MAXPD && Pd <= FB_MAXPD && (Dp % 4) == 0;
}

size_t txe_gat_collapse_bwd_fused_ws_bytes(int n_nodes, int n_edges, int G, int Kh, int Pd, int D, int vocab, int Hp) {
    return plan_fused_ws(nullptr, n_nodes, n_edges, G, Kh, round_up(Kh + Pd, 32), D, Pd, vocab, Hp).total;
}

// txe_gat_collapse_bwd FUSED with txe_gat_aggregate_bwd of the layer below: same inputs as txe_gat_collapse_bwd plus
// that layer's projection output Yp [N][ld_yp] = [ft | a1 | a2] (Hp heads of Dp columns, Hp*Dp == Kh), its attention alpha_p [E][Hp]
// (destination-CSR order), attention slope / dropout / seed.  Instead of d_X it returns that layer's d_Yp [N][ld_dyp] =
// [d_ft | d_a1 | d_a2 | n_pad zero columns] directly; dz_p [E][Hp] is scratch.  act_slope: slope of the activation between the two
// layers (1 = none).  dP / d_pw / dW / d_attn as txe_gat_collapse_bwd.  phases: TXE_FUSED_ALL = everything; or, for a caller that overlaps the
// independent weight-gradient GEMM with the sweeps on a second stream, separate calls with _DZ (dZ GEMM), _DW (dW GEMM partials: needs
// only d_hg and Z), _SWEEP (sweeps + first reduction stage: needs DZ), _REDUCE (final reductions: needs DW and SWEEP) and the same workspace.
// phases | TXE_FUSED_NO_EGO_WALK: the source-side sweep does not walk egonets from registers (gat_fused_bwd_kernel for every head count: the A/B switch).
// phases | TXE_WALK_NO_REFORM: the egonet walk loads every X' row instead of forming the parents' and siblings' rows again from Yp (the
// A/B switch -- and what a caller must say whose X' feature columns are not leaky(aggregate of Yp, act_slope), stored un-dropped).
int txe_gat_collapse_bwd_fused(const struct txe_graph_batch* batch, const struct txe_gat_fold_layer* layer, const struct txe_gat_fold_below* below,
                               const struct txe_fold_match* match, const struct txe_gat_fold_grads* grads, const float* d_hg, long long ld_dhg,
                               float act_slope, int phases, const float* dw_main, int dw_slices, const int* walk_plan, void* chain, void* ws,
                               size_t ws_bytes, void* stream) {
    if (!batch || !layer || !below || !grads) return TXE_ERR_ARG;
    const int *rowptr_in = batch->rowptr_in, *col_src = batch->col_src, *rowptr_out = batch->rowptr_out, *col_dst = batch->col_dst,
              *pos_out = batch->pos_out, *graph_off = batch->graph_off, *pos = layer->pos, *gid = layer->gid;
    const int n_nodes = batch->n_nodes, n_edges = batch->n_edges, G = batch->G, Kh = layer->Kh, Pd = layer->Pd, D = layer->D, vocab = layer->vocab;
    const float *X = layer->X, *Wp = layer->Wp, *W = layer->W, *attn_l = layer->attn_l, *attn_r = layer->attn_r, *pw = layer->pw, *a12 = layer->a12,
                *alpha = layer->alpha, *coef = layer->coef, *wsum = layer->wsum, *Z = layer->Z, *hg = layer->hg;
    const unsigned* mask = layer->mask;
    const float feat_drop_p = layer->feat_drop_p, attn_slope = layer->attn_slope, attn_drop_p = layer->attn_drop_p;
    const unsigned long long seed = layer->seed, seed_p = below->seed_p;
    const long long ld_hg = layer->ld_hg, ld_yp = below->ld_yp, ld_dyp = below->ld_dyp;
    const float *Yp = below->Yp, *alpha_p = below->alpha_p;
    const int Hp = below->Hp, Dp = below->Dp, n_pad = below->n_pad;
    const float attn_slope_p = below->attn_slope_p, attn_drop_p_p = below->attn_drop_p_p;
    float *d_Yp = below->d_Yp, *dz_p = below->dz_p;
    float *dW = grads->dW, *d_attn_l = grads->d_attn_l, *d_attn_r = grads->d_attn_r, *dP = grads->dP, *d_pw = grads->d_pw;
    const float *e_part = match ? match->e_part : nullptr, *m_ds = match ? match->m_ds : nullptr, *m_s = match ? match->m_s : nullptr,
                *Tf = match ? match->Tf : nullptr;
    const int m_exp = match ? match->m_exp : 0, *zrow = match ? match->zrow : nullptr;
    int* zgid = match ? match->zgid : nullptr;
    // phases | TXE_FUSED_EDOT (with | TXE_FUSED_DZ_GIVEN): the <dZ, X> sweep was done in forward (txe_gat_collapse_fwd's e_part); m_ds / m_s [G]: the folded matcher's
    // score gradient and scores, m_exp: it exponentiates -- see cl_fold_dc_kernel
    // phases | TXE_FUSED_DZ_GIVEN: `d_hg` IS dZ [G][Kp] (ld_dhg its row pitch) -- whoever consumed Z folded hg = Z W^T into its own product
    // (txe_bilinear_folded_*) and hands back dZ and the main part of dW as dw_slices slices [D][Kp] at dw_main (summed in order; 0: none)
    const bool dz_given = (phases & TXE_FUSED_DZ_GIVEN) != 0;
    if (n_nodes < 0 || n_edges < 0 || G < 0 || Kh < 1 || Pd < 0 || D < 1 || !rowptr_in || !rowptr_out || !graph_off || !X || !Wp || !W ||
        !attn_l || !attn_r || !a12 || !alpha || !coef || !wsum || !gid || !Z || (!hg && !dz_given) || (!d_hg && !(phases & TXE_FUSED_EDOT)) || !dW || !d_attn_l || !d_attn_r ||
        !ws || !Yp || !alpha_p || !d_Yp || !dz_p || n_pad < 0 || dw_slices < 0 || (dw_slices > 0 && !dw_main))
        return TXE_ERR_ARG;
    if (!txe_gat_fused_bwd_supported(Kh, Pd, Hp, Dp)) return TXE_ERR_ARG;
    if ((Pd > 0 || pw) && (!pos || vocab < 1 || vocab > MAX_VOCAB)) return TXE_ERR_ARG;
    if ((Pd > 0 && !dP) || (pw && !d_pw)) return TXE_ERR_ARG;
    if (feat_drop_p < 0.f || feat_drop_p >= 1.f || attn_drop_p < 0.f || attn_drop_p >= 1.f || attn_drop_p_p < 0.f || attn_drop_p_p >= 1.f)
        return TXE_ERR_ARG;
    const int Kt = Kh + Pd, Kp = round_up(Kt, 32), F = Hp * Dp;
    FusedWs fw = plan_fused_ws(ws, n_nodes, n_edges, G, Kh, Kp, D, Pd, vocab, Hp, (phases & TXE_FUSED_DW_BESIDE) ? DW_BESIDE_SPLITS : 0);
    CollapseWs& p = fw.c;
    if (ws_bytes < fw.total) return TXE_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const unsigned* mk = (mask && feat_drop_p > 0.f) ? mask : nullptr;
    const int mask_ld = (Kt + 31) / 32;
    const float fs = mk ? 1.f / (1.f - feat_drop_p) : 1.f, as = 1.f / (1.f - attn_drop_p);
    const float* wa = Wp + (long long)D * Kp;
    const unsigned* dummy_mask = reinterpret_cast<const unsigned*>(X);
    int rc;
    if (dz_given) phases &= ~(TXE_FUSED_DZ | TXE_FUSED_DW);
    const float* const dZv = dz_given ? d_hg : (const float*)p.dZ;
    const long long ld_dz = dz_given ? ld_dhg : (long long)Kp;
    if (dz_given && ld_dz != Kp) return TXE_ERR_ARG;               // (the sweeps walk dZ rows with the padded pitch)
    if (phases & TXE_FUSED_DZ) {   // dZ = d_hg W
        VMat A = vmat_plain(d_hg, ld_dhg, G, D);
        VMat B = vmat_plain(Wp, Kp, D, Kp);
        Epi E = epi_plain(p.dZ, Kp, Kp);
        E.alg_flops = 2.0 * G * (double)Kt * D;
        rc = gemm_nn(A, B, E, G, Kp, D, 1, s, p.tail, p.tail_bytes);
        if (rc) return rc;
    }
    const long long split_stride = (long long)D * Kp;
    if (phases & TXE_FUSED_DW) {   // dW (main part, split-K partial slices) = d_hg^T Z
        VMat A = vmat_plain(d_hg, ld_dhg, G, D);
        VMat B = vmat_plain(Z, Kp, G, Kp);
        Epi E = epi_plain(p.part, Kp, Kp);
        E.split_stride = split_stride;
        E.alg_flops = 2.0 * D * (double)Kt * G;
        rc = gemm_tn(A, B, E, D, Kp, G, p.splits, s);
        if (rc) return rc;
    }
    const int S = dz_given ? dw_slices : (G > 0 ? p.splits : 0);
    const float* const partv = dz_given ? dw_main : (const float*)p.part;
    const int nblk = (G > 0 && n_nodes > 0) ? fw.nblocks : 0;
    if ((phases & TXE_FUSED_SWEEP) && G > 0 && n_nodes > 0) {

        FoldDcArgs fdc{};
        if (phases & TXE_FUSED_EDOT) {
            if (!dz_given || !e_part || !m_ds || !m_s || !Tf || !zrow || !zgid) return TXE_ERR_ARG;
            const int nt_e = txe_gat_collapse_e_tiles(n_nodes, G, Kh, Pd);
            if (nt_e <= 0) return TXE_ERR_ARG;
            fdc = FoldDcArgs{e_part, nt_e, m_ds, m_s, m_exp, fs, wsum, coef, p.dc, p.cn, p.dS, zrow, zgid};      // (the edge kernel's prologue)
        } else {
        // (dS[g] = -<dZ[g], Z[g]> / S_g; with d_hg at hand it is <d_hg[g], hg[g]>, D columns instead of Kp)
        rc = cl_bwd_dot_launch(n_nodes, gid, X, Kp, mk, dummy_mask, mask_ld, fs, dZv, wsum, coef, p.dc, p.cn, (G + 3) / 4, G, dz_given ? Kp : D,
                               d_hg, ld_dhg, dz_given ? Z : hg, dz_given ? (long long)Kp : ld_hg, p.dS, 4.0 * ((n_nodes + (double)G) * Kp + 2.0 * G * D), s);
        if (rc) return rc;
        }
        cl_attn_bwd_launch((phases & TXE_FUSED_EDOT) != 0, rowptr_in, col_src, rowptr_out, pos_out, graph_off, G, a12, attn_slope, alpha, attn_drop_p, as, seed, pos,
                           pw, p.dc, p.dS, p.dz, p.da1, p.da2, p.dwv, fdc, s);
        {
            FusedBwdArgs a;
            memset(&a, 0, sizeof(a));
            a.rowptr_out = rowptr_out; a.col_dst = col_dst; a.pos_out = pos_out; a.gid = (phases & TXE_FUSED_EDOT) ? (const int*)zgid : gid; a.pos = pos ? pos : gid;
            a.n_nodes = n_nodes;
            a.X = X; a.Kp = Kp; a.Kh = Kh; a.Pd = Pd; a.mask = mk ? mk : dummy_mask; a.mask_ld = mask_ld; a.fscale = fs;
            a.dZ = (phases & TXE_FUSED_EDOT) ? Tf : dZv; a.cn = p.cn; a.da1 = p.da1; a.da2 = p.da2; a.wa = wa; a.act_slope = act_slope; a.vocab = vocab > 0 ? vocab : 1;
            a.Y = Yp; a.ld_y = ld_yp; a.H = Hp; a.D = Dp; a.alpha = alpha_p; a.drop_p = attn_drop_p_p;
            a.drop_scale = 1.f / (1.f - attn_drop_p_p); a.seed = seed_p;
            a.d_Y = d_Yp; a.ld_dy = ld_dyp; a.dal = fw.dal; a.dwa_part = fw.dwa_part; a.ppart = fw.ppart;
            a.npw = fw.npw;
            a.rowptr_in = rowptr_in; a.col_src = col_src; a.goff = graph_off; a.ggid = gid; a.G = G; a.hpart = fw.hpart;
            a.plan = walk_plan;
            const int nvec = F / 16, ni = (nvec + 63) / 64, nwh = 4 / Hp;
            // algorithmic bytes: read X' (own row + once per out-edge is an L2 matter), dZ, Y; write d_Y
            // (reform: a batch of egonets has one hub per graph, and only the hubs' feature columns of X' are read)
            char name[64];
            const bool ego = Hp == 4 && !(phases & TXE_FUSED_NO_EGO_WALK);            // one head per wave: the egonet-walking variant (generic graphs inside)
            // the walk forms the X' rows of parents and siblings again instead of reading them (REFORM): unless the caller says that X' is
            // not the plain activated aggregate of Yp (| TXE_WALK_NO_REFORM: stored dropped, or written by something else).  Same launch name.
            const bool reform = ego && X != nullptr && !(phases & TXE_WALK_NO_REFORM);
            if (ego) snprintf(name, sizeof(name), "gat_fused_bwd_ego_kernel<%s, %d>", mk ? "true" : "false", ni);
            else snprintf(name, sizeof(name), "gat_fused_bwd_kernel<%s, %d, %d>", mk ? "true" : "false", ni, nwh);
            const double x_skipped = reform ? (double)(n_nodes > G ? n_nodes - G : 0) * F : 0.0;
            ProfScope prof(name, s, 4.0 * (n_nodes * ((double)Kp + 2.0 * F) + (double)G * Kp - x_skipped), 1);
#define TXE_FB(M_, NI_, NW_) hipLaunchKernelGGL((gat_fused_bwd_kernel<M_, NI_, NW_>), dim3(fw.nblocks), dim3(256), (size_t)(4 * Kp + a.vocab * (Pd > 0 ? Pd : 1)) * sizeof(float), s, a)
#define TXE_FB_NI(M_, NW_) do { if (ni == 1) TXE_FB(M_, 1, NW_); else if (ni == 2) TXE_FB(M_, 2, NW_); else if (ni == 3) TXE_FB(M_, 3, NW_); else TXE_FB(M_, 4, NW_); } while (0)
#define TXE_FB_NW(M_) do { if (nwh == 1) TXE_FB_NI(M_, 1); else if (nwh == 2) TXE_FB_NI(M_, 2); else TXE_FB_NI(M_, 4); } while (0)
            if (ego) {
#define TXE_FBE(M_, NI_, R_) hipLaunchKernelGGL((gat_fused_bwd_ego_kernel<M_, NI_, R_>), dim3(fw.nblocks), dim3(256), (size_t)(4 * Kp + a.vocab * (Pd > 0 ? Pd : 1)) * sizeof(float), s, a)
#define TXE_FBE_NI(M_, R_) do { if (ni == 1) TXE_FBE(M_, 1, R_); else if (ni == 2) TXE_FBE(M_, 2, R_); else if (ni == 3) TXE_FBE(M_, 3, R_); else TXE_FBE(M_, 4, R_); } while (0)
                if (reform) { if (mk) TXE_FBE_NI(true, true); else TXE_FBE_NI(false, true); }
                else if (mk) TXE_FBE_NI(true, false); else TXE_FBE_NI(false, false);
#undef TXE_FBE_NI
#undef TXE_FBE
            } else if (mk) TXE_FB_NW(true); else TXE_FB_NW(false);
#undef TXE_FB_NW
#undef TXE_FB_NI
#undef TXE_FB
        }
        TXE_CHECK_LAUNCH();
    }
    // ---- the layer below's attention backward (edge level, from the sweep's raw d alpha) + phase A: d_wa = sum of the per-workgroup
    //      partials; readout position-weight partial sums -- one launch ----
    const int nseg = n_nodes > 0 ? p.seg_blocks : 0;
    if (phases & TXE_FUSED_SWEEP) {
    TailA ta;
    memset(&ta, 0, sizeof(ta));
    ta.nb_s1a = 0;
    ta.nb_s1b = pw ? nseg : 0; ta.s1b = Seg1Args{p.dwv, 1, 1, p.ppart2};
    ta.pos = pos; ta.n_rows = n_nodes; ta.vocab = vocab; ta.rows_per_block = p.seg_rows;
    ta.r_kind = 2; ta.nb_r = (2 * Kp + 63) / 64; ta.r2 = Seg2Args{fw.dwa_part, nblk, 2 * Kp, p.dwa};
    const bool attn = G > 0 && n_nodes > 0;
    AttnBwdArgs aa{rowptr_in, col_src, rowptr_out, pos_out, graph_off, G, Yp, ld_yp, Hp, F, attn_slope_p, alpha_p, (const float*)fw.dal, dz_p, d_Yp,
                   ld_dyp, n_pad};
    const int nb_attn = attn ? (G + FA_GRAPHS - 1) / FA_GRAPHS : 0;
    const bool ego = Hp == 4 && !(phases & TXE_FUSED_NO_EGO_WALK) && attn;
    HubFixArgs hf{graph_off, gid, rowptr_out, col_dst, n_nodes, fw.npw, fw.nblocks, F, fw.hpart, d_Yp, ld_dyp};
    const int nb_fix = ego ? fw.nblocks - 1 : 0;
    ProfScope prof("gat_attn_bwd_reduce_a_kernel", s, attn ? 4.0 * (n_edges * (4.0 * Hp + 2.0) + n_nodes * (4.0 * Hp + n_pad)) : 0.0, 1);
    hipLaunchKernelGGL(gat_attn_bwd_reduce_a_kernel, dim3(nb_fix + nb_attn + ta.nb_s1b + ta.nb_r), dim3(256), 0, s, aa, nb_attn, ta, hf, nb_fix);
    TXE_CHECK_LAUNCH();
    }
    if (!(phases & TXE_FUSED_REDUCE)) return TXE_OK;
    // ---- phase B: dW = main + attn (x) d_wa, d_attn = <d_wa, W> (unfold);  dP (from the fused sweep's partials), d_pw ----
    TailB tb;
    memset(&tb, 0, sizeof(tb));
    tb.nb_u = D;
    tb.u = UnfoldArgs{partv, S, split_stride, p.dwa, (long long)Kp, W, (long long)Kt, attn_l, attn_r, 1, D, Kt, dW, (long long)Kt, d_attn_l,
                      d_attn_r};
    tb.nb_2a = Pd > 0 ? (vocab * Pd + 63) / 64 : 0;
    tb.s2a = Seg2Args{fw.ppart, nblk, vocab * Pd, dP};
    tb.nb_2b = pw ? (vocab + 63) / 64 : 0;
    tb.s2b = Seg2Args{p.ppart2, nseg, vocab, d_pw};
    return tail_b_submit(&tb, chain, (phases & TXE_PH_DEFER) != 0, s);
}

}  // extern "C"
