// Taxonomy-aware evaluation ON DEVICE: for every slot (query q, list position r) the prediction a = pred[q][r] against q's gold
// parents -- the depth of the deepest common ancestor, the gold that maximises Wu & Palmer similarity and the relation of the
// prediction to that gold.  Integers only: the index (longest-path depth, ancestor closure as CSR, each row ascending and
// holding the node itself) is built and validated on the host (taxoexpan_amd/taxometric.py: TaxonomyIndex) and is read-only here.
//
// One lane group of TAXO_GROUP = 16 lanes per slot.  Ancestor lists are short (synthetic MAG-CS: mean 5.6, longest 24; MAG-Full: mean
// 6.1, longest 38), so a whole wave per slot would idle three lanes in four; 16 lanes are one DPP row, so the group's integer max / or is
// four row-local DPP steps and never touches another slot's lanes -- slots of one wave may sit in different loop iterations.  Longer
// lists (a chain) are covered by the stride loop.  For each gold b the lanes stride over the SHORTER of anc(a), anc(b) and
// binary-search the longer one; a hit contributes its depth to the max, and a hit on a (resp. b) itself says a is an ancestor of b
// (resp. b of a).  Lane 0 of the group keeps the best gold by exact 64-bit cross-multiplication and writes the slot's three outputs:
// every output element has exactly one writer, there are no atomics, no floating point and no LDS, so two launches give the same bits.
//
// Bounds: a and every gold id are compared against [0, n_nodes) BEFORE they index anything; gold_off entries are clamped to
// [0, n_gold].  A bad prediction gives relation 6, a bad gold is skipped.
#include "txe_common.h"

#define TAXO_GROUP 16
#define TAXO_REL_EXACT 0
#define TAXO_REL_ANCESTOR 1
#define TAXO_REL_DESCENDANT 2
#define TAXO_REL_SIBLING 3
#define TAXO_REL_RELATED 4
#define TAXO_REL_UNRELATED 5
#define TAXO_REL_NONE 6

namespace txe {

template <int CTRL>
__device__ __forceinline__ int taxo_dpp(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}
// max / or over the 16 lanes of a DPP row (quad permutes, row_half_mirror, row_mirror: txe_common.h wave_sum's first four steps), left
// in every lane of the row.  v >= 0.  The 16 lanes of a group run the same control flow, so all of a row's lanes are active together.
__device__ __forceinline__ int group_max(int v) {
    v = max(v, taxo_dpp<0xB1>(v));
    v = max(v, taxo_dpp<0x4E>(v));
    v = max(v, taxo_dpp<0x141>(v));
    v = max(v, taxo_dpp<0x140>(v));
    return v;
}
__device__ __forceinline__ int group_or(int v) {
    v |= taxo_dpp<0xB1>(v);
    v |= taxo_dpp<0x4E>(v);
    v |= taxo_dpp<0x141>(v);
    v |= taxo_dpp<0x140>(v);
    return v;
}

// first position of the sorted row r[0..n) whose value is >= v (txe_sample.hip's lower_bound)
__device__ __forceinline__ int taxo_lower_bound(const int* __restrict__ r, int n, int v) {
    int lo = 0;
    while (n > 0) {
        const int half = n >> 1;
        if (r[lo + half] < v) { lo += half + 1; n -= half + 1; } else { n = half; }
    }
    return lo;
}

__global__ __launch_bounds__(256) void taxo_slots_kernel(const int* __restrict__ anc_ptr, const int* __restrict__ anc_idx,
                                                         const int* __restrict__ depth, const int* __restrict__ par_ptr,
                                                         const int* __restrict__ par_idx, int n_nodes, const int* __restrict__ pred,
                                                         long long n_slots, int K, const int* __restrict__ gold_off,
                                                         const int* __restrict__ gold_idx, int n_gold, int* __restrict__ lca_depth,
                                                         int* __restrict__ best_gold, int* __restrict__ relation) {
    const int gl = threadIdx.x & (TAXO_GROUP - 1);
    const long long slot = (long long)blockIdx.x * (256 / TAXO_GROUP) + (threadIdx.x / TAXO_GROUP);
    if (slot >= n_slots) return;                       // (the whole group leaves)
    const int q = (int)(slot / K);
    const int a = pred[slot];
    int g0 = gold_off[q], g1 = gold_off[q + 1];
    g0 = min(max(g0, 0), n_gold);
    g1 = min(max(g1, 0), n_gold);
    int best_l = 0, best_j = -1, best_rel = TAXO_REL_NONE, best_d = 0;
    if (a >= 0 && a < n_nodes) {
        const int da = depth[a];
        const int ab = anc_ptr[a], na = anc_ptr[a + 1] - ab;
        const int pab = par_ptr[a], npa = par_ptr[a + 1] - pab;
        for (int j = g0; j < g1; ++j) {
            const int b = gold_idx[j];
            if (b < 0 || b >= n_nodes) continue;       // (group-uniform: every lane of the group read the same b)
            const int db = depth[b];
            const int bb = anc_ptr[b], nb = anc_ptr[b + 1] - bb;
            const bool a_short = na <= nb;
            const int* __restrict__ S = anc_idx + (a_short ? ab : bb);
            const int* __restrict__ L = anc_idx + (a_short ? bb : ab);
            const int ns = a_short ? na : nb, nl = a_short ? nb : na;
            int m = 0, f = 0;
            for (int i = gl; i < ns; i += TAXO_GROUP) {
                const int v = S[i];
                const int at = taxo_lower_bound(L, nl, v);
                if (at < nl && L[at] == v) {
                    m = max(m, depth[v]);
                    f |= (v == a ? 1 : 0) | (v == b ? 2 : 0);
                }
            }
            const int l = group_max(m);
            f = group_or(f);
            int rel;
            if (a == b) rel = TAXO_REL_EXACT;
            else if (f & 1) rel = TAXO_REL_ANCESTOR;
            else if (f & 2) rel = TAXO_REL_DESCENDANT;
            else if (l == 0) rel = TAXO_REL_UNRELATED;
            else {
                const int pbb = par_ptr[b], npb = par_ptr[b + 1] - pbb;
                const long long pairs = (long long)npa * npb;
                int s = 0;
                for (long long t = gl; t < pairs; t += TAXO_GROUP)
                    s |= par_idx[pab + (int)(t / npb)] == par_idx[pbb + (int)(t % npb)] ? 1 : 0;
                rel = group_or(s) ? TAXO_REL_SIBLING : TAXO_REL_RELATED;
            }
            // wup = 2 l / (da + d): l (da + best_d) against best_l (da + db), exactly; ties: the smaller relation code, then the smaller j
            const long long lhs = (long long)l * ((long long)da + best_d), rhs = (long long)best_l * ((long long)da + db);
            if (best_j < 0 || lhs > rhs || (lhs == rhs && rel < best_rel)) {
                best_l = l; best_j = j - g0; best_rel = rel; best_d = db;
            }
        }
    }
    if (best_j < 0) { best_l = 0; best_rel = TAXO_REL_NONE; }
    if (gl == 0) {
        lca_depth[slot] = best_l;
        best_gold[slot] = best_j;
        relation[slot] = best_rel;
    }
}

}  // namespace txe

using namespace txe;

extern "C" {

int txe_taxo_slots(const int* anc_ptr, const int* anc_idx, const int* depth, const int* par_ptr, const int* par_idx, int n_nodes,
                   const int* pred, int Q, int K, const int* gold_off, const int* gold_idx, int n_gold, int* lca_depth, int* best_gold,
                   int* relation, void* stream) {
    if (!anc_ptr || !anc_idx || !depth || !par_ptr || !par_idx || !pred || !gold_off || !gold_idx || !lca_depth || !best_gold || !relation)
        return TXE_ERR_ARG;
    if (K < 1 || Q < 0 || n_nodes < 0 || n_gold < 0 || (long long)Q * K > 0x7fffffffLL) return TXE_ERR_ARG;
    if (Q == 0) return TXE_OK;
    const long long n_slots = (long long)Q * K;
    const int per_block = 256 / TAXO_GROUP;
    ProfScope prof("taxo_slots", (hipStream_t)stream, 16.0 * n_slots, 1);
    hipLaunchKernelGGL(taxo_slots_kernel, dim3((unsigned)((n_slots + per_block - 1) / per_block)), dim3(256), 0, (hipStream_t)stream, anc_ptr,
                       anc_idx, depth, par_ptr, par_idx, n_nodes, pred, n_slots, K, gold_off, gold_idx, n_gold, lca_depth, best_gold, relation);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

}  // extern "C"
