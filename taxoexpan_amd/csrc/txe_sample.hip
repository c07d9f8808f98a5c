// Training-anchor sampling ON DEVICE for sampling_mode 1 (data_loader/dataset.py:334-381: one positive per query through the positive
// pointer, exactly k negatives): one launch writes a batch straight into the packed index layout begin_device_batch uploads, so the
// egonet builder (txe_egonet_offsets / txe_egonet_fill) takes it unchanged.
//
// Negative slot j of the query at epoch position s: attempt t = 0, 1, .. draws pool[(hi32(h) * n_pool) >> 32] with
// h = mix64(seed ^ mix64(ctr(epoch, s, j, t))) and keeps the first draw that is not in the query's (sorted) mask row.  The draw is a pure
// function of (seed, epoch, s, j, t): it does not depend on the batch size or on the batch index (taxoexpan_amd/sampler.py host_draw
// restates it).  After SAMPLE_TRIES rejections the slot keeps its last draw and counts itself in n_padded -- the reference's corner case
// (dataset.py:370-375) pads with queue-head nodes that may be masked too; the anchor is always a pool node, never an invalid id.
#include "txe_common.h"

#define SAMPLE_TRIES 64

namespace txe {

// bits: t [0, 6) | j [6, 20) | s [20, 44) | epoch [44, 64) -- the argument checks keep every field inside its range
__host__ __device__ __forceinline__ uint64_t sample_ctr(int epoch, int s, int j, int t) {
    return ((uint64_t)epoch << 44) | ((uint64_t)s << 20) | ((uint64_t)j << 6) | (uint64_t)t;
}

// first position of the sorted row r[0..n) whose value is >= v
__device__ __forceinline__ int lower_bound(const int* __restrict__ r, int n, int v) {
    int lo = 0;
    while (n > 0) {
        const int half = n >> 1;
        if (r[lo + half] < v) { lo += half + 1; n -= half + 1; } else { n = half; }
    }
    return lo;
}

__device__ __forceinline__ int group_draw(unsigned long long seed, int epoch, int s, int j, int t, const int* __restrict__ pool, int n_pool) {
    const uint64_t h = mix64(seed ^ mix64(sample_ctr(epoch, s, j, t)));
    return pool[(int)(((h >> 32) * (uint64_t)n_pool) >> 32)];
}

__device__ __forceinline__ bool unmasked(const int* __restrict__ mrow, int mn, int a) {
    const int at = lower_bound(mrow, mn, a);
    return !(at < mn && mrow[at] == a);
}

// ---- sampling_mode 1: ONE kernel body, sample_anchors_kernel<HARD, NEAR>, compiled for the three routes of txe_sample_anchors (pool;
// table + pool; near + optional table + pool).  The rules of a slot are written out in include/txe.h, in order: table, near, pool.
// Every piece below exists once, so a slot that no table or near rule claims -- or whose proposal is refused -- is the same code in every
// instantiation: the same hash of (seed, epoch, s, j, t), the same tries, the same n_padded accounting.
// Why a mined or near negative is a plain negative with exclude = -1: an anchor's egonet is its parents, itself and its children
// (dataset.py:404-437), so the query can appear in it only if the anchor is the query, one of its parents or one of its children -- all
// of them in node2masks[q]; mining selects among unmasked candidates only, and a masked proposal is refused here whatever its source.
// Nothing addresses memory before it is compared with its range: a table entry that is negative or above the largest pool id (pool is
// ascending: sorted(all_positions)), a near proposal outside [0, n_nodes) or the pool, a CSR row of a node outside [0, n_nodes), with a
// negative start, an end before its start or beyond its index array (near_row: such a row is EMPTY) send their slots down the pool route.
#define HARD_ROT_SLOT 16383                           // the one value of the 14-bit slot field no negative slot takes (k < 1 << 14)

// row v of the CSR (ptr [n_nodes + 1], index array of `len` entries): its start, and its length as the result (0: see above)
__device__ __forceinline__ int near_row(const int* __restrict__ ptr, int n_nodes, int len, int v, int& b) {
    b = 0;
    if (v < 0 || v >= n_nodes) return 0;
    const int lo = ptr[v], hi = ptr[v + 1];
    if (lo < 0 || hi < lo || hi > len) return 0;
    b = lo;
    return hi - lo;
}

// one rotation per query, epoch and list: t = 0 the table row, t = 1, 2, 3 the siblings, grandparents, uncles
__device__ __forceinline__ int near_rotation(unsigned long long seed, int epoch, int s, int t, int n) {
    const uint64_t h = mix64(seed ^ mix64(sample_ctr(epoch, s, HARD_ROT_SLOT, t)));
    return (int)(((h >> 32) * (uint64_t)n) >> 32);    // < n
}

// The positive of query q, batch row i: dataset.py:336-340's pointer walk by lane 0, handed to every lane BEFORE the pointer advances
// (the near slots need p), then the positive's entries and the query's id / run entry.  A row outside par_idx is not read: p = q.
__device__ __forceinline__ int emit_positive(const txe_sample_source& src, int q, int i, int Q, int B, int base, int l,
                                             int* __restrict__ pos_ptr, int repeated, int* __restrict__ packed) {
    int p = q, c0 = 0, np_ = 0;                       // (a query always has a parent: sampler.py checks; never an invalid id regardless)
    if (l == 0) {
        const int pb = src.par_ptr[q], pe = src.par_ptr[q + 1];
        np_ = pe - pb;
        if (np_ > 0 && pb >= 0 && pe <= src.n_par_idx) {
            c0 = pos_ptr[q];
            c0 = (c0 >= 0 && c0 < np_) ? c0 : 0;
            p = src.par_idx[pb + c0];
        } else {
            np_ = 0;
        }
    }
    p = __builtin_amdgcn_readfirstlane(p);
    if (l == 0) {
        if (np_ > 0) pos_ptr[q] = (c0 + 1) % np_;
        packed[base] = p;                             // anchors
        packed[B + base] = q;                         // exclude
        if (repeated) {                               // one run per query: the distinct id and the run's first pair
            packed[2 * B + i] = q;
            packed[3 * B + i] = base;
            if (i == Q - 1) packed[3 * B + Q] = B;
        } else {
            packed[2 * B + base] = q;
        }
    }
    return p;
}

// negative a at pair o of the packed layout
__device__ __forceinline__ void store_slot(int* __restrict__ packed, int B, int o, int a, int q, int repeated) {
    packed[o] = a;
    packed[B + o] = -1;
    if (!repeated) packed[2 * B + o] = q;
}

// the pool route of slot j: the draws of (seed, epoch, s, j, t), t < SAMPLE_TRIES, until one is unmasked; a = the last draw either way
__device__ __forceinline__ bool pool_slot(const txe_sample_span& sp, int s, int j, const int* __restrict__ pool, int n_pool,
                                          const int* __restrict__ mrow, int mn, int& a) {
    bool ok = false;
    for (int t = 0; t < SAMPLE_TRIES && !ok; ++t) {
        a = group_draw(sp.seed, sp.epoch, s, j, t, pool, n_pool);
        ok = unmasked(mrow, mn, a);
    }
    return ok;
}

// wave-uniform: the table row of order index oi, its count c, its hard slots m = min(slots, c), its rotation r
struct TableRow {
    const int* row;
    int c, m, r;
};

__device__ __forceinline__ TableRow table_row(const txe_sample_hard& hard, int oi, const txe_sample_span& sp, int s) {
    TableRow tr = {hard.idx, 0, 0, 0};
    if (hard.slots > 0) {                             // (a near launch may come without a table: no slot asks for it then)
        const int c = hard.cnt[oi];
        tr.c = c < 0 ? 0 : (c > hard.H ? hard.H : c); // (a count above the row width reads no further than the row)
        tr.m = hard.slots < tr.c ? hard.slots : tr.c;
        tr.row = hard.idx + (size_t)oi * (size_t)hard.H;
        if (tr.m > 0) tr.r = near_rotation(sp.seed, sp.epoch, s, 0, tr.c);
    }
    return tr;
}

// slot j < m: no rejection loop, the entries of a row are distinct
__device__ __forceinline__ bool table_propose(const TableRow& tr, int j, int id_max, const int* __restrict__ mrow, int mn, int& a) {
    a = tr.row[(tr.r + j) % tr.c];                    // r < c and j < m <= c: r + j < 2c, no overflow
    return a >= 0 && a <= id_max && unmasked(mrow, mn, a);
}

// wave-uniform, formed once per wave: the lists of the positive p in the MASKED taxonomy (S = chd(p) from sb, G = par(p) from gb,
// U = chd(g_0) ++ chd(g_1) ++ .. over g_i in G), the slots each class fills (m_X = min(c_X, n_X)) and the three rotations
struct NearLists {
    int sb, gb, nS, nG, nU, mS, mG, mU, rS, rG, rU;
};

__device__ __forceinline__ NearLists near_lists(const txe_sample_near& tx, int p, int l, const txe_sample_span& sp, int s) {
    NearLists n;
    n.nS = near_row(tx.chd_ptr, tx.n_nodes, tx.n_chd, p, n.sb);
    n.nG = near_row(tx.par_ptr, tx.n_nodes, tx.n_par, p, n.gb);
    unsigned long long tot = 0;                       // |U|: the lanes share the grandparents, then add up
    for (int g = l; g < n.nG; g += 64) {
        int cb;
        tot += (unsigned long long)near_row(tx.chd_ptr, tx.n_nodes, tx.n_chd, tx.par_idx[n.gb + g], cb);
    }
    for (int d = 32; d > 0; d >>= 1) tot += __shfl_xor(tot, d);
    n.nU = tot > 0x7fffffffull ? 0 : (int)tot;        // (a list no int can index is no list)
    n.mS = tx.n_sib < n.nS ? tx.n_sib : n.nS;
    n.mG = tx.n_gpar < n.nG ? tx.n_gpar : n.nG;
    n.mU = tx.n_unc < n.nU ? tx.n_unc : n.nU;
    n.rS = n.mS > 0 ? near_rotation(sp.seed, sp.epoch, s, 1, n.nS) : 0;
    n.rG = n.mG > 0 ? near_rotation(sp.seed, sp.epoch, s, 2, n.nG) : 0;
    n.rU = n.mU > 0 ? near_rotation(sp.seed, sp.epoch, s, 3, n.nU) : 0;
    return n;
}

// the slot at offset e >= 0 behind the table slots: 1, 2, 3 when it is a sibling, grandparent, uncle slot whose proposal a is kept (in
// [0, n_nodes), a pool node, unmasked), 0 otherwise.  (r_X < n_X and e < m_X <= n_X: the sums below stay under 2^32)
__device__ __forceinline__ int near_propose(const txe_sample_near& tx, const NearLists& n, int e, const int* __restrict__ pool, int n_pool,
                                            const int* __restrict__ mrow, int mn, int& a) {
    int cls = 0;
    if (e < tx.n_sib) {
        if (e < n.mS) { a = tx.chd_idx[n.sb + (int)(((unsigned)n.rS + (unsigned)e) % (unsigned)n.nS)]; cls = 1; }
    } else if ((e -= tx.n_sib) < tx.n_gpar) {
        if (e < n.mG) { a = tx.par_idx[n.gb + (int)(((unsigned)n.rG + (unsigned)e) % (unsigned)n.nG)]; cls = 2; }
    } else if ((e -= tx.n_gpar) < tx.n_unc) {
        if (e < n.mU) {                               // entry u of U: walk par(p), subtracting child counts (the rows near_lists counted)
            int u = (int)(((unsigned)n.rU + (unsigned)e) % (unsigned)n.nU);
            for (int g = 0; g < n.nG; ++g) {
                int cb;
                const int cn = near_row(tx.chd_ptr, tx.n_nodes, tx.n_chd, tx.par_idx[n.gb + g], cb);
                if (u < cn) { a = tx.chd_idx[cb + u]; cls = 3; break; }
                u -= cn;
            }
        }
    }
    if (cls == 0 || a < 0 || a >= tx.n_nodes) return 0;
    const int at = lower_bound(pool, n_pool, a);
    return at < n_pool && pool[at] == a && unmasked(mrow, mn, a) ? cls : 0;
}

// One wavefront per query, lane = negative slot (strides of 64 for k >= 64); lane 0 also takes the positive.  Every lane of a live wave
// stays in the slot loop to its end: the padded (and accepted near) slots are counted by wave-uniform ballots, one atomic per counter and wave.
// A query appears once in an epoch order, and the loader's two batches in flight run on its one side stream, so no two waves -- of one
// launch or of two -- touch the same positive pointer at the same time: the read-modify-write of pos_ptr needs no atomic.
// HARD: table slots in front (read only when hard.slots > 0);  NEAR: the three class ranges behind them.  Without HARD / NEAR the
// instantiation holds no load of a table / taxonomy array and none of their bookkeeping.
template <bool HARD, bool NEAR>
__global__ __launch_bounds__(256) void sample_anchors_kernel(const txe_sample_source src, const txe_sample_span sp, int* __restrict__ pos_ptr,
                                                             int* __restrict__ packed, int* __restrict__ n_padded, const txe_sample_hard hard,
                                                             const txe_sample_near tx) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + w;
    if (i >= sp.Q) return;                            // (wave-uniform: every lane of a live wave takes part in the ballots)
    const int s = sp.start + i, k = src.k;
    const int oi = sp.order[s];
    const int q = src.node_list[oi];
    const int B = sp.Q * (1 + k);
    const int base = i * (1 + k);
    const int p = emit_positive(src, q, i, sp.Q, B, base, l, pos_ptr, sp.repeated, packed);
    const int mb = src.mask_ptr[q], mn = src.mask_ptr[q + 1] - mb;
    const int* mrow = src.mask_idx + mb;
    TableRow tr = {};
    int id_max = 0;
    if constexpr (HARD) {
        tr = table_row(hard, oi, sp, s);
        id_max = src.pool[src.n_pool - 1];            // the largest pool id
    }
    NearLists nl = {};
    if constexpr (NEAR) nl = near_lists(tx, p, l, sp, s);
    int pad = 0, accS = 0, accG = 0, accU = 0;        // wave-uniform counts
    for (int j0 = 0; j0 < k; j0 += 64) {
        const int j = j0 + l;
        int a = 0, cls = 0;                           // cls 1, 2, 3: an accepted proposal of S, G, U
        bool ok = false;
        if (j < k) {
            if constexpr (HARD) {
                if (j < tr.m) ok = table_propose(tr, j, id_max, mrow, mn, a);
            }
            if constexpr (NEAR) {
                if (j >= hard.slots) {                // (m <= slots: never a slot the table took)
                    cls = near_propose(tx, nl, j - hard.slots, src.pool, src.n_pool, mrow, mn, a);
                    ok = cls != 0;
                }
            }
            if (!ok) ok = pool_slot(sp, s, j, src.pool, src.n_pool, mrow, mn, a);
            store_slot(packed, B, base + 1 + j, a, q, sp.repeated);
        }
        if constexpr (NEAR) {
            accS += __popcll(__ballot(cls == 1));
            accG += __popcll(__ballot(cls == 2));
            accU += __popcll(__ballot(cls == 3));
        }
        pad += __popcll(__ballot(j < k && !ok));
    }
    if (l == 0) {                                     // one integer atomic per counter and wave
        if (pad) atomicAdd(n_padded, pad);
        if constexpr (NEAR) {
            if (accS) atomicAdd(tx.counts, accS);
            if (accG) atomicAdd(tx.counts + 1, accG);
            if (accU) atomicAdd(tx.counts + 2, accU);
        }
    }
}

// ---- sampling_mode 0 (data_loader/dataset.py:304-307,340-355): every parent of the query (label 1), then AT MOST k negatives (label 0).
// Negative slot j of the query at epoch position s in round t draws pool[(hi32(h) * n_pool) >> 32], h = mix64(seed ^ mix64(ctr(epoch, s,
// j, t))) -- the hash above -- and the query keeps, in slot order, the draws of round t that are not in its mask row (the reference
// drops masked entries of its k-wide queue window).  Round 0 is used unless all k of its draws are masked; then all k slots are redrawn in
// round 1, and so on.  When SAMPLE_TRIES rounds leave no survivor, the query keeps slot 0 of the last round (masked) and counts itself in
// n_padded.  (The reference's `while True` spins forever on such a window; the host sampler raises.)
// Three launches: count (one wave per query: the round and its survivor count), scan (one workgroup: per-query offsets and the batch
// total B, on the device), fill (one wave per query, the same draws again, written compacted at the final layout stride B).
__global__ __launch_bounds__(256) void sample_groups_count_kernel(const int* __restrict__ order, int start, int Q, const int* __restrict__ node_list,
                                                                  const int* __restrict__ par_ptr, const int* __restrict__ mask_ptr,
                                                                  const int* __restrict__ mask_idx, const int* __restrict__ pool, int n_pool, int k,
                                                                  unsigned long long seed, int epoch, int* __restrict__ qcnt,
                                                                  int* __restrict__ qround, int* __restrict__ n_padded) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + w;
    if (i >= Q) return;                               // (wave-uniform: every lane of a live wave takes part in the ballots)
    const int s = start + i;
    const int q = node_list[order[s]];
    const int mb = mask_ptr[q], mn = mask_ptr[q + 1] - mb;
    const int* mrow = mask_idx + mb;
    int t = 0, n = 0;
    for (; t < SAMPLE_TRIES; ++t) {
        n = 0;
        for (int j0 = 0; j0 < k; j0 += 64) {
            const int j = j0 + l;
            const bool ok = j < k && unmasked(mrow, mn, group_draw(seed, epoch, s, j, t, pool, n_pool));
            n += __popcll(__ballot(ok));
        }
        if (n > 0) break;
    }
    if (l == 0) {
        if (n == 0) {                                 // t == SAMPLE_TRIES: one padded (masked) negative
            atomicAdd(n_padded, 1);
            n = 1;
        }
        qcnt[i] = par_ptr[q + 1] - par_ptr[q] + n;
        qround[i] = t;
    }
}

// exclusive scan of qcnt [Q] into qoff [Q + 1] by one workgroup of 1024 threads; *total = qoff[Q] = B
__global__ __launch_bounds__(1024) void sample_groups_scan_kernel(const int* __restrict__ qcnt, int Q, int* __restrict__ qoff, int* __restrict__ total) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    int carry = 0;
    for (int b0 = 0; b0 < Q; b0 += 1024) {
        const int i = b0 + tid;
        const int v = i < Q ? qcnt[i] : 0;
        int x = v;                                    // inclusive scan inside the wave
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d);
            if (l >= d) x += y;
        }
        if (l == 63) wsum[w] = x;
        __syncthreads();
        int before = 0, all = 0;
        for (int u = 0; u < 16; ++u) {
            before += (u < w) ? wsum[u] : 0;
            all += wsum[u];
        }
        if (i < Q) qoff[i] = carry + before + x - v;
        carry += all;
        __syncthreads();                              // (wsum is rewritten by the next chunk)
    }
    if (tid == 0) {
        qoff[Q] = carry;
        *total = carry;
    }
}

__global__ __launch_bounds__(256) void sample_groups_fill_kernel(const int* __restrict__ order, int start, int Q, const int* __restrict__ node_list,
                                                                 const int* __restrict__ par_ptr, const int* __restrict__ par_idx,
                                                                 const int* __restrict__ mask_ptr, const int* __restrict__ mask_idx,
                                                                 const int* __restrict__ pool, int n_pool, int k, unsigned long long seed, int epoch,
                                                                 int repeated, int cap, const int* __restrict__ qoff,
                                                                 const int* __restrict__ qround, const int* __restrict__ total,
                                                                 int* __restrict__ packed, long long* __restrict__ labels) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + w;
    const int B = *total;
    if (i >= Q || B < 0 || B > cap) return;           // (a capacity below the batch writes nothing: the caller checks B <= cap)
    const int s = start + i;
    const int q = node_list[order[s]];
    const int base = qoff[i];
    int* anchors = packed;
    int* exclude = packed + B;
    int* qids = packed + 2 * B;
    const int pb = par_ptr[q], np_ = par_ptr[q + 1] - pb;
    for (int c = l; c < np_; c += 64) {               // the positives: node2parents[q] in order
        const int o = base + c;
        anchors[o] = par_idx[pb + c];
        exclude[o] = q;
        labels[o] = 1;
        if (!repeated) qids[o] = q;
    }
    const int t = qround[i];
    int o = base + np_;
    if (t >= SAMPLE_TRIES) {                          // padded: slot 0 of the last round
        if (l == 0) {
            anchors[o] = group_draw(seed, epoch, s, 0, SAMPLE_TRIES - 1, pool, n_pool);
            exclude[o] = -1;
            labels[o] = 0;
            if (!repeated) qids[o] = q;
        }
    } else {
        const int mb = mask_ptr[q], mn = mask_ptr[q + 1] - mb;
        const int* mrow = mask_idx + mb;
        for (int j0 = 0; j0 < k; j0 += 64) {          // the survivors of round t, compacted in slot order
            const int j = j0 + l;
            int a = 0;
            bool ok = false;
            if (j < k) {
                a = group_draw(seed, epoch, s, j, t, pool, n_pool);
                ok = unmasked(mrow, mn, a);
            }
            const unsigned long long m = __ballot(ok);
            if (ok) {
                const int p = o + __popcll(m & ((1ull << l) - 1ull));
                anchors[p] = a;
                exclude[p] = -1;
                labels[p] = 0;
                if (!repeated) qids[p] = q;
            }
            o += __popcll(m);
        }
    }
    if (repeated && l == 0) {                         // one run per query: the distinct id and the run's first pair
        qids[i] = q;
        packed[3 * B + i] = base;
        if (i == Q - 1) packed[3 * B + Q] = B;
    }
}

}  // namespace txe

using namespace txe;

extern "C" {

// what both entry points ask of their (src, span) pair; the capacity checks differ and stay with each entry
// (in argument order: nothing of span is read before src is sound)
static bool sample_args_ok(const txe_sample_source* src, const txe_sample_span* sp) {
    if (!src || !src->node_list || !src->par_ptr || !src->par_idx || !src->mask_ptr || !src->mask_idx || !src->pool) return false;
    if (src->k < 1 || src->k >= (1 << 14) || src->n_pool < 1 || src->n_par_idx < 0) return false;
    if (!sp || !sp->order) return false;
    if (sp->n_order < 0 || sp->start < 0 || sp->Q < 0 || sp->epoch < 0 || sp->epoch >= (1 << 20)) return false;
    return (long long)sp->start + sp->Q <= sp->n_order && (long long)sp->start + sp->Q <= (1 << 24);
}

int txe_sample_anchors(const struct txe_sample_source* src, const struct txe_sample_span* span, int* pos_ptr, int* packed, int* n_padded,
                       const struct txe_sample_hard* hard, const struct txe_sample_near* near, void* stream) {
    if (!sample_args_ok(src, span) || !pos_ptr || !packed || !n_padded) return TXE_ERR_ARG;
    const int k = src->k, Q = span->Q;
    if (hard && (!hard->idx || !hard->cnt || hard->H < 1 || hard->slots < 0 || hard->slots > k)) return TXE_ERR_ARG;
    if (near) {
        if (!near->par_ptr || !near->par_idx || !near->chd_ptr || !near->chd_idx || !near->counts) return TXE_ERR_ARG;
        if (near->n_nodes < 1 || near->n_par < 0 || near->n_chd < 0 || near->n_sib < 0 || near->n_gpar < 0 || near->n_unc < 0) return TXE_ERR_ARG;
        if ((long long)(hard ? hard->slots : 0) + near->n_sib + near->n_gpar + near->n_unc > k) return TXE_ERR_ARG;
    }
    if (4LL * Q * (1 + k) + 1 > 0x7fffffffLL) return TXE_ERR_ARG;
    if (Q == 0) return TXE_OK;
    const txe_sample_hard no_table = {};              // (slots = 0: the near instantiation reads no table)
    const txe_sample_near no_near = {};
    auto kernel = near ? sample_anchors_kernel<true, true> : hard ? sample_anchors_kernel<true, false> : sample_anchors_kernel<false, false>;
    hipLaunchKernelGGL(kernel, dim3((Q + 3) / 4), dim3(256), 0, (hipStream_t)stream, *src, *span, pos_ptr, packed, n_padded,
                       hard ? *hard : no_table, near ? *near : no_near);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

int txe_sample_groups(const struct txe_sample_source* src, const struct txe_sample_span* span, int cap, int* packed, long long* labels,
                      int* total, int* ws, int* n_padded, void* stream) {
    if (!sample_args_ok(src, span) || !packed || !labels || !total || !ws || !n_padded) return TXE_ERR_ARG;
    const int Q = span->Q;
    if (cap < Q || 4LL * cap + 1 > 0x7fffffffLL) return TXE_ERR_ARG;
    if (Q == 0) return TXE_OK;
    hipStream_t s = (hipStream_t)stream;
    int* qcnt = ws;
    int* qround = ws + Q;
    int* qoff = ws + 2 * Q;
    hipLaunchKernelGGL(sample_groups_count_kernel, dim3((Q + 3) / 4), dim3(256), 0, s, span->order, span->start, Q, src->node_list, src->par_ptr,
                       src->mask_ptr, src->mask_idx, src->pool, src->n_pool, src->k, span->seed, span->epoch, qcnt, qround, n_padded);
    TXE_CHECK_LAUNCH();
    hipLaunchKernelGGL(sample_groups_scan_kernel, dim3(1), dim3(1024), 0, s, qcnt, Q, qoff, total);
    TXE_CHECK_LAUNCH();
    hipLaunchKernelGGL(sample_groups_fill_kernel, dim3((Q + 3) / 4), dim3(256), 0, s, span->order, span->start, Q, src->node_list, src->par_ptr,
                       src->par_idx, src->mask_ptr, src->mask_idx, src->pool, src->n_pool, src->k, span->seed, span->epoch, span->repeated, cap,
                       qoff, qround, total, packed, labels);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

}  // extern "C"
