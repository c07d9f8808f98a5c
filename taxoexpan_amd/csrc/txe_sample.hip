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

// The positive of query q, batch row i (one lane per query calls it): dataset.py:336-340's pointer walk, and the query's id / run entry.
__device__ __forceinline__ void emit_positive(int q, int i, int Q, int B, int base, const int* __restrict__ par_ptr,
                                              const int* __restrict__ par_idx, int* __restrict__ pos_ptr, int repeated,
                                              int* __restrict__ packed) {
    int* anchors = packed;
    int* exclude = packed + B;
    int* qids = packed + 2 * B;
    const int pb = par_ptr[q], np_ = par_ptr[q + 1] - pb;
    int p = q;                                        // (a query always has a parent: sampler.py checks; never an invalid id regardless)
    if (np_ > 0) {
        int c = pos_ptr[q];
        c = (c >= 0 && c < np_) ? c : 0;
        p = par_idx[pb + c];
        pos_ptr[q] = (c + 1) % np_;
    }
    anchors[base] = p;
    exclude[base] = q;
    if (repeated) {                                   // one run per query: the distinct id and the run's first pair
        qids[i] = q;
        packed[3 * B + i] = base;
        if (i == Q - 1) packed[3 * B + Q] = B;
    } else {
        qids[base] = q;
    }
}

// One wavefront per query, lane = negative slot (strides of 64 for k >= 64); lane 0 also takes the positive.
// A query appears once in an epoch order, and the loader's two batches in flight run on its one side stream, so no two waves -- of one
// launch or of two -- touch the same positive pointer at the same time: the read-modify-write of pos_ptr needs no atomic.
__global__ __launch_bounds__(256) void sample_anchors_kernel(const int* __restrict__ order, int start, int Q, const int* __restrict__ node_list,
                                                             const int* __restrict__ par_ptr, const int* __restrict__ par_idx,
                                                             const int* __restrict__ mask_ptr, const int* __restrict__ mask_idx,
                                                             const int* __restrict__ pool, int n_pool, int* __restrict__ pos_ptr, int k,
                                                             unsigned long long seed, int epoch, int repeated, int* __restrict__ packed,
                                                             int* __restrict__ n_padded) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + w;
    if (i >= Q) return;
    const int s = start + i;
    const int q = node_list[order[s]];
    const int B = Q * (1 + k);
    const int base = i * (1 + k);
    int* anchors = packed;
    int* exclude = packed + B;
    int* qids = packed + 2 * B;
    if (l == 0) emit_positive(q, i, Q, B, base, par_ptr, par_idx, pos_ptr, repeated, packed);
    const int mb = mask_ptr[q], mn = mask_ptr[q + 1] - mb;
    const int* mrow = mask_idx + mb;
    for (int j0 = 0; j0 < k; j0 += 64) {
        const int j = j0 + l;
        if (j >= k) break;
        int a = 0;
        bool ok = false;
        for (int t = 0; t < SAMPLE_TRIES && !ok; ++t) {
            const uint64_t h = mix64(seed ^ mix64(sample_ctr(epoch, s, j, t)));
            a = pool[(int)(((h >> 32) * (uint64_t)n_pool) >> 32)];
            const int at = lower_bound(mrow, mn, a);
            ok = !(at < mn && mrow[at] == a);
        }
        if (!ok) atomicAdd(n_padded, 1);
        const int o = base + 1 + j;
        anchors[o] = a;
        exclude[o] = -1;
        if (!repeated) qids[o] = q;
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
__device__ __forceinline__ int group_draw(unsigned long long seed, int epoch, int s, int j, int t, const int* __restrict__ pool, int n_pool) {
    const uint64_t h = mix64(seed ^ mix64(sample_ctr(epoch, s, j, t)));
    return pool[(int)(((h >> 32) * (uint64_t)n_pool) >> 32)];
}

__device__ __forceinline__ bool unmasked(const int* __restrict__ mrow, int mn, int a) {
    const int at = lower_bound(mrow, mn, a);
    return !(at < mn && mrow[at] == a);
}

// ---- hard negatives: the first slots of a query come from a mined table (sampler.mine_hard_negatives: the best unmasked pool nodes of
// node_list[i] under the model, best first), the rest from the pool route above.  Row i = order[s] of hard_idx [n_queries, H] holds
// c = min(max(hard_cnt[i], 0), H) entries; m = min(hard_slots, c) slots are hard.  One rotation per query and epoch,
// r = (hi32(h) c) >> 32 with h = mix64(seed ^ mix64(ctr(epoch, s, HARD_ROT_SLOT, 0))), and slot j < m takes row[(r + j) % c]: no
// rejection loop, the entries of a row are distinct.  Every other slot is txe_sample_anchors' slot bit for bit (the same hash of
// (seed, epoch, s, j, t), the same tries, the same n_padded accounting).
// Why a mined negative is a plain negative with exclude = -1: an anchor's egonet is its parents, itself and its children
// (dataset.py:404-437), so the query can appear in it only if the anchor is the query, one of its parents or one of its children -- all
// of them in node2masks[q], and mining selects among unmasked candidates only.  The kernel does not rely on the table for that: an entry
// that is in q's mask row, negative or above the largest pool id (pool is ascending: sorted(all_positions)) sends its slot down the
// pool route, so a bad table cannot put an invalid or masked id into a batch.
#define HARD_ROT_SLOT 16383                           // the one value of the 14-bit slot field no negative slot takes (k < 1 << 14)

__global__ __launch_bounds__(256) void sample_anchors_hard_kernel(const int* __restrict__ order, int start, int Q, const int* __restrict__ node_list,
                                                                  const int* __restrict__ par_ptr, const int* __restrict__ par_idx,
                                                                  const int* __restrict__ mask_ptr, const int* __restrict__ mask_idx,
                                                                  const int* __restrict__ pool, int n_pool, int* __restrict__ pos_ptr, int k,
                                                                  unsigned long long seed, int epoch, int repeated, int* __restrict__ packed,
                                                                  int* __restrict__ n_padded, const int* __restrict__ hard_idx,
                                                                  const int* __restrict__ hard_cnt, int H, int hard_slots) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + w;
    if (i >= Q) return;
    const int s = start + i;
    const int oi = order[s];
    const int q = node_list[oi];
    const int B = Q * (1 + k);
    const int base = i * (1 + k);
    int* anchors = packed;
    int* exclude = packed + B;
    int* qids = packed + 2 * B;
    if (l == 0) emit_positive(q, i, Q, B, base, par_ptr, par_idx, pos_ptr, repeated, packed);
    const int mb = mask_ptr[q], mn = mask_ptr[q + 1] - mb;
    const int* mrow = mask_idx + mb;
    int c = hard_cnt[oi];
    c = c < 0 ? 0 : (c > H ? H : c);                  // (a count above the row width reads no further than the row)
    const int m = hard_slots < c ? hard_slots : c;
    const int* hrow = hard_idx + (size_t)oi * (size_t)H;
    int r = 0;
    if (m > 0) {
        const uint64_t h = mix64(seed ^ mix64(sample_ctr(epoch, s, HARD_ROT_SLOT, 0)));
        r = (int)(((h >> 32) * (uint64_t)c) >> 32);
    }
    const int id_max = pool[n_pool - 1];              // the largest pool id
    for (int j0 = 0; j0 < k; j0 += 64) {
        const int j = j0 + l;
        if (j >= k) break;
        int a = 0;
        bool ok = false;
        if (j < m) {                                  // r < c and j < m <= c: r + j < 2c, no overflow
            a = hrow[(r + j) % c];
            ok = a >= 0 && a <= id_max && unmasked(mrow, mn, a);
        }
        for (int t = 0; t < SAMPLE_TRIES && !ok; ++t) {
            a = group_draw(seed, epoch, s, j, t, pool, n_pool);
            ok = unmasked(mrow, mn, a);
        }
        if (!ok) atomicAdd(n_padded, 1);
        const int o = base + 1 + j;
        anchors[o] = a;
        exclude[o] = -1;
        if (!repeated) qids[o] = q;
    }
}

// ---- near negatives: behind the hard slots, n_sib / n_gpar / n_unc slots propose a node of the positive's taxonomy neighbourhood.  With
// p the positive of the query at epoch position s, and par / chd the MASKED taxonomy's CSR (dataset.device_taxonomy; not the sampler's
// query-parent CSR): S = chd(p), the query's siblings (the query itself among them unless it is held out); G = par(p), its grandparents;
// U = chd(g_0) ++ chd(g_1) ++ .. over g_i in par(p) in order, its uncles (p among them; a DAG may repeat a node, repeats stay).
// Class X in (S, G, U) with t_X = 1, 2, 3, list length n_X and c_X slots: m_X = min(c_X, n_X), one rotation per query, epoch and class
// r_X = (hi32(h) n_X) >> 32, h = mix64(seed ^ mix64(ctr(epoch, s, HARD_ROT_SLOT, t_X))) (the table's rotation is t = 0), and the slot at
// class offset e < m_X proposes L_X[(r_X + e) % n_X].  The proposal stays iff it is in [0, n_nodes), a pool node and not in q's mask
// row; a refused proposal, a class slot e >= m_X and every slot outside the three ranges is txe_sample_anchors' slot bit for bit (the same
// hash of (seed, epoch, s, j, t), the same tries, the same n_padded accounting).  No rejection loop on the near side.
// Why a near negative is a plain negative with exclude = -1: the argument made for mined ones.  An anchor's egonet is its parents, itself
// and its children, so it holds the query only if the anchor is the query, one of its parents or one of its children -- all of them in
// node2masks[q], and a masked proposal is refused here.
// Nothing addresses memory before it is compared with its range: a CSR row of a node outside [0, n_nodes), with a negative start, an end
// before its start or beyond its index array is EMPTY (near_row), so a malformed row sends its slots down the pool route.
struct NearTaxonomy {
    const int* par_ptr;
    const int* par_idx;
    const int* chd_ptr;
    const int* chd_idx;
    int n_nodes, n_par, n_chd;                        // nodes; lengths of par_idx / chd_idx
};

// row v of the CSR (ptr [n_nodes + 1], index array of `len` entries): its start, and its length as the result (0: see above)
__device__ __forceinline__ int near_row(const int* __restrict__ ptr, int n_nodes, int len, int v, int& b) {
    b = 0;
    if (v < 0 || v >= n_nodes) return 0;
    const int lo = ptr[v], hi = ptr[v + 1];
    if (lo < 0 || hi < lo || hi > len) return 0;
    b = lo;
    return hi - lo;
}

__device__ __forceinline__ int near_rotation(unsigned long long seed, int epoch, int s, int t, int n) {
    const uint64_t h = mix64(seed ^ mix64(sample_ctr(epoch, s, HARD_ROT_SLOT, t)));
    return (int)(((h >> 32) * (uint64_t)n) >> 32);    // < n
}

// One wavefront per query, lane = negative slot, as above.  Wave-uniform and formed once per wave: the positive p, the three list bases
// and lengths, the three rotations; the lanes part ways in the binary searches (and in the uncle walk) only.
__global__ __launch_bounds__(256) void sample_anchors_near_kernel(const int* __restrict__ order, int start, int Q, const int* __restrict__ node_list,
                                                                  const int* __restrict__ par_ptr, const int* __restrict__ par_idx,
                                                                  const int* __restrict__ mask_ptr, const int* __restrict__ mask_idx,
                                                                  const int* __restrict__ pool, int n_pool, int* __restrict__ pos_ptr, int k,
                                                                  unsigned long long seed, int epoch, int repeated, int* __restrict__ packed,
                                                                  int* __restrict__ n_padded, const int* __restrict__ hard_idx,
                                                                  const int* __restrict__ hard_cnt, int H, int hard_slots, NearTaxonomy tx,
                                                                  int n_qpar, int n_sib, int n_gpar, int n_unc, int* __restrict__ n_near) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + w;
    if (i >= Q) return;                               // (wave-uniform: every lane of a live wave takes part in the ballots)
    const int s = start + i;
    const int oi = order[s];
    const int q = node_list[oi];
    const int B = Q * (1 + k);
    const int base = i * (1 + k);
    int* anchors = packed;
    int* exclude = packed + B;
    int* qids = packed + 2 * B;
    // the positive: emit_positive's walk by lane 0, handed to every lane BEFORE the pointer advances (the near slots need p)
    int p = q, c0 = 0, np_ = 0;
    if (l == 0) {
        const int pb = par_ptr[q], pe = par_ptr[q + 1];
        np_ = pe - pb;
        if (np_ > 0 && pb >= 0 && pe <= n_qpar) {
            c0 = pos_ptr[q];
            c0 = (c0 >= 0 && c0 < np_) ? c0 : 0;
            p = par_idx[pb + c0];
        } else {
            np_ = 0;
        }
    }
    p = __builtin_amdgcn_readfirstlane(p);
    if (l == 0) {
        if (np_ > 0) pos_ptr[q] = (c0 + 1) % np_;
        anchors[base] = p;
        exclude[base] = q;
        if (repeated) {                               // one run per query: the distinct id and the run's first pair
            qids[i] = q;
            packed[3 * B + i] = base;
            if (i == Q - 1) packed[3 * B + Q] = B;
        } else {
            qids[base] = q;
        }
    }
    const int mb = mask_ptr[q], mn = mask_ptr[q + 1] - mb;
    const int* mrow = mask_idx + mb;
    int c = 0;
    const int* hrow = hard_idx;
    if (hard_slots > 0) {                             // (the table may be absent when no slot asks for it)
        c = hard_cnt[oi];
        c = c < 0 ? 0 : (c > H ? H : c);
        hrow = hard_idx + (size_t)oi * (size_t)H;
    }
    const int m = hard_slots < c ? hard_slots : c;
    int r = 0;
    if (m > 0) {
        const uint64_t h = mix64(seed ^ mix64(sample_ctr(epoch, s, HARD_ROT_SLOT, 0)));
        r = (int)(((h >> 32) * (uint64_t)c) >> 32);
    }
    const int id_max = pool[n_pool - 1];              // the largest pool id
    // the three lists of p, once per wave
    int sb, gb;
    const int nS = near_row(tx.chd_ptr, tx.n_nodes, tx.n_chd, p, sb);
    const int nG = near_row(tx.par_ptr, tx.n_nodes, tx.n_par, p, gb);
    unsigned long long tot = 0;                       // |U|: the lanes share the grandparents, then add up
    for (int g = l; g < nG; g += 64) {
        int cb;
        tot += (unsigned long long)near_row(tx.chd_ptr, tx.n_nodes, tx.n_chd, tx.par_idx[gb + g], cb);
    }
    for (int d = 32; d > 0; d >>= 1) tot += __shfl_xor(tot, d);
    const int nU = tot > 0x7fffffffull ? 0 : (int)tot;           // (a list no int can index is no list)
    const int mS = n_sib < nS ? n_sib : nS, mG = n_gpar < nG ? n_gpar : nG, mU = n_unc < nU ? n_unc : nU;
    const int rS = mS > 0 ? near_rotation(seed, epoch, s, 1, nS) : 0;
    const int rG = mG > 0 ? near_rotation(seed, epoch, s, 2, nG) : 0;
    const int rU = mU > 0 ? near_rotation(seed, epoch, s, 3, nU) : 0;
    int accS = 0, accG = 0, accU = 0, pad = 0;        // wave-uniform counts
    for (int j0 = 0; j0 < k; j0 += 64) {
        const int j = j0 + l;
        int a = 0, cls = 0;                           // cls 1, 2, 3: an accepted proposal of S, G, U
        bool ok = false;
        if (j < k) {
            if (j < m) {                              // r < c and j < m <= c: r + j < 2c, no overflow
                a = hrow[(r + j) % c];
                ok = a >= 0 && a <= id_max && unmasked(mrow, mn, a);
            } else if (j >= hard_slots) {
                int e = j - hard_slots;               // (r_X < n_X and e < m_X <= n_X: the sums below stay under 2^32)
                bool prop = false;
                if (e < n_sib) {
                    if (e < mS) { a = tx.chd_idx[sb + (int)(((unsigned)rS + (unsigned)e) % (unsigned)nS)]; prop = true; cls = 1; }
                } else if ((e -= n_sib) < n_gpar) {
                    if (e < mG) { a = tx.par_idx[gb + (int)(((unsigned)rG + (unsigned)e) % (unsigned)nG)]; prop = true; cls = 2; }
                } else if ((e -= n_gpar) < n_unc) {
                    if (e < mU) {                     // entry u of U: walk par(p), subtracting child counts (the rows counted above)
                        int u = (int)(((unsigned)rU + (unsigned)e) % (unsigned)nU);
                        for (int g = 0; g < nG; ++g) {
                            int cb;
                            const int cn = near_row(tx.chd_ptr, tx.n_nodes, tx.n_chd, tx.par_idx[gb + g], cb);
                            if (u < cn) { a = tx.chd_idx[cb + u]; prop = true; cls = 3; break; }
                            u -= cn;
                        }
                    }
                }
                if (prop) {
                    ok = a >= 0 && a < tx.n_nodes;
                    if (ok) {
                        const int at = lower_bound(pool, n_pool, a);
                        ok = at < n_pool && pool[at] == a && unmasked(mrow, mn, a);
                    }
                }
                if (!ok) cls = 0;
            }
            for (int t = 0; t < SAMPLE_TRIES && !ok; ++t) {
                a = group_draw(seed, epoch, s, j, t, pool, n_pool);
                ok = unmasked(mrow, mn, a);
            }
            const int o = base + 1 + j;
            anchors[o] = a;
            exclude[o] = -1;
            if (!repeated) qids[o] = q;
        }
        accS += __popcll(__ballot(cls == 1));
        accG += __popcll(__ballot(cls == 2));
        accU += __popcll(__ballot(cls == 3));
        pad += __popcll(__ballot(j < k && !ok));
    }
    if (l == 0) {                                     // one integer atomic per counter and wave
        if (pad) atomicAdd(n_padded, pad);
        if (accS) atomicAdd(n_near, accS);
        if (accG) atomicAdd(n_near + 1, accG);
        if (accU) atomicAdd(n_near + 2, accU);
    }
}

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

int txe_sample_anchors(const int* order, int n_order, int start, int Q, const int* node_list, const int* par_ptr, const int* par_idx,
                       const int* mask_ptr, const int* mask_idx, const int* pool, int n_pool, int* pos_ptr, int k, unsigned long long seed,
                       int epoch, int repeated, int* packed, int* n_padded, void* stream) {
    if (!order || !node_list || !par_ptr || !par_idx || !mask_ptr || !mask_idx || !pool || !pos_ptr || !packed || !n_padded) return TXE_ERR_ARG;
    if (k < 1 || k >= (1 << 14) || Q < 0 || n_pool < 1 || n_order < 0 || start < 0 || epoch < 0 || epoch >= (1 << 20)) return TXE_ERR_ARG;
    if ((long long)start + Q > n_order || (long long)start + Q > (1 << 24)) return TXE_ERR_ARG;
    if (4LL * Q * (1 + k) + 1 > 0x7fffffffLL) return TXE_ERR_ARG;
    if (Q == 0) return TXE_OK;
    hipLaunchKernelGGL(sample_anchors_kernel, dim3((Q + 3) / 4), dim3(256), 0, (hipStream_t)stream, order, start, Q, node_list, par_ptr,
                       par_idx, mask_ptr, mask_idx, pool, n_pool, pos_ptr, k, seed, epoch, repeated, packed, n_padded);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

int txe_sample_anchors_hard(const int* order, int n_order, int start, int Q, const int* node_list, const int* par_ptr, const int* par_idx,
                            const int* mask_ptr, const int* mask_idx, const int* pool, int n_pool, int* pos_ptr, int k,
                            unsigned long long seed, int epoch, int repeated, int* packed, int* n_padded, const int* hard_idx,
                            const int* hard_cnt, int H, int hard_slots, void* stream) {
    if (!order || !node_list || !par_ptr || !par_idx || !mask_ptr || !mask_idx || !pool || !pos_ptr || !packed || !n_padded) return TXE_ERR_ARG;
    if (!hard_idx || !hard_cnt || H < 1) return TXE_ERR_ARG;
    if (k < 1 || k >= (1 << 14) || Q < 0 || n_pool < 1 || n_order < 0 || start < 0 || epoch < 0 || epoch >= (1 << 20)) return TXE_ERR_ARG;
    if (hard_slots < 0 || hard_slots > k) return TXE_ERR_ARG;
    if ((long long)start + Q > n_order || (long long)start + Q > (1 << 24)) return TXE_ERR_ARG;
    if (4LL * Q * (1 + k) + 1 > 0x7fffffffLL) return TXE_ERR_ARG;
    if (Q == 0) return TXE_OK;
    hipLaunchKernelGGL(sample_anchors_hard_kernel, dim3((Q + 3) / 4), dim3(256), 0, (hipStream_t)stream, order, start, Q, node_list, par_ptr,
                       par_idx, mask_ptr, mask_idx, pool, n_pool, pos_ptr, k, seed, epoch, repeated, packed, n_padded, hard_idx, hard_cnt, H,
                       hard_slots);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

int txe_sample_anchors_near(const int* order, int n_order, int start, int Q, const int* node_list, const int* par_ptr, const int* par_idx,
                            const int* mask_ptr, const int* mask_idx, const int* pool, int n_pool, int* pos_ptr, int k,
                            unsigned long long seed, int epoch, int repeated, int* packed, int* n_padded, const int* hard_idx,
                            const int* hard_cnt, int H, int hard_slots, const int* tax_par_ptr, const int* tax_par_idx,
                            const int* tax_chd_ptr, const int* tax_chd_idx, int n_nodes, int n_qpar, int n_tax_par, int n_tax_chd,
                            int n_sib, int n_gpar, int n_unc, int* n_near, void* stream) {
    if (!order || !node_list || !par_ptr || !par_idx || !mask_ptr || !mask_idx || !pool || !pos_ptr || !packed || !n_padded) return TXE_ERR_ARG;
    if (!tax_par_ptr || !tax_par_idx || !tax_chd_ptr || !tax_chd_idx || !n_near) return TXE_ERR_ARG;
    if (k < 1 || k >= (1 << 14) || Q < 0 || n_pool < 1 || n_order < 0 || start < 0 || epoch < 0 || epoch >= (1 << 20)) return TXE_ERR_ARG;
    if (hard_slots < 0 || (hard_slots > 0 && (!hard_idx || !hard_cnt || H < 1))) return TXE_ERR_ARG;
    if (n_nodes < 1 || n_qpar < 0 || n_tax_par < 0 || n_tax_chd < 0 || n_sib < 0 || n_gpar < 0 || n_unc < 0) return TXE_ERR_ARG;
    if ((long long)hard_slots + n_sib + n_gpar + n_unc > k) return TXE_ERR_ARG;
    if ((long long)start + Q > n_order || (long long)start + Q > (1 << 24)) return TXE_ERR_ARG;
    if (4LL * Q * (1 + k) + 1 > 0x7fffffffLL) return TXE_ERR_ARG;
    if (Q == 0) return TXE_OK;
    const NearTaxonomy tx = {tax_par_ptr, tax_par_idx, tax_chd_ptr, tax_chd_idx, n_nodes, n_tax_par, n_tax_chd};
    hipLaunchKernelGGL(sample_anchors_near_kernel, dim3((Q + 3) / 4), dim3(256), 0, (hipStream_t)stream, order, start, Q, node_list, par_ptr,
                       par_idx, mask_ptr, mask_idx, pool, n_pool, pos_ptr, k, seed, epoch, repeated, packed, n_padded, hard_idx, hard_cnt, H,
                       hard_slots, tx, n_qpar, n_sib, n_gpar, n_unc, n_near);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

int txe_sample_groups(const int* order, int n_order, int start, int Q, const int* node_list, const int* par_ptr, const int* par_idx,
                      const int* mask_ptr, const int* mask_idx, const int* pool, int n_pool, int k, unsigned long long seed, int epoch,
                      int repeated, int cap, int* packed, long long* labels, int* total, int* ws, int* n_padded, void* stream) {
    if (!order || !node_list || !par_ptr || !par_idx || !mask_ptr || !mask_idx || !pool || !packed || !labels || !total || !ws || !n_padded)
        return TXE_ERR_ARG;
    if (k < 1 || k >= (1 << 14) || Q < 0 || n_pool < 1 || n_order < 0 || start < 0 || epoch < 0 || epoch >= (1 << 20)) return TXE_ERR_ARG;
    if ((long long)start + Q > n_order || (long long)start + Q > (1 << 24)) return TXE_ERR_ARG;
    if (cap < Q || 4LL * cap + 1 > 0x7fffffffLL) return TXE_ERR_ARG;
    if (Q == 0) return TXE_OK;
    hipStream_t s = (hipStream_t)stream;
    int* qcnt = ws;
    int* qround = ws + Q;
    int* qoff = ws + 2 * Q;
    hipLaunchKernelGGL(sample_groups_count_kernel, dim3((Q + 3) / 4), dim3(256), 0, s, order, start, Q, node_list, par_ptr, mask_ptr, mask_idx,
                       pool, n_pool, k, seed, epoch, qcnt, qround, n_padded);
    TXE_CHECK_LAUNCH();
    hipLaunchKernelGGL(sample_groups_scan_kernel, dim3(1), dim3(1024), 0, s, qcnt, Q, qoff, total);
    TXE_CHECK_LAUNCH();
    hipLaunchKernelGGL(sample_groups_fill_kernel, dim3((Q + 3) / 4), dim3(256), 0, s, order, start, Q, node_list, par_ptr, par_idx, mask_ptr,
                       mask_idx, pool, n_pool, k, seed, epoch, repeated, cap, qoff, qround, total, packed, labels);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

}  // extern "C"
