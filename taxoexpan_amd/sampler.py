"""Training-anchor sampling on the GPU for sampling_mode 1 (data_loader/dataset.py:334-381: one positive per query through the positive
pointer, exactly negative_size negatives): csrc/txe_sample.hip writes a batch straight into the packed index layout begin_device_batch
uploads, so the egonet builder behind it is unchanged.

What is reproduced: the positive walk exactly (the same pointer arithmetic over the same parent lists, so the positives of any sequence
of epoch orders equal the host sampler's), and the distribution of the negatives -- uniform over the distinct content of the reference's
5x queue (sorted(all_positions)), rejected while masked.  What is not: the `random`-module trace of the queue shuffles (a negative slot
is a counter-based hash of (seed, epoch, epoch position, slot, attempt), host_draw restates it bit for bit) and the negative-egonet
cache (dataset.py:390-400), which the device egonet builder never had either.

Hard negatives (off by default): mine_hard_negatives ranks every pool node for every training query under the model as it stands
(candidate encode, score blocks, ops.select_k with the query's masks) and keeps the best `size` per query in a HardNegatives table;
txe_sample_anchors' table slots then fill the first `hard_slots` negative slots of a query from its row (one rotation per query and epoch)
and the rest from the pool as before.  host_draw(hard=..., hard_slots=...) restates that draw, host_hard_table the table.

Near negatives (off by default): txe_sample_anchors' near slots fill the slots behind the hard ones from the taxonomy neighbourhood of the
query's positive -- its other children (siblings), its parents (grandparents), the children of its parents (uncles) -- read off the
masked taxonomy's CSR that is resident anyway; no model pass, no table.  host_draw(near=..., taxonomy=near_arrays(dataset)) restates it."""
import numpy as np
import torch

from . import _lib
from .rng import _mix64

TRIES = 64           # SAMPLE_TRIES of csrc/txe_sample.hip: rejections before a slot keeps its (masked) last draw
HARD_ROT_SLOT = 16383    # HARD_ROT_SLOT of csrc/txe_sample.hip: the slot value of the rotation's counter (no negative slot takes it: k < 2^14)


def _check(dataset):
    if dataset.mode == "test":
        raise ValueError("device sampling draws training negatives: mode 'test' emits all candidates (use evaluate())")
    if dataset.sampling_mode != 1:
        raise ValueError(f"device sampling implements sampling_mode 1 only, got {dataset.sampling_mode}")
    if dataset.negative_size < 1:
        raise ValueError(f"device sampling needs negative_size >= 1, got {dataset.negative_size}")


def _csr(n, rows):
    """{node: iterable of ids} -> (ptr [n+1], idx) int32, rows in the given order"""
    cnt = np.zeros(n, dtype=np.int64)
    for v, r in rows.items():
        cnt[v] = len(r)
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    idx = np.zeros(int(ptr[-1]), dtype=np.int32)
    for v, r in rows.items():
        idx[ptr[v]:ptr[v + 1]] = r
    return ptr, idx


def sampler_arrays(dataset):
    """The resident inputs of txe_sample_anchors as numpy int32 arrays, from a MaskedGraphDataset (no GPU needed):
    node_list, the query-parent CSR (par_ptr / par_idx, node2parents' order), the mask CSR (mask_ptr / mask_idx, node2masks[q] sorted),
    pool = sorted(all_positions), ptr = node2positive_pointer per node, and k = negative_size."""
    _check(dataset)
    n = int(dataset.node_features.shape[0])
    node_list = np.asarray(dataset.node_list, dtype=np.int32)
    par_ptr, par_idx = _csr(n, dataset.node2parents)
    if len(node_list) and (np.diff(par_ptr)[node_list] == 0).any():
        raise ValueError("a query without a parent cannot be sampled")
    mask_ptr, mask_idx = _csr(n, {q: sorted(m) for q, m in dataset.node2masks.items()})
    ptr = np.zeros(n, dtype=np.int32)
    for v, c in dataset.node2positive_pointer.items():
        ptr[v] = c
    pool = np.asarray(sorted(dataset.all_positions), dtype=np.int32)
    if len(pool) == 0:
        raise ValueError("device sampling needs a non-empty negative pool (all_positions)")
    return dict(node_list=node_list, par_ptr=par_ptr, par_idx=par_idx, mask_ptr=mask_ptr, mask_idx=mask_idx, pool=pool, ptr=ptr,
                k=int(dataset.negative_size))


def _ctr(epoch, s, j, t):
    u = lambda a: np.asarray(a).astype(np.uint64)
    return (u(epoch) << np.uint64(44)) | (u(s) << np.uint64(20)) | (u(j) << np.uint64(6)) | u(t)


def _hard_arrays(hard):
    """(idx int64 [n_queries, H], cnt int64 [n_queries]) on the host from a HardNegatives or an (idx, cnt) pair of arrays"""
    idx, cnt = hard.numpy() if isinstance(hard, HardNegatives) else hard
    idx, cnt = np.asarray(idx).astype(np.int64), np.asarray(cnt).astype(np.int64).reshape(-1)
    if idx.ndim != 2 or idx.shape[1] < 1 or idx.shape[0] != cnt.shape[0]:
        raise ValueError(f"a hard-negative table is idx [n_queries, H >= 1] and cnt [n_queries], got {idx.shape} and {cnt.shape}")
    return idx, cnt


def near_arrays(dataset):
    """The masked taxonomy as dataset.device_taxonomy uploads it, as numpy int32 arrays (no GPU needed): dict(par_ptr, par_idx, chd_ptr,
    chd_idx, n_nodes) -- graph.pred / graph.succ per node in CSR order.  host_draw(near=..., taxonomy=this) reads it; it is NOT the
    query-parent CSR of sampler_arrays (held-out in-edges are removed here)."""
    n = int(dataset.node_features.shape[0])
    out = dict(n_nodes=n)
    for name, adj in (("par", dataset.graph.pred), ("chd", dataset.graph.succ)):
        rows = [list(adj.get(i, ())) for i in range(n)]
        out[name + "_ptr"] = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        out[name + "_idx"] = np.asarray([v for r in rows for v in r], dtype=np.int32)
    return out


def _checked_near(near, k, h0, who="near negatives"):
    """(n_s, n_g, n_u) as ints; ValueError unless each is an integer (no bool, no float) >= 0 and h0 + n_s + n_g + n_u <= k"""
    near = (0, 0, 0) if near is None else tuple(near)
    if len(near) != 3 or any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) or c < 0 for c in near):
        raise ValueError(f"{who}: three integer slot counts (siblings, grandparents, uncles), each >= 0, got {near!r}")
    near = tuple(int(c) for c in near)
    if h0 + sum(near) > k:
        raise ValueError(f"{who}: hard slots {h0} + siblings {near[0]} + grandparents {near[1]} + uncles {near[2]} exceed "
                         f"negative_size = {k}")
    return near


def _near_row(ptr, n_nodes, length, v):
    """(start, length) of row v of a CSR whose index array holds `length` entries; (0, 0) for a node outside [0, n_nodes) or a row with a
    negative start, an end before its start or beyond the index array -- near_row of csrc/txe_sample.hip"""
    if not 0 <= v < n_nodes:
        return 0, 0
    lo, hi = int(ptr[v]), int(ptr[v + 1])
    return (0, 0) if lo < 0 or hi < lo or hi > length else (lo, hi - lo)


def near_lists(taxonomy, p):
    """(S, G, U) of the positive p as int64 arrays: S = chd(p), G = par(p), U = chd(g_0) ++ chd(g_1) ++ .. over g_i in par(p), in CSR
    order (malformed rows are empty, as the kernel reads them)"""
    n, par_idx, chd_idx = int(taxonomy["n_nodes"]), np.asarray(taxonomy["par_idx"]), np.asarray(taxonomy["chd_idx"])
    sb, ns = _near_row(taxonomy["chd_ptr"], n, len(chd_idx), int(p))
    gb, ng = _near_row(taxonomy["par_ptr"], n, len(par_idx), int(p))
    G = par_idx[gb:gb + ng].astype(np.int64)
    rows = [_near_row(taxonomy["chd_ptr"], n, len(chd_idx), int(g)) for g in G]
    U = np.concatenate([chd_idx[b:b + c] for b, c in rows]).astype(np.int64) if rows else np.zeros(0, dtype=np.int64)
    if len(U) > 0x7fffffff:
        U = U[:0]
    return chd_idx[sb:sb + ns].astype(np.int64), G, U


def host_draw(arrays, order, start, Q, epoch, seed, ptr=None, repeated_queries=False, hard=None, hard_slots=0, near=None, taxonomy=None):
    """numpy restatement of txe_sample_anchors for the Q queries at positions start .. start+Q-1 of `order` (indices into node_list).
    ptr: the positive pointers (int32 [n]), advanced in place; default a copy of arrays['ptr'].  Returns dict(anchors, exclude, query
    [B]; runs [Q] and offsets [Q+1] with repeated_queries; n_padded) -- the arrays the kernel writes, bit for bit.
    hard (a HardNegatives, or its (idx, cnt) as arrays) with hard_slots in [0, k]: the restatement of the table slots, in
    integers like the rest: query i = order[s] has c = min(max(cnt[i], 0), H) entries, m = min(hard_slots, c) hard slots and the rotation
    r = (hi32(h) c) >> 32, h = mix64(seed ^ mix64(ctr(epoch, s, HARD_ROT_SLOT, 0))); slot j < m is idx[i, (r + j) % c] unless that entry
    is masked for the query, negative or above the largest pool id -- then, and for j >= m, the slot is the pool draw it is without a table.
    near = (n_s, n_g, n_u) with taxonomy = near_arrays(dataset) (the masked graph's host CSR): the restatement of the near slots.
    With p the query's positive and h0 = hard_slots (0 without a table), sibling slots are j in [h0, h0 + n_s), grandparent slots the next
    n_g, uncle slots the next n_u, over the lists near_lists(taxonomy, p) = (S, G, U).  Class X (t_X = 1, 2, 3; list length n_X, c_X slots)
    has m_X = min(c_X, n_X) and one rotation r_X = (hi32(h) n_X) >> 32, h = mix64(seed ^ mix64(ctr(epoch, s, HARD_ROT_SLOT, t_X))); the
    slot at class offset e < m_X proposes L_X[(r_X + e) % n_X], kept iff it is in [0, n_nodes), a pool node and not in q's mask row -- a
    refused proposal, and every class slot e >= m_X, is the pool draw of its own j.  near None or (0, 0, 0) changes nothing but the new key:
    the dict gains n_near = [accepted sibling, grandparent, uncle proposals] when `near` is given.  ValueError: counts that are not
    integers >= 0, h0 + n_s + n_g + n_u > k, nonzero counts without a taxonomy."""
    k = arrays["k"]
    if hard is not None and not 0 <= int(hard_slots) <= k:
        raise ValueError(f"hard_slots must be in [0, {k}], got {hard_slots}")
    h0 = int(hard_slots) if hard is not None else 0
    counts = _checked_near(near, k, h0, "host_draw: near")
    if any(counts) and taxonomy is None:
        raise ValueError("host_draw: near slots need taxonomy=near_arrays(dataset)")
    pool, mask_ptr, mask_idx = arrays["pool"], arrays["mask_ptr"], arrays["mask_idx"]
    ptr = arrays["ptr"].copy() if ptr is None else ptr
    s = np.arange(start, start + Q, dtype=np.int64)
    q = arrays["node_list"][np.asarray(order, dtype=np.int64)[s]].astype(np.int64)
    pos = np.empty(Q, dtype=np.int64)
    for i, v in enumerate(q):                                  # dataset.py:336-340, in order (a query appears once per epoch)
        b, n = arrays["par_ptr"][v], arrays["par_ptr"][v + 1] - arrays["par_ptr"][v]
        c = int(ptr[v])
        pos[i] = arrays["par_idx"][b + c]
        ptr[v] = (c + 1) % n
    with np.errstate(over="ignore"):
        j, t = np.arange(k)[None, :, None], np.arange(TRIES)[None, None, :]
        h = _mix64(np.uint64(seed) ^ _mix64(_ctr(epoch, s[:, None, None], j, t)))
        draws = pool[(((h >> np.uint64(32)) * np.uint64(len(pool))) >> np.uint64(32)).astype(np.int64)]      # [Q, k, TRIES]
        if hard is not None:
            hidx, hcnt = _hard_arrays(hard)
            rows = np.asarray(order, dtype=np.int64)[s]
            cnt = np.clip(hcnt[rows], 0, hidx.shape[1])
            n_hard = np.minimum(int(hard_slots), cnt)
            hr = _mix64(np.uint64(seed) ^ _mix64(_ctr(epoch, s, HARD_ROT_SLOT, 0)))
            rot = (((hr >> np.uint64(32)) * cnt.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
    neg = np.empty((Q, k), dtype=np.int64)
    n_padded, n_near = 0, [0, 0, 0]
    for i, v in enumerate(q):
        row = mask_idx[mask_ptr[v]:mask_ptr[v + 1]]
        ok = ~np.isin(draws[i], row)
        first = np.where(ok.any(1), ok.argmax(1), TRIES - 1)
        padded = ~ok.any(1)
        neg[i] = draws[i, np.arange(k), first]
        if hard is not None:
            for j in range(int(n_hard[i])):
                e = int(hidx[rows[i], (rot[i] + j) % cnt[i]])
                if 0 <= e <= int(pool[-1]) and e not in row:       # else: the pool route, as without a table
                    neg[i, j], padded[j] = e, False
        if any(counts):
            at = h0
            for x, (c, L) in enumerate(zip(counts, near_lists(taxonomy, pos[i]))):
                n = len(L)
                if min(c, n) > 0:
                    with np.errstate(over="ignore"):
                        hx = _mix64(np.uint64(seed) ^ _mix64(_ctr(epoch, s[i], HARD_ROT_SLOT, 1 + x)))
                    r_x = (int(hx) >> 32) * n >> 32
                    for e in range(min(c, n)):
                        a = int(L[(r_x + e) % n])
                        hit = np.searchsorted(pool, a) if 0 <= a < int(taxonomy["n_nodes"]) else len(pool)
                        if hit < len(pool) and int(pool[hit]) == a and a not in row:      # else: the pool route of slot at + e
                            neg[i, at + e], padded[at + e] = a, False
                            n_near[x] += 1
                at += c
        n_padded += int(padded.sum())
    anchors = np.concatenate([pos[:, None], neg], 1).reshape(-1)
    exclude = np.concatenate([q[:, None], np.full((Q, k), -1, dtype=np.int64)], 1).reshape(-1)
    out = dict(anchors=anchors, exclude=exclude, query=np.repeat(q, 1 + k), n_padded=n_padded)
    if repeated_queries:
        out["runs"], out["offsets"] = q, np.arange(Q + 1, dtype=np.int64) * (1 + k)
    if near is not None:
        out["n_near"] = n_near
    return out


class HardNegatives:
    """The mined hard negatives of every training query, on a device: idx int32 [n_queries, H] -- row i belongs to dataset.node_list[i]
    (the index an epoch order holds), node ids best first, unused entries -1 at the tail only -- and cnt int32 [n_queries], the valid
    entries of each row.  mine_hard_negatives makes one from the model; from_numpy validates one made elsewhere."""

    def __init__(self, idx, cnt):
        if idx.dim() != 2 or idx.shape[1] < 1 or cnt.shape != (idx.shape[0],) or idx.dtype != torch.int32 or cnt.dtype != torch.int32:
            raise ValueError(f"HardNegatives: idx int32 [n_queries, H >= 1] and cnt int32 [n_queries], got {tuple(idx.shape)} {idx.dtype} "
                             f"and {tuple(cnt.shape)} {cnt.dtype}")
        self.idx, self.cnt = idx.contiguous(), cnt.contiguous()

    n_queries = property(lambda self: int(self.idx.shape[0]))
    H = property(lambda self: int(self.idx.shape[1]))
    device = property(lambda self: self.idx.device)

    def numpy(self):
        """(idx, cnt) as host arrays (synchronises the device)"""
        return self.idx.cpu().numpy(), self.cnt.cpu().numpy()

    @classmethod
    def from_numpy(cls, idx, dataset, device):
        """a table from a host array idx [len(node_list), H] of node ids (-1 = unused), checked on the host: ValueError for another shape,
        H < 1, an entry that is neither -1 nor in all_positions, a valid entry after a -1, a duplicate in a row, or an entry in the
        query's node2masks.  cnt is the number of valid entries per row."""
        a = np.asarray(idx)
        n = len(dataset.node_list)
        if a.ndim != 2 or a.shape[0] != n or a.shape[1] < 1 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"HardNegatives: an integer array [{n}, H >= 1] is needed (one row per entry of node_list), got "
                             f"{a.dtype} {a.shape}")
        a = a.astype(np.int64)
        valid = a >= 0
        if (a < -1).any() or not np.isin(a[valid], np.asarray(sorted(dataset.all_positions), dtype=np.int64)).all():
            raise ValueError("HardNegatives: an entry is neither -1 nor a member of all_positions")
        if (valid[:, 1:] & ~valid[:, :-1]).any():
            raise ValueError("HardNegatives: a valid entry follows a -1 (unused entries sit at the tail only)")
        cnt = valid.sum(1)
        for i, q in enumerate(dataset.node_list):
            row = a[i, :cnt[i]].tolist()
            if len(set(row)) != len(row):
                raise ValueError(f"HardNegatives: row {i} (query {q}) holds a duplicate")
            if not dataset.node2masks[q].isdisjoint(row):
                raise ValueError(f"HardNegatives: row {i} holds an entry that node2masks[{q}] masks")
        return cls(torch.from_numpy(a.astype(np.int32)).to(device), torch.from_numpy(cnt.astype(np.int32)).to(device))


def _hard_size(size, n_pool):
    from . import ops
    if isinstance(size, bool) or int(size) != size or not 1 <= int(size) <= min(ops.SELECT_K_MAX, n_pool):
        raise ValueError(f"hard negatives: 1 <= size <= min({ops.SELECT_K_MAX}, pool of {n_pool}), got {size!r}")
    return int(size)


def host_hard_table(S, pool, mask_off, mask_idx, size):
    """numpy restatement of the table mine_hard_negatives selects from a score array S [n_queries, len(pool)] (larger = harder; negate
    first when smaller is better): scoring.host_select_k's best `size` unmasked columns per row -- best first, equal scores by ascending
    column, NaN last -- mapped to node ids through `pool`, -1 where fewer exist.  mask_off / mask_idx: the masked COLUMNS per query as a
    CSR.  Returns (idx int32 [n_queries, size], cnt int32 [n_queries])."""
    from .scoring import host_select_k
    pool = np.asarray(pool, dtype=np.int64)
    size = _hard_size(size, len(pool))
    sel = host_select_k(S, size, mask_off, mask_idx).astype(np.int64)
    idx = np.where(sel >= 0, pool[np.maximum(sel, 0)], -1).astype(np.int32)
    return idx, (sel >= 0).sum(1).astype(np.int32)


def _mining_inputs(model, dataset, device, seed=0, batch_size=-1, dtax=None):
    """what mining scores: dict(hg = the encoded egonets of pool = sorted(all_positions) (evaluate.candidate_graphs on the dataset's
    device taxonomy, scoring.encode_candidates in eval mode under no_grad; the model's mode is restored), qf = the raw features of
    node_list in order, pool, and mask_off / mask_idx = node2masks[q] as candidate rows (evaluate._retrieval_masks))"""
    from .evaluate import _retrieval_masks, candidate_graphs
    from .scoring import encode_candidates
    device = torch.device(device)
    pool = sorted(dataset.all_positions)
    index = {a: i for i, a in enumerate(pool)}
    g = candidate_graphs(dtax if dtax is not None else dataset.device_taxonomy(device), pool, dataset.expand_factor, seed, batch_size)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            hg = encode_candidates(model, g)
    finally:
        model.train(was_training)
    qf = dataset.node_features[torch.as_tensor(list(dataset.node_list), dtype=torch.long)].to(device)
    mask_off, mask_idx = _retrieval_masks(dataset, dataset.node_list, index)
    return dict(hg=hg, qf=qf, pool=np.asarray(pool, dtype=np.int64), mask_off=mask_off, mask_idx=mask_idx)


def mine_hard_negatives(model, dataset, device, size, qblock=None, seed=0, batch_size=-1, larger_is_better=True, dtax=None, timings=None):
    """The `size` hardest negatives of every training query under `model` as it stands, as a HardNegatives on `device`: per query of
    node_list the best-scoring nodes of the sampler's pool (sorted(all_positions)) that node2masks[q] does not name, best first (ties by
    ascending pool position, NaN last), -1 where fewer exist.  The pool's egonets are encoded once (eval mode, no_grad; the model's mode
    is restored), then score blocks of at most scoring.RETRIEVE_BLOCK_BYTES (qblock: fewer queries per block) -- the prepared matcher's
    block kernel for BIM / LBM / MLP / NTN, the literal loop for any other matcher (evaluate._score_blocks) -- negated when smaller is
    better, each followed by one masked ops.select_k.  A [queries x pool] matrix is never held.
    ValueError unless 1 <= size <= min(ops.SELECT_K_MAX, len(pool)).  seed / batch_size: the candidate egonets' sampling seed and encode
    chunk, as evaluate().  dtax: the dataset's device taxonomy when the caller holds one (a loader's .dtax; default: made here).
    timings: a dict that receives the seconds of encode / score / select (the stages are then separated by device synchronises)."""
    import time
    from . import ops
    from .evaluate import _score_blocks
    from .scoring import RETRIEVE_BLOCK_BYTES
    _check(dataset)
    device = torch.device(device)
    size = _hard_size(size, len(dataset.all_positions))
    clock = None
    if timings is not None:
        def clock(name, t0):
            torch.cuda.synchronize(device)
            timings[name] = timings.get(name, 0.0) + time.perf_counter() - t0
            return time.perf_counter()
    t0 = time.perf_counter()
    m = _mining_inputs(model, dataset, device, seed, batch_size, dtax)
    if clock:
        t0 = clock("encode", t0)
    hg, qf = m["hg"], m["qf"]
    Q, G = int(qf.shape[0]), int(hg.shape[0])
    sel = torch.full((Q, size), -1, dtype=torch.int32, device=device)
    moff = midx = None
    if m["mask_idx"].size:
        moff = torch.from_numpy(m["mask_off"].astype(np.int32)).to(device)
        midx = torch.from_numpy(m["mask_idx"].astype(np.int32)).to(device)
    block = max(1, RETRIEVE_BLOCK_BYTES // (4 * ((G + 3) // 4 * 4)))
    if qblock is not None:
        block = max(1, min(block, int(qblock)))
    was_training = model.training
    model.eval()                                                   # (the literal loop calls model.match)
    try:
        with torch.no_grad():
            for q0, S in _score_blocks(model, hg, qf, block):
                S = S.float()
                if not larger_is_better:
                    S = -S
                if clock:
                    t0 = clock("score", t0)
                q1 = q0 + S.shape[0]
                ops.select_k(S, size, None if moff is None else moff[q0:q1 + 1].contiguous(), midx, out=sel[q0:q1])
                if clock:
                    t0 = clock("select", t0)
    finally:
        model.train(was_training)
    pool_dev = torch.from_numpy(m["pool"].astype(np.int32)).to(device)
    idx = torch.where(sel >= 0, pool_dev[sel.clamp_min(0).long()], sel)
    return HardNegatives(idx, (sel >= 0).sum(1).to(torch.int32))


def _source(arrays, k):
    """struct txe_sample_source over the resident device tensors of `arrays` (the caller keeps them alive as long as the struct)"""
    a = arrays
    return _lib.SampleSource(node_list=_lib.ptr(a["node_list"]), par_ptr=_lib.ptr(a["par_ptr"]), par_idx=_lib.ptr(a["par_idx"]),
                             n_par_idx=int(a["par_idx"].numel()), mask_ptr=_lib.ptr(a["mask_ptr"]), mask_idx=_lib.ptr(a["mask_idx"]),
                             pool=_lib.ptr(a["pool"]), n_pool=int(a["pool"].numel()), k=int(k))


def _span(order_dev, start, Q, epoch, seed, repeated_queries):
    """struct txe_sample_span: the Q queries at positions start .. start+Q-1 of the uploaded epoch order, and the hash's inputs"""
    return _lib.SampleSpan(order=_lib.ptr(order_dev), n_order=int(order_dev.numel()), start=int(start), Q=int(Q), epoch=int(epoch),
                           seed=seed, repeated=int(bool(repeated_queries)))


class DeviceAnchorSampler:
    """sampler_arrays(dataset) resident on `device`, with the positive pointers (from node2positive_pointer when made; device sampling
    does NOT advance the host dict) and a padded-slot counter.  begin() launches the sampler and the egonet node count on one stream.
    launch() / begin() call txe_sample_anchors; what they hand it decides the route.  set_hard_negatives(table, slots): table slots in
    front of the pool slots; without a table the pool alone.  set_near_negatives(siblings, grandparents, uncles): with a nonzero count
    near slots behind the table slots (table or not), which read self.dtax's CSR and add to the counters near_counts() returns; with all
    counts 0 (the default) nothing changes."""

    def __init__(self, dataset, device, seed=0, dtax=None):
        _check(dataset)
        self.dataset, self.device, self.seed = dataset, torch.device(device), int(seed)
        a = sampler_arrays(dataset)
        self.k, self.n_pool, self.n_queries = a["k"], len(a["pool"]), len(a["node_list"])
        up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(self.device)
        self.arrays = {name: up(v) for name, v in a.items() if name != "k"}
        self._src = _source(self.arrays, self.k)
        self._padded = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.dtax = dtax if dtax is not None else dataset.device_taxonomy(self.device)
        self._near = torch.zeros(3, dtype=torch.int32, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()     # resident before a side stream reads them

    def upload_order(self, order, stream=None):
        """an epoch's order (indices into node_list) as an int32 device tensor, copied on `stream` (once per epoch)"""
        o = np.asarray(order, dtype=np.int64)
        if o.size and (o.min() < 0 or o.max() >= self.n_queries):
            raise ValueError("order holds an index outside the dataset")
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            return torch.from_numpy(o.astype(np.int32)).to(self.device)

    hard, hard_slots, in_epoch = None, 0, False
    near = (0, 0, 0)                                             # (sibling, grandparent, uncle) slots; all 0: no near route
    _hard_arg = _near_arg = None                                 # struct txe_sample_hard / txe_sample_near of the launches, or None

    def set_near_negatives(self, siblings=0, grandparents=0, uncles=0):
        """from the next launch on, the `siblings` negative slots behind the hard slots propose a child of the query's positive, the
        next `grandparents` a parent of it and the next `uncles` a child of one of its parents (the near slots of txe_sample_anchors; a
        proposal that is masked, outside the pool or absent leaves its slot to the pool draw).  All 0: launch() takes the route it took
        before.
        ValueError: a count that is not an integer >= 0 (bools and floats included), or hard_slots + the three counts above k.
        RuntimeError while a loader iterates an epoch over this sampler: it takes effect between epochs only."""
        if self.in_epoch:
            raise RuntimeError("set_near_negatives while an epoch is being iterated: it takes effect between epochs only")
        self.near = _checked_near((siblings, grandparents, uncles), self.k, self.hard_slots)
        t = self.dtax                                            # (resident as long as the sampler: the struct borrows its tensors)
        self._near_arg = _lib.SampleNear(par_ptr=_lib.ptr(t.par_ptr), par_idx=_lib.ptr(t.par_idx), chd_ptr=_lib.ptr(t.chd_ptr),
                                         chd_idx=_lib.ptr(t.chd_idx), n_nodes=int(t.par_ptr.numel()) - 1, n_par=int(t.par_idx.numel()),
                                         n_chd=int(t.chd_idx.numel()), n_sib=self.near[0], n_gpar=self.near[1], n_unc=self.near[2],
                                         counts=_lib.ptr(self._near)) if any(self.near) else None

    def set_hard_negatives(self, table, slots=0):
        """from the next launch on, the first `slots` negative slots of a query come from `table` (a HardNegatives on this device; None:
        the pool alone again).  ValueError: slots outside [0, k], a table with another row count than node_list, or one on another
        device.  RuntimeError while a loader iterates an epoch over this sampler (its batches in flight read the table on a side
        stream).  The device is synchronised once: the table, written on the caller's stream, is complete before a side stream reads
        it, and no launch in flight still reads the table it replaces."""
        if self.in_epoch:
            raise RuntimeError("set_hard_negatives while an epoch is being iterated: it takes effect between epochs only")
        if isinstance(slots, bool) or int(slots) != slots or not 0 <= int(slots) <= self.k:
            raise ValueError(f"hard slots must be in [0, negative_size = {self.k}], got {slots!r}")
        if table is not None:
            _checked_near(self.near, self.k, int(slots))         # (the near slots sit behind the hard ones: the same sum)
            if not isinstance(table, HardNegatives):
                raise ValueError(f"set_hard_negatives takes a sampler.HardNegatives or None, got {type(table).__name__}")
            if table.n_queries != self.n_queries:
                raise ValueError(f"the table holds {table.n_queries} rows, the dataset's node_list {self.n_queries} queries")
            if table.device != self.device:
                raise ValueError(f"the table lives on {table.device}, the sampler on {self.device}")
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self.hard, self.hard_slots = table, int(slots) if table is not None else 0
        self._hard_arg = _lib.SampleHard(idx=_lib.ptr(table.idx), cnt=_lib.ptr(table.cnt), H=table.H, slots=self.hard_slots) \
            if table is not None else None                       # (self.hard keeps the table's tensors alive)

    def launch(self, order_dev, start, Q, epoch, repeated_queries=True, stream=None):
        """txe_sample_anchors alone (the route: table slots with a table set, near slots with a nonzero near count): the packed [4B + 1]
        int32 index arrays of the batch, written on `stream` (default: current)"""
        B = Q * (1 + self.k)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)), _lib.on_device(self.device):
            packed = torch.empty(4 * B + 1, dtype=torch.int32, device=self.device)
            span = _span(order_dev, start, Q, epoch, self.seed, repeated_queries)
            _lib.call("txe_sample_anchors", _lib.ref(self._src), _lib.ref(span), _lib.ptr(self.arrays["ptr"]), _lib.ptr(packed),
                      _lib.ptr(self._padded), _lib.ref(self._hard_arg), _lib.ref(self._near_arg), _lib.stream_ptr())
        return packed

    def begin(self, order_dev, start, Q, epoch, repeated_queries=True, stream=None, egonet_seed=0):
        """begin_device_batch's job for the Q queries at positions start .. start+Q-1 of the epoch order: sampled, egonet node counts
        launched, nothing waited for (data_loaders.finish_device_batch completes it)"""
        from .graph import device_egonet_begin
        dev = self.device
        side = stream if stream is not None else torch.cuda.current_stream(dev)
        B = Q * (1 + self.k)
        packed = self.launch(order_dev, start, Q, epoch, repeated_queries, side)
        with torch.cuda.stream(side):
            job = device_egonet_begin(self.dtax, packed[:B], packed[B:2 * B], expand_factor=self.dataset.expand_factor, seed=egonet_seed)
        return dict(job=job, packed=packed, B=B, side=side, dev=dev, n_runs=Q if repeated_queries else None)

    def padded(self):
        """negative slots that kept a masked draw since the sampler was made (synchronises the device)"""
        torch.cuda.synchronize(self.device)
        return int(self._padded.item())

    def near_counts(self):
        """accepted (sibling, grandparent, uncle) proposals since the sampler was made (synchronises the device)"""
        torch.cuda.synchronize(self.device)
        return tuple(int(v) for v in self._near.cpu().tolist())

    def pointers(self):
        """the positive pointers (int32 numpy [n_nodes]) after every launch so far (synchronises the device)"""
        torch.cuda.synchronize(self.device)
        return self.arrays["ptr"].cpu().numpy()


class InBatchGroups:
    """What the in-batch loss (loss.in_batch_info_nce) needs to know about a batch of Q queries and G egonet columns, as
    int32 device tensors: anchor [G] = the taxonomy node of every column, qnode [Q] = every query's node, pos_col [Q] = the column of
    every query's own positive, and node2masks as a CSR (mask_ptr [n + 1], mask_idx, rows ascending; both None: nothing is masked).
    Column g counts for query i iff g == pos_col[i] or anchor[g] is not in the mask row of qnode[i].  A DeviceBatchLoader(in_batch=True)
    attaches one to every batch as `g.in_batch` (views of the sampler's packed index array and of its resident mask CSR: nothing is
    copied); from_numpy builds one from host arrays, validated."""

    def __init__(self, anchor, qnode, pos_col, mask_ptr=None, mask_idx=None):
        if (mask_ptr is None) != (mask_idx is None):
            raise ValueError("mask_ptr and mask_idx come together")
        for name, t in (("anchor", anchor), ("qnode", qnode), ("pos_col", pos_col), ("mask_ptr", mask_ptr), ("mask_idx", mask_idx)):
            if t is not None and not (torch.is_tensor(t) and t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous() and
                                      t.device == anchor.device):
                raise ValueError(f"InBatchGroups: {name} must be a contiguous int32 vector on the anchors' device")
        if qnode.numel() != pos_col.numel():
            raise ValueError(f"InBatchGroups: one pos_col per query, got {pos_col.numel()} for {qnode.numel()} queries")
        self.anchor, self.qnode, self.pos_col, self.mask_ptr, self.mask_idx = anchor, qnode, pos_col, mask_ptr, mask_idx
        self.Q, self.G = int(qnode.numel()), int(anchor.numel())

    device = property(lambda self: self.anchor.device)

    @classmethod
    def from_numpy(cls, anchor, qnode, pos_col, mask_ptr=None, mask_idx=None, device="cpu"):
        """from host integer arrays.  ValueError: arrays that are not one-dimensional, another number of pos_col than of queries, a
        pos_col outside [0, G), a negative anchor, exactly one of the mask arrays, a mask_ptr that does not start at 0, decreases or
        ends elsewhere than at len(mask_idx), a query node outside the CSR's rows, a mask row that is not ascending."""
        arr = lambda a: None if a is None else np.asarray(a)
        anchor, qnode, pos_col, mask_ptr, mask_idx = (arr(a) for a in (anchor, qnode, pos_col, mask_ptr, mask_idx))
        for name, a in (("anchor", anchor), ("qnode", qnode), ("pos_col", pos_col), ("mask_ptr", mask_ptr), ("mask_idx", mask_idx)):
            if a is not None and (a.ndim != 1 or not (np.issubdtype(a.dtype, np.integer) or a.size == 0)):
                raise ValueError(f"InBatchGroups.from_numpy: {name} must be a one-dimensional integer array")
        if (mask_ptr is None) != (mask_idx is None):
            raise ValueError("InBatchGroups.from_numpy: mask_ptr and mask_idx come together")
        Q, G = qnode.shape[0], anchor.shape[0]
        if pos_col.shape[0] != Q:
            raise ValueError(f"InBatchGroups.from_numpy: {pos_col.shape[0]} pos_col for {Q} queries")
        if Q and (pos_col.min() < 0 or pos_col.max() >= G):
            raise ValueError(f"InBatchGroups.from_numpy: a pos_col lies outside [0, G = {G})")
        if G and anchor.min() < 0:
            raise ValueError("InBatchGroups.from_numpy: a negative anchor")
        if Q and qnode.min() < 0:
            raise ValueError("InBatchGroups.from_numpy: a negative query node")
        if mask_ptr is not None:
            if mask_ptr.shape[0] < 1 or mask_ptr[0] != 0 or (np.diff(mask_ptr) < 0).any() or mask_ptr[-1] != mask_idx.shape[0]:
                raise ValueError("InBatchGroups.from_numpy: mask_ptr must start at 0, never decrease and end at len(mask_idx)")
            if Q and qnode.max() >= mask_ptr.shape[0] - 1:
                raise ValueError(f"InBatchGroups.from_numpy: a query node lies outside the mask CSR's {mask_ptr.shape[0] - 1} rows")
            if mask_idx.shape[0] > 1:
                row_start = np.zeros(mask_idx.shape[0], dtype=bool)
                row_start[mask_ptr[:-1][mask_ptr[:-1] < mask_idx.shape[0]]] = True
                if ((np.diff(mask_idx.astype(np.int64)) <= 0) & ~row_start[1:]).any():
                    raise ValueError("InBatchGroups.from_numpy: every mask row must be strictly ascending (sorted(node2masks[q]))")
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(device)
        if mask_idx is not None and mask_idx.shape[0] == 0:
            mask_idx = np.zeros(1, dtype=np.int32)         # (a CSR without entries: one unused element, so that its pointer is not NULL)
        return cls(up(anchor), up(qnode), up(pos_col), up(mask_ptr), up(mask_idx))

    @classmethod
    def from_packed(cls, packed, Q, k, pos_col, mask_ptr, mask_idx):
        """the views of a DeviceAnchorSampler batch (repeated_queries layout: anchors at packed[:B], the queries' nodes at
        packed[2B:2B + Q], B = Q (1 + k)); pos_col = i (1 + k), made once per batch size by the loader"""
        B = Q * (1 + k)
        return cls(packed[:B], packed[2 * B:2 * B + Q], pos_col, mask_ptr, mask_idx)

    def numpy(self):
        """dict of the host copies (synchronises)"""
        get = lambda t: None if t is None else t.cpu().numpy()
        return dict(anchor=get(self.anchor), qnode=get(self.qnode), pos_col=get(self.pos_col), mask_ptr=get(self.mask_ptr),
                    mask_idx=get(self.mask_idx))

    def record_stream(self, stream):
        """mark the batch's own views as used on `stream` (the resident mask CSR and the cached pos_col outlive every batch)"""
        self.anchor.record_stream(stream)
        self.qnode.record_stream(stream)


# ---- sampling_mode 0 (validation batches of the shipped configs): every parent, then at most k negatives ---------------------------------

def _check_groups(dataset):
    if dataset.mode == "test":
        raise ValueError("device sampling draws validation negatives: mode 'test' emits all candidates (use evaluate())")
    if dataset.sampling_mode != 0:
        raise ValueError(f"device group sampling implements sampling_mode 0 only, got {dataset.sampling_mode}")
    if dataset.negative_size < 1:
        raise ValueError(f"device sampling needs negative_size >= 1, got {dataset.negative_size}")


def group_sampler_arrays(dataset):
    """The resident inputs of txe_sample_groups as numpy int32 arrays, from a MaskedGraphDataset in sampling_mode 0 (no GPU needed):
    node_list, the query-parent CSR (node2parents' order), the mask CSR (node2masks[q] sorted), pool = sorted(all_positions), and
    k = negative_size.  (sampling_mode 0 has no positive pointer: every parent is emitted.)"""
    _check_groups(dataset)
    n = int(dataset.node_features.shape[0])
    node_list = np.asarray(dataset.node_list, dtype=np.int32)
    par_ptr, par_idx = _csr(n, dataset.node2parents)
    mask_ptr, mask_idx = _csr(n, {q: sorted(m) for q, m in dataset.node2masks.items()})
    pool = np.asarray(sorted(dataset.all_positions), dtype=np.int32)
    if len(pool) == 0:
        raise ValueError("device sampling needs a non-empty negative pool (all_positions)")
    return dict(node_list=node_list, par_ptr=par_ptr, par_idx=par_idx, mask_ptr=mask_ptr, mask_idx=mask_idx, pool=pool,
                k=int(dataset.negative_size))


def host_draw_groups(arrays, order, start, Q, epoch, seed, repeated_queries=False):
    """numpy restatement of txe_sample_groups for the Q queries at positions start .. start+Q-1 of `order` (indices into node_list):
    per query its parents (label 1, exclude = q), then the unmasked draws of the first round t whose k slot draws are not all masked, in
    slot order (label 0, exclude = -1); after TRIES empty rounds, slot 0 of the last round, counted in n_padded.  Returns dict(anchors,
    exclude, query, label [B]; runs [Q] and offsets [Q+1] with repeated_queries; n_padded) -- what the kernel writes, bit for bit."""
    k = arrays["k"]
    pool, mask_ptr, mask_idx = arrays["pool"], arrays["mask_ptr"], arrays["mask_idx"]
    par_ptr, par_idx = arrays["par_ptr"], arrays["par_idx"]
    s = np.arange(start, start + Q, dtype=np.int64)
    q = arrays["node_list"][np.asarray(order, dtype=np.int64)[s]].astype(np.int64)
    neg = [None] * Q
    pending = np.arange(Q)
    n_padded = 0
    for t in range(TRIES):                                     # round t for the queries whose earlier rounds were all masked
        if not len(pending):
            break
        with np.errstate(over="ignore"):
            h = _mix64(np.uint64(seed) ^ _mix64(_ctr(epoch, s[pending, None], np.arange(k)[None, :], t)))
            draws = pool[(((h >> np.uint64(32)) * np.uint64(len(pool))) >> np.uint64(32)).astype(np.int64)]     # [pending, k]
        left = []
        for r, i in enumerate(pending):
            row = mask_idx[mask_ptr[q[i]]:mask_ptr[q[i] + 1]]
            keep = draws[r][~np.isin(draws[r], row)]
            if len(keep):
                neg[i] = keep.astype(np.int64)
            elif t == TRIES - 1:
                neg[i] = draws[r][:1].astype(np.int64)
                n_padded += 1
            else:
                left.append(i)
        pending = np.asarray(left, dtype=np.int64)
    anchors, exclude, query, label, offsets = [], [], [], [], [0]
    for i, v in enumerate(q):
        par = par_idx[par_ptr[v]:par_ptr[v + 1]].astype(np.int64)
        n = len(par) + len(neg[i])
        anchors += [par, neg[i]]
        exclude += [np.full(len(par), v, dtype=np.int64), np.full(len(neg[i]), -1, dtype=np.int64)]
        query.append(np.full(n, v, dtype=np.int64))
        label += [np.ones(len(par), dtype=np.int64), np.zeros(len(neg[i]), dtype=np.int64)]
        offsets.append(offsets[-1] + n)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    out = dict(anchors=cat(anchors), exclude=cat(exclude), query=cat(query), label=cat(label), n_padded=n_padded)
    if repeated_queries:
        out["runs"], out["offsets"] = q, np.asarray(offsets, dtype=np.int64)
    return out


class DeviceGroupSampler:
    """group_sampler_arrays(dataset) resident on `device`, and a padded-query counter.  A batch's total B is known on the device only:
    sample() launches txe_sample_groups into buffers sized by the host-known capacity (sum of |parents| + Q k) and starts an
    asynchronous read-back of B into a pinned slot; egonet_begin() later waits for that read-back (long arrived when it is one loader
    step old) and begins the egonet node count on the B pairs.  The negative-egonet cache of the reference (dataset.py:390-400) is not
    reproduced: the device egonet builder never had one."""

    def __init__(self, dataset, device, seed=0, dtax=None):
        _check_groups(dataset)
        self.dataset, self.device, self.seed = dataset, torch.device(device), int(seed)
        a = group_sampler_arrays(dataset)
        self.k, self.n_pool, self.n_queries = a["k"], len(a["pool"]), len(a["node_list"])
        self._n_par = np.diff(a["par_ptr"]).astype(np.int64)[a["node_list"].astype(np.int64)]      # |parents| per node_list entry
        up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(self.device)
        self.arrays = {name: up(v) for name, v in a.items() if name != "k"}
        self._src = _source(self.arrays, self.k)
        self._padded = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.dtax = dtax if dtax is not None else dataset.device_taxonomy(self.device)
        self._slots = []                                             # free pinned int32 read-back slots
        torch.cuda.current_stream(self.device).synchronize()

    def upload_order(self, order, stream=None):
        """an epoch's order (indices into node_list) as an int32 device tensor, copied on `stream` (once per epoch)"""
        o = np.asarray(order, dtype=np.int64)
        if o.size and (o.min() < 0 or o.max() >= self.n_queries):
            raise ValueError("order holds an index outside the dataset")
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            t = torch.from_numpy(o.astype(np.int32)).to(self.device)
        t.host_order = o
        return t

    def capacity(self, order, start, Q):
        """the largest B the Q queries at positions start .. start+Q-1 can give: their parents plus k negatives each"""
        o = np.asarray(order, dtype=np.int64)[start:start + Q]
        return int(self._n_par[o].sum()) + Q * self.k

    def launch(self, order_dev, start, Q, epoch, repeated_queries=True, stream=None):
        """txe_sample_groups alone, on `stream` (default: current): dict(packed [4 cap + 1] int32, labels [cap] int64, total [1] int32
        (B, on the device), cap).  packed's layout uses the stride B: packed[:4B + 1] is what begin_device_batch would upload."""
        cap = self.capacity(order_dev.host_order, start, Q)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)), _lib.on_device(self.device):
            packed = torch.empty(4 * cap + 1, dtype=torch.int32, device=self.device)
            labels = torch.empty(max(cap, 1), dtype=torch.int64, device=self.device)
            total = torch.empty(2 + 3 * Q, dtype=torch.int32, device=self.device)         # [B | pad | ws 3Q + 1 ... ]
            span = _span(order_dev, start, Q, epoch, self.seed, repeated_queries)
            _lib.call("txe_sample_groups", _lib.ref(self._src), _lib.ref(span), cap, _lib.ptr(packed), _lib.ptr(labels), _lib.ptr(total),
                      _lib.ptr(total[1:]), _lib.ptr(self._padded), _lib.stream_ptr())
        return dict(packed=packed, labels=labels, total=total[:1], cap=cap, Q=Q)

    def sample(self, order_dev, start, Q, epoch, repeated_queries=True, stream=None):
        """launch() plus the asynchronous read-back of B into a pinned slot (nothing is waited for)"""
        side = stream if stream is not None else torch.cuda.current_stream(self.device)
        out = self.launch(order_dev, start, Q, epoch, repeated_queries, side)
        slot = self._slots.pop() if self._slots else torch.empty(1, dtype=torch.int32).pin_memory()
        with torch.cuda.stream(side):
            slot.copy_(out["total"], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        out.update(host_B=slot, ready=ev, side=side, repeated=bool(repeated_queries))
        return out

    def egonet_begin(self, sampled, egonet_seed=0):
        """begin_device_batch's job for a sample() result: waits for its B (one step old in DeviceBatchLoader: already there), then
        launches the egonet node count on the side stream.  Returns (pending for data_loaders.finish_device_batch, labels [B])."""
        from .graph import device_egonet_begin
        sampled["ready"].synchronize()
        B = int(sampled["host_B"][0])
        self._slots.append(sampled["host_B"])
        if not 0 < B <= sampled["cap"]:
            raise RuntimeError(f"txe_sample_groups gave a batch of {B} pairs for a capacity of {sampled['cap']}")
        packed, side = sampled["packed"], sampled["side"]
        with torch.cuda.stream(side):
            job = device_egonet_begin(self.dtax, packed[:B], packed[B:2 * B], expand_factor=self.dataset.expand_factor, seed=egonet_seed)
        pending = dict(job=job, packed=packed[:4 * B + 1], B=B, side=side, dev=self.device, n_runs=sampled["Q"] if sampled["repeated"] else None)
        return pending, sampled["labels"][:B]

    def padded(self):
        """queries that kept a masked negative since the sampler was made (synchronises the device)"""
        torch.cuda.synchronize(self.device)
        return int(self._padded.item())
