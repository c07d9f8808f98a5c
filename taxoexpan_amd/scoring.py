"""The batched egonet scoring loop of test_fast.py:99-225 / infer.py:82-159, MI355X-native.

Reference: encode every candidate egonet once, then for each query expand it to G rows and call model.match -- a
G x l x r bilinear per query, a D2H copy per query, numpy ranking per query.
Here:  U = HG W is formed once (txe_bilinear_project); a block of queries is ONE fp32-MFMA GEMM with the exp fused
(txe_score_block); ranks are counted on device (txe_rank_block).  Multi-GPU: candidates are sharded contiguously over
the ranks of one node; each rank scores its shard and the score blocks are all-gathered over xGMI (RCCL) so that every
rank holds the full [queries x candidates] block, as the north star asks.
"""
import collections
import math

import torch
import torch.distributed as dist

from . import ops


class _PreparedMatcher:
    """a matcher over a candidate set: the family's candidate side once (ops._BilinearFamily: U = hg W; ops._MLP: A = hg W1a^T + b1;
    ops._NTN: the k slices U_j = hg W_j and a = V1 hg^T + b), then every query block through ONE function per mode whatever the family
    (ops._store_block / _count_block / _topk_block / _lse_block / _moments_block) -- the same scratch and count conventions for all.  The
    blocks of positives / count / topk / lse / moments are row blocks of .queries(all queries); score takes raw query rows."""

    def __init__(self, fam, match, hg):
        self.fam, self.prep = fam, fam.project(hg, match)

    def queries(self, Q):
        return self.fam.loop_queries(Q, self.prep)

    def score(self, qb, out=None):
        return ops._store_block(self.fam, qb, self.prep, out)

    def positives(self, qb, off, rows, out):
        return self.fam.positives(qb, self.prep, off, rows, out)

    def count(self, qb, off, thr, larger_is_better, counts):
        return ops._count_block(self.fam, qb, self.prep, off, thr, larger_is_better, counts, q_padded=True)

    def topk(self, qb, k, larger_is_better, idx_base, scratch):
        return ops._topk_block(self.fam, qb, self.prep, k, larger_is_better, idx_base, scratch, q_padded=True)

    def lse(self, qb, larger_is_better, scratch):
        return ops._lse_block(self.fam, qb, self.prep, larger_is_better, scratch, q_padded=True)

    def moments(self, qb, larger_is_better, beta, scratch):
        return ops._moments_block(self.fam, qb, self.prep, larger_is_better, beta, scratch, q_padded=True)


def _ntn_fused_ok(match):
    """an NTN whose non-linearity is the tanh the kernel evaluates, with a slice count its entry points accept"""
    return (match.f is torch.tanh or match.f is torch.nn.functional.tanh) and 1 <= int(match.W.weight.shape[0]) <= ops.NTN_MAX_K


def fused_matcher_ok(match):
    """does `match` have a fused all-candidate route (prepare_matcher)?  BIM / LBM, MLP and NTN (with tanh and at most 16 slices) do;
    anything else (an NTN with another non_linear, a user's module) is scored by calling it (evaluate._score_blocks)"""
    from .model_zoo import MLP, NTN
    if isinstance(match, NTN):
        return _ntn_fused_ok(match)
    return isinstance(match, MLP) or (hasattr(match, "W") and hasattr(match, "apply_exp"))


def prepare_matcher(match, hg):
    """the one place that dispatches on the matcher: a prepared candidate side with score / positives / count / topk / lse over query
    blocks (blocks of .queries(all queries) for the last four)"""
    from .model_zoo import MLP, NTN
    if isinstance(match, NTN):
        if not _ntn_fused_ok(match):
            raise TypeError("no fused all-candidate route for an NTN matcher with a non_linear other than tanh or more than "
                            f"{ops.NTN_MAX_K} slices")
        return _PreparedMatcher(ops._NTN, match, hg)
    if isinstance(match, MLP):
        return _PreparedMatcher(ops._MLP, match, hg)
    if hasattr(match, "W") and hasattr(match, "apply_exp"):
        return _PreparedMatcher(ops._BilinearFamily(match.apply_exp), match, hg)
    raise TypeError(f"no fused all-candidate route for a {type(match).__name__} matcher (BIM / LBM / MLP / NTN have one)")


def _default_block(Q):
    """queries per launch when the caller names none: a query set of up to 4,096 goes in ONE block (score_all says why; the fused loops:
    five launches in all instead of five per 1,024 queries), larger sets in blocks of 1,024 (a [1024 x G] tile pass per block; the
    thresholds' small score matrix grows with block x positives)"""
    return 1024 if Q > 4096 else max(int(Q), 1)


def _ntn_params(m):
    """(W [k, l, r], b [k], V [k, l + r], u [k]) as float64 arrays from an NTN module or a (W, b, V, u) tuple / dict"""
    import numpy as np
    if isinstance(m, dict):
        m = (m["W.weight"], m["W.bias"], m["V.weight"], m["u_R.weight"])
    elif not isinstance(m, (tuple, list)):
        m = (m.W.weight, m.W.bias, m.V.weight, m.u_R.weight)
    W, b, V, u = (np.asarray(torch.as_tensor(t).detach().cpu(), dtype=np.float64) for t in m)
    return W, b.reshape(-1), V, u.reshape(-1)


def host_ntn_scores(match_or_params, hg, queries):
    """score_all of an NTN matcher on the host, in float64 (the host_retrieve / sampler.host_draw pattern: the tests' reference and any
    CPU caller's route): S[q][g] = sum_j u_j tanh(hg[g]^T W_j q + V_j . [hg[g] | q] + b_j) as a [Q, G] numpy array.
    match_or_params: an NTN module, or its (W.weight, W.bias, V.weight, u_R.weight) as a tuple or a state-dict-keyed dict."""
    import numpy as np
    W, b, V, u = _ntn_params(match_or_params)
    H = np.asarray(torch.as_tensor(hg).detach().cpu(), dtype=np.float64)
    Q = np.asarray(torch.as_tensor(queries).detach().cpu(), dtype=np.float64)
    l = W.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.einsum("gl,klr,qr->qgk", H, W, Q) + (H @ V[:, :l].T + b)[None, :, :] + (Q @ V[:, l:].T)[:, None, :]
        return np.tanh(t) @ u


def score_all(match, hg, queries, block=None, out=None):
    """S[q][g] = match(hg[g], queries[q]) for all pairs; match is a BIM / LBM / MLP / NTN module.
    block: queries per GEMM launch; default: a query set of up to 4,096 goes in ONE launch (MAG-CS: 2,459 queries x 24.7 k candidates
    are 7.6 rounds of tiles -- in blocks of 1,024 every block pays its own partial last round and a second, 16-tile launch), larger
    sets in blocks of 1,024."""
    pm = prepare_matcher(match, hg)
    Q = queries.shape[0]
    G = hg.shape[0]
    if block is None:
        block = _default_block(Q)
    S = out if out is not None else torch.empty((Q, (G + 3) // 4 * 4), dtype=torch.float32, device=hg.device)[:, :G]
    for q0 in range(0, Q, block):
        pm.score(queries[q0:q0 + block], out=S[q0:q0 + block])
    return S


def host_log_partition(S, larger_is_better=True):
    """log_partition_fused on the host, in float64 (the host_retrieve / host_ntn_scores pattern: the tests' reference and any CPU
    caller's route): per row of the score array S [Q, G], lse = log sum_g exp(z) with z = S (larger is better) or -S, as a float64
    numpy array [Q].  A NaN in the row gives NaN; otherwise a z = +Inf gives +Inf; otherwise all z = -Inf (or G = 0) gives -Inf;
    otherwise M + log(sum exp(z - M)), M = max z."""
    import numpy as np
    z = np.asarray(torch.as_tensor(S).detach().cpu(), dtype=np.float64)
    z = z if larger_is_better else -z
    out = np.full(z.shape[0], -np.inf, dtype=np.float64)
    for q in range(z.shape[0]):
        row = z[q]
        if row.size == 0:
            continue
        M = row.max()                                             # (numpy's max keeps a NaN)
        if np.isnan(M) or np.isinf(M):
            out[q] = M
        else:
            out[q] = M + np.log(np.exp(row - M).sum())
    return out


def log_partition_fused(match, hg, queries, larger_is_better=True, block=None):
    """lse[q] = log sum_g exp(z(q, g)) over ALL candidates g, z = the matcher's score (larger is better) or its negative: the exact
    denominator of the likelihood p(a | q) = exp(z(q, a)) / sum_a' exp(z(q, a')) that info_nce_loss (loss.py:52-57) estimates from
    sampled negatives.  BIM / LBM / MLP / NTN: per query block ONE launch of the score kernel whose epilogue reduces every tile row to a
    (max, sum exp) pair + a merge launch (txe_*_score_lse_block) -- no [Q, G] scores.  Any other matcher is scored block by block
    (evaluate._score_blocks) and reduced with torch.logsumexp.  Returns fp32 [Q] on hg's device; special values as host_log_partition
    (no candidate at all: -inf).  block: queries per launch, rank_all_fused's default.  Candidates are not sharded here."""
    dev = hg.device
    Q, G = queries.shape[0], hg.shape[0]
    if block is None:
        block = _default_block(Q)
    if Q == 0 or G == 0:
        return torch.full((Q,), -float("inf"), dtype=torch.float32, device=dev)
    if fused_matcher_ok(match):
        pm = prepare_matcher(match, hg)
        Qp = pm.queries(queries)
        scratch = {}
        return torch.cat([pm.lse(Qp[q0:q0 + block], larger_is_better, scratch) for q0 in range(0, Q, block)])
    import types
    from .evaluate import _score_blocks
    out = []
    for _q0, S in _score_blocks(types.SimpleNamespace(match=match), hg, queries, block):
        out.append(torch.logsumexp(S.float() if larger_is_better else -S.float(), dim=1))
    return torch.cat(out)


# (lse, mean, var, entropy) of every query's predictive distribution p = softmax(t) over all candidates: float64 [Q] each
ScoreMoments = collections.namedtuple("ScoreMoments", "lse mean var entropy")


def _beta_of(temperature):
    """beta = 1 / temperature as the fp32 the kernels scale by; ValueError unless the temperature and its reciprocal are finite and > 0"""
    try:
        T = float(temperature)
    except (TypeError, ValueError):
        raise ValueError(f"temperature must be a finite number > 0, got {temperature!r}") from None
    if isinstance(temperature, bool) or not (math.isfinite(T) and T > 0.0):
        raise ValueError(f"temperature must be finite and > 0, got {temperature!r}")
    return ops._check_beta(1.0 / T, "1 / temperature")


def host_score_moments(S, temperature=1.0, larger_is_better=True):
    """score_moments_fused on the host (the host_log_partition pattern: the tests' reference and any CPU caller's route): per row of the
    score array S [Q, G], with z = S (larger is better) or -S and t = fl32(beta * z) -- the product formed in fp32, beta = fl32(1 /
    temperature) -- the float64 values
        lse = M + log S0,  mean = M + S1 / S0 = E_p[t],  var = max(S2 / S0 - (S1 / S0)^2, 0) = Var_p[t],  entropy = max(log S0 - S1 / S0, 0)
    where M = max t, d = t - M, S0 / S1 / S2 = sum of exp(d), d exp(d), d^2 exp(d) over the candidates with t > -Inf, p = softmax(t).
    lse: a NaN in the row gives NaN; otherwise a t = +Inf gives +Inf; otherwise all t = -Inf (or G = 0) gives -Inf; wherever lse is not
    finite the other three are NaN.  Returns a ScoreMoments of float64 numpy arrays [Q]."""
    import numpy as np
    beta = np.float32(_beta_of(temperature))
    z = np.asarray(torch.as_tensor(S).detach().cpu(), dtype=np.float32)
    z = z if larger_is_better else -z
    with np.errstate(invalid="ignore", over="ignore"):
        t = (beta * z).astype(np.float32).astype(np.float64)       # one fp32 product, rounded on its own
    Q = t.shape[0]
    out = np.full((4, Q), np.nan, dtype=np.float64)
    out[0] = -np.inf
    for q in range(Q):
        row = t[q]
        if row.size == 0:
            continue
        M = row.max()                                             # (numpy's max keeps a NaN)
        if np.isnan(M) or np.isinf(M):
            out[0, q] = M
            continue
        d = row[row > -np.inf] - M
        e = np.exp(d)
        S0, S1, S2 = e.sum(), (d * e).sum(), (d * d * e).sum()
        r1 = S1 / S0
        out[:, q] = (M + np.log(S0), M + r1, max(S2 / S0 - r1 * r1, 0.0), max(np.log(S0) - r1, 0.0))
    return ScoreMoments(*out)


def _moments_of_block(S, beta, larger_is_better):
    """float64 [nq, 4] of a materialised score block: host_score_moments' formulas in float64 torch ops (t is the fp32 product)"""
    z = S.float() if larger_is_better else -S.float()
    t = (z * torch.tensor(beta, dtype=torch.float32, device=S.device)).to(torch.float64)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=S.device)
    M = torch.where(torch.isnan(t).any(dim=1), nan, t.max(dim=1).values)
    fin = torch.isfinite(M)
    d = t - torch.where(fin, M, torch.zeros_like(M))[:, None]
    e = torch.exp(d)
    dz = torch.where(torch.isinf(d), torch.zeros_like(d), d)
    S0, S1, S2 = e.sum(1), (dz * e).sum(1), (dz * dz * e).sum(1)
    r1 = S1 / S0
    ls = torch.log(S0)
    vals = torch.stack([M + ls, M + r1, (S2 / S0 - r1 * r1).clamp(min=0.0), (ls - r1).clamp(min=0.0)], dim=1)
    special = torch.stack([M, nan.expand_as(M), nan.expand_as(M), nan.expand_as(M)], dim=1)
    return torch.where(fin[:, None], vals, special)


def score_moments_fused(match, hg, queries, larger_is_better=True, temperature=1.0, block=None):
    """The first two moments of the scaled score under the predictive distribution over ALL candidates, per query: with z = the
    matcher's score (larger is better) or its negative, beta = 1 / temperature and t = fl32(beta * z), a ScoreMoments of float64 [Q]
    tensors on hg's device -- lse = log sum_g exp(t), mean = E_p[t], var = Var_p[t], entropy = H(p), p = softmax(t).  They are the
    derivatives a temperature fit needs (d lse / d beta = mean / beta, d^2 lse / d beta^2 = var / beta^2; calibrate.py) and the query's
    predictive entropy.  BIM / LBM / MLP / NTN: per query block ONE launch of the score kernel whose epilogue reduces every tile row to
    a quadruple + a merge launch (txe_*_score_moments_block; include/txe.h states the definitions) -- no [Q, G] scores.  Any other
    matcher is scored block by block (evaluate._score_blocks) and reduced with the same formulas in float64 torch ops.  Special values
    as host_score_moments (no candidate at all: lse -inf, the rest NaN).  block: queries per launch, rank_all_fused's default."""
    beta = _beta_of(temperature)
    dev = hg.device
    Q, G = queries.shape[0], hg.shape[0]
    if block is None:
        block = _default_block(Q)
    if Q == 0 or G == 0:
        out = torch.full((Q, 4), float("nan"), dtype=torch.float64, device=dev)
        out[:, 0] = -float("inf")
    elif fused_matcher_ok(match):
        pm = prepare_matcher(match, hg)
        Qp = pm.queries(queries)
        scratch = {}
        out = torch.cat([pm.moments(Qp[q0:q0 + block], larger_is_better, beta, scratch) for q0 in range(0, Q, block)])
    else:
        import types
        from .evaluate import _score_blocks
        out = torch.cat([_moments_of_block(S, beta, larger_is_better)
                         for _q0, S in _score_blocks(types.SimpleNamespace(match=match), hg, queries, block)])
    return ScoreMoments(*out.t().contiguous().unbind(0))


def encode_candidates(model, graph, chunk=None, device=None):
    """encode_graph over all candidate egonets (test_fast.py:99-108 small mode; :149-179 chunks of `-b` egonets).
    `graph` is one batched graph (chunk=None) or a list of batched graphs; features are taken from ndata['x']."""
    graphs = graph if isinstance(graph, (list, tuple)) else [graph]
    device = device or next(model.parameters()).device
    outs = []
    total = sum(int(bg.number_of_nodes()) for bg in graphs)
    with torch.no_grad(), ops.projection_cache(total):   # weights are fixed for the pass: table projections are shared by the chunks
        for bg in graphs:
            h = bg.ndata['x'].to(device, non_blocking=True)
            pos = bg.ndata['pos'].to(device)
            had_pos = 'pos' in bg.ndata
            bg.ndata['h'] = model.graph_propagate(bg, h)
            outs.append(model.readout(bg, pos))
            if had_pos:
                bg.ndata['pos'] = pos          # PGAT/PGCN pop it (model_zoo.py:163,212); keep the graph reusable
    return outs[0] if len(outs) == 1 else torch.cat(outs, 0)


# ---------------------------------------------------------------------------------------------------------------
# sharding helpers (pure index math: unit-tested on CPU)
# ---------------------------------------------------------------------------------------------------------------
def shard_bounds(n, world, rank):
    """contiguous shard [lo, hi) of n items: every rank but the last gets ceil(n/world) items, so the concatenation of
    equal-width padded shards has its padding only at the very end."""
    c = math.ceil(n / world) if world > 0 else n
    lo = min(rank * c, n)
    return lo, min(lo + c, n)


class ShardedScoreBlock:
    """One query block of the candidate-sharded scoring loop after its all-gather: `shards` [world, nq, c] holds, for rank r, the
    scores of candidates [r*c, (r+1)*c) (c = ceil(G / world); the tail of the last shard is padding).  Consumers index it in place --
    `columns(r)` is rank r's [nq, n_r] slab -- or ask for the dense [nq, G] matrix, which costs one more pass over the block."""

    def __init__(self, shards, n_total):
        self.shards, self.n_total = shards, int(n_total)

    @property
    def shape(self):
        return (self.shards.shape[1], self.n_total)

    def columns(self, r):
        c = self.shards.shape[2]
        return self.shards[r, :, :max(0, min(c, self.n_total - r * c))]

    def dense(self):
        world, nq, c = self.shards.shape
        return self.shards.permute(1, 0, 2).reshape(nq, world * c)[:, :self.n_total]


def all_gather_score_block(local_block, n_total, group=None):
    """local_block [nq, c] (this rank's candidate shard, padded to the common width c = ceil(G/world)) ->
    full [nq, G] on every rank.  One RCCL all-gather (blocking form; score_all_sharded pipelines it)."""
    world = dist.get_world_size(group)
    nq, c = local_block.shape
    buf = torch.empty((world, nq, c), dtype=local_block.dtype, device=local_block.device)   # rank-major concatenation
    dist.all_gather_into_tensor(buf.view(world * nq, c), local_block.contiguous(), group=group)
    return ShardedScoreBlock(buf, n_total).dense()


def score_all_sharded(match, hg_local, n_total, queries, block=1024, group=None, local_score_fn=None, on_block=None, pipeline=True):
    """Candidate-sharded scoring.  hg_local: this rank's [hi-lo, l] candidate representations (shard_bounds order).
    For every query block: local scores -> all-gather over xGMI -> on_block(q0, ShardedScoreBlock) (default: collect the dense
    [Q, G] matrix and return it).
    Pipelined (a 1,024-query MAG-Full block is 182 MB per rank, ~8 ms on the ring against ~0.2 ms of GEMM): the gather of
    block i is issued asynchronously (RCCL's own stream) and waited for only after block i+1's local GEMM has been enqueued, on
    THREE rotating pairs of preallocated buffers -- nothing is allocated, zero-filled or permuted inside the loop, and the consumer
    reads the [world, nq, c] gather buffer in place.  A block handed to on_block stays valid until on_block is called again (the
    gather issued in between writes the third buffer; with two, block i-1's buffer was re-used by gather i+1 BEFORE on_block(i) ran).
    local_score_fn(queries_block, out_padded) is injectable so the collective logic is testable without a GPU."""
    world = dist.get_world_size(group)
    c = math.ceil(n_total / world)
    dev = hg_local.device
    if local_score_fn is None:
        n_local = hg_local.shape[0]
        pm = prepare_matcher(match, hg_local) if n_local > 0 else None

        def local_score_fn(qb, out):
            if pm is not None:
                pm.score(qb, out=out[:, :n_local])
    Q = queries.shape[0]
    bmax = min(block, max(Q, 1))
    nbuf = 3 if pipeline else 1
    loc = [torch.zeros((bmax, c), dtype=torch.float32, device=dev) for _ in range(nbuf)]     # padding columns: zeroed once, never written
    full = [torch.empty((world * bmax * c,), dtype=torch.float32, device=dev) for _ in range(nbuf)]
    collected = []

    def consume(q0, nq, b, work):
        if work is not None:
            work.wait()                                   # the CURRENT stream waits for the collective; the host does not block
        blk = ShardedScoreBlock(full[b][:world * nq * c].view(world, nq, c), n_total)
        if on_block is not None:
            on_block(q0, blk)
        else:
            d = blk.dense()                               # (world > 1: a fresh tensor already; world == 1: a view of the gather buffer)
            collected.append(d.clone() if (pipeline and world == 1) else d)
    pending = None
    for i, q0 in enumerate(range(0, Q, block)):
        qb = queries[q0:q0 + block]
        nq, b = qb.shape[0], i % nbuf
        local_score_fn(qb, loc[b][:nq])
        out = full[b][:world * nq * c].view(world * nq, c)
        if pipeline:
            work = dist.all_gather_into_tensor(out, loc[b][:nq], group=group, async_op=True)
            if pending is not None:
                consume(*pending)                         # block i-1: its gather ran under this block's local GEMM
            pending = (q0, nq, b, work)
        else:
            dist.all_gather_into_tensor(out, loc[b][:nq], group=group)
            consume(q0, nq, b, None)
    if pending is not None:
        consume(*pending)
    return None if on_block is not None else (torch.cat(collected, 0) if collected else torch.zeros((0, n_total), device=dev))


def _sharded_call(group, sharded):
    """is this a candidate-SHARDED call (collectives inside)?  Only when the caller says so -- a process group handed over, or
    sharded=True for the default group.  An initialised world alone decides nothing: evaluate() / infer() on rank 0 of a DDP job, or on
    every rank with the whole candidate list, stay local and issue no collective."""
    on = bool(sharded) or group is not None
    if on and not (dist.is_available() and dist.is_initialized()):
        raise RuntimeError("candidate-sharded scoring asked for (group / sharded=True) but torch.distributed is not initialised")
    return on


def rank_all_fused(match, hg, queries, pos_off, pos_idx, block=None, larger_is_better=True, group=None, shard_lo=0, local_fns=None,
                   sharded=False, return_thresholds=False):
    """Ranks of every query's true parents among ALL candidates without materialising the score matrix.
    hg: this rank's candidate representations (rows [shard_lo, shard_lo + len) of the global candidate list; the whole list when
    not distributed).  pos_off [Q+1] / pos_idx: GLOBAL candidate columns of each query's true parents.
    Per query block: thresholds = scores of the positives (each computed by the rank that owns the candidate, summed over ranks),
    counts = fused score-and-compare over the local shard (summed over ranks), ranks = 1 + counts - own positives that beat it.
    The only collectives are two all-reduces of [n_positives] vectors per block -- instead of the [queries x candidates] all-gather.
    Sharded ONLY when asked: `group` given, or sharded=True (the default group) -- see _sharded_call.
    local_fns = (positive_scores, score_count) is injectable so that the collective logic is testable without a GPU.
    return_thresholds: (ranks, thr) -- thr fp32 [n_positives] = the positives' own scores, the values the counts compared against."""
    dev = hg.device
    distributed = _sharded_call(group, sharded)
    if block is None:
        block = _default_block(queries.shape[0])
    if local_fns is None and hg.shape[0] > 0:
        ranks, thr = _rank_all_fused_device(match, hg, queries, pos_off, pos_idx, block, larger_is_better, group, shard_lo, distributed)
        return (ranks, thr) if return_thresholds else ranks
    if local_fns is None:                                          # (an empty shard: it scores nothing, but joins the collectives)
        def f_thr(qb, off, idx_local):
            return torch.zeros(idx_local.numel(), device=dev)

        def f_cnt(qb, off, thr):
            return torch.zeros(max(int(thr.numel()), 1), dtype=torch.int32, device=dev)
    else:
        f_thr, f_cnt = local_fns
    pos_off_h = torch.as_tensor(pos_off).to(torch.int64).cpu()            # block boundaries are host integers
    pos_off_d = pos_off_h.to(dev)                                          # one upload for the whole loop
    idx_all = torch.as_tensor(pos_idx).to(torch.int64).to(dev) - shard_lo
    n_local = hg.shape[0]
    idx_all = torch.where((idx_all >= 0) & (idx_all < n_local), idx_all, torch.full_like(idx_all, -1)).to(torch.int32)
    out, thrs = [], []
    if idx_all.numel() == 0:                                       # (the same early exit and the same skipped blocks as the device
        ranks = torch.zeros(0, dtype=torch.int32, device=dev)      #  path: a rank with an empty shard issues the same collectives)
        return (ranks, torch.zeros(0, dtype=torch.float32, device=dev)) if return_thresholds else ranks
    for q0 in range(0, queries.shape[0], block):
        q1 = min(q0 + block, queries.shape[0])
        lo, hi = int(pos_off_h[q0]), int(pos_off_h[q1])
        if hi == lo:
            continue
        off = (pos_off_d[q0:q1 + 1] - lo).to(torch.int32)
        idx_local = idx_all[lo:hi]
        qb = queries[q0:q1]
        thr = f_thr(qb, off, idx_local)
        if distributed:
            dist.all_reduce(thr, op=dist.ReduceOp.SUM, group=group)          # each positive lives in exactly one shard
        thrs.append(thr)
        counts = f_cnt(qb, off, thr)[:hi - lo]
        if distributed:
            dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=group)
        if local_fns is None:
            out.append(ops.rank_finalize(off, thr, counts, larger_is_better))
        else:
            out.append(_rank_finalize_host(off, thr, counts, larger_is_better))
    ranks = torch.cat(out) if out else torch.zeros(0, dtype=torch.int32, device=dev)
    if not return_thresholds:
        return ranks
    return ranks, (torch.cat(thrs).to(torch.float32) if thrs else torch.zeros(0, dtype=torch.float32, device=dev))


def _rank_all_fused_device(match, hg, queries, pos_off, pos_idx, block, larger_is_better, group, shard_lo, distributed):
    """rank_all_fused on the HIP kernels with everything that does not depend on the scores prepared ONCE, on the host, for all query
    blocks (the positives' rows and block-local offsets): the
    loop itself is four launches per block, no host synchronisation, no per-block index arithmetic on the device.  (The first version
    did that arithmetic per block with a dozen torch launches and a repeat_interleave sync: 0.65 ms of host time against 0.69 ms of
    kernels on the MAG-CS shape -- the fused route lost to materialise + rank by 2x for that reason alone.)"""
    import numpy as np
    dev = hg.device
    n_local, Q = hg.shape[0], queries.shape[0]
    off_h = np.asarray(torch.as_tensor(pos_off).cpu(), dtype=np.int64)
    idx_h = np.asarray(torch.as_tensor(pos_idx).cpu(), dtype=np.int64) - int(shard_lo)
    n_pos = int(idx_h.shape[0])
    if n_pos == 0 or Q == 0:
        return torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.float32, device=dev)
    nblk = (Q + block - 1) // block
    q0s = np.minimum(np.arange(nblk + 1) * block, Q)
    lo_b = off_h[q0s]                                                     # first positive of every block (+ the end)
    local_h = (idx_h >= 0) & (idx_h < n_local)
    offs_h = np.concatenate([off_h[q0s[b]:q0s[b + 1] + 1] - lo_b[b] for b in range(nblk)]).astype(np.int32)   # block-local offsets, back to back
    up = lambda a, dt: torch.as_tensor(a, dtype=dt).to(dev, non_blocking=True)
    idxc = up(np.where(local_h, idx_h, 0), torch.int64)
    offs = up(offs_h, torch.int32)
    all_local = bool(local_h.all())
    localb = None if all_local else up(local_h, torch.bool)
    pm = prepare_matcher(match, hg)
    Qp = pm.queries(queries)
    counts = torch.zeros(n_pos, dtype=torch.int32, device=dev)
    ranks = torch.empty(n_pos, dtype=torch.int32, device=dev)
    thr_all = torch.empty(n_pos, dtype=torch.float32, device=dev)
    o0 = 0
    for b in range(nblk):
        q0, q1, lo, hi = int(q0s[b]), int(q0s[b + 1]), int(lo_b[b]), int(lo_b[b + 1])
        off = offs[o0:o0 + (q1 - q0) + 1]
        o0 += (q1 - q0) + 1
        if hi == lo:
            continue
        qb = Qp[q0:q1]
        # thresholds: the positives' scores through the SAME score kernel as the block (bit-identical values), the staircase of tiles
        # that holds them only
        thr = pm.positives(qb, off, idxc[lo:hi], thr_all[lo:hi])
        if localb is not None:                                           # a positive that lives in another shard contributes 0 here
            thr.copy_(torch.where(localb[lo:hi], thr, torch.zeros((), device=dev)))      # (not a product: the placeholder may be inf)
        if distributed:
            dist.all_reduce(thr, op=dist.ReduceOp.SUM, group=group)      # each positive lives in exactly one shard
        pm.count(qb, off, thr, larger_is_better, counts[lo:hi])
        if distributed:
            dist.all_reduce(counts[lo:hi], op=dist.ReduceOp.SUM, group=group)
        ops.rank_finalize(off, thr, counts[lo:hi], larger_is_better, out=ranks[lo:hi])
    return ranks, thr_all


def _rank_finalize_host(off, thr, counts, larger_is_better):
    off, thr, counts = off.cpu().tolist(), thr.cpu(), counts.cpu().to(torch.int64)
    ranks = torch.empty(len(thr), dtype=torch.int32)
    for q in range(len(off) - 1):
        for j in range(off[q], off[q + 1]):
            t = thr[off[q]:off[q + 1]]
            ranks[j] = 1 + int(counts[j]) - int(((t > thr[j]) if larger_is_better else (t < thr[j])).sum())
    return ranks


def allreduce_gradients(params, group=None, skip=None):
    """Data-parallel training: the InfoNCE loss is a SUM over queries (loss.py:57) and queries are sharded over ranks,
    so gradients simply add: one flat bucket (1.76 M fp32 = 7 MB for the MAG config), one RCCL all-reduce.
    skip: an overlapped_gradient_allreduce whose gradients were already reduced during backward."""
    done = skip.reduced if skip is not None else ()
    todo = [p for p in params if p.requires_grad and id(p) not in done]
    if not todo:
        return
    # the bucket has the same layout on every rank whatever each rank's backward produced: a parameter without a gradient here (an
    # empty shard, a branch this rank did not take) contributes zeros and receives the sum
    for p in todo:
        if p.grad is None:
            p.grad = torch.zeros_like(p)
    grads = [p.grad for p in todo]
    flat = torch.cat([g.reshape(-1) for g in grads])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    parts = flat.split([g.numel() for g in grads])
    torch._foreach_copy_(grads, [q.view_as(g) for q, g in zip(parts, grads)])      # one multi-tensor kernel


def gradient_bucket_plan(model, min_layer=1):
    """the buckets overlapped_gradient_allreduce will see, from the model alone: for every GAT layer l >= min_layer of
    `model.graph_propagate` its fc.weight / attn_l / attn_r / position-embedding table -- [(layer, [parameters])], top layer first, as
    backward announces them.  Exactly the four tensors EVERY route of ops.GATStackFunction.backward announces for a layer: the weighted
    readout's position weights (three floats, announced only by the folded route) are left to the flat bucket, so the plan holds whether
    the output layer runs folded or not.  Every rank derives the same plan, so a rank whose backward never reaches the stack can still
    issue matching collectives."""
    prop = getattr(model, "graph_propagate", None)
    layers = getattr(prop, "gat_layers", None)
    if layers is None:
        return []
    emb = getattr(prop, "prop_position_embeddings", None)
    plan = []
    L = len(layers)
    for l in range(L - 1, min_layer - 1, -1):
        ps = [layers[l].fc.weight, layers[l].attn_l, layers[l].attn_r]
        if emb is not None:
            ps.append(emb[l].weight)
        plan.append((l, ps))
    return plan


class overlapped_gradient_allreduce:
    """`with overlapped_gradient_allreduce(group, model=model) as ov: loss.backward()` -- the propagation stack's backward announces each
    layer's parameter gradients the moment they exist (ops._GRAD_READY, with the ids of their parameters); they go into one flat bucket
    per layer whose all-reduce is issued asynchronously right there, under the backward of the layers below (the output layer's 4 MB
    bucket rides under ~0.6 ms of layer-0 kernels on the MAG step), and is waited for -- by the stream, not the host -- before the
    stack hands its gradients to autograd.  `allreduce_gradients(params, skip=ov)` then reduces what is left (the first layer,
    readout, matcher).
    The collective schedule is RANK-INVARIANT when `model` is given: the buckets are planned from the model (gradient_bucket_plan) and
    go out in plan order; an announcement for a layer the plan does not hold is left to the flat bucket; a planned bucket this rank's
    backward never announced (an empty shard whose readout returned zeros without running the stack, a model that runs its layers one by
    one) is issued ON EXIT -- when .grad is final -- with what the rank holds (zeros if nothing): it receives the sum, like its peers.
    A planned layer announced out of plan order, or with other tensors than planned, cannot be reconciled mid-backward (its real gradients
    would reach autograd un-reduced while the peers' collectives go out of step) and raises.  Without `model` every rank must take the
    same route through backward.
    Not re-entrant and not thread-safe: the hooks are process-global (ops._GRAD_READY / _GRAD_FLUSH); one backward at a time."""

    def __init__(self, group=None, min_layer=1, model=None):
        self.group, self.min_layer = group, min_layer
        self.reduced, self._pending = set(), []
        self.plan = gradient_bucket_plan(model, min_layer) if model is not None else None
        self._fired = set()
        # the matcher's parameters (model.py:86) get their gradients FIRST in backward: their bucket goes out from a
        # post-accumulate hook and rides under the whole encoder backward (with the plan: rank-invariant, like the layer buckets)
        match = getattr(model, "match", None) if model is not None else None
        self._early = [p for p in match.parameters() if p.requires_grad] if match is not None else []
        self._early_done, self._hooks = False, []

    def __enter__(self):
        self._prev = (ops._GRAD_READY, ops._GRAD_FLUSH)
        ops._GRAD_READY, ops._GRAD_FLUSH = self._ready, self._flush
        if self._early:
            left = {id(p) for p in self._early}

            def hook(p):
                left.discard(id(p))
                if not left and not self._early_done:        # the last of the matcher's gradients has been accumulated
                    self._reduce_early()
            self._hooks = [p.register_post_accumulate_grad_hook(hook) for p in self._early]
        return self

    def _reduce_early(self):
        self._early_done = True
        grads = [(p.grad if p.grad is not None else torch.zeros_like(p)) for p in self._early]
        for p, g in zip(self._early, grads):
            if p.grad is None:
                p.grad = g
        flat = torch.cat([g.reshape(-1) for g in grads])
        work = dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        self._pending.append((work, flat, grads, [id(p) for p in self._early]))

    def __exit__(self, *exc):
        for h in self._hooks:
            h.remove()
        self._hooks = []
        if self._early and not self._early_done and exc[0] is None:
            self._reduce_early()                             # (a rank without a loss term: zeros, FIRST like on its peers)
        self._flush()
        ops._GRAD_READY, ops._GRAD_FLUSH = self._prev
        if self.plan is not None and exc[0] is None:
            self._issue_missing()
        return False

    def _ready(self, layer, tensors, param_ids):
        if self.plan is not None:
            want = next((ps for l, ps in self.plan if l == layer), None)
            have = {i: t for t, i in zip(tensors, param_ids) if t is not None}
            if want is None or layer in self._fired:
                return                                     # not a planned bucket: the flat bucket after backward takes it
            if any(id(p) not in have or have[id(p)].numel() != p.numel() for p in want):
                raise RuntimeError(f"overlapped_gradient_allreduce: layer {layer} announced other gradients than gradient_bucket_plan() "
                                   "holds for it -- the ranks' collectives would go out of step")
            skipped = [l for l, _ in self.plan if l > layer and l not in self._fired]
            if skipped:                                    # (buckets fire top layer first, on every rank)
                raise RuntimeError(f"overlapped_gradient_allreduce: layer {layer} announced before the planned layers {skipped} above it")
            self._fired.add(layer)
            tensors, ids = [have[id(p)] for p in want], [id(p) for p in want]
        else:
            keep = [(t, i) for t, i in zip(tensors, param_ids) if t is not None]
            if layer < self.min_layer or not keep:           # the bottom layer's gradients arrive last: nothing left to hide them under
                return
            tensors, ids = [t for t, _ in keep], [i for _, i in keep]
        flat = torch.cat([t.reshape(-1) for t in tensors])
        work = dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        self._pending.append((work, flat, tensors, ids))

    def _issue_missing(self):
        """on exit (every .grad is final): the planned buckets this rank's backward never announced, in plan order -- all-reduce whatever
        gradient the rank holds for them (zeros if none), keep the sum"""
        for l, ps in self.plan:
            if l in self._fired:
                continue
            self._fired.add(l)
            flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in ps])   # (what this rank has)
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group)
            for p, q in zip(ps, flat.split([p.numel() for p in ps])):
                p.grad = q.view_as(p).clone() if p.grad is None else p.grad.copy_(q.view_as(p))
            self.reduced.update(id(p) for p in ps)

    def _flush(self):
        for work, flat, tensors, ids in self._pending:
            work.wait()
            torch._foreach_copy_(tensors, [q.view_as(t) for q, t in zip(flat.split([t.numel() for t in tensors]), tensors)])
            self.reduced.update(ids)
        self._pending = []


# the widest k evaluate._best_parents gives to the fused rounds (<= ops.TOPK_WIDE_MAX = 64); above it the score block + select route.
# Measured (tools/topk_wide_timing.py, MAG-Full, 8,192 queries x 356 k candidates, one MI355X; profiles/NOTES.md): the rounds cost
# 22.0 / 26.1 / 35.5 / 40.1 / 53.0 / 99.8 ms at k = 9 / 16 / 17 / 24 / 32 / 64, score blocks + txe_select_k 47.4-48.4 ms at every k:
# 24 is the largest measured k at which the rounds are not the slower route.
TOPK_FUSED_MAX = 24


def host_topk_rounds(S, k, larger_is_better=True, idx_base=0):
    """the wide best-k kernels' specification in numpy, literally as they run (csrc/txe_common.h): rounds of 8 under a ceiling.  The
    order is total over (key, column) -- better key first, equal keys by ascending column; key = the score, negated when smaller is
    better, NaN as -inf -- so a row's best k are its best 8, then the best 8 among the entries strictly worse than the 8th chosen, ...
    Each round scans the row keeping a sorted list of at most 8 eligible entries (an entry enters only if it beats the list's last) and
    hands its last SLOT to the next round as the ceiling exactly as it stands: an empty slot is (-inf, INT_MAX), under which nothing is
    eligible.  S [nq, G] -> (idx int64 [nq, k] = column + idx_base, -1 behind the row's last entry; key float64 [nq, k], -inf there).
    Ceiling columns are local: idx_base is added on output only."""
    import numpy as np
    S = np.asarray(S, dtype=np.float64)
    key = S if larger_is_better else -S
    key = np.where(np.isnan(key), -np.inf, key)
    nq, G = key.shape
    k = int(k)
    EMPTY = (-np.inf, 0x7fffffff)

    def better(a, b):                                   # topk_better: (key, column) a strictly before b
        return a[0] > b[0] or (a[0] == b[0] and a[1] < b[1])
    idx, out = np.full((nq, k), -1, dtype=np.int64), np.full((nq, k), -np.inf)
    for q in range(nq):
        ceil = None                                     # first round: every entry is eligible
        for k0 in range(0, k, 8):
            kr = min(8, k - k0)
            slots = [EMPTY] * kr
            for n in range(G):
                e = (float(key[q, n]), n)
                if ceil is not None and not better(ceil, e):
                    continue
                if better(e, slots[-1]):
                    slots[-1] = e
                    t = kr - 1
                    while t > 0 and better(slots[t], slots[t - 1]):
                        slots[t - 1], slots[t] = slots[t], slots[t - 1]
                        t -= 1
            for t, (kv, n) in enumerate(slots):
                idx[q, k0 + t] = -1 if n == EMPTY[1] else n + idx_base
                out[q, k0 + t] = kv
            ceil = slots[-1]
    return idx, out


def topk_parents_fused(match, hg, queries, candidate_ids=None, k=5, larger_is_better=True, block=None, group=None, shard_lo=0, sharded=False,
                       return_scores=False):
    """infer.py:96-106 / test_fast.py:121-131 without the score matrix: per query block ONE launch of the score GEMM whose epilogue keeps
    each tile's best k columns per row (txe_score_topk_block) + a merge launch -- no [Q, G] scores, no [Q, G] index temporaries (the
    torch composite topk_parents below needs two int64 [Q, G] ones: 3.5 GB per 1,024-query block on MAG-Full).  k <= 64: above 8 the
    selection runs in ceil(k / 8) rounds of 8 under a ceiling (txe_score_topk_wide_block; host_topk_rounds states them), one pass of the
    score tiles per round, still without a score block.  Same selection and
    order as topk_parents on the materialised scores of the same kernel (bit-identical values): better score first, ties by ascending
    candidate position (Python's stable sort), NaN last.  match: BIM / LBM / MLP / NTN.  hg: this rank's candidate rows (positions
    [shard_lo, shard_lo + len) of the global list).  Candidate-sharded (ONLY when asked: `group` given or sharded=True, _sharded_call
    -- every rank then holds a DISJOINT slice, which the merge relies on): every rank's [Q, k] lists
    are all-gathered (k * 8 bytes per query instead of the [queries x candidates] block) and merged by the same kernel.
    Returns candidate_ids[...] (or the positions themselves when candidate_ids is None) [Q, min(k, G)].
    return_scores: (ids, scores) -- scores fp32 [Q, min(k, G)] = the matcher's own values of the chosen pairs, un-negated, bit-equal to
    score_all's entries (a NaN score, which ranks last, is reported as the worst value: -inf, or +inf when smaller is better)."""
    dev = hg.device
    distributed = _sharded_call(group, sharded)
    Q, G = queries.shape[0], hg.shape[0]
    k_loc = min(int(k), G, ops.TOPK_WIDE_MAX)
    assert int(k) <= ops.TOPK_WIDE_MAX, "topk_parents_fused: k <= 64 (rounds of 8 under a ceiling; wider lists: score blocks + ops.select_k)"
    if block is None:
        block = _default_block(Q)
    outs = []
    if k_loc > 0 and Q > 0:
        pm = prepare_matcher(match, hg)
        Qp = pm.queries(queries)
        scratch = {}
        for q0 in range(0, Q, block):
            outs.append(pm.topk(Qp[q0:q0 + block], k_loc, larger_is_better, shard_lo, scratch))
    if outs:
        idx, key = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    else:
        idx = torch.full((Q, 0), 0, dtype=torch.int32, device=dev)
        key = torch.zeros((Q, 0), dtype=torch.float32, device=dev)
    if distributed:
        world = dist.get_world_size(group)
        kk = min(int(k), ops.TOPK_WIDE_MAX)
        # every rank contributes kk slots per query (a rank with fewer candidates pads with empty slots)
        pad_i = torch.full((Q, kk), 0x7fffffff, dtype=torch.int32, device=dev)
        pad_k = torch.full((Q, kk), -float("inf"), dtype=torch.float32, device=dev)
        pad_i[:, :idx.shape[1]] = torch.where(idx >= 0, idx, torch.full_like(idx, 0x7fffffff))
        pad_k[:, :key.shape[1]] = key
        all_i = torch.empty((world, Q, kk), dtype=torch.int32, device=dev)
        all_k = torch.empty((world, Q, kk), dtype=torch.float32, device=dev)
        dist.all_gather_into_tensor(all_i.view(world * Q, kk), pad_i, group=group)
        dist.all_gather_into_tensor(all_k.view(world * Q, kk), pad_k, group=group)
        cat_i = all_i.permute(1, 0, 2).reshape(Q, world * kk).contiguous()
        cat_k = all_k.permute(1, 0, 2).reshape(Q, world * kk).contiguous()
        n_real = int((cat_i[0] != 0x7fffffff).sum().item()) if Q > 0 else 0      # = min(total candidates, world * kk): the same for every query
        idx, key = ops.topk_merge(cat_k, cat_i, kk) if Q > 0 else (cat_i, cat_k)
        idx = idx[:, :min(kk, n_real)]
    ids = idx.long() if candidate_ids is None else candidate_ids.to(dev)[idx.long()]
    if not return_scores:
        return ids
    key = key[:, :idx.shape[1]]
    return ids, (key if larger_is_better else -key)


# ---------------------------------------------------------------------------------------------------------------
# retrieval stage (data_loader/dataset.py:316-330): the k unmasked candidates nearest to a query by cosine distance
# ---------------------------------------------------------------------------------------------------------------
RETRIEVE_K_MAX = 4096                        # ops.SELECT_K_MAX: the select kernel keeps its survivors in LDS
RETRIEVE_BLOCK_BYTES = 256 * 2 ** 20         # one [block, G] similarity block stays at or below this


def _retrieve_args(k, mask_off, mask_idx, n_queries=None, n_candidates=None):
    """the argument rules of retrieve_candidates / host_retrieve / host_select_k, checked before anything runs; the masks come back as
    host int64 arrays (or None, None)"""
    import numpy as np
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= RETRIEVE_K_MAX:
        raise ValueError(f"retrieval: 1 <= k <= {RETRIEVE_K_MAX}, got {k!r}")
    if (mask_off is None) != (mask_idx is None):
        raise ValueError("retrieval: masks are a CSR -- mask_off [Q + 1] and mask_idx go together")
    if mask_off is None:
        return int(k), None, None
    off = np.asarray(torch.as_tensor(mask_off).cpu(), dtype=np.int64).reshape(-1)
    idx = np.asarray(torch.as_tensor(mask_idx).cpu(), dtype=np.int64).reshape(-1)
    if n_queries is not None and off.shape[0] != n_queries + 1:
        raise ValueError(f"retrieval: mask_off holds {off.shape[0]} entries for {n_queries} queries (Q + 1 wanted)")
    if off.shape[0] < 1 or off[0] != 0 or np.any(np.diff(off) < 0) or off[-1] != idx.shape[0] or idx.shape[0] >= 2 ** 31:
        raise ValueError("retrieval: mask_off must rise from 0 to len(mask_idx)")
    if n_candidates is not None and idx.size and (idx.min() < 0 or idx.max() >= n_candidates):
        raise ValueError("retrieval: mask_idx names a column outside the candidates")
    return int(k), off, idx


def host_select_k(S, k, mask_off=None, mask_idx=None):
    """numpy restatement of txe_select_k: per row of S the k unmasked columns with the largest value, best first, equal values by
    ascending column, NaN last (as -inf); int32 [nq, k], -1 where fewer than k unmasked columns exist.  S is compared in the dtype
    it comes in."""
    import numpy as np
    S = np.asarray(S)
    k, off, idx = _retrieve_args(k, mask_off, mask_idx, S.shape[0], S.shape[1])
    out = np.full((S.shape[0], k), -1, dtype=np.int32)
    for q in range(S.shape[0]):
        keep = np.ones(S.shape[1], dtype=bool)
        if off is not None:
            keep[idx[off[q]:off[q + 1]]] = False                 # masks applied by list
        cols = np.flatnonzero(keep)
        key = S[q, cols].astype(np.float64)
        key[np.isnan(key)] = -np.inf
        best = cols[np.argsort(-key, kind="stable")[:k]]          # stable: equal keys (-0.0 == +0.0 too) keep ascending column order
        out[q, :len(best)] = best
    return out


def host_retrieve(query_features, candidate_features, k, mask_off=None, mask_idx=None, block=None):
    """retrieve_candidates on the host, in float64 (the sampler.host_draw pattern: the tests' reference and any CPU caller's route):
    cosine similarities of the normalised rows, masks applied by list, best first, exact ties by ascending candidate row, NaN last.
    `block` is accepted for symmetry and changes nothing."""
    import numpy as np
    Qf = np.asarray(torch.as_tensor(query_features).detach().cpu(), dtype=np.float64)
    Cf = np.asarray(torch.as_tensor(candidate_features).detach().cpu(), dtype=np.float64)
    k, off, idx = _retrieve_args(k, mask_off, mask_idx, Qf.shape[0], Cf.shape[0])
    if Cf.shape[0] == 0 or Qf.shape[0] == 0:
        return np.full((Qf.shape[0], k), -1, dtype=np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        Qn = Qf / np.linalg.norm(Qf, axis=1, keepdims=True)
        Cn = Cf / np.linalg.norm(Cf, axis=1, keepdims=True)
        S = Qn @ Cn.T
    return host_select_k(S, k, off, idx)


def retrieve_candidates(query_features, candidate_features, k, mask_off=None, mask_idx=None, block=None):
    """The retrieval stage of the reference's two-stage test protocol (data_loader/dataset.py:316-330, `-k` of test_fast.py / infer.py) on
    the device: idx int32 [Q, k] = for every query the k candidate rows nearest by cosine distance that its mask list does not name,
    nearest first, -1 where fewer than k unmasked candidates exist.  mask_off [Q + 1] / mask_idx: CSR of masked candidate rows per query
    (any order, duplicates allowed); both None: nothing is masked.
    Rows are normalised once (txe_row_normalize), a block of queries is one score GEMM without exp (the fp32-accurate bf16-pipe product
    of the scoring loop) and one masked select-k launch (txe_select_k).  block: queries per launch; default: as many as keep the
    [block, G] similarity block at or below 256 MB -- a [Q, G] matrix for all queries is never allocated.
    Deviations from the reference: exact distance ties break by ascending candidate row (the reference: iteration order of a Python set),
    and the selection runs on fp32 similarities of normalised rows, not on numpy's 1 - cos: the same order wherever two distances differ
    by more than fp32 rounding.  ValueError (before any launch): k < 1, k > 4096, masks without offsets or offsets without masks."""
    G = int(candidate_features.shape[0])
    Q = int(query_features.shape[0])
    k, off, idx = _retrieve_args(k, mask_off, mask_idx, Q, G)
    ops._need_cuda(query_features, candidate_features)
    dev = candidate_features.device
    out = torch.full((Q, k), -1, dtype=torch.int32, device=dev)
    if Q == 0 or G == 0:
        return out
    Cn = ops.normalized_rows(candidate_features)
    Qn = ops.normalized_rows(query_features, pack=False).full
    ld = (G + 3) // 4 * 4
    if block is None:
        block = RETRIEVE_BLOCK_BYTES // (4 * ld)
    block = max(1, min(int(block), Q))
    moff = midx = None
    if off is not None and idx.size:
        moff = torch.as_tensor(off, dtype=torch.int32).to(dev, non_blocking=True)
        midx = torch.as_tensor(idx, dtype=torch.int32).to(dev, non_blocking=True)
    S = torch.empty((block, ld), dtype=torch.float32, device=dev)
    for q0 in range(0, Q, block):
        q1 = min(q0 + block, Q)
        Sb = ops.cosine_block(Qn[q0:q1], Cn, S[:q1 - q0, :G])
        ops.select_k(Sb, k, None if moff is None else moff[q0:q1 + 1], midx, out=out[q0:q1])
    return out


def topk_parents(S, candidate_ids, k=5, larger_is_better=True):
    """infer.py:100-106 / test_fast.py:125-131: the k best candidate positions per query -- `sorted(enumerate(scores), key=-score)[:k]`
    (descending score for info_nce, ascending otherwise).  Python's sort is stable, so equal scores come out in ascending candidate
    order, and that is what this returns (torch.topk alone leaves the order of ties unspecified): the strictly better candidates,
    then the lowest-index members of the tie group at the k-th value.  S [Q, G] -> candidate_ids[...] [Q, min(k, G)]."""
    Q, G = S.shape
    k = min(int(k), G)
    if k == 0 or Q == 0:
        return candidate_ids.new_zeros((Q, 0)).to(S.device)
    key = S if larger_is_better else -S
    # a NaN score compares false with everything: Python's sorted() leaves it wherever it happens to stand, here it ranks last (and the
    # selection below never indexes past the row: without this a row holding a NaN selected only filler columns)
    key = torch.where(torch.isnan(key), torch.full_like(key, -float("inf")), key)
    vk = torch.topk(key, k, dim=1).values[:, -1:]                                     # the k-th best value of each row
    ar = torch.arange(G, device=S.device).expand(Q, G)
    fill = torch.full_like(ar, G)
    better = torch.topk(torch.where(key > vk, ar, fill), k, dim=1, largest=False).values     # <= k-1 real columns, ascending, then G
    tied = torch.topk(torch.where(key == vk, ar, fill), k, dim=1, largest=False).values      # lowest k columns of the tie group
    cand = torch.cat([better, tied], 1)                                                       # [Q, 2k], fillers = G
    ckey = torch.where(cand < G, torch.gather(key, 1, cand.clamp(max=G - 1)), torch.full((), -float("inf"), device=S.device, dtype=key.dtype))
    # order by (key descending, column ascending): columns are ascending inside each half; one stable sort by column, one by key
    o1 = torch.sort(cand, dim=1, stable=True).indices
    cand, ckey = torch.gather(cand, 1, o1), torch.gather(ckey, 1, o1)
    o2 = torch.sort(ckey, dim=1, descending=True, stable=True).indices
    idx = torch.gather(cand, 1, o2)[:, :k].clamp(max=G - 1)
    return candidate_ids.to(idx.device)[idx]
