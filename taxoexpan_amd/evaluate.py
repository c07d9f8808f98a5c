"""All-candidate evaluation (test_fast.py:82-225) and inference on new terms (infer.py:77-159) on the MI355X path, end to end on
device: egonets of every candidate position built by `txe_egonet_*`, the encoder in one batch (`-b -1`) or in chunks of `-b`
egonets, then fused scoring + ranking with the reference's per-query metric aggregation (`evaluate`), or the top-5 parents of every
new term (`infer`)."""
import numpy as np
import torch

from .graph import device_egonet_batch
from . import scoring
from .scoring import (_retrieve_args, encode_candidates, fused_matcher_ok, log_partition_fused, prepare_matcher, rank_all_fused,
                      retrieve_candidates, topk_parents, topk_parents_fused)


def candidate_graphs(dtax, anchors, expand_factor, seed, batch_size=-1):
    """the candidate egonets `_get_subgraph(-1, anchor, 0)` of test_fast.py:93-97 / infer.py:80-82 as one device-built batch
    (batch_size == -1: the scripts' small mode) or as chunks of batch_size egonets (`-b`, test_fast.py:149-179 / infer.py:108-139)"""
    anchors = np.asarray(anchors, dtype=np.int64)
    if batch_size is None or batch_size <= 0 or batch_size >= len(anchors):
        return device_egonet_batch(dtax, anchors, expand_factor=expand_factor, seed=seed, with_features="lazy")
    return [device_egonet_batch(dtax, anchors[i:i + batch_size], expand_factor=expand_factor, seed=seed, with_features="lazy", index_base=i)
            for i in range(0, len(anchors), batch_size)]


def _per_query_means(values, pos_off):
    """mean over queries of the mean of `values` over the query's positives"""
    off = torch.as_tensor(pos_off).to(device=values.device, dtype=torch.int64)
    cnt = off[1:] - off[:-1]
    qid = torch.repeat_interleave(torch.arange(cnt.numel(), device=values.device), cnt)
    sums = torch.zeros(cnt.numel(), dtype=torch.float64, device=values.device).index_add_(0, qid, values.to(torch.float64))
    return float((sums / cnt.to(torch.float64)).mean().item())


CASE_METRICS = ("macro_mr", "micro_mr", "hit_at_1", "hit_at_3", "hit_at_5", "mrr_scaled_10")     # config.mag.json "metrics"


def _score_blocks(model, hg, qf, qblock):
    """score blocks [<= qblock queries, G candidates] of the per-query loop test_fast.py:121-123 / infer.py:96-98: the prepared matcher's
    block kernel for BIM / LBM / MLP / NTN (scoring.prepare_matcher), the literal expand loop for any other matcher"""
    pm = None
    for q0 in range(0, qf.shape[0], qblock):
        if fused_matcher_ok(model.match):
            pm = prepare_matcher(model.match, hg) if pm is None else pm
            yield q0, pm.score(qf[q0:q0 + qblock])
        else:
            yield q0, torch.stack([model.match(hg, q.expand(hg.shape[0], -1)).reshape(-1) for q in qf[q0:q0 + qblock]])


def _best_parents(model, hg, qf, cand_ids, topk, larger_is_better, qblock, with_scores=False):
    """the `topk` best candidates of every query, best first (infer.py:100-106 / test_fast.py:125-131).  BIM / LBM / MLP / NTN: up to
    scoring.TOPK_FUSED_MAX through the fused score + select kernels (no score matrix; above 8 in rounds of 8 under a ceiling); above
    that and up to 4,096 the retrieval stage's kernels on model scores -- score blocks of at most scoring.RETRIEVE_BLOCK_BYTES, then
    ops.select_k (the same order: ties by ascending column, NaN last; no [Q, G] index temporaries).  Anything else (a wider list, a
    matcher without a fused route) by materialising score blocks for the torch composite topk_parents.
    with_scores: (ids, fp32 scores of the chosen pairs -- the matcher's own values; on the first two routes a NaN score, which ranks
    last, is reported as the worst value)"""
    from . import ops
    fused = fused_matcher_ok(model.match) and hg.shape[0] > 0 and qf.shape[0] > 0
    if fused and 1 <= topk <= scoring.TOPK_FUSED_MAX:
        return topk_parents_fused(model.match, hg, qf, cand_ids, topk, larger_is_better, block=qblock, return_scores=with_scores)
    if fused and topk <= ops.SELECT_K_MAX:
        G = hg.shape[0]
        kk = min(int(topk), G)
        pm = prepare_matcher(model.match, hg)
        block = max(1, min(qf.shape[0], scoring.RETRIEVE_BLOCK_BYTES // (4 * G)))
        pitch = (G + 3) // 4 * 4                                           # 16-byte row pitch, as score_block's own blocks
        S = torch.empty((block, pitch), dtype=torch.float32, device=hg.device)
        top, sc = [], []
        for q0 in range(0, qf.shape[0], block):
            qb = qf[q0:q0 + block]
            Sb = pm.score(qb, out=S[:qb.shape[0], :G])
            if not larger_is_better:
                Sb.neg_()
            idx, key = ops.select_k(Sb, kk, want_keys=True)
            top.append(cand_ids.to(idx.device)[idx.long()])
            sc.append(key if larger_is_better else -key)
        ids = torch.cat(top)
        return (ids, torch.cat(sc)) if with_scores else ids
    top, sc = [], []
    cols = torch.arange(hg.shape[0], device=hg.device)
    for _q0, S in _score_blocks(model, hg, qf, qblock or 1024):
        pos = topk_parents(S, cols, topk, larger_is_better)
        top.append(cand_ids.to(pos.device)[pos])
        sc.append(torch.gather(S, 1, pos).float())
    ids = torch.cat(top) if top else cand_ids.new_zeros((0, 0))
    if not with_scores:
        return ids
    return ids, (torch.cat(sc) if sc else torch.zeros((0, 0), dtype=torch.float32, device=hg.device))


def _ranks_of(model, hg, qf, pos_off, pos_idx, larger_is_better, qblock, with_thr=False):
    """ranks of every query's true parents: fused (no score matrix) for BIM / LBM / MLP / NTN; any other matcher materialises score blocks with
    the literal loop and ranks them on device (ops.rank_block).  with_thr: (ranks, the positives' own scores fp32 [n_positives])"""
    from . import ops
    if fused_matcher_ok(model.match):
        return rank_all_fused(model.match, hg, qf, pos_off, pos_idx, block=qblock, larger_is_better=larger_is_better, return_thresholds=with_thr)
    off = np.asarray(pos_off, dtype=np.int64)
    idx = np.asarray(pos_idx, dtype=np.int64)
    out, thr = [], []
    for q0, S in _score_blocks(model, hg, qf, qblock or 1024):
        q1 = q0 + S.shape[0]
        lo, hi = int(off[q0]), int(off[q1])
        if hi > lo:
            out.append(ops.rank_block(S.contiguous(), torch.from_numpy(off[q0:q1 + 1] - lo), torch.from_numpy(idx[lo:hi]), larger_is_better))
            if with_thr:
                rows = torch.from_numpy(np.repeat(np.arange(q1 - q0), np.diff(off[q0:q1 + 1]))).to(S.device)
                thr.append(S[rows, torch.from_numpy(idx[lo:hi]).to(S.device)].float())
    ranks = torch.cat(out) if out else torch.zeros(0, dtype=torch.int32, device=hg.device)
    if not with_thr:
        return ranks
    return ranks, (torch.cat(thr) if thr else torch.zeros(0, dtype=torch.float32, device=hg.device))


def _nll_of(lse, thr, pos_off, larger_is_better):
    """mean over queries of the mean over the query's positives j of lse[q] - z_j, z_j = the positive's score (or its negative), in
    float64 on the device from the fp32 operands"""
    off = torch.as_tensor(pos_off).to(device=lse.device, dtype=torch.int64)
    qid = torch.repeat_interleave(torch.arange(off.numel() - 1, device=lse.device), off[1:] - off[:-1])
    z = thr.to(torch.float64)
    return _per_query_means(lse.to(torch.float64)[qid] - (z if larger_is_better else -z), pos_off)


def _scaled(s, beta, larger_is_better):
    """t = fl32(beta * z) of fp32 scores s as the moments kernels form it (one fp32 product; z = s or its negative), in float64"""
    z = s.float() if larger_is_better else -s.float()
    return (z * torch.tensor(beta, dtype=torch.float32, device=s.device)).to(torch.float64)


def _predictive(model, hg, qf, mom, ranks, pos_off, beta, larger_is_better, qblock):
    """evaluate's `predictive` metrics from the moments of every query's distribution and its first predicted parent: (entropy /
    confidence / ece floats, the per-query device tensors)"""
    from .calibrate import _ece_device
    dev = hg.device
    cols = torch.arange(hg.shape[0], device=dev)
    _ids, top = _best_parents(model, hg, qf, cols, 1, larger_is_better, qblock, with_scores=True)
    top1_prob = torch.exp(_scaled(top[:, 0], beta, larger_is_better) - mom.lse)
    off = torch.as_tensor(pos_off).to(device=dev, dtype=torch.int64)
    Q = off.numel() - 1
    qid = torch.repeat_interleave(torch.arange(Q, device=dev), off[1:] - off[:-1])
    best = torch.full((Q,), 2 ** 31 - 1, dtype=torch.int32, device=dev).scatter_reduce_(0, qid, ranks.to(torch.int32), "amin")
    correct = best == 1
    vals = torch.stack([mom.entropy.mean(), top1_prob.mean(), _ece_device(top1_prob, correct)]).cpu().tolist()
    return dict(entropy=vals[0], confidence=vals[1], ece=vals[2]), \
        dict(lse=mom.lse, mean=mom.mean, var=mom.var, entropy=mom.entropy, top1_prob=top1_prob, correct=correct)


def _retrieval_masks(dataset, queries, index):
    """node2masks[q] (descendants, parents, q itself, roots: dataset.py:262-268) as candidate rows, CSR over the queries"""
    off, idx = [0], []
    for q in queries:
        idx.extend(sorted(index[a] for a in dataset.node2masks[q] if a in index))
        off.append(len(idx))
    return np.asarray(off, dtype=np.int64), np.asarray(idx, dtype=np.int64)


def _retrieved_groups(model, hg, qf, pos_off, pos_idx, ridx, larger_is_better, qblock):
    """the retrieve-then-rank instances of dataset.py:316-330 as one labelled score vector: per query its positives (label 1) followed by
    its k retrieved candidate rows `ridx` (label 0; a -1 slot scores worst, so it never counts against a positive).  Only these pairs
    are scored: the prepared matcher's gathered route for BIM / LBM / MLP / NTN, model.match on the gathered rows for anything else.
    Returns (score [B] fp32, label [B] int32, ret_dst [Q, k] = where each retrieved slot sits in them)."""
    dev = hg.device
    Q, k = ridx.shape
    pos_off = np.asarray(pos_off, dtype=np.int64)
    cnt = np.diff(pos_off)
    n_pos = int(pos_off[-1])
    goff_h = pos_off + np.arange(Q + 1, dtype=np.int64) * k
    B = int(goff_h[-1])
    if B >= 2 ** 31:
        raise ValueError("retrieve: positives + queries x k must stay below 2^31 pairs")
    up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev, non_blocking=True)
    pos_dst = up(np.arange(n_pos, dtype=np.int64) + np.repeat(np.arange(Q, dtype=np.int64), cnt) * k, torch.int64)
    ret_dst = up((goff_h[:-1] + cnt)[:, None] + np.arange(k, dtype=np.int64)[None, :], torch.int64)
    rows = torch.empty(B, dtype=torch.int64, device=dev)
    rows[pos_dst] = up(pos_idx, torch.int64)
    rows[ret_dst.reshape(-1)] = ridx.reshape(-1).clamp(min=0).long()
    label = torch.zeros(B, dtype=torch.int32, device=dev)
    label[pos_dst] = 1
    score = torch.empty(B, dtype=torch.float32, device=dev)
    block = max(1, min(int(qblock) if qblock else 1024, Q, max(1, 2 ** 20 // (k + 1))))     # <= ~1 M gathered candidate rows per block
    fused = fused_matcher_ok(model.match)
    if fused:
        pm = prepare_matcher(model.match, hg)
        Qp = pm.queries(qf)
        goff = up(goff_h, torch.int32)
    else:
        qid = up(np.repeat(np.arange(Q, dtype=np.int64), cnt + k), torch.int64)
    for q0 in range(0, Q, block):
        q1 = min(q0 + block, Q)
        lo, hi = int(goff_h[q0]), int(goff_h[q1])
        if fused:
            pm.positives(Qp[q0:q1], goff[q0:q1 + 1] - lo, rows[lo:hi], score[lo:hi])
        else:
            score[lo:hi] = model.match(hg[rows[lo:hi]], qf[qid[lo:hi]]).reshape(-1)
    flat = ret_dst.reshape(-1)
    worst = torch.full((), -float("inf") if larger_is_better else float("inf"), device=dev)
    score[flat] = torch.where(ridx.reshape(-1) < 0, worst, score[flat])
    return score, label, ret_dst


def _best_retrieved(score, ret_dst, ridx, topk, larger_is_better):
    """the `topk` best of every query's retrieved rows by matcher score, best first, equal scores by ascending candidate row, NaN last
    (the order of topk_parents): int32 [Q, min(topk, k)] candidate rows, -1 where fewer were retrieved"""
    from . import ops
    key = score[ret_dst]
    key = key if larger_is_better else -key
    key = torch.where(torch.isnan(key), torch.full_like(key, -float("inf")), key).contiguous()
    empty = 0x7fffffff
    idx = torch.where(ridx >= 0, ridx, torch.full_like(ridx, empty)).contiguous()
    kk = min(int(topk), idx.shape[1])
    if idx.shape[0] == 0 or kk < 1:
        return idx[:, :0]
    if kk <= ops.TOPK_WIDE_MAX:                                             # (above 8: the same merge in rounds of 8 under a ceiling)
        return ops.topk_merge(key, idx, kk)[0]
    o1 = torch.sort(idx, dim=1, stable=True).indices                       # columns ascending (empty slots last), then keys descending
    idx, key = torch.gather(idx, 1, o1), torch.gather(key, 1, o1)
    o2 = torch.sort(key, dim=1, descending=True, stable=True).indices
    idx = torch.gather(idx, 1, o2)[:, :kk]                                  # (an empty slot: key -inf, the largest column -- last)
    return torch.where(idx == empty, torch.full_like(idx, -1), idx)


def _case_rows(dataset, queries, pos_off, ranks, top, metric_names, per_query_values=None):
    """the case-study table of test_fast.py:112-147: per test query its name, true parents, predicted top-5 parents and every
    metric evaluated on that query's ranks alone (`metric([ranks])`, model/metric.py:62-90), as strings.
    per_query_values: {name: one value per query} for the columns that are not functions of the ranks ("wu_palmer")"""
    r = ranks.cpu().to(torch.float64).numpy()
    extra = per_query_values or {}
    per_query = {
        "macro_mr": lambda x: float(x.mean()), "micro_mr": lambda x: float(x.mean()),
        "hit_at_1": lambda x: float(1.0 * np.sum(x <= 1) / len(x)), "hit_at_3": lambda x: float(1.0 * np.sum(x <= 3) / len(x)),
        "hit_at_5": lambda x: float(1.0 * np.sum(x <= 5) / len(x)), "mrr_scaled_10": lambda x: float((1.0 / np.ceil(x / 10)).mean()),
    }
    vocab = dataset.vocab
    rows = [["Test node index", "True parents", "Predicted parents"] + list(metric_names)]
    for i, q in enumerate(queries):
        x = r[pos_off[i]:pos_off[i + 1]]
        rows.append([vocab[q], ", ".join(vocab[p] for p in dataset.node2parents[q]), ", ".join(vocab[p] for p in top[i])] +
                    [str(float(extra[m][i])) if m in extra else str(per_query[m](x)) for m in metric_names])
    return rows


def _taxonomic(index_dev, best, pos_off, gold_idx, Q):
    """the taxonomy-aware evaluation of the best lists `best` [Q, K] (node ids, -1 = no prediction) against the gold parents
    `gold_idx` under `pos_off`: (scalar metrics, dict of the [Q, K] device tensors)"""
    from . import taxometric
    dev = index_dev.device
    if Q == 0 or best.shape[1] == 0:
        empty = torch.zeros((Q, 0), dtype=torch.int32, device=dev)
        return taxometric.summarize(empty, empty.to(torch.float64)), dict(pred=empty, lca_depth=empty, best_gold=empty, relation=empty,
                                                                           wu_palmer=empty.to(torch.float64))
    pred = best.to(torch.int32).contiguous()
    out = taxometric.taxonomic_slots(index_dev, pred, pos_off, gold_idx)
    node = taxometric.best_gold_nodes(out["best_gold"], pos_off, gold_idx)
    wup = taxometric.wu_palmer(index_dev, pred, node, out["lca_depth"])
    return taxometric.summarize(out["relation"], wup), dict(pred=pred, wu_palmer=wup, **out)


def _hedged(model, hg, qf, tindex, cand, pos_off, pos_idx, thr, beta, larger_is_better, lse):
    """evaluate's `hedge` metrics: the hedged parent of every query per threshold (hedge.hedged_parents) judged against the query's gold
    parents by taxometric.taxonomic_slots -- the T thresholds are the T slots of one [Q, T] list, one launch.  Returns (metric lists, the
    [Q, T] device tensors)"""
    from . import hedge as _hedge, taxometric
    dev = hg.device
    Q, T = int(qf.shape[0]), len(thr)
    cand_np = np.asarray(cand, dtype=np.int64)
    hix = _hedge.HedgeIndex.build(tindex, cand_np).to(dev)
    h = _hedge.hedged_parents(model.match, hg, qf, hix, thr, 1.0 / beta, larger_is_better, lse=lse)
    nan = [float("nan")] * T
    if Q == 0:
        return dict(hedge_thresholds=list(thr), hedge_accuracy=nan, hedge_exact=list(nan), hedge_wu_palmer=list(nan), hedge_depth=list(nan),
                    hedge_mass=list(nan), hedge_none=list(nan)), dict(node_col=h.node_col, mass=h.mass, depth=h.depth)
    cand_ids = torch.as_tensor(cand_np, device=dev)
    answered = h.node_col >= 0
    node = torch.where(answered, cand_ids[h.node_col.long().clamp(min=0)], torch.full_like(h.node_col, -1, dtype=torch.int64)) \
        if len(cand) else torch.full_like(h.node_col, -1, dtype=torch.int64)
    _m, t = _taxonomic(tindex, node, pos_off, cand_np[pos_idx], Q)
    rel = t["relation"]
    n_ans = answered.sum(0).to(torch.float64)
    sums = torch.stack([((rel == taxometric.EXACT) | (rel == taxometric.ANCESTOR)).sum(0).to(torch.float64),
                        (rel == taxometric.EXACT).sum(0).to(torch.float64), t["wu_palmer"].sum(0), h.depth.sum(0).to(torch.float64),
                        torch.where(answered, h.mass, torch.zeros_like(h.mass)).sum(0), n_ans]).cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        metrics = dict(hedge_thresholds=list(thr), hedge_accuracy=(sums[0] / Q).tolist(), hedge_exact=(sums[1] / Q).tolist(),
                       hedge_wu_palmer=(sums[2] / Q).tolist(), hedge_depth=(sums[3] / Q).tolist(), hedge_mass=(sums[4] / sums[5]).tolist(),
                       hedge_none=((Q - sums[5]) / Q).tolist())
    return metrics, dict(node=node, node_col=h.node_col, mass=h.mass, depth=h.depth, relation=rel, wu_palmer=t["wu_palmer"])


def evaluate(model, dataset, device, larger_is_better=True, qblock=None, seed=0, batch_size=-1, case=None, metric_names=CASE_METRICS,
             topk=5, retrieve=None, nll=False, taxonomic=False, taxonomy_index=None, temperature=None, predictive=False, hedge=None):
    """dataset: taxoexpan_amd.dataset.MaskedGraphDataset in 'validation' or 'test' mode.  Returns (metrics dict, ranks int32
    [n_positives], pos_off [Q+1], queries list).  Queries whose true parents are not candidate positions are skipped, like the
    reference's rearrange() would fail on them.
    case: test_fast.py's `-c` -- a path (the TSV of :142-147 is written) or a list (the rows are appended): per query its name, true
    parents, the `topk` predicted parents (best first: descending score when larger_is_better, i.e. the info_nce losses, ascending
    otherwise; ties in candidate order like Python's stable sort) and the metrics of `metric_names` on that query alone.
    topk: any size.  For BIM / LBM / MLP / NTN no [queries x candidates] index temporaries are made up to 4,096: up to
    scoring.TOPK_FUSED_MAX the list comes from the fused kernels (no score matrix either; above 8 in rounds of 8 under a ceiling), above
    it from score blocks + ops.select_k (_best_parents).  The order is the same on every route.
    retrieve: None = every positive against ALL candidates, unmasked (test_fast.py; `dataset.test_topk` is ignored).  retrieve=k
    (1 <= k <= 4096, else ValueError before any launch) = the retrieve-then-rank protocol of dataset.py:316-330 (`-k`): a query's
    instance is its true parents plus the k candidates nearest to it by cosine distance of `dataset.node_features` among those
    node2masks[q] does not name (scoring.retrieve_candidates); only those pairs are scored, a rank is 1 + the retrieved candidates
    strictly better (metric.obtain_ranks' grouped ranking), `case` lists the best `topk` of the retrieved rows only, and the metrics
    dict gains n_retrieved = k.  Deviations from the reference: exact distance ties break by ascending candidate id (there: the
    iteration order of a Python set), and the selection compares fp32 similarities of normalised rows instead of numpy's 1 - cos.
    nll=True: metrics["nll"] = the exact negative log-likelihood of the true parents against ALL candidates -- the mean over queries
    of the mean over the query's positives j of lse[q] - z_j, lse[q] = log sum_g exp(z(q, g)) (scoring.log_partition_fused: one more
    pass over the candidates, no score matrix), z = the score when larger_is_better, else its negative; the full-partition value of
    what info_nce_loss (loss.py:52-57) estimates from sampled negatives.  Formed in float64 from the fp32 lse and the fp32 scores of
    the positives the ranks were counted against.  Non-finite values propagate: a NaN or +-Inf score of a positive or in a query's row
    makes that query's term, and so the mean, NaN or +-Inf.  Not with retrieve=k (ValueError before any launch): a partition over a
    retrieved subset is not the likelihood.  With nll=False the dict, the ranks and the offsets are what they were without it.
    taxonomic: truthy (True, or a dict -- an empty one too) = also judge the best `topk` list of every query (the list `case` shows:
    _best_parents, or _best_retrieved with retrieve=k, computed once for both) on the masked taxonomy `dataset.graph.pred`
    (taxometric.py; one more launch, csrc/txe_taxometric.hip).  Gold = the query's true parents among the candidates, the
    ones the ranks are counted for.  The metrics dict gains wu_palmer (mean over queries of Wu & Palmer similarity between the first
    prediction and the gold parent nearest to it), wu_palmer_at_k (the best value in the list), taxonomic_k (the list's length) and
    rel_exact / rel_ancestor / rel_descendant / rel_sibling / rel_related / rel_unrelated / rel_none: the shares of queries by the first
    prediction's relation to that gold (too general, too specific, ...; rel_none: no prediction, an empty retrieved slot).  A dict is
    also filled with the [Q, K] device tensors pred (node ids), lca_depth, best_gold, relation, wu_palmer.  taxonomy_index: a
    taxometric.TaxonomyIndex of that taxonomy (or its .to(device)) to reuse; default TaxonomyIndex.from_dataset(dataset).  "wu_palmer"
    in `metric_names` adds the first prediction's value as a per-query column of the case study (ValueError before any launch without
    `taxonomic`).  Every other metric, the ranks and the offsets are bit-equal to a call without it.
    temperature=T (finite and > 0, else ValueError before any launch; calibrate.fit_temperature finds it on the validation split): the
    predictive distribution is p = softmax(t) over ALL candidates, t = fl32(z / T) (scoring.score_moments_fused: one pass
    over the candidates, no score matrix), and nll=True reports the NLL under it -- calibrate's f(1 / T), the true parents' terms taken
    as their own t.  predictive: truthy (True, or a dict -- an empty one too) = three more metrics of that distribution (at T = 1 without
    `temperature`): entropy = the mean over queries of H(p); confidence = the mean probability of the first predicted parent,
    exp(t_top - lse); ece = the expected calibration error of that probability over 10 equal-width bins (the sum of share x |accuracy -
    mean confidence|; accurate = the query's best rank is 1).  A dict is also filled with the per-query device tensors lse, mean, var,
    entropy, top1_prob (float64 [Q]) and correct (bool [Q]).  Neither goes with retrieve=k (ValueError before any launch).  Ranks,
    offsets and every other metric are bit-equal to a call without the two keywords -- nll too while `temperature` is None (it stays on
    log_partition_fused's fp32 lse then) --; without both the code path is what it was.
    hedge: a threshold, a sequence of at most hedge.MAX_THRESHOLDS of them (each finite and in (0, 1]), or a dict {"thresholds": ...} =
    also answer every query with the DEEPEST candidate whose subtree probability reaches the threshold (hedge.py; Deng et
    al. 2012) under p = softmax(t) over ALL candidates at `temperature` (T = 1 without it), on the masked taxonomy (`taxonomy_index`, built
    once and shared with `taxonomic`).  The metrics dict gains, one entry per threshold and in their order, the lists hedge_thresholds,
    hedge_accuracy (the share of queries whose hedged node is a gold parent or an ancestor of one: relations exact / ancestor of
    taxometric.taxonomic_slots), hedge_exact, hedge_wu_palmer, hedge_depth (the mean depth over all queries, 0 for an unanswered one),
    hedge_mass (the mean subtree mass over the answered queries; NaN when there is none) and hedge_none (the share left unanswered: no
    candidate's subtree reaches the threshold).  A dict is also filled with the [Q, T] device tensors node (node ids, -1 = unanswered),
    node_col, mass, depth, relation and wu_palmer.  Not with retrieve=k (ValueError before any launch): a subset is not the
    distribution.  Every other metric, the ranks and the offsets are bit-equal to a call without the keyword.
    Averaged weights (optim.Adam(ema_decay=...)): `with optimizer.averaged_parameters(): evaluate(model, ...)` evaluates the averaged
    model -- the parameters are the averages inside the context; or load a checkpoint's with trainer.load_averaged."""
    device = torch.device(device)
    want_hedge = hedge is not None
    if want_hedge:
        from . import hedge as _hedge
        if isinstance(hedge, dict) and "thresholds" not in hedge:
            raise ValueError('evaluate: a hedge dict names its thresholds, {"thresholds": ...}')
        hedge_thr = _hedge.check_thresholds(hedge["thresholds"] if isinstance(hedge, dict) else hedge)
        hedge_beta = scoring._beta_of(1.0 if temperature is None else temperature)
        if retrieve is not None:
            raise ValueError("evaluate: hedge sums the distribution over every candidate's subtree; with retrieve=k a retrieved subset is "
                             "not the distribution")
    want_pred = isinstance(predictive, dict) or bool(predictive)
    calibrated = temperature is not None or want_pred
    if calibrated:
        beta = scoring._beta_of(1.0 if temperature is None else temperature)
    if retrieve is not None:
        if nll:
            raise ValueError("evaluate: nll=True scores every candidate; with retrieve=k the partition over a retrieved subset is not the likelihood")
        if calibrated:
            raise ValueError("evaluate: temperature / predictive describe the distribution over every candidate; with retrieve=k the partition "
                             "over a retrieved subset is not the likelihood")
        retrieve = _retrieve_args(retrieve, None, None)[0]
    want_taxo = isinstance(taxonomic, dict) or bool(taxonomic)
    if case is not None and "wu_palmer" in metric_names and not want_taxo:
        raise ValueError('evaluate: the "wu_palmer" column of the case study needs taxonomic=True')
    if want_taxo or want_hedge:
        from .taxometric import TaxonomyIndex
        tindex = (taxonomy_index if taxonomy_index is not None else TaxonomyIndex.from_dataset(dataset)).to(device)
    cand = sorted(dataset.all_positions)                                    # test_fast.py:93
    index = {a: i for i, a in enumerate(cand)}
    dtax = dataset.device_taxonomy(device)
    g = candidate_graphs(dtax, cand, dataset.expand_factor, seed, batch_size)    # x = features[_id]: the table is projected once
    was_training = model.training
    model.eval()
    hg = encode_candidates(model, g)                                        # test_fast.py:99-108
    queries, pos_lists = [], []
    for q in dataset.node_list:
        p = [index[a] for a in dataset.node2parents[q] if a in index]
        if p:
            queries.append(q)
            pos_lists.append(p)
    pos_off = np.concatenate([[0], np.cumsum([len(p) for p in pos_lists])]).astype(np.int64)
    pos_idx = np.concatenate(pos_lists).astype(np.int64) if pos_lists else np.zeros(0, dtype=np.int64)
    qf = dataset.node_features[torch.as_tensor(queries, dtype=torch.long)].to(device)
    mom = None
    with torch.no_grad():
        if retrieve is None and calibrated:
            ranks, thr = _ranks_of(model, hg, qf, pos_off, pos_idx, larger_is_better, qblock, with_thr=True) if nll else \
                (_ranks_of(model, hg, qf, pos_off, pos_idx, larger_is_better, qblock), None)
            if queries:
                if want_pred or nll and temperature is not None:          # (a temperature alone asks for nothing that needs the pass)
                    mom = scoring.score_moments_fused(model.match, hg, qf, larger_is_better, 1.0 / beta, block=qblock)
                if nll and temperature is not None:
                    nll_value = _nll_of(mom.lse, _scaled(thr, beta, larger_is_better), pos_off, True)
                elif nll:                                                 # no temperature: the value a call without `predictive` reports
                    nll_value = _nll_of(log_partition_fused(model.match, hg, qf, larger_is_better, block=qblock), thr, pos_off, larger_is_better)
                if want_pred:
                    pred_metrics, pred_tensors = _predictive(model, hg, qf, mom, ranks, pos_off, beta, larger_is_better, qblock)
            else:
                nll_value = float("nan")
                pred_metrics, pred_tensors = dict(entropy=float("nan"), confidence=float("nan"), ece=float("nan")), {}
            if isinstance(predictive, dict):
                predictive.update(pred_tensors)
        elif retrieve is None:
            if nll:
                ranks, thr = _ranks_of(model, hg, qf, pos_off, pos_idx, larger_is_better, qblock, with_thr=True)
                nll_value = _nll_of(log_partition_fused(model.match, hg, qf, larger_is_better, block=qblock), thr, pos_off, larger_is_better) \
                    if queries else float("nan")
            else:
                ranks = _ranks_of(model, hg, qf, pos_off, pos_idx, larger_is_better, qblock)
        else:
            from .metric import _device_group_ranks
            cf = dataset.node_features[torch.as_tensor(cand, dtype=torch.long)].to(device)     # the rows `kv` holds (dataset.py:227-229)
            ridx = retrieve_candidates(qf, cf, retrieve, *_retrieval_masks(dataset, queries, index)) if queries else \
                torch.zeros((0, retrieve), dtype=torch.int32, device=device)
            if queries:
                score, label, ret_dst = _retrieved_groups(model, hg, qf, pos_off, pos_idx, ridx, larger_is_better, qblock)
                ranks = _device_group_ranks(score, label, 1 if larger_is_better else 0)[0][:len(pos_idx)]
            else:
                ranks = torch.zeros(0, dtype=torch.int32, device=device)
        if case is not None or want_taxo:                                  # the best `topk` list, once for both
            cand_ids = torch.as_tensor(np.asarray(cand, dtype=np.int64), device=device)
            if retrieve is None:
                best = _best_parents(model, hg, qf, cand_ids, topk, larger_is_better, qblock)
            elif queries:
                best = _best_retrieved(score, ret_dst, ridx, topk, larger_is_better)      # candidate rows, -1 = an empty slot
            else:
                best = torch.zeros((0, 0), dtype=torch.int32, device=device)
        if want_taxo:
            nodes = best
            if retrieve is not None and best.numel():
                nodes = torch.where(best >= 0, cand_ids[best.long().clamp(min=0)], torch.full_like(best, -1, dtype=torch.int64))
            taxo_metrics, taxo_tensors = _taxonomic(tindex, nodes, pos_off, np.asarray(cand, dtype=np.int64)[pos_idx], len(queries))
            if isinstance(taxonomic, dict):
                taxonomic.update(taxo_tensors)
        if want_hedge:
            hedge_metrics, hedge_tensors = _hedged(model, hg, qf, tindex, cand, pos_off, pos_idx, hedge_thr, hedge_beta, larger_is_better,
                                                   mom.lse if mom is not None else None)
            if isinstance(hedge, dict):
                hedge.update(hedge_tensors)
        if case is not None:                                               # test_fast.py:112-147
            top = best.cpu().tolist() if retrieve is None else [[cand[i] for i in row if i >= 0] for row in best.cpu().tolist()]
            per_query_values = None
            if "wu_palmer" in metric_names:
                w = taxo_tensors["wu_palmer"]
                per_query_values = {"wu_palmer": w[:, 0].cpu().tolist() if w.shape[1] else [float("nan")] * len(queries)}
            rows = _case_rows(dataset, queries, pos_off, ranks, top, metric_names, per_query_values)
            if isinstance(case, list):
                case.extend(rows)
            else:
                with open(case, "w") as fout:
                    for row in rows:
                        fout.write("\t".join(row))
                        fout.write("\n")
    model.train(was_training)
    r = ranks.to(torch.float64)
    metrics = dict(macro_mr=_per_query_means(r, pos_off), hit_at_1=_per_query_means(ranks <= 1, pos_off),
                   hit_at_3=_per_query_means(ranks <= 3, pos_off), hit_at_5=_per_query_means(ranks <= 5, pos_off),
                   mrr_scaled_10=_per_query_means(1.0 / torch.ceil(r / 10.0), pos_off), n_queries=len(queries),
                   n_candidates=len(cand))
    if retrieve is not None:
        metrics["n_retrieved"] = retrieve
    if nll:
        metrics["nll"] = nll_value
    if want_taxo:
        metrics.update(taxo_metrics)
    if want_pred:
        metrics.update(pred_metrics)
    if want_hedge:
        metrics.update(hedge_metrics)
    return metrics, ranks, pos_off, queries


def infer(model, dataset, new_taxons, device, loss="info_nce_loss", batch_size=-1, save=None, topk=5, normalize=False, qblock=1024,
          seed=0, retrieve=None, with_scores=False, temperature=None, hedge=None, taxonomy_index=None):
    """infer.py:77-159: the `topk` best parents of every NEW term.  dataset: MaskedGraphDataset in 'test' mode (infer.py:43-57);
    new_taxons: path of the `<name>\t<v0 v1 ...>` file (infer.py:23-38) or an already loaded (vocab, array) pair.  Candidates are ALL
    nodes of the dataset's graph (infer.py:80-82 iterates `test_dataset.graph.nodes()`, not `all_positions`), in node order; best =
    descending score for the info_nce losses, ascending otherwise (infer.py:100-106), ties in candidate order like Python's stable
    sort.  Returns [(query, [parent vocab entries])]; `save` writes infer.py's TSV (header `Query\tPredicted parents`).
    topk: any size (a curator's 10 or 20, a re-ranker's 50): evaluate()'s routes -- fused up to scoring.TOPK_FUSED_MAX, score blocks +
    ops.select_k up to 4,096, the same order and (with_scores) the same fp32 scores on each.
    retrieve=k (infer.py's `-k`; 1 <= k <= 4096, else ValueError before any launch): the candidates of each new term are its k
    cosine-nearest graph nodes (the new-term vectors against `dataset.node_features`; no masks, a new term has none), and the `topk`
    best parents are chosen among them by matcher score.  Exact distance ties break by ascending node position.
    with_scores=True: every item is (query, parents, scores, log_probs) -- scores = the matcher's own fp32 values of the chosen pairs
    (bit-equal to scoring.score_all's entries), log_probs = z - lse[q]: the log of p(parent | query) = exp(z) / sum over ALL candidates
    of exp(z') (scoring.log_partition_fused; z = the score for the info_nce losses, its negative otherwise), formed in float64; `save`
    then writes two more tab-separated columns, `Scores` and `Log-probabilities` (%.6g, comma separated like the parents).  Not with
    retrieve=k (ValueError before any launch): a partition over a retrieved subset is not the likelihood.
    temperature=T (with with_scores=True only; finite and > 0; both ValueError before any launch): the calibrated form, log_probs =
    t - lse_T[q] with t = fl32(z / T) and lse_T over the scaled scores of all candidates (scoring.score_moments_fused) -- T from
    calibrate.fit_temperature on the validation split.  temperature=None: what it was.
    hedge: a threshold or a sequence of at most hedge.MAX_THRESHOLDS of them (with with_scores=True only; each finite and in (0, 1]; both
    ValueError before any launch): every item gains a fifth entry, per threshold the triple (hedged parent's vocab entry or None, subtree
    mass, depth) -- the deepest graph node whose subtree probability under p (at `temperature`, T = 1 without it) reaches the threshold
    (hedge.py), on the dataset's taxonomy (`taxonomy_index`: a taxometric.TaxonomyIndex of it to reuse; default
    TaxonomyIndex.from_dataset(dataset)) -- and `save` writes three more tab-separated columns per threshold, `Hedged parent@tau`,
    `Mass@tau` and `Depth@tau` (an unanswered query: an empty name, nan, 0).  hedge=None: what it was.
    Averaged weights (optim.Adam(ema_decay=...)): `with optimizer.averaged_parameters(): infer(model, ...)` infers with the averaged
    model; or load a checkpoint's with trainer.load_averaged."""
    from .dataset import load_new_taxons
    device = torch.device(device)
    if temperature is not None:
        if not with_scores:
            raise ValueError("infer: temperature scales the probabilities that with_scores=True reports; without it there is nothing to calibrate")
        beta = scoring._beta_of(temperature)
    if hedge is not None:
        from . import hedge as _hedge
        if not with_scores:
            raise ValueError("infer: hedge reports subtree probabilities beside those of with_scores=True; without it there is nothing to hedge")
        hedge_thr = _hedge.check_thresholds(hedge)
        hedge_beta = scoring._beta_of(1.0 if temperature is None else temperature)
    if retrieve is not None:
        if with_scores:
            raise ValueError("infer: with_scores=True normalises over every candidate; with retrieve=k the partition over a retrieved subset is not "
                             "the likelihood")
        retrieve = _retrieve_args(retrieve, None, None)[0]
    vocab, nf = load_new_taxons(new_taxons, normalize) if isinstance(new_taxons, (str, bytes)) or hasattr(new_taxons, "__fspath__") else new_taxons
    anchors = np.asarray(list(dataset.graph.nodes), dtype=np.int64)
    dtax = dataset.device_taxonomy(device)
    g = candidate_graphs(dtax, anchors, dataset.expand_factor, seed, batch_size)
    was_training = model.training
    model.eval()
    hg = encode_candidates(model, g)
    larger = str(loss).startswith("info_nce")
    qf = torch.as_tensor(np.asarray(nf), dtype=torch.float32).to(device)
    cand_ids = torch.as_tensor(anchors, device=device)
    with torch.no_grad():
        if retrieve is None and with_scores:
            ids, sc = _best_parents(model, hg, qf, cand_ids, topk, larger, qblock, with_scores=True)
            if temperature is None:
                lse = log_partition_fused(model.match, hg, qf, larger, block=qblock).to(torch.float64)
                z = sc.to(torch.float64)
                logp = ((z if larger else -z) - lse[:, None]).cpu().tolist()
            else:
                lse = scoring.score_moments_fused(model.match, hg, qf, larger, 1.0 / beta, block=qblock).lse
                logp = (_scaled(sc, beta, larger) - lse[:, None]).cpu().tolist()
            if hedge is not None:
                from .taxometric import TaxonomyIndex
                hix = _hedge.HedgeIndex.build(taxonomy_index if taxonomy_index is not None else TaxonomyIndex.from_dataset(dataset), anchors)
                h = _hedge.hedged_parents(model.match, hg, qf, hix.to(device), hedge_thr, 1.0 / hedge_beta, larger,
                                          lse=lse if temperature is not None else None)
                hedged = [[(dataset.vocab[int(anchors[c])] if c >= 0 else None, m, d) for c, m, d in zip(cs, ms, ds)]
                          for cs, ms, ds in zip(h.node_col.cpu().tolist(), h.mass.cpu().tolist(), h.depth.cpu().tolist())]
            picks, sc = ids.cpu().tolist(), sc.cpu().tolist()
        elif retrieve is None:
            picks = _best_parents(model, hg, qf, cand_ids, topk, larger, qblock).cpu().tolist()
        elif qf.shape[0] == 0 or len(anchors) == 0:
            picks = [[] for _ in range(qf.shape[0])]
        else:
            cf = dataset.node_features[torch.as_tensor(anchors, dtype=torch.long)].to(device)
            ridx = retrieve_candidates(qf, cf, retrieve)
            score, _label, ret_dst = _retrieved_groups(model, hg, qf, np.zeros(qf.shape[0] + 1, dtype=np.int64), np.zeros(0, dtype=np.int64),
                                                       ridx, larger, qblock)
            best = _best_retrieved(score, ret_dst, ridx, topk, larger).cpu().tolist()
            picks = [[int(anchors[i]) for i in row if i >= 0] for row in best]
    model.train(was_training)
    out = [(q, [dataset.vocab[i] for i in row]) for q, row in zip(vocab, picks)]
    if with_scores:
        out = [(q, parents, s, lp) for (q, parents), s, lp in zip(out, sc, logp)]
        if hedge is not None:
            out = [item + (hd,) for item, hd in zip(out, hedged)]
    if save is not None:
        with open(save, "w") as fout:
            if with_scores:
                more = "" if hedge is None else "".join(f"\tHedged parent@{t:g}\tMass@{t:g}\tDepth@{t:g}" for t in hedge_thr)
                fout.write("Query\tPredicted parents\tScores\tLog-probabilities" + more + "\n")
                for q, parents, s, lp, *hd in out:
                    more = "".join(f"\t{name if name is not None else ''}\t{m:.6g}\t{d}" for name, m, d in (hd[0] if hd else ()))
                    fout.write(f"{q}\t{', '.join(parents)}\t{', '.join('%.6g' % v for v in s)}\t{', '.join('%.6g' % v for v in lp)}{more}\n")
            else:
                fout.write("Query\tPredicted parents\n")
                for q, parents in out:
                    fout.write(f"{q}\t{', '.join(parents)}\n")
    return out


VALIDATION_METRICS = ("macro_mr", "micro_mr", "hit_at_1", "hit_at_3", "mrr_scaled_10")


def validate(model, loader, metrics=VALIDATION_METRICS, larger_is_better=True):
    """trainer.py:96-124 (Trainer._valid_epoch) on the device: model.eval() and no_grad over every batch of `loader` (the training flag
    is restored after), then per batch the forward, the grouped ranks (metric.obtain_ranks, csrc/txe_grouprank.hip) and the requested
    metrics of the batch, added in one launch to an fp64 device accumulator; ONE host read-back per epoch.
    loader: any iterable of (g, h, qf, label) -- DeviceBatchLoader with either sampler -- or of (g, qf, label) -- MaskedGraphDataLoader's
    small batches: h = g.ndata.pop('x'), and the tensors are moved to the model's device as trainer.py:109-112 does.
    Returns dict(val_metrics=[mean over batches, in the order of `metrics`], n_batches, n_groups, n_positives)."""
    from . import _lib
    from .metric import METRIC_IDS, _check_batch, _device_group_ranks
    metrics = list(metrics)
    if not 1 <= len(metrics) <= 16 or any(m not in METRIC_IDS for m in metrics):
        raise ValueError(f"metrics must be 1 to 16 names out of {sorted(METRIC_IDS)}, got {metrics}")
    which = sum(METRIC_IDS[m] << (4 * i) for i, m in enumerate(metrics))
    mode = 1 if larger_is_better else 0
    dev = next(model.parameters()).device
    acc = torch.zeros(len(metrics) + 2, dtype=torch.float64, device=dev)
    n_batches = 0
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for batch in loader:
                if len(batch) == 4:
                    g, h, qf, label = batch
                else:
                    g, qf, label = batch
                    h = g.ndata.pop("x")
                h = h.to(dev, non_blocking=True)
                qf = qf.to(dev, non_blocking=True) if torch.is_tensor(qf) else qf
                label = label.to(dev, non_blocking=True)
                score, label = _check_batch(model(g, h, qf), label)
                if score.shape[0] == 0:
                    raise ValueError("validate() got an empty batch")
                ranks, pos_off, counts = _device_group_ranks(score, label, mode)
                with _lib.on_device(dev):
                    _lib.call("txe_group_metrics", _lib.ptr(ranks), _lib.ptr(pos_off), _lib.ptr(counts), which, len(metrics), _lib.ptr(acc),
                              _lib.stream_ptr())
                n_batches += 1
    finally:
        model.train(was_training)
    host = acc.cpu().numpy()
    vals = (host[:len(metrics)] / n_batches).tolist() if n_batches else [float("nan")] * len(metrics)
    return dict(val_metrics=vals, n_batches=n_batches, n_groups=int(host[len(metrics)]), n_positives=int(host[len(metrics) + 1]))
