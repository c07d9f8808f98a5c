#!/usr/bin/env python3
"""All-candidate ranking and top-5 selection with an NTN matcher (model_zoo.py:331-346, k = 4 slices) at the inference shape of
tools/infer_bench.py (default: MAG-CS -- the candidates, test queries and true parents of the synthetic taxonomy, l = 500, r = 250), one
MI355X.  Two routes:
  fused    scoring.rank_all_fused / topk_parents_fused on the NTN score kernel (txe_ntn_*): every query, nothing materialised
  literal  the per-query loop of evaluate._score_blocks (NTN.forward on the query expanded to every candidate) + ops.rank_block /
           scoring.topk_parents on the materialised block, on a bounded SAMPLE of queries (--literal-queries, default 64); its totals
           are that sample's time SCALED to the full query count and say so in their names
Both are reported per query.  The candidate vectors are random (the encoder is not what is timed; neither route's work depends on the
values).  --literal-only needs nothing of the fused route: the literal side can be timed on a tree that does not have it.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from taxoexpan_amd import ops, synthetic as syn  # noqa: E402
from taxoexpan_amd.model_zoo import NTN  # noqa: E402
from taxoexpan_amd.scoring import topk_parents  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="mag_cs", choices=list(syn.SHAPES))
ap.add_argument("--out-dim", type=int, default=500, help="width of a candidate's graph vector (bench.MAG out_dim)")
ap.add_argument("--k", type=int, default=4)
ap.add_argument("--topk", type=int, default=5)
ap.add_argument("--literal-queries", type=int, default=64)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--literal-only", action="store_true")
ap.add_argument("--fused-only", action="store_true")
args = ap.parse_args()

dev = torch.device("cuda:0")
tax = syn.make_named_taxonomy(args.shape, seed=47)
cand, _val, test = syn.split_candidates(tax)
cand_index = np.full(tax.n_nodes, -1, dtype=np.int64)
cand_index[cand] = np.arange(len(cand))
pos_lists = [cand_index[tax.par_idx[tax.par_ptr[q]:tax.par_ptr[q + 1]]] for q in test]
pos_lists = [p[p >= 0] for p in pos_lists]
keep = [i for i, p in enumerate(pos_lists) if len(p)]
test, pos_lists = test[keep], [pos_lists[i] for i in keep]
queries = tax.features[torch.from_numpy(test)].to(dev)
G, Q, r = len(cand), len(test), queries.shape[1]
torch.manual_seed(47)
hg = torch.randn(G, args.out_dim, device=dev) * 0.1
match = NTN(args.out_dim, r, k=args.k).to(dev).eval()
cand_ids = torch.arange(G, device=dev)
pos_off = np.concatenate([[0], np.cumsum([len(p) for p in pos_lists])]).astype(np.int64)
pos_idx = np.concatenate(pos_lists).astype(np.int64)


def timed(fn):
    fn()                                        # warm-up: allocator, code objects
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


res = dict(shape=args.shape, candidates=G, queries=Q, l=args.out_dim, r=r, k=args.k, topk=args.topk)
with torch.no_grad():
    if not args.literal_only:
        from taxoexpan_amd.scoring import rank_all_fused, topk_parents_fused
        t_rank = timed(lambda: rank_all_fused(match, hg, queries, pos_off, pos_idx))
        t_top = timed(lambda: topk_parents_fused(match, hg, queries, cand_ids, args.topk, True))
        res.update(fused_rank_all_s=t_rank, fused_rank_us_per_query=1e6 * t_rank / Q, fused_topk_s=t_top,
                   fused_topk_us_per_query=1e6 * t_top / Q)
    if not args.fused_only:
        n = min(args.literal_queries, Q)
        qs = queries[:n]
        off = torch.from_numpy(pos_off[:n + 1])
        idx = torch.from_numpy(pos_idx[:pos_off[n]])

        def literal_block():
            return torch.stack([match(hg, q.expand(G, -1)).reshape(-1) for q in qs])

        t_rank = timed(lambda: ops.rank_block(literal_block().contiguous(), off, idx, True))
        t_top = timed(lambda: topk_parents(literal_block(), cand_ids, args.topk, True))
        res.update(literal_sample_queries=n, literal_rank_us_per_query=1e6 * t_rank / n, literal_topk_us_per_query=1e6 * t_top / n,
                   literal_rank_all_s_scaled_from_sample=t_rank / n * Q, literal_topk_s_scaled_from_sample=t_top / n * Q)
    if not args.literal_only and not args.fused_only:
        res.update(rank_speedup_scaled=res["literal_rank_us_per_query"] / res["fused_rank_us_per_query"],
                   topk_speedup_scaled=res["literal_topk_us_per_query"] / res["fused_topk_us_per_query"])
print(json.dumps(res))
