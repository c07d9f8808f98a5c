#!/usr/bin/env python3
"""The best-k parents of every query at the bench's inference shape (BASELINE configs[2]: the MAG-Full-shaped synthetic taxonomy, 356 k
candidates, 8,192 test queries, PGAT+WMR+LBM), on one MI355X, for a list of k:

    python tools/topk_wide_timing.py [--shape mag_full] [--queries 8192] [--ks 5,8,9,16,32,64,128] [--routes fused,select,composite]
                                     [--reps 5] [--out FILE.json]

The candidates are encoded once (not timed: every route shares them).  Timed with device events, every (route, k) warmed up once, median
and min..max of `--reps` repetitions, the routes alternating inside one repetition loop (tools/log_partition_timing.py's method):
  composite  score blocks of 1,024 queries (the prepared matcher's score kernel into one [1024, G] fp32 block at a time) + the torch
             composite scoring.topk_parents on each: the route evaluate._best_parents took above k = 8 before the wide kernels
  fused      scoring.topk_parents_fused, blocks of 1,024 queries: ceil(k / 8) rounds of the score tiles' best-k epilogue + merge, no
             score matrix (k <= 64)
  select     evaluate._best_parents' route above scoring.TOPK_FUSED_MAX: score blocks of at most scoring.RETRIEVE_BLOCK_BYTES +
             ops.select_k (k <= 4,096)
Every route prepares the matcher's candidate side inside the timed call, as its callers do.  Beside each time: the peak of allocated
device memory above what was allocated before the call.  The routes' selections are compared (they must be equal).
Prints one JSON line.  Uses nothing a k <= 8 run needs beyond scoring.topk_parents_fused, so `--routes fused --ks 5` also runs on a
checkout from before the wide kernels -- the check that they cost the old path nothing."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="mag_full")
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--ks", default="5,8,9,16,32,64,128")
    ap.add_argument("--routes", default="fused,select,composite")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_wide_timing.py measures on the GPU; none found")
    import bench
    from taxoexpan_amd import graph as G, ops, scoring, synthetic as syn
    from taxoexpan_amd.scoring import encode_candidates, prepare_matcher, topk_parents, topk_parents_fused
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    tax = syn.make_named_taxonomy(args.shape, seed=47)
    model = bench.make_model("pgat", dev).eval()
    cand, _val, test = syn.split_candidates(tax)
    test = test[:args.queries]
    ks = [int(k) for k in args.ks.split(",")]
    routes = args.routes.split(",")
    fused_max = getattr(ops, "TOPK_WIDE_MAX", 8)
    with torch.no_grad():
        dtax = G.DeviceTaxonomy(tax.par_ptr, tax.par_idx, tax.chd_ptr, tax.chd_idx, tax.features, dev)
        hg = encode_candidates(model, G.device_egonet_batch(dtax, cand, seed=7, with_features="lazy"))
        qf = tax.features[torch.from_numpy(test)].to(dev)
        n_cand = hg.shape[0]
        cols = torch.arange(n_cand, device=dev)
        pitch = (n_cand + 3) // 4 * 4

        def composite(k):
            pm, out = prepare_matcher(model.match, hg), []
            buf = torch.empty((1024, pitch), dtype=torch.float32, device=dev)
            for q0 in range(0, qf.shape[0], 1024):
                qb = qf[q0:q0 + 1024]
                out.append(topk_parents(pm.score(qb, out=buf[:qb.shape[0], :n_cand]), cols, k, True))
            return torch.cat(out)

        def fused(k):
            return topk_parents_fused(model.match, hg, qf, None, k, True, block=1024)

        def select(k):
            pm, out = prepare_matcher(model.match, hg), []
            block = max(1, min(qf.shape[0], scoring.RETRIEVE_BLOCK_BYTES // (4 * n_cand)))
            buf = torch.empty((block, pitch), dtype=torch.float32, device=dev)
            for q0 in range(0, qf.shape[0], block):
                qb = qf[q0:q0 + block]
                out.append(ops.select_k(pm.score(qb, out=buf[:qb.shape[0], :n_cand]), k))
            return torch.cat(out).long()

        fns = {"composite": composite, "fused": fused, "select": select}
        runs = [(r, k) for k in ks for r in routes if not (r == "fused" and k > fused_max) and not (r == "select" and k > ops.SELECT_K_MAX)]
        times, peaks, equal = {rk: [] for rk in runs}, {}, {}
        for r, k in runs:                                   # warm-up: code objects, the caching allocator's blocks; the peak; the selection
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            got = fns[r](k)
            torch.cuda.synchronize()
            peaks[(r, k)] = int(torch.cuda.max_memory_allocated() - base)
            ref = equal.setdefault(k, (r, got))
            if ref[0] != r:
                equal[(r, k)] = bool(torch.equal(ref[1], got))
            del got
        for _ in range(args.reps):
            for r, k in runs:                               # alternating: a drift of the machine hits every route alike
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fns[r](k)
                e1.record()
                e1.synchronize()
                times[(r, k)].append(e0.elapsed_time(e1) * 1e-3)
    out = dict(shape=args.shape, candidates=int(n_cand), queries=int(qf.shape[0]), r=int(qf.shape[1]), reps=args.reps,
               timing="device events, median and min..max of reps, routes alternating, one warm-up call each; encode not included",
               topk_fused_max=getattr(scoring, "TOPK_FUSED_MAX", 8), results=[])
    for r, k in runs:
        ts = times[(r, k)]
        out["results"].append(dict(route=r, k=k, s=float(np.median(ts)), spread=[float(min(ts)), float(max(ts))], peak_bytes=peaks[(r, k)],
                                   equals_first_route=equal.get((r, k))))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
