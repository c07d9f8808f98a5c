#!/usr/bin/env python3
"""The all-candidate log-partition at the bench's inference shape (BASELINE configs[2]: the MAG-Full-shaped synthetic taxonomy, 356 k
candidates, 8,192 test queries, PGAT+WMR+LBM), on one MI355X:

    python tools/log_partition_timing.py [--shape mag_full] [--queries 8192] [--reps 5] [--out FILE.json]

The candidates are encoded once (not timed: every variant shares it).  Timed with device events, every variant warmed up twice, median
of `--reps` repetitions, the variants alternating inside one repetition loop (tools/retrieval_timing.py's method):
  fused         scoring.log_partition_fused, blocks of 1,024 queries: the score kernel's lse epilogue + the merge, no score matrix
  materialised  the only route without the fused kernels: scoring.score_all's loop in blocks of 1,024 queries (the prepared matcher's
                score kernel into one [1024, G] fp32 block at a time, 1.46 GB on MAG-Full) + torch.logsumexp of each block
  rank_all      scoring.rank_all_fused on the same blocks, as context: the other fused pass over the same tiles
All three prepare the matcher's candidate side (U = hg W and its packed planes) inside the timed call, as their callers do.
Prints one JSON line: the three times with min..max, and the largest |fused - materialised| over the queries."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("log_partition_timing.py measures on the GPU; none found")
    import bench
    from taxoexpan_amd import graph as G, synthetic as syn
    from taxoexpan_amd.scoring import encode_candidates, log_partition_fused, prepare_matcher, rank_all_fused
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    tax = syn.make_named_taxonomy(args.shape, seed=47)
    model = bench.make_model("pgat", dev).eval()
    cand, _val, test = syn.split_candidates(tax)
    test = test[:args.queries]
    pos_off, pos_idx = bench._positives(tax, cand, test)
    with torch.no_grad():
        dtax = G.DeviceTaxonomy(tax.par_ptr, tax.par_idx, tax.chd_ptr, tax.chd_idx, tax.features, dev)
        hg = encode_candidates(model, G.device_egonet_batch(dtax, cand, seed=7, with_features="lazy"))
        qf = tax.features[torch.from_numpy(test)].to(dev)
        block_buf = torch.empty((1024, (hg.shape[0] + 3) // 4 * 4), dtype=torch.float32, device=dev)

        def fused():
            return log_partition_fused(model.match, hg, qf, True, block=1024)

        def materialised():
            pm, out = prepare_matcher(model.match, hg), []
            for q0 in range(0, qf.shape[0], 1024):
                qb = qf[q0:q0 + 1024]
                out.append(torch.logsumexp(pm.score(qb, out=block_buf[:qb.shape[0], :hg.shape[0]]), dim=1))
            return torch.cat(out)

        def rank_all():
            return rank_all_fused(model.match, hg, qf, pos_off, pos_idx, block=1024)

        variants = [("fused", fused), ("materialised", materialised), ("rank_all", rank_all)]
        for _name, fn in variants:                      # warm-up: code objects, the caching allocator's blocks
            fn()
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in variants}
        for _ in range(args.reps):
            for name, fn in variants:                   # alternating: a drift of the machine hits every variant alike
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e-3)
        a, b = fused().double(), materialised().double()
        diff = float((a - b).abs().max())
    out = dict(shape=args.shape, candidates=int(hg.shape[0]), queries=int(qf.shape[0]), r=int(qf.shape[1]), reps=args.reps,
               timing="device events, median of reps, variants alternating, two warm-up calls each; encode not included",
               block_bytes=4 * 1024 * int(hg.shape[0]), max_abs_fused_minus_materialised=diff, mean_lse=float(a.mean()))
    for name, ts in times.items():
        out[name + "_s"] = float(np.median(ts))
        out[name + "_spread"] = [float(min(ts)), float(max(ts))]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
