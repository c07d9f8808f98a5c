#!/usr/bin/env python3
"""Retrieve-then-rank against all-candidate ranking at the bench's inference shape (BASELINE configs[2]: the MAG-Full-shaped synthetic
taxonomy, 356 k candidates, 8,192 test queries, PGAT+WMR+LBM), on one MI355X:

    python tools/retrieval_timing.py [--shape mag_full] [--queries 8192] [--reps 5] [--out FILE.json]

The candidates are encoded once (not timed: both protocols share it).  Timed with device events, every shape warmed up first, median
of `--reps` repetitions, the variants alternating inside one repetition loop:
  all_candidates   scoring.rank_all_fused -- what evaluate() runs after the encode: every positive against all candidates
  retrieval k      scoring.retrieve_candidates alone: normalise, cosine GEMM blocks, masked select-k (masks: parents + roots -- the test
                   queries are leaves)
  retrieve+rank k  what evaluate(retrieve=k) runs after the encode: retrieval, the gathered scores of positives + retrieved rows, the
                   grouped ranking
for k in {64, 1024}.  Bytes: the select kernel reads a row of G fp32 similarities four times (three histogram passes + the emit pass;
five when ties straddle the k-th place) -- its roof is ONE read of the block, G x 4 bytes per row.  Prints one JSON line."""
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
        raise SystemExit("retrieval_timing.py measures on the GPU; none found")
    import bench
    from taxoexpan_amd import graph as G, synthetic as syn
    from taxoexpan_amd.evaluate import _retrieved_groups
    from taxoexpan_amd.metric import _device_group_ranks
    from taxoexpan_amd.scoring import encode_candidates, rank_all_fused, retrieve_candidates
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    tax = syn.make_named_taxonomy(args.shape, seed=47)
    model = bench.make_model("pgat", dev).eval()
    cand, _val, test = syn.split_candidates(tax)
    test = test[:args.queries]
    pos_off, pos_idx = bench._positives(tax, cand, test)
    cand_index = np.full(tax.n_nodes, -1, dtype=np.int64)
    cand_index[cand] = np.arange(len(cand))
    roots = cand_index[np.nonzero(np.diff(tax.par_ptr) == 0)[0]]
    roots = roots[roots >= 0]
    mask_lists = [np.concatenate([pos_idx[pos_off[i]:pos_off[i + 1]], roots]) for i in range(len(test))]
    mask_off = np.concatenate([[0], np.cumsum([len(m) for m in mask_lists])])
    mask_idx = np.concatenate(mask_lists)
    with torch.no_grad():
        dtax = G.DeviceTaxonomy(tax.par_ptr, tax.par_idx, tax.chd_ptr, tax.chd_idx, tax.features, dev)
        hg = encode_candidates(model, G.device_egonet_batch(dtax, cand, seed=7, with_features="lazy"))
        qf = tax.features[torch.from_numpy(test)].to(dev)
        cf = tax.features[torch.from_numpy(cand)].to(dev)

        def all_candidates():
            return rank_all_fused(model.match, hg, qf, pos_off, pos_idx, block=1024)

        def retrieval(k):
            return retrieve_candidates(qf, cf, k, mask_off, mask_idx)

        def retrieve_rank(k):
            ridx = retrieve_candidates(qf, cf, k, mask_off, mask_idx)
            score, label, _ = _retrieved_groups(model, hg, qf, pos_off, pos_idx, ridx, True, None)
            return _device_group_ranks(score, label, 1)[0][:len(pos_idx)]

        variants = [("all_candidates", all_candidates)]
        for k in (64, 1024):
            variants += [(f"retrieval_k{k}", lambda k=k: retrieval(k)), (f"retrieve_rank_k{k}", lambda k=k: retrieve_rank(k))]
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
        r_all = all_candidates().cpu().numpy()
        r_1024 = retrieve_rank(1024).cpu().numpy()
    nq, ng = len(test), len(cand)
    out = dict(shape=args.shape, candidates=ng, queries=nq, positives=int(len(pos_idx)), masked_per_query=float(len(mask_idx)) / max(nq, 1),
               reps=args.reps, timing="device events, median of reps, variants alternating, two warm-up calls each; encode not included",
               select_bytes_per_row_read=4 * 4 * ng, select_roof_bytes_per_row=4 * ng,
               mean_rank_all_candidates=float(r_all.mean()), mean_rank_retrieved_1024=float(r_1024.mean()))
    for name, ts in times.items():
        out[name + "_s"] = float(np.median(ts))
        out[name + "_spread"] = [float(min(ts)), float(max(ts))]
    for k in (64, 1024):
        out[f"retrieval_k{k}_block_bytes_per_s"] = 4.0 * nq * ng / out[f"retrieval_k{k}_s"]      # one read of the similarity blocks over the whole stage
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
