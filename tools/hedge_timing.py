#!/usr/bin/env python3
"""Hedged placement (taxoexpan_amd/hedge.py) at the bench's inference shape (BASELINE configs[2]: the MAG-Full-shaped
synthetic taxonomy, 356 k candidates, 8,192 test queries, PGAT+WMR with a BIM matcher), on one MI355X:

    python tools/hedge_timing.py [--shape mag_full] [--queries 8192] [--reps 5] [--out FILE.json]

The candidates are encoded once (not timed: every variant shares it).  Host: the index build (TaxonomyIndex.from_parents once, wall
clock; HedgeIndex.build, median of `--reps`).  Device: timed with device events, every variant warmed up twice, median of `--reps`
repetitions with min..max, the variants alternating inside one repetition loop (tools/log_partition_timing.py's method):
  probs      ONE txe_hedge_probs launch on a materialised score block of the driver's block size
  sweep      ONE txe_hedge_sweep in hedge mode (4 thresholds) on that block's probabilities
  hedged     hedge.hedged_parents over all queries: the moments pass, then per block the score kernel, probs and the sweep
  rank       scoring.rank_all_fused over all queries, blocks of 1,024: the fused ranking pass evaluate() runs anyway
  composite  what a user would write without the kernels, per block of the same size: the score block, a float64 softmax, torch.sparse.mm
             of the closure (a [G, G] CSR of ones) with it, and per threshold a masked argmax over depth (no tie rules)
Prints one JSON line: sizes, the times, and the share of (query, threshold) answers on which composite and hedged agree."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

THRESHOLDS = [0.5, 0.7, 0.9, 0.99]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="mag_full")
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--temperature", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hedge_timing.py measures on the GPU; none found")
    import bench
    from taxoexpan_amd import graph as G, hedge, model_zoo, scoring, synthetic as syn
    from taxoexpan_amd.taxometric import TaxonomyIndex
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    tax = syn.make_named_taxonomy(args.shape, seed=47)
    model = bench.make_model("pgat", dev).eval()
    l, r = model.match.W.weight.shape[-2:]              # the bench's model carries an LBM: the same W without the exp
    bim = model_zoo.BIM(l, r).to(dev)
    with torch.no_grad():
        bim.W.weight.copy_(model.match.W.weight)
    model.match = bim.eval()
    cand, _val, test = syn.split_candidates(tax)
    test = test[:args.queries]
    pos_off, pos_idx = bench._positives(tax, cand, test)
    test = test[np.diff(pos_off) > 0]
    pos_off, pos_idx = bench._positives(tax, cand, test)
    T = args.temperature
    t0 = time.perf_counter()
    tix = TaxonomyIndex.from_parents(tax.par_ptr, tax.par_idx)
    taxonomy_index_s = time.perf_counter() - t0
    build = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        ix = hedge.HedgeIndex.build(tix, cand)
        build.append(time.perf_counter() - t0)
    ixd = ix.to(dev)
    with torch.no_grad():
        dtax = G.DeviceTaxonomy(tax.par_ptr, tax.par_idx, tax.chd_ptr, tax.chd_idx, tax.features, dev)
        hg = scoring.encode_candidates(model, G.device_egonet_batch(dtax, cand, seed=7, with_features="lazy"))
        qf = tax.features[torch.from_numpy(test)].to(dev)
        Q, Gn = int(qf.shape[0]), int(hg.shape[0])
        block = hedge.default_block(Gn, Q)
        beta = scoring._beta_of(T)
        lse_all = scoring.score_moments_fused(model.match, hg, qf, True, T).lse
        pm = scoring.prepare_matcher(model.match, hg)
        sbuf = torch.empty((block, (Gn + 3) // 4 * 4), dtype=torch.float32, device=dev)
        S0 = pm.score(qf[:block], out=sbuf[:min(block, Q), :Gn])
        pbuf = torch.empty((Gn, hedge._pitch(block)), dtype=torch.float32, device=dev)
        PT0 = hedge.probabilities(S0, lse_all[:S0.shape[0]], beta, out=pbuf)
        # the composite's operands: the closure as a CSR of ones and the depths
        closure = torch.sparse_csr_tensor(torch.from_numpy(ix.sub_ptr.astype(np.int64)), torch.from_numpy(ix.sub_idx.astype(np.int64)),
                                          torch.ones(ix.nnz, dtype=torch.float64), size=(Gn, Gn)).to(dev)
        depth = ixd.depth.to(torch.int64)

        def probs():
            return hedge.probabilities(S0, lse_all[:S0.shape[0]], beta, out=pbuf)

        def sweep():
            return hedge.hedge_block(ixd, PT0, THRESHOLDS)

        def hedged():
            return hedge.hedged_parents(model.match, hg, qf, ixd, THRESHOLDS, T, block=block)

        def rank():
            return scoring.rank_all_fused(model.match, hg, qf, pos_off, pos_idx, block=1024)

        def composite():
            pmc, out = scoring.prepare_matcher(model.match, hg), []
            for q0 in range(0, Q, block):
                qb = qf[q0:q0 + block]
                S = pmc.score(qb, out=sbuf[:qb.shape[0], :Gn])
                P = torch.softmax(S.to(torch.float64) * beta, dim=1)
                mass = torch.sparse.mm(closure, P.t().contiguous())                      # [G, nq]
                cols = []
                for tau in THRESHOLDS:
                    key = torch.where(mass >= tau, depth[:, None], torch.full_like(depth[:, None], -1))
                    best = key.max(dim=0)
                    cols.append(torch.where(best.values > 0, best.indices, torch.full_like(best.indices, -1)))
                out.append(torch.stack(cols, dim=1))
            return torch.cat(out)

        variants = [("probs", probs), ("sweep", sweep), ("hedged", hedged), ("rank", rank), ("composite", composite)]
        composite_error = None
        for name, fn in list(variants):                 # warm-up: code objects, the caching allocator's blocks
            try:
                fn()
                fn()
            except RuntimeError as e:                   # (only the torch composite may be missing an operator: say so, time the rest)
                if name != "composite":
                    raise
                composite_error = str(e).splitlines()[0][:200]
                variants.remove((name, fn))
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
        h = hedged()
        agree = float((h.node_col.long() == composite()).double().mean()) if composite_error is None else None
        none = [float(v) for v in (h.node_col < 0).double().mean(dim=0).cpu()]
        mean_depth = [float(v) for v in h.depth.double().mean(dim=0).cpu()]
    out = dict(shape=args.shape, candidates=Gn, queries=Q, closure_entries=ix.nnz, work_items=ix.n_items, long_rows=ix.n_long,
               longest_row=int(np.diff(ix.sub_ptr).max()), block=block, thresholds=THRESHOLDS, temperature=T, reps=args.reps,
               timing="device events, median of reps, variants alternating, two warm-up calls each; encode not included; measured once",
               taxonomy_index_s=taxonomy_index_s, index_build_s=float(np.median(build)), index_build_spread=[min(build), max(build)],
               probs_bytes=8 * S0.shape[0] * Gn, sweep_bytes_read=4 * 64 * ix.nnz * ((S0.shape[0] + 63) // 64),
               composite_agrees=agree, composite_error=composite_error, hedge_none=none, hedge_mean_depth=mean_depth)
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
