#!/usr/bin/env python3
"""The all-candidate moments pass and the temperature fit at the bench's inference shape (BASELINE configs[2]: the MAG-Full-shaped
synthetic taxonomy, 356 k candidates, 8,192 test queries, PGAT+WMR with a BIM matcher), on one MI355X:

    python tools/calibration_timing.py [--shape mag_full] [--queries 8192] [--reps 5] [--match bim] [--out FILE.json]

The candidates are encoded once (not timed: every variant shares it).  Timed with device events, every variant warmed up twice, median
of `--reps` repetitions, the variants alternating inside one repetition loop (tools/log_partition_timing.py's method):
  moments       scoring.score_moments_fused at T = 2, blocks of 1,024 queries: the score kernel's moments epilogue + the merge
  lse           scoring.log_partition_fused on the same blocks: the pass the moments mode extends (the same-process comparison)
  materialised  the route without the fused kernels: the prepared matcher's score kernel into one [1024, G] fp32 block at a time + the
                same four quantities in float64 torch ops (scoring._moments_of_block)
  fit           calibrate.fit_temperature_scores: the positives' scores once, then one moments pass + one read-back per evaluation
All of them prepare the matcher's candidate side (U = hg W and its packed planes) inside the timed call, as their callers do.
Prints one JSON line: the times with min..max, the fit's result and evaluation count, and the largest |moments - materialised| per
quantity over the queries."""
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
    ap.add_argument("--match", default="bim", choices=["bim", "lbm"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("calibration_timing.py measures on the GPU; none found")
    import bench
    from taxoexpan_amd import calibrate, graph as G, model_zoo, scoring, synthetic as syn
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    tax = syn.make_named_taxonomy(args.shape, seed=47)
    model = bench.make_model("pgat", dev).eval()
    if args.match == "bim":                             # the bench's model carries an LBM: the same W without the exp
        l, r = model.match.W.weight.shape[-2:]
        bim = model_zoo.BIM(l, r).to(dev)
        with torch.no_grad():
            bim.W.weight.copy_(model.match.W.weight)
        model.match = bim.eval()
    cand, _val, test = syn.split_candidates(tax)
    test = test[:args.queries]
    pos_off, pos_idx = bench._positives(tax, cand, test)
    test = test[np.diff(pos_off) > 0]                   # (evaluate's rule: a query without a true parent among the candidates is skipped)
    pos_off, pos_idx = bench._positives(tax, cand, test)
    T = 2.0
    with torch.no_grad():
        dtax = G.DeviceTaxonomy(tax.par_ptr, tax.par_idx, tax.chd_ptr, tax.chd_idx, tax.features, dev)
        hg = scoring.encode_candidates(model, G.device_egonet_batch(dtax, cand, seed=7, with_features="lazy"))
        qf = tax.features[torch.from_numpy(test)].to(dev)
        block_buf = torch.empty((1024, (hg.shape[0] + 3) // 4 * 4), dtype=torch.float32, device=dev)
        beta = scoring._beta_of(T)

        def moments():
            return torch.stack(scoring.score_moments_fused(model.match, hg, qf, True, temperature=T, block=1024), dim=1)

        def lse():
            return scoring.log_partition_fused(model.match, hg, qf, True, block=1024)

        def materialised():
            pm, out = scoring.prepare_matcher(model.match, hg), []
            for q0 in range(0, qf.shape[0], 1024):
                qb = qf[q0:q0 + 1024]
                out.append(scoring._moments_of_block(pm.score(qb, out=block_buf[:qb.shape[0], :hg.shape[0]]), beta, True))
            return torch.cat(out)

        fits = []

        def fit():
            fits.append(calibrate.fit_temperature_scores(model.match, hg, qf, pos_off, pos_idx, block=1024))
            return fits[-1]

        variants = [("moments", moments), ("lse", lse), ("materialised", materialised), ("fit", fit)]
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
        a, b = moments(), materialised()
        diff = [float(v) for v in (a - b).abs().max(dim=0).values.cpu()]
        c = fits[-1]
    out = dict(shape=args.shape, match=args.match, candidates=int(hg.shape[0]), queries=int(qf.shape[0]), r=int(qf.shape[1]), reps=args.reps,
               timing="device events, median of reps, variants alternating, two warm-up calls each; encode not included",
               block_bytes=4 * 1024 * int(hg.shape[0]), temperature=T,
               max_abs_moments_minus_materialised=dict(zip(("lse", "mean", "var", "entropy"), diff)),
               mean_entropy=float(a[:, 3].mean()), fit=dict(temperature=c.temperature, beta=c.beta, nll_before=c.nll_before, nll_after=c.nll_after,
                                                            iterations=c.iterations, at_bound=c.at_bound, evaluations=len(c.history)))
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
