#!/usr/bin/env python3
"""The taxonomy-aware evaluation kernel (csrc/txe_taxometric.hip, taxometric.taxonomic_slots) on the MAG-Full-shaped synthetic
taxonomy (431,416 nodes), on one MI355X:

    python tools/taxometric_timing.py [--shape mag_full] [--queries 8192] [--reps 20] [--host-sample 256] [--out FILE.json]

Reported: the index build on the host (wall time, closure size, list statistics); for K in {1, 5, 64}, Q queries with 1-3 random gold
parents each and random predictions:
  launch   txe_taxo_slots alone on resident operands, device events around each of `--reps` launches after two warm-up launches
           (median, min..max; an event pair around any launch has a floor of several us)
  call     taxometric.taxonomic_slots as evaluate() calls it (argument checks, the upload of the gold lists, the launch), device events
           around each of `--reps` calls after a warm-up call (median)
  host     taxometric.host_taxonomic on the first `--host-sample` queries, scaled to all of them -- the only thing to compare against:
           nothing computed these quantities before
and whether the device integers equal the host's on that sample.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def make_lists(n, Q, K, seed):
    rs = np.random.RandomState(seed)
    cnt = rs.randint(1, 4, size=Q)
    return (rs.randint(0, n, size=(Q, K)).astype(np.int32), np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64),
            rs.randint(0, n, size=int(cnt.sum())).astype(np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="mag_full")
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-sample", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("taxometric_timing.py measures on the GPU; none found")
    from taxoexpan_amd import _lib, synthetic as syn
    from taxoexpan_amd.taxometric import TaxonomyIndex, host_taxonomic, taxonomic_slots
    dev = torch.device("cuda:0")
    tax = syn.make_named_taxonomy(args.shape, seed=47, features=False)
    t0 = time.perf_counter()
    host = TaxonomyIndex.from_parents(tax.par_ptr, tax.par_idx)
    build_s = time.perf_counter() - t0
    lens = np.diff(host.anc_ptr)
    out = dict(shape=args.shape, n_nodes=host.n_nodes, index_build_s=build_s, closure_entries=int(host.anc_idx.size),
               longest_ancestor_list=int(lens.max()), mean_ancestor_list=float(lens.mean()), max_depth=int(host.depth.max()),
               queries=args.queries, reps=args.reps, host_sample=args.host_sample,
               timing="launch: device events around each launch, median (min..max) after two warm-ups; call: device events around each "
                      "wrapper call, median; host: numpy on host_sample queries, scaled to all")
    index = host.to(dev)
    for K in (1, 5, 64):
        pred, off, idx = make_lists(host.n_nodes, args.queries, K, seed=K)
        p = torch.from_numpy(pred).to(dev)
        goff, gidx = torch.from_numpy(off.astype(np.int32)).to(dev), torch.from_numpy(idx.astype(np.int32)).to(dev)
        res = [torch.empty((args.queries, K), dtype=torch.int32, device=dev) for _ in range(3)]

        def launch():
            _lib.call("txe_taxo_slots", _lib.ptr(index.anc_ptr), _lib.ptr(index.anc_idx), _lib.ptr(index.depth), _lib.ptr(index.par_ptr),
                      _lib.ptr(index.par_idx), index.n_nodes, _lib.ptr(p), args.queries, K, _lib.ptr(goff), _lib.ptr(gidx), int(idx.size),
                      _lib.ptr(res[0]), _lib.ptr(res[1]), _lib.ptr(res[2]), _lib.stream_ptr())

        launch()
        launch()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        got = taxonomic_slots(index, p, off, idx)
        torch.cuda.synchronize()
        tc = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            got = taxonomic_slots(index, p, off, idx)
            e1.record()
            e1.synchronize()
            tc.append(e0.elapsed_time(e1) * 1e-3)
        call_s = float(np.median(tc))
        ns = min(args.host_sample, args.queries)
        t0 = time.perf_counter()
        want = host_taxonomic(host, pred[:ns], off[:ns + 1], idx)
        host_s = (time.perf_counter() - t0) * args.queries / max(ns, 1)
        equal = all(np.array_equal(got[k][:ns].cpu().numpy(), want[k]) and torch.equal(got[k], r)
                    for k, r in zip(("lca_depth", "best_gold", "relation"), res))
        out[f"k{K}"] = dict(slots=args.queries * K, launch_s=float(np.median(ts)), launch_spread=[float(min(ts)), float(max(ts))],
                            call_s=call_s, host_scaled_s=host_s, equal_on_sample=bool(equal),
                            relations=np.bincount(want["relation"].reshape(-1), minlength=7).tolist())
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
