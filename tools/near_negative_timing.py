#!/usr/bin/env python3
"""What near negatives cost on a MAG-CS-shaped masked dataset (tools/sampler_timing.py's: synthetic.make_named_taxonomy("mag_cs"),
sampling_mode 1, 128 queries x (1 + 31) = 4,096 egonets per step, PGAT + Adam + info_nce_loss).  Legs, alternating in ONE process for
--rounds rounds (medians with ranges over the rounds):

  no_near   the DeviceBatchLoader(sampler="device") training loop as it is: txe_sample_anchors' pool instantiation
  near_15   15 of the 31 negative slots near, split 8 siblings / 2 grandparents / 5 uncles: its near instantiation
  mined_15  (unless --no-mined) 15 slots from a table mined once at size 16 with the model as it stands: its table instantiation -- the
            same number of model-ranked slots, for the comparison per step; the mining pass itself is timed once

Each leg reports wall ms per step, the egonet nodes and edges a step held, the sampler launch alone between HIP events, and for near_15
the three accepted shares (accepted proposals / requested slots over the batches the leg sampled).

    python tools/near_negative_timing.py [--steps 60] [--warmup 5] [--rounds 3] [--no-mined]      (steps: at most what one epoch holds)"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from hard_negative_timing import loop_ms  # noqa: E402
from sampler_timing import kernel_us, masked_mag_cs  # noqa: E402
from taxoexpan_amd.data_loaders import DeviceBatchLoader  # noqa: E402
from taxoexpan_amd.optim import Adam  # noqa: E402
from taxoexpan_amd.sampler import mine_hard_negatives  # noqa: E402

NEAR = dict(siblings=8, grandparents=2, uncles=5)


def spread(values):
    """median [min, max]"""
    return [round(float(np.median(values)), 4), round(float(min(values)), 4), round(float(max(values)), 4)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-mined", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "near_negative_timing.py times the MI355X: no GPU found"
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        _tax, train = masked_mag_cs(d)
        print(f"dataset: {train.node_features.shape[0]} nodes, {len(train)} training queries, pool {len(train.all_positions)} "
              f"(built in {time.perf_counter() - t0:.1f} s)", flush=True)
    torch.manual_seed(47)
    model = bench.make_model("pgat", dev)
    opt = Adam(model.parameters(), lr=bench.LR, weight_decay=0, amsgrad=True)
    loader = DeviceBatchLoader(train, bench.N_QUERIES, dev, shuffle=True, seed=0, sampler="device")
    args.steps = min(args.steps, len(loader) - args.warmup)           # (one epoch per loop)
    assert args.steps >= 1
    sampler, k = loader.sampler, loader.sampler.k
    assert sum(NEAR.values()) == 15 and k == 31
    sampled = min(args.warmup + args.steps + 1, len(loader)) * bench.N_QUERIES      # (the loader samples one batch ahead)
    out = dict(steps=args.steps, rounds=args.rounds, n_queries=len(train), n_pool=sampler.n_pool, negative_size=k, near=NEAR)
    table = None
    if not args.no_mined:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        table = mine_hard_negatives(model, train, dev, 16, dtax=loader.dtax)
        torch.cuda.synchronize()
        out["mining_ms_size_16_first_call"] = round(1e3 * (time.perf_counter() - t0), 2)
    legs = ["no_near", "near_15"] + ([] if table is None else ["mined_15"])
    runs = {leg: dict(ms_per_step=[], nodes_per_step=[], edges_per_step=[], sampler_kernel_us=[], shares=[]) for leg in legs}
    for r in range(args.rounds):
        for leg in legs:
            loader.set_near_negatives()
            loader.set_hard_negatives(None, 0)
            if leg == "near_15":
                loader.set_near_negatives(**NEAR)
            elif leg == "mined_15":
                loader.set_hard_negatives(table, 15)
            before = sampler.near_counts()
            res = loop_ms(loader, model, opt, args.steps, args.warmup)
            got = [b - a for a, b in zip(before, sampler.near_counts())]
            rec = runs[leg]
            for f in ("ms_per_step", "nodes_per_step", "edges_per_step"):
                rec[f].append(res[f])
            rec["sampler_kernel_us"].append(kernel_us(sampler, len(train)))
            if leg == "near_15":
                rec["shares"].append([round(x / (sampled * c), 4) for x, c in zip(got, NEAR.values())])
            print(f"round {r} {leg}: {res}", flush=True)
    loader.set_near_negatives()
    loader.set_hard_negatives(None, 0)
    out["legs"] = {}
    for leg, rec in runs.items():
        out["legs"][leg] = {f: spread(rec[f]) for f in ("ms_per_step", "nodes_per_step", "edges_per_step", "sampler_kernel_us")}
        if rec["shares"]:
            out["legs"][leg]["accepted_share_sibling_grandparent_uncle"] = [spread([s[c] for s in rec["shares"]]) for c in range(3)]
    out["padded_slots"] = sampler.padded()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
