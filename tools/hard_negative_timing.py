#!/usr/bin/env python3
"""What hard-negative mining costs on a MAG-CS-shaped masked dataset (tools/sampler_timing.py's: synthetic.make_named_taxonomy("mag_cs"),
sampling_mode 1, 128 queries x (1 + 31) = 4,096 egonets per step, PGAT + Adam + info_nce_loss):

  mining   sampler.mine_hard_negatives for all training queries x the pool at size 16 and 64, split into encode (candidate egonets +
           encoder), score (the matcher's block kernel) and select (ops.select_k with the masks); median of --reps runs after a warm-up
  loop     wall ms per step of the DeviceBatchLoader(sampler="device") training loop without a table (txe_sample_anchors, pool only), with a table
           and hard_slots = 0, and with hard_slots = negative_size // 2 (both its table route), each with the egonet nodes and
           edges a step held; the table-free loop runs twice (first and last) -- the spread of the same code -- and the sampler launch
           alone is timed between HIP events

    python tools/hard_negative_timing.py [--steps 100] [--warmup 5] [--reps 3]      (steps: at most what one epoch holds)"""
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
from sampler_timing import kernel_us, masked_mag_cs, step  # noqa: E402
from taxoexpan_amd.data_loaders import DeviceBatchLoader  # noqa: E402
from taxoexpan_amd.optim import Adam  # noqa: E402
from taxoexpan_amd.sampler import mine_hard_negatives  # noqa: E402


def mining_ms(model, train, dev, size, dtax, reps):
    """median ms of encode / score / select / the whole call over `reps` runs of mine_hard_negatives (one warm-up first)"""
    runs = []
    table = None
    for r in range(reps + 1):
        t = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        table = mine_hard_negatives(model, train, dev, size, dtax=dtax, timings=t)
        torch.cuda.synchronize()
        t["total"] = time.perf_counter() - t0
        if r:
            runs.append(t)
    return table, {name: round(1e3 * float(np.median([t[name] for t in runs])), 3) for name in ("encode", "score", "select", "total")}


def loop_ms(loader, model, opt, steps, warmup):
    """`steps` steps of one epoch of `loader` after `warmup` steps: wall ms per step, and what a step held -- the batch's egonet nodes
    and edges (hard negatives are other anchors than uniform ones, so other graphs) and the last loss"""
    it = iter(loader)
    for _ in range(warmup):
        g, x, qf, _label = next(it)
        step(model, opt, g, x, qf, bench.N_QUERIES)
    torch.cuda.synchronize()
    nodes = edges = 0
    t0 = time.perf_counter()
    for _ in range(steps):
        g, x, qf, _label = next(it)
        nodes, edges = nodes + g.number_of_nodes(), edges + g.number_of_edges()      # (host-known: no read-back)
        loss = step(model, opt, g, x, qf, bench.N_QUERIES)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps
    bench.assert_finite(model, loss, "hard_negative_timing")
    del it                                                         # (the epoch ends here: the table may change again)
    return dict(ms_per_step=round(1e3 * wall, 4), nodes_per_step=round(nodes / steps, 1), edges_per_step=round(edges / steps, 1),
                last_loss=round(float(loss), 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "hard_negative_timing.py times the MI355X: no GPU found"
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
    k = loader.sampler.k
    out = dict(steps=args.steps, n_queries=len(train), n_pool=loader.sampler.n_pool, steps_per_epoch=len(loader), negative_size=k,
               mining_ms={}, loop_ms_per_step={}, sampler_kernel_us={})
    out["loop_ms_per_step"]["no_table_first"] = loop_ms(loader, model, opt, args.steps, args.warmup)
    out["sampler_kernel_us"]["no_table"] = round(kernel_us(loader.sampler, len(train)), 2)
    table = None
    for size in (16, 64):
        table, out["mining_ms"][f"size_{size}"] = mining_ms(model, train, dev, size, loader.dtax, args.reps)
        print(f"mining size={size}: {out['mining_ms'][f'size_{size}']}", flush=True)
    out["hard_mean_count"] = float(table.cnt.double().mean().item())
    for name, slots in (("hard_slots_0", 0), ("hard_slots_half", k // 2)):
        loader.set_hard_negatives(table, slots)
        out["loop_ms_per_step"][name] = loop_ms(loader, model, opt, args.steps, args.warmup)
        out["sampler_kernel_us"][name] = round(kernel_us(loader.sampler, len(train)), 2)
    loader.set_hard_negatives(None, 0)
    out["loop_ms_per_step"]["no_table_last"] = loop_ms(loader, model, opt, args.steps, args.warmup)
    out["padded_slots"] = loader.sampler.padded()
    out["epoch_ms_no_table"] = [round(out["loop_ms_per_step"][name]["ms_per_step"] * len(loader), 1) for name in ("no_table_first", "no_table_last")]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
