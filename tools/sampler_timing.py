#!/usr/bin/env python3
"""The training loop of INTEGRATION.md -- `for g, x, qf, label in DeviceBatchLoader(train, 128, ...)` -- on a MAG-CS-shaped masked dataset
(synthetic.make_named_taxonomy("mag_cs") written as raw .terms / .taxo / .terms.embed files and read back; sampling_mode 1, 128 queries
x (1 + 31) = 4,096 egonets per step), with the host sampler (dataset.sample_anchors) and with the device sampler (csrc/txe_sample.hip:
txe_sample_anchors without a table or near slots, its pool-only instantiation).
Prints, per sampler: host ms spent in next(), wall ms per PGAT step (bench.make_model("pgat"), Adam, info_nce_loss); the sampler
kernel's time from HIP events around single launches; the host time of next()'s two halves; and, for comparison, bench.py's
resident-batch step and its fresh-batch loop (numpy sampler without masks, batch i+1 begun before step i) measured in the same process.

    python tools/sampler_timing.py [--steps 30] [--warmup 5]"""
import argparse
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from taxoexpan_amd import graph as Gr, synthetic as syn  # noqa: E402
from taxoexpan_amd.data_loaders import DeviceBatchLoader, finish_device_batch  # noqa: E402
from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset  # noqa: E402
from taxoexpan_amd.loss import info_nce_loss  # noqa: E402
from taxoexpan_amd.optim import Adam  # noqa: E402


def masked_mag_cs(directory):
    tax = syn.make_named_taxonomy("mag_cs", seed=47)
    syn.write_raw(directory, "magcs", syn.taxonomy_edges(tax), tax.features.numpy())
    random.seed(0)
    raw = MAGDataset("magcs", directory, raw=True)
    return tax, MaskedGraphDataset(raw, mode="train", sampling_mode=1, negative_size=bench.NEG, expand_factor=50, normalize_embed=True)


def step(model, opt, g, x, qf, Q):
    opt.zero_grad(set_to_none=True)
    loss = info_nce_loss(model(g, x, qf).reshape(Q, -1))
    loss.backward()
    opt.step()
    return loss


def loader_loop(train, model, opt, dev, sampler, steps, warmup):
    loader = DeviceBatchLoader(train, bench.N_QUERIES, dev, shuffle=True, seed=0, sampler=sampler)
    assert len(loader) >= steps + warmup
    it = iter(loader)
    for _ in range(warmup):
        g, x, qf, _label = next(it)
        step(model, opt, g, x, qf, bench.N_QUERIES)
    torch.cuda.synchronize()
    t_next = 0.0
    t0 = time.perf_counter()
    for _ in range(steps):
        a = time.perf_counter()
        g, x, qf, _label = next(it)
        t_next += time.perf_counter() - a
        loss = step(model, opt, g, x, qf, bench.N_QUERIES)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps
    bench.assert_finite(model, loss, f"sampler={sampler}")
    return loader, 1e3 * t_next / steps, 1e3 * wall


def kernel_us(sampler, n_queries, reps=50):
    """median of `reps` single launches of the 128-query sampler between HIP events on a side stream"""
    side = torch.cuda.Stream(device=sampler.device)
    order = list(range(n_queries))
    random.Random(1).shuffle(order)
    order_dev = sampler.upload_order(order, side)
    ts = []
    with torch.cuda.stream(side):
        for r in range(reps + 5):
            start = (r * bench.N_QUERIES) % (n_queries - bench.N_QUERIES)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            sampler.launch(order_dev, start, bench.N_QUERIES, 1000 + r, True, side)
            e1.record()
            e1.synchronize()
            if r >= 5:
                ts.append(1e3 * e0.elapsed_time(e1))
    return float(np.median(ts))


def next_breakdown(sampler, n_queries, reps=30):
    """host ms of the two halves of a device-sampled next(): sampler.begin (sampler launch + node-count launch + the count's read-back
    enqueued) and finish_device_batch (fill, feature gathers, walk plan), with the device idle -- and of the sampler launch alone"""
    side = torch.cuda.Stream(device=sampler.device)
    order = list(range(n_queries))
    random.Random(2).shuffle(order)
    order_dev = sampler.upload_order(order, side)
    t_launch = t_begin = t_finish = 0.0
    for r in range(reps + 3):
        start = (r * bench.N_QUERIES) % (n_queries - bench.N_QUERIES)
        torch.cuda.synchronize()
        a = time.perf_counter()
        sampler.launch(order_dev, start, bench.N_QUERIES, 2000 + r, True, side)
        b = time.perf_counter()
        pend = sampler.begin(order_dev, start, bench.N_QUERIES, 3000 + r, True, side, egonet_seed=r)
        c = time.perf_counter()
        finish_device_batch(pend, sampler.dtax.features)
        d = time.perf_counter()
        if r >= 3:
            t_launch, t_begin, t_finish = t_launch + b - a, t_begin + c - b, t_finish + d - c
    torch.cuda.synchronize()
    return dict(sampler_launch_host_ms=round(1e3 * t_launch / reps, 4), begin_host_ms=round(1e3 * t_begin / reps, 4),
                finish_host_ms=round(1e3 * t_finish / reps, 4))


def bench_reference(tax, model, opt, dev, steps, warmup):
    """bench.py's resident-batch step and its fresh-batch loop (step_incl_batch_build_repeated_queries_ms), same model"""
    target = torch.zeros(bench.N_QUERIES, dtype=torch.long, device=dev)
    batches = bench.build_batches(tax, 2, seed0=1, device=dev)
    it = iter(range(10 ** 9))
    resident = bench.median_time(lambda: bench.train_step(model, opt, batches[next(it) % 2], target, 1), reps=5, inner=steps, warm=warmup)
    dtax = Gr.DeviceTaxonomy(tax.par_ptr, tax.par_idx, tax.chd_ptr, tax.chd_idx, tax.features, dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for i in range(warmup):
        bench.train_step(model, opt, bench.fresh_batch(tax, dtax, 5000 + i, dev, side), target, 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pend = bench.fresh_batch_begin(tax, dtax, 6000, dev, side, True)
    for i in range(steps):
        b = finish_device_batch(pend, dtax.features)
        if i + 1 < steps:
            pend = bench.fresh_batch_begin(tax, dtax, 6000 + 17 * (i + 1), dev, side, True)
        bench.train_step(model, opt, b, target, 1)
    torch.cuda.synchronize()
    return 1e3 * resident, 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sampler_timing.py times the MI355X: no GPU found"
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        tax, train = masked_mag_cs(d)
        print(f"dataset: {train.node_features.shape[0]} nodes, {len(train)} training queries, pool {len(train.all_positions)} "
              f"(built in {time.perf_counter() - t0:.1f} s)", flush=True)
    torch.manual_seed(47)
    model = bench.make_model("pgat", dev)
    opt = Adam(model.parameters(), lr=bench.LR, weight_decay=0, amsgrad=True)
    out = {}
    for sampler in ("host", "device"):
        loader, next_ms, wall_ms = loader_loop(train, model, opt, dev, sampler, args.steps, args.warmup)
        out[sampler] = dict(next_host_ms=round(next_ms, 4), loop_wall_ms_per_step=round(wall_ms, 4))
        if sampler == "device":
            out[sampler]["padded_slots"] = loader.sampler.padded()
            out[sampler]["sampler_kernel_us"] = round(kernel_us(loader.sampler, len(train)), 2)
            out[sampler]["next_breakdown"] = next_breakdown(loader.sampler, len(train))
        print(f"sampler={sampler}: {out[sampler]}", flush=True)
    resident_ms, fresh_ms = bench_reference(tax, model, opt, dev, args.steps, args.warmup)
    out["bench"] = dict(resident_ms_per_step=round(resident_ms, 4), fresh_batch_loop_ms_per_step=round(fresh_ms, 4))
    print(f"bench: {out['bench']}")
    print(f"device loop / bench fresh-batch loop: {out['device']['loop_wall_ms_per_step'] / fresh_ms:.3f}")


if __name__ == "__main__":
    main()
