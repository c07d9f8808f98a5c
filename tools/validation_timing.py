#!/usr/bin/env python3
"""One validation epoch (trainer.py:96-124) on a MAG-CS-shaped masked dataset (synthetic.make_named_taxonomy("mag_cs", seed=47) written as
raw files and read back; validation mode, sampling_mode 0, negative_size 256, batches of 128 queries, bench.make_model("pgat")), two
legs alternating in one process:
  (a) the parent's route: DeviceBatchLoader(sampler="host") (dataset.sample_anchors in host Python), the model forward, and the batch's
      ranks and metrics on the host by the numpy restatement below (the reference's obtain_ranks and metric formulas);
  (b) DeviceBatchLoader(sampler="device") (csrc/txe_sample.hip, sampling_mode 0) + evaluate.validate (csrc/txe_grouprank.hip).
Prints per leg and epoch: the wall time, host ms per next(); for (b) also the sampler's kernel time and the rank-and-metric kernel time
from HIP events around single launches.

    python tools/validation_timing.py [--epochs 3]"""
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
from taxoexpan_amd import _lib, metric, synthetic as syn  # noqa: E402
from taxoexpan_amd.data_loaders import DeviceBatchLoader  # noqa: E402
from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset  # noqa: E402
from taxoexpan_amd.evaluate import VALIDATION_METRICS, validate  # noqa: E402

BS, K = 128, 256


def masked_mag_cs_validation(directory):
    tax = syn.make_named_taxonomy("mag_cs", seed=47)
    syn.write_raw(directory, "magcs", syn.taxonomy_edges(tax), tax.features.numpy())
    random.seed(0)
    raw = MAGDataset("magcs", directory, raw=True)
    return MaskedGraphDataset(raw, mode="validation", sampling_mode=0, negative_size=K, expand_factor=50, normalize_embed=True)


def host_metrics(pred, label, mode=1):
    """leg (a)'s host work per batch: the reference's obtain_ranks (groups at every 0 -> 1 label transition, rank = 1 + better negatives of
    the group) and macro_mr, micro_mr, hit_at_1, hit_at_3, mrr_scaled_10, in numpy"""
    s = pred.cpu().numpy().reshape(-1)
    lab = label.cpu().numpy()
    starts = np.flatnonzero(np.concatenate([[True], (lab[:-1] == 0) & (lab[1:] == 1)]))
    ends = np.append(starts[1:], len(lab))
    groups = []
    for a, b in zip(starts, ends):
        g, pos = s[a:b], lab[a:b] == 1
        better = g[~pos][None, :] > g[pos][:, None] if mode == 1 else g[~pos][None, :] < g[pos][:, None]
        groups.append(1 + better.sum(1))
    flat = np.concatenate(groups)
    return np.array([np.mean([r.mean() for r in groups]), flat.mean(), (flat <= 1).mean(), (flat <= 3).mean(), (1.0 / np.ceil(flat / 10)).mean()])


def leg_a(val, model, dev):
    loader = DeviceBatchLoader(val, BS, dev, shuffle=True, seed=0, sampler="host")
    model.eval()
    total, t_next, n = np.zeros(5), 0.0, 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        it = iter(loader)
        while True:
            a = time.perf_counter()
            try:
                g, x, qf, label = next(it)
            except StopIteration:
                break
            t_next += time.perf_counter() - a
            total += host_metrics(model(g, x, qf), label)
            n += 1
    torch.cuda.synchronize()
    return time.perf_counter() - t0, 1e3 * t_next / n, (total / n).tolist()


class _Timed:
    """an iterable over a loader that adds up the host time of every next()"""

    def __init__(self, loader):
        self.loader, self.t_next, self.n = loader, 0.0, 0

    def __iter__(self):
        it = iter(self.loader)
        while True:
            a = time.perf_counter()
            try:
                b = next(it)
            except StopIteration:
                return
            self.t_next += time.perf_counter() - a
            self.n += 1
            yield b


def leg_b(val, model, dev):
    loader = DeviceBatchLoader(val, BS, dev, shuffle=True, seed=0, sampler="device")
    timed = _Timed(loader)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = validate(model, timed, metrics=VALIDATION_METRICS, larger_is_better=True)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, 1e3 * timed.t_next / timed.n, out["val_metrics"], loader


def kernel_us(loader, model, dev, reps=20):
    """medians over `reps` single launches between HIP events: txe_sample_groups for 128 queries; txe_group_rank + txe_group_metrics on
    one validation batch's scores"""
    s = loader.sampler
    order = list(range(len(loader.dataset)))
    random.Random(1).shuffle(order)
    order_dev = s.upload_order(order)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    t_s, t_r = [], []
    for r in range(reps + 3):
        e0, e1 = ev(), ev()
        e0.record()
        s.launch(order_dev, (r * BS) % (len(order) - BS), BS, 500 + r, True)
        e1.record()
        e1.synchronize()
        if r >= 3:
            t_s.append(1e3 * e0.elapsed_time(e1))
    g, x, qf, label = next(iter(loader))
    with torch.no_grad():
        pred = model.eval()(g, x, qf)
    score, label = metric._check_batch(pred, label)
    acc = torch.zeros(7, dtype=torch.float64, device=dev)
    for r in range(reps + 3):
        e0, e1 = ev(), ev()
        e0.record()
        ranks, pos_off, counts = metric._device_group_ranks(score, label, 1)
        _lib.call("txe_group_metrics", _lib.ptr(ranks), _lib.ptr(pos_off), _lib.ptr(counts), 0x53210, 5, _lib.ptr(acc), _lib.stream_ptr())
        e1.record()
        e1.synchronize()
        if r >= 3:
            t_r.append(1e3 * e0.elapsed_time(e1))
    return float(np.median(t_s)), float(np.median(t_r)), int(score.shape[0])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--epochs", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "validation_timing.py times the MI355X: no GPU found"
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        val = masked_mag_cs_validation(d)
        print(f"dataset: {val.node_features.shape[0]} nodes, {len(val)} validation queries, pool {len(val.all_positions)} "
              f"(built in {time.perf_counter() - t0:.1f} s)", flush=True)
    torch.manual_seed(47)
    model = bench.make_model("pgat", dev)
    leg_a(val, model, dev)                                   # warm-up of both legs (first-call costs, allocator)
    _w, _n, _m, loader = leg_b(val, model, dev)
    a_s, b_s = [], []
    for e in range(args.epochs):
        wa, na, ma = leg_a(val, model, dev)
        wb, nb, mb, loader = leg_b(val, model, dev)
        a_s.append(wa)
        b_s.append(wb)
        print(f"epoch {e}: (a) host route {1e3 * wa:.1f} ms/epoch, next() {na:.3f} ms | (b) device route {1e3 * wb:.1f} ms/epoch, "
              f"next() {nb:.3f} ms | macro_mr (a) {ma[0]:.2f} (b) {mb[0]:.2f}", flush=True)
    ks, kr, B = kernel_us(loader, model, dev)
    print(f"sampler kernels (128 queries x <= {K}): {ks:.1f} us; rank + metrics on one batch (B = {B}): {kr:.1f} us; padded queries "
          f"{loader.sampler.padded()}")
    print(f"summary: (a) {1e3 * min(a_s):.1f}-{1e3 * max(a_s):.1f} ms/epoch, (b) {1e3 * min(b_s):.1f}-{1e3 * max(b_s):.1f} ms/epoch; "
          f"(b) <= (a) in every epoch: {all(b <= a for a, b in zip(a_s, b_s))}")


if __name__ == "__main__":
    main()
