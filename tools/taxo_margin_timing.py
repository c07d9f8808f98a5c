#!/usr/bin/env python3
"""What the taxonomy-aware InfoNCE costs, at the MAG-CS training shape (tools/train_epoch_timing.py's dataset, model,
optimizer and loader: 128 queries x 32 columns, PGAT+WMR+LBM on bench.py's synthetic taxonomy):
  - the loss launch alone: device events around each of --calls calls of txe_info_nce_taxo (its launch and its finish step between
    the events) on the anchors of the epoch's first batch, beside txe_info_nce on the same scores, and the two public functions
    loss.taxo_info_nce / loss.info_nce_loss (forward only) the same way, all in this process; medians and ranges;
  - trainer.train_epoch per step without (d) and with (t) taxo_margin: alternating rounds in one process over the same --steps batches
    of an epoch, each leg warmed up first; wall time per step (host clock around an epoch that ends in the log's read-back and a device
    synchronise); medians and ranges over --rounds rounds.

    python tools/taxo_margin_timing.py [--steps 60] [--rounds 5] [--calls 200] [--gamma 0.5]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import train_epoch_timing as tet  # noqa: E402  (tools/train_epoch_timing.py: the dataset, _First, timed, profiled_kernels)
from taxoexpan_amd import _lib, loss  # noqa: E402
from taxoexpan_amd.data_loaders import DeviceBatchLoader  # noqa: E402
from taxoexpan_amd.optim import Adam  # noqa: E402
from taxoexpan_amd.taxometric import TaxonomyIndex  # noqa: E402
from taxoexpan_amd.trainer import train_epoch  # noqa: E402


def event_timed(fn, calls):
    """device events around each of `calls` calls of fn (20 more first): microseconds"""
    us = []
    for c in range(20 + calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        if c >= 20:
            us.append(1e3 * t0.elapsed_time(t1))
    return us


def loss_launch_alone(loader, index, dev, gamma, calls):
    anchors = next(iter(loader))[0].anchors
    lib = _lib.load()
    Q, C = anchors.shape
    torch.manual_seed(1)
    x = torch.rand(Q, C, device=dev) * 12 - 6
    d_x, out = torch.empty(Q, C, device=dev), torch.empty(1, device=dev)
    wsb = lib.txe_info_nce_taxo_ws_bytes(Q)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    stream = _lib.stream_ptr()

    def taxo():
        assert lib.txe_info_nce_taxo(x.data_ptr(), C, Q, C, anchors.data_ptr(), C, index.anc_ptr.data_ptr(), index.anc_idx.data_ptr(),
                                     index.depth.data_ptr(), index.n_nodes, gamma, out.data_ptr(), d_x.data_ptr(), C, None, None,
                                     ws.data_ptr(), wsb, stream) == 0

    def plain():
        assert lib.txe_info_nce(x.data_ptr(), C, Q, C, None, out.data_ptr(), d_x.data_ptr(), C, stream) == 0

    rows = [("txe_info_nce_taxo (launch + finish)", event_timed(taxo, calls)), ("txe_info_nce", event_timed(plain, calls)),
            ("loss.taxo_info_nce (forward)", event_timed(lambda: loss.taxo_info_nce(x, anchors, index, gamma), calls)),
            ("loss.info_nce_loss (forward)", event_timed(lambda: loss.info_nce_loss(x), calls))]
    return Q, C, rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--gamma", type=float, default=0.5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "taxo_margin_timing.py times the MI355X: no GPU found"
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        ds = tet.masked_mag_cs_train(d)
        print(f"dataset: {ds.node_features.shape[0]} nodes, {len(ds)} training queries (built in {time.perf_counter() - t0:.1f} s)", flush=True)
    t0 = time.perf_counter()
    host_index = TaxonomyIndex.from_dataset(ds)
    index = host_index.to(dev)
    rows = np.diff(host_index.anc_ptr)
    print(f"taxonomy index: closure rows mean {rows.mean():.1f}, longest {rows.max()} (staging capacity {_lib.TAXO_STAGE_CAP}); built in "
          f"{time.perf_counter() - t0:.1f} s", flush=True)
    torch.manual_seed(47)
    model = bench.make_model("pgat", dev)
    opt = Adam(model.parameters(), lr=bench.LR, weight_decay=0, amsgrad=True)
    loaders = {"d": DeviceBatchLoader(ds, tet.BS, dev, shuffle=True, seed=0, sampler="device"),
               "t": DeviceBatchLoader(ds, tet.BS, dev, shuffle=True, seed=0, sampler="device", attach_anchors=True)}
    steps = min(args.steps, len(loaders["d"]))

    def leg(name, n):
        kw = dict(taxo_margin=args.gamma, taxonomy_index=index) if name == "t" else {}
        t, r = tet.timed(lambda: train_epoch(model, tet._First(loaders[name], n), opt, **kw))
        assert r["first_nonfinite"] == -1, "the model diverged: the timing is void"
        return t, r

    for name in "dt":                                           # warm-up: first-call costs, allocator, every shape of the timed window
        leg(name, min(30, steps))
    ms = {name: [] for name in "dt"}
    for r in range(args.rounds):
        line = []
        for name in "dt":
            t, res = leg(name, steps)
            ms[name].append(1e3 * t / res["n_batches"])
            line.append(f"({name}) {ms[name][-1]:.3f} ms/step [loss {res['loss']:.2f}"
                        + (f", mean taxonomic distance {res['mean_taxo_distance']:.3f}]" if name == "t" else "]"))
        print(f"round {r}: " + " | ".join(line), flush=True)
    for name, what in (("d", "default step"), ("t", f"taxo_margin={args.gamma}")):
        v = ms[name]
        print(f"({name}) {what}: median {float(np.median(v)):.3f} ms/step, range {min(v):.3f}-{max(v):.3f} over {len(v)} rounds of {steps} steps")
    delta = float(np.median(ms["t"])) - float(np.median(ms["d"]))
    spread = max(max(v) - min(v) for v in ms.values())
    print(f"difference of the medians {delta:+.3f} ms/step; the widest range of a leg is {spread:.3f} ms/step"
          + (" -- the difference lies inside the run's spread" if abs(delta) <= spread else ""))
    Q, C, table = loss_launch_alone(loaders["t"], index, dev, args.gamma, args.calls)
    for what, us in table:
        print(f"{what}, [{Q}, {C}] scores: median {float(np.median(us)):.2f} us, range {min(us):.2f}-{max(us):.2f} over {len(us)} calls")
    prof = tet.profiled_kernels(model, loaders["t"], opt, min(steps, 30), taxo_margin=args.gamma, taxonomy_index=index)
    for kname in ("info_nce_taxo_kernel", "info_nce_taxo_finish_kernel"):
        if kname in prof:
            mean, med, n, _work = prof[kname]
            print(f"{kname}: mean {mean:.2f} us, median {med:.2f} us over {n} launches inside leg (t)")


if __name__ == "__main__":
    main()
