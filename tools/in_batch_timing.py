#!/usr/bin/env python3
"""What training on in-batch negatives costs per step, at the MAG-CS shape (tools/train_epoch_timing.py's dataset, model, optimizer and
loader: 128 queries x 32 egonets, PGAT+WMR+LBM), three legs alternating in one process over the same --steps batches of an epoch:
  (d) trainer.train_epoch on the default route (the output layer folded into the matcher, the grouped loss);
  (m) the same with ops._NO_MATCH_FOLD: hg materialised, the grouped loss -- what the in-batch step adds its launches to;
  (i) trainer.train_epoch(in_batch=True): hg materialised, loss.in_batch_info_nce (two products, exp, the loss's two launches, three
      products back).
Each leg is warmed up first; per round the wall time per step (host clock around an epoch that ends in the log's read-back and a device
synchronise); medians and ranges over --rounds rounds.  Then the loss launch alone -- txe_inbatch_nce on a [128, 4096] score matrix with
the epoch's first batch's groups -- with device events around each of --calls calls, and leg (i)'s library launches by kernel name.

    python tools/in_batch_timing.py [--steps 60] [--rounds 5] [--calls 200]"""
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
from taxoexpan_amd import _lib, ops  # noqa: E402
from taxoexpan_amd.data_loaders import DeviceBatchLoader  # noqa: E402
from taxoexpan_amd.optim import Adam  # noqa: E402
from taxoexpan_amd.trainer import train_epoch  # noqa: E402


def leg(name, model, loaders, opt, steps):
    """one epoch part of `steps` steps on leg d / m / i: (seconds, train_epoch's dict, the match route it took)"""
    prev = ops._NO_MATCH_FOLD
    ops._NO_MATCH_FOLD = name == "m"
    ops.ROUTES.pop("match", None)
    try:
        t, r = tet.timed(lambda: train_epoch(model, tet._First(loaders[name], steps), opt, in_batch=name == "i"))
    finally:
        ops._NO_MATCH_FOLD = prev
    assert r["first_nonfinite"] == -1, "the model diverged: the timing is void"
    return t, r, ops.ROUTES.get("match", "-")


def loss_launch_alone(loader, dev, calls):
    """txe_inbatch_nce on a fresh [Q, G] score matrix per call (in place), device events around each call: microseconds"""
    g = next(iter(loader))[0].in_batch
    lib = _lib.load()
    Q, G = g.Q, g.G
    torch.manual_seed(1)
    scores = torch.rand(Q, G, device=dev) * 12 - 6
    wsb = lib.txe_inbatch_nce_ws_bytes(Q)
    ws, loss = torch.empty(wsb, dtype=torch.uint8, device=dev), torch.empty(1, device=dev)
    us = []
    for c in range(20 + calls):
        S = scores.clone()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        rc = lib.txe_inbatch_nce(S.data_ptr(), G, Q, G, g.pos_col.data_ptr(), g.anchor.data_ptr(), g.qnode.data_ptr(), g.mask_ptr.data_ptr(),
                                 g.mask_idx.data_ptr(), 1, loss.data_ptr(), S.data_ptr(), G, None, None, ws.data_ptr(), wsb, _lib.stream_ptr())
        t1.record()
        t1.synchronize()
        assert rc == 0
        if c >= 20:
            us.append(1e3 * t0.elapsed_time(t1))
    return Q, G, us


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "in_batch_timing.py times the MI355X: no GPU found"
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        ds = tet.masked_mag_cs_train(d)
        print(f"dataset: {ds.node_features.shape[0]} nodes, {len(ds)} training queries (built in {time.perf_counter() - t0:.1f} s)", flush=True)
    torch.manual_seed(47)
    model = bench.make_model("pgat", dev)
    opt = Adam(model.parameters(), lr=bench.LR, weight_decay=0, amsgrad=True)
    plain = DeviceBatchLoader(ds, tet.BS, dev, shuffle=True, seed=0, sampler="device")
    loaders = {"d": plain, "m": plain, "i": DeviceBatchLoader(ds, tet.BS, dev, shuffle=True, seed=0, sampler="device", in_batch=True)}
    steps = min(args.steps, len(plain))
    for name in "dmi":                                          # warm-up: first-call costs, allocator, every shape of the timed window
        leg(name, model, loaders, opt, min(30, steps))
    ms = {name: [] for name in "dmi"}
    for r in range(args.rounds):
        line = []
        for name in "dmi":
            t, res, route = leg(name, model, loaders, opt, steps)
            ms[name].append(1e3 * t / res["n_batches"])
            line.append(f"({name}) {ms[name][-1]:.3f} ms/step [match route {route}, loss {res['loss']:.2f}"
                        + (f", mean negatives {res['mean_negatives']:.1f}]" if name == "i" else "]"))
        print(f"round {r}: " + " | ".join(line), flush=True)
    for name, what in (("d", "default route"), ("m", "_NO_MATCH_FOLD"), ("i", "in_batch=True")):
        v = ms[name]
        print(f"({name}) {what}: median {float(np.median(v)):.3f} ms/step, range {min(v):.3f}-{max(v):.3f} over {len(v)} rounds of {steps} steps")
    print(f"in-batch over _NO_MATCH_FOLD: {float(np.median(ms['i'])) - float(np.median(ms['m'])):+.3f} ms/step at the medians; over the default "
          f"route: {float(np.median(ms['i'])) - float(np.median(ms['d'])):+.3f} ms/step")
    Q, G, us = loss_launch_alone(loaders["i"], dev, args.calls)
    print(f"txe_inbatch_nce alone, [{Q}, {G}] scores, chain_exp 1, in place (both launches between the events): median "
          f"{float(np.median(us)):.2f} us, range {min(us):.2f}-{max(us):.2f} over {len(us)} calls")
    prof = tet.profiled_kernels(model, loaders["i"], opt, min(steps, 30), in_batch=True)
    for kname in ("inbatch_nce_kernel", "inbatch_nce_finish_kernel", "inbatch_exp_kernel"):
        if kname in prof:
            mean, med, n, _work = prof[kname]
            print(f"{kname}: mean {mean:.2f} us, median {med:.2f} us over {n} launches inside leg (i)")
    print(f"leg (i): {sum(v[2] for v in prof.values()) / min(steps, 30):.1f} library launches per step")


if __name__ == "__main__":
    main()
