#!/usr/bin/env python3
"""What training the term-embedding table costs per step, at the MAG-CS shape (tools/train_epoch_timing.py's dataset, model, optimizer and
device-sampling loader: 128 queries x 32 = 4,096 egonets, PGAT+WMR+LBM).
  1. the DEFAULT step (no table) of this tree and, with --parent DIR, of another checkout (the parent commit, built): fresh child
     processes of this same file, alternating, each printing its ms/step per round -- the two must agree within the run's spread;
  2. in this process, alternating per round: (d) trainer.train_epoch as it is, (t) train_epoch(feature_table=...) on a loader that
     gathers from the table;
  3. the two new launches alone (txe_rowgrad_group + txe_sparse_adam_rows) on one training batch's per-occurrence gradients, device events
     around each pair of calls;
  4. the torch alternatives on the same ids and gradients, from the gathers' backward to the updated table: a dense nn.Parameter table
     with index_select and torch.optim.Adam, and nn.Embedding(sparse=True) with torch.optim.SparseAdam.
Wall times are a host clock around an epoch part that ends in the log's read-back and a device synchronise; medians and ranges over
--rounds rounds.  No accuracy is measured here.

    python tools/feature_table_timing.py [--steps 60] [--rounds 5] [--calls 200] [--parent DIR]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _tree_imports(tree):
    """bench, tools/train_epoch_timing and the package of the checkout at `tree`"""
    sys.path[:0] = [os.path.join(tree, "tools"), tree]
    import bench
    import train_epoch_timing as tet
    return bench, tet


def child_default(tree, steps, rounds):
    """the default step of the checkout at `tree`: one JSON line {"ms": [per round]}"""
    bench, tet = _tree_imports(tree)
    from taxoexpan_amd.data_loaders import DeviceBatchLoader
    from taxoexpan_amd.optim import Adam
    from taxoexpan_amd.trainer import train_epoch
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as d:
        ds = tet.masked_mag_cs_train(d)
    torch.manual_seed(47)
    model = bench.make_model("pgat", dev)
    opt = Adam(model.parameters(), lr=bench.LR, weight_decay=0, amsgrad=True)
    loader = DeviceBatchLoader(ds, tet.BS, dev, shuffle=True, seed=0, sampler="device")
    steps = min(steps, len(loader))
    train_epoch(model, tet._First(loader, min(30, steps)), opt)
    ms = []
    for _ in range(rounds):
        t, r = tet.timed(lambda: train_epoch(model, tet._First(loader, steps), opt))
        assert r["first_nonfinite"] == -1
        ms.append(1e3 * t / r["n_batches"])
    print(json.dumps({"ms": ms, "steps": steps}), flush=True)


def spread(v):
    return f"median {float(np.median(v)):.3f}, range {min(v):.3f}-{max(v):.3f}"


def launches_alone(table, ids_a, d_a, ids_b, d_b, calls):
    """microseconds of txe_rowgrad_group + txe_sparse_adam_rows per call pair (the table keeps stepping: the rows touched do not change)"""
    from taxoexpan_amd import _lib
    lib = _lib.load()
    na, nb, (n_rows, d) = ids_a.numel(), ids_b.numel(), table.weight.shape
    wsb = lib.txe_rowgrad_ws_bytes(na, nb)
    ws = torch.empty(wsb, dtype=torch.uint8, device=table.device)
    x = table.max_exp_avg_sq
    us = []
    for c in range(20 + calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        rc = lib.txe_rowgrad_group(ids_a.data_ptr(), na, ids_b.data_ptr(), nb, n_rows, ws.data_ptr(), wsb, _lib.stream_ptr())
        rc |= lib.txe_sparse_adam_rows(table.weight.data_ptr(), table.exp_avg.data_ptr(), table.exp_avg_sq.data_ptr(),
                                       None if x is None else x.data_ptr(), d, n_rows, d, d_a.data_ptr(), d_a.stride(0), na, d_b.data_ptr(),
                                       d_b.stride(0), nb, ws.data_ptr(), wsb, None, table.lr, table.betas[0], table.betas[1], table.eps,
                                       c + 1, None, _lib.stream_ptr())
        t1.record()
        t1.synchronize()
        assert rc == 0
        if c >= 20:
            us.append(1e3 * t0.elapsed_time(t1))
    return us


def torch_alternatives(weight, ids_a, d_a, ids_b, d_b, calls, lr):
    """from the gathers' backward to the updated table, microseconds per step: {name: [us]}"""
    ia, ib = ids_a.long(), ids_b.long()
    out = {}
    dense = torch.nn.Parameter(weight.detach().clone())
    emb = torch.nn.Embedding(weight.shape[0], weight.shape[1], sparse=True, _weight=weight.detach().clone()).to(weight.device)
    legs = {"dense nn.Parameter + index_select + torch.optim.Adam(amsgrad)":
            (torch.optim.Adam([dense], lr=lr, amsgrad=True), lambda: (dense.index_select(0, ia), dense.index_select(0, ib))),
            "nn.Embedding(sparse=True) + torch.optim.SparseAdam":
            (torch.optim.SparseAdam(list(emb.parameters()), lr=lr), lambda: (emb(ia), emb(ib)))}
    for name, (opt, gather) in legs.items():
        us = []
        for c in range(10 + calls):
            opt.zero_grad(set_to_none=True)
            xa, xb = gather()                                    # (the forward gathers are outside the timed window, as for the kernels)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            torch.autograd.backward([xa, xb], [d_a, d_b])
            opt.step()
            t1.record()
            t1.synchronize()
            if c >= 10:
                us.append(1e3 * t0.elapsed_time(t1))
        out[name] = us
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--parent", default=None, metavar="DIR", help="a built checkout of the parent commit to time the default step of")
    ap.add_argument("--child-default", default=None, metavar="TREE", help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "feature_table_timing.py times the MI355X: no GPU found"
    if args.child_default:
        return child_default(os.path.abspath(args.child_default), args.steps, args.rounds)
    root = os.path.dirname(HERE)
    # 1. the default step, this tree and the parent's, alternating fresh processes
    trees = [("this tree", root)] + ([("parent", os.path.abspath(args.parent))] if args.parent else [])
    ms = {name: [] for name, _ in trees}
    for rep in range(2):
        for name, tree in trees:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-default", tree, "--steps", str(args.steps), "--rounds",
                                str(args.rounds)], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit(f"the child for {name} failed ({r.returncode}):\n{r.stderr[-2000:]}")
            got = json.loads(r.stdout.strip().splitlines()[-1])
            ms[name] += got["ms"]
            print(f"default step, {name}, process {rep}: " + " ".join(f"{v:.3f}" for v in got["ms"]) + " ms/step", flush=True)
    for name, _ in trees:
        print(f"default step, {name}: {spread(ms[name])} ms/step over {len(ms[name])} rounds of {args.steps} steps in 2 processes")
    if not args.parent:
        print("default step, parent: not measured (no --parent)")
    # 2. with and without the table, one process
    bench, tet = _tree_imports(root)
    from taxoexpan_amd.data_loaders import DeviceBatchLoader
    from taxoexpan_amd.feature_table import FeatureTable
    from taxoexpan_amd.optim import Adam
    from taxoexpan_amd.trainer import train_epoch
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        ds = tet.masked_mag_cs_train(d)
        print(f"dataset: {ds.node_features.shape[0]} nodes, {len(ds)} training queries (built in {time.perf_counter() - t0:.1f} s)", flush=True)
    torch.manual_seed(47)
    model = bench.make_model("pgat", dev)
    opt = Adam(model.parameters(), lr=bench.LR, weight_decay=0, amsgrad=True)
    table = FeatureTable(ds, dev, lr=bench.LR, amsgrad=True)
    loaders = {"d": DeviceBatchLoader(ds, tet.BS, dev, shuffle=True, seed=0, sampler="device"),
               "t": DeviceBatchLoader(ds, tet.BS, dev, shuffle=True, seed=0, sampler="device", feature_table=table)}
    steps = min(args.steps, len(loaders["d"]))

    def leg(name, n):
        kw = dict(feature_table=table) if name == "t" else {}
        t, r = tet.timed(lambda: train_epoch(model, tet._First(loaders[name], n), opt, **kw))
        assert r["first_nonfinite"] == -1, "the model diverged: the timing is void"
        return 1e3 * t / r["n_batches"]

    for name in "dt":
        leg(name, min(30, steps))
    per = {"d": [], "t": []}
    for r in range(args.rounds):
        for name in "dt":
            per[name].append(leg(name, steps))
        print(f"round {r}: (d) {per['d'][-1]:.3f} ms/step | (t) {per['t'][-1]:.3f} ms/step", flush=True)
    print(f"(d) default: {spread(per['d'])} ms/step; (t) table training: {spread(per['t'])} ms/step; (t) - (d) at the medians: "
          f"{float(np.median(per['t'])) - float(np.median(per['d'])):+.3f} ms/step")
    # 3. and 4. one training batch's ids and per-occurrence gradients
    g, x, qf, _label = next(iter(loaders["t"]))
    x, qf, ids_a, ids_b = table.leaves(g, qf, x)
    model.train()
    from taxoexpan_amd.loss import info_nce_loss
    info_nce_loss(model(g, x, qf).reshape(-1, 1 + tet.K), None).backward()
    d_a, d_b = x.grad.contiguous(), qf.rows.grad.contiguous()
    touched = int(torch.unique(torch.cat([ids_a, ids_b])).numel())
    longest = int(torch.bincount(torch.cat([ids_a, ids_b]).long()).max())
    print(f"one batch: {ids_a.numel()} + {ids_b.numel()} occurrences of {touched} of {table.weight.shape[0]} rows (longest segment {longest}), "
          f"d = {table.weight.shape[1]}")
    us = launches_alone(table, ids_a, d_a, ids_b, d_b, args.calls)
    print(f"txe_rowgrad_group + txe_sparse_adam_rows alone: {spread(us)} us over {len(us)} calls")
    for name, v in torch_alternatives(table.weight, ids_a, d_a, ids_b, d_b, args.calls, bench.LR).items():
        print(f"{name}: {spread(v)} us over {len(v)} calls (backward of the two gathers + optimizer step)")
    tab_mb = table.weight.numel() * 4 / 1e6
    print(f"extra device memory: {2 * tab_mb:.1f} MB of moments for a {tab_mb:.1f} MB table (+ {tab_mb:.1f} MB with amsgrad)")


if __name__ == "__main__":
    main()
