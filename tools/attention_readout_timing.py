#!/usr/bin/env python3
"""What the attention readout costs at the training batch shape of BASELINE configs[1] (bench.py's batch: 128 queries x 32 = 4,096
synthetic MAG-CS egonets, D = out_dim = 500, A = attention_dim = 100), per call, median of --reps repetitions of --inner calls:

  op       ops.ReadoutAttnFunction (txe_readout_attn_fwd; + txe_readout_attn_bwd and its reduce launch), forward and forward + backward,
           on seeded h [N, D] and Y [N, A] -- the gate's dense product Y = gate_hidden(h) is ops.LinearFunction's and is timed apart
  wmr      ops.ReadoutFunction with position weights (WeightedMeanReadout's kernels) on the same h
  torch    the same expression in torch ops on the same device (tanh, a matrix-vector product, a segment softmax from scatter_reduce /
           index_add, a weighted index_add), autograd's backward
  step     one training step (forward, InfoNCE, backward, Adam) of PGAT + AR + BIM beside PGAT + CR + BIM, the other readout whose
           coefficients cannot be folded into the matcher

    python tools/attention_readout_timing.py [--reps 5] [--inner 20]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from taxoexpan_amd import TaxoExpan, ops, synthetic as syn  # noqa: E402
from taxoexpan_amd.optim import Adam  # noqa: E402

ATTENTION_DIM = 100


def torch_attention(goff, gid, h, Y, pos, P, u):
    s = torch.tanh(Y + P[pos]) @ u.reshape(-1)
    G = goff.numel() - 1
    m = torch.full((G,), -float("inf"), device=h.device).scatter_reduce(0, gid, s, "amax")
    e = torch.exp(s - m[gid])
    alpha = e / torch.zeros(G, device=h.device).index_add(0, gid, e)[gid]
    return torch.zeros((G, h.shape[1]), device=h.device).index_add(0, gid, alpha[:, None] * h)


def timed(fn, reps, inner):
    return round(1e6 * bench.median_time(fn, reps=reps, inner=inner, warm=3), 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "attention_readout_timing.py times the MI355X: no GPU found"
    dev = torch.device("cuda:0")
    tax = syn.make_named_taxonomy("mag_cs", seed=47)
    batches = bench.build_batches(tax, 2, seed0=1, device=dev)
    b = batches[0]
    csr, pos, N, D, A = b["g"].csr(dev), b["pos"], b["n_nodes"], bench.MAG["out_dim"], ATTENTION_DIM
    G = csr.n_graphs
    torch.manual_seed(47)
    h, Y = torch.randn((N, D), device=dev, requires_grad=True), torch.randn((N, A), device=dev, requires_grad=True)
    P, u = torch.randn((3, A), device=dev, requires_grad=True), torch.randn((1, A), device=dev, requires_grad=True)
    W, bias = torch.randn((A, D), device=dev) * D ** -0.5, torch.zeros(A, device=dev)
    pw = torch.randn((3, 1), device=dev, requires_grad=True)
    d_hg = torch.randn((G, D), device=dev)
    goff = csr.graph_off.long()
    gid = torch.repeat_interleave(torch.arange(G, device=dev), goff[1:] - goff[:-1])
    posl = pos.long()
    out = dict(egonets=G, nodes=N, D=D, A=A, h_mb=round(4e-6 * N * D, 1), reps=args.reps, inner=args.inner, us_per_call={})

    def fb(fn):
        def run():
            for t in (h, Y, P, u, pw):
                t.grad = None
            fn().backward(d_hg)
        return run
    attn = lambda: ops.ReadoutAttnFunction.apply(csr, h, Y, pos, P, u)[0]
    wmr = lambda: ops.ReadoutFunction.apply(csr, h, pos, pw)
    tor = lambda: torch_attention(goff, gid, h, Y, posl, P, u)
    us = out["us_per_call"]
    for name, fn in (("attention_readout", attn), ("weighted_mean_readout", wmr), ("torch_ops", tor)):
        with torch.no_grad():
            us[name + "_fwd"] = timed(fn, args.reps, args.inner)
        us[name + "_fwd_bwd"] = timed(fb(fn), args.reps, args.inner)
    with torch.no_grad():
        us["gate_hidden_linear_fwd"] = timed(lambda: ops.LinearFunction.apply(h, None, W, bias, 0), args.reps, args.inner)
        err = (attn() - tor()).abs().max().item()
    out["max_abs_difference_op_vs_torch"] = err
    print(json.dumps(out), flush=True)
    target = torch.zeros(bench.N_QUERIES, dtype=torch.long, device=dev)
    out["step_ms"] = {}
    for readout in ("AR", "CR"):
        torch.manual_seed(47)
        model = TaxoExpan("PGAT", readout, "BIM", **dict(bench.MAG, attention_dim=A)).to(dev).train()
        opt = Adam(model.parameters(), lr=bench.LR, weight_decay=0, amsgrad=True)
        it = iter(range(10 ** 9))
        t = bench.median_time(lambda: bench.train_step(model, opt, batches[next(it) % 2], target, 1), reps=args.reps, inner=args.inner, warm=5)
        bench.assert_finite(model, bench.train_step(model, opt, batches[0], target, 1), "attention_readout_timing")
        out["step_ms"]["PGAT+" + readout + "+BIM"] = round(1e3 * t, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
