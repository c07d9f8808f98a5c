#!/usr/bin/env python3
"""HIP-event time per call, forward plus gradient (`loss_fn(x, label).backward()` on a leaf x), of the three labelled device losses
-- loss.bce_loss, loss.square_exp_loss, loss.margin_rank_loss -- beside the torch expression of the same loss on the same device:

    bce          F.binary_cross_entropy_with_logits(x.squeeze(), 1.0 - label.float(), reduction="sum")          (model/loss.py:28)
    square_exp   (x[label == 1] ** 2).sum() + beta * torch.exp(-1.0 * x[label == 0]).sum()                      (model/loss.py:18)
    margin_rank  (a) clamp_min((x[p] - x[n]) + margin, 0).sum() with the pair indices ALREADY on the device: the expression alone
                 (b) the literal route of model/loss.py:31-50: the labels read back, the group boundaries found on the host, the pairs
                     formed with itertools.product, uploaded again, then the expression -- what one training step pays

Shapes: B = 2,048 x 31 (the SemEval bce shape: 2,048 queries, one positive and 30 negatives each) and 4,096 x 32.  The legs alternate in
one process, `--rounds` windows of `--iters` calls each per leg (the literal route: `--literal-iters`); per leg the minimum and the median
over its windows are printed, in microseconds per call.  The loss values of both sides are compared first.

    python tools/loss_timing.py [--iters 200] [--rounds 5] [--literal-iters 3]"""
import argparse
import itertools
import os
import re
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from taxoexpan_amd import loss as txe_loss  # noqa: E402

SHAPES = ((2048, 31), (4096, 32))


def host_pairs(label):
    """the host route of model/loss.py:32-46 in this project's words: labels on the host, a group ends where a 0 is followed by a 1,
    its positives end where a 1 is followed by a 0, the pairs are the product of both ranges"""
    lab = label.cpu().numpy()                                          # the read-back
    raw, w = lab.tobytes(), lab.itemsize

    def after(first, second):                                          # the indices just behind every [first, second] step (a byte search)
        sep = re.escape(np.array([first, second], dtype=lab.dtype).tobytes())
        return [m.start() // w + 1 for m in re.finditer(sep, raw) if m.start() % w == 0]

    ends = after(0, 1) + [len(lab)]
    middles = after(1, 0)
    starts = [0] + ends[:-1]
    pairs = []
    for a, m, b in zip(starts, middles, ends):
        pairs.extend(itertools.product(range(a, m), range(m, b)))
    return [p for p, _n in pairs], [n for _p, n in pairs]


def torch_bce(x, label):
    return F.binary_cross_entropy_with_logits(x.squeeze(), 1.0 - label.float(), reduction="sum")


def torch_square_exp(x, label, beta=1.0):
    return (x[label == 1] ** 2).sum() + beta * torch.exp(-1.0 * x[label == 0]).sum()


def torch_margin(x, pi, ni, margin=1.0):
    return torch.clamp_min((x[pi, 0] - x[ni, 0]) + margin, 0).sum()


def torch_margin_literal(x, label, margin=1.0):
    pi, ni = host_pairs(label)
    return torch_margin(x, torch.tensor(pi, device=x.device), torch.tensor(ni, device=x.device), margin)


def window(fn, x, iters):
    """microseconds per call of `fn(x).backward()` over one window of `iters` calls between two events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        x.grad = None
        fn(x).backward()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--literal-iters", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "loss_timing.py times the MI355X: no GPU found"
    dev = torch.device("cuda:0")
    for q, k in SHAPES:
        B = q * k
        torch.manual_seed(B)
        x = torch.randn(B, 1, device=dev).requires_grad_(True)
        label = torch.zeros(q, k, dtype=torch.int64, device=dev)
        label[:, 0] = 1
        label = label.reshape(-1)
        pi, ni = (torch.tensor(v, device=dev) for v in host_pairs(label))
        legs = [("bce", "device", lambda t: txe_loss.bce_loss(t, label), args.iters),
                ("bce", "torch", lambda t: torch_bce(t, label), args.iters),
                ("square_exp", "device", lambda t: txe_loss.square_exp_loss(t, label), args.iters),
                ("square_exp", "torch", lambda t: torch_square_exp(t, label), args.iters),
                ("margin_rank", "device", lambda t: txe_loss.margin_rank_loss(t, label), args.iters),
                ("margin_rank", "torch (pairs given)", lambda t: torch_margin(t, pi, ni), args.iters),
                ("margin_rank", "torch (literal host pairs)", lambda t: torch_margin_literal(t, label), args.literal_iters)]
        print(f"B = {q} x {k} = {B} scores, {pi.numel()} margin-rank pairs", flush=True)
        values = {}
        for name, side, fn, _n in legs:                                # first calls, and the values side by side
            x.grad = None
            v = fn(x)
            v.backward()
            values.setdefault(name, []).append((side, float(v.detach()), x.grad.detach().clone()))
        for name, rows in values.items():
            ref = rows[0]
            for side, v, g in rows[1:]:
                print(f"  {name}: device {ref[1]:.4f} | {side} {v:.4f} | max |d_x difference| {float((g - ref[2]).abs().max()):.3e}")
        times = {(name, side): [] for name, side, _f, _n in legs}
        for _ in range(args.rounds):
            for name, side, fn, n in legs:
                times[(name, side)].append(window(fn, x, n))
        for (name, side), t in times.items():
            print(f"  {name:12s} {side:28s} min {min(t):10.1f} us   median {float(np.median(t)):10.1f} us per call (forward + gradient)", flush=True)


if __name__ == "__main__":
    main()
