#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/losses.npz from the UNMODIFIED reference model/loss.py.

Run on a machine that has the reference tree (never on the GPU machine, never by a test):

    python tools/gen_loss_golden.py --reference /path/to/the/reference

The reference's loss.py is loaded from its file as it is.  One shim, of the same kind as oracle/dgl_shim: the installed torch's
F.margin_ranking_loss refuses the reference's `[n, 1], [n, 1], [n]` arguments ("All input tensors should have same dimension"), so the
loaded module's `F` is replaced by a thin object that forwards every attribute to torch.nn.functional except `margin_ranking_loss`,
which flattens its two inputs first (what older torch versions did by broadcasting against y [n] is NOT what the reference means: it
pairs row i with row i).  A second forwarder serves the float64 run alone: the reference's bce_loss builds its target with
`target.float()`, and the installed torch's binary_cross_entropy_with_logits computes and returns in the TARGET's dtype, so a float64
input would still be evaluated in float32; `binary_cross_entropy_with_logits` therefore converts the target (exactly 0.0 or 1.0) to the
input's dtype first -- a no-op in the float32 run.  Nothing else of the module is touched; no reference source is copied: the file holds arrays only.

For a fixed-seed set of (x, label) cases the file holds, for each of bce_loss, square_exp_loss and margin_rank_loss, the reference's loss
and autograd gradient in float32 and in float64 (`<case>__<fn>_loss32`, `_grad32`, `_loss64`, `_grad64`, and `_ok` = 0 where the
reference raises: its bce_loss at B == 1), beside the inputs (`<case>__x` fp32, `__label` int32 or int64, `__beta`, `__margin`) and the
list of case names (`cases`).  Cases: label vectors inside the reference's domain (every group 1-3 ones followed by 1-5 zeros) of 1
(`[1]`), 63, 64, 65 and 1,025 entries, one group of 3 ones + 200 zeros, both label widths, beta 0.5 / margin 0.7 beside the defaults,
and the two vectors of the documented margin-rank deviation (`[0, 1, 0]`, `[0, 0, 1, 0]`: the reference returns 0 there)."""
import argparse
import importlib.util
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "losses.npz")
FUNCTIONS = ("bce_loss", "square_exp_loss", "margin_rank_loss")


class _Functional:
    """torch.nn.functional, except that margin_ranking_loss flattens its two inputs (see the module docstring)"""

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)

    @staticmethod
    def margin_ranking_loss(input1, input2, target, **kw):
        return torch.nn.functional.margin_ranking_loss(input1.reshape(-1), input2.reshape(-1), target, **kw)

    @staticmethod
    def binary_cross_entropy_with_logits(input, target, **kw):
        return torch.nn.functional.binary_cross_entropy_with_logits(input, target.to(input.dtype), **kw)


def load_reference(root):
    spec = importlib.util.spec_from_file_location("reference_model_loss", os.path.join(root, "model", "loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.F = _Functional()
    return mod


def domain_labels(rng, B):
    """B labels, every group 1-3 ones followed by 1-5 zeros ([1] for B == 1)"""
    if B == 1:
        return [1]
    out, left = [], B
    while left:
        p, n = int(rng.randint(1, 4)), int(rng.randint(1, 6))
        if left <= 8:                                   # the last group takes what is left (2 <= left <= 8)
            p = min(p, left - 1)
            if left - p > 5:
                p = left - 5
            n = left - p
        elif left - (p + n) == 1:                       # never leave a single entry behind
            n = n + 1 if n < 5 else n - 1
        out += [1] * p + [0] * n
        left -= p + n
    assert len(out) == B
    return out


def cases():
    rng = np.random.RandomState(20240607)
    out = []

    def add(name, label, width, beta=1.0, margin=1.0):
        label = np.asarray(label, dtype=np.int32 if width == 32 else np.int64)
        x = (rng.randn(label.shape[0]) * 2.0).astype(np.float32)
        out.append((name, x, label, beta, margin))

    add("b1", [1], 64)
    add("b63", domain_labels(rng, 63), 32)
    add("b64", domain_labels(rng, 64), 64)
    add("b65", domain_labels(rng, 65), 32)
    add("b65_params", domain_labels(rng, 65), 64, beta=0.5, margin=0.7)
    add("b1025", domain_labels(rng, 1025), 64)
    add("b1025_i32_params", domain_labels(rng, 1025), 32, beta=0.5, margin=0.7)
    add("g3x200", [1] * 3 + [0] * 200, 64)
    add("g3x200_i32_params", [1] * 3 + [0] * 200, 32, beta=0.5, margin=0.7)
    add("dev_010", [0, 1, 0], 64)
    add("dev_0010", [0, 0, 1, 0], 32)
    return out


def run(ref, fn, x, label, dtype, beta, margin):
    out = torch.from_numpy(x).to(dtype).reshape(-1, 1).requires_grad_(True)
    tgt = torch.from_numpy(label)
    kw = {"margin": margin} if fn == "margin_rank_loss" else {"beta": beta}
    loss = getattr(ref, fn)(out, tgt, **kw)
    assert loss.dtype == dtype, (fn, loss.dtype)
    grad = torch.zeros_like(out)
    if loss.requires_grad:
        (g,) = torch.autograd.grad(loss, out, allow_unused=True)
        if g is not None:
            grad = g
    return loss.detach().numpy().reshape(()), grad.reshape(-1).numpy()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="root of the reference tree (the directory that holds model/loss.py)")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    ref = load_reference(args.reference)
    data = {}
    names = []
    for name, x, label, beta, margin in cases():
        names.append(name)
        data[f"{name}__x"], data[f"{name}__label"] = x, label
        data[f"{name}__beta"], data[f"{name}__margin"] = np.float64(beta), np.float64(margin)
        for fn in FUNCTIONS:
            ok = 1
            for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
                try:
                    loss, grad = run(ref, fn, x, label, dtype, beta, margin)
                except (ValueError, RuntimeError, IndexError) as e:
                    print(f"{name}: the reference's {fn} raises ({type(e).__name__}: {str(e)[:80]})")
                    ok = 0
                    loss = np.asarray(np.nan, dtype=np.float32 if tag == "32" else np.float64)
                    grad = np.full(x.shape[0], np.nan, dtype=loss.dtype)
                data[f"{name}__{fn}_loss{tag}"], data[f"{name}__{fn}_grad{tag}"] = loss, grad
            data[f"{name}__{fn}_ok"] = np.int32(ok)
        print(name, len(x), label.dtype, *(f"{fn}={float(data[f'{name}__{fn}_loss64']):.6f}" for fn in FUNCTIONS))
    data["cases"] = np.asarray(names)
    np.savez_compressed(args.out, **data)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, {len(names)} cases")


if __name__ == "__main__":
    main()
