#!/usr/bin/env python3
"""The MLP matcher's all-candidate scoring loop (txe_mlp_*) on the MAG shapes, one MI355X: store, fused rank and fused top-5 in pairs/s,
the fraction of the VALU roof (two-op form: one max + one FMA per pair and hidden unit), and the literal per-query loop
(evaluate._score_blocks: model.match(hg, q.expand(G, -1)) per query) timed on a few queries and extrapolated.  One JSON line per shape.
    python tools/mlp_score_bench.py [--shapes cs,full]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import median_time  # noqa: E402
from taxoexpan_amd.model_zoo import MLP  # noqa: E402
from taxoexpan_amd.scoring import rank_all_fused, score_all, topk_parents_fused  # noqa: E402

SHAPES = {"cs": (24736, 2459, 64), "full": (356000, 8192, 2)}     # candidates, queries, queries of the literal loop
L, R, H = 500, 250, 500
# spec VALU rate: 256 CUs x 4 SIMDs x 32 lanes/clk x 2.4 GHz element-ops/s; the two-op form spends two per (pair, h)
ROOF_PAIR_H = 256 * 4 * 32 * 2.4e9 / 2


def shader_clock_mhz():
    """the current shader clock as the driver reports it (read only), or None"""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
    except Exception:
        return None
    for ln in out.splitlines():
        if "sclk" in ln and "Mhz" in ln:
            try:
                return float(ln.split("(")[1].split("Mhz")[0])
            except (IndexError, ValueError):
                pass
    return None


def run(name, G, Q, n_lit):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = MLP(L, R, H).to(dev).eval()
    gen = torch.Generator().manual_seed(1)
    hg = (torch.randn(G, L, generator=gen) * 0.3).to(dev)
    q = torch.nn.functional.normalize(torch.randn(Q, R, generator=gen), dim=1).to(dev)
    rs = np.random.RandomState(2)
    npos = 1 + rs.randint(0, 3, size=Q)
    pos_off = np.concatenate([[0], np.cumsum(npos)]).astype(np.int64)
    pos_idx = np.concatenate([rs.choice(G, size=k, replace=False) for k in npos]).astype(np.int64)
    pairs = float(G) * Q
    hp = (H + 15) // 16 * 16
    res = dict(shape=name, G=G, Q=Q, l=L, r=R, H=H)
    with torch.no_grad():
        S = score_all(m, hg, q)
        t_store = median_time(lambda: score_all(m, hg, q, out=S), reps=3)
        del S
        torch.cuda.empty_cache()
        t_rank = median_time(lambda: rank_all_fused(m, hg, q, pos_off, pos_idx), reps=3)
        clk = shader_clock_mhz()
        t_top = median_time(lambda: topk_parents_fused(m, hg, q, None, 5, True), reps=3)
        qs = q[:n_lit]
        t_lit = median_time(lambda: [m(hg, v.expand(G, -1)) for v in qs], reps=1) / n_lit * Q
    for key, t in (("store", t_store), ("rank", t_rank), ("top5", t_top)):
        res[f"{key}_s"] = t
        res[f"{key}_pairs_per_s"] = pairs / t
        res[f"{key}_roof_fraction"] = pairs * hp / t / ROOF_PAIR_H
    res["literal_loop_s_extrapolated"] = t_lit
    res["literal_over_fused_rank"] = t_lit / t_rank
    res["shader_clock_mhz"] = clk
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cs,full")
    args = ap.parse_args()
    for s in args.shapes.split(","):
        run(s, *SHAPES[s])
