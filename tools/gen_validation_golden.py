#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY (CPU, never on the GPU machine): write tests/golden/obtain_ranks.npz from the UNMODIFIED reference's
model/metric.py, imported at run time from the reference checkout given with --reference (as oracle/gen_golden.py does).

About 30 seeded labelled score vectors in the validation-batch layout (per query: its positives, label 1, then its negatives, label 0):
multi-group batches with 1-6 positives and 1-300 negatives per group, ties (scores rounded to a few values), NaN and +-Inf, a leading
all-negative group, B = 2, mode 0 and mode 1, int32 and int64 labels.  Every group with a positive has a negative (a group without one is
outside the reference's domain).  Recorded per case c: c:score fp32 [B], c:label [B], c:mode, the reference's per-group ranks flattened
(c:ranks int32) with their offsets (c:pos_off), and c:metrics fp64 [7] = macro_mr, micro_mr, hit_at_1, hit_at_3, hit_at_5,
mrr_scaled_10, combined_metrics of the reference on those ranks.

    python tools/gen_validation_golden.py --reference PATH_TO_REFERENCE_CHECKOUT
"""
import argparse
import importlib.util
import os
import warnings

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "obtain_ranks.npz")
METRICS = ("macro_mr", "micro_mr", "hit_at_1", "hit_at_3", "hit_at_5", "mrr_scaled_10", "combined_metrics")


def _reference_metric(ref):
    spec = importlib.util.spec_from_file_location("ref_metric", os.path.join(ref, "model", "metric.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _case(rng, n_groups, max_pos=6, max_neg=300, ties=0, nonfinite=0.0, lead_negatives=0, dtype=np.int64):
    labels, scores = [], []
    if lead_negatives:
        labels.append(np.zeros(lead_negatives, dtype=dtype))
    for _ in range(n_groups):
        p, n = rng.randint(1, max_pos + 1), rng.randint(1, max_neg + 1)
        labels += [np.ones(p, dtype=dtype), np.zeros(n, dtype=dtype)]
    label = np.concatenate(labels)
    score = rng.randn(len(label)).astype(np.float32)
    if ties:
        score = np.round(score * ties).astype(np.float32) / np.float32(ties)
    if nonfinite:
        m = rng.rand(len(label))
        score[m < nonfinite / 3] = np.nan
        score[(m >= nonfinite / 3) & (m < 2 * nonfinite / 3)] = np.inf
        score[(m >= 2 * nonfinite / 3) & (m < nonfinite)] = -np.inf
    return score, label


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout (holds model/metric.py)")
    args = ap.parse_args()
    ref = _reference_metric(args.reference)
    rng = np.random.RandomState(20261016)
    cases = []
    for i in range(8):                                   # plain multi-group batches
        cases.append(_case(rng, rng.randint(2, 12), dtype=np.int64 if i % 2 else np.int32) + (i % 2,))
    for i in range(6):                                   # ties
        cases.append(_case(rng, rng.randint(2, 10), ties=(1, 2, 4)[i % 3], dtype=np.int32 if i % 2 else np.int64) + (i % 2,))
    for i in range(6):                                   # NaN and +-Inf (with ties in half of them)
        cases.append(_case(rng, rng.randint(2, 10), ties=2 * (i % 2), nonfinite=(0.05, 0.2, 0.5)[i % 3],
                           dtype=np.int64 if i % 2 else np.int32) + ((i // 2) % 2,))
    for i in range(4):                                   # a leading all-negative group
        cases.append(_case(rng, rng.randint(1, 6), lead_negatives=rng.randint(1, 40), dtype=np.int32 if i % 2 else np.int64) + (i % 2,))
    for mode in (0, 1):                                  # B = 2
        for dt in (np.int32, np.int64):
            cases.append((np.array([0.5, -0.25], dtype=np.float32) * (1 if dt is np.int32 else -1), np.array([1, 0], dtype=dt), mode))
    for i in range(2):                                   # one positive per group, short groups
        cases.append(_case(rng, 40, max_pos=1, max_neg=3, ties=2, dtype=np.int64) + (i,))
    save = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                  # the reference's mean of an empty group (NaN) and its deprecated tostring
        for c, (score, label, mode) in enumerate(cases):
            all_ranks = ref.obtain_ranks(torch.from_numpy(score)[:, None], torch.from_numpy(label), mode=mode)
            flat = [int(r) for rs in all_ranks for r in rs]
            off = np.concatenate([[0], np.cumsum([len(rs) for rs in all_ranks])]).astype(np.int32)
            save[f"{c}:score"], save[f"{c}:label"], save[f"{c}:mode"] = score, label, np.int64(mode)
            save[f"{c}:ranks"], save[f"{c}:pos_off"] = np.asarray(flat, dtype=np.int32), off
            save[f"{c}:metrics"] = np.asarray([float(getattr(ref, m)(all_ranks)) for m in METRICS], dtype=np.float64)
    save["n_cases"] = np.int64(len(cases))
    np.savez_compressed(OUT, **save)
    print(f"{OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
