"""Independent reference of the scoring loop's log-partition (txe_*_score_lse_block, txe_lse_merge, scoring.log_partition_fused): plain
numpy, float64.  Written from the definition in include/txe.h, not from the kernels or from scoring.host_log_partition (which
tests/test_log_partition_cpu.py holds to it).

    z = S (larger is better) or -S;   lse[q] = log sum_g exp(z[q][g])   as the IEEE value of the float64 formula on the given scores:
    a NaN in the row -> NaN; otherwise a +Inf -> +Inf; otherwise nothing above -Inf (an empty row too) -> -Inf; otherwise
    M + log(sum exp(z - M)), M = max z.
"""
import math

import numpy as np


def _lse_of(z):
    """one row, a float64 vector"""
    if z.size == 0:
        return -math.inf
    if np.isnan(z).any():
        return math.nan
    if (z == math.inf).any():
        return math.inf
    M = float(z.max())
    if M == -math.inf:
        return -math.inf
    return M + math.log(math.fsum(np.exp(z - M).tolist()))


def row_lse(S, larger_is_better=True):
    """float64 [Q] from a score array [Q, G] of any float dtype (taken to float64 exactly)"""
    z = np.asarray(S, dtype=np.float64)
    z = z if larger_is_better else -z
    return np.array([_lse_of(z[q]) for q in range(z.shape[0])], dtype=np.float64)


def tile_pairs(S, larger_is_better=True, tile=128):
    """the (max, sum exp(z - max)) pairs of every row over column tiles of `tile`, float64 [Q, tiles] each, in the convention of the
    scratch: an empty or all -Inf part is (-Inf, 0); a part with a NaN has max NaN, one with +Inf has max +Inf (its sum is not read)"""
    z = np.asarray(S, dtype=np.float64)
    z = z if larger_is_better else -z
    Q, G = z.shape
    nt = (G + tile - 1) // tile
    pm, ps = np.full((Q, nt), -np.inf), np.zeros((Q, nt))
    for q in range(Q):
        for t in range(nt):
            part = z[q, t * tile:(t + 1) * tile]
            if np.isnan(part).any():
                pm[q, t] = np.nan
            elif part.size and part.max() == np.inf:
                pm[q, t] = np.inf
            elif part.size and part.max() > -np.inf:
                pm[q, t] = part.max()
                ps[q, t] = math.fsum(np.exp(part - part.max()).tolist())
    return pm, ps


def merge_pairs(part_max, part_sum):
    """expected lse [Q] (float64) of rows given as `cnt` (max, sum) pairs each ([Q, cnt]; cnt may be 0)"""
    pm, ps = np.asarray(part_max, dtype=np.float64), np.asarray(part_sum, dtype=np.float64)
    out = np.empty(pm.shape[0], dtype=np.float64)
    for q in range(pm.shape[0]):
        m, s = pm[q], ps[q]
        if np.isnan(m).any():
            out[q] = np.nan
        elif (m == np.inf).any():
            out[q] = np.inf
        elif m.size == 0 or m.max() == -np.inf:
            out[q] = -np.inf
        else:
            M = float(m.max())
            live = m > -np.inf
            out[q] = M + math.log(math.fsum((s[live] * np.exp(m[live] - M)).tolist()))
    return out


def nll(lse, z_pos, pos_off):
    """mean over queries of the mean over the query's positives j of lse[q] - z_j (float64)"""
    lse, z_pos, off = np.asarray(lse, dtype=np.float64), np.asarray(z_pos, dtype=np.float64), np.asarray(pos_off, dtype=np.int64)
    per = [np.mean(lse[q] - z_pos[off[q]:off[q + 1]]) for q in range(len(off) - 1)]
    return float(np.mean(per))
