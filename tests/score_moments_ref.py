"""Independent reference of the scoring loop's moments mode (txe_*_score_moments_block, txe_moments_merge, scoring.score_moments_fused):
plain numpy, float64.  Written from the definitions in include/txe.h, not from the kernels or from scoring.host_score_moments (which
tests/test_score_moments_cpu.py holds to it).  The sibling of log_partition_ref.py.

    z = S (larger is better) or -S;   t = fl32(beta * z), ONE fp32 product (beta fp32);   p = softmax(t) over the row
    lse = log sum exp t,   mean = sum p t,   var = sum p (t - mean)^2,   entropy = -sum p log p            (direct formulas, row_moments)
    a NaN in the row -> lse NaN; otherwise a +Inf -> +Inf; otherwise nothing above -Inf (an empty row too) -> -Inf; wherever lse is not
    finite the other three are NaN.  A t = -Inf has p = 0 and adds nothing anywhere.

tile_quads / merge_quads restate the centred quadruples (m, s0, s1, s2) of a part of a row and their merge, as the header gives them.
"""
import math

import numpy as np

NAN3 = (math.nan, math.nan, math.nan)


def scaled(S, beta, larger_is_better=True):
    """t [Q, G] as float64 values of the fp32 product fl32(beta * z)"""
    z = np.asarray(S, dtype=np.float32)
    z = z if larger_is_better else -z
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.float32(beta) * z).astype(np.float32).astype(np.float64)


def _row(t):
    """one row of scaled scores, a float64 vector -> (lse, mean, var, entropy)"""
    if t.size == 0:
        return (-math.inf,) + NAN3
    if np.isnan(t).any():
        return (math.nan,) + NAN3
    if (t == math.inf).any():
        return (math.inf,) + NAN3
    M = float(t.max())
    if M == -math.inf:
        return (-math.inf,) + NAN3
    live = t[t > -math.inf]
    e = np.exp(live - M)
    total = math.fsum(e.tolist())
    lse = M + math.log(total)
    p = e / total                                          # (normalised by the sum itself: exp(t - lse) loses log(total) beside a huge |t|)
    logp = (live - M) - math.log(total)
    mean = math.fsum((p * live).tolist())
    var = math.fsum((p * (live - mean) ** 2).tolist())
    ent = -math.fsum((p * logp).tolist())
    return lse, mean, var, max(ent, 0.0)


def row_moments(S, beta=1.0, larger_is_better=True):
    """float64 [Q, 4] = (lse, mean, var, entropy) from a score array [Q, G]"""
    t = scaled(S, beta, larger_is_better)
    return np.array([_row(t[q]) for q in range(t.shape[0])], dtype=np.float64).reshape(t.shape[0], 4)


def tile_quads(S, beta=1.0, larger_is_better=True, tile=128):
    """the quadruples (max t, sum e, sum d e, sum d^2 e; d = t - max, e = exp(d)) of every row over column tiles of `tile`, float64
    [Q, tiles] each, in the convention of the scratch: an empty or all -Inf part is (-Inf, 0, 0, 0); a part with a NaN has max NaN, one
    with +Inf has max +Inf (its sums are not read)"""
    t = scaled(S, beta, larger_is_better)
    Q, G = t.shape
    nt = (G + tile - 1) // tile
    pm = np.full((Q, nt), -np.inf)
    p0, p1, p2 = np.zeros((Q, nt)), np.zeros((Q, nt)), np.zeros((Q, nt))
    for q in range(Q):
        for k in range(nt):
            part = t[q, k * tile:(k + 1) * tile]
            if np.isnan(part).any():
                pm[q, k] = np.nan
            elif part.size and part.max() == np.inf:
                pm[q, k] = np.inf
            elif part.size and part.max() > -np.inf:
                m = part.max()
                d = part[part > -np.inf] - m
                e = np.exp(d)
                pm[q, k] = m
                p0[q, k], p1[q, k], p2[q, k] = math.fsum(e.tolist()), math.fsum((d * e).tolist()), math.fsum((d * d * e).tolist())
    return pm, p0, p1, p2


def merge_quads(part_max, part_s0, part_s1, part_s2):
    """expected (lse, mean, var, entropy) [Q, 4] (float64) of rows given as `cnt` quadruples each ([Q, cnt]; cnt may be 0):
    M = max m, delta = m - M, w = exp(delta); S0 = sum w s0, S1 = sum w (s1 + delta s0), S2 = sum w (s2 + 2 delta s1 + delta^2 s0);
    lse = M + log S0, mean = M + S1 / S0, var = max(S2 / S0 - (S1 / S0)^2, 0), entropy = max(log S0 - S1 / S0, 0).
    The formulas as they stand: the device's merge also drops a part more than 104 below M from S1 and S2 (include/txe.h), which this
    does not restate -- such a part's terms are below e^-104 ~ 1e-46 of the sums, far under any tolerance used against this function;
    only an exact "entropy == 0" differs, and that is asserted on the device's output, not on this one's."""
    pm, p0, p1, p2 = (np.asarray(a, dtype=np.float64) for a in (part_max, part_s0, part_s1, part_s2))
    out = np.full((pm.shape[0], 4), np.nan, dtype=np.float64)
    for q in range(pm.shape[0]):
        m = pm[q]
        if np.isnan(m).any():
            continue
        if (m == np.inf).any():
            out[q, 0] = np.inf
        elif m.size == 0 or m.max() == -np.inf:
            out[q, 0] = -np.inf
        else:
            M = float(m.max())
            live = m > -np.inf
            delta = m[live] - M
            w = np.exp(delta)
            s0, s1, s2 = p0[q][live], p1[q][live], p2[q][live]
            S0 = math.fsum((w * s0).tolist())
            S1 = math.fsum((w * (s1 + delta * s0)).tolist())
            S2 = math.fsum((w * (s2 + 2.0 * delta * s1 + delta * delta * s0)).tolist())
            r1 = S1 / S0
            out[q] = (M + math.log(S0), M + r1, max(S2 / S0 - r1 * r1, 0.0), max(math.log(S0) - r1, 0.0))
    return out


def nll(lse, t_pos, pos_off):
    """mean over queries of the mean over the query's positives j of lse[q] - t_j (float64)"""
    lse, t_pos, off = np.asarray(lse, dtype=np.float64), np.asarray(t_pos, dtype=np.float64), np.asarray(pos_off, dtype=np.int64)
    return float(np.mean([np.mean(lse[q] - t_pos[off[q]:off[q + 1]]) for q in range(len(off) - 1)]))


def ece(confidence, correct, bins=10):
    """expected calibration error over equal-width bins of the confidence (1.0 in the last): sum of share x |accuracy - mean confidence|"""
    p, c = np.asarray(confidence, dtype=np.float64), np.asarray(correct, dtype=np.float64)
    total = 0.0
    for k in range(bins):
        lo, hi = k / bins, (k + 1) / bins
        sel = (p >= lo) & ((p < hi) if k < bins - 1 else (p <= 1.0))
        if sel.any():
            total += sel.mean() * abs(c[sel].mean() - p[sel].mean())
    return total


def planted(Q, G, scale, bump, seed=0):
    """the fit's planted scores: N(0, 1) noise, the positive + bump, times a scale -> (S fp32 [Q, G], pos_off [Q + 1], pos_idx [Q])"""
    rng = np.random.default_rng(seed)
    S = rng.normal(size=(Q, G))
    pos = rng.integers(0, G, size=Q)
    S[np.arange(Q), pos] += bump
    return (S * scale).astype(np.float32), np.arange(Q + 1, dtype=np.int64), pos.astype(np.int64)


# (the recipes and their outcomes are the issue's; its figures for the first -- beta 0.587, NLL 2.420 -> 2.030 -- are seed 0's draw and
#  are asserted; the other draws behind its figures are not known: seed 0 gives beta 18.53 and 0.1594 where it lists 14.02 and 0.163)
#          (Q, G, scale, bump)  -> outcome
RECIPES = [((96, 300, 5, 3), "interior"), ((64, 129, 0.2, 3), "interior"), ((40, 1000, 12, 2), "interior"),
           ((33, 257, 1, 50), "upper"), ((33, 257, 1, -1), "lower")]
