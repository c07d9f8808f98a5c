"""Calibrated probabilities: one scalar, a temperature T, fitted on the validation split by minimising the exact NLL.

The model is trained on a 32-way softmax (loss.py:52-57: 1 positive + 31 sampled negatives) and then normalised over every candidate,
and the matcher's output scale is arbitrary (LBM emits exp(b)), so p(a | q) = exp(z(q, a) - lse[q]) cannot be thresholded as it stands.
With t = beta z, beta = 1 / T, the objective is evaluate's own NLL at beta,

    f(beta)   = mean over queries of the mean over the query's positives j of (lse_beta[q] - beta z_j)
    f'(beta)  = mean_q (mean_beta[q] / beta - mean_j z_j)
    f''(beta) = mean_q var_beta[q] / beta^2  >= 0                                  (convex in beta)

with beta z_j taken as the kernels take every candidate's: t_j = fl32(beta z_j), one fp32 product -- so that a true parent's term is the
very t its own column contributed to lse_beta (a probability exp(t_j - lse_beta) never exceeds 1, and f' is exactly 0 on a row whose
true parent leads by more than fp32's exp can see) --

where lse_beta, mean_beta = E_p[t] and var_beta = Var_p[t] are the moments of the all-candidate loop (scoring.score_moments_fused: one
pass over the candidates per evaluation, no score matrix).  The fit is a bracketed Newton iteration on beta; every iteration is one
moments pass and one read-back of three float64 scalars.
"""
import collections
import math
import types

import numpy as np
import torch

from . import ops, scoring

ECE_BINS = 10


class Calibration(collections.namedtuple("Calibration", "temperature beta nll_before nll_after iterations at_bound history")):
    """the result of a temperature fit: temperature = 1 / beta (beta: the fp32 scale the kernels multiply by, as a Python float),
    nll_before = f(1), nll_after = f(beta), iterations = the steps taken (0 at a bound), at_bound = the minimiser lies outside `bounds`
    and the bound is returned, history = [(beta, f, f', f'')] of every evaluation in order"""
    __slots__ = ()

    def state_dict(self):
        d = self._asdict()
        d["history"] = [list(map(float, h)) for h in self.history]
        return d

    @classmethod
    def from_state_dict(cls, d):
        return cls(float(d["temperature"]), float(d["beta"]), float(d["nll_before"]), float(d["nll_after"]), int(d["iterations"]),
                   bool(d["at_bound"]), [tuple(map(float, h)) for h in d["history"]])


def _fit_args(bounds, rtol, max_iter):
    try:
        lo, hi = (ops._check_beta(b, "fit_temperature: a bound on beta") for b in bounds)
    except TypeError:
        raise ValueError(f"fit_temperature: bounds = (lo, hi) on beta, got {bounds!r}") from None
    if not lo < hi:
        raise ValueError(f"fit_temperature: bounds must rise, got {bounds!r}")
    if isinstance(rtol, bool) or not (math.isfinite(float(rtol)) and float(rtol) > 0.0):
        raise ValueError(f"fit_temperature: rtol must be finite and > 0, got {rtol!r}")
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or int(max_iter) < 1:
        raise ValueError(f"fit_temperature: max_iter must be an integer >= 1, got {max_iter!r}")
    return lo, hi, float(rtol), int(max_iter)


def _newton_bracket(evaluate_at, lo, hi, rtol, max_iter):
    """the deterministic search both fits share.  evaluate_at(beta) -> (f, f', f'') at an fp32-representable beta; the bounds are on
    beta.  f'(lo) >= 0: lo; f'(hi) <= 0: hi (at_bound, no iteration).  Otherwise from beta = 1 (sqrt(lo hi) if 1 is not inside) with
    the bracket f'(lo) < 0 < f'(hi): the Newton step beta - f' / f'', or sqrt(lo hi) when that is not strictly inside the bracket or
    f'' is not positive and finite; stop when the step is below rtol * beta, or at max_iter.
    One addition to that search: f is evaluated on fp32-rounded t, so it is convex only up to ~1e-8 of noise; should the last iterate's
    f lie above f(1) -- possible only when 1 is the minimiser to within the last step -- beta = 1 is returned with f(1) (iterations and
    history still describe the search), so that nll_after <= nll_before holds for every caller."""
    history = []

    def ev(b):
        v = tuple(float(x) for x in evaluate_at(b))
        history.append((b,) + v)
        return v
    f1 = ev(1.0)
    nll_before = f1[0]
    at_lo = f1 if lo == 1.0 else ev(lo)
    if at_lo[1] >= 0.0:
        return Calibration(1.0 / lo, lo, nll_before, at_lo[0], 0, True, history)
    at_hi = f1 if hi == 1.0 else ev(hi)
    if at_hi[1] <= 0.0:
        return Calibration(1.0 / hi, hi, nll_before, at_hi[0], 0, True, history)
    if lo < 1.0 < hi:
        beta, cur = 1.0, f1
    else:
        beta = ops._check_beta(math.sqrt(lo * hi))
        cur = ev(beta)
    iterations = 0
    while iterations < max_iter:
        f, g, h = cur
        if g == 0.0:
            break
        if g < 0.0:
            lo = beta
        else:
            hi = beta
        new = beta - g / h if (math.isfinite(h) and h > 0.0) else float("nan")
        if not (lo < new < hi):
            new = math.sqrt(lo * hi)
        new = ops._check_beta(new)
        if not (lo < new < hi):                       # (the bracket has closed to neighbouring fp32 values)
            break
        step, beta = abs(new - beta), new
        cur = ev(beta)
        iterations += 1
        if step < rtol * beta:
            break
    if cur[0] > nll_before:                           # (the docstring's addition: rounding noise around a minimiser at 1)
        beta, cur = 1.0, f1
    return Calibration(1.0 / beta, beta, nll_before, cur[0], iterations, False, history)


def _host_positive_means(S, pos_off, pos_idx, larger_is_better, beta=1.0):
    """float64 [Q]: the mean over each query's positives j of t_j = fl32(beta z_j), z_j = S[q, pos_idx[j]] (or its negative)"""
    off = np.asarray(pos_off, dtype=np.int64)
    idx = np.asarray(pos_idx, dtype=np.int64)
    n = np.diff(off)
    if off.shape[0] != S.shape[0] + 1 or off[0] != 0 or off[-1] != idx.shape[0] or np.any(n < 1):
        raise ValueError("fit_temperature: pos_off [Q + 1] must rise from 0 to len(pos_idx) with at least one true parent per query")
    qid = np.repeat(np.arange(len(n)), n)
    z = S[qid, idx] if larger_is_better else -S[qid, idx]
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.float32(beta) * z).astype(np.float32).astype(np.float64)
        return np.bincount(qid, weights=t, minlength=len(n)) / n


def _raise_first_bad(per_query):
    bad = np.flatnonzero(~np.isfinite(per_query))
    if bad.size:
        raise ValueError(f"fit_temperature: the NLL at temperature 1 is not finite -- first at query {int(bad[0])} "
                         f"(its term is {per_query[bad[0]]!r}: a non-finite score in its row or of one of its true parents)")


def host_nll(S, pos_off, pos_idx, beta=1.0, larger_is_better=True):
    """f(beta) and its first two derivatives on a numpy score array S [Q, G] (the device fit's restatement): (f, f', f'') as floats"""
    beta = ops._check_beta(beta)
    S = np.asarray(S, dtype=np.float32)
    tbar = _host_positive_means(S, pos_off, pos_idx, larger_is_better, beta)
    m = scoring.host_score_moments(S, 1.0 / beta, larger_is_better)
    return (float(np.mean(m.lse - tbar)), float(np.mean(m.mean - tbar) / beta), float(np.mean(m.var) / (beta * beta)))


def host_fit_temperature(S, pos_off, pos_idx, larger_is_better=True, bounds=(1e-3, 1e3), rtol=1e-4, max_iter=30):
    """fit_temperature_scores on a numpy score array S [Q, G] (pos_off [Q + 1] / pos_idx: each query's true columns): the same algorithm
    with scoring.host_score_moments in place of the device pass.  Returns a Calibration."""
    lo, hi, rtol, max_iter = _fit_args(bounds, rtol, max_iter)
    S = np.asarray(S, dtype=np.float32)
    _host_positive_means(S, pos_off, pos_idx, larger_is_better)         # (the argument rules, before anything is evaluated)

    def evaluate_at(beta):
        # (1 / beta in float64 comes back to the very fp32 beta: host_score_moments scales by fl32(1 / temperature))
        m = scoring.host_score_moments(S, 1.0 / beta, larger_is_better)
        tbar = _host_positive_means(S, pos_off, pos_idx, larger_is_better, beta)
        if beta == 1.0:
            _raise_first_bad(m.lse - tbar)
        return np.mean(m.lse - tbar), np.mean(m.mean - tbar) / beta, np.mean(m.var) / (beta * beta)
    return _newton_bracket(evaluate_at, lo, hi, rtol, max_iter)


def _device_positive_scores(pm, Qp, pos_off, pos_idx, block):
    """fp32 [n_positives]: the true parents' scores through the prepared matcher's own staircase (rank_all_fused's thresholds)"""
    dev = Qp.device
    off_h = np.asarray(pos_off, dtype=np.int64)
    idx = torch.as_tensor(np.asarray(pos_idx, dtype=np.int64)).to(dev)
    thr = torch.empty(int(idx.numel()), dtype=torch.float32, device=dev)
    for q0 in range(0, Qp.shape[0], block):
        q1 = min(q0 + block, Qp.shape[0])
        lo, hi = int(off_h[q0]), int(off_h[q1])
        if hi > lo:
            off = torch.as_tensor(off_h[q0:q1 + 1] - lo, dtype=torch.int32).to(dev)
            pm.positives(Qp[q0:q1], off, idx[lo:hi], thr[lo:hi])
    return thr


def fit_temperature_scores(match, hg, qf, pos_off, pos_idx, larger_is_better=True, bounds=(1e-3, 1e3), rtol=1e-4, max_iter=30, block=None):
    """The temperature that minimises the exact NLL of the true parents (pos_off [Q + 1] / pos_idx: candidate rows, evaluate's layout)
    of the queries qf [Q, r] against ALL candidates hg [G, l], already encoded.  The matcher is prepared once and the positives' fp32
    scores are taken once (the staircase the ranks' thresholds come from); every iteration is one moments pass over the candidates
    (scoring.score_moments_fused's kernels) + one read-back of (f, f', f'') as three float64 scalars.  bounds: on beta = 1 / T.
    A non-finite f(1) raises ValueError naming the first offending query.  Returns a Calibration.  Deterministic."""
    lo, hi, rtol, max_iter = _fit_args(bounds, rtol, max_iter)
    Q, G = int(qf.shape[0]), int(hg.shape[0])
    off_h = np.asarray(pos_off, dtype=np.int64)
    if Q == 0 or G == 0 or off_h[-1] == 0:
        raise ValueError("fit_temperature: nothing to fit -- no query, no candidate or no true parent")
    if np.any(np.diff(off_h) < 1):
        raise ValueError("fit_temperature: every query needs at least one true parent among the candidates")
    dev = hg.device
    if block is None:
        block = scoring._default_block(Q)
    with torch.no_grad():
        if scoring.fused_matcher_ok(match):
            pm = scoring.prepare_matcher(match, hg)
            Qp = pm.queries(qf)
            thr = _device_positive_scores(pm, Qp, pos_off, pos_idx, block)
            scratch = {}

            def moments(beta):
                return torch.cat([pm.moments(Qp[q0:q0 + block], larger_is_better, beta, scratch) for q0 in range(0, Q, block)])
        else:
            from .evaluate import _ranks_of
            thr = _ranks_of(types.SimpleNamespace(match=match), hg, qf, pos_off, pos_idx, larger_is_better, block, with_thr=True)[1]

            def moments(beta):
                return torch.stack(scoring.score_moments_fused(match, hg, qf, larger_is_better, 1.0 / beta, block), dim=1)
        off = torch.as_tensor(off_h).to(dev)
        qid = torch.repeat_interleave(torch.arange(Q, device=dev), off[1:] - off[:-1])
        n = (off[1:] - off[:-1]).to(torch.float64)
        z = thr if larger_is_better else -thr

        def evaluate_at(beta):
            m = moments(beta)
            t = (z * torch.tensor(beta, dtype=torch.float32, device=dev)).to(torch.float64)        # fl32(beta z_j)
            tbar = torch.zeros(Q, dtype=torch.float64, device=dev).index_add_(0, qid, t) / n
            out = torch.stack([(m[:, 0] - tbar).mean(), (m[:, 1] - tbar).mean() / beta, m[:, 2].mean() / (beta * beta)]).cpu().tolist()
            if beta == 1.0 and not math.isfinite(out[0]):             # (the per-query terms are read back only to name the query)
                _raise_first_bad((m[:, 0] - tbar).cpu().numpy())
            return out
        return _newton_bracket(evaluate_at, lo, hi, rtol, max_iter)


def fit_temperature(model, dataset, device, larger_is_better=True, bounds=(1e-3, 1e3), rtol=1e-4, max_iter=30, qblock=None, seed=0,
                    batch_size=-1):
    """fit_temperature_scores on a dataset the way evaluate() gets there: `dataset` (a MaskedGraphDataset in 'validation' mode) gives
    the candidates (all_positions, encoded once) and the queries with their true parents (queries whose parents are not candidates are
    skipped).  Returns a Calibration; pass its .temperature to evaluate(..., temperature=) / infer(..., temperature=)."""
    from .evaluate import candidate_graphs
    device = torch.device(device)
    _fit_args(bounds, rtol, max_iter)
    cand = sorted(dataset.all_positions)
    index = {a: i for i, a in enumerate(cand)}
    dtax = dataset.device_taxonomy(device)
    g = candidate_graphs(dtax, cand, dataset.expand_factor, seed, batch_size)
    was_training = model.training
    model.eval()
    try:
        hg = scoring.encode_candidates(model, g)
        queries, pos_lists = [], []
        for q in dataset.node_list:
            p = [index[a] for a in dataset.node2parents[q] if a in index]
            if p:
                queries.append(q)
                pos_lists.append(p)
        pos_off = np.concatenate([[0], np.cumsum([len(p) for p in pos_lists])]).astype(np.int64)
        pos_idx = np.concatenate(pos_lists).astype(np.int64) if pos_lists else np.zeros(0, dtype=np.int64)
        qf = dataset.node_features[torch.as_tensor(queries, dtype=torch.long)].to(device)
        return fit_temperature_scores(model.match, hg, qf, pos_off, pos_idx, larger_is_better, bounds, rtol, max_iter, qblock)
    finally:
        model.train(was_training)


# ---------------------------------------------------------------------------------------------------------------
# calibration metrics
# ---------------------------------------------------------------------------------------------------------------
def expected_calibration_error(confidence, correct, bins=ECE_BINS):
    """ECE over `bins` equal-width bins of the confidence in [0, 1] (1.0 falls into the last): the sum over bins of
    share x |accuracy - mean confidence|, share = the bin's part of all n samples.  A NaN confidence falls into no bin.  Host, numpy;
    nan for no sample."""
    p = np.asarray(confidence, dtype=np.float64).reshape(-1)
    c = np.asarray(correct, dtype=np.float64).reshape(-1)
    if p.size == 0:
        return float("nan")
    ok = ~np.isnan(p)
    b = np.minimum(np.floor(np.where(ok, p, 0.0) * bins).astype(np.int64), bins - 1)
    ece = 0.0
    for k in range(bins):
        sel = ok & (b == k)
        if sel.any():
            ece += sel.sum() / p.size * abs(c[sel].mean() - p[sel].mean())
    return float(ece)


def _ece_device(confidence, correct, bins=ECE_BINS):
    """expected_calibration_error on device tensors (float64 confidence [n], bool correct [n]): a 0-dim float64 tensor, no read-back"""
    n = confidence.numel()
    if n == 0:
        return torch.full((), float("nan"), dtype=torch.float64, device=confidence.device)
    ok = ~torch.isnan(confidence)
    p = torch.where(ok, confidence, torch.zeros_like(confidence))
    b = torch.clamp((p * bins).floor().long(), max=bins - 1)
    w = ok.to(torch.float64)
    sp = torch.zeros(bins, dtype=torch.float64, device=p.device).index_add_(0, b, p * w)
    sc = torch.zeros(bins, dtype=torch.float64, device=p.device).index_add_(0, b, correct.to(torch.float64) * w)
    return ((sc - sp).abs() / n).sum()            # share x |accuracy - confidence| = (cnt / n) |sc / cnt - sp / cnt| per bin
