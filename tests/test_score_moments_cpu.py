"""CPU: the moments mode's host side -- scoring.host_score_moments against the independent reference (tests/score_moments_ref.py), the
reference's two halves against each other (merged tile quadruples = the direct row formulas, ragged G), the special-value table,
calibrate.host_fit_temperature on the five planted recipes with the fit's invariants, ECE on a hand-made example, every new ValueError,
every documented TXE_ERR_ARG of the four new entry points (returned before any device work: no GPU needed) and the ctypes table."""
import ctypes
import inspect
import math

import numpy as np
import pytest

import score_moments_ref as mr

BETAS = (1.0, 0.03, 7.5)


def _special_scores():
    rs = np.random.RandomState(3)
    S = (rs.standard_normal((12, 37)) * 6).astype(np.float32)
    S[1, 5] = np.nan
    S[2, 7] = np.inf
    S[3, 9] = -np.inf                                      # a finite row with a -Inf entry (larger) / a +Inf row (smaller)
    S[4, :] = -np.inf
    S[5, :] = np.inf
    S[6, 3], S[6, 4] = np.nan, np.inf
    S[7, 0] = 3000.0                                       # a leader far ahead at every beta: entropy 0, mean = max
    S[8, :] = -200.0
    S[9, 2], S[9, 3] = np.inf, -np.inf
    return S


def _close(got, want, rel=1e-12, abs_=1e-12):
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf])
    fin = np.isfinite(want)
    assert (np.abs(got[fin] - want[fin]) <= rel * np.abs(want[fin]) + abs_).all(), np.abs(got[fin] - want[fin]).max()


@pytest.mark.parametrize("larger", [True, False])
@pytest.mark.parametrize("beta", BETAS)
def test_host_score_moments_equals_the_reference(beta, larger):
    from taxoexpan_amd.scoring import ScoreMoments, host_score_moments
    S = _special_scores()
    got = host_score_moments(S, 1.0 / np.float32(beta).item(), larger)
    assert isinstance(got, ScoreMoments) and got._fields == ("lse", "mean", "var", "entropy")
    assert all(a.dtype == np.float64 and a.shape == (12,) for a in got)
    want = mr.row_moments(S, beta, larger)
    # (the direct formulas and the centred sums round differently: entropy and variance of a few units to 1e-12)
    _close(np.stack(got, axis=1), want, rel=1e-12, abs_=2e-12)


def test_special_value_table():
    from taxoexpan_amd.scoring import host_score_moments
    S = _special_scores()
    for larger in (True, False):
        for fn in (lambda: np.stack(host_score_moments(S, 1.0, larger), axis=1), lambda: mr.row_moments(S, 1.0, larger),
                   lambda: mr.merge_quads(*mr.tile_quads(S, 1.0, larger, tile=8))):
            m = fn()
            assert np.isnan(m[1]).all() and np.isnan(m[6]).all(), "a NaN in the row: all four NaN"
            inf_rows, ninf_rows = ([2, 5, 9], [4]) if larger else ([3, 4, 9], [5])
            for q in inf_rows:
                assert m[q, 0] == np.inf and np.isnan(m[q, 1:]).all(), (larger, q, m[q])
            for q in ninf_rows:
                assert m[q, 0] == -np.inf and np.isnan(m[q, 1:]).all(), (larger, q, m[q])
            fin = [q for q in range(12) if q not in (1, 6) + tuple(inf_rows) + tuple(ninf_rows)]
            assert np.isfinite(m[fin]).all()
    # a finite row with -Inf entries = the same row without them
    with_inf = host_score_moments(S[3:4], 0.5, True)
    without = host_score_moments(np.delete(S[3:4], 9, axis=1), 0.5, True)
    assert all(np.array_equal(a, b) for a, b in zip(with_inf, without))
    # one candidate; a leader more than 110 ahead after scaling
    one = host_score_moments(np.array([[2.5]], dtype=np.float32), 4.0, False)
    t = float(np.float32(0.25) * np.float32(-2.5))
    assert one.lse[0] == t and one.mean[0] == t and one.var[0] == 0.0 and one.entropy[0] == 0.0
    led = host_score_moments(S[7:8], 1.0, True)
    assert led.lse[0] == 3000.0 and led.mean[0] == 3000.0 and led.entropy[0] == 0.0 and led.var[0] == 0.0
    empty = host_score_moments(np.zeros((2, 0), dtype=np.float32))
    assert (empty.lse == -np.inf).all() and np.isnan(empty.entropy).all()


@pytest.mark.parametrize("G", [1, 127, 129, 300, 1000])
def test_tile_quads_merge_to_the_row_values(G):
    """the reference's two halves agree to 1e-12 relative: merging the per-tile quadruples gives the direct row formulas"""
    rs = np.random.RandomState(G)
    S = (rs.standard_normal((7, G)) * 4).astype(np.float32)
    S[2, G // 2] = -np.inf
    if G > 128:
        S[3, :128] = -np.inf                               # a whole tile empty
        S[4, 5] = 400.0                                    # a leader in the first tile: the other tiles lie far below
    for beta in BETAS:
        for larger in (True, False):
            want = mr.row_moments(S, beta, larger)
            got = mr.merge_quads(*mr.tile_quads(S, beta, larger, tile=128))
            scale = np.maximum(np.abs(want), 1.0)
            fin = np.isfinite(want)
            assert np.array_equal(fin, np.isfinite(got))
            assert np.array_equal(np.isnan(got), np.isnan(want))
            # (1e-12 relative, with an absolute floor of 1e-12 for the near-zero entropy and variance of a led row)
            assert (np.abs(got[fin] - want[fin]) <= 1e-12 * scale[fin]).all(), (G, beta, larger, np.abs(got[fin] - want[fin]).max())


@pytest.mark.parametrize("recipe,outcome", mr.RECIPES, ids=["x".join(map(str, r)) for r, _ in mr.RECIPES])
def test_host_fit_on_the_planted_recipes(recipe, outcome):
    from taxoexpan_amd import calibrate
    S, off, idx = mr.planted(*recipe)
    c = calibrate.host_fit_temperature(S, off, idx)
    assert c == calibrate.Calibration.from_state_dict(c.state_dict())
    assert c.temperature == 1.0 / c.beta and np.float32(c.beta) == c.beta
    assert c.nll_after <= c.nll_before
    f = lambda b: mr.nll(mr.row_moments(S, b)[:, 0], mr.scaled(S, b)[np.arange(len(idx)), idx], off)        # the reference's own NLL
    assert abs(f(1.0) - c.nll_before) <= 1e-10 * abs(c.nll_before) + 1e-12 and abs(f(c.beta) - c.nll_after) <= 1e-10 * abs(c.nll_after) + 1e-12
    if outcome == "interior":
        assert not c.at_bound and 1 <= c.iterations <= 10 and 1e-3 < c.beta < 1e3
        assert f(c.beta) <= f(c.beta * 1.05) and f(c.beta) <= f(c.beta / 1.05)
        # one positive per query: f - mean entropy = mean_q (E_p[t] - t_pos) = beta f' identically, and f' = 0 at the minimiser: the NLL
        # equals the mean entropy within |f'| beta rtol plus the moments' gate (its floor, 2e-5 of the value)
        b, _f, g, _h = c.history[-1]
        assert b == c.beta
        ent = mr.row_moments(S, c.beta)[:, 3].mean()
        assert abs((c.nll_after - ent) - c.beta * g) <= 1e-10 * max(1.0, c.nll_after), (c.nll_after, ent, g)
        assert abs(c.nll_after - ent) <= abs(g) * c.beta * 1e-4 + 2e-5 * max(abs(ent), 1.0), (c.nll_after, ent, g)
    else:
        assert c.at_bound and c.iterations == 0
        assert c.beta == float(np.float32(1e3 if outcome == "upper" else 1e-3))
    if recipe == (96, 300, 5, 3):                          # the figures written down with the algorithm (score_moments_ref.RECIPES: the other draws are not the issue's)
        assert abs(c.beta - 0.587) < 5e-4 and abs(c.nll_before - 2.420) < 5e-4 and abs(c.nll_after - 2.030) < 5e-4
    again = calibrate.host_fit_temperature(S, off, idx)
    assert again == c, "the fit is deterministic"
    got = calibrate.host_nll(S, off, idx, c.beta)
    assert got[0] == c.nll_after and got[2] >= 0.0


def test_fit_names_the_first_query_with_a_non_finite_term():
    from taxoexpan_amd import calibrate
    S, off, idx = mr.planted(12, 40, 1.0, 2.0)
    S[5, 3], S[9, 1] = np.nan, np.inf
    with pytest.raises(ValueError, match="query 5"):
        calibrate.host_fit_temperature(S, off, idx)


def test_ece_on_a_hand_made_example():
    from taxoexpan_amd import calibrate
    import torch
    conf = [0.95, 0.95, 0.55, 0.05, 1.0, 0.0]
    hit = [1, 1, 0, 0, 1, 1]
    # bins: [0.9, 1.0] holds 0.95, 0.95, 1.0 (accuracy 1, confidence 2.9 / 3); [0.5, 0.6) holds 0.55 (0 / 0.55); [0, 0.1) holds 0.05, 0.0 (1/2, 0.025)
    want = 3 / 6 * abs(1 - 2.9 / 3) + 1 / 6 * 0.55 + 2 / 6 * abs(0.5 - 0.025)
    assert abs(calibrate.expected_calibration_error(conf, hit) - want) < 1e-15
    assert abs(mr.ece(conf, hit) - want) < 1e-15
    dev = calibrate._ece_device(torch.tensor(conf, dtype=torch.float64), torch.tensor(hit, dtype=torch.bool))
    assert abs(float(dev) - want) < 1e-15
    assert calibrate.expected_calibration_error([0.5, 0.5], [1, 0]) == 0.0
    assert math.isnan(calibrate.expected_calibration_error([], []))


def test_every_new_value_error():
    from taxoexpan_amd import calibrate, ops, scoring
    from taxoexpan_amd.evaluate import evaluate, infer
    S, off, idx = mr.planted(6, 9, 1.0, 1.0)
    for T in (0.0, -1.0, float("nan"), float("inf"), 1e-46, 1e46, "x", None, True):
        with pytest.raises(ValueError):
            scoring.host_score_moments(S, T)
        with pytest.raises(ValueError):
            scoring.score_moments_fused(None, None, None, temperature=T)
        if T is not None:
            with pytest.raises(ValueError, match="temperature"):
                evaluate(None, None, "cpu", temperature=T)
            with pytest.raises(ValueError, match="temperature"):
                infer(None, None, None, "cpu", with_scores=True, temperature=T)
    for b in (0.0, -2.0, float("nan"), float("inf"), 1e-46):
        with pytest.raises(ValueError):
            ops._check_beta(b)
    with pytest.raises(ValueError, match="with_scores"):
        infer(None, None, None, "cpu", temperature=2.0)
    for kw in (dict(temperature=2.0), dict(predictive=True), dict(predictive={})):
        with pytest.raises(ValueError, match="retrieve"):
            evaluate(None, None, "cpu", retrieve=3, **kw)
    for kw in (dict(bounds=(1.0, 1.0)), dict(bounds=(2.0, 1.0)), dict(bounds=(0.0, 1.0)), dict(bounds=(1e-3, float("inf"))), dict(bounds=3.0),
               dict(rtol=0.0), dict(rtol=float("nan")), dict(max_iter=0), dict(max_iter=2.5)):
        with pytest.raises(ValueError):
            calibrate.host_fit_temperature(S, off, idx, **kw)
        with pytest.raises(ValueError):
            calibrate.fit_temperature_scores(None, None, None, off, idx, **kw)
    with pytest.raises(ValueError, match="true parent"):
        calibrate.host_fit_temperature(S, np.array([0, 1, 1, 2, 3, 4, 5]), idx[:5])
    assert inspect.signature(evaluate).parameters["temperature"].default is None
    assert inspect.signature(evaluate).parameters["predictive"].default is False
    assert inspect.signature(infer).parameters["temperature"].default is None
    assert list(inspect.signature(scoring.score_moments_fused).parameters) == ["match", "hg", "queries", "larger_is_better", "temperature", "block"]
    import taxoexpan_amd
    assert taxoexpan_amd.calibrate is calibrate and "calibrate" in taxoexpan_amd.__all__


def test_ctypes_table_names_the_new_symbols_and_their_argument_rules():
    """the four symbols; every documented TXE_ERR_ARG (-1) / TXE_ERR_WORKSPACE (-3) comes back before anything is launched (the pointers
    are host addresses, never read), and nq == 0 is TXE_OK without a launch"""
    from taxoexpan_amd import _lib
    names = ("txe_score_moments_block", "txe_mlp_score_moments_block", "txe_ntn_score_moments_block", "txe_moments_merge")
    assert all(n in _lib.SIGNATURES for n in names)
    lse, mom = _lib.SIGNATURES["txe_score_lse_block"][1], _lib.SIGNATURES["txe_score_moments_block"][1]
    assert len(mom) == len(lse) + 3 and mom[9] is ctypes.c_float
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    nan, inf = float("nan"), float("inf")
    # txe_score_moments_block(Q, ld_q, nq, U, ld_u, G, r, apply_exp, larger, beta, part_max, part_s0, part_s1, part_s2, out, sws, sws_bytes, u_packed, stream)
    good = [a, 8, 4, a, 8, 5, 8, 0, 1, 1.0, a, a, a, a, a, None, 0, None, None]

    def score(**kw):
        pos = dict(Q=0, ld_q=1, nq=2, U=3, ld_u=4, G=5, r=6, beta=9, part_max=10, part_s0=11, part_s1=12, part_s2=13, out=14, sws=15, sws_bytes=16,
                   u_packed=17)
        args = list(good)
        for k, v in kw.items():
            args[pos[k]] = v
        return lib.txe_score_moments_block(*args)
    for bad in (dict(nq=-1), dict(G=0), dict(G=-3), dict(r=0), dict(ld_u=7), dict(ld_q=7), dict(Q=None), dict(U=None), dict(part_max=None),
                dict(part_s0=None), dict(part_s1=None), dict(part_s2=None), dict(out=None), dict(beta=0.0), dict(beta=-1.0), dict(beta=nan),
                dict(beta=inf), dict(beta=-inf)):
        assert score(**bad) == -1, bad
    assert score(nq=0) == 0 and score(nq=0, beta=0.0) == -1
    need = lib.txe_score_split_ws_bytes(4, 5, 8)
    assert need > 0 and score(sws=a, sws_bytes=need - 1) == -3 and score(sws=a, sws_bytes=0) == -3
    # txe_moments_merge(part_max, part_s0, part_s1, part_s2, nq, cnt, out, stream)
    mgood = [a, a, a, a, 2, 3, a, None]
    for i, v in ((0, None), (1, None), (2, None), (3, None), (4, -1), (5, -1), (6, None)):
        args = list(mgood)
        args[i] = v
        assert lib.txe_moments_merge(*args) == -1, (i, v)
    assert lib.txe_moments_merge(a, a, a, a, 0, 3, a, None) == 0
    # txe_mlp_score_moments_block(Ap, flag_a, G, nB, c, flag_b, nq, H, mw, larger, beta, part_max, part_s0, part_s1, part_s2, out, stream)
    pgood = [a, a, 5, a, a, a, 4, 6, a, 1, 1.0, a, a, a, a, a, None]
    for i, v in ((0, None), (1, None), (2, 0), (2, -1), (3, None), (4, None), (5, None), (6, -1), (7, 0), (8, None), (10, 0.0), (10, nan), (10, inf),
                 (11, None), (12, None), (13, None), (14, None), (15, None)):
        args = list(pgood)
        args[i] = v
        assert lib.txe_mlp_score_moments_block(*args) == -1, (i, v)
    args = list(pgood)
    args[6] = 0
    assert lib.txe_mlp_score_moments_block(*args) == 0
    # txe_ntn_score_moments_block(Q, ld_q, nq, U, ld_u, slice_u, G, r, a, ld_a, c, ld_c, u, k, larger, beta, part_max, part_s0, part_s1, part_s2, out, stream)
    ngood = [a, 8, 4, a, 32, 8, 5, 8, a, 5, a, 4, a, 4, 1, 1.0, a, a, a, a, a, None]
    for i, v in ((0, None), (1, 7), (2, -1), (3, None), (4, 7), (5, 7), (6, 0), (6, -2), (7, 0), (8, None), (9, 4), (10, None), (11, 3), (12, None),
                 (13, 0), (13, 17), (15, 0.0), (15, -3.0), (15, nan), (15, inf), (16, None), (17, None), (18, None), (19, None), (20, None)):
        args = list(ngood)
        args[i] = v
        assert lib.txe_ntn_score_moments_block(*args) == -1, (i, v)
    args = list(ngood)
    args[2] = 0
    assert lib.txe_ntn_score_moments_block(*args) == 0
