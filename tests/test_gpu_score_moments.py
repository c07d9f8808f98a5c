"""The scoring loop's moments mode (the moments epilogue of gemm_tile_epilogue under gemm_kernel<true, true, V, V, -129>,
gemm_nt_split_kernel<2, 3, 2, 4> and ntn_score_kernel<-V>; mlp_pair_kernel<5>; moments_merge_kernel) against an INDEPENDENT reference, entry
point by entry point through the C ABI -- the test owns every pitch, scratch buffer and workspace -- then scoring.score_moments_fused,
calibrate.fit_temperature_scores on planted scores and evaluate(temperature=, predictive=) / infer(temperature=) on the toy taxonomy.

Reference: tests/score_moments_ref.py (plain numpy, float64; tests/test_score_moments_cpu.py holds the project's host code to it).
  (a) VALUES: (lse, mean, var, entropy) of every row against the reference applied to the device's OWN materialised fp32 scores of the same
      route (txe_score_block / txe_mlp_score_block / txe_ntn_score_block), through golden_util.gate_against_f64 at its defaults; the
      yardstick is the same four quantities formed with fp32 torch ops (softmax, weighted mean and variance) on those scores.  Every gate
      prints "[gate] op what device yardstick".  beta in {1, 0.03, 7.5}, both apply_exp values, both directions, the three routes of the
      bilinear form; MLP with H = 8, 100; NTN with k = 1, 4.
  (b) EXACT, no tolerance: at beta = 1 (float)lse has txe_*_score_lse_block's bits; G = 1 gives entropy == 0, var == 0, mean == (double)t;
      a row whose leader is more than 110 ahead after scaling gives entropy == 0 and mean == max; rows with NaN / +Inf / only -Inf follow
      the special-value table; -Inf entries behind a finite row change no bit; the same query alone, in a block of 130 at another row
      position and in a second run gives equal bits; the three routes give equal bits wherever their scores do.
  (c) txe_moments_merge alone on quadruples the test writes (cnt = 0 too), and the error codes.
Shapes (G, nq, r): (1, 1, 8), (127, 3, 20), (129, 130, 250) -- a ragged second column tile and a second row panel --, (300, 5, 64),
(1000, 257, 12).

Measured on the MI355X (256 CUs), one run of the file: 46 cases in 5.4 s, the slowest 0.6 s.  Errors as fractions of the case's largest
|reference|: lse at most 2.1e-7 (yardstick 2.2e-7); mean 3.0e-6 (a flat row at beta = 0.03 whose mean lies near 0: M + S1/S0 cancels;
yardstick 2.1e-7); entropy 1.7e-6 (yardstick 2.0e-6); var 8.0e-6 (129 x 130 x 250 under the exp at beta = 0.03: S2/S0 - (S1/S0)^2 is
centred at the maximum, not at the mean; yardstick 1.1e-7) -- all below the gate's floor of 2e-5.  The fitted beta equals the host
restatement's on the device's scores to the last bit on all five planted recipes.  profiles/NOTES.md, "Calibrated probabilities".
"""
import os
import shutil

import numpy as np
import pytest
import torch

import score_moments_ref as mr
from golden_util import GOLDEN_DIR
from test_gpu_log_partition import _bits, _lse_block, _lse_names, _plain
from test_gpu_readout_match_ops import _profiled
from test_gpu_scoring_loop_ops import GUARD, ROUTES, _gate, _L, _dev, _nan, _ok, _rc, _score_block, _st, _tail_intact

pytestmark = pytest.mark.gpu

BETAS = (1.0, 0.03, 7.5)
#        G    nq    r  ld_q ld_u
CASES = [(1, 1, 8, 8, 8), (127, 3, 20, 21, 23), (129, 130, 250, 252, 252), (300, 5, 64, 64, 68), (1000, 257, 12, 12, 12)]
QUANT = ("lse", "mean", "var", "entropy")


def _inputs(G, nq, r, seed, exp):
    rs = np.random.RandomState(seed)
    Q = (rs.standard_normal((nq, r)) * (0.5 if exp else 2.0) / np.sqrt(r)).astype(np.float32)     # scores of order 2 (under the exp: 1/2)
    U = rs.standard_normal((G, r)).astype(np.float32)
    return Q, U


def _dnan(n):
    return torch.full((max(int(n), 1),), float("nan"), dtype=torch.float64, device=_dev())


def _mom_names(I, route):
    sub = {"lse_merge_kernel": "moments_merge_kernel", "gemm_nt_split_kernel<2, 3, 2, 3>": "gemm_nt_split_kernel<2, 3, 2, 4>"}
    return [sub.get(n, n.replace(", -128>", ", -129>") if n.startswith("gemm_kernel<") else n) for n in _lse_names(I, route)]


def _scratch(nq, tiles):
    return [_nan(nq * tiles + GUARD) for _ in range(4)], _dnan(4 * nq + GUARD)


def _out(parts, out, nq, tiles):
    for t in parts:
        _tail_intact(t, nq * tiles)
    assert bool(torch.isnan(out[4 * nq:]).all()), "words behind out's documented size were written"
    return out.cpu().numpy()[:4 * nq].reshape(nq, 4).copy()


def _mom_block(I, route, exp, larger, beta, nq=None, G=None, qp=None):
    """txe_score_moments_block into primed scratch: float64 [nq, 4]; every word behind a buffer's documented size still NaN"""
    nq, G = I.nq if nq is None else nq, I.G if G is None else G
    tiles = (G + 127) // 128
    parts, out = _scratch(nq, tiles)
    sb, swp, swb, upk = I.sws(route, "topk")
    _r, names = _profiled(lambda: _ok("txe_score_moments_block", I.Qp if qp is None else qp, I.ld_q, nq, I.Up_, I.ld_u, G, I.r, int(exp), int(larger),
                                       float(beta), *(t.data_ptr() for t in parts), out.data_ptr(), swp, swb, upk, _st()))
    if nq == I.nq and G == I.G:
        assert names == _mom_names(I, route), (names, _mom_names(I, route))
    if sb is not None:
        _tail_intact(sb, swb // 4)
    return _out(parts, out, nq, tiles)


def _b64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _yard(S, beta, larger):
    """the four quantities with fp32 torch ops on the scores: softmax, weighted mean and variance"""
    z = torch.from_numpy(np.ascontiguousarray(S if larger else -S))
    t = z * torch.tensor(beta, dtype=torch.float32)
    lse = torch.logsumexp(t, dim=1)
    logp = torch.log_softmax(t, dim=1)
    p = torch.softmax(t, dim=1)
    tz = torch.where(p > 0, t, torch.zeros_like(t))
    mean = (p * tz).sum(1)
    var = (p * torch.where(p > 0, (t - mean[:, None]) ** 2, torch.zeros_like(t))).sum(1)
    ent = -(p * torch.where(p > 0, logp, torch.zeros_like(t))).sum(1)
    return torch.stack([lse, mean, var, ent], dim=1).numpy().astype(np.float64)


def _same_pattern(got, ref):
    """the special-value table, exactly: lse's NaN / +Inf / -Inf as the reference's, the other three NaN there -> the finite rows"""
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf]), (got, ref)
    fin = np.isfinite(ref[:, 0])
    assert np.isfinite(got[fin]).all() and np.isnan(got[~fin, 1:]).all()
    return fin


def _gate_rows(items, what, got, S, beta, larger):
    ref = mr.row_moments(S, beta, larger)
    fin = _same_pattern(got, ref)
    assert (got[fin, 2] >= 0).all() and (got[fin, 3] >= 0).all()
    if fin.any():
        yard = _yard(S, beta, larger)
        for k, name in enumerate(QUANT):
            items.append((f"{name} {what}", got[fin, k], ref[fin, k], yard[fin, k]))


def _lse_bits_equal(mom, lse):
    """(float)out[q][0] has the lse entry point's bits (a NaN is a NaN on both sides)"""
    a, b = mom[:, 0].astype(np.float32), np.asarray(lse, dtype=np.float32)
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan) and np.array_equal(_bits(a[~nan]), _bits(b[~nan])), (a, b)


# ---- (a) + (b): the bilinear form -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exp", [0, 1])
@pytest.mark.parametrize("case", range(len(CASES)), ids=["x".join(map(str, c[:3])) for c in CASES])
def test_bilinear_values_and_bits(case, exp):
    G, nq, r, ld_q, ld_u = CASES[case]
    Q, U = _inputs(G, nq, r, 20 + case, exp)
    I = _plain(Q, U, ld_q, ld_u)
    items, by_route = [], {}
    for route in ROUTES:
        S = _score_block(I, route, exp)
        for larger in (1, 0):
            for beta in BETAS:
                got = _mom_block(I, route, exp, larger, beta)
                _gate_rows(items, f"[{G}x{nq}x{r} {route} exp {exp} larger {larger} beta {beta}]", got, S, beta, larger)
                if beta == 1.0:
                    _lse_bits_equal(got, _lse_block(I, route, exp, larger))
                if G == 1:
                    t = mr.scaled(S, beta, larger)[:, 0]
                    assert (got[:, 3] == 0).all() and (got[:, 2] == 0).all() and np.array_equal(_b64(got[:, 1]), _b64(t)) and \
                        np.array_equal(_b64(got[:, 0]), _b64(t)), "one candidate: entropy 0, variance 0, mean = lse = (double)t"
                by_route[route, larger, beta] = (S, got)
    for larger in (1, 0):                                   # the same scores give the same four values on every route
        for beta in BETAS:
            S0, g0 = by_route["mfma", larger, beta]
            for route in ROUTES[1:]:
                S1, g1 = by_route[route, larger, beta]
                same = (_bits(S0) == _bits(S1)).all(axis=1)
                assert np.array_equal(_b64(g0)[same], _b64(g1)[same]), route
            assert np.array_equal(_b64(by_route["split", larger, beta][1]), _b64(by_route["packed", larger, beta][1])), "planes packed per call / once"
    _gate("txe_score_moments_block", items)


def test_bilinear_leader_and_special_values():
    """exact results: a leader more than 110 ahead after scaling (in another tile than most of the row); NaN / +Inf / -Inf planted through
    query rows; huge values planted in the rows behind nq and the candidates behind G"""
    G, nq, r = 257, 130, 32
    rs = np.random.RandomState(G)
    Q = (rs.standard_normal((nq + 3, r)) * 0.5).astype(np.float32)
    U = (rs.standard_normal((G + 5, r)) * 0.5).astype(np.float32)
    Q[:, 0], Q[:, 1] = 1.0, 1.0
    U[:, 0] = rs.uniform(0.5, 1.5, size=G + 5).astype(np.float32)             # (positive: an infinite query entry there gives one sign)
    lead = [G // 2, G - 1]                                                   # one leader per direction, in different tiles
    U[lead[0], 1], U[lead[1], 1] = 200.0, -200.0
    Q[nq:], U[G:] = 1e30, 1e30                                               # the padding: never read as a query, never counted as a candidate
    Q[3], Q[64], Q[65], Q[127] = np.nan, 0.0, 0.0, 0.0
    Q[64, 0], Q[65, 0], Q[127, 0], Q[127, 1] = np.inf, -np.inf, 1e38, 1e37    # all +Inf; all -Inf; finite but for the leaders' overflow
    I = _plain(Q, U, r + 4, r)
    Iref = _plain(Q[:nq].copy(), U[:G].copy(), I.ld_q, I.ld_u)
    items = []
    for route in ROUTES:
        S = _score_block(Iref, route, 0)
        if route == "mfma":
            assert np.isnan(S[3]).all() and (S[64] == np.inf).all() and (S[65] == -np.inf).all() and S[127, lead[0]] == np.inf and S[127, lead[1]] == -np.inf
        for larger in (1, 0):
            for beta in (1.0, 7.5):
                got = _mom_block(I, route, 0, larger, beta, nq=nq, G=G)
                assert np.array_equal(_b64(got), _b64(_mom_block(Iref, route, 0, larger, beta))), "rows >= nq or columns >= G leaked into the sums"
                _gate_rows(items, f"[{G}x{nq}x{r} {route} larger {larger} beta {beta}]", got, S, beta, larger)
                if beta == 1.0:
                    _lse_bits_equal(got, _lse_block(Iref, route, 0, larger))
                t = mr.scaled(S, beta, larger)
                top = np.sort(np.where(np.isnan(t), -np.inf, t), axis=1)
                with np.errstate(invalid="ignore"):
                    led = np.isfinite(got[:, 0]) & (top[:, -1] - top[:, -2] > 110)
                assert led.sum() >= nq - 8
                assert (got[led, 3] == 0).all() and np.array_equal(_b64(got[led, 1]), _b64(top[led, -1])) and \
                    np.array_equal(_b64(got[led, 0]), _b64(top[led, -1])), "a leader more than 110 ahead: entropy 0, mean = lse = the maximum"
                assert (got[led, 2] == 0).all()
    _gate("txe_score_moments_block special", items)


@pytest.mark.parametrize("larger", [1, 0])
def test_minus_inf_entries_add_nothing(larger):
    """a finite row with t = -Inf entries: four finite outputs, bit-equal to the same row without those entries (they stand behind the
    row's other candidates, in a tile of their own and in a shared one, so that no other candidate changes its place in the sums)"""
    r, nq = 8, 5
    for G, n_inf in ((131, 2), (131, 3), (260, 4)):        # the -Inf tail: part of the last tile; reaching into the tile before it; a whole tile + 1
        Q, U = _inputs(G, nq, r, G + n_inf, 0)
        Q[:, 2] = 1e38 if larger else -1e38
        U[:, 2] = 0.0
        U[G - n_inf:, 2] = -16.0                            # 1e38 x -16 overflows: s = -Inf (larger) / +Inf, z = -Inf (smaller is better)
        I = _plain(Q, U, r, r)
        Iw = _plain(Q, U[:G - n_inf].copy(), r, r)          # the same rows without those entries
        for route in ROUTES:
            S = _score_block(I, route, 0)
            z = S if larger else -S
            assert (z[:, G - n_inf:] == -np.inf).all() and np.isfinite(z[:, :G - n_inf]).all(), route
            for beta in (1.0, 0.03):
                got = _mom_block(I, route, 0, larger, beta)
                assert np.isfinite(got).all()
                assert np.array_equal(_b64(got), _b64(_mom_block(Iw, route, 0, larger, beta))), (route, G, n_inf, beta)


def test_bilinear_purity_over_blocks_and_positions():
    """a query's four values are a function of its row's scores and beta: alone in a block of 1, in a block of 130 at another row position,
    in blocks of 50, and in a second run"""
    G, nq, r = 300, 130, 32
    Q, U = _inputs(G, nq, r, 5, 0)
    I = _plain(Q, U, r, r)
    Ir = _plain(np.roll(Q, 37, axis=0), U, r, r)
    for route in ROUTES:
        for larger, beta in ((1, 7.5), (0, 0.03), (1, 1.0)):
            whole = _mom_block(I, route, 0, larger, beta)
            for q in (0, 57, 129):
                alone = _mom_block(I, route, 0, larger, beta, nq=1, qp=I.Qp + 4 * q * I.ld_q)
                assert np.array_equal(_b64(whole[q:q + 1]), _b64(alone)), (route, "a block of 1", q)
            parts = [_mom_block(I, route, 0, larger, beta, nq=min(50, nq - q0), qp=I.Qp + 4 * q0 * I.ld_q) for q0 in range(0, nq, 50)]
            assert np.array_equal(_b64(whole), _b64(np.concatenate(parts))), (route, "blocks of 50")
            assert np.array_equal(_b64(whole), _b64(np.roll(_mom_block(Ir, route, 0, larger, beta), -37, axis=0))), (route, "row position")
            assert np.array_equal(_b64(whole), _b64(_mom_block(I, route, 0, larger, beta))), (route, "run to run")


def test_rejected_calls_leave_everything_primed():
    G, nq, r = 129, 7, 32
    Q, U = _inputs(G, nq, r, 1, 0)
    I = _plain(Q, U, r, r)
    need = _L().call("txe_score_split_ws_bytes", nq, G, r)
    assert need > 16
    parts, out = _scratch(nq, 2)
    sws = _nan(need // 4)
    p = [t.data_ptr() for t in parts]

    def args(G_=G, ld_q=I.ld_q, nq_=nq, beta=1.0, parts_=p, out_=out.data_ptr(), sw=None, swb=0):
        return (I.Qp, ld_q, nq_, I.Up_, I.ld_u, G_, r, 0, 1, beta, *parts_, out_, sw, swb, None, _st())
    calls = [(-1, args(G_=0)), (-1, args(ld_q=r - 1)), (-1, args(beta=0.0)), (-1, args(beta=-2.0)), (-1, args(beta=float("nan"))),
             (-1, args(beta=float("inf"))), (-1, args(out_=None)), (-3, args(sw=sws.data_ptr(), swb=need - 16)), (0, args(nq_=0))]
    calls += [(-1, args(parts_=p[:i] + [None] + p[i + 1:])) for i in range(4)]
    for want, a in calls:
        rc, names = _profiled(lambda: _rc("txe_score_moments_block", *a))
        assert rc == want and names == [], (want, rc, names)
    rc, names = _profiled(lambda: _rc("txe_moments_merge", *p, nq, -1, out.data_ptr(), _st()))
    assert rc == -1 and names == []
    rc, names = _profiled(lambda: _rc("txe_moments_merge", *p, 0, 2, out.data_ptr(), _st()))
    assert rc == 0 and names == []
    for t in parts + [sws]:
        _tail_intact(t, 0)
    assert bool(torch.isnan(out).all())


# ---- (c) the merge alone ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cnt", [0, 1, 3, 64, 65, 200])
def test_moments_merge_alone(cnt):
    nq = 9
    rs = np.random.RandomState(cnt)
    pm = (rs.standard_normal((nq, cnt)) * 20).astype(np.float32)
    p0 = rs.uniform(1.0, 128.0, size=(nq, cnt)).astype(np.float32)
    u = rs.uniform(0.0, 3.0, size=(nq, cnt))
    p1 = (-u * p0).astype(np.float32)                                        # sum d e = -u s0
    p2 = (1.5 * u * u * p0).astype(np.float32)                               # sum d^2 e >= (sum d e)^2 / s0
    if cnt:
        pm[1, :], p0[1, :], p1[1, :], p2[1, :] = -np.inf, 0.0, 0.0, 0.0      # every slot empty
        pm[2, ::2], p0[2, ::2], p1[2, ::2], p2[2, ::2] = -np.inf, 0.0, 0.0, 0.0   # empty slots among real ones
        pm[3, cnt // 2] = np.nan
        pm[4, cnt - 1] = np.inf
        pm[5, cnt - 1], pm[5, 0] = np.inf, np.nan                            # NaN wins over +Inf
        pm[6, :] = -300.0
        pm[6, 0], p0[6, 0], p1[6, 0], p2[6, 0] = 7.25, 1.0, 0.0, 0.0         # a lone leader: the rest vanish beside it
    want = mr.merge_quads(pm, p0, p1, p2)
    dev = []
    for a in (pm, p0, p1, p2):
        t = _nan(nq * cnt + GUARD)
        t[:nq * cnt].copy_(torch.from_numpy(a.reshape(-1)))
        dev.append(t)
    out = _dnan(4 * nq + GUARD)
    _r, names = _profiled(lambda: _ok("txe_moments_merge", *(t.data_ptr() for t in dev), nq, cnt, out.data_ptr(), _st()))
    assert names == ["moments_merge_kernel"]
    assert bool(torch.isnan(out[4 * nq:]).all())
    got = out.cpu().numpy()[:4 * nq].reshape(nq, 4)
    fin = _same_pattern(got, want)
    if cnt == 0:
        assert (got[:, 0] == -np.inf).all() and np.isnan(got[:, 1:]).all()
        return
    assert np.isneginf(got[1, 0]) and np.isnan(got[3, 0]) and got[4, 0] == np.inf and np.isnan(got[5, 0])
    assert got[6, 0] == 7.25 and got[6, 1] == 7.25 and got[6, 2] == 0.0 and got[6, 3] == 0.0
    # float64 arithmetic on the given quadruples: the device differs from the reference by the rounding of exp, log and the sums alone
    err = np.abs(got[fin] - want[fin])
    assert (err <= 1e-12 * np.maximum(np.abs(want[fin]), 1.0) * max(1, cnt)).all(), (got, want)


# ---- NTN and MLP ---------------------------------------------------------------------------------------------------------------------------------
def _primed_call(name, head, larger, beta, nq, G, want_names):
    tiles = (G + 127) // 128
    parts, out = _scratch(nq, tiles)
    _r, names = _profiled(lambda: _ok(name, *head, int(larger), float(beta), *(t.data_ptr() for t in parts), out.data_ptr(), _st()))
    assert names == want_names, names
    return _out(parts, out, nq, tiles)


def _primed_lse(name, head, larger, nq, G):
    tiles = (G + 127) // 128
    pm, ps, out = _nan(nq * tiles + GUARD), _nan(nq * tiles + GUARD), _nan(nq + GUARD)
    _ok(name, *head, int(larger), pm.data_ptr(), ps.data_ptr(), out.data_ptr(), _st())
    return out.cpu().numpy()[:nq].copy()


@pytest.mark.parametrize("G,nq,l,r,k", [(129, 130, 5, 9, 1), (300, 5, 17, 12, 4), (1, 1, 3, 3, 4)])
def test_ntn_values_and_bits(G, nq, l, r, k):
    from taxoexpan_amd import ops
    from taxoexpan_amd.model_zoo import NTN
    torch.manual_seed(G + k)
    m = NTN(l, r, k=k, non_linear=torch.tanh).to(_dev())
    with torch.no_grad():
        m.u_R.weight.mul_(6.0)                                               # scores spread over several units: the sums are not flat
    hg, q = torch.randn(G, l, device=_dev()), torch.randn(nq, r, device=_dev())
    prep = ops.ntn_project(hg, m)
    qp = ops.ntn_prepare_queries(q, prep)
    head = ops._ntn_args(qp, prep)
    S = ops.ntn_score_block(qp, prep).cpu().numpy()
    names = ["ntn_score_kernel[moments]", "moments_merge_kernel"]
    items = []
    for larger in (1, 0):
        for beta in BETAS:
            got = _primed_call("txe_ntn_score_moments_block", head, larger, beta, nq, G, names)
            _gate_rows(items, f"ntn [{G}x{nq}x{r} k {k} larger {larger} beta {beta}]", got, S, beta, larger)
            if beta == 1.0:
                _lse_bits_equal(got, _primed_lse("txe_ntn_score_lse_block", head, larger, nq, G))
            if G == 1:
                assert (got[:, 2:] == 0).all() and np.array_equal(_b64(got[:, 1]), _b64(mr.scaled(S, beta, larger)[:, 0]))
            if nq > 1:
                sub = ops.NTNQueries(qp.Qp[nq // 2:], qp.c[:, nq // 2:], nq - nq // 2)                   # the second half as a block of its own
                half = _primed_call("txe_ntn_score_moments_block", ops._ntn_args(sub, prep), larger, beta, sub.n, G, names)
                assert np.array_equal(_b64(half), _b64(got[nq // 2:])), "a row's values depend on the block it is in"
    _gate("txe_ntn_score_moments_block", items)


@pytest.mark.parametrize("G,nq,H,r", [(129, 130, 8, 9), (300, 5, 100, 12), (1000, 257, 8, 3), (1, 1, 100, 8)])
def test_mlp_values_and_bits_with_flagged_rows(G, nq, H, r):
    from taxoexpan_amd import ops
    from taxoexpan_amd.model_zoo import MLP
    l = 6
    torch.manual_seed(G + H)
    m = MLP(l, r, H).to(_dev())
    hg, q = torch.randn(G, l, device=_dev()) * 3, torch.randn(nq, r, device=_dev()) * 3
    if G > 100:
        hg[G // 3] = 1e37                                                    # a flagged candidate row (the literal per-pair formula): huge
    if nq == 130:
        q[5] = -2e37                                                         # flagged query rows
        q[129, 1] = float("nan")
    prep = ops.mlp_project(hg, m)
    qp = ops.mlp_prepare_queries(q, prep)
    head = ops._mlp_args(qp, prep)
    S = ops.mlp_score_block(qp, prep).cpu().numpy()
    names = ["mlp_pair_kernel[moments]", "moments_merge_kernel"]
    items = []
    for larger in (1, 0):
        for beta in BETAS:
            got = _primed_call("txe_mlp_score_moments_block", head, larger, beta, nq, G, names)
            _gate_rows(items, f"mlp [{G}x{nq} H {H} larger {larger} beta {beta}]", got, S, beta, larger)
            if beta == 1.0:
                _lse_bits_equal(got, _primed_lse("txe_mlp_score_lse_block", head, larger, nq, G))
            if G == 1:
                assert (got[:, 2:] == 0).all() and np.array_equal(_b64(got[:, 1]), _b64(mr.scaled(S, beta, larger)[:, 0]))
            if nq == 130:
                assert np.isnan(got[129]).all()
    _gate("txe_mlp_score_moments_block", items)


# ---- module level: the fit on planted scores ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recipe,outcome", mr.RECIPES, ids=["x".join(map(str, r)) for r, _ in mr.RECIPES])
def test_fit_temperature_scores_on_planted_scores(recipe, outcome):
    """the planted scores go through a BIM whose W is the identity: candidate g's vector is column g of S, query q is the unit vector e_q"""
    from taxoexpan_amd import calibrate, scoring
    from taxoexpan_amd.model_zoo import BIM
    S, off, idx = mr.planted(*recipe)
    host = calibrate.host_fit_temperature(S, off, idx)      # the outcome on the host restatement, before the device is compared with anything
    assert host.at_bound == (outcome != "interior") and (host.iterations == 0) == host.at_bound
    Q, G = S.shape
    m = BIM(Q, Q).to(_dev())
    with torch.no_grad():
        m.W.weight.copy_(torch.eye(Q)[None])
        hg = torch.from_numpy(np.ascontiguousarray(S.T)).to(_dev())
        qf = torch.eye(Q, device=_dev())
        Sd = scoring.score_all(m, hg, qf).cpu().numpy()
    assert np.allclose(Sd, S, rtol=1e-6, atol=0.0), "the planted scores come back"
    host = calibrate.host_fit_temperature(Sd, off, idx)     # ... and on the device's own scores, which the device fit is compared with
    rtol = 1e-4
    c = calibrate.fit_temperature_scores(m, hg, qf, off, idx, rtol=rtol)
    assert c == calibrate.Calibration.from_state_dict(c.state_dict())
    print(f"[fit] {recipe} device beta {c.beta!r} host {host.beta!r} nll {c.nll_before!r} -> {c.nll_after!r} iterations {c.iterations} ({host.iterations})")
    assert abs(c.beta - host.beta) <= 10 * rtol * host.beta
    assert c.at_bound == host.at_bound and c.nll_after <= c.nll_before
    f = lambda b: calibrate.host_nll(Sd, off, idx, b)[0]     # the host f on the device's scores
    _gate("fit_temperature_scores", [(f"nll_before {recipe}", np.array([c.nll_before]), np.array([f(1.0)]), np.array([f(1.0)], dtype=np.float32)),
                                      (f"nll_after {recipe}", np.array([c.nll_after]), np.array([f(c.beta)]), np.array([f(c.beta)], dtype=np.float32))])
    if outcome == "interior":
        assert f(c.beta) <= f(c.beta * 1.05) and f(c.beta) <= f(c.beta / 1.05)
        ent = float(np.mean(mr.row_moments(Sd, c.beta)[:, 3]))
        b, _f, g, _h = c.history[-1]
        # f - mean entropy = beta f' identically (one positive per query) and f' = 0 at the minimiser: within |f'| beta rtol plus the
        # moments' gate (its floor, 2e-5 of the value)
        assert b == c.beta and abs(c.nll_after - ent) <= abs(g) * c.beta * rtol + 2e-5 * max(abs(ent), 1.0), (c.nll_after, ent, g)
    else:
        assert c.iterations == 0 and c.beta == float(np.float32(1e3 if outcome == "upper" else 1e-3))
    assert calibrate.fit_temperature_scores(m, hg, qf, off, idx, rtol=rtol) == c, "the fit is deterministic"


# ---- module level: the toy taxonomy ------------------------------------------------------------------------------------------------------------
def _toy(tmp_path, mode="test"):
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    for fn in os.listdir(os.path.join(GOLDEN_DIR, "toy_taxo")):
        shutil.copy(os.path.join(GOLDEN_DIR, "toy_taxo", fn), tmp_path)
    return MaskedGraphDataset(MAGDataset("toy", str(tmp_path), raw=True), mode=mode, sampling_mode=0, expand_factor=100, normalize_embed=True)


def _model(match):
    from test_gpu_log_partition import _model as model
    return model(match)


def _toy_scores(model, ds, rows, queries=None):
    """(S [Q, G] numpy of the candidate rows `rows` against the dataset's queries or the given vectors, hg, qf)"""
    from taxoexpan_amd import scoring
    from taxoexpan_amd.evaluate import _score_blocks, candidate_graphs
    with torch.no_grad():
        hg = scoring.encode_candidates(model, candidate_graphs(ds.device_taxonomy(_dev()), rows, ds.expand_factor, 0))
        qf = queries if queries is not None else ds.node_features[torch.as_tensor(list(ds.node_list), dtype=torch.long)].to(_dev())
        if scoring.fused_matcher_ok(model.match):
            S = scoring.score_all(model.match, hg, qf)
        else:
            S = torch.cat([s for _q0, s in _score_blocks(model, hg, qf, 1024)])
    return S.cpu().numpy(), hg, qf


@pytest.mark.parametrize("match", ["LBM", "BIM", "MLP", "NTN", "NTN-relu"])
def test_score_moments_fused_on_the_toy_taxonomy(tmp_path, match):
    from taxoexpan_amd import scoring
    ds = _toy(tmp_path)
    model = _model(match)
    assert scoring.fused_matcher_ok(model.match) == (match != "NTN-relu")
    S, hg, qf = _toy_scores(model, ds, sorted(ds.all_positions))
    items = []
    with torch.no_grad():
        for larger in (True, False):
            for T in (1.0, 4.0, 0.2):
                got = scoring.score_moments_fused(model.match, hg, qf, larger, temperature=T)
                assert isinstance(got, scoring.ScoreMoments)
                assert all(a.dtype == torch.float64 and a.shape == (qf.shape[0],) and a.device == hg.device for a in got)
                beta = float(np.float32(1.0 / T))
                g = torch.stack(got, dim=1).cpu().numpy()
                _gate_rows(items, f"{match} larger {larger} T {T}", g, S, beta, larger)
                host = np.stack(scoring.host_score_moments(S, T, larger), axis=1)
                assert np.allclose(host, mr.row_moments(S, beta, larger), rtol=1e-10, atol=1e-10)
                if match != "NTN-relu":
                    blocked = scoring.score_moments_fused(model.match, hg, qf, larger, temperature=T, block=3)
                    assert all(torch.equal(a, b) for a, b in zip(blocked, got)), "blocks of 3 queries"
                    if T == 1.0:
                        _lse_bits_equal(g, scoring.log_partition_fused(model.match, hg, qf, larger).cpu().numpy())
    _gate("score_moments_fused", items)


@pytest.mark.parametrize("match,larger", [("LBM", True), ("BIM", False), ("MLP", True), ("NTN", True)])
def test_evaluate_with_temperature_and_predictive(tmp_path, match, larger):
    from taxoexpan_amd import calibrate
    from taxoexpan_amd.evaluate import evaluate
    ds = _toy(tmp_path)
    model = _model(match)
    T = 2.5
    beta = float(np.float32(1.0 / T))
    m0, r0, off0, q0 = evaluate(model, ds, _dev(), larger_is_better=larger)
    m1, r1, off1, q1 = evaluate(model, ds, _dev(), larger_is_better=larger, nll=True)
    tensors = {}
    m2, r2, off2, q2 = evaluate(model, ds, _dev(), larger_is_better=larger, nll=True, temperature=T, predictive=tensors)
    new = {"nll", "entropy", "confidence", "ece"}
    assert set(m2) == set(m0) | new and {k: v for k, v in m2.items() if k not in new} == m0
    assert torch.equal(r0, r2) and np.array_equal(off0, off2) and q0 == q2 and torch.equal(r0, r1)
    m3 = evaluate(model, ds, _dev(), larger_is_better=larger, predictive=True)[0]
    assert set(m3) == set(m0) | (new - {"nll"})
    m4 = evaluate(model, ds, _dev(), larger_is_better=larger, nll=True, predictive=True)[0]
    assert m4["nll"] == m1["nll"], "without a temperature nll stays on the lse route: the value a call without `predictive` reports"
    assert evaluate(model, ds, _dev(), larger_is_better=larger, temperature=T)[0] == m0, "a temperature alone changes nothing reported"
    assert set(tensors) == {"lse", "mean", "var", "entropy", "top1_prob", "correct"}
    cand = sorted(ds.all_positions)
    index = {a: i for i, a in enumerate(cand)}
    S, _hg, _qf = _toy_scores(model, ds, cand, ds.node_features[torch.as_tensor(q2, dtype=torch.long)].to(_dev()))
    pos = [i for q in q2 for i in (index[a] for a in ds.node2parents[q] if a in index)]
    rows = np.repeat(np.arange(len(q2)), np.diff(off2))
    items = []
    for name, b, got in (("nll T=1", 1.0, m1["nll"]), (f"nll T={T}", beta, m2["nll"])):
        want = mr.nll(mr.row_moments(S, b, larger)[:, 0], mr.scaled(S, b, larger)[rows, pos], off2)
        yard = mr.nll(_yard(S, b, larger)[:, 0], mr.scaled(S, b, larger)[rows, pos].astype(np.float32), off2)
        print(f"[nll] {match} {name} device {got!r} float64 {want!r} fp32 yardstick {yard!r}")
        items.append((f"{name} {match}", np.array([got]), np.array([want]), np.array([yard])))
    assert abs(calibrate.host_nll(S, off2, pos, beta, larger)[0] - items[1][2][0]) <= 1e-10 * max(1.0, abs(items[1][2][0]))
    ref, yard = mr.row_moments(S, beta, larger), _yard(S, beta, larger)
    for k, name in enumerate(QUANT):
        items.append((f"predictive {name} {match}", tensors[name].cpu().numpy(), ref[:, k], yard[:, k]))
    t = mr.scaled(S, beta, larger)
    p_ref = np.exp(t.max(axis=1) - ref[:, 0])
    p_yard = np.exp((t.max(axis=1) - yard[:, 0]).astype(np.float32)).astype(np.float64)
    p_dev = tensors["top1_prob"].cpu().numpy()
    items.append((f"top1_prob {match}", p_dev, p_ref, p_yard))
    assert (p_dev <= 1.0 + 1e-12).all() and (p_dev > 0).all()
    best = np.array([r2.cpu().numpy()[off2[q]:off2[q + 1]].min() for q in range(len(q2))])
    assert np.array_equal(tensors["correct"].cpu().numpy(), best == 1)
    items.append((f"entropy metric {match}", np.array([m2["entropy"]]), np.array([ref[:, 3].mean()]), np.array([yard[:, 3].mean()])))
    items.append((f"confidence metric {match}", np.array([m2["confidence"]]), np.array([p_ref.mean()]), np.array([p_yard.mean()])))
    assert abs(m2["ece"] - mr.ece(p_dev, best == 1)) <= 1e-12, "ece of the device's own probabilities and ranks"
    _gate("evaluate temperature / predictive", items)


@pytest.mark.parametrize("match,loss", [("LBM", "info_nce_loss"), ("BIM", "bce_loss"), ("NTN-relu", "info_nce_loss")])
def test_infer_with_temperature(tmp_path, match, loss):
    from taxoexpan_amd.evaluate import infer
    ds = _toy(tmp_path)
    model = _model(match)
    rs = np.random.RandomState(5)
    names, vecs = [f"new_{i}" for i in range(9)], rs.standard_normal((9, 8)).astype(np.float32)
    T = 0.4
    beta = float(np.float32(1.0 / T))
    out0 = infer(model, ds, (names, vecs), _dev(), loss=loss, with_scores=True)
    out1 = infer(model, ds, (names, vecs), _dev(), loss=loss, with_scores=True, temperature=T)
    assert [(q, p, s) for q, p, s, _l in out1] == [(q, p, s) for q, p, s, _l in out0], "the parents and their scores do not depend on T"
    larger = loss.startswith("info_nce")
    anchors = list(ds.graph.nodes)
    where = {ds.vocab[a]: i for i, a in enumerate(anchors)}
    S, _hg, _qf = _toy_scores(model, ds, np.asarray(anchors, dtype=np.int64), torch.from_numpy(vecs).to(_dev()))
    t = mr.scaled(S, beta, larger)
    lse64, lse32 = mr.row_moments(S, beta, larger)[:, 0], _yard(S, beta, larger)[:, 0]
    got, want, yard = [], [], []
    for i, (_q, parents, _sc, lq) in enumerate(out1):
        cols = [where[v] for v in parents]
        got += lq
        want += (t[i, cols] - lse64[i]).tolist()
        yard += (t[i, cols].astype(np.float32) - lse32[i].astype(np.float32)).tolist()
    _gate("infer log_probs", [(f"log_probs {match} T {T}", np.array(got), np.array(want), np.array(yard))])
    assert all(v <= 1e-6 for v in got)                                       # probabilities


def test_fit_temperature_on_the_toy_taxonomy(tmp_path):
    """fit_temperature gets to fit_temperature_scores the way evaluate does: the fitted T lowers evaluate's own NLL on that split"""
    from taxoexpan_amd import calibrate
    from taxoexpan_amd.evaluate import evaluate
    ds = _toy(tmp_path, mode="validation")
    model = _model("LBM")
    c = calibrate.fit_temperature(model, ds, _dev())
    assert c.nll_after <= c.nll_before and c.temperature == 1.0 / c.beta
    before = evaluate(model, ds, _dev(), nll=True, temperature=1.0)[0]["nll"]
    after = evaluate(model, ds, _dev(), nll=True, temperature=c.temperature)[0]["nll"]
    print(f"[fit] toy LBM T {c.temperature!r} nll {c.nll_before!r} -> {c.nll_after!r} (evaluate: {before!r} -> {after!r}) iterations {c.iterations}")
    # evaluate(temperature=T) reports the fit's own objective (float64 on both sides, the per-query means summed in another order)
    assert abs(before - c.nll_before) <= 1e-12 * max(1.0, abs(before)) and abs(after - c.nll_after) <= 1e-12 * max(1.0, abs(after))
    assert model.training is False
