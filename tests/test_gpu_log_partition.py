"""The scoring loop's log-partition (the lse mode of gemm_tile_epilogue under gemm_kernel<true, true, V, V, -128>, gemm_nt_split_kernel<2, 3, 2, 3>
and ntn_score_kernel<V, true>; mlp_pair_kernel<3>; lse_merge_kernel) against an INDEPENDENT reference, entry point by entry point through
the C ABI -- the test owns every pitch, scratch buffer and workspace -- and scoring.log_partition_fused / evaluate(nll=True) /
infer(with_scores=True) on the toy taxonomy.

Reference: tests/log_partition_ref.py (plain numpy, float64; tests/test_log_partition_cpu.py holds the project's host code to it).
  (a) VALUES: lse of every row against the reference applied to the device's OWN materialised fp32 scores of the same route
      (txe_score_block / txe_mlp_score_block / txe_ntn_score_block), through golden_util.gate_against_f64 at its defaults; the yardstick is
      fp32 torch.logsumexp of those scores.  Every gate prints "[gate] op what device yardstick".  Both apply_exp values, both directions,
      the three routes of the bilinear form; NTN with k = 1, 4, 16; MLP with H = 5, 40 and flagged rows.
  (b) EXACT, no tolerance: G = 1 gives lse == z bit for bit; a row whose best score leads the rest by more than 110 gives lse == max; rows
      planted through operand rows with NaN, +Inf and -Inf give the reference's NaN / +Inf / -Inf pattern under each direction; rows >= nq
      and columns >= G (huge values planted there) contribute nothing; the same query in blocks of 50, in one block and at another row
      position gives equal bits; the three routes give equal bits wherever their scores do.
  (c) txe_lse_merge alone on pairs the test writes: (-Inf, 0) slots among real ones, all slots empty, no slot at all, more than a wave of
      pairs, NaN and +Inf parts.
NaN priming: part_max, part_sum, lse and sws start as NaN and the words behind their documented size keep that; a rejected call returns
its code, records no launch and leaves all of them primed.  Every call asserts the launch names its profiler recorded.

Measured on the MI355X (256 CUs), one run of the file: 60 cases in 5 s, the slowest 0.5 s.  Errors as fractions of the case's largest
|lse|: largest device error 2.1e-7; largest device / yardstick ratio 3.72 (2 candidates x 1 query under the exp on the bf16 pipe: 7.1e-8
against 1.9e-8), then 2.2 (the relu-NTN fallback: 1.3e-7 against 5.7e-8) and 1.65; all two orders below the gate's floor of 2e-5.
profiles/NOTES.md, "Log-partition of the scoring loop", has the table.
"""
import os
import shutil

import numpy as np
import pytest
import torch

import log_partition_ref as lp
import scoring_loop_ref as sl
from golden_util import GOLDEN_DIR
from test_gpu_readout_match_ops import _profiled
from test_gpu_scoring_loop_ops import GUARD, ROUTES, _gate, _Inputs, _L, _dev, _nan, _ok, _rc, _score_block, _st, _tail_intact

pytestmark = pytest.mark.gpu

#        G    nq    r  ld_q ld_u     every G of {1, 2, 63, 64, 65, 127, 128, 129, 257, 8201}, nq of {1, 7, 127, 129, 130}, r of {3, 32, 33};
CASES = [(1, 7, 3, 4, 4), (2, 1, 32, 32, 32), (63, 127, 33, 36, 36), (64, 129, 3, 3, 3), (65, 130, 32, 32, 36), (127, 7, 33, 33, 34),
         (128, 129, 32, 32, 32), (129, 127, 3, 4, 8), (257, 130, 33, 36, 36), (8201, 130, 32, 32, 32), (8201, 1, 3, 4, 4),
         (129, 7, 32, 32, 34), (129, 7, 32, 34, 32), (129, 7, 32, 34, 38)]
#        pitches: 16-byte rows (loader 4), 8-byte (2), odd (1), and the mixed pairs 4/2, 2/4, 2/2 -- every loader pair has an lse instance
#        of its own; 8201 = 65 tiles: more than a wave of pairs per row


def _inputs(G, nq, r, ld_q, ld_u, seed, exp):
    rs = np.random.RandomState(seed)
    Q = rs.standard_normal((nq, r)).astype(np.float32)
    U = rs.standard_normal((G, r)).astype(np.float32)
    if exp:
        Q *= np.float32(0.5 / np.sqrt(r))                   # raw scores of order 1/2: exp(raw) stays far from fp32's range under a second exp
    return Q, U


def _plain(Q, U, ld_q, ld_u):
    z = np.zeros(1, dtype=np.int64)
    return _Inputs(Q, U, np.zeros(Q.shape[0] + 1, dtype=np.int64), z[:0], ld_q, 0, ld_u, 0, sl.round_up(U.shape[0], 4) + 4, 0)


def _lse_names(I, route):
    sub = {"topk_merge_kernel": "lse_merge_kernel", sl.SPLIT_KERNEL: "gemm_nt_split_kernel<2, 3, 2, 3>"}
    return [sub.get(n, n.replace(", 128>", ", -128>") if n.startswith("gemm_kernel<") else n) for n in I.names("topk", route)]


def _lse_block(I, route, exp, larger, nq=None, G=None, qp=None):
    """txe_score_lse_block into primed scratch: lse fp32 [nq]; every word behind a buffer's documented size still NaN"""
    nq, G = I.nq if nq is None else nq, I.G if G is None else G
    tiles = _L().call("txe_score_topk_tiles", G)
    assert tiles == (G + 127) // 128
    pm, ps, out = _nan(nq * tiles + GUARD), _nan(nq * tiles + GUARD), _nan(nq + GUARD)
    sb, swp, swb, upk = I.sws(route, "topk")
    _r, names = _profiled(lambda: _ok("txe_score_lse_block", I.Qp if qp is None else qp, I.ld_q, nq, I.Up_, I.ld_u, G, I.r, int(exp), int(larger), pm.data_ptr(),
                                       ps.data_ptr(), out.data_ptr(), swp, swb, upk, _st()))
    if nq == I.nq and G == I.G:
        assert names == _lse_names(I, route), (names, _lse_names(I, route))
    for t, n in ((pm, nq * tiles), (ps, nq * tiles), (out, nq)):
        _tail_intact(t, n)
    assert not bool(torch.isnan(ps[:nq * tiles]).any()) or bool(torch.isnan(pm[:nq * tiles]).any()), "a NaN sum beside a real maximum"
    if sb is not None:
        _tail_intact(sb, swb // 4)
    return out.cpu().numpy()[:nq].copy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _z(S, larger):
    return S if larger else -S


def _yard(S, larger):
    return torch.logsumexp(torch.from_numpy(np.ascontiguousarray(_z(S, larger))), dim=1).numpy()


def _same_pattern(got, ref):
    """the NaN / +Inf / -Inf pattern of the reference, exactly; -> the mask of the finite rows"""
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf].astype(np.float32)), (got, ref)
    return np.isfinite(ref)


def _gate_rows(items, what, got, S, larger):
    ref = lp.row_lse(S, larger)
    fin = _same_pattern(got, ref)
    if fin.any():
        items.append((what, got[fin], ref[fin], _yard(S, larger)[fin]))


# ---- (a) + (b): the bilinear form -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exp", [0, 1])
@pytest.mark.parametrize("case", range(len(CASES)), ids=["x".join(map(str, c)) for c in CASES])
def test_bilinear_values_and_bits(case, exp):
    G, nq, r, ld_q, ld_u = CASES[case]
    Q, U = _inputs(G, nq, r, ld_q, ld_u, 10 + case, exp)
    I = _plain(Q, U, ld_q, ld_u)
    items, by_route = [], {}
    for route in ROUTES:
        S = _score_block(I, route, exp)
        for larger in (1, 0):
            got = _lse_block(I, route, exp, larger)
            _gate_rows(items, f"lse [{G}x{nq}x{r} {route} exp {exp} larger {larger}]", got, S, larger)
            if G == 1:
                assert np.array_equal(_bits(got), _bits(_z(S, larger)[:, 0])), "one candidate: lse is its z, bit for bit"
            by_route[route, larger] = (S, got)
    for larger in (1, 0):                                   # the same scores give the same lse on every route
        S0, g0 = by_route["mfma", larger]
        for route in ROUTES[1:]:
            S1, g1 = by_route[route, larger]
            same = (_bits(S0) == _bits(S1)).all(axis=1)
            assert np.array_equal(_bits(g0)[same], _bits(g1)[same]), route
        assert np.array_equal(_bits(by_route["split", larger][1]), _bits(by_route["packed", larger][1])), "planes packed per call / once"
    _gate("txe_score_lse_block", items)


@pytest.mark.parametrize("G,nq,r", [(257, 130, 32), (129, 7, 3)])
def test_bilinear_leader_special_values_and_padding(G, nq, r):
    """exact results: a leader more than 110 ahead; NaN / +Inf / -Inf planted through query rows; huge values planted in the rows behind
    nq and the candidates behind G"""
    rs = np.random.RandomState(G)
    Q = (rs.standard_normal((nq + 3, r)) * 0.5).astype(np.float32)
    U = (rs.standard_normal((G + 5, r)) * 0.5).astype(np.float32)
    Q[:, 0], Q[:, 1] = 1.0, 1.0
    U[:, 0] = rs.uniform(0.5, 1.5, size=G + 5).astype(np.float32)             # (positive: an infinite query entry there gives one sign)
    lead = [G // 2, G - 1]                                                   # one leader per direction, in different tiles
    U[lead[0], 1], U[lead[1], 1] = 200.0, -200.0
    Q[nq:], U[G:] = 1e30, 1e30                                               # the padding: never read as a query, never counted as a candidate
    special = nq >= 100
    if special:
        Q[3], Q[64], Q[65], Q[127] = np.nan, 0.0, 0.0, 0.0
        Q[64, 0], Q[65, 0], Q[127, 0], Q[127, 1] = np.inf, -np.inf, 1e38, 1e37    # all +Inf; all -Inf; finite but for the leaders' overflow
    I = _plain(Q, U, r + 4 if r % 4 == 0 else r, r)
    Iref = _plain(Q[:nq].copy(), U[:G].copy(), I.ld_q, I.ld_u)
    items = []
    for route in ROUTES:
        S = _score_block(Iref, route, 0)
        if route == "mfma" and special:
            assert np.isnan(S[3]).all() and (S[64] == np.inf).all() and (S[65] == -np.inf).all() and S[127, lead[0]] == np.inf and S[127, lead[1]] == -np.inf
        for larger in (1, 0):
            got = _lse_block(I, route, 0, larger, nq=nq, G=G)
            assert np.array_equal(_bits(got), _bits(_lse_block(Iref, route, 0, larger))), "rows >= nq or columns >= G leaked into the sums"
            z = _z(S, larger)
            ref = lp.row_lse(S, larger)
            _gate_rows(items, f"lse [{G}x{nq}x{r} {route} larger {larger}]", got, S, larger)
            top = np.sort(np.where(np.isnan(z), -np.inf, z), axis=1)
            with np.errstate(invalid="ignore"):
                led = np.isfinite(ref) & (top[:, -1] - top[:, -2] > 110)
            assert led.sum() >= nq - 8
            assert np.array_equal(_bits(got[led]), _bits(top[led, -1])), "a leader more than 110 ahead: lse is the maximum, bit for bit"
    _gate("txe_score_lse_block special", items)


def test_bilinear_purity_over_blocks_and_positions():
    """lse[q] is a function of row q's scores: the same queries in one block, in blocks of 50 and rolled to other row positions"""
    G, nq, r = 300, 130, 32
    Q, U = _inputs(G, nq, r, r, r, 5, 0)
    I = _plain(Q, U, r, r)
    for route in ROUTES:
        for larger in (1, 0):
            whole = _lse_block(I, route, 0, larger)
            parts = [_lse_block(I, route, 0, larger, nq=min(50, nq - q0), qp=I.Qp + 4 * q0 * I.ld_q) for q0 in range(0, nq, 50)]
            assert np.array_equal(_bits(whole), _bits(np.concatenate(parts))), (route, "blocks of 50")
            Ir = _plain(np.roll(Q, 37, axis=0), U, r, r)
            assert np.array_equal(_bits(whole), _bits(np.roll(_lse_block(Ir, route, 0, larger), -37))), (route, "row position")
            assert np.array_equal(_bits(whole), _bits(_lse_block(I, route, 0, larger))), (route, "run to run")


def test_rejected_calls_leave_everything_primed():
    G, nq, r = 129, 7, 32
    Q, U = _inputs(G, nq, r, r, r, 1, 0)
    I = _plain(Q, U, r, r)
    need = _L().call("txe_score_split_ws_bytes", nq, G, r)
    assert need > 16
    pm, ps, out, sws = _nan(nq * 2 + GUARD), _nan(nq * 2 + GUARD), _nan(nq + GUARD), _nan(need // 4)
    calls = [(-1, (I.Qp, I.ld_q, nq, I.Up_, I.ld_u, 0, r, 0, 1, pm.data_ptr(), ps.data_ptr(), out.data_ptr(), None, 0, None, _st())),
             (-1, (I.Qp, r - 1, nq, I.Up_, I.ld_u, G, r, 0, 1, pm.data_ptr(), ps.data_ptr(), out.data_ptr(), None, 0, None, _st())),
             (-1, (I.Qp, I.ld_q, nq, I.Up_, I.ld_u, G, r, 0, 1, pm.data_ptr(), None, out.data_ptr(), None, 0, None, _st())),
             (-3, (I.Qp, I.ld_q, nq, I.Up_, I.ld_u, G, r, 0, 1, pm.data_ptr(), ps.data_ptr(), out.data_ptr(), sws.data_ptr(), need - 16, None, _st())),
             (0, (I.Qp, I.ld_q, 0, I.Up_, I.ld_u, G, r, 0, 1, pm.data_ptr(), ps.data_ptr(), out.data_ptr(), None, 0, None, _st()))]
    for want, args in calls:
        rc, names = _profiled(lambda: _rc("txe_score_lse_block", *args))
        assert rc == want and names == [], (want, rc, names)
    rc, names = _profiled(lambda: _rc("txe_lse_merge", pm.data_ptr(), ps.data_ptr(), nq, -1, out.data_ptr(), _st()))
    assert rc == -1 and names == []
    for t in (pm, ps, out, sws):
        _tail_intact(t, 0)


# ---- (c) the merge alone ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cnt", [0, 1, 3, 64, 65, 200])
def test_lse_merge_alone(cnt):
    nq = 9
    rs = np.random.RandomState(cnt)
    pm = (rs.standard_normal((nq, cnt)) * 20).astype(np.float32)
    ps = rs.uniform(1.0, 128.0, size=(nq, cnt)).astype(np.float32)
    if cnt:
        pm[1, :], ps[1, :] = -np.inf, 0.0                                    # every slot empty
        pm[2, ::2], ps[2, ::2] = -np.inf, 0.0                                # empty slots among real ones
        pm[3, cnt // 2] = np.nan
        pm[4, cnt - 1] = np.inf
        pm[5, cnt - 1], pm[5, 0] = np.inf, np.nan                            # NaN wins over +Inf
        pm[6, :], ps[6, :] = -300.0, 1.0
        pm[6, 0] = 7.25                                                      # a leader: the rest vanish beside it
        ps[7, :] = 1.0
    want = lp.merge_pairs(pm, ps)
    out = _nan(nq + GUARD)
    pmd, psd = _nan(nq * cnt + GUARD), _nan(nq * cnt + GUARD)
    pmd[:nq * cnt].copy_(torch.from_numpy(pm.reshape(-1)))
    psd[:nq * cnt].copy_(torch.from_numpy(ps.reshape(-1)))
    _r, names = _profiled(lambda: _ok("txe_lse_merge", pmd.data_ptr(), psd.data_ptr(), nq, cnt, out.data_ptr(), _st()))
    assert names == ["lse_merge_kernel"]
    _tail_intact(out, nq)
    got = out.cpu().numpy()[:nq]
    fin = _same_pattern(got, want)
    if cnt == 0:
        assert (got == -np.inf).all()
        return
    assert np.isneginf(got[1]) and np.isnan(got[3]) and got[4] == np.inf and np.isnan(got[5]) and _bits(got[6:7])[0] == _bits(np.float32(7.25))
    if cnt == 1:
        assert np.array_equal(_bits(got[7:8]), _bits(pm[7, :1])), "one pair with a sum of 1: its maximum, bit for bit"
    # float64 of the given pairs, rounded once: the device's double arithmetic differs from it by the rounding of log alone
    err = np.abs(got[fin].astype(np.float64) - want[fin])
    assert (err <= np.abs(want[fin]) * 2.0 ** -23 + 1e-7).all(), (got, want)


# ---- NTN and MLP ---------------------------------------------------------------------------------------------------------------------------------
def _primed_call(name, head, larger, nq, G, want_names):
    tiles = (G + 127) // 128
    pm, ps, out = _nan(nq * tiles + GUARD), _nan(nq * tiles + GUARD), _nan(nq + GUARD)
    _r, names = _profiled(lambda: _ok(name, *head, int(larger), pm.data_ptr(), ps.data_ptr(), out.data_ptr(), _st()))
    assert names == want_names, names
    for t, n in ((pm, nq * tiles), (ps, nq * tiles), (out, nq)):
        _tail_intact(t, n)
    return out.cpu().numpy()[:nq].copy()


@pytest.mark.parametrize("G,nq,l,r,k", [(129, 7, 5, 9, 1), (257, 130, 17, 12, 4), (8201, 7, 8, 33, 4), (300, 129, 16, 32, 16), (1, 1, 3, 3, 4)])
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
    items = []
    for larger in (1, 0):
        got = _primed_call("txe_ntn_score_lse_block", head, larger, nq, G, ["ntn_score_kernel[lse]", "lse_merge_kernel"])
        _gate_rows(items, f"ntn lse [{G}x{nq}x{r} k {k} larger {larger}]", got, S, larger)
        if G == 1:
            assert np.array_equal(_bits(got), _bits(_z(S, larger)[:, 0]))
        sub = ops.NTNQueries(qp.Qp[nq // 2:], qp.c[:, nq // 2:], nq - nq // 2)                       # the second half as a block of its own
        half = _primed_call("txe_ntn_score_lse_block", ops._ntn_args(sub, prep), larger, sub.n, G, ["ntn_score_kernel[lse]", "lse_merge_kernel"])
        assert np.array_equal(_bits(half), _bits(got[nq // 2:])), "a row's lse depends on the block it is in"
    _gate("txe_ntn_score_lse_block", items)


@pytest.mark.parametrize("G,nq,H,r", [(129, 7, 5, 9), (257, 130, 40, 12), (300, 127, 40, 12), (8201, 65, 5, 3), (1, 1, 40, 8)])
def test_mlp_values_and_bits_with_flagged_rows(G, nq, H, r):
    from taxoexpan_amd import ops
    from taxoexpan_amd.model_zoo import MLP
    l = 6
    torch.manual_seed(G + H)
    m = MLP(l, r, H).to(_dev())
    hg, q = torch.randn(G, l, device=_dev()) * 3, torch.randn(nq, r, device=_dev()) * 3
    if G > 100:
        hg[G // 3] = 1e37                                                    # a flagged candidate row (the literal per-pair formula): huge,
    if G == 257:
        hg[G - 2, 0] = float("inf")                                          # ... and one that gives +-Inf / NaN scores down its column
    if nq == 130:
        q[5] = -2e37                                                         # flagged query rows
        q[129, 1] = float("nan")
    prep = ops.mlp_project(hg, m)
    qp = ops.mlp_prepare_queries(q, prep)
    if G > 100:
        assert int(prep.flags.sum()) == (2 if G == 257 else 1) and (nq != 130 or int(qp.flags.sum()) == 2)
    head = ops._mlp_args(qp, prep)
    S = ops.mlp_score_block(qp, prep).cpu().numpy()
    items = []
    for larger in (1, 0):
        got = _primed_call("txe_mlp_score_lse_block", head, larger, nq, G, ["mlp_pair_kernel[lse]", "lse_merge_kernel"])
        _gate_rows(items, f"mlp lse [{G}x{nq} H {H} larger {larger}]", got, S, larger)
        if G == 1:
            assert np.array_equal(_bits(got), _bits(_z(S, larger)[:, 0]))
        if nq == 130:
            assert np.isnan(got[129])
    _gate("txe_mlp_score_lse_block", items)


# ---- module level: the toy taxonomy ------------------------------------------------------------------------------------------------------------
def _toy(tmp_path):
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    for fn in os.listdir(os.path.join(GOLDEN_DIR, "toy_taxo")):
        shutil.copy(os.path.join(GOLDEN_DIR, "toy_taxo", fn), tmp_path)
    return MaskedGraphDataset(MAGDataset("toy", str(tmp_path), raw=True), mode="test", sampling_mode=0, expand_factor=100, normalize_embed=True)


def _model(match):
    """the PGAT+WMR toy model; "NTN" / "NTN-relu": an NTN (k = 4; tanh, or relu -- no fused route: scored by calling the module) in the
    place of an LBM module, as tests/test_gpu_ntn_scoring.py builds it"""
    from taxoexpan_amd import TaxoExpan, model_zoo
    torch.manual_seed(11)
    ntn = match.startswith("NTN")
    model = TaxoExpan("PGAT", "WMR", "LBM" if ntn else match, in_dim=8, hidden_dim=6, out_dim=5, pos_dim=3, num_layers=1, heads=[2, 1], feat_drop=0.1,
                      attn_drop=0.1, hidden_drop=0.1, out_drop=0.1)
    if ntn:
        l, r = model.match.W.weight.shape[-2:]
        model.match = model_zoo.NTN(l, r, k=4, non_linear=torch.relu if match == "NTN-relu" else torch.tanh)
    return model.to(_dev()).eval()


@pytest.mark.parametrize("match", ["LBM", "BIM", "MLP", "NTN", "NTN-relu"])
def test_log_partition_fused_on_the_toy_taxonomy(tmp_path, match):
    from taxoexpan_amd import scoring
    from taxoexpan_amd.evaluate import _score_blocks, candidate_graphs
    ds = _toy(tmp_path)
    model = _model(match)
    assert scoring.fused_matcher_ok(model.match) == (match != "NTN-relu")
    cand = sorted(ds.all_positions)
    with torch.no_grad():
        hg = scoring.encode_candidates(model, candidate_graphs(ds.device_taxonomy(_dev()), cand, ds.expand_factor, 0))
        qf = ds.node_features[torch.as_tensor(list(ds.node_list), dtype=torch.long)].to(_dev())
        if match == "NTN-relu":
            S = torch.cat([s for _q0, s in _score_blocks(model, hg, qf, 1024)])
        else:
            S = scoring.score_all(model.match, hg, qf)
        items = []
        for larger in (True, False):
            got = scoring.log_partition_fused(model.match, hg, qf, larger)
            assert got.dtype == torch.float32 and got.shape == (qf.shape[0],) and got.device == hg.device
            want = scoring.host_log_partition(S, larger)
            assert np.isfinite(want).all()
            items.append((f"{match} larger {larger}", got.cpu().numpy(), want, _yard(S.cpu().numpy(), larger)))
            blocked = scoring.log_partition_fused(model.match, hg, qf, larger, block=3)
            if match != "NTN-relu":
                assert torch.equal(blocked, got), "blocks of 3 queries"
    _gate("log_partition_fused", items)


@pytest.mark.parametrize("match,larger", [("LBM", True), ("BIM", False), ("MLP", True), ("NTN", True)])
def test_evaluate_nll(tmp_path, match, larger):
    from taxoexpan_amd import scoring
    from taxoexpan_amd.evaluate import candidate_graphs, evaluate
    ds = _toy(tmp_path)
    model = _model(match)
    m0, r0, off0, q0 = evaluate(model, ds, _dev(), larger_is_better=larger)
    m1, r1, off1, q1 = evaluate(model, ds, _dev(), larger_is_better=larger, nll=True)
    assert "nll" not in m0 and {k: v for k, v in m1.items() if k != "nll"} == m0 and set(m1) == set(m0) | {"nll"}
    assert torch.equal(r0, r1) and np.array_equal(off0, off1) and q0 == q1
    cand = sorted(ds.all_positions)
    index = {a: i for i, a in enumerate(cand)}
    with torch.no_grad():
        hg = scoring.encode_candidates(model, candidate_graphs(ds.device_taxonomy(_dev()), cand, ds.expand_factor, 0))
        S = scoring.score_all(model.match, hg, ds.node_features[torch.as_tensor(q1, dtype=torch.long)].to(_dev())).cpu().numpy()
    z = _z(S, larger)
    pos = [i for q in q1 for i in (index[a] for a in ds.node2parents[q] if a in index)]
    rows = np.repeat(np.arange(len(q1)), np.diff(off1))
    want = lp.nll(lp.row_lse(S, larger), z[rows, pos], off1)
    yard = lp.nll(_yard(S, larger), z[rows, pos], off1)
    print(f"[nll] {match} device {m1['nll']!r} float64 {want!r} fp32 yardstick {yard!r}")
    _gate("evaluate nll", [(f"nll {match}", np.array([m1["nll"]]), np.array([want]), np.array([yard]))])


@pytest.mark.parametrize("match,loss", [("LBM", "info_nce_loss"), ("BIM", "bce_loss"), ("NTN-relu", "info_nce_loss")])
def test_infer_with_scores(tmp_path, match, loss):
    from taxoexpan_amd import scoring
    from taxoexpan_amd.evaluate import _score_blocks, candidate_graphs, infer
    ds = _toy(tmp_path)
    model = _model(match)
    rs = np.random.RandomState(5)
    names, vecs = [f"new_{i}" for i in range(9)], rs.standard_normal((9, 8)).astype(np.float32)
    plain, rich = tmp_path / "plain.tsv", tmp_path / "rich.tsv"
    out0 = infer(model, ds, (names, vecs), _dev(), loss=loss, save=str(plain))
    out1 = infer(model, ds, (names, vecs), _dev(), loss=loss, save=str(rich), with_scores=True)
    assert [(q, p) for q, p, _s, _l in out1] == out0 and all(len(s) == len(p) == len(lq) == 5 for _q, p, s, lq in out1)
    lines = open(plain).read().splitlines()
    assert lines[0] == "Query\tPredicted parents" and lines[1:] == [f"{q}\t{', '.join(p)}" for q, p in out0]
    rl = open(rich).read().splitlines()
    assert rl[0] == "Query\tPredicted parents\tScores\tLog-probabilities" and len(rl) == 10
    q, p, s, lq = out1[0]
    assert rl[1] == f"{q}\t{', '.join(p)}\t{', '.join('%.6g' % v for v in s)}\t{', '.join('%.6g' % v for v in lq)}"
    larger = loss.startswith("info_nce")
    anchors = list(ds.graph.nodes)
    where = {ds.vocab[a]: i for i, a in enumerate(anchors)}
    with torch.no_grad():
        hg = scoring.encode_candidates(model, candidate_graphs(ds.device_taxonomy(_dev()), np.asarray(anchors, dtype=np.int64), ds.expand_factor, 0))
        qf = torch.from_numpy(vecs).to(_dev())
        if match == "NTN-relu":
            S = torch.cat([b for _q0, b in _score_blocks(model, hg, qf, 1024)]).cpu().numpy()
        else:
            S = scoring.score_all(model.match, hg, qf).cpu().numpy()
    lse64, lse32 = lp.row_lse(S, larger), _yard(S, larger)
    got, want, yard = [], [], []
    for i, (_q, parents, sc, lq) in enumerate(out1):
        cols = [where[v] for v in parents]
        assert np.array_equal(_bits(np.asarray(sc, dtype=np.float32)), _bits(S[i, cols])), "the scores are score_all's entries, bit for bit"
        got += lq
        want += (_z(S, larger)[i, cols].astype(np.float64) - lse64[i]).tolist()
        yard += (_z(S, larger)[i, cols] - lse32[i]).tolist()
    _gate("infer log_probs", [(f"log_probs {match}", np.array(got), np.array(want), np.array(yard))])
    assert all(v <= 1e-6 for v in got)                                       # probabilities
