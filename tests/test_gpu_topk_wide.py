"""GPU: the fused all-candidate best-k for 9 <= k <= 64 -- rounds of 8 under a ceiling (csrc/txe_common.h; scoring.host_topk_rounds
states them).  The raw entry points (txe_score_topk_wide_block, txe_mlp_score_topk_wide_block, txe_ntn_score_topk_wide_block,
txe_topk_merge_wide) against tests/scoring_loop_ref.topk on the scores the same kernels materialise, keys bit for bit; k <= 8 bit-equal
to the k <= 8 siblings; the edge rows of the rounds; both score routes; ragged query blocks; the merge of candidate shards, by hand and
in a world of 2; rejected calls; and infer() / evaluate(case=) end to end on the toy taxonomy, on the fused rounds and on the score
block + select route.  Every comparison is exact."""
import os
import shutil

import numpy as np
import pytest
import torch

import scoring_loop_ref as sl
from golden_util import GOLDEN_DIR
from test_gpu_readout_match_ops import _profiled
from test_gpu_scoring_loop_ops import NANI, _Inputs, _L, _nan, _nani, _ok, _ptr, _rc, _score_block, _st, _tail_intact, _topk

pytestmark = pytest.mark.gpu

KS = (9, 16, 17, 24, 63, 64)
NQS, GS = (5, 130), (10, 129, 300, 1000)       # below / across one 128-row tile; below, just over one, three and eight 128-column tiles
COMBOS = ((0, True, 0), (0, False, 77), (1, True, 77), (1, False, 0))       # (apply_exp, larger_is_better, idx_base)
ROUND = "topk_merge_round_kernel"


def _dev():
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _key32(S, larger):
    """the selection keys of fp32 scores, as fp32: the score, negated when smaller is better, NaN as -inf"""
    key = np.array(S if larger else -S, dtype=np.float32)
    key[np.isnan(key)] = -np.inf
    return key


def _check(S, larger, k, base, oi, okey, what):
    """indices == scoring_loop_ref.topk on the materialised scores S; keys == S's own keys at the chosen columns, bit for bit (-inf
    behind a row's last entry)"""
    wi, _wk = sl.topk(S, k, larger, idx_base=base)
    assert np.array_equal(oi, wi), what
    if okey is not None:
        key = _key32(S, larger)
        want = np.full(oi.shape, -np.inf, dtype=np.float32)
        q, t = np.nonzero(wi >= 0)
        want[q, t] = key[q, wi[q, t] - base]
        assert np.array_equal(_bits(okey), _bits(want)), what


def _plain_inputs(Q, U, ld_q=None, ld_u=None):
    nq, r = Q.shape
    return _Inputs(Q, U, np.zeros(nq + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), ld_q or r, 0, ld_u or r, 0, (U.shape[0] + 3) // 4 * 4, 0)


def _wide_names(I, route, k):
    base = I.names("topk", route)                  # [split_pack_kernel ...] + [the score kernel, "topk_merge_kernel"]
    return base[:-2] + [base[-2], ROUND] * ((k + 7) // 8)


def _wide(I, route, exp, larger, k, idx_base, with_key=True):
    """txe_score_topk_wide_block into primed buffers: the launches it records, nothing written behind a documented size"""
    nq, tiles, kr = I.nq, sl.topk_tiles(I.G), min(k, 8)
    pk, pi, fl, ceil = _nan(nq * tiles * kr + 8), _nani(nq * tiles * kr + 8), _nani(nq + 8), _nani(2 * nq + 8)
    oi, okey = _nani(nq * k + 8), (_nan(nq * k + 8) if with_key else None)
    sb, swp, swb, upk = I.sws(route, "topk")
    _r, names = _profiled(lambda: _ok("txe_score_topk_wide_block", I.Qp, I.ld_q, nq, I.Up_, I.ld_u, I.G, I.r, int(exp), int(larger), k, idx_base,
                                       pk.data_ptr(), pi.data_ptr(), fl.data_ptr(), oi.data_ptr(), _ptr(okey), swp, swb, upk, ceil.data_ptr(), _st()))
    assert names == _wide_names(I, route, k), (names, _wide_names(I, route, k))
    for t, n in ((pk, nq * tiles * kr), (pi, nq * tiles * kr), (fl, nq), (ceil, 2 * nq), (oi, nq * k)) + (((okey, nq * k),) if with_key else ()):
        _tail_intact(t, n)
    if sb is not None:
        _tail_intact(sb, swb // 4)
    return oi.cpu().numpy()[:nq * k].reshape(nq, k).astype(np.int64), (okey.cpu().numpy()[:nq * k].reshape(nq, k) if with_key else None)


# ---- BIM / LBM: txe_score_topk_wide_block ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["mfma", "packed"])
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("nq", NQS)
def test_bilinear_wide_block(nq, G, route):
    """r = 12, exact inputs (scoring_loop_ref.exact_inputs: duplicated candidate rows, so exact ties within and across tiles): every k of KS,
    exp off and on, both directions, idx_base 0 and 77; exp off the materialised scores are the float64 ones exactly"""
    r = 12
    for exp in (0, 1):
        Q, U = sl.exact_inputs(nq, G, r, 100 * nq + G + exp, thin=bool(exp))
        I = _plain_inputs(Q, U)
        S = _score_block(I, route, exp)
        if not exp:
            assert np.array_equal(S, sl.scores64(Q, U, False).astype(np.float32))
        for e, larger, base in COMBOS:
            if e != exp:
                continue
            for k in KS:
                oi, okey = _wide(I, route, exp, larger, k, base, with_key=(k != 17))
                _check(S, larger, k, base, oi, okey, (nq, G, route, exp, larger, k, base))


def test_bilinear_wide_block_padded_r_250():
    """r = 256 on a zero-padded pitch (250 columns of data), the bf16 pipe packing per call"""
    nq, G, r = 130, 300, 256
    Q, U = sl.exact_inputs(nq, G, r, 9, zero_from=250)
    I = _plain_inputs(Q, U)
    for route in ("split", "mfma"):
        S = _score_block(I, route, 0)
        assert np.array_equal(S, sl.scores64(Q, U, False).astype(np.float32))
        for larger, k, base in ((True, 24, 0), (False, 63, 77)):
            oi, okey = _wide(I, route, 0, larger, k, base)
            _check(S, larger, k, base, oi, okey, (route, larger, k))


@pytest.mark.parametrize("route", ["mfma", "split", "packed"])
def test_wide_entry_is_bit_equal_to_the_sibling_for_k_up_to_8(route):
    nq, G, r = 130, 300, 12
    Q, U = sl.exact_inputs(nq, G, r, 3, special=True)
    I = _plain_inputs(Q, U)
    for k in (1, 5, 8):
        for larger in (True, False):
            a_i, a_k = _topk(I, route, 0, larger, k, 77)
            b_i, b_k = _wide(I, route, 0, larger, k, 77)
            assert np.array_equal(a_i, b_i) and np.array_equal(_bits(a_k), _bits(b_k)), (route, k, larger)


# ---- edge rows ------------------------------------------------------------------------------------------------------------------------
def _first_column_inputs(nq, col0, r=12, scale=None):
    """queries (s_q, 0, ..., 0) against candidates whose first column is col0: score[q][g] = s_q * col0[g] exactly on either route (small
    integers are exact on the bf16 pipe; the other products are 0 * finite)"""
    G = len(col0)
    rs = np.random.RandomState(G)
    U = rs.randint(-16, 17, size=(G, r)).astype(np.float32) / 4
    U[:, 0] = col0
    Q = np.zeros((nq, r), dtype=np.float32)
    Q[:, 0] = scale if scale is not None else np.array([1, 2, -1, 1, -2] * nq, dtype=np.float32)[:nq]
    return Q, U


@pytest.mark.parametrize("route", ["mfma", "packed"])
def test_every_candidate_equal(route):
    """every candidate row identical (G = 1000, eight column tiles): columns 0 .. k-1 in order, whatever the floors did in between"""
    nq, G, r = 5, 1000, 12
    Q, U = sl.exact_inputs(nq, G, r, 1)
    U[:] = U[0]
    I = _plain_inputs(Q, U)
    for larger, k, base in ((True, 9, 0), (False, 24, 77), (True, 64, 77)):
        oi, okey = _wide(I, route, 0, larger, k, base)
        assert np.array_equal(oi, np.tile(np.arange(k) + base, (nq, 1))), (larger, k)
        assert np.array_equal(_bits(okey), _bits(np.repeat(_key32(sl.scores64(Q, U[:1], False).astype(np.float32), larger), k, 1)))


@pytest.mark.parametrize("route", ["mfma", "packed"])
def test_equal_keys_straddle_the_round_boundaries(route):
    """6 leaders, 5 candidates tied at places 7..11 (across the first round's end), 3 more, 4 tied at places 15..18 (across the second's),
    the tied rows spread over three column tiles; the rest small integers with many ties"""
    G, nq = 300, 5
    rs = np.random.RandomState(2)
    col0 = rs.randint(-50, 51, size=G).astype(np.float32)
    where = rs.choice(G, 18, replace=False)
    col0[where] = np.array([200 - i for i in range(6)] + [150] * 5 + [140, 139, 138] + [100] * 4, dtype=np.float32)
    Q, U = _first_column_inputs(nq, col0)
    I = _plain_inputs(Q, U)
    S = _score_block(I, route, 0)
    assert np.array_equal(S, Q[:, :1] * col0[None, :])
    for larger in (True, False):
        for k in (9, 16, 17, 24):
            oi, okey = _wide(I, route, 0, larger, k, 0)
            _check(S, larger, k, 0, oi, okey, (route, larger, k))
    oi, _ = _wide(I, route, 0, True, 24, 0)
    assert oi[0, 6:11].tolist() == sorted(where[6:11].tolist()) and oi[0, 14:18].tolist() == sorted(where[14:18].tolist())
    assert {int(c) for c in where[6:11]} != {int(c) for c in where[6:11] if c < 128}          # (not all in one tile)


@pytest.mark.parametrize("route", ["mfma", "packed"])
def test_more_than_8_nan_and_more_than_8_inf_scores(route):
    """LBM (exp on): 12 raw scores of 100 overflow to +inf, 11 candidate rows are NaN, 17 are finite -- a whole round of equal infinite
    keys, k reaching into the NaNs (last, in column order) and past the row's end (-1 / -inf)"""
    G, nq = 40, 5
    rs = np.random.RandomState(3)
    col0 = rs.randint(-3, 4, size=G).astype(np.float32)
    perm = rs.permutation(G)
    col0[perm[:12]] = 100.0
    Q, U = _first_column_inputs(nq, col0, scale=np.ones(nq, dtype=np.float32))
    U[perm[12:23]] = np.nan
    I = _plain_inputs(Q, U)
    S = _score_block(I, route, 1)
    assert int(np.isposinf(S[0]).sum()) == 12 and int(np.isnan(S[0]).sum()) == 11
    for larger in (True, False):
        for k in (9, 16, 24, 63, 64):
            oi, okey = _wide(I, route, 1, larger, k, 77)
            _check(S, larger, k, 77, oi, okey, (route, larger, k))
    oi, _ = _wide(I, route, 1, True, 63, 0)
    assert oi[0, :12].tolist() == sorted(perm[:12].tolist()) and oi[0, 29:40].tolist() == sorted(perm[12:23].tolist()) and (oi[0, 40:] == -1).all()


# ---- MLP and NTN: their own materialised scores ----------------------------------------------------------------------------------------------
def _generic(nq, G, l, r, seed):
    gen = torch.Generator().manual_seed(seed)
    hg = torch.randn(G, l, generator=gen)
    for _ in range(G // 4):                                   # duplicated candidate rows: exact ties, within and across tiles
        s, d = torch.randint(0, G, (2,), generator=gen).tolist()
        hg[d] = hg[s]
    return hg.to(_dev()), torch.randn(nq, r, generator=gen).to(_dev())


def _matcher_wide(name, args, nq, G, larger, k, base, names_kernel):
    tiles, kr = sl.topk_tiles(G), min(k, 8)
    pk, pi, fl, ceil = _nan(nq * tiles * kr + 8), _nani(nq * tiles * kr + 8), _nani(nq + 8), _nani(2 * nq + 8)
    oi, okey = _nani(nq * k + 8), _nan(nq * k + 8)
    _r, names = _profiled(lambda: _ok(name, *args, int(larger), k, base, pk.data_ptr(), pi.data_ptr(), fl.data_ptr(), oi.data_ptr(), okey.data_ptr(),
                                       ceil.data_ptr(), _st()))
    assert names == [names_kernel, ROUND] * ((k + 7) // 8), names
    for t, n in ((pk, nq * tiles * kr), (pi, nq * tiles * kr), (fl, nq), (ceil, 2 * nq), (oi, nq * k), (okey, nq * k)):
        _tail_intact(t, n)
    return oi.cpu().numpy()[:nq * k].reshape(nq, k).astype(np.int64), okey.cpu().numpy()[:nq * k].reshape(nq, k)


def _matcher_sibling(name, args, nq, G, larger, k, base):
    tiles = sl.topk_tiles(G)
    pk, pi, fl = _nan(nq * tiles * k + 8), _nani(nq * tiles * k + 8), _nani(nq + 8)
    oi, okey = _nani(nq * k + 8), _nan(nq * k + 8)
    _ok(name, *args, int(larger), k, base, pk.data_ptr(), pi.data_ptr(), fl.data_ptr(), oi.data_ptr(), okey.data_ptr(), _st())
    torch.cuda.synchronize()
    return oi.cpu().numpy()[:nq * k].reshape(nq, k).astype(np.int64), okey.cpu().numpy()[:nq * k].reshape(nq, k)


def _matcher_grid(nq, G, wide, sibling, args, S, kernel):
    for larger, base in ((True, 0), (False, 77)):
        for k in KS:
            oi, okey = _matcher_wide(wide, args, nq, G, larger, k, base, kernel)
            _check(S, larger, k, base, oi, okey, (wide, nq, G, larger, k))
    for k in (1, 5, 8):
        a_i, a_k = _matcher_sibling(sibling, args, nq, G, True, k, 77)
        b_i, b_k = _matcher_wide(wide, args, nq, G, True, k, 77, kernel)
        assert np.array_equal(a_i, b_i) and np.array_equal(_bits(a_k), _bits(b_k)), (wide, k)


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("nq", NQS)
def test_mlp_wide_block(nq, G):
    from taxoexpan_amd import ops
    from taxoexpan_amd.model_zoo import MLP
    l, r, H = 20, 12, 37
    torch.manual_seed(3)
    m = MLP(l, r, H).to(_dev())
    hg, q = _generic(nq, G, l, r, 10 * G + nq)
    with torch.no_grad():
        prep = ops.mlp_project(hg, m)
        qp = ops.mlp_prepare_queries(q, prep)
        S = ops.mlp_score_block(qp, prep).cpu().numpy()
        _matcher_grid(nq, G, "txe_mlp_score_topk_wide_block", "txe_mlp_score_topk_block", ops._mlp_args(qp, prep), S, "mlp_pair_kernel[topk]")


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("nq", NQS)
def test_ntn_wide_block(nq, G):
    from taxoexpan_amd import ops
    from taxoexpan_amd.model_zoo import NTN
    l, r = 10, 12
    torch.manual_seed(4)
    m = NTN(l, r, k=4).to(_dev())
    hg, q = _generic(nq, G, l, r, 10 * G + nq + 1)
    with torch.no_grad():
        prep = ops.ntn_project(hg, m)
        qp = ops.ntn_prepare_queries(q, prep)
        S = ops.ntn_score_block(qp, prep).cpu().numpy()
        _matcher_grid(nq, G, "txe_ntn_score_topk_wide_block", "txe_ntn_score_topk_block", ops._ntn_args(qp, prep), S, "ntn_score_kernel[topk]")


# ---- the merge alone, routes, blocks, shards -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cnt,nq", [(0, 1), (7, 5), (64, 5), (257, 5), (1000, 1)])
def test_topk_merge_wide_alone(cnt, nq):
    """txe_topk_merge_wide on lists the test writes (test_topk_merge_alone's: ties, +-inf, NaN keys, signed zeros, real -inf keys beside
    empty slots, short and empty rows) against scoring_loop_ref.merge; k <= 8 bit-equal to txe_topk_merge"""
    rs = np.random.RandomState(cnt + nq)
    keys = (np.round(rs.randn(nq, cnt) * 2) / 2).astype(np.float32)
    idx = np.stack([rs.permutation(max(4 * cnt, 1))[:cnt] for _ in range(nq)]).astype(np.int32).reshape(nq, cnt)
    for q in range(nq):
        for v in (np.nan, np.inf, -np.inf, -np.inf, -0.0, 0.0)[:cnt]:
            keys[q, rs.randint(0, cnt)] = v
        real = [cnt, 3, 0, cnt // 2, 1][q % 5]
        empty = rs.permutation(cnt)[:max(cnt - real, 0)]
        idx[q, empty], keys[q, empty[::2]] = sl.INT_MAX, np.nan
    kd = torch.from_numpy(keys).to(_dev()) if cnt else _nan(1)
    idd = torch.from_numpy(idx).to(_dev()) if cnt else _nani(1)
    for k in (1, 8, 9, 16, 17, 24, 63, 64):
        for base, with_key in ((0, True), (7, False)):
            oi, okey, ceil = _nani(nq * k + 8), (_nan(nq * k + 8) if with_key else None), _nani(2 * nq + 8)
            _r, names = _profiled(lambda: _ok("txe_topk_merge_wide", kd.data_ptr(), idd.data_ptr(), nq, cnt, k, base, oi.data_ptr(), _ptr(okey),
                                               ceil.data_ptr(), _st()))
            assert names == [ROUND] * ((k + 7) // 8)
            wi, wk = sl.merge(keys, idx, k, base)
            _tail_intact(oi, nq * k)
            _tail_intact(ceil, 2 * nq)
            assert np.array_equal(oi.cpu().numpy()[:nq * k].reshape(nq, k), wi), (cnt, nq, k, base)
            if with_key:
                _tail_intact(okey, nq * k)
                assert np.array_equal(okey.cpu().numpy()[:nq * k].reshape(nq, k).astype(np.float64), wk), (cnt, nq, k, base)
            if k <= 8 and with_key:
                o2, k2 = _nani(nq * k), _nan(nq * k)
                _ok("txe_topk_merge", kd.data_ptr(), idd.data_ptr(), nq, cnt, k, base, o2.data_ptr(), k2.data_ptr(), _st())
                torch.cuda.synchronize()
                assert torch.equal(o2[:nq * k], oi[:nq * k]) and torch.equal(k2[:nq * k].view(torch.int32), okey[:nq * k].view(torch.int32))


def test_both_score_routes_select_the_same(monkeypatch):
    """ops.score_topk_block(k = 16 / 64) with ops._NO_SPLIT_GEMM set and unset (the fp32 MFMA, the bf16 pipe): exact inputs, so the
    scores and hence the selections are the same -- and the float64 reference's"""
    from taxoexpan_amd import ops
    nq, G, r = 130, 1000, 12
    Q, U = sl.exact_inputs(nq, G, r, 21)
    Qd, Ud = torch.from_numpy(Q).to(_dev()), torch.from_numpy(U).to(_dev())
    for larger in (True, False):
        for k in (16, 64):
            got = []
            for no_split in (True, False):
                monkeypatch.setattr(ops, "_NO_SPLIT_GEMM", no_split)
                got.append(ops.score_topk_block(Qd, Ud, False, k, larger, idx_base=5))
            assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), (larger, k)
            wi, wk = sl.topk(sl.scores64(Q, U, False), k, larger, idx_base=5)
            assert np.array_equal(got[0][0].cpu().numpy(), wi) and np.array_equal(got[0][1].cpu().numpy().astype(np.float64), wk)


def _lbm(l, r, seed=5):
    from taxoexpan_amd import model_zoo as mz
    torch.manual_seed(seed)
    return mz.LBM(l, r).to(_dev())


def test_ragged_query_blocks_change_nothing():
    """topk_parents_fused(k = 16, block = 7) == block = None, and both == topk_parents on the materialised scores"""
    from taxoexpan_amd.scoring import score_all, topk_parents, topk_parents_fused
    G, Q, l, r = 300, 40, 24, 12
    hg, q = _generic(Q, G, l, r, 8)
    hg, q = hg * 0.3, torch.nn.functional.normalize(q, dim=1)          # (scores that stay finite under LBM's exp)
    m = _lbm(l, r)
    ids = torch.arange(G, device=_dev()) * 3 + 1
    with torch.no_grad():
        S = score_all(m, hg, q)
        for larger in (True, False):
            a = topk_parents_fused(m, hg, q, ids, 16, larger, block=7, return_scores=True)
            b = topk_parents_fused(m, hg, q, ids, 16, larger, block=None, return_scores=True)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            want = topk_parents(S, torch.arange(G, device=_dev()), 16, larger)
            assert torch.equal(a[0], ids[want]) and torch.equal(a[1], torch.gather(S, 1, want))


def test_three_uneven_shards_merge_to_the_unsharded_selection():
    """candidates split by hand into shards of 100 / 550 / 350 rows: each shard's best 24 (idx_base = its first row), concatenated and
    merged by ops.topk_merge(k = 24) == the unsharded selection == topk_parents on the materialised scores"""
    from taxoexpan_amd import ops
    from taxoexpan_amd.scoring import topk_parents, topk_parents_fused
    G, Q, l, r, k = 1000, 70, 40, 25, 24
    hg, q = _generic(Q, G, l, r, 12)
    hg, q = hg * 0.3, torch.nn.functional.normalize(q, dim=1)
    hg[G // 2:] = hg[:G - G // 2].clone()                          # every candidate row twice: exact ties across the shards
    ids = torch.arange(G, device=_dev())
    for kind in ("LBM", "BIM"):
        from taxoexpan_amd import model_zoo as mz
        torch.manual_seed(5)
        match = getattr(mz, kind)(l, r).to(_dev())
        with torch.no_grad():
            S = ops.score_block(q, ops.bilinear_project(hg, match.W.weight), match.apply_exp)
            for larger in (True, False):
                parts = []
                for lo, hi in ((0, 100), (100, 650), (650, G)):
                    Us = ops.bilinear_project(hg[lo:hi], match.W.weight)
                    parts.append(ops.score_topk_block(q, Us, match.apply_exp, k, larger, idx_base=lo))
                idx, key = ops.topk_merge(torch.cat([p[1] for p in parts], 1), torch.cat([p[0] for p in parts], 1), k)
                want = topk_parents(S, ids, k, larger)
                assert torch.equal(idx.long(), want), (kind, larger)
                assert torch.equal(idx.long(), topk_parents_fused(match, hg, q, None, k, larger)), (kind, larger)
                assert torch.equal(key if larger else -key, torch.gather(S, 1, want)), (kind, larger)


def test_world_2_sharded_equals_unsharded():
    """world 2 on cuda:0 over gloo (tests/dist_gpu_topk_wide_worker.py): topk_parents_fused(k = 20, sharded=True) is torch.equal to the
    unsharded result on every rank, LBM and MLP"""
    import socket
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(repo, "tests", "dist_gpu_topk_wide_worker.py")],
                         cwd=repo, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    assert all(out.stdout.count(f"OK {r}") == 1 for r in range(2)), out.stdout[-500:]


# ---- rejected calls ------------------------------------------------------------------------------------------------------------------------
def test_rejected_wide_calls_launch_nothing():
    """every refusal txe.h states for the four new entry points: the code, no launch recorded, outputs and scratch still primed"""
    from taxoexpan_amd import ops
    from taxoexpan_amd.model_zoo import MLP, NTN
    nq, G, r, k = 5, 70, 12, 16
    Q, U = sl.exact_inputs(nq, G, r, 4)
    I = _plain_inputs(Q, U)
    tiles = sl.topk_tiles(G)
    pk, pi, fl, oi, okey, ceil = _nan(nq * tiles * 8), _nani(nq * tiles * 8), _nani(nq), _nani(nq * k), _nan(nq * k), _nani(2 * nq)
    sws = _nan(1 << 18)
    planes = I.planes().data_ptr()
    full = _L().call("txe_score_split_ws_bytes", nq, G, r)
    qonly = sl.round_up(_L().call("txe_split_packed_bytes", nq, r), 256)
    st, sp = _st(), sws.data_ptr()
    A, W = sl.ERR_ARG, sl.ERR_WORKSPACE
    out = dict(pkp=pk.data_ptr(), pip=pi.data_ptr(), flp=fl.data_ptr(), oip=oi.data_ptr(), cp=ceil.data_ptr())

    def bil(Qp=I.Qp, ld_q=r, nq_=nq, Up=I.Up_, ld_u=r, G_=G, r_=r, k_=k, sw=None, swb=0, upk=None, **o):
        o = dict(out, **o)
        return lambda: _rc("txe_score_topk_wide_block", Qp, ld_q, nq_, Up, ld_u, G_, r_, 0, 1, k_, 0, o["pkp"], o["pip"], o["flp"], o["oip"], okey.data_ptr(),
                           sw, swb, upk, o["cp"], st)

    def mrg(kp=pk.data_ptr(), ip=pi.data_ptr(), nq_=nq, cnt_=tiles * 8, k_=k, **o):
        o = dict(out, **o)
        return lambda: _rc("txe_topk_merge_wide", kp, ip, nq_, cnt_, k_, 0, o["oip"], okey.data_ptr(), o["cp"], st)

    torch.manual_seed(1)
    hg, q = _generic(nq, G, 10, r, 2)
    with torch.no_grad():
        mprep = ops.mlp_project(hg, MLP(10, r, 20).to(_dev()))
        margs = list(ops._mlp_args(ops.mlp_prepare_queries(q, mprep), mprep))        # (Ap, flag_a, G, nB, c, flag_b, nq, H, mw)
        nprep = ops.ntn_project(hg, NTN(10, r, k=4).to(_dev()))
        nargs = list(ops._ntn_args(ops.ntn_prepare_queries(q, nprep), nprep))        # (Q, ld_q, nq, U, ld_u, slice_u, G, r, a, ld_a, c, ld_c, u, k)

    def mlp(k_=k, edit=None, **o):
        o, a = dict(out, **o), list(margs)
        if edit:
            a[edit[0]] = edit[1]
        return lambda: _rc("txe_mlp_score_topk_wide_block", *a, 1, k_, 0, o["pkp"], o["pip"], o["flp"], o["oip"], okey.data_ptr(), o["cp"], st)

    def ntn(k_=k, edit=None, **o):
        o, a = dict(out, **o), list(nargs)
        if edit:
            a[edit[0]] = edit[1]
        return lambda: _rc("txe_ntn_score_topk_wide_block", *a, 1, k_, 0, o["pkp"], o["pip"], o["flp"], o["oip"], okey.data_ptr(), o["cp"], st)

    cases = [
        ("wide k = 0", bil(k_=0), A), ("wide k = 65", bil(k_=65), A), ("wide G = 0", bil(G_=0), A), ("wide NULL ceil_ws", bil(cp=None), A), ("wide nq < 0", bil(nq_=-1), A),
        ("wide r < 1", bil(r_=0), A), ("wide ld_u < r", bil(ld_u=r - 1), A), ("wide ld_q < r", bil(ld_q=r - 1), A), ("wide NULL Q", bil(Qp=None), A),
        ("wide NULL U", bil(Up=None), A), ("wide NULL part_key", bil(pkp=None), A), ("wide NULL part_idx", bil(pip=None), A), ("wide NULL floor_ws", bil(flp=None), A),
        ("wide NULL out_idx", bil(oip=None), A), ("wide sws short", bil(sw=sp, swb=full - 1), W), ("wide sws short, u_packed", bil(sw=sp, swb=qonly - 1, upk=planes), W),
        ("merge k = 0", mrg(k_=0), A), ("merge k = 65", mrg(k_=65), A), ("merge nq < 0", mrg(nq_=-1), A), ("merge cnt < 0", mrg(cnt_=-1), A), ("merge NULL keys", mrg(kp=None), A),
        ("merge NULL idx", mrg(ip=None), A), ("merge NULL out_idx", mrg(oip=None), A), ("merge NULL ceil_ws", mrg(cp=None), A),
        ("mlp k = 0", mlp(k_=0), A), ("mlp k = 65", mlp(k_=65), A), ("mlp G = 0", mlp(edit=(2, 0)), A), ("mlp NULL ceil_ws", mlp(cp=None), A), ("mlp nq < 0", mlp(edit=(6, -1)), A),
        ("mlp H < 1", mlp(edit=(7, 0)), A), ("mlp NULL Ap", mlp(edit=(0, None)), A), ("mlp NULL mw", mlp(edit=(8, None)), A), ("mlp NULL part_key", mlp(pkp=None), A),
        ("mlp NULL part_idx", mlp(pip=None), A), ("mlp NULL floor_ws", mlp(flp=None), A), ("mlp NULL out_idx", mlp(oip=None), A),
        ("ntn topk = 0", ntn(k_=0), A), ("ntn topk = 65", ntn(k_=65), A), ("ntn G = 0", ntn(edit=(6, 0)), A), ("ntn NULL ceil_ws", ntn(cp=None), A), ("ntn nq < 0", ntn(edit=(2, -1)), A),
        ("ntn k = 17", ntn(edit=(13, 17)), A), ("ntn r < 1", ntn(edit=(7, 0)), A), ("ntn NULL Q", ntn(edit=(0, None)), A), ("ntn NULL u", ntn(edit=(12, None)), A),
        ("ntn ld_a < G", ntn(edit=(9, G - 1)), A), ("ntn NULL part_key", ntn(pkp=None), A), ("ntn NULL part_idx", ntn(pip=None), A), ("ntn NULL floor_ws", ntn(flp=None), A),
        ("ntn NULL out_idx", ntn(oip=None), A),
    ]
    for what, fn, code in cases:
        rc, names = _profiled(fn)
        assert rc == code and names == [], (what, rc, names)
    # empty blocks are TXE_OK and launch nothing
    for what, fn in (("wide nq 0", bil(nq_=0)), ("merge nq 0", mrg(nq_=0)), ("mlp nq 0", mlp(edit=(6, 0))), ("ntn nq 0", ntn(edit=(2, 0)))):
        rc, names = _profiled(fn)
        assert rc == 0 and names == [], (what, rc, names)
    for t in (pk, okey, sws):
        assert bool(torch.isnan(t).all()), "a rejected call wrote"
    for t in (pi, fl, oi, ceil):
        assert bool((t == NANI).all()), "a rejected call wrote"


# ---- end to end on the toy taxonomy ------------------------------------------------------------------------------------------------------------
def _toy(tmp_path):
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    for fn in os.listdir(os.path.join(GOLDEN_DIR, "toy_taxo")):
        shutil.copy(os.path.join(GOLDEN_DIR, "toy_taxo", fn), tmp_path)
    return MaskedGraphDataset(MAGDataset("toy", str(tmp_path), raw=True), mode="test", sampling_mode=0, expand_factor=100,
                              normalize_embed=True)


def _model(match, non_linear=torch.tanh):
    from taxoexpan_amd import TaxoExpan, model_zoo
    torch.manual_seed(11)
    model = TaxoExpan("PGAT", "WMR", "LBM" if match == "NTN" else match, in_dim=8, hidden_dim=6, out_dim=5, pos_dim=3, num_layers=1, heads=[2, 1],
                      feat_drop=0.1, attn_drop=0.1, hidden_drop=0.1, out_drop=0.1)
    if match == "NTN":
        l, r = model.match.W.weight.shape[-2:]
        model.match = model_zoo.NTN(l, r, k=4, non_linear=non_linear)
    return model.to(_dev())


def _forbid_forward(monkeypatch, model):
    def boom(*a, **k):
        raise AssertionError("the matcher's forward was called on a fused route")
    monkeypatch.setattr(type(model.match), "forward", boom)


def _new_terms():
    rs = np.random.RandomState(5)
    return [f"t{i}" for i in range(9)], rs.standard_normal((9, 8)).astype(np.float32)


def _all_node_candidates(model, ds):
    from taxoexpan_amd.evaluate import candidate_graphs
    from taxoexpan_amd.scoring import encode_candidates
    anchors = list(ds.graph.nodes())
    model.eval()
    hg = encode_candidates(model, candidate_graphs(ds.device_taxonomy(_dev()), anchors, ds.expand_factor, 0)).detach()
    return anchors, hg


@pytest.mark.parametrize("match,loss", [("LBM", "info_nce_loss"), ("MLP", "bce_loss"), ("NTN", "info_nce_loss")])
def test_infer_and_evaluate_top_12_on_the_fused_rounds(tmp_path, monkeypatch, match, loss):
    """infer(topk=12, with_scores=True) and evaluate(case=, topk=12) == scoring.topk_parents on score_all's materialised scores (parents,
    order and the scores themselves), with the matcher's forward forbidden: the fused rounds were taken"""
    from taxoexpan_amd.evaluate import candidate_graphs, evaluate, infer
    from taxoexpan_amd.scoring import encode_candidates, score_all, topk_parents
    ds = _toy(tmp_path)
    model = _model(match)
    larger = loss.startswith("info_nce")
    names, vecs = _new_terms()
    _forbid_forward(monkeypatch, model)
    out = infer(model, ds, (names, vecs), _dev(), loss=loss, topk=12, with_scores=True)
    anchors, hg_all = _all_node_candidates(model, ds)
    assert len(anchors) > 12
    S = score_all(model.match, hg_all, torch.from_numpy(vecs).to(_dev()))
    top = topk_parents(S, torch.arange(len(anchors), device=_dev()), 12, larger)
    want_sc = torch.gather(S, 1, top).cpu().tolist()
    for i, (_q, parents, sc, _lp) in enumerate(out):
        assert parents == [ds.vocab[anchors[j]] for j in top[i].tolist()], (match, i)
        assert [float(v) for v in sc] == want_sc[i], (match, i)
    # the case study: the candidates are the dataset's positions
    cand = sorted(ds.all_positions)
    hg = encode_candidates(model, candidate_graphs(ds.device_taxonomy(_dev()), cand, ds.expand_factor, 0)).detach()
    cand_ids = torch.as_tensor(np.asarray(cand, dtype=np.int64), device=_dev())
    rows = []
    _metrics, _ranks, _pos_off, queries = evaluate(model, ds, _dev(), larger_is_better=larger, case=rows, topk=12)
    qf = ds.node_features[torch.as_tensor(queries, dtype=torch.long)].to(_dev())
    top = topk_parents(score_all(model.match, hg, qf), cand_ids, 12, larger).cpu().tolist()
    assert len(queries) >= 5 and len(top[0]) == 12
    for i in range(len(queries)):
        assert rows[1 + i][2] == ", ".join(ds.vocab[p] for p in top[i]), (match, i)


def test_infer_top_100_on_the_select_route_and_on_the_unfused_matcher(tmp_path, monkeypatch):
    """infer(topk=100) with scoring.TOPK_FUSED_MAX = 64: score blocks + ops.select_k (forward still forbidden), both directions; and an NTN
    with relu, which has no fused route, on the composite -- the same reference: topk_parents on the materialised scores"""
    from taxoexpan_amd import scoring
    from taxoexpan_amd.evaluate import infer
    from taxoexpan_amd.scoring import fused_matcher_ok, score_all, topk_parents
    ds = _toy(tmp_path)
    names, vecs = _new_terms()
    qn = torch.from_numpy(vecs).to(_dev())
    monkeypatch.setattr(scoring, "TOPK_FUSED_MAX", 64)
    for match, loss in (("LBM", "info_nce_loss"), ("MLP", "bce_loss")):
        model = _model(match)
        larger = loss.startswith("info_nce")
        anchors, hg_all = _all_node_candidates(model, ds)
        S = score_all(model.match, hg_all, qn)
        top = topk_parents(S, torch.arange(len(anchors), device=_dev()), 100, larger)
        assert top.shape[1] == min(100, len(anchors)) > 64
        with monkeypatch.context() as mp:
            _forbid_forward(mp, model)
            out = infer(model, ds, (names, vecs), _dev(), loss=loss, topk=100, with_scores=True)
        want_sc = torch.gather(S, 1, top).cpu().tolist()
        for i, (_q, parents, sc, _lp) in enumerate(out):
            assert parents == [ds.vocab[anchors[j]] for j in top[i].tolist()], (match, i)
            assert [float(v) for v in sc] == want_sc[i], (match, i)
    model = _model("NTN", torch.relu)
    assert not fused_matcher_ok(model.match)
    anchors, hg_all = _all_node_candidates(model, ds)
    with torch.no_grad():
        S = torch.stack([model.match(hg_all, q.expand(hg_all.shape[0], -1)).reshape(-1) for q in qn])
    top = topk_parents(S, torch.arange(len(anchors), device=_dev()), 100, True)
    out = infer(model, ds, (names, vecs), _dev(), loss="info_nce_loss", topk=100)
    assert [p for _q, p in out] == [[ds.vocab[anchors[j]] for j in row] for row in top.tolist()]
