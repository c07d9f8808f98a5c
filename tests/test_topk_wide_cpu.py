"""CPU: the wide best-k (9 <= k <= 64) without a device.  scoring.host_topk_rounds -- the kernels' specification, written as they run:
rounds of 8 under a ceiling -- against tests/scoring_loop_ref.topk (one stable sort, any k) on the rows the rounds can get wrong, and
the new C entry points' documented refusals through ctypes (every one returns before a launch, so none needs a GPU)."""
import ctypes

import numpy as np
import pytest

import scoring_loop_ref as sl

KS = (1, 8, 9, 16, 17, 63, 64)
P_ = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)     # a readable address: never read, every call below returns first


def _rows():
    """name -> S [nq][G] (fp32): the edge rows of the rounds"""
    rs = np.random.RandomState(11)
    rows = {}
    rows["all equal"] = np.full((2, 70), 1.5, dtype=np.float32)
    S = rs.permutation(200).astype(np.float32)[None, :].repeat(2, 0)
    # a tie group that straddles positions 8 / 9 and 16 / 17: 6 leaders, 5 tied at 900 (places 7..11), 3 more, 4 tied at 800 (places 15..18)
    S[:, rs.choice(200, 18, replace=False)] = np.array([1000 + i for i in range(6)] + [900] * 5 + [850, 851, 852] + [800] * 4, dtype=np.float32)
    rows["ties across 8/9 and 16/17"] = S
    S = rs.randn(3, 90).astype(np.float32)
    S[0, rs.choice(90, 11, replace=False)] = np.nan            # more than 8 NaNs: k = 90 - 11 + ... reaches into them
    S[1, rs.choice(90, 85, replace=False)] = np.nan            # ... and k = 9 already does
    S[2, :] = np.nan
    rows["NaNs"] = S
    S = np.round(rs.randn(3, 75) * 2).astype(np.float32)
    S[0, [3, 40, 41]], S[0, [7, 8]] = np.inf, -np.inf
    S[1, rs.choice(75, 12, replace=False)] = np.inf            # more than 8 +inf: a whole round of equal infinite keys
    S[1, rs.choice(75, 12, replace=False)] = -np.inf
    S[2, :20] = np.tile(np.array([0.0, -0.0], dtype=np.float32), 10)      # -0.0 and +0.0 tie: column order decides
    rows["infinities and signed zeros"] = S
    for G in (1, 5, 8, 9, 16, 17, 24, 63, 64, 65):             # G < k, G == k, G == 8 R
        rows[f"G = {G}"] = np.round(rs.randn(2, G) * 2).astype(np.float32)
    return rows


@pytest.mark.parametrize("name", list(_rows()))
def test_rounds_of_8_under_a_ceiling_are_the_stable_sort(name):
    """host_topk_rounds == scoring_loop_ref.topk for every k of KS, both directions, idx_base 0 and 77: indices and keys, exactly"""
    from taxoexpan_amd.scoring import host_topk_rounds
    S = _rows()[name]
    for larger in (True, False):
        for k in KS:
            for base in (0, 77):
                want_i, want_k = sl.topk(S, k, larger, idx_base=base)
                got_i, got_k = host_topk_rounds(S, k, larger, idx_base=base)
                assert np.array_equal(got_i, want_i), (name, larger, k, base)
                assert np.array_equal(got_k, want_k), (name, larger, k, base)


def test_rounds_reach_into_the_nans_and_fill_short_rows():
    """the cases above do what they are there for: k reaches into a NaN group of more than 8, a short row ends in -1 / -inf, and the
    straddling tie groups come out in column order"""
    from taxoexpan_amd.scoring import host_topk_rounds
    rows = _rows()
    S = rows["NaNs"]
    idx, key = host_topk_rounds(S, 64, True)
    nan_cols = np.flatnonzero(np.isnan(S[1]))
    assert len(nan_cols) > 8 and idx[1, 5:64].tolist() == nan_cols[:59].tolist() and np.all(key[1, 5:] == -np.inf)
    assert idx[2].tolist() == list(range(64))
    idx, key = host_topk_rounds(rows["G = 9"], 17, False, idx_base=5)
    assert np.all(idx[:, 9:] == -1) and np.all(key[:, 9:] == -np.inf) and np.all(idx[:, :9] >= 5)
    S = rows["ties across 8/9 and 16/17"]
    idx, _ = host_topk_rounds(S, 24, True)
    tied = np.flatnonzero(S[0] == 900)
    assert idx[0, 6:11].tolist() == tied.tolist() and idx[0, 14:18].tolist() == np.flatnonzero(S[0] == 800).tolist()
    assert host_topk_rounds(rows["all equal"], 64, True)[0][0].tolist() == list(range(64))


def test_wide_entry_points_refuse_before_any_launch():
    """txe_topk_wide_max() == 64 == ops.TOPK_WIDE_MAX; k = 0 / 65, G < 1, a NULL ceil_ws, every refusal of the k <= 8 sibling, and a
    short bf16-pipe workspace (TXE_ERR_WORKSPACE) -- each new entry point returns its code with no device in the machine"""
    from taxoexpan_amd import _lib, ops
    lib = _lib.load()
    p = P_
    assert lib.txe_topk_wide_max() == 64 == ops.TOPK_WIDE_MAX

    # txe_score_topk_wide_block(Q, ld_q, nq, U, ld_u, G, r, exp, larger, k, idx_base, part_key, part_idx, floor, out_idx, out_key, sws, sws_bytes, u_packed, ceil_ws, stream)
    def bil(Q=p, ld_q=4, nq=5, U=p, ld_u=4, G=10, r=3, k=16, pk=p, pi=p, fl=p, oi=p, ok=p, sws=None, swb=0, up=None, ceil=p):
        return lib.txe_score_topk_wide_block(Q, ld_q, nq, U, ld_u, G, r, 0, 1, k, 0, pk, pi, fl, oi, ok, sws, swb, up, ceil, None)
    for kw in (dict(k=0), dict(k=65), dict(k=-1), dict(G=0), dict(G=-3), dict(ceil=None), dict(nq=-1), dict(r=0), dict(ld_u=2), dict(ld_q=2),
               dict(Q=None), dict(U=None), dict(pk=None), dict(pi=None), dict(fl=None), dict(oi=None)):
        assert bil(**kw) == sl.ERR_ARG, kw
    assert bil(sws=p, swb=1) == sl.ERR_WORKSPACE and bil(sws=p, swb=1, up=p) == sl.ERR_WORKSPACE
    assert bil(nq=0) == 0 and bil(nq=0, ok=None) == 0                          # nothing to do: success without a launch
    assert bil(nq=1, ld_q=1, k=65) == sl.ERR_ARG                               # (a single row has no pitch; k is still refused)

    # txe_topk_merge_wide(keys, idx, nq, cnt, k, idx_base, out_idx, out_key, ceil_ws, stream)
    def mrg(keys=p, idx=p, nq=5, cnt=30, k=16, oi=p, ok=p, ceil=p):
        return lib.txe_topk_merge_wide(keys, idx, nq, cnt, k, 0, oi, ok, ceil, None)
    for kw in (dict(k=0), dict(k=65), dict(nq=-1), dict(cnt=-1), dict(keys=None), dict(idx=None), dict(oi=None), dict(ceil=None)):
        assert mrg(**kw) == sl.ERR_ARG, kw
    assert mrg(nq=0) == 0

    # txe_mlp_score_topk_wide_block(Ap, flag_a, G, nB, c, flag_b, nq, H, mw, larger, k, idx_base, part_key, part_idx, floor, out_idx, out_key, ceil_ws, stream)
    def mlp(Ap=p, fa=p, G=10, nB=p, c=p, fb=p, nq=5, H=4, mw=p, k=16, pk=p, pi=p, fl=p, oi=p, ok=p, ceil=p):
        return lib.txe_mlp_score_topk_wide_block(Ap, fa, G, nB, c, fb, nq, H, mw, 1, k, 0, pk, pi, fl, oi, ok, ceil, None)
    for kw in (dict(k=0), dict(k=65), dict(G=0), dict(G=-1), dict(ceil=None), dict(nq=-1), dict(H=0), dict(Ap=None), dict(fa=None), dict(nB=None),
               dict(c=None), dict(fb=None), dict(mw=None), dict(pk=None), dict(pi=None), dict(fl=None), dict(oi=None)):
        assert mlp(**kw) == sl.ERR_ARG, kw
    assert mlp(nq=0) == 0

    # txe_ntn_score_topk_wide_block(Q, ld_q, nq, U, ld_u, slice_u, G, r, a, ld_a, c, ld_c, u, k, larger, topk, idx_base, part_key, ..., ceil_ws, stream)
    def ntn(nq=5, G=10, r=3, k=4, ld_q=3, ld_u=3, slice_u=30, ld_a=10, ld_c=5, Q=p, U=p, a=p, c=p, u=p, topk=16, pk=p, pi=p, fl=p, oi=p, ceil=p):
        return lib.txe_ntn_score_topk_wide_block(Q, ld_q, nq, U, ld_u, slice_u, G, r, a, ld_a, c, ld_c, u, k, 1, topk, 0, pk, pi, fl, oi, p, ceil, None)
    for kw in (dict(topk=0), dict(topk=65), dict(G=0), dict(ceil=None), dict(k=0), dict(k=17), dict(r=0), dict(nq=-1), dict(G=-2), dict(ld_u=2),
               dict(ld_q=2), dict(slice_u=2), dict(ld_a=9), dict(ld_c=4), dict(Q=None), dict(U=None), dict(a=None), dict(c=None), dict(u=None),
               dict(pk=None), dict(pi=None), dict(fl=None), dict(oi=None)):
        assert ntn(**kw) == sl.ERR_ARG, kw
    assert ntn(nq=0) == 0


def test_old_entry_points_still_refuse_k_9():
    """the k <= 8 entry points are not widened: k = 9 is TXE_ERR_ARG as before (the wide ones are new symbols)"""
    from taxoexpan_amd import _lib
    lib = _lib.load()
    p = P_
    assert lib.txe_score_topk_block(p, 4, 5, p, 4, 10, 3, 0, 1, 9, 0, p, p, p, p, p, None, 0, None, None) == sl.ERR_ARG
    assert lib.txe_topk_merge(p, p, 5, 30, 9, 0, p, p, None) == sl.ERR_ARG


def test_route_constants():
    from taxoexpan_amd import ops, scoring
    assert 8 <= scoring.TOPK_FUSED_MAX <= ops.TOPK_WIDE_MAX == 64 < ops.SELECT_K_MAX == scoring.RETRIEVE_K_MAX == 4096
