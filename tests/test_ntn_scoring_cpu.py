"""CPU: the NTN matcher's all-candidate route without a device -- the float64 host restatement (scoring.host_ntn_scores) against the
oracle's per-query NTN and the reference's golden, which matchers scoring.fused_matcher_ok sends to the fused route, and the txe_ntn_*
entry points' argument checks (they reject bad arguments, and return at once for empty work, before touching a device)."""
import os

import numpy as np
import torch

import txe_oracle as orc
from golden_util import GOLDEN_DIR

P_ = 0x1000          # a non-NULL pointer value that is never dereferenced: every call below fails its argument checks first


def test_host_ntn_scores_equals_the_oracle_per_query():
    from taxoexpan_amd import scoring
    G, Q, l, r, k = 13, 5, 7, 4, 3
    gen = torch.Generator().manual_seed(5)
    hg = torch.randn(G, l, generator=gen, dtype=torch.float64)
    q = torch.randn(Q, r, generator=gen, dtype=torch.float64)
    W = torch.randn(k, l, r, generator=gen, dtype=torch.float64) * 0.4
    b = torch.randn(k, generator=gen, dtype=torch.float64)
    V = torch.randn(k, l + r, generator=gen, dtype=torch.float64) * 0.4
    u = torch.randn(1, k, generator=gen, dtype=torch.float64)
    want = torch.stack([orc.ntn_match(hg, qq.expand(G, -1), u, W, b, V).squeeze(1) for qq in q]).numpy()
    got = scoring.host_ntn_scores((W, b, V, u), hg, q)
    assert got.shape == (Q, G) and got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-13)
    # the same parameters by state-dict keys, and from a module
    got_d = scoring.host_ntn_scores({"W.weight": W, "W.bias": b, "V.weight": V, "u_R.weight": u}, hg, q)
    assert np.array_equal(got_d, got)
    from taxoexpan_amd.model_zoo import NTN
    m = NTN(l, r, k=k).double()
    with torch.no_grad():
        m.W.weight.copy_(W); m.W.bias.copy_(b); m.V.weight.copy_(V); m.u_R.weight.copy_(u)
    assert np.array_equal(scoring.host_ntn_scores(m, hg, q), got)


def test_host_ntn_scores_diagonal_is_the_reference_golden():
    from taxoexpan_amd import scoring
    g = np.load(os.path.join(GOLDEN_DIR, "extras.npz"))
    params = (g["ntn.p.W.weight"], g["ntn.p.W.bias"], g["ntn.p.V.weight"], g["ntn.p.u_R.weight"])
    S = scoring.host_ntn_scores(tuple(torch.as_tensor(np.asarray(p)) for p in params), np.asarray(g["ntn.e1"]), np.asarray(g["ntn.e2"]))
    n = np.asarray(g["ntn.e1"]).shape[0]
    assert S.shape == (n, n)
    np.testing.assert_allclose(np.diagonal(S), np.asarray(g["ntn.out"]).reshape(-1), rtol=0, atol=1e-5)


def test_fused_matcher_ok_answers():
    from taxoexpan_amd import model_zoo as mz
    from taxoexpan_amd.scoring import fused_matcher_ok
    assert fused_matcher_ok(mz.NTN(5, 4)) is True
    assert fused_matcher_ok(mz.NTN(5, 4, non_linear=torch.nn.functional.tanh)) is True
    assert fused_matcher_ok(mz.NTN(5, 4, k=1)) is True and fused_matcher_ok(mz.NTN(5, 4, k=16)) is True
    assert fused_matcher_ok(mz.NTN(5, 4, non_linear=torch.relu)) is False
    assert fused_matcher_ok(mz.NTN(5, 4, k=17)) is False
    # unchanged answers
    assert fused_matcher_ok(mz.BIM(5, 4)) and fused_matcher_ok(mz.LBM(5, 4)) and fused_matcher_ok(mz.MLP(5, 4, 6))
    assert not fused_matcher_ok(torch.nn.Linear(5, 4))


def test_prepare_matcher_refuses_an_ntn_without_a_fused_route():
    import pytest
    from taxoexpan_amd import model_zoo as mz
    from taxoexpan_amd.scoring import prepare_matcher
    with pytest.raises(TypeError, match="NTN"):
        prepare_matcher(mz.NTN(5, 4, non_linear=torch.relu), torch.zeros(3, 5))


def _score_args(nq=5, G=10, r=3, k=4, ld_q=3, ld_u=3, slice_u=30, ld_a=10, ld_c=5, Q=P_, U=P_, a=P_, c=P_, u=P_):
    return (Q, ld_q, nq, U, ld_u, slice_u, G, r, a, ld_a, c, ld_c, u, k)


def test_ntn_entry_points_reject_bad_arguments_without_a_device():
    from taxoexpan_amd import _lib
    lib = _lib.load()
    p = P_
    # candidate side: (hg, ld_hg, G, l, V1, ld_v, b, k, a, ld_a, stream)
    assert lib.txe_ntn_project(p, 7, 10, 7, p, 11, p, 0, p, 10, None) == -1            # k < 1
    assert lib.txe_ntn_project(p, 7, 10, 7, p, 11, p, 17, p, 10, None) == -1           # k > 16
    assert lib.txe_ntn_project(p, 7, -1, 7, p, 11, p, 4, p, 10, None) == -1            # G < 0
    assert lib.txe_ntn_project(p, 7, 10, 0, p, 11, p, 4, p, 10, None) == -1            # l < 1
    assert lib.txe_ntn_project(p, 6, 10, 7, p, 11, p, 4, p, 10, None) == -1            # ld_hg < l
    assert lib.txe_ntn_project(p, 7, 10, 7, p, 6, p, 4, p, 10, None) == -1             # ld_v < l
    assert lib.txe_ntn_project(p, 7, 10, 7, p, 11, p, 4, p, 9, None) == -1             # ld_a < G
    for hole in range(4):
        ptrs = [p, p, p, p]
        ptrs[hole] = None
        assert lib.txe_ntn_project(ptrs[0], 7, 10, 7, ptrs[1], 11, ptrs[2], 4, ptrs[3], 10, None) == -1
    assert lib.txe_ntn_project(p, 7, 0, 7, p, 11, p, 4, p, 10, None) == 0              # no candidates: nothing to launch
    # query side: (Q, ld_q, nq, r, V2, ld_v, k, c, ld_c, stream)
    assert lib.txe_ntn_query_project(p, 3, 5, 3, p, 10, 0, p, 5, None) == -1
    assert lib.txe_ntn_query_project(p, 3, 5, 3, p, 10, 17, p, 5, None) == -1
    assert lib.txe_ntn_query_project(p, 3, -5, 3, p, 10, 4, p, 5, None) == -1
    assert lib.txe_ntn_query_project(p, 3, 5, 0, p, 10, 4, p, 5, None) == -1           # r < 1
    assert lib.txe_ntn_query_project(p, 2, 5, 3, p, 10, 4, p, 5, None) == -1           # ld_q < r
    assert lib.txe_ntn_query_project(p, 3, 5, 3, p, 2, 4, p, 5, None) == -1            # ld_v < r
    assert lib.txe_ntn_query_project(p, 3, 5, 3, p, 10, 4, p, 4, None) == -1           # ld_c < nq
    assert lib.txe_ntn_query_project(None, 3, 5, 3, p, 10, 4, p, 5, None) == -1
    assert lib.txe_ntn_query_project(p, 3, 5, 3, None, 10, 4, p, 5, None) == -1
    assert lib.txe_ntn_query_project(p, 3, 5, 3, p, 10, 4, None, 5, None) == -1
    assert lib.txe_ntn_query_project(p, 3, 0, 3, p, 10, 4, p, 5, None) == 0
    # the four scoring entry points share their leading arguments: every bad one is refused by each of them
    tails = {
        "txe_ntn_score_block": (p, 12, None),                                           # S, ld_s
        "txe_ntn_score_positives": (p, p, None),                                        # pos_off, thr
        "txe_ntn_score_count_block": (p, p, 1, p, None),                                # pos_off, thr, larger, counts
        "txe_ntn_score_topk_block": (1, 5, 0, p, p, p, p, p, None),                     # larger, topk, idx_base, part_key, part_idx, floor, out_idx, out_key
    }
    bad = [dict(k=0), dict(k=17), dict(r=0), dict(nq=-1), dict(G=-2), dict(ld_u=2), dict(ld_q=2), dict(slice_u=2), dict(ld_a=9), dict(ld_c=4),
           dict(Q=None), dict(U=None), dict(a=None), dict(c=None), dict(u=None)]
    for name, tail in tails.items():
        fn = getattr(lib, name)
        for kw in bad:
            assert fn(*_score_args(**kw), *tail) == -1, (name, kw)
    assert lib.txe_ntn_score_block(*_score_args(), p, 8, None) == -1                    # ld_s < G
    assert lib.txe_ntn_score_block(*_score_args(), None, 12, None) == -1
    assert lib.txe_ntn_score_positives(*_score_args(), None, p, None) == -1
    assert lib.txe_ntn_score_positives(*_score_args(), p, None, None) == -1
    assert lib.txe_ntn_score_count_block(*_score_args(), None, p, 1, p, None) == -1
    assert lib.txe_ntn_score_count_block(*_score_args(), p, None, 1, p, None) == -1
    assert lib.txe_ntn_score_count_block(*_score_args(), p, p, 1, None, None) == -1
    for topk in (0, 9):
        assert lib.txe_ntn_score_topk_block(*_score_args(), 1, topk, 0, p, p, p, p, p, None) == -1
    assert lib.txe_ntn_score_topk_block(*_score_args(G=0), 1, 5, 0, p, p, p, p, p, None) == -1      # no candidates to select from
    for hole in range(4):
        ptrs = [p, p, p, p]
        ptrs[hole] = None
        assert lib.txe_ntn_score_topk_block(*_score_args(), 1, 5, 0, *ptrs, p, None) == -1
    # nothing to do: success without a launch
    for kw in (dict(nq=0), dict(G=0)):
        assert lib.txe_ntn_score_block(*_score_args(**kw), p, 12, None) == 0
        assert lib.txe_ntn_score_positives(*_score_args(**kw), p, p, None) == 0
        assert lib.txe_ntn_score_count_block(*_score_args(**kw), p, p, 1, p, None) == 0
    assert lib.txe_ntn_score_topk_block(*_score_args(nq=0), 1, 5, 0, p, p, p, p, p, None) == 0
