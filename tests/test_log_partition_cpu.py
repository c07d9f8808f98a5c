"""CPU: the log-partition's host side -- scoring.host_log_partition against the independent reference (tests/log_partition_ref.py), the
definition against F.cross_entropy (the call of loss.py:57), every documented TXE_ERR_ARG / TXE_ERR_WORKSPACE of the four entry points
(returned before any device work: no GPU needed), and the refusals of evaluate(nll=True) / infer(with_scores=True) with retrieve=k."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import log_partition_ref as lp


def _special_scores():
    rs = np.random.RandomState(3)
    S = (rs.standard_normal((12, 37)) * 6).astype(np.float32)
    S[1, 5] = np.nan
    S[2, 7] = np.inf
    S[3, 9] = -np.inf
    S[4, :] = -np.inf
    S[5, :] = np.inf
    S[6, 3], S[6, 4] = np.nan, np.inf
    S[7, 0] = 300.0                                        # a leader far ahead: lse == max
    S[8, :] = -200.0                                       # exp underflows in fp32, not in the float64 formula
    S[9, 2], S[9, 3] = np.inf, -np.inf
    return S


@pytest.mark.parametrize("larger", [True, False])
def test_host_log_partition_equals_the_reference(larger):
    from taxoexpan_amd.scoring import host_log_partition
    S = _special_scores()
    got, want = host_log_partition(S, larger), lp.row_lse(S, larger)
    assert got.dtype == np.float64 and got.shape == (12,)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])          # the signs of the infinities
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-14, atol=0)
    # the documented pattern itself, on the rows planted above
    z = S.astype(np.float64) if larger else -S.astype(np.float64)
    assert np.isnan(want[1]) and np.isnan(want[6]) and want[2] == (np.inf if larger else lp._lse_of(z[2]))
    assert want[4] == (-np.inf if larger else np.inf) and want[5] == (np.inf if larger else -np.inf)
    assert want[7] == 300.0 if larger else want[8] == pytest.approx(200.0 + np.log(37), rel=1e-15)
    assert host_log_partition(torch.from_numpy(S), larger).tolist() == pytest.approx(got.tolist(), nan_ok=True)
    assert host_log_partition(np.zeros((3, 0), dtype=np.float32), larger).tolist() == [-np.inf] * 3


def test_tile_pairs_merge_to_the_row_value():
    """the reference's two halves agree: merging the per-tile pairs gives the row's lse, special values included"""
    S = np.concatenate([_special_scores()] * 8, axis=1)                                      # 296 columns: three tiles
    for larger in (True, False):
        want, got = lp.row_lse(S, larger), lp.merge_pairs(*lp.tile_pairs(S, larger))
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        inf = ok & np.isinf(want)
        assert np.array_equal(got[inf], want[inf])
        np.testing.assert_allclose(got[ok & ~inf], want[ok & ~inf], rtol=1e-14, atol=0)
    assert lp.merge_pairs(np.zeros((2, 0)), np.zeros((2, 0))).tolist() == [-np.inf, -np.inf]


def test_definition_is_cross_entropy_over_the_group():
    """loss.py:52-57: info_nce_loss = F.cross_entropy(prediction.reshape(B, 1 + k), zeros, reduction="sum") -- on a [B, 1 + k] group matrix
    that is sum_b (lse[b] - z[b][0]): the log-partition over ALL candidates is the same formula with the whole candidate list as the group"""
    from taxoexpan_amd.scoring import host_log_partition
    torch.manual_seed(0)
    z = (torch.randn(9, 1 + 31) * 4).float()
    want = float(torch.nn.functional.cross_entropy(z.double(), torch.zeros(9, dtype=torch.long), reduction="sum"))
    got = float(np.sum(host_log_partition(z) - z[:, 0].double().numpy()))
    assert got == pytest.approx(want, rel=1e-13)
    assert float(np.sum(lp.row_lse(z.numpy()) - z[:, 0].double().numpy())) == pytest.approx(want, rel=1e-13)
    assert lp.nll(lp.row_lse(z.numpy()), z[:, 0].numpy(), np.arange(10)) == pytest.approx(want / 9, rel=1e-13)


def test_argument_validation_needs_no_gpu():
    """every documented TXE_ERR_ARG (-1) / TXE_ERR_WORKSPACE (-3) of the four entry points comes back before anything is launched (the
    pointers are host addresses, never read), and nq == 0 is TXE_OK without a launch"""
    from taxoexpan_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    # txe_score_lse_block(Q, ld_q, nq, U, ld_u, G, r, apply_exp, larger, part_max, part_sum, lse, sws, sws_bytes, u_packed, stream)
    good = [a, 8, 4, a, 8, 5, 8, 0, 1, a, a, a, None, 0, None, None]

    def score(**kw):
        pos = dict(Q=0, ld_q=1, nq=2, U=3, ld_u=4, G=5, r=6, part_max=9, part_sum=10, lse=11, sws=12, sws_bytes=13, u_packed=14)
        args = list(good)
        for k, v in kw.items():
            args[pos[k]] = v
        return lib.txe_score_lse_block(*args)
    for bad in (dict(nq=-1), dict(G=0), dict(G=-3), dict(r=0), dict(ld_u=7), dict(ld_q=7), dict(Q=None), dict(U=None), dict(part_max=None),
                dict(part_sum=None), dict(lse=None)):
        assert score(**bad) == -1, bad
    assert score(nq=0) == 0 and score(nq=0, Q=a, lse=a) == 0
    assert score(nq=1, ld_q=0, G=0) == -1                                  # (a single row has no pitch; G < 1 still counts)
    need = lib.txe_score_split_ws_bytes(4, 5, 8)
    assert need > 0 and score(sws=a, sws_bytes=need - 1) == -3 and score(sws=a, sws_bytes=0) == -3
    packed_q = (lib.txe_split_packed_bytes(4, 8) + 255) // 256 * 256
    assert score(sws=a, sws_bytes=packed_q - 1, u_packed=a) == -3
    # txe_lse_merge(part_max, part_sum, nq, cnt, lse, stream)
    assert lib.txe_lse_merge(a, a, -1, 3, a, None) == -1 and lib.txe_lse_merge(a, a, 2, -1, a, None) == -1
    assert lib.txe_lse_merge(None, a, 2, 3, a, None) == -1 and lib.txe_lse_merge(a, None, 2, 3, a, None) == -1
    assert lib.txe_lse_merge(a, a, 2, 3, None, None) == -1 and lib.txe_lse_merge(a, a, 0, 3, a, None) == 0
    # txe_mlp_score_lse_block(Ap, flag_a, G, nB, c, flag_b, nq, H, mw, larger, part_max, part_sum, lse, stream)
    mgood = [a, a, 5, a, a, a, 4, 6, a, 1, a, a, a, None]
    for i, v in ((0, None), (1, None), (2, 0), (2, -1), (3, None), (4, None), (5, None), (6, -1), (7, 0), (8, None), (10, None), (11, None),
                 (12, None)):
        args = list(mgood)
        args[i] = v
        assert lib.txe_mlp_score_lse_block(*args) == -1, (i, v)
    args = list(mgood)
    args[6] = 0
    assert lib.txe_mlp_score_lse_block(*args) == 0
    # txe_ntn_score_lse_block(Q, ld_q, nq, U, ld_u, slice_u, G, r, a, ld_a, c, ld_c, u, k, larger, part_max, part_sum, lse, stream)
    ngood = [a, 8, 4, a, 32, 8, 5, 8, a, 5, a, 4, a, 4, 1, a, a, a, None]
    for i, v in ((0, None), (1, 7), (2, -1), (3, None), (4, 7), (5, 7), (6, 0), (6, -2), (7, 0), (8, None), (9, 4), (10, None), (11, 3), (12, None),
                 (13, 0), (13, 17), (15, None), (16, None), (17, None)):
        args = list(ngood)
        args[i] = v
        assert lib.txe_ntn_score_lse_block(*args) == -1, (i, v)
    args = list(ngood)
    args[2] = 0
    assert lib.txe_ntn_score_lse_block(*args) == 0


def test_partition_over_a_retrieved_subset_is_refused():
    """nll=True / with_scores=True with retrieve=k: ValueError before anything is touched (no model, no dataset, no device needed)"""
    from taxoexpan_amd import scoring
    from taxoexpan_amd.evaluate import evaluate, infer
    with pytest.raises(ValueError, match="retrieve"):
        evaluate(None, None, "cpu", retrieve=3, nll=True)
    with pytest.raises(ValueError, match="retrieve"):
        infer(None, None, None, "cpu", retrieve=3, with_scores=True)
    params = inspect.signature(scoring.log_partition_fused).parameters
    assert list(params) == ["match", "hg", "queries", "larger_is_better", "block"] and "group" not in params
    assert inspect.signature(evaluate).parameters["nll"].default is False
    assert inspect.signature(infer).parameters["with_scores"].default is False
    assert inspect.signature(scoring.topk_parents_fused).parameters["return_scores"].default is False
