"""CPU: tests/scoring_loop_ref.py, the reference of tests/test_gpu_scoring_loop_ops.py, held to the project's own host code
(scoring.topk_parents, scoring._rank_finalize_host, the loop of test_rank_kernel_against_metric_definition), to the goldens that hold the
same quantities (tests/golden/scoring.npz, obtain_ranks.npz), its exact generator to its claim (fp32 sums in any order are exact, planes 1
and 2 of the three-bf16 decomposition are zero, |raw| <= 80 under the exp), and its case tables to every edge they are there for at 256
CUs -- a table that stops reaching a branch fails here, not silently on the GPU."""
import os

import numpy as np
import pytest
import torch

import golden_cases as gc
import scoring_loop_ref as sl
from golden_util import GOLDEN_DIR
from test_split_arithmetic import split3


def _tied_scores(nq, G, seed):
    rs = np.random.RandomState(seed)
    S = np.round(rs.randn(nq, G) * 3).astype(np.float32) / 2          # many exact ties
    S[0, :3] = (0.0, -0.0, 0.0)
    return rs, S


def test_topk_is_pythons_stable_sort_and_topk_parents():
    """topk() == `sorted(enumerate(scores), key=-score)[:k]` literally (infer.py:100-106) and == scoring.topk_parents, both directions, ties,
    NaN (last) and infinities; a row shorter than k is filled with -1"""
    from taxoexpan_amd.scoring import topk_parents
    rs, S = _tied_scores(9, 203, 5)
    for larger in (True, False):
        for k in (1, 5, 8):
            idx, key = sl.topk(S, k, larger)
            for q in range(S.shape[0]):
                lit = [g for g, _ in sorted(enumerate(S[q].tolist()), key=lambda e: -e[1] if larger else e[1])[:k]]
                assert idx[q].tolist() == lit
                assert np.array_equal(key[q], sl.keys_of(S, larger)[q][lit])
    S[2, 7], S[3, 100], S[4, 5], S[5, :] = np.nan, np.inf, -np.inf, np.nan
    for larger in (True, False):
        for k in (1, 5, 8):
            want = topk_parents(torch.from_numpy(S), torch.arange(S.shape[1]), k, larger).numpy()
            assert np.array_equal(sl.topk(S, k, larger)[0], want)
    idx, key = sl.topk(S[:, :3], 5, True, idx_base=7)
    assert (idx[:, 3:] == -1).all() and np.isneginf(key[:, 3:]).all() and (idx[:, :3] >= 7).all()


def test_merge_is_topk_on_scattered_entries():
    """merge() over a row's (key, idx) entries in any order, with empty slots between them, == topk() of the row they came from"""
    rs, S = _tied_scores(5, 300, 6)
    S[1, 4], S[2, 9] = np.nan, -np.inf
    for k in (1, 4, 8):
        perm = np.stack([rs.permutation(400) for _ in range(5)])
        keys, idx = np.full((5, 400), -np.inf, dtype=np.float32), np.full((5, 400), sl.INT_MAX, dtype=np.int64)
        for q in range(5):
            keys[q, perm[q, :300]], idx[q, perm[q, :300]] = S[q], np.arange(300)
        oi, ok = sl.merge(keys, idx, k, 11)
        ti, tk = sl.topk(S, k, True, 11)
        assert np.array_equal(oi, ti) and np.array_equal(ok, tk)
    oi, ok = sl.merge(np.zeros((2, 0)), np.zeros((2, 0)), 3)
    assert (oi == -1).all() and np.isneginf(ok).all()


@pytest.mark.parametrize("larger", [True, False])
def test_ranks_counts_and_finalize_agree_with_the_host_code(larger):
    """ranks() == the loop of test_rank_kernel_against_metric_definition; finalize(counts()) == ranks() when the thresholds are the
    positives' own scores; finalize() == scoring._rank_finalize_host"""
    from taxoexpan_amd.scoring import _rank_finalize_host
    rs, S = _tied_scores(23, 1003, 7)
    S[3, 10], S[4, 11] = np.nan, np.inf
    npos = rs.randint(0, 10, size=23)
    pos_idx = np.concatenate([rs.choice(1003, size=k, replace=False) for k in npos]).astype(np.int32)
    pos_off = np.concatenate([[0], np.cumsum(npos)]).astype(np.int32)
    want = []
    for q in range(23):
        P = pos_idx[pos_off[q]:pos_off[q + 1]]
        neg = np.ones(1003, dtype=bool)
        neg[P] = False
        for p in P:
            want.append(1 + int(((S[q][neg] > S[q][p]) if larger else (S[q][neg] < S[q][p])).sum()))
    got = sl.ranks(S, pos_off, pos_idx, larger)
    assert got.tolist() == want
    thr = np.concatenate([S[q, pos_idx[pos_off[q]:pos_off[q + 1]]] for q in range(23)])
    cnt = sl.counts(S, pos_off, thr, larger)
    fin = sl.finalize(pos_off, thr, cnt, larger)
    assert fin.tolist() == want
    host = _rank_finalize_host(torch.from_numpy(pos_off), torch.from_numpy(thr), torch.from_numpy(cnt), larger)
    assert host.tolist() == want


def test_reference_against_the_goldens():
    """scoring.npz: scores64 of the golden's inputs within the golden's own tolerance, ranks() on the golden's scores exactly;
    obtain_ranks.npz: every group is one score row whose positives lead it -- ranks() gives the reference's ranks"""
    z = dict(np.load(os.path.join(GOLDEN_DIR, "scoring.npz")))
    hg, qs, W, positives = gc.make_scoring_inputs()
    U = hg.astype(np.float64) @ W[0].astype(np.float64)
    pos_off = np.concatenate([[0], np.cumsum([len(p) for p in positives])])
    pos_idx = np.concatenate(positives)
    for kind, ex in (("lbm", True), ("bim", False)):
        np.testing.assert_allclose(sl.scores64(qs, U, ex), z[f"S_{kind}"], rtol=2e-5, atol=1e-6)
        assert sl.ranks(z[f"S_{kind}"], pos_off, pos_idx, True).tolist() == z[f"ranks_{kind}"].tolist()
        assert pos_off.tolist() == z[f"ranks_{kind}_off"].tolist()
        thr = z[f"S_{kind}"][np.repeat(np.arange(len(positives)), np.diff(pos_off)), pos_idx]
        assert sl.finalize(pos_off, thr, sl.counts(z[f"S_{kind}"], pos_off, thr, True), True).tolist() == z[f"ranks_{kind}"].tolist()
    z = np.load(os.path.join(GOLDEN_DIR, "obtain_ranks.npz"))
    groups = 0
    for c in range(int(z["n_cases"])):
        score, label, mode = z[f"{c}:score"], z[f"{c}:label"], int(z[f"{c}:mode"])
        starts = np.flatnonzero(np.concatenate([[True], (label[:-1] == 0) & (label[1:] == 1)]))
        got = []
        for a, b in zip(starts, np.append(starts[1:], len(label))):
            P = np.flatnonzero(label[a:b] == 1)
            if len(P) < b - a:                                    # (a group without negatives is outside the reference's domain)
                got += sl.ranks(score[None, a:b], np.array([0, len(P)]), P, mode == 1).tolist()
                groups += 1
            else:
                got += [1] * len(P)
        assert got == z[f"{c}:ranks"].tolist(), c
    assert groups > 100


def _exact_cases():
    out = []
    for c in sl.SCORE_CASES:
        for v in c["variants"]:
            out.append((c["nq"], c["G"], c["r"], c["pos"], v, c["zero_from"], 17))
    nq, G, p = sl.wide_shape()
    out += [(nq, G, sl.WIDE_CASE["r"], "wide", v, None, p) for v in sl.WIDE_CASE["variants"]]
    out += [(nq, G, r, None, "plain", None, 17) for nq, G, r, _ in sl.persist_shapes()[1:]]
    return out


@pytest.mark.parametrize("case", _exact_cases(), ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-{c[4]}")
def test_exact_inputs_are_exact(case):
    """for every exact case: the fp32 product in two summation orders (ascending and descending k, one fp32 addition at a time) is
    bit-equal to float64 cast to fp32; planes 1 and 2 of the three-bf16 decomposition are zero; |raw| <= 80 under the exp; the NaN / Inf
    pattern of the float64 reference is the one of the fp32 sums; ties are there"""
    nq, G, r, pos, variant, zero_from, wide_p = case
    off, idx = sl.positives(nq, G, pos, 1, wide_p) if pos else (None, None)
    Q, U = sl.exact_inputs(nq, G, r, 3, thin=variant == "exp", special=variant == "special", pos_off=off, pos_idx=idx, zero_from=zero_from)
    assert Q.dtype == U.dtype == np.float32
    for a in (Q, U):
        f = a[np.isfinite(a)]
        assert np.array_equal(f * 4, np.round(f * 4)) and np.abs(f).max(initial=0) <= 4
        _x1, x2, x3 = split3(f)
        assert not x2.any() and not x3.any()
    rows = np.unique(np.concatenate([np.arange(min(nq, 3)), [nq // 2, nq - 1]]))         # a few whole rows: the claim is per entry
    S64 = sl.scores64(Q[rows], U, False)
    with np.errstate(all="ignore"):
        fwd, bwd = np.zeros((len(rows), G), dtype=np.float32), np.zeros((len(rows), G), dtype=np.float32)
        for k in range(r):
            fwd += Q[rows, k][:, None] * U[None, :, k]
            bwd += Q[rows, r - 1 - k][:, None] * U[None, :, r - 1 - k]
        want = S64.astype(np.float32)
    assert np.array_equal(fwd, want, equal_nan=True) and np.array_equal(bwd, want, equal_nan=True)
    if variant == "exp":
        assert np.abs(sl.scores64(Q, U, False)).max() <= 80
    if variant == "special":
        assert np.isnan(S64).any() and np.isposinf(S64).any() and np.isneginf(S64).any() and np.isfinite(S64).any()
    if G > 8:
        assert max(len(S64[i]) - len(np.unique(S64[i])) for i in range(len(rows))) >= G // 8             # exact ties


def test_predicates_on_known_shapes():
    """the restated predicates at shapes whose answers the project's documents state: MAG-CS scoring (1,024 x 31,138... k 256) runs on
    the persistent kernel with leftover whole tiles; a 512 x 8,201 block takes 128-wide tiles at 256 CUs"""
    assert sl.loader_pair(12, 0, 10, 0) == (4, 2) and sl.loader_pair(32, 2, 32, 2) == (2, 2) and sl.loader_pair(33, 0, 36, 0) == (1, 1)
    assert sl.loader_pair(32, 0, 32, 1) == (1, 1) and sl.loader_pair(34, 0, 32, 0) == (2, 4)
    assert sl.choose_bn(512, 8201) == 128 and sl.choose_bn(300, 1003) == 64 and sl.choose_bn(1, 64) == 64
    assert sl.persist_plan(1024, 16600, 160, 4, 4, True)["rest"] == 16 and sl.persist_plan(1024, 16600, 160, 4, 4, False) is None
    assert sl.persist_plan(1024, 16600, 160, 4, 2, True) is None and sl.persist_plan(1024, 16600, 128, 4, 4, True) is None
    assert sl.persist_plan(1024, 16600, 288, 4, 4, True)["name"] == "gemm_persist_kernel<true, true, 8, 4>"
    assert sl.launches("topk", "packed", 5, 300, 10) == ["split_pack_kernel", sl.SPLIT_KERNEL, "topk_merge_kernel"]
    assert sl.launches("count", "mfma", 0, 300, 10) == [] and sl.launches("positives", "split", 5, 0, 10) == []
    assert sl.topk_tiles(128) == 1 and sl.topk_tiles(129) == 2


def test_tables_reach_every_edge_at_256_cus():
    e = sl.edges(256)
    assert len(e) > 60
    missing = [k for k, v in e.items() if not v]
    assert not missing, missing
    nq, G, p = sl.wide_shape(256)
    assert (nq, G) == (512, 8201) and p == 17
    assert [s[:3] for s in sl.persist_shapes(256)] == [(1024, 16344, 160), (1024, 16600, 160)]
    for c in sl.SCORE_CASES:
        assert c["ld_q"] >= c["r"] and c["ld_u"] >= c["r"] and c["ld_s"] >= c["G"] and c["why"]
