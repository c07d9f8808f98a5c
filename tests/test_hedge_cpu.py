"""CPU: hedged placement's host side -- HedgeIndex.build against brute-force descendant sets, the numpy restatement of the subtree
mass (value and summation order) and of the hedging rule, and every argument check that must come before a device call."""
import ctypes
import math
import os
import shutil

import numpy as np
import pytest
import torch

import hedge_cases as hc
from golden_util import GOLDEN_DIR
from taxoexpan_amd import hedge
from taxoexpan_amd.hedge import SLICE, HedgeIndex


def _rows(ix):
    return [ix.row(a).tolist() for a in range(ix.G)]


def _check_index(parents, n, cand):
    ix = HedgeIndex.build(hc.index_of(parents, n), cand)
    assert _rows(ix) == hc.brute_sub(parents, n, cand)
    assert ix.depth.tolist() == [hc.brute_depth(parents, n)[a] for a in cand]
    assert all(a.dtype == np.int32 for a in (ix.sub_ptr, ix.sub_idx, ix.depth, ix.item_row, ix.item_slice, ix.item_part, ix.long_row, ix.long_ptr))
    assert ix.sub_ptr.shape == (len(cand) + 1,) and ix.sub_ptr[0] == 0 and ix.sub_ptr[-1] == ix.sub_idx.size
    # the work list: every row's slices, in row order then slice order, and the long rows' workspace positions in the same order
    want = [(a, s) for a in range(ix.G) for s in range(max(1, -(-len(ix.row(a)) // SLICE)))]
    assert list(zip(ix.item_row.tolist(), ix.item_slice.tolist())) == want
    longs = [a for a in range(ix.G) if len(ix.row(a)) > SLICE]
    assert ix.long_row.tolist() == longs
    parts = [p for p in ix.item_part.tolist() if p >= 0]
    assert parts == list(range(ix.n_part)) and ix.long_ptr[-1] == ix.n_part
    assert all((p >= 0) == (a in longs) for a, p in zip(ix.item_row.tolist(), ix.item_part.tolist()))
    return ix


@pytest.mark.parametrize("case", ["chain", "star", "diamond", "forest"])
def test_index_against_brute_force_sets(case):
    parents, n = getattr(hc, case)()
    ix = _check_index(parents, n, list(range(n)))
    if case == "diamond":                               # node 3 and its child are reached along two paths and counted once
        assert ix.row(0).tolist() == [0, 1, 2, 3, 4] and ix.row(1).tolist() == [1, 3, 4] and ix.row(2).tolist() == [2, 3, 4]
    if case == "forest":
        assert ix.row(0).tolist() == [0, 1, 2] and ix.row(3).tolist() == [3, 4, 5, 6]
    # a shuffled candidate list: columns are positions in `cand`, not node ids
    _check_index(parents, n, np.random.RandomState(1).permutation(n).tolist())


def test_index_on_a_candidate_subset():
    """an interior node (3) and a leaf (2) are not candidates: 3's child 4 still counts for every ancestor above the dropped node"""
    parents, n = hc.diamond()
    ix = _check_index(parents, n, [0, 1, 4])
    assert _rows(ix) == [[0, 1, 2], [1, 2], [2]]
    parents, n = hc.forest()
    _check_index(parents, n, [6, 3, 0, 1])


def test_index_with_long_rows():
    parents, n, who = hc.star_plus_chain(SLICE)
    cand = list(range(n))
    ix = _check_index(parents, n, cand)
    assert n == 3 * SLICE + 6
    lens = {k: len(ix.row(v)) for k, v in who.items()}
    assert lens == dict(root=3 * SLICE + 5, b=SLICE + 1, c=SLICE, lone=1)
    assert ix.n_long == 2 and ix.n_part == 4 + 2 and ix.n_items == n + 3 + 1


def _toy(tmp_path):
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    for fn in os.listdir(os.path.join(GOLDEN_DIR, "toy_taxo")):
        shutil.copy(os.path.join(GOLDEN_DIR, "toy_taxo", fn), tmp_path)
    return MaskedGraphDataset(MAGDataset("toy", str(tmp_path), raw=True), mode="test", sampling_mode=0, expand_factor=100, normalize_embed=True)


def test_index_on_the_toy_taxonomy(tmp_path):
    from taxoexpan_amd.taxometric import TaxonomyIndex
    ds = _toy(tmp_path)
    n = int(ds.node_features.shape[0])
    parents = {v: list(ds.graph.pred.get(v, ())) for v in range(n)}
    tix = TaxonomyIndex.from_dataset(ds)
    for cand in (sorted(ds.all_positions), list(ds.graph.nodes)):
        ix = HedgeIndex.build(tix, cand)
        assert _rows(ix) == hc.brute_sub(parents, n, cand) and ix.G == len(cand) > 20
        assert ix.depth.tolist() == [hc.brute_depth(parents, n)[a] for a in cand]
    assert max(len(r) for r in _rows(ix)) > 10                      # (the toy has real subtrees)


def test_index_refuses_bad_candidate_lists():
    parents, n = hc.chain()
    tix = hc.index_of(parents, n)
    for cand in ([0, 1, 1], [0, n], [-1, 2]):
        with pytest.raises(ValueError):
            HedgeIndex.build(tix, cand)
    ix = HedgeIndex.build(tix, [])
    assert ix.G == 0 and ix.nnz == 0 and ix.n_items == 0 and ix.sub_ptr.tolist() == [0]


@pytest.mark.parametrize("case", ["chain", "star", "diamond", "forest"])
def test_host_mass_equals_fsum_over_the_sets(case):
    parents, n = getattr(hc, case)()
    cand = np.random.RandomState(2).permutation(n).tolist()
    ix = HedgeIndex.build(hc.index_of(parents, n), cand)
    P = hc.probabilities(7, n, seed=4)
    mass = hedge.host_subtree_mass(ix, P)
    assert mass.shape == (n, 7) and mass.dtype == np.float64
    sets = hc.brute_sub(parents, n, cand)
    for a in range(n):
        for q in range(7):
            assert abs(mass[a, q] - math.fsum(float(P[q, d]) for d in sets[a])) <= 1e-12


def test_host_mass_follows_the_literal_slice_order():
    """a row of 3 * SLICE + 5 entries: every slice summed left to right from 0.0, the slice sums added left to right -- bit for bit"""
    parents, n, who = hc.star_plus_chain(SLICE)
    ix = HedgeIndex.build(hc.index_of(parents, n), list(range(n)))
    P = hc.probabilities(3, n, seed=5, sharp=8.0)          # (a wide range: fp32 terms that a float64 sum cannot all hold exactly)
    mass = hedge.host_subtree_mass(ix, P)
    n_differs = 0
    for a in (who["root"], who["b"], who["c"], who["lone"]):
        row = ix.row(a).tolist()
        for q in range(3):
            sums = []
            for s0 in range(0, len(row), SLICE):
                acc = 0.0
                for d in row[s0:s0 + SLICE]:
                    acc = acc + float(P[q, d])
                sums.append(acc)
            tot = sums[0]
            for s in sums[1:]:
                tot = tot + s
            assert mass[a, q] == tot, (a, q)
            flat = 0.0
            for d in row:
                flat = flat + float(P[q, d])
            n_differs += flat != tot
    assert len(ix.row(who["root"])) == 3 * SLICE + 5
    assert n_differs > 0                        # (the order is observable: one flat left-to-right sum gives other bits somewhere)


def test_deepest_node_wins_on_a_chain():
    parents, n = hc.chain(4)
    ix = HedgeIndex.build(hc.index_of(parents, n), list(range(n)))
    P = np.asarray([[0.1, 0.2, 0.3, 0.4]], dtype=np.float32)
    h = hedge.host_hedge(ix, P, [0.35, 0.5, 0.8, 0.95])
    assert h.node_col.tolist() == [[3, 2, 1, 0]] and h.depth.tolist() == [[4, 3, 2, 1]]
    assert h.node_col.dtype == np.int32 and h.mass.dtype == np.float64 and h.depth.dtype == np.int32
    m = hedge.host_subtree_mass(ix, P)
    assert h.mass.tolist() == [[m[3, 0], m[2, 0], m[1, 0], m[0, 0]]]


def test_tie_rules():
    parents, n = hc.star(4)
    ix = HedgeIndex.build(hc.index_of(parents, n), list(range(n)))
    # equal depth: the larger mass
    h = hedge.host_hedge(ix, np.asarray([[0.0, 0.3, 0.4, 0.3]], dtype=np.float32), 0.25)
    assert h.node_col.tolist() == [[2]] and h.depth.tolist() == [[2]]
    # masses exactly equal: the smaller column
    P = np.asarray([[0.25, 0.375, 0.0, 0.375]], dtype=np.float32)
    h = hedge.host_hedge(ix, P, 0.375)
    assert h.node_col.tolist() == [[1]] and h.mass.tolist() == [[0.375]]
    # ... in a shuffled candidate order too: column, not node id, breaks the tie
    ix2 = HedgeIndex.build(hc.index_of(parents, n), [3, 0, 2, 1])
    h = hedge.host_hedge(ix2, P[:, [3, 0, 2, 1]], 0.375)
    assert h.node_col.tolist() == [[0]]


def test_threshold_one_on_exact_binary_fractions():
    parents = {1: [0], 2: [0], 3: [2]}
    ix = HedgeIndex.build(hc.index_of(parents, 4), [0, 1, 2, 3])
    P = np.asarray([[0.125, 0.125, 0.25, 0.5]], dtype=np.float32)
    h = hedge.host_hedge(ix, P, [1.0, 0.75, 0.5])
    assert h.node_col.tolist() == [[0, 2, 3]] and h.mass.tolist() == [[1.0, 0.75, 0.5]] and h.depth.tolist() == [[1, 2, 3]]


def test_forest_and_non_finite_lse_give_no_answer():
    parents, n = hc.forest()
    ix = HedgeIndex.build(hc.index_of(parents, n), list(range(n)))
    P = np.asarray([[0.2, 0.2, 0.15, 0.15, 0.1, 0.1, 0.1]], dtype=np.float32)          # 0.55 under root 0, 0.45 under root 3
    h = hedge.host_hedge(ix, P, [0.6, 0.5])
    assert h.node_col.tolist() == [[-1, 0]] and np.isnan(h.mass[0, 0]) and h.depth.tolist() == [[0, 1]]
    S = np.random.RandomState(0).standard_normal((4, n)).astype(np.float32)
    lse = np.asarray([np.nan, np.inf, -np.inf, 1.0])
    p = hedge.host_probabilities(S, lse, 0.7)
    assert p.dtype == np.float32 and not p[:3].any() and p[3].all()
    h = hedge.host_hedge(ix, p[:3], 0.01)
    assert (h.node_col == -1).all() and np.isnan(h.mass).all() and not h.depth.any()
    h = hedge.host_hedge(HedgeIndex.build(hc.index_of(parents, n), []), np.zeros((2, 0), dtype=np.float32), 0.5)
    assert h.node_col.tolist() == [[-1], [-1]]


def test_host_probabilities_follow_the_definition():
    from taxoexpan_amd import scoring
    S = np.random.RandomState(1).standard_normal((5, 9)).astype(np.float32) * 3
    for T, larger in ((1.0, True), (0.6, False)):
        lse = scoring.host_score_moments(S, T, larger).lse
        p = hedge.host_probabilities(S, lse, T, larger)
        beta = np.float32(1.0 / T)
        for q in range(5):
            for g in range(9):
                t = np.float32(beta * (S[q, g] if larger else -S[q, g]))
                want = np.float32(math.exp(float(t) - lse[q]))     # (two exp routines: equal or neighbouring fp32 values)
                assert abs(float(p[q, g]) - float(want)) <= float(np.spacing(want)), (q, g)
        assert np.abs(p.astype(np.float64).sum(1) - 1.0).max() < 1e-6


def test_several_thresholds_equal_single_threshold_calls():
    parents, n, _who = hc.star_plus_chain(8)
    ix = HedgeIndex.build(hc.index_of(parents, n), list(range(n)))
    P = hc.probabilities(20, n, seed=9)
    thr = [0.05, 0.2, 0.5, 0.9, 1.0, 0.3, 0.7, 0.01]
    h = hedge.host_hedge(ix, P, thr)
    mass = hedge.host_subtree_mass(ix, P)
    for t, tau in enumerate(thr):
        one = hedge.host_hedge(ix, None, tau, mass=mass)
        assert np.array_equal(one.node_col[:, 0], h.node_col[:, t]) and np.array_equal(one.depth[:, 0], h.depth[:, t])
        assert np.array_equal(one.mass[:, 0], h.mass[:, t], equal_nan=True)
    assert len({tuple(r) for r in h.node_col.tolist()}) > 1


@pytest.mark.parametrize("bad", [0.0, -0.1, 1.0000001, float("nan"), float("inf"), [], [0.5] * 9, [0.5, 2.0], "0.5", None, True])
def test_thresholds_are_validated(bad):
    with pytest.raises(ValueError):
        hedge.check_thresholds(bad)
    parents, n = hc.chain()
    ix = HedgeIndex.build(hc.index_of(parents, n), list(range(n)))
    with pytest.raises(ValueError):
        hedge.host_hedge(ix, hc.probabilities(2, n), bad)
    if bad is not None:
        with pytest.raises(ValueError):                 # before the model, the dataset or the device are looked at
            from taxoexpan_amd.evaluate import evaluate
            evaluate(None, None, "cpu", hedge=bad)
        with pytest.raises(ValueError):
            from taxoexpan_amd.evaluate import infer
            infer(None, None, None, "cpu", with_scores=True, hedge=bad)


def test_thresholds_accepted_forms():
    assert hedge.check_thresholds(0.5) == [0.5] and hedge.check_thresholds((0.5, 1.0)) == [0.5, 1.0]
    assert hedge.check_thresholds(np.asarray([0.25, 0.75])) == [0.25, 0.75] and len(hedge.check_thresholds([0.1] * 8)) == 8
    assert hedge.MAX_THRESHOLDS == 8 and SLICE >= 2 and SLICE & (SLICE - 1) == 0


def test_keyword_combinations_raise_before_any_device_call():
    from taxoexpan_amd.evaluate import evaluate, infer
    with pytest.raises(ValueError, match="retrieve"):
        evaluate(None, None, "cpu", retrieve=5, hedge=0.5)
    with pytest.raises(ValueError, match="thresholds"):
        evaluate(None, None, "cpu", hedge={})
    with pytest.raises(ValueError, match="with_scores"):
        infer(None, None, None, "cpu", hedge=0.9)
    with pytest.raises(ValueError):
        infer(None, None, None, "cpu", with_scores=True, retrieve=5, hedge=0.9)
    parents, n = hc.chain()
    ix = HedgeIndex.build(hc.index_of(parents, n), list(range(n)))
    with pytest.raises(TypeError):
        hedge.subtree_mass(ix, torch.zeros(n, 2))                       # a host index
    with pytest.raises(TypeError):
        hedge.hedged_parents(None, torch.zeros(n, 3), torch.zeros(2, 3), ix, 0.5)


def test_slice_constant_is_the_header():
    import re
    from taxoexpan_amd import _lib
    hdr = open(os.path.join(os.path.dirname(GOLDEN_DIR), "..", "include", "txe.h")).read()
    assert int(re.search(r"#define TXE_HEDGE_SLICE (\d+)", hdr).group(1)) == SLICE == _lib.HEDGE_SLICE
    assert int(re.search(r"#define TXE_HEDGE_MAX_THRESHOLDS (\d+)", hdr).group(1)) == hedge.MAX_THRESHOLDS


def test_entry_point_argument_checks_need_no_gpu():
    """error codes before anything is launched; nq == 0 or G == 0 return TXE_OK without a device call"""
    from taxoexpan_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    thr = (ctypes.c_double * 8)(0.5, 0.9, 1.0, 0.1, 0.2, 0.3, 0.4, 0.6)
    t = ctypes.addressof(thr)
    probs = lambda S=a, ldS=8, nq=2, G=8, lse=a, beta=1.0, PT=a, ldq=64: lib.txe_hedge_probs(S, ldS, nq, G, lse, beta, 0, PT, ldq, None)
    assert probs(nq=0) == 0 and probs(G=0, ldS=0) == 0 and probs(nq=0, S=None, lse=None, PT=None) == 0
    for kw in (dict(nq=-1), dict(G=-1), dict(beta=0.0), dict(beta=float("nan")), dict(beta=float("inf")), dict(S=None), dict(lse=None),
               dict(PT=None), dict(ldS=7), dict(ldq=1)):
        assert probs(**kw) == -1, kw

    def sweep(G=4, nnz=4, n_items=4, n_long=0, n_part=0, PT=a, ldq=64, nq=2, thresholds=t, n_thr=2, mass=a, ldm=2, out=a, ws=a, ws_bytes=0,
              sub=a):
        return lib.txe_hedge_sweep(sub, a, a, G, nnz, a, a, a, n_items, a, a, n_long, n_part, PT, ldq, nq, thresholds, n_thr, mass, ldm, out,
                                   out, out, ws, ws_bytes, None)
    assert sweep(nq=0) == 0 and sweep(G=0) == 0 and sweep(nq=0, n_thr=0) == 0
    for kw in (dict(nq=-1), dict(G=-1), dict(nnz=-1), dict(n_items=-1), dict(n_long=-1), dict(n_part=-1), dict(n_thr=9), dict(n_thr=-1),
               dict(thresholds=None), dict(sub=None), dict(PT=None), dict(ldq=1), dict(out=None), dict(n_thr=0, mass=None),
               dict(n_thr=0, ldm=1)):
        assert sweep(**kw) == -1, kw
    for bad in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        thr2 = (ctypes.c_double * 2)(0.5, bad)
        assert sweep(thresholds=ctypes.addressof(thr2)) == -1, bad
        assert sweep(thresholds=ctypes.addressof(thr2), nq=0) == -1, bad        # (the thresholds are checked before the empty-shape return)
    assert sweep() == -3 and sweep(ws=None, ws_bytes=1 << 30) == -3 and sweep(n_thr=0) == -3
    need = lib.txe_hedge_sweep_ws_bytes(4, 0, 0, 2, 2)
    assert need > 0 and lib.txe_hedge_sweep_ws_bytes(4, 2, 6, 130, 0) >= 6 * 192 * 8 and lib.txe_hedge_sweep_ws_bytes(4, 0, 0, 2, 9) == 0
    assert sweep(ws_bytes=need - 1) == -3
