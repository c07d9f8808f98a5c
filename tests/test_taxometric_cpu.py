"""CPU: the taxonomy index (longest-path depth, ancestor closure) and the numpy restatement of the taxonomy-aware evaluation
(taxoexpan_amd/taxometric.py) against a brute force written here from the definitions alone: upward BFS with Python sets
from the parent lists, longest-path depth by recursion, Wu & Palmer as exact fractions."""
import ctypes
import os
import shutil
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest

from golden_util import GOLDEN_DIR
from taxoexpan_amd import taxometric  # noqa: F401  (the feature under test: without it nothing here can run)
from taxoexpan_amd.synthetic import make_taxonomy


# ---- taxonomies: (par_ptr, par_idx) ---------------------------------------------------------------------------------------------
def _csr(par_lists):
    ptr = np.concatenate([[0], np.cumsum([len(p) for p in par_lists])]).astype(np.int64)
    return ptr, np.asarray([p for row in par_lists for p in row], dtype=np.int64)


def _lists(ptr, idx):
    return [[int(p) for p in idx[ptr[v]:ptr[v + 1]]] for v in range(len(ptr) - 1)]


def _synthetic(n, e, seed):
    t = make_taxonomy(n, e, 8, seed=seed, features=False)
    return _lists(t.par_ptr, t.par_idx)


def _forest():
    """two DAGs side by side: the only place where a pair has no common ancestor"""
    a, b = _synthetic(60, 90, 3), _synthetic(60, 90, 4)
    return a + [[p + 60 for p in row] for row in b]


TAXONOMIES = {
    "single": [[]],
    "chain": [[]] + [[i - 1] for i in range(1, 130)],                # ancestor lists up to 130: more than two strides of a whole wave
    "diamond": [[], [0], [0], [1, 2], [3]],
    "star": [[]] + [[0]] * 200,                                      # 200 siblings with ancestor lists of length 2
    "dag40": _synthetic(40, 60, 5),
    "forest": _forest(),
}


# ---- the brute force ------------------------------------------------------------------------------------------------------------
class Brute:
    def __init__(self, par_lists):
        self.par = par_lists
        self.n = len(par_lists)

        @lru_cache(maxsize=None)
        def depth(v):
            return 1 + max((depth(p) for p in par_lists[v]), default=0)
        self.depth = [depth(v) for v in range(self.n)]
        self.anc = []
        for v in range(self.n):
            seen, todo = {v}, [v]
            while todo:
                for p in par_lists[todo.pop()]:
                    if p not in seen:
                        seen.add(p)
                        todo.append(p)
            self.anc.append(seen)

    def lca_depth(self, a, b):
        return max((self.depth[c] for c in self.anc[a] & self.anc[b]), default=0)

    def relation(self, a, b):
        if a == b:
            return 0
        if a in self.anc[b]:
            return 1
        if b in self.anc[a]:
            return 2
        if set(self.par[a]) & set(self.par[b]):
            return 3
        return 4 if self.anc[a] & self.anc[b] else 5

    def slots(self, pred, gold_off, gold_idx):
        """(lca_depth, best_gold, relation, wup as Fractions) per slot, from the definitions"""
        Q, K = pred.shape
        l_out, j_out, r_out = np.zeros((Q, K), np.int32), np.full((Q, K), -1, np.int32), np.full((Q, K), 6, np.int32)
        w_out = [[Fraction(0)] * K for _ in range(Q)]
        for q in range(Q):
            golds = [int(g) for g in gold_idx[gold_off[q]:gold_off[q + 1]]]
            for r in range(K):
                a = int(pred[q, r])
                if not 0 <= a < self.n or not golds:
                    continue
                cands = []
                for j, b in enumerate(golds):
                    l = self.lca_depth(a, b)
                    cands.append((-Fraction(2 * l, self.depth[a] + self.depth[b]), self.relation(a, b), j, l))
                w, rel, j, l = min(cands)                            # largest wup, then the smaller code, then the smaller j
                l_out[q, r], j_out[q, r], r_out[q, r], w_out[q][r] = l, j, rel, -w
        return l_out, j_out, r_out, w_out


def _index(name):
    from taxoexpan_amd.taxometric import TaxonomyIndex
    return TaxonomyIndex.from_parents(*_csr(TAXONOMIES[name]))


def random_lists(n, Q, K, seed, max_gold=3, min_gold=1, bad_pred=0.0, ends=False):
    """pred [Q, K], gold_off, gold_idx: random node ids, gold lists of min_gold..max_gold entries; bad_pred: the share of predictions
    replaced by ids outside [0, n); ends: half of all ids are the first or the last node (the chain: lists of 1 and of n)"""
    rs = np.random.RandomState(seed)
    draw = lambda size: np.where(rs.uniform(size=size) < 0.5, rs.choice([0, n - 1], size=size), rs.randint(0, n, size=size)) if ends \
        else rs.randint(0, n, size=size)
    pred = draw((Q, K)).astype(np.int64)
    if bad_pred:
        bad = rs.uniform(size=(Q, K)) < bad_pred
        pred[bad] = rs.choice([-1, n, n + 5, -7, 2 ** 31 - 1], size=int(bad.sum()))
    cnt = rs.randint(min_gold, max_gold + 1, size=Q)
    gold_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    return pred, gold_off, draw(int(cnt.sum())).astype(np.int64)


# ---- the index ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TAXONOMIES))
def test_index_equals_the_brute_force(name):
    par = TAXONOMIES[name]
    brute, ix = Brute(par), _index(name)
    assert ix.n_nodes == len(par) and ix.depth.dtype == ix.anc_ptr.dtype == ix.anc_idx.dtype == np.int32
    assert ix.depth.tolist() == brute.depth
    assert ix.anc_ptr[0] == 0 and ix.anc_ptr[-1] == ix.anc_idx.size == sum(len(s) for s in brute.anc)
    for v in range(len(par)):
        row = ix.ancestors(v).tolist()
        assert row == sorted(brute.anc[v]) and v in row and all(x < y for x, y in zip(row, row[1:])), v
        assert ix.parents(v).tolist() == sorted(set(par[v]))
        assert all(brute.depth[c] < brute.depth[v] for c in brute.anc[v] if c != v)      # why depth is the longest path
    if name == "dag40":
        assert sum(len(p) > 1 for p in par) == 11 and max(brute.depth) <= 6
    if name == "chain":
        assert ix.anc_ptr[-1] - ix.anc_ptr[-2] == 130


def test_index_refuses_cycles_bad_ids_and_an_oversized_closure(monkeypatch):
    from taxoexpan_amd import taxometric
    from taxoexpan_amd.taxometric import TaxonomyIndex
    with pytest.raises(ValueError, match="cycle"):
        TaxonomyIndex.from_parents(*_csr([[2], [0], [1]]))
    with pytest.raises(ValueError, match="cycle"):
        TaxonomyIndex.from_parents(*_csr([[], [1]]))
    with pytest.raises(ValueError, match="cycle"):
        TaxonomyIndex.from_parents(*_csr([[], [0], [1, 4], [2], [3]]))   # a cycle below a sound root
    with pytest.raises(ValueError, match="outside"):
        TaxonomyIndex.from_parents(*_csr([[], [2]]))
    with pytest.raises(ValueError):
        TaxonomyIndex.from_parents([0, 2], [0])
    monkeypatch.setattr(taxometric, "MAX_CLOSURE", 130 * 131 // 2)      # the chain's closure has exactly this many entries
    with pytest.raises(ValueError, match="closure"):
        _index("chain")
    monkeypatch.setattr(taxometric, "MAX_CLOSURE", 130 * 131 // 2 + 1)
    assert _index("chain").anc_idx.size == 130 * 131 // 2


def test_unsorted_and_repeated_parent_rows():
    from taxoexpan_amd.taxometric import TaxonomyIndex
    ix = TaxonomyIndex.from_parents(*_csr([[], [0], [0], [2, 1, 2]]))
    assert ix.parents(3).tolist() == [1, 2] and ix.ancestors(3).tolist() == [0, 1, 2, 3] and ix.depth.tolist() == [1, 2, 2, 3]


# ---- host_taxonomic against the brute force -------------------------------------------------------------------------------------
def _dag40_inputs():
    """all 40 x 40 pairs: query q's list is every node, its first gold is q itself; 0-2 more golds"""
    rs = np.random.RandomState(11)
    pred = np.tile(np.arange(40, dtype=np.int64), (40, 1))
    golds = [[q] + rs.randint(0, 40, size=rs.randint(0, 3)).tolist() for q in range(40)]
    return pred, np.concatenate([[0], np.cumsum([len(g) for g in golds])]).astype(np.int64), np.asarray([g for row in golds for g in row])


def _forest_inputs():
    """Q = 120, K = 8: random slots, the query itself as slot 0 of every third query, predictions outside [0, n) and a query
    without golds"""
    pred, off, idx = random_lists(120, 120, 8, seed=2)
    pred[::3, 0] = idx[off[:-1][::3]]
    pred[5, 2], pred[6, 0], pred[9, 7] = -1, 120, 2 ** 31 - 1
    cut = slice(off[7], off[8])
    idx = np.delete(idx, np.arange(cut.start, cut.stop))
    off = off.copy()
    off[8:] -= cut.stop - cut.start
    assert off[7] == off[8]
    return pred, off, idx


def _check_against_brute(name, pred, off, idx, codes):
    from taxoexpan_amd.taxometric import best_gold_nodes, host_taxonomic, wu_palmer
    brute, ix = Brute(TAXONOMIES[name]), _index(name)
    l, j, rel, w = brute.slots(pred, off, idx)
    assert set(codes) <= set(np.unique(rel).tolist()), np.bincount(rel.reshape(-1), minlength=7)      # the inputs cover the codes
    got = host_taxonomic(ix, pred, off, idx)
    assert all(got[k].dtype == np.int32 and got[k].shape == pred.shape for k in ("lca_depth", "best_gold", "relation"))
    assert np.array_equal(got["lca_depth"], l) and np.array_equal(got["best_gold"], j) and np.array_equal(got["relation"], rel)
    wup = wu_palmer(ix, pred, best_gold_nodes(got["best_gold"], off, idx), got["lca_depth"])
    assert wup.dtype == np.float64 and wup.shape == pred.shape
    want = np.asarray([[float(x) for x in row] for row in w])        # one correctly rounded quotient either way
    assert np.array_equal(wup, want)
    return got, wup


def test_host_taxonomic_on_all_pairs_of_the_dag():
    pred, off, idx = _dag40_inputs()
    assert pred.shape == (40, 40) and 1 <= np.diff(off).min() and np.diff(off).max() <= 3
    _check_against_brute("dag40", pred, off, idx, codes=(0, 1, 2, 3, 4))


def test_host_taxonomic_on_the_forest_with_bad_slots():
    pred, off, idx = _forest_inputs()
    got, wup = _check_against_brute("forest", pred, off, idx, codes=(0, 1, 2, 3, 4, 5, 6))
    for q, r in ((5, 2), (6, 0), (9, 7)):
        assert (got["relation"][q, r], got["lca_depth"][q, r], got["best_gold"][q, r], wup[q, r]) == (6, 0, -1, 0.0)
    assert (got["relation"][7] == 6).all() and (got["best_gold"][7] == -1).all() and (wup[7] == 0).all()


@pytest.mark.parametrize("name", ["single", "chain", "diamond", "star"])
def test_host_taxonomic_on_the_small_shapes(name):
    n = len(TAXONOMIES[name])
    pred, off, idx = random_lists(n, 40, 6, seed=3, max_gold=2, min_gold=0, bad_pred=0.1, ends=name in ("chain", "star"))
    codes = {"single": (0, 6), "chain": (0, 1, 2, 6), "diamond": (0, 1, 2, 3, 6), "star": (0, 1, 2, 3, 6)}[name]
    _check_against_brute(name, pred, off, idx, codes)


def test_gold_ids_outside_the_taxonomy_are_skipped():
    from taxoexpan_amd.taxometric import host_taxonomic
    ix = _index("diamond")
    got = host_taxonomic(ix, np.asarray([[3], [3]]), [0, 3, 5], [-1, 1, 99, 5, -2])
    assert got["best_gold"].tolist() == [[1], [-1]] and got["relation"].tolist() == [[2], [6]] and got["lca_depth"].tolist() == [[2], [0]]


# ---- properties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dag40", "forest", "chain"])
def test_wu_palmer_properties(name):
    from taxoexpan_amd.taxometric import best_gold_nodes, host_taxonomic, wu_palmer
    ix = _index(name)
    n = ix.n_nodes
    pred, off, idx = random_lists(n, 60, 6, seed=9, ends=name == "chain")
    pred[::4, 1] = idx[off[:-1][::4]]
    got = host_taxonomic(ix, pred, off, idx)
    wup = wu_palmer(ix, pred, best_gold_nodes(got["best_gold"], off, idx), got["lca_depth"])
    assert (wup >= 0).all() and (wup <= 1).all()
    in_gold = np.asarray([[pred[q, r] in idx[off[q]:off[q + 1]] for r in range(pred.shape[1])] for q in range(pred.shape[0])])
    assert in_gold.any() and not in_gold.all()
    assert np.array_equal(wup == 1.0, in_gold) and np.array_equal(got["relation"] == 0, in_gold)
    # lca_depth(a, b) == lca_depth(b, a): every slot against a single gold, then the two swapped
    rs = np.random.RandomState(4)
    a, b = rs.randint(0, n, size=(300, 1)), rs.randint(0, n, size=300)
    one = np.arange(301)
    ab, ba = host_taxonomic(ix, a, one, b), host_taxonomic(ix, b[:, None], one, a[:, 0])
    assert np.array_equal(ab["lca_depth"], ba["lca_depth"])
    swapped = np.asarray([0, 2, 1, 3, 4, 5, 6])[ab["relation"]]              # too general <-> too specific
    assert np.array_equal(ba["relation"], swapped)


def test_summarize_on_numpy():
    from taxoexpan_amd.taxometric import summarize
    rel = np.asarray([[0, 4], [1, 0], [5, 5], [6, 6], [0, 1]], dtype=np.int32)
    wup = np.asarray([[1.0, 0.5], [0.8, 1.0], [0.0, 0.0], [0.0, 0.0], [1.0, 0.4]])
    m = summarize(rel, wup)
    assert m["taxonomic_k"] == 2 and m["wu_palmer"] == (1.0 + 0.8 + 0.0 + 0.0 + 1.0) / 5 and m["wu_palmer_at_k"] == (1.0 + 1.0 + 0.0 + 0.0 + 1.0) / 5
    shares = [m["rel_" + k] for k in ("exact", "ancestor", "descendant", "sibling", "related", "unrelated", "none")]
    assert shares == [2 / 5, 1 / 5, 0.0, 0.0, 0.0, 1 / 5, 1 / 5] and sum(shares) == 1.0
    assert np.isnan(summarize(rel[:0], wup[:0])["wu_palmer"])


# ---- the toy dataset ------------------------------------------------------------------------------------------------------------
def test_from_dataset_reads_the_masked_taxonomy(tmp_path):
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    from taxoexpan_amd.taxometric import TaxonomyIndex
    for fn in os.listdir(os.path.join(GOLDEN_DIR, "toy_taxo")):
        shutil.copy(os.path.join(GOLDEN_DIR, "toy_taxo", fn), tmp_path)
    ds = MaskedGraphDataset(MAGDataset("toy", str(tmp_path), raw=True), mode="test", sampling_mode=0, expand_factor=100, normalize_embed=True)
    got = TaxonomyIndex.from_dataset(ds)
    dtax = ds.device_taxonomy("cpu")
    want = TaxonomyIndex.from_parents(dtax.par_ptr.numpy(), dtax.par_idx.numpy())
    assert got.n_nodes == ds.node_features.shape[0] > 0
    for k in ("depth", "anc_ptr", "anc_idx", "par_ptr", "par_idx"):
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    brute = Brute([list(ds.graph.pred.get(v, ())) for v in range(got.n_nodes)])
    assert got.depth.tolist() == brute.depth and max(brute.depth) >= 3
    assert all(got.depth[q] == 1 for q in ds.node_list)              # held-out queries lost their in-edges: they are not in the tree


# ---- the C entry point's argument checks (nothing is launched) -------------------------------------------------------------------
def test_entry_point_argument_validation_needs_no_gpu():
    from taxoexpan_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int * 16)()
    a = ctypes.addressof(buf)
    ok = [a, a, a, a, a, 4, a, 0, 3, a, a, 2, a, a, a, None]
    assert lib.txe_taxo_slots(*ok) == 0                              # Q == 0: no launch
    for i in (0, 1, 2, 3, 4, 6, 9, 10, 12, 13, 14):
        bad = list(ok)
        bad[i] = None
        assert lib.txe_taxo_slots(*bad) == -1, i
    for i, v in ((8, 0), (7, -1), (5, -1), (11, -1)):
        bad = list(ok)
        bad[i] = v
        assert lib.txe_taxo_slots(*bad) == -1, (i, v)
    big = list(ok)
    big[7], big[8] = 2 ** 16, 2 ** 15                                # Q K = 2^31
    assert lib.txe_taxo_slots(*big) == -1
