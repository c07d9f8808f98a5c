"""GPU: the taxonomy-aware evaluation kernel (csrc/txe_taxometric.hip) against its numpy restatement, integer for integer, and
evaluate(taxonomic=...) on the toy taxonomy against the same restatement on the lists it judged."""
import os
import shutil

import numpy as np
import pytest
import torch

from golden_util import GOLDEN_DIR
from taxoexpan_amd import taxometric  # noqa: F401  (the feature under test: without it nothing here can run)
from test_taxometric_cpu import TAXONOMIES, _csr, random_lists

pytestmark = pytest.mark.gpu

INT_KEYS = ("lca_depth", "best_gold", "relation")
TAXO_KEYS = {"wu_palmer", "wu_palmer_at_k", "taxonomic_k", "rel_exact", "rel_ancestor", "rel_descendant", "rel_sibling", "rel_related",
             "rel_unrelated", "rel_none"}


def _dev():
    return torch.device("cuda:0")


_INDEX = {}


def _index(name):
    """(host index, resident index) of a test taxonomy, built once"""
    from taxoexpan_amd.taxometric import TaxonomyIndex
    if name not in _INDEX:
        host = TaxonomyIndex.from_parents(*_csr(TAXONOMIES[name]))
        _INDEX[name] = (host, host.to(_dev()))
    return _INDEX[name]


@pytest.mark.parametrize("Q,K", [(1, 1), (3, 8), (37, 5), (64, 64)])
@pytest.mark.parametrize("name", list(TAXONOMIES))
def test_slots_equal_the_host_restatement(name, Q, K):
    from taxoexpan_amd.taxometric import best_gold_nodes, host_taxonomic, taxonomic_slots, wu_palmer
    host, dev = _index(name)
    n = host.n_nodes
    pred, off, idx = random_lists(n, Q, K, seed=Q * 100 + K, max_gold=4, min_gold=0, bad_pred=0.1, ends=name in ("chain", "star"))
    if name == "chain" and Q >= 3:                                    # lists of 1 and of 130 on either side
        pred[0, 0], pred[1, 0] = 0, n - 1
        idx[off[0]:off[1]] = n - 1
        idx[off[1]:off[2]] = 0
    want = host_taxonomic(host, pred, off, idx)
    p = torch.from_numpy(pred).to(_dev())
    got = taxonomic_slots(dev, p, off, idx)
    again = taxonomic_slots(dev, p, off, idx)
    as_int32 = taxonomic_slots(dev, p.to(torch.int32), torch.from_numpy(off), torch.from_numpy(idx))
    for k in INT_KEYS:
        assert got[k].dtype == torch.int32 and got[k].shape == (Q, K) and got[k].device == p.device
        assert np.array_equal(got[k].cpu().numpy(), want[k]), (k, np.argwhere(got[k].cpu().numpy() != want[k])[:5])
        assert torch.equal(got[k], again[k]) and torch.equal(got[k], as_int32[k]), k
    if (Q, K) == (64, 64) and name not in ("single",):
        assert (want["relation"] == 6).any() and (want["relation"] < 6).any()
    w_dev = wu_palmer(dev, p, best_gold_nodes(got["best_gold"], off, idx), got["lca_depth"])
    w_host = wu_palmer(host, pred, best_gold_nodes(want["best_gold"], off, idx), want["lca_depth"])
    assert w_dev.dtype == torch.float64 and np.array_equal(w_dev.cpu().numpy(), w_host)      # bit for bit


def test_slots_refuse_bad_golds_and_host_tensors():
    from taxoexpan_amd.taxometric import taxonomic_slots
    host, dev = _index("diamond")
    p = torch.zeros((2, 3), dtype=torch.int32, device=_dev())
    for idx in ([0, 5], [-1, 0]):
        with pytest.raises(ValueError, match="gold id"):
            taxonomic_slots(dev, p, [0, 1, 2], idx)
    with pytest.raises(ValueError, match="gold_off"):
        taxonomic_slots(dev, p, [0, 1], [0, 1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        taxonomic_slots(dev, p.cpu(), [0, 1, 2], [0, 1])
    with pytest.raises(TypeError):
        taxonomic_slots(host, p, [0, 1, 2], [0, 1])


# ---- evaluate(taxonomic=...) ----------------------------------------------------------------------------------------------------
def _toy(tmp_path):
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    for fn in os.listdir(os.path.join(GOLDEN_DIR, "toy_taxo")):
        shutil.copy(os.path.join(GOLDEN_DIR, "toy_taxo", fn), tmp_path)
    return MaskedGraphDataset(MAGDataset("toy", str(tmp_path), raw=True), mode="test", sampling_mode=0, expand_factor=100, normalize_embed=True)


def _model(match):
    from taxoexpan_amd import TaxoExpan
    torch.manual_seed(11)
    return TaxoExpan("PGAT", "WMR", match, in_dim=8, hidden_dim=6, out_dim=5, pos_dim=3, num_layers=1, heads=[2, 1], feat_drop=0.1,
                     attn_drop=0.1, hidden_drop=0.1, out_drop=0.1).to(_dev()).eval()


def _golds(ds, queries):
    cand = set(ds.all_positions)
    lists = [[a for a in ds.node2parents[q] if a in cand] for q in queries]
    return np.concatenate([[0], np.cumsum([len(g) for g in lists])]).astype(np.int64), np.asarray([a for g in lists for a in g], dtype=np.int64)


def _check_tensors_and_metrics(ds, host, d, metrics, queries, pos_off):
    """the dict's integer tensors = host_taxonomic on d["pred"]; shares exactly, the two means within 1e-12 of a float64 recomputation
    (the only freedom is the summation order over at most a few thousand values in [0, 1])"""
    from taxoexpan_amd.taxometric import best_gold_nodes, host_taxonomic, wu_palmer
    off, idx = _golds(ds, queries)
    assert np.array_equal(off, pos_off)
    pred = d["pred"].cpu().numpy()
    Q, K = pred.shape
    assert Q == len(queries) and metrics["taxonomic_k"] == K
    want = host_taxonomic(host, pred, off, idx)
    for k in INT_KEYS:
        assert d[k].dtype == torch.int32 and d[k].is_cuda and np.array_equal(d[k].cpu().numpy(), want[k]), k
    wup = wu_palmer(host, pred, best_gold_nodes(want["best_gold"], off, idx), want["lca_depth"])
    assert d["wu_palmer"].dtype == torch.float64 and np.array_equal(d["wu_palmer"].cpu().numpy(), wup)
    names = ("exact", "ancestor", "descendant", "sibling", "related", "unrelated", "none")
    counts = np.bincount(want["relation"][:, 0], minlength=7)
    for c, name in zip(counts, names):
        assert metrics["rel_" + name] == float(c) / Q, name
    assert abs(sum(metrics["rel_" + name] for name in names) - 1.0) < 1e-15
    w0, wk = float(np.sum(wup[:, 0])) / Q, float(np.sum(wup.max(axis=1))) / Q
    print(f"[taxometric] Q {Q} K {K} wu_palmer {metrics['wu_palmer']!r} numpy {w0!r}  at_k {metrics['wu_palmer_at_k']!r} numpy {wk!r}  "
          f"relations {counts.tolist()}")
    assert abs(metrics["wu_palmer"] - w0) <= 1e-12 and abs(metrics["wu_palmer_at_k"] - wk) <= 1e-12
    assert metrics["wu_palmer_at_k"] >= metrics["wu_palmer"] - 1e-12
    return want, wup


@pytest.mark.parametrize("topk", [1, 5])
@pytest.mark.parametrize("match,larger", [("BIM", True), ("MLP", True), ("BIM", False)])
def test_evaluate_taxonomic_on_the_toy_taxonomy(tmp_path, match, larger, topk):
    from taxoexpan_amd import scoring
    from taxoexpan_amd.evaluate import CASE_METRICS, candidate_graphs, evaluate
    from taxoexpan_amd.taxometric import TaxonomyIndex
    ds = _toy(tmp_path)
    model = _model(match)
    host = TaxonomyIndex.from_dataset(ds)
    m0, r0, off0, q0 = evaluate(model, ds, _dev(), larger_is_better=larger, topk=topk)
    d = {}
    m1, r1, off1, q1 = evaluate(model, ds, _dev(), larger_is_better=larger, topk=topk, taxonomic=d)
    assert set(m1) == set(m0) | TAXO_KEYS and {k: v for k, v in m1.items() if k not in TAXO_KEYS} == m0
    assert torch.equal(r0, r1) and np.array_equal(off0, off1) and q0 == q1 and r0.dtype == r1.dtype
    assert set(d) == {"pred", "wu_palmer"} | set(INT_KEYS)
    # the list: the stable descending (ascending for a loss that is not info_nce) argsort of the score matrix, through the candidates
    cand = np.asarray(sorted(ds.all_positions), dtype=np.int64)
    with torch.no_grad():
        hg = scoring.encode_candidates(model, candidate_graphs(ds.device_taxonomy(_dev()), cand, ds.expand_factor, 0))
        S = scoring.score_all(model.match, hg, ds.node_features[torch.as_tensor(q1, dtype=torch.long)].to(_dev())).cpu().numpy()
    key = S if larger else -S
    order = np.argsort(-key, axis=1, kind="stable")[:, :topk]
    assert d["pred"].shape == (len(q1), topk) and np.array_equal(d["pred"].cpu().numpy(), cand[order])
    want, wup = _check_tensors_and_metrics(ds, host, d, m1, q1, off1)
    # a resident index given by the caller, and a plain True, give the same numbers
    m2 = evaluate(model, ds, _dev(), larger_is_better=larger, topk=topk, taxonomic=True, taxonomy_index=host.to(_dev()))[0]
    assert m2 == m1
    # against the ranks: where the best score is untied, the first prediction is a gold parent exactly when a rank is 1
    top2 = -np.sort(-key, axis=1)[:, :2]
    untied = top2[:, 0] > top2[:, 1]
    best_rank = np.asarray([r1.cpu().numpy()[off1[i]:off1[i + 1]].min() for i in range(len(q1))])
    assert untied.any()
    assert np.array_equal(want["relation"][untied, 0] == 0, best_rank[untied] == 1)
    # the case study: the column only when it is named
    rows0, rows1, rows2 = [], [], []
    evaluate(model, ds, _dev(), larger_is_better=larger, topk=topk, case=rows0)
    evaluate(model, ds, _dev(), larger_is_better=larger, topk=topk, case=rows1, taxonomic=True)
    evaluate(model, ds, _dev(), larger_is_better=larger, topk=topk, case=rows2, taxonomic=True, metric_names=CASE_METRICS + ("wu_palmer",))
    assert rows1 == rows0 and rows0[0][-1] != "wu_palmer"
    assert [row[:-1] for row in rows2] == rows0 and rows2[0][-1] == "wu_palmer"
    assert [row[-1] for row in rows2[1:]] == [str(float(v)) for v in wup[:, 0]]
    with pytest.raises(ValueError, match="wu_palmer"):
        evaluate(model, ds, _dev(), case=[], metric_names=("macro_mr", "wu_palmer"))


@pytest.mark.parametrize("topk", [1, 5])
@pytest.mark.parametrize("match", ["BIM", "MLP"])
def test_evaluate_taxonomic_with_retrieval(tmp_path, match, topk):
    from taxoexpan_amd.evaluate import evaluate
    from taxoexpan_amd.taxometric import TaxonomyIndex
    ds = _toy(tmp_path)
    model = _model(match)
    host = TaxonomyIndex.from_dataset(ds)
    m0, r0, off0, q0 = evaluate(model, ds, _dev(), topk=topk, retrieve=8)
    d, rows, rows0 = {}, [], []
    m1, r1, off1, q1 = evaluate(model, ds, _dev(), topk=topk, retrieve=8, taxonomic=d, case=rows)
    evaluate(model, ds, _dev(), topk=topk, retrieve=8, case=rows0)
    assert set(m1) == set(m0) | TAXO_KEYS and {k: v for k, v in m1.items() if k not in TAXO_KEYS} == m0
    assert torch.equal(r0, r1) and np.array_equal(off0, off1) and q0 == q1 and rows == rows0
    assert d["pred"].shape == (len(q1), min(topk, 8))
    _check_tensors_and_metrics(ds, host, d, m1, q1, off1)
    # the list the case study shows is the list that was judged
    pred = d["pred"].cpu().tolist()
    assert [row[2] for row in rows[1:]] == [", ".join(ds.vocab[a] for a in p if a >= 0) for p in pred]
