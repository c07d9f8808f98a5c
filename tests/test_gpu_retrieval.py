"""GPU: the retrieval stage (csrc/txe_retrieve.hip, scoring.retrieve_candidates) and the retrieve-then-rank protocol of
data_loader/dataset.py:316-330 in evaluate(retrieve=k) / infer(retrieve=k), against the host restatement (scoring.host_retrieve /
host_select_k, pinned to the reference's sampler by tests/test_retrieval_cpu.py) and ranks recomputed on the host."""
import os
import shutil

import numpy as np
import pytest
import torch

from golden_util import GOLDEN_DIR
from test_retrieval_cpu import MIN_GAP, sorted_pool_gaps, toy_masks

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _toy(tmp_path, normalize_embed=True):
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    for fn in os.listdir(os.path.join(GOLDEN_DIR, "toy_taxo")):
        shutil.copy(os.path.join(GOLDEN_DIR, "toy_taxo", fn), tmp_path)
    return MaskedGraphDataset(MAGDataset("toy", str(tmp_path), raw=True), mode="test", sampling_mode=0, expand_factor=100,
                              normalize_embed=normalize_embed)


def _model(match):
    """the toy model; "NTN" (a matcher model.py never builds, without a fused route) replaces the LBM module of one"""
    from taxoexpan_amd import TaxoExpan, model_zoo
    torch.manual_seed(11)
    model = TaxoExpan("PGAT", "WMR", "LBM" if match == "NTN" else match, in_dim=8, hidden_dim=6, out_dim=5, pos_dim=3, num_layers=1,
                      heads=[2, 1], feat_drop=0.1, attn_drop=0.1, hidden_drop=0.1, out_drop=0.1)
    if match == "NTN":
        l, r = model.match.W.weight.shape[-2:]
        model.match = model_zoo.NTN(l, r, k=4)
    return model.to(_dev())


# ---- 1. the select kernel alone ------------------------------------------------------------------------------------------------
def _rows(nq, G, rs):
    """rows of every kind the selection can go wrong on, by row index mod 6"""
    S = rs.standard_normal((nq, G)).astype(np.float32)
    special = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 1.0, -1.0], dtype=np.float32)
    for r in range(nq):
        kind = r % 6
        if kind == 1:
            S[r] = np.float32(0.25)                                             # all equal
        elif kind == 2:
            S[r] = rs.randint(0, 4, size=G).astype(np.float32)                  # four values: ties straddle every k-th place
        elif kind == 3:
            hit = rs.rand(G) < 0.4                                             # +-Inf, NaN, -0.0, +0.0 among ordinary values
            S[r, hit] = special[rs.randint(0, len(special), size=int(hit.sum()))]
        elif kind == 4:
            S[r] = np.round(S[r], 1)                                            # many duplicated values
        elif kind == 5:
            S[r] = rs.uniform(-1.0, 1.0, size=G).astype(np.float32)             # cosine-like: one exponent for most of the row
    return S


def _masks(kind, nq, G, rs):
    if kind == "none":
        return None, None
    lists = []
    for r in range(nq):
        if kind == "empty":
            lists.append([])
        elif kind == "one":
            lists.append([(r * 7) % G])
        elif kind == "unsorted_dups":
            lists.append([] if r % 3 == 0 else rs.randint(0, G, size=rs.randint(1, 2 * G + 2)).tolist())
        elif kind == "lead64":
            lists.append(list(range(min(64, G))))
        elif kind == "all_but_two":
            keep = {(r * 5) % G, (r * 11 + G // 2) % G}
            lists.append([c for c in rs.permutation(G).tolist() if c not in keep])
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    idx = np.asarray([c for x in lists for c in x], dtype=np.int64)
    return off, idx


@pytest.mark.parametrize("G", [1, 63, 64, 65, 257, 4097])
@pytest.mark.parametrize("nq", [1, 3, 130])
def test_select_k_equals_the_host_restatement(nq, G):
    """txe_select_k against host_select_k on the SAME fp32 rows: exact equality of the columns, their order and the keys -- every mask
    form, every k (k above G and above the unmasked count pads with -1), a padded row pitch, with and without out_key"""
    from taxoexpan_amd import ops
    from taxoexpan_amd.scoring import host_select_k
    rs = np.random.RandomState(1000 * nq + G)
    S = _rows(nq, G, rs)
    dev = _dev()
    dense = torch.from_numpy(S).to(dev)
    wide = torch.full((nq, G + 5), float("nan"), dtype=torch.float32, device=dev)      # a non-contiguous pitch (and an odd one)
    wide[:, :G] = dense
    keyed = np.where(np.isnan(S), -np.inf, S).astype(np.float32)
    n = 0
    for kind in ("none", "empty", "one", "unsorted_dups", "lead64", "all_but_two"):
        off, idx = _masks(kind, nq, G, rs)
        moff = None if off is None else torch.as_tensor(off, dtype=torch.int32).to(dev)
        midx = None if idx is None else torch.as_tensor(idx, dtype=torch.int32).to(dev)
        for k in (1, 5, 64, 1000):
            want = host_select_k(S, k, off, idx)
            n += 1
            Sd = wide[:, :G] if n % 2 else dense
            if n % 3:
                got, keys = ops.select_k(Sd, k, moff, midx, want_keys=True)
                keys = keys.cpu().numpy()
            else:
                got, keys = ops.select_k(Sd, k, moff, midx), None
            got = got.cpu().numpy()
            assert np.array_equal(got, want), (kind, k, np.argwhere(got != want)[:5])
            if keys is not None:
                wk = np.where(want >= 0, np.take_along_axis(keyed, np.maximum(want, 0).astype(np.int64), 1), -np.inf).astype(np.float32)
                assert np.array_equal(keys, wk), (kind, k)
    for Sd in (wide[:, :G].contiguous(), dense):                                       # S is not written
        assert np.array_equal(Sd.cpu().numpy().view(np.uint32), S.view(np.uint32))


def test_select_k_rejects_bad_arguments_on_the_device():
    from taxoexpan_amd import ops
    S = torch.zeros((2, 8), device=_dev())
    for k in (0, 4097):
        with pytest.raises(ValueError):
            ops.select_k(S, k)
    with pytest.raises(ValueError):
        ops.select_k(S, 2, mask_off=torch.zeros(3, dtype=torch.int32, device=_dev()))
    assert ops.select_k(S, 4096).shape == (2, 4096)


# ---- 2. retrieve_candidates on the toy taxonomy --------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize_embed", [False, True])
def test_retrieve_candidates_on_the_toy_taxonomy(tmp_path, normalize_embed):
    from taxoexpan_amd.scoring import host_retrieve, retrieve_candidates
    ds = _toy(tmp_path, normalize_embed)
    cand = sorted(ds.all_positions)
    off, idx = toy_masks(ds, cand)
    cf = ds.node_features[torch.as_tensor(cand)]
    qf = ds.node_features[torch.as_tensor(ds.node_list)]
    for k in (5, 16, 64):
        assert min(float(sorted_pool_gaps(ds, cand, q, k).min()) for q in ds.node_list) > MIN_GAP       # exact equality is owed
        want = host_retrieve(qf, cf, k, off, idx)
        for block in (None, 3):
            got = retrieve_candidates(qf.to(_dev()), cf.to(_dev()), k, off, idx, block=block)
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (k, block)


# ---- 3. retrieve_candidates where gaps can be tiny -----------------------------------------------------------------------------
def test_retrieve_candidates_on_a_synthetic_table():
    """4,097 candidates x 250 dims, 67 queries, k = 64, 0-40 masked columns per query.  eps = 4 x the largest difference between numpy's
    fp32 distances and the float64 ones on this input (floored at 1e-6): every pool member nearer than d_k - eps is returned, none
    farther than d_k + eps, no masked column, no column twice; and at least 0.9 k of every row lie outside the band, so the band
    cannot hide a failure."""
    from taxoexpan_amd.scoring import host_retrieve, retrieve_candidates
    rs = np.random.RandomState(7)
    G, D, Q, k = 4097, 250, 67, 64
    cf = rs.standard_normal((G, D)).astype(np.float32)
    qf = rs.standard_normal((Q, D)).astype(np.float32)
    cnt = rs.randint(0, 41, size=Q)
    off = np.concatenate([[0], np.cumsum(cnt)])
    idx = rs.randint(0, G, size=off[-1])
    c64, q64 = cf.astype(np.float64), qf.astype(np.float64)
    d64 = 1.0 - (q64 @ c64.T) / (np.linalg.norm(q64, axis=1)[:, None] * np.linalg.norm(c64, axis=1)[None, :])
    d32 = np.stack([1.0 - (cf @ v) / (np.linalg.norm(cf, axis=1) * np.linalg.norm(v)) for v in qf])          # KeyedRows.distances
    eps = max(4.0 * float(np.abs(d32.astype(np.float64) - d64).max()), 1e-6)
    print(f"eps = {eps:.3e}")
    ref = host_retrieve(qf, cf, k, off, idx)
    got = retrieve_candidates(torch.from_numpy(qf).to(_dev()), torch.from_numpy(cf).to(_dev()), k, off, idx).cpu().numpy()
    assert got.shape == (Q, k) and (got >= 0).all()
    for q in range(Q):
        masked = set(idx[off[q]:off[q + 1]].tolist())
        row = got[q].tolist()
        assert len(set(row)) == k and not masked & set(row)
        pool = np.asarray([c for c in range(G) if c not in masked])
        d_k = d64[q, ref[q, -1]]
        must = set(pool[d64[q, pool] < d_k - eps].tolist())
        assert len(must) >= 0.9 * k                                              # the float64 reference pins most of the row
        assert must <= set(row)
        assert (d64[q, got[q]] <= d_k + eps).all()
        assert (np.diff(d64[q, got[q]]) > -2 * eps).all()                        # nearest first, up to the band


# ---- 4. evaluate(retrieve=k) ---------------------------------------------------------------------------------------------------
def _host_protocol(model, ds, k, larger=True):
    """dataset.py:316-330 + metric.py:33-60 on the host: every query's positives and host_retrieve's rows, scored by the materialised
    all-candidate scores of the same model, ranked by the numpy restatement of the grouped ranking"""
    from taxoexpan_amd.evaluate import candidate_graphs
    from taxoexpan_amd.metric import _host_group_ranks
    from taxoexpan_amd.scoring import encode_candidates, fused_matcher_ok, host_retrieve, score_all
    dev = _dev()
    cand = sorted(ds.all_positions)
    index = {a: i for i, a in enumerate(cand)}
    model.eval()
    with torch.no_grad():
        hg = encode_candidates(model, candidate_graphs(ds.device_taxonomy(dev), cand, ds.expand_factor, 0, -1))
        qf = ds.node_features[torch.as_tensor(ds.node_list)].to(dev)
        if fused_matcher_ok(model.match):
            S = score_all(model.match, hg, qf).cpu().numpy()
        else:
            S = torch.stack([model.match(hg, q.expand(hg.shape[0], -1)).reshape(-1) for q in qf]).cpu().numpy()
    off, idx = toy_masks(ds, cand)
    ret = host_retrieve(ds.node_features[torch.as_tensor(ds.node_list)], ds.node_features[torch.as_tensor(cand)], k, off, idx)
    score, label = [], []
    for i, q in enumerate(ds.node_list):
        pos = [index[a] for a in ds.node2parents[q] if a in index]
        score += S[i, pos].tolist() + S[i, ret[i]].tolist()
        label += [1] * len(pos) + [0] * k
    ranks, pos_off = _host_group_ranks(np.asarray(score, dtype=np.float32), np.asarray(label), 1 if larger else 0)
    return ranks, pos_off, ret, S, cand


@pytest.mark.parametrize("match", ["LBM", "MLP", "NTN"])
@pytest.mark.parametrize("k", [5, 16])
def test_evaluate_with_retrieval_equals_the_host_protocol(tmp_path, match, k):
    """ranks of evaluate(retrieve=k) == the host protocol on score_all's materialised scores (the gathered route promises the block
    kernel's bits for LBM and MLP, so equality is exact; NTN takes the per-call fallback on the gathered rows), the metrics dict is
    metric.* of those ranks, and the case table lists retrieved parents only, best first"""
    from taxoexpan_amd import metric
    from taxoexpan_amd.evaluate import evaluate
    from taxoexpan_amd.scoring import topk_parents
    ds = _toy(tmp_path)
    model = _model(match)
    want, pos_off_w, ret, S, cand = _host_protocol(model, ds, k)
    rows = []
    metrics, ranks, pos_off, queries = evaluate(model, ds, _dev(), retrieve=k, case=rows)
    assert queries == list(ds.node_list) and np.array_equal(np.asarray(pos_off), pos_off_w)
    assert ranks.dtype == torch.int32 and ranks.is_cuda
    r = ranks.cpu()
    assert np.array_equal(r.numpy(), want), (r.tolist(), want.tolist())
    assert metrics["n_retrieved"] == k and metrics["n_queries"] == len(queries) and metrics["n_candidates"] == len(cand)
    off_t = torch.as_tensor(pos_off_w)
    assert metrics["macro_mr"] == pytest.approx(metric.macro_mr(r, off_t), rel=1e-12)
    per_q = [r[a:b].double() for a, b in zip(pos_off_w[:-1], pos_off_w[1:])]           # evaluate() averages per query, like test_fast.py
    for name, f in (("hit_at_1", lambda x: (x <= 1).double().mean()), ("hit_at_3", lambda x: (x <= 3).double().mean()),
                    ("hit_at_5", lambda x: (x <= 5).double().mean()), ("mrr_scaled_10", lambda x: (1.0 / torch.ceil(x / 10)).mean())):
        assert metrics[name] == pytest.approx(float(np.mean([float(f(x)) for x in per_q])), rel=1e-12), name
    # the case table: the best 5 of the RETRIEVED rows by matcher score, ties by ascending candidate
    assert len(rows) == 1 + len(queries)
    St = torch.from_numpy(S)
    for i, row in enumerate(rows[1:]):
        cols = sorted(ret[i].tolist())
        top = topk_parents(St[i, cols][None], torch.as_tensor([cand[c] for c in cols]), 5, True)[0].tolist()
        assert row[0] == ds.vocab[queries[i]]
        assert row[2] == ", ".join(ds.vocab[a] for a in top), (i, row[2])
        assert set(top) <= {cand[c] for c in ret[i]}
    assert float(rows[1][3]) == float(per_q[0].mean())


def test_evaluate_without_retrieval_is_unchanged(tmp_path):
    """retrieve=None: the all-candidate path -- rank_all_fused's ranks, the same dict keys, test_topk ignored"""
    from taxoexpan_amd.evaluate import candidate_graphs, evaluate
    from taxoexpan_amd.scoring import encode_candidates, rank_all_fused
    ds = _toy(tmp_path)
    ds.test_topk = 5
    model = _model("LBM")
    m0, r0, off0, q0 = evaluate(model, ds, _dev())
    m1, r1, off1, q1 = evaluate(model, ds, _dev(), retrieve=None)
    assert set(m0) == {"macro_mr", "hit_at_1", "hit_at_3", "hit_at_5", "mrr_scaled_10", "n_queries", "n_candidates"} and m0 == m1
    assert torch.equal(r0, r1) and np.array_equal(off0, off1) and q0 == q1
    cand = sorted(ds.all_positions)
    index = {a: i for i, a in enumerate(cand)}
    with torch.no_grad():
        hg = encode_candidates(model.eval(), candidate_graphs(ds.device_taxonomy(_dev()), cand, ds.expand_factor, 0, -1))
        qf = ds.node_features[torch.as_tensor(q0)].to(_dev())
        pos_idx = np.asarray([index[a] for q in q0 for a in ds.node2parents[q] if a in index])
        assert torch.equal(r0, rank_all_fused(model.match, hg, qf, off0, pos_idx))


# ---- 5. infer(retrieve=k) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("match,loss", [("LBM", "info_nce_loss"), ("MLP", "bce_loss")])
def test_infer_with_retrieval(tmp_path, match, loss):
    """every predicted parent of a new term is among its 8 cosine-nearest graph nodes, in topk_parents' order on the retrieved scores"""
    from taxoexpan_amd.evaluate import candidate_graphs, infer
    from taxoexpan_amd.scoring import encode_candidates, host_retrieve, score_all, topk_parents
    ds = _toy(tmp_path)
    model = _model(match)
    rs = np.random.RandomState(5)
    names = ["new_a", "new_b", "new_c"]
    vecs = rs.standard_normal((3, 8)).astype(np.float32)
    anchors = list(ds.graph.nodes())
    nf = ds.node_features[torch.as_tensor(anchors)]
    x = nf.numpy().astype(np.float64)
    for v in vecs.astype(np.float64):                                                  # the 8 nearest are pinned beyond fp32 rounding
        d = np.sort(1.0 - (x @ v) / (np.linalg.norm(x, axis=1) * np.linalg.norm(v)))
        assert np.diff(d[:9]).min() > MIN_GAP
    save = tmp_path / "pred.tsv"
    out = infer(model, ds, (names, vecs), _dev(), loss=loss, retrieve=8, topk=5, save=str(save))
    near = host_retrieve(vecs, nf, 8)
    larger = loss.startswith("info_nce")
    with torch.no_grad():
        hg = encode_candidates(model.eval(), candidate_graphs(ds.device_taxonomy(_dev()), anchors, ds.expand_factor, 0, -1))
        S = score_all(model.match, hg, torch.from_numpy(vecs).to(_dev())).cpu()
    assert [q for q, _ in out] == names
    for i, (_q, parents) in enumerate(out):
        cols = sorted(near[i].tolist())
        want = topk_parents(S[i, cols][None], torch.as_tensor([anchors[c] for c in cols]), 5, larger)[0].tolist()
        assert parents == [ds.vocab[a] for a in want], (i, parents)
        assert set(parents) <= {ds.vocab[anchors[c]] for c in near[i]}
    lines = open(save).read().splitlines()
    assert lines[0] == "Query\tPredicted parents" and lines[1] == f"{names[0]}\t{', '.join(out[0][1])}" and len(lines) == 4
    few = infer(model, ds, (names, vecs), _dev(), loss=loss, retrieve=3, topk=5)       # fewer retrieved than topk: all of them, ranked
    assert all(len(p) == 3 and set(p) == {ds.vocab[anchors[c]] for c in host_retrieve(vecs, nf, 3)[i]} for i, (_q, p) in enumerate(few))
