"""GPU: the all-candidate scoring loop of the NTN matcher (txe_ntn_*: the score GEMM's tile once per bilinear slice, tanh and the sum over
slices in registers) -- the accuracy gate against float64 (scoring.host_ntn_scores), three weight scales (tanh near zero, saturated),
bit-identity among its four modes, the non-finite domain, counts over shards, query blocking, evaluate() / evaluate(case=...) /
infer() on it, and the reference's golden scores.

The gate is the MLP scoring loop's: max |HIP - f64| <= max(2 x max |fp32 literal - f64|, 2e-5 x max |f64|), the fp32 literal being
NTN.forward's arithmetic in torch on the device, one query at a time."""
import functools
import itertools
import os
import shutil

import numpy as np
import pytest
import torch

import txe_oracle as orc
from golden_util import GOLDEN_DIR

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _ntn(l, r, k, seed, non_linear=torch.tanh):
    from taxoexpan_amd.model_zoo import NTN
    torch.manual_seed(seed)
    return NTN(l, r, k=k, non_linear=non_linear)


def _scale(m, s):
    with torch.no_grad():
        for p in (m.W.weight, m.W.bias, m.V.weight):
            p.mul_(s)


def _saturating(m, hg):
    """make every pre-activation of (m, hg) against any query of ordinary size large once the weights are scaled up: the first two
    columns of hg hold +-32 by candidate, W ignores them, V1 reads column 0 in the even slices and column 1 in the odd ones, so
    t_j(q, g) = +-32 + (terms that stay below ~15 in magnitude) before the scale, and its sign -- hence the score, one of at most four
    signed sums of u -- depends on the candidate alone"""
    G, k = hg.shape[0], m.W.weight.shape[0]
    rs = np.random.RandomState(G)
    hg[:, 0] = torch.from_numpy(32.0 * rs.choice([-1.0, 1.0], size=G)).float()
    hg[:, 1] = torch.from_numpy(32.0 * rs.choice([-1.0, 1.0], size=G)).float()
    with torch.no_grad():
        m.W.weight[:, :2, :] = 0.0
        m.V.weight[:, 0] = torch.tensor([1.0 if j % 2 == 0 else 0.0 for j in range(k)])
        m.V.weight[:, 1] = torch.tensor([0.0 if j % 2 == 0 else 1.0 for j in range(k)])


def _literal_dev(m, hg, q):
    """the literal route on the device in torch: u_R(f(W(hg, q) + V([hg | q]))) per query (model_zoo.py:339-346 under test_fast.py:121-123)"""
    F = torch.nn.functional
    with torch.no_grad():
        out = []
        for qq in q:
            e2 = qq.expand(hg.shape[0], -1)
            out.append((m.f(F.bilinear(hg, e2, m.W.weight, m.W.bias) + torch.cat((hg, e2), 1) @ m.V.weight.t()) @ m.u_R.weight.t()).squeeze(1))
        return torch.stack(out)


def _yard(lit, ref):
    return max(2 * float(np.abs(lit - ref).max()), 2e-5 * float(np.abs(ref).max()))


def _pre_activations_f64(m, hg, q):
    W, b, V = (t.detach().double().cpu().numpy() for t in (m.W.weight, m.W.bias, m.V.weight))
    H, Q = hg.double().cpu().numpy(), q.double().cpu().numpy()
    l = H.shape[1]
    return np.einsum("gl,klr,qr->qgk", H, W, Q, optimize=True) + (H @ V[:, :l].T + b)[None] + (Q @ V[:, l:].T)[:, None]


@functools.lru_cache(maxsize=None)
def _case(G, nq, l, r, k, scale=1.0, saturate=False, dup=False):
    """one matcher and its inputs on the device, with the three score matrices every test of the shape shares: S (score_all), ref (the
    float64 host restatement) and lit (the fp32 literal route on the device)"""
    from taxoexpan_amd.scoring import host_ntn_scores, score_all
    m = _ntn(l, r, k, seed=G + nq + k)
    gen = torch.Generator().manual_seed(G * 7 + k)
    hg = torch.randn(G, l, generator=gen)
    q = torch.randn(nq, r, generator=gen)
    if dup:
        hg[G // 2:G // 2 + 5] = hg[3]                       # duplicated candidate rows: exact ties, some across tiles
        hg[G - 1] = hg[3]
        q[nq // 2] = q[0]                                   # duplicated queries
    if saturate:
        _saturating(m, hg)
    _scale(m, scale)
    m, hg, q = m.to(_dev()), hg.to(_dev()), q.to(_dev())
    S = score_all(m, hg, q)
    ref = host_ntn_scores(m, hg, q)
    lit = _literal_dev(m, hg, q).double().cpu().numpy()
    return m, hg, q, S, ref, lit


@pytest.mark.parametrize("G,nq,l,r,k", [(1, 1, 3, 2, 1), (31, 7, 5, 9, 4), (129, 129, 17, 12, 4), (257, 130, 33, 12, 3), (4099, 7, 40, 25, 5),
                                         (257, 1, 500, 250, 4), (300, 130, 64, 33, 16)])
def test_accuracy_gate_against_float64(G, nq, l, r, k):
    """k = 1, k not dividing 4, the k limit, single rows, tile edges at 128, a long r"""
    _m, _hg, _q, S, ref, lit = _case(G, nq, l, r, k)
    assert S.shape == (nq, G)
    err, yard = float(np.abs(S.double().cpu().numpy() - ref).max()), _yard(lit, ref)
    print(f"NTN gate {(G, nq, l, r, k)}: err {err:.3e} yard {yard:.3e} max|f64| {float(np.abs(ref).max()):.3e}")
    assert err <= yard, (err, yard)


@pytest.mark.parametrize("scale", [1.0, 1e-3, 1e4])
def test_three_weight_scales(scale):
    """x1e-3: tanh near zero, where the gate's floor is tiny (a tanh that cancels there fails it); x1e4: every pre-activation
    saturates -- every score is finite and a signed sum of the u_j"""
    sat = scale == 1e4
    m, hg, q, S, ref, lit = _case(257, 130, 33, 12, 4, scale, sat)
    Sd = S.double().cpu().numpy()
    err, yard = float(np.abs(Sd - ref).max()), _yard(lit, ref)
    print(f"NTN scale {scale:g}: err {err:.3e} yard {yard:.3e} max|f64| {float(np.abs(ref).max()):.3e}")
    assert err <= yard, (scale, err, yard)
    if sat:
        assert float(np.abs(_pre_activations_f64(m, hg, q)).min()) > 1e4      # the premise: nothing near tanh's slope
        assert np.isfinite(Sd).all()
        u = m.u_R.weight.detach().double().cpu().numpy().reshape(-1)
        sums = np.array([float(np.dot(s, u)) for s in itertools.product((-1.0, 1.0), repeat=len(u))])
        assert float(np.abs(Sd[..., None] - sums).min(axis=-1).max()) <= yard
        assert len(np.unique(Sd)) <= 4                                          # (and they tie: four sign patterns by construction)


def _pos_lists(nq, G, rs):
    """1-3 positives per query, some lists naming a candidate twice"""
    lists = []
    for i in range(nq):
        p = sorted(rs.choice(G, size=min(G, 1 + (i % 3)), replace=False).tolist())
        if i % 4 == 2 and len(p) >= 2:
            p[1] = p[0]
        lists.append(p)
    off = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int64)
    return off, np.concatenate(lists).astype(np.int64)


@pytest.mark.parametrize("scale", [1.0, 1e4])
@pytest.mark.parametrize("G,nq,l,r,k", [(257, 130, 17, 12, 4), (4099, 7, 40, 25, 3)])
def test_fused_modes_equal_the_stored_block(G, nq, l, r, k, scale):
    """positives == the stored block's entries; fused ranks == rank_block on the stored scores; fused top-k (k = 1, 5, 8) ==
    scoring.topk_parents on them -- torch.equal, both directions, duplicated candidates / queries / positives, G no multiple of the
    tile.  At x1e4 most scores tie exactly: ties break by ascending candidate row."""
    from taxoexpan_amd import ops
    from taxoexpan_amd.scoring import rank_all_fused, topk_parents, topk_parents_fused
    m, hg, q, S, _ref, _lit = _case(G, nq, l, r, k, scale, scale == 1e4, True)
    off, idx = _pos_lists(nq, G, np.random.RandomState(G + nq))
    if scale == 1e4:
        assert len(torch.unique(S)) <= 4
    prep = ops.ntn_project(hg, m)
    thr = ops.ntn_positive_scores(q, prep, torch.from_numpy(off), torch.from_numpy(idx))
    qid = np.repeat(np.arange(nq), np.diff(off))
    assert torch.equal(thr, S[torch.from_numpy(qid).to(_dev()), torch.from_numpy(idx).to(_dev())])
    ids = torch.arange(G, device=_dev())
    for larger in (True, False):
        want = ops.rank_block(S.contiguous(), torch.from_numpy(off), torch.from_numpy(idx), larger)
        for block in (None, 33):
            got = rank_all_fused(m, hg, q, off, idx, block=block, larger_is_better=larger)
            assert torch.equal(got, want), (larger, block)
        for kk in (1, 5, 8):
            assert torch.equal(topk_parents_fused(m, hg, q, None, kk, larger, block=50), topk_parents(S, ids, kk, larger)), (kk, larger)


def test_non_finite_domain_follows_the_literal_route():
    """a candidate row of NaN and a query holding one NaN: exactly that column and that row of S are NaN, as on the literal route; NaN
    sorts last in top-k and never counts as better in ranks (the materialised path's answers).  W.bias[0] = +inf: all-finite scores,
    the literal route's within the gate."""
    from taxoexpan_amd import ops
    from taxoexpan_amd.scoring import host_ntn_scores, rank_all_fused, score_all, topk_parents, topk_parents_fused
    G, nq, l, r, k = 300, 9, 10, 6, 4
    m = _ntn(l, r, k, seed=9).to(_dev())
    gen = torch.Generator().manual_seed(5)
    hg = torch.randn(G, l, generator=gen)
    q = torch.randn(nq, r, generator=gen)
    hg[140, :] = float("nan")
    q[4, 1] = float("nan")
    hg, q = hg.to(_dev()), q.to(_dev())
    S = score_all(m, hg, q)
    L = _literal_dev(m, hg, q)
    want_nan = torch.zeros((nq, G), dtype=torch.bool, device=_dev())
    want_nan[4, :] = True
    want_nan[:, 140] = True
    assert torch.equal(torch.isnan(S), want_nan) and torch.equal(torch.isnan(L), want_nan)
    assert bool(torch.isfinite(S[~want_nan]).all())
    rs = np.random.RandomState(1)
    off, idx = _pos_lists(nq, G, rs)
    idx[0] = 140                                                    # a NaN positive
    prep = ops.ntn_project(hg, m)
    qid = np.repeat(np.arange(nq), np.diff(off))
    thr = ops.ntn_positive_scores(q, prep, torch.from_numpy(off), torch.from_numpy(idx))
    assert torch.equal(thr.nan_to_num(7.0), S[torch.from_numpy(qid).to(_dev()), torch.from_numpy(idx).to(_dev())].nan_to_num(7.0))
    ids = torch.arange(G, device=_dev())
    for larger in (True, False):
        assert torch.equal(rank_all_fused(m, hg, q, off, idx, larger_is_better=larger),
                           ops.rank_block(S.contiguous(), torch.from_numpy(off), torch.from_numpy(idx), larger))
        top = topk_parents_fused(m, hg, q, None, 5, larger)
        assert torch.equal(top, topk_parents(S, ids, 5, larger))
        assert not bool((top[[0, 1, 2, 3, 5, 6, 7, 8]] == 140).any())            # NaN last: never among the best of a finite row
    # an infinite bias saturates its slice for every pair
    hg2, q2 = torch.randn(G, l, generator=gen).to(_dev()), torch.randn(nq, r, generator=gen).to(_dev())
    with torch.no_grad():
        m.W.bias[0] = float("inf")
    S2 = score_all(m, hg2, q2)
    assert bool(torch.isfinite(S2).all())
    ref = host_ntn_scores(m, hg2, q2)
    lit = _literal_dev(m, hg2, q2).double().cpu().numpy()
    assert np.isfinite(ref).all() and np.isfinite(lit).all()
    err, yard = float(np.abs(S2.double().cpu().numpy() - ref).max()), _yard(lit, ref)
    assert err <= yard, (err, yard)


def test_counts_add_over_candidate_shards():
    """count over hg[:100] and hg[100:] into one buffer == one call over hg"""
    from taxoexpan_amd import ops
    G, nq, h = 257, 130, 100
    m, hg, q, _S, _ref, _lit = _case(G, nq, 17, 12, 4, 1.0, False, True)
    off, idx = _pos_lists(nq, G, np.random.RandomState(3))
    off_t, idx_t = torch.from_numpy(off), torch.from_numpy(idx)
    prep = ops.ntn_project(hg, m)
    thr = ops.ntn_positive_scores(q, prep, off_t, idx_t)
    for larger in (True, False):
        whole = ops.ntn_score_count_block(q, prep, off_t, thr, larger)
        parts = torch.zeros_like(whole)
        for lo, hi in ((0, h), (h, G)):
            ops.ntn_score_count_block(q, ops.ntn_project(hg[lo:hi], m), off_t, thr, larger, counts=parts)
        assert torch.equal(parts, whole) and int(whole.sum()) > 0, larger


def test_query_blocking_changes_no_bit():
    from taxoexpan_amd.scoring import score_all
    m, hg, q, S, _ref, _lit = _case(257, 130, 17, 12, 4, 1.0, False, True)
    assert torch.equal(score_all(m, hg, q, block=64), S)
    assert torch.equal(score_all(m, hg, q, block=None), S)


@pytest.mark.parametrize("G,nq,l,r,k", [(31, 7, 5, 9, 4), (300, 130, 64, 33, 16), (257, 130, 17, 12, 4), (129, 5, 6, 64, 2)])
def test_unpadded_operands_through_the_entry_point_change_no_bit(G, nq, l, r, k):
    """txe_ntn_score_block on operands as they come -- queries and slices on a pitch of r floats (odd pitches: the scalar loader; r = 12:
    16-byte rows with a ragged only k-tile; r = 64: whole k-tiles only), the slices one after the other -- == the padded, stacked layout
    ops.ntn_project makes: zeros add exactly nothing"""
    from taxoexpan_amd import _lib, ops
    m, hg, q, S, _ref, _lit = _case(G, nq, l, r, k, 1.0, False, G == 257)
    prep = ops.ntn_project(hg, m)
    qp = ops.ntn_prepare_queries(q, prep)
    U = torch.stack([prep.slice(j) for j in range(k)]).contiguous()            # [k, G, r]
    Qc = q.contiguous()
    out = torch.full((nq, G), float("nan"), dtype=torch.float32, device=_dev())
    _lib.call("txe_ntn_score_block", Qc.data_ptr(), r, nq, U.data_ptr(), r, G * r, G, r, prep.a.data_ptr(), prep.a.stride(0), qp.c.data_ptr(),
              qp.c.stride(0), prep.u.data_ptr(), k, out.data_ptr(), G, _lib.stream_ptr())
    assert torch.equal(out, S)


def test_golden_extras_ntn():
    """the reference's NTN outputs of extras.npz (e1 n x 12, e2 n x 7, k = 4) on the diagonal of score_all"""
    from taxoexpan_amd.model_zoo import NTN
    from taxoexpan_amd.scoring import score_all
    z = np.load(os.path.join(GOLDEN_DIR, "extras.npz"))
    m = NTN(12, 7, k=4)
    m.load_state_dict({k: torch.from_numpy(z["ntn.p." + k]) for k in ("u_R.weight", "W.weight", "W.bias", "V.weight")}, strict=True)
    m = m.to(_dev())
    S = score_all(m, torch.from_numpy(z["ntn.e1"]).to(_dev()), torch.from_numpy(z["ntn.e2"]).to(_dev()))
    np.testing.assert_allclose(torch.diagonal(S).cpu().numpy(), z["ntn.out"].reshape(-1), rtol=1e-4, atol=1e-4)


# ---- end to end on the toy taxonomy -------------------------------------------------------------------------------------------------
def _toy(tmp_path):
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    for fn in os.listdir(os.path.join(GOLDEN_DIR, "toy_taxo")):
        shutil.copy(os.path.join(GOLDEN_DIR, "toy_taxo", fn), tmp_path)
    return MaskedGraphDataset(MAGDataset("toy", str(tmp_path), raw=True), mode="test", sampling_mode=0, expand_factor=100,
                              normalize_embed=True)


def _model(non_linear=torch.tanh):
    """the PGAT+WMR toy model of test_gpu_retrieval._model("NTN"): an NTN (k = 4) in the place of its LBM module"""
    from taxoexpan_amd import TaxoExpan, model_zoo
    torch.manual_seed(11)
    model = TaxoExpan("PGAT", "WMR", "LBM", in_dim=8, hidden_dim=6, out_dim=5, pos_dim=3, num_layers=1, heads=[2, 1], feat_drop=0.1,
                      attn_drop=0.1, hidden_drop=0.1, out_drop=0.1)
    l, r = model.match.W.weight.shape[-2:]
    model.match = model_zoo.NTN(l, r, k=4, non_linear=non_linear)
    return model.to(_dev())


def _forbid_forward(monkeypatch):
    from taxoexpan_amd.model_zoo import NTN

    def boom(*a, **k):
        raise AssertionError("NTN.forward called on the fused route")
    monkeypatch.setattr(NTN, "forward", boom)


def test_evaluate_and_infer_take_the_fused_route(tmp_path, monkeypatch):
    """evaluate(): ranks == the host ranking (metric.py) of score_all's own materialised scores, both directions; chunked candidates
    (-b 17) == one batch; case= lists topk_parents of those scores; infer(topk=5) == topk_parents on score_all; score_all passes the
    gate; NTN.forward is never called"""
    from taxoexpan_amd.evaluate import CASE_METRICS, candidate_graphs, evaluate, infer
    from taxoexpan_amd.scoring import encode_candidates, host_ntn_scores, score_all, topk_parents
    ds = _toy(tmp_path)
    model = _model()
    cand = sorted(ds.all_positions)
    index = {a: i for i, a in enumerate(cand)}
    model.eval()
    hg = encode_candidates(model, candidate_graphs(ds.device_taxonomy(_dev()), cand, ds.expand_factor, 0)).detach()
    cand_ids = torch.as_tensor(np.asarray(cand, dtype=np.int64), device=_dev())
    _forbid_forward(monkeypatch)
    S = None
    for larger in (True, False):
        rows = []
        metrics, ranks, pos_off, queries = evaluate(model, ds, _dev(), larger_is_better=larger, case=rows)
        assert len(queries) >= 5 and rows[0] == ["Test node index", "True parents", "Predicted parents"] + list(CASE_METRICS)
        if S is None:
            qf = ds.node_features[torch.as_tensor(queries, dtype=torch.long)].to(_dev())
            S = score_all(model.match, hg, qf)
        Sh = S.cpu().numpy()
        want = []
        for i, q in enumerate(queries):
            want += list(orc.ranks_of_positives(Sh[i], [index[a] for a in ds.node2parents[q] if a in index], larger))
        np.testing.assert_array_equal(ranks.cpu().numpy(), np.asarray(want))
        top = topk_parents(S, cand_ids, 5, larger).cpu().tolist()
        for i, q in enumerate(queries):
            assert rows[1 + i][0] == ds.vocab[q] and rows[1 + i][2] == ", ".join(ds.vocab[p] for p in top[i]), rows[1 + i]
        m2, r2, _, _ = evaluate(model, ds, _dev(), larger_is_better=larger, batch_size=17)
        assert torch.equal(r2, ranks) and m2 == metrics
    # inference on new terms: all graph nodes are candidates
    rs = np.random.RandomState(5)
    vecs = rs.standard_normal((9, 8)).astype(np.float32)
    out = infer(model, ds, ([f"t{i}" for i in range(9)], vecs), _dev(), loss="info_nce_loss", topk=5)
    anchors = list(ds.graph.nodes())
    hg_all = encode_candidates(model, candidate_graphs(ds.device_taxonomy(_dev()), anchors, ds.expand_factor, 0)).detach()
    qn = torch.from_numpy(vecs).to(_dev())
    S_all = score_all(model.match, hg_all, qn)
    top = topk_parents(S_all, torch.as_tensor(np.asarray(anchors, dtype=np.int64), device=_dev()), 5, True).cpu().tolist()
    assert [got for _name, got in out] == [[ds.vocab[i] for i in row] for row in top]
    monkeypatch.undo()
    # the materialised scores themselves: within the gate of float64
    ref = host_ntn_scores(model.match, hg, qf)
    lit = _literal_dev(model.match, hg, qf).double().cpu().numpy()
    assert float(np.abs(S.double().cpu().numpy() - ref).max()) <= _yard(lit, ref)


def test_another_non_linear_keeps_the_literal_loop(tmp_path):
    """non_linear=torch.relu has no fused route: the same evaluate() runs NTN.forward per query and gives finite ranks"""
    from taxoexpan_amd.evaluate import evaluate
    from taxoexpan_amd.scoring import fused_matcher_ok
    ds = _toy(tmp_path)
    model = _model(torch.relu)
    assert not fused_matcher_ok(model.match)
    calls = []
    orig = type(model.match).forward
    model.match.forward = lambda *a, **k: (calls.append(1), orig(model.match, *a, **k))[1]
    metrics, ranks, pos_off, queries = evaluate(model, ds, _dev())
    assert len(calls) >= len(queries) >= 5
    r = ranks.cpu().numpy()
    assert r.shape[0] == pos_off[-1] and (r >= 1).all() and (r <= metrics["n_candidates"]).all() and np.isfinite(metrics["macro_mr"])
