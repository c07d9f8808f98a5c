"""GPU: hedged placement (csrc/txe_hedge.hip) against its numpy restatement -- the probability launch to 2 fp32 ulps and exactly by
position, the subtree masses bit for bit on probabilities downloaded from the device, the hedging rule exactly, and evaluate / infer
with the `hedge` keyword end to end."""
import os
import shutil

import numpy as np
import pytest
import torch

import hedge_cases as hc
from golden_util import GOLDEN_DIR
from taxoexpan_amd import hedge, scoring
from taxoexpan_amd.hedge import SLICE, HedgeIndex

pytestmark = pytest.mark.gpu
THR4 = [0.3, 0.5, 0.9, 1.0]


def _dev():
    return torch.device("cuda:0")


def _taxonomy(name):
    """(HedgeIndex, G) of a named case; "subset": the star-plus-chain without an interior node, a leaf and the lone node"""
    if name in ("long", "subset"):
        parents, n, who = hc.star_plus_chain(SLICE)
        cand = list(range(n))
        if name == "subset":
            drop = {who["c"], who["lone"], max(v for v, p in parents.items() if p == [who["root"]] and v != who["b"])}
            cand = [v for v in np.random.RandomState(6).permutation(n).tolist() if v not in drop]
    else:
        parents, n = getattr(hc, name)()
        cand = list(range(n))
    return HedgeIndex.build(hc.index_of(parents, n), cand)


def _device_probs(G, nq, seed, T=0.8, larger=True, scale=6.0):
    """(PT device view [G, nq], P host [nq, G] downloaded from it): scores of a wide range, so that the order of a float64 sum of the
    fp32 probabilities is observable"""
    S = (torch.from_numpy(np.random.RandomState(seed).standard_normal((nq, G)).astype(np.float32)) * scale).to(_dev())
    lse = torch.from_numpy(scoring.host_score_moments(S.cpu(), T, larger).lse).to(_dev())
    PT = hedge.probabilities(S, lse, 1.0 / T, larger)
    return PT, PT.cpu().numpy().T.copy()


def _ulps(a, b):
    """distance in representable fp32 values of non-negative arrays (below 2^-126 that is an absolute distance in units of 2^-149)"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("G", [1, 37, 300])
@pytest.mark.parametrize("nq", [1, 63, 65, 130])
def test_probabilities_against_the_restatement(nq, G):
    rs = np.random.RandomState(nq * 1000 + G)
    S = (rs.standard_normal((nq, G)) * 4).astype(np.float32)
    if G > 8:
        S[:, 3] -= 85.0                                             # p below 2^-126: the subnormal range
        S[0, 5] -= 101.0
    for r, v in ((1, np.nan), (2, np.inf), (3, -np.inf)):
        if nq > 3:
            S[r, :] = v if v == -np.inf else S[r, :]
            S[r, G // 2] = v
    for T, larger in ((1.0, True), (0.7, False)):
        lse = scoring.host_score_moments(S, T, larger).lse
        Sd = torch.full((nq, G + 5), 7.0, dtype=torch.float32, device=_dev())     # a row pitch larger than G
        Sd[:, :G] = torch.from_numpy(S)
        PT = hedge.probabilities(Sd[:, :G], torch.from_numpy(lse).to(_dev()), 1.0 / T, larger)
        assert PT.shape == (G, nq) and PT.stride(1) == 1 and PT.stride(0) % 64 == 0 and PT.dtype == torch.float32
        got = PT.cpu().numpy().T
        want = hedge.host_probabilities(S, lse, T, larger)
        assert np.isfinite(got).all() and (got >= 0).all()
        assert _ulps(np.ascontiguousarray(got), want).max() <= 2
        bad = ~np.isfinite(lse)
        assert not got[bad].any() and bad.sum() >= (2 if nq > 3 else 0)     # (NaN and all -Inf; +Inf unless its sign is turned)
        if G > 8 and larger and nq >= 63:
            assert ((want[~bad] > 0) & (want[~bad] < 2.0 ** -126)).any()
        # the padding columns of the buffer behind the view are zeros
        full = torch.as_strided(PT, (G, PT.stride(0)), (PT.stride(0), 1)).cpu().numpy()
        assert not full[:, nq:].any()


@pytest.mark.parametrize("nq,G", [(1, 300), (65, 37), (130, 300), (63, 1)])
def test_transposition_is_exact_by_position(nq, G):
    """scores 0 or -Inf at lse 0: p is exactly 1 or 0, in a pattern no transposition error survives"""
    q, g = np.meshgrid(np.arange(nq), np.arange(G), indexing="ij")
    one = ((q * 7 + g * 13 + (q * g) % 5) % 3) == 0
    S = np.where(one, 0.0, -np.inf).astype(np.float32)
    PT = hedge.probabilities(torch.from_numpy(S).to(_dev()), torch.zeros(nq, dtype=torch.float64, device=_dev()))
    assert np.array_equal(PT.cpu().numpy(), one.T.astype(np.float32))


@pytest.mark.parametrize("nq", [130, 1])
@pytest.mark.parametrize("case", ["long", "diamond", "forest", "subset"])
def test_mass_block_is_bit_equal(case, nq):
    ix = _taxonomy(case)
    if case == "long":
        assert ix.G == 3 * SLICE + 6 and sorted({len(ix.row(a)) for a in range(ix.G)}) == [1, SLICE, SLICE + 1, 3 * SLICE + 5]
    PT, P = _device_probs(ix.G, nq, seed=11)
    mass = hedge.subtree_mass(ix.to(_dev()), PT)
    assert mass.shape == (ix.G, nq) and mass.dtype == torch.float64
    want = hedge.host_subtree_mass(ix, P)
    assert np.array_equal(mass.cpu().numpy(), want)
    assert want.max() > 0.5
    # probabilities on a pitch of the caller's own (no padding, rows not 256-byte aligned)
    mass2 = hedge.subtree_mass(ix.to(_dev()), torch.from_numpy(np.ascontiguousarray(P.T)).to(_dev()))
    assert torch.equal(mass, mass2)


@pytest.mark.parametrize("thr", [[0.5], THR4])
@pytest.mark.parametrize("case", ["long", "diamond", "forest", "subset"])
def test_hedge_block_against_the_restatement(case, thr):
    ix = _taxonomy(case)
    ixd = ix.to(_dev())
    PT, P = _device_probs(ix.G, 130, seed=12, scale=4.0)
    h = hedge.hedge_block(ixd, PT, thr)
    want = hedge.host_hedge(ix, P, thr)
    assert h.node_col.dtype == torch.int32 and h.mass.dtype == torch.float64 and h.depth.dtype == torch.int32
    assert np.array_equal(h.node_col.cpu().numpy(), want.node_col) and np.array_equal(h.depth.cpu().numpy(), want.depth)
    assert np.array_equal(h.mass.cpu().numpy(), want.mass, equal_nan=True)
    # = the argmax over the stored mass block
    arg = hedge.host_hedge(ix, None, thr, mass=hedge.subtree_mass(ixd, PT).cpu().numpy())
    assert np.array_equal(arg.node_col, want.node_col) and np.array_equal(arg.mass, want.mass, equal_nan=True)
    # two runs: equal bytes
    h2 = hedge.hedge_block(ixd, PT, thr)
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(h, h2))
    # a threshold's result does not depend on the others
    one = hedge.hedge_block(ixd, PT, thr[-1])
    assert torch.equal(one.node_col[:, 0], h.node_col[:, -1]) and torch.equal(one.mass.view(torch.int64)[:, 0], h.mass.view(torch.int64)[:, -1])
    if case == "forest" and len(thr) == 4:
        assert (want.node_col[:, -1] == -1).all() and np.isnan(want.mass[:, -1]).all()        # no tree holds everything
    if case == "long" and len(thr) == 4:
        assert len(np.unique(want.node_col)) > 3                  # (leaves, interior nodes, the root and no answer)


def test_hedge_block_tie_rules():
    """equal depth: the larger mass; masses exactly equal: the smaller column; a zero row (a non-finite lse): no answer"""
    parents, n = hc.star(4)
    ix = HedgeIndex.build(hc.index_of(parents, n), list(range(n)))
    P = np.asarray([[0.0, 0.3, 0.4, 0.3], [0.25, 0.375, 0.0, 0.375], [0.0, 0.0, 0.0, 0.0], [0.125, 0.125, 0.25, 0.5]], dtype=np.float32)
    thr = [0.25, 0.375, 1.0]
    h = hedge.hedge_block(ix.to(_dev()), torch.from_numpy(np.ascontiguousarray(P.T)).to(_dev()), thr)
    want = hedge.host_hedge(ix, P, thr)
    assert want.node_col.tolist() == [[2, 2, 0], [1, 1, 0], [-1, -1, -1], [3, 3, 0]]
    assert h.node_col.cpu().tolist() == want.node_col.tolist() and h.depth.cpu().tolist() == want.depth.tolist()
    assert np.array_equal(h.mass.cpu().numpy(), want.mass, equal_nan=True)
    ix2 = HedgeIndex.build(hc.index_of(parents, n), [3, 0, 2, 1])
    h = hedge.hedge_block(ix2.to(_dev()), torch.from_numpy(np.ascontiguousarray(P[:, [3, 0, 2, 1]].T)).to(_dev()), 0.375)
    assert h.node_col.cpu().tolist() == [[2], [0], [-1], [0]]


def test_a_query_does_not_depend_on_its_block():
    """the same queries in blocks of 64, 65 and 130: equal bytes per query, masses and hedged answers"""
    ix = _taxonomy("long")
    ixd = ix.to(_dev())
    T = 0.8
    S = (torch.from_numpy(np.random.RandomState(21).standard_normal((130, ix.G)).astype(np.float32)) * 5).to(_dev())
    lse = torch.from_numpy(scoring.host_score_moments(S.cpu(), T).lse).to(_dev())
    ref = None
    for nb in (130, 65, 64):
        mass, hs = [], []
        for q0 in range(0, 130, nb):
            PT = hedge.probabilities(S[q0:q0 + nb], lse[q0:q0 + nb], 1.0 / T)
            mass.append(hedge.subtree_mass(ixd, PT).t())
            hs.append(hedge.hedge_block(ixd, PT, THR4))
        got = [torch.cat(mass)] + [torch.cat([h[i] for h in hs]) for i in range(3)]
        if ref is None:
            ref = got
        assert all(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)) for a, b in zip(got, ref)), nb


def test_empty_shapes_launch_nothing():
    ix = _taxonomy("diamond").to(_dev())
    h = hedge.hedge_block(ix, torch.zeros((ix.G, 0), dtype=torch.float32, device=_dev()), 0.5)
    assert h.node_col.shape == (0, 1) and hedge.subtree_mass(ix, torch.zeros((ix.G, 0), dtype=torch.float32, device=_dev())).shape == (ix.G, 0)
    empty = HedgeIndex.build(hc.index_of(*hc.chain()), []).to(_dev())
    h = hedge.hedge_block(empty, torch.zeros((0, 3), dtype=torch.float32, device=_dev()), [0.5, 0.9])
    assert h.node_col.cpu().tolist() == [[-1, -1]] * 3 and torch.isnan(h.mass).all() and not h.depth.any()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hedge.subtree_mass(ix, torch.zeros((ix.G, 2)))


# ---------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------
TEMPERATURE = 0.25
E2E_THR = (0.5, 0.9)


def _toy(tmp_path):
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    for fn in os.listdir(os.path.join(GOLDEN_DIR, "toy_taxo")):
        shutil.copy(os.path.join(GOLDEN_DIR, "toy_taxo", fn), tmp_path)
    return MaskedGraphDataset(MAGDataset("toy", str(tmp_path), raw=True), mode="test", sampling_mode=0, expand_factor=100, normalize_embed=True)


def _model(match):
    from taxoexpan_amd import TaxoExpan
    torch.manual_seed(11)
    return TaxoExpan("PGAT", "WMR", match, in_dim=8, hidden_dim=6, out_dim=5, pos_dim=3, num_layers=1, heads=[2, 1], feat_drop=0.1,
                     attn_drop=0.1, hidden_drop=0.1, out_drop=0.1).to(_dev())


def _encode(model, ds, cand):
    from taxoexpan_amd.evaluate import candidate_graphs
    model.eval()
    g = candidate_graphs(ds.device_taxonomy(_dev()), cand, ds.expand_factor, 0, -1)
    return scoring.encode_candidates(model, g)


@pytest.mark.parametrize("match", ["BIM", "MLP"])
def test_evaluate_with_hedge_end_to_end(tmp_path, match):
    """evaluate(hedge=(0.5, 0.9), temperature=T) against host_hedge fed from scoring.score_all and the device lse: the hedged columns
    and depths are equal for every query none of whose host masses lies within 1e-5 of a threshold (the device-side error of a mass is a
    few 1e-7: 2 ulps of each p, and the masses sum to at most 1); at most 5 % of the queries may be left out by that rule (asserted; with
    this seed, on the toy's 8 test queries, it leaves out none for BIM and none for MLP).  Every other metric, the ranks and the offsets
    are bit-equal to a call without the keyword."""
    from taxoexpan_amd.evaluate import evaluate
    from taxoexpan_amd.taxometric import TaxonomyIndex
    ds = _toy(tmp_path)
    model = _model(match)
    base = evaluate(model, ds, _dev(), temperature=TEMPERATURE, nll=True, taxonomic=True)
    tensors = {"thresholds": E2E_THR}
    got = evaluate(model, ds, _dev(), temperature=TEMPERATURE, nll=True, taxonomic=True, hedge=tensors)
    for k, v in base[0].items():
        assert got[0][k] == v or (v != v and got[0][k] != got[0][k]), k
    assert torch.equal(base[1], got[1]) and np.array_equal(base[2], got[2]) and base[3] == got[3]
    extra = set(got[0]) - set(base[0])
    assert extra == {"hedge_thresholds", "hedge_accuracy", "hedge_exact", "hedge_wu_palmer", "hedge_depth", "hedge_mass", "hedge_none"}
    m = got[0]
    assert m["hedge_thresholds"] == list(E2E_THR) and all(len(m[k]) == 2 for k in extra)
    # the restatement
    cand = sorted(ds.all_positions)
    queries = got[3]
    Q = len(queries)
    tix = TaxonomyIndex.from_dataset(ds)
    ix = HedgeIndex.build(tix, cand)
    hg = _encode(model, ds, cand)
    qf = ds.node_features[torch.as_tensor(queries, dtype=torch.long)].to(_dev())
    with torch.no_grad():
        S = scoring.score_all(model.match, hg, qf).cpu().numpy()
        lse = scoring.score_moments_fused(model.match, hg, qf, True, TEMPERATURE).lse.cpu().numpy()
    P = hedge.host_probabilities(S, lse, TEMPERATURE)
    mass = hedge.host_subtree_mass(ix, P)
    want = hedge.host_hedge(ix, None, E2E_THR, mass=mass)
    near = np.zeros(Q, dtype=bool)
    for tau in E2E_THR:
        near |= (np.abs(mass - tau) <= 1e-5).any(axis=0)
    print("hedge end to end:", match, "queries", Q, "left out", int(near.sum()))
    assert near.sum() <= 0.05 * Q
    col, dep, ms = tensors["node_col"].cpu().numpy(), tensors["depth"].cpu().numpy(), tensors["mass"].cpu().numpy()
    assert col.shape == (Q, 2)
    assert np.array_equal(col[~near], want.node_col[~near]) and np.array_equal(dep[~near], want.depth[~near])
    ok = ~near[:, None] & (want.node_col >= 0)
    assert ok.any() and np.abs(ms[ok] - want.mass[ok]).max() <= 1e-5 and np.isnan(ms[col < 0]).all()
    # the metrics are those of the tensors
    node = tensors["node"].cpu().numpy()
    assert np.array_equal(node, np.where(col >= 0, np.asarray(cand)[np.clip(col, 0, None)], -1))
    rel = tensors["relation"].cpu().numpy()
    for t in range(2):
        assert m["hedge_none"][t] == float((col[:, t] < 0).sum()) / Q
        assert m["hedge_exact"][t] == float((rel[:, t] == 0).sum()) / Q and m["hedge_accuracy"][t] == float((rel[:, t] <= 1).sum()) / Q
        assert m["hedge_depth"][t] == float(dep[:, t].sum()) / Q
        assert abs(m["hedge_wu_palmer"][t] - tensors["wu_palmer"].cpu().numpy()[:, t].mean()) < 1e-12
    # an ancestor of a gold parent is a right answer: the laxer threshold never answers shallower than the stricter one
    assert (dep[:, 0] >= dep[:, 1]).all() and m["hedge_none"][0] <= m["hedge_none"][1]
    gold_cols = [[cand.index(a) for a in ds.node2parents[q] if a in set(cand)] for q in queries]
    for i in np.flatnonzero(col[:, 1] >= 0)[:20]:
        if rel[i, 1] <= 1:                                          # exact / ancestor: a gold parent lies in the hedged node's subtree
            assert any(g in ix.row(col[i, 1]).tolist() for g in gold_cols[i]), i


def test_infer_with_hedge(tmp_path):
    """infer(with_scores=True, hedge=0.9): the items' fifth entry and the saved columns agree with hedged_parents on the same encoding"""
    from taxoexpan_amd.evaluate import infer
    from taxoexpan_amd.taxometric import TaxonomyIndex
    ds = _toy(tmp_path)
    model = _model("BIM")
    rs = np.random.RandomState(5)
    names = [f"new_{i}" for i in range(9)]
    vecs = rs.standard_normal((9, 8))
    taxon_file = tmp_path / "new.tsv"
    with open(taxon_file, "w") as f:
        for n, v in zip(names, vecs):
            f.write(n + "\t" + " ".join(repr(float(t)) for t in v) + "\n")
    plain, saved = tmp_path / "plain.tsv", tmp_path / "hedged.tsv"
    base = infer(model, ds, str(taxon_file), _dev(), with_scores=True, temperature=TEMPERATURE, save=str(plain))
    out = infer(model, ds, str(taxon_file), _dev(), with_scores=True, temperature=TEMPERATURE, hedge=0.9, save=str(saved))
    assert [item[:4] for item in out] == base and all(len(item) == 5 and len(item[4]) == 1 for item in out)
    anchors = list(ds.graph.nodes)
    ixd = HedgeIndex.build(TaxonomyIndex.from_dataset(ds), anchors).to(_dev())
    hg = _encode(model, ds, anchors)
    qf = torch.as_tensor(vecs, dtype=torch.float32).to(_dev())
    h = hedge.hedged_parents(model.match, hg, qf, ixd, 0.9, TEMPERATURE)
    col, ms, dp = h.node_col.cpu().tolist(), h.mass.cpu().tolist(), h.depth.cpu().tolist()
    plain_lines, lines = open(plain).read().splitlines(), open(saved).read().splitlines()
    assert lines[0] == plain_lines[0] + "\tHedged parent@0.9\tMass@0.9\tDepth@0.9" and len(lines) == 10
    for i, item in enumerate(out):
        name, mass, depth = item[4][0]
        assert name == (ds.vocab[anchors[col[i][0]]] if col[i][0] >= 0 else None) and depth == dp[i][0]
        assert mass == ms[i][0] or (mass != mass and col[i][0] < 0)
        assert lines[i + 1] == plain_lines[i + 1] + f"\t{name if name is not None else ''}\t{mass:.6g}\t{depth}"
    # blocks of the driver's own choosing and blocks of 64: the same answers
    h2 = hedge.hedged_parents(model.match, hg, qf.repeat(15, 1), ixd, [0.5, 0.9], TEMPERATURE, block=64)
    assert h2.node_col.shape == (135, 2) and torch.equal(h2.node_col[:9, 1], h.node_col[:, 0]) and torch.equal(h2.node_col[126:], h2.node_col[:9])
