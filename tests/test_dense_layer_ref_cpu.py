"""The float64 references of tests/test_gpu_dense_layer_ops.py (tests/dense_layer_ref.py) against the oracle's own layers, which the
reference goldens pin -- gat_dense against the projection step of orc.gat_layer (ft, a1, a2), gcn_dense against orc.gcn_layer on a graph
of self loops (norm 1, every node its own only source), build_x against the input concatenation of orc.pgat_forward -- in float64 to
1e-12 of the tensor's largest entry; the backward's activation factor; that the fp32 yardstick runs; and the ROUTE ARITHMETIC: every
host predicate evaluated for every case of the tables, each route named on either side of its threshold."""
import numpy as np
import pytest
import torch

import dense_layer_ref as dl
import txe_oracle as orc


def _close(got, want, what):
    got, want = got.detach().numpy(), want.detach().numpy()
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), what


def _inputs(n, Kh, Pd, H, D, seed=3):
    rs = np.random.RandomState(seed)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s))
    return dict(h=t(n, Kh), P=t(3, Pd), pos=torch.from_numpy(rs.randint(0, 3, n)), W=t(H * D, Kh + Pd), al=t(H, D), ar=t(H, D),
                keep=torch.from_numpy((rs.random_sample((n, Kh + Pd)) >= 0.3).astype(np.float64)))


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_gat_dense_reference_is_the_oracle_projection_step(p):
    n, Kh, Pd, H, D = 37, 7, 3, 3, 5
    a = _inputs(n, Kh, Pd, H, D)
    X = dl.build_x(a["h"], a["pos"], a["P"])
    src = dst = torch.arange(n)
    keep = a["keep"] if p else None
    _out, parts = orc.gat_layer(src, dst, n, X, a["W"], a["al"].reshape(1, H, D), a["ar"].reshape(1, H, D), 0.2, feat_keep=keep, feat_scale=1.0 / (1.0 - p),
                                return_parts=True)
    Y = dl.gat_dense(X, a["W"], a["al"], a["ar"], keep, p)
    assert Y.dtype == torch.float64 and Y.shape == (n, H * D + 2 * H)
    _close(Y[:, :H * D], parts["ft"].reshape(n, H * D), "ft")
    _close(Y[:, H * D:H * D + H], parts["a1"].reshape(n, H), "a1")
    _close(Y[:, H * D + H:], parts["a2"].reshape(n, H), "a2")
    # the folded rows give the same logits as one more product: a1 = dropout(X) wa^T
    wa = dl.folded_rows(a["W"], a["al"], a["ar"])
    _close((X * keep / (1.0 - p) if p else X) @ wa.t(), Y[:, H * D:], "a12 through the folded rows")


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_gcn_dense_reference_is_the_oracle_layer_on_self_loops(p):
    n, Kh, Pd, Fo = 37, 7, 3, 5
    a = _inputs(n, Kh, Pd, 1, Fo)
    X = dl.build_x(a["h"], a["pos"], a["P"])
    W = a["W"].t().contiguous()
    src = dst = torch.arange(n)
    keep = a["keep"] if p else None
    want = orc.gcn_layer(src, dst, n, X, W, None, orc.gcn_norm(dst, n, torch.float64), keep=keep, keep_scale=1.0 / (1.0 - p))
    _close(dl.gcn_dense(X, W, keep, p), want, "hw")


def test_build_x_reference_is_the_oracle_input_concatenation():
    n, Kh, Pd, H, D = 37, 7, 3, 3, 5
    a = _inputs(n, Kh, Pd, H, D)
    params = {"gat_layers.0.fc.weight": a["W"], "gat_layers.0.attn_l": a["al"].reshape(1, H, D), "gat_layers.0.attn_r": a["ar"].reshape(1, H, D),
              "prop_position_embeddings.0.weight": a["P"]}
    src = dst = torch.arange(n)
    _h, parts = orc.pgat_forward(params, dict(src=src, dst=dst, pos=a["pos"], num_nodes=n), a["h"], [H], 0, return_parts=True)
    X = dl.build_x(a["h"], a["pos"], a["P"])
    assert X.shape == (n, Kh + Pd) and torch.equal(X[:, :Kh], a["h"]) and torch.equal(X[:, Kh:], a["P"][a["pos"]])
    _close(dl.gat_dense(X, a["W"], a["al"], a["ar"], None, 0.0)[:, :H * D], parts[0]["ft"].reshape(n, H * D), "ft of the stack's first layer")
    assert dl.build_x(a["h"], a["pos"], None) is a["h"] and dl.build_x(a["h"], a["pos"], a["P"][:, :0]) is a["h"]


@pytest.mark.parametrize("kind", ["gat", "gcn"])
def test_backward_is_autograd_of_the_oracle_and_carries_the_activation_factor(kind):
    """backward() against the closed forms d_X = (dY Wfull) keep / (1 - p) [x leaky'(h) on columns < Kh], dP = the rows of d_X summed by
    class, dW = dY^T dropout(X) -- with Wfull = [W; wa] for the GAT layer -- and the fp32 yardstick beside it"""
    n, Kh, Pd, H, D, p, slope = 41, 6, 3, 2, 4, 0.3, 0.01
    a = {k: v.numpy() for k, v in _inputs(n, Kh, Pd, H, D, 4).items()}
    W = a["W"] if kind == "gat" else np.ascontiguousarray(a["W"].T)
    Fe = H * D + 2 * H if kind == "gat" else H * D
    seed = np.random.RandomState(5).standard_normal((n, Fe))
    attn = (a["al"], a["ar"]) if kind == "gat" else None
    g = dl.backward(kind, torch.float64, a["h"], a["P"], a["pos"], W, attn, a["keep"], p, seed, True, slope)
    X = np.concatenate([a["h"], a["P"][a["pos"]]], 1)
    Wfull = np.concatenate([a["W"], dl.folded_rows(*(torch.from_numpy(v) for v in (a["W"], a["al"], a["ar"]))).numpy()], 0) if kind == "gat" else a["W"]
    dX = seed @ Wfull * a["keep"] / (1.0 - p)
    dX[:, :Kh] *= np.where(a["h"] > 0, 1.0, slope)
    np.testing.assert_allclose(g["d_X"], dX, rtol=1e-12, atol=1e-13)
    dP = np.stack([dX[a["pos"] == c, Kh:].sum(0) for c in range(3)])
    np.testing.assert_allclose(g["dP"], dP, rtol=1e-12, atol=1e-13)
    if kind == "gcn":
        np.testing.assert_allclose(g["dW"], (X * a["keep"] / (1.0 - p)).T @ seed, rtol=1e-12, atol=1e-13)
    plain = dl.backward(kind, torch.float64, a["h"], a["P"], a["pos"], W, attn, a["keep"], p, seed, False)
    assert np.array_equal(plain["d_X"][:, Kh:], g["d_X"][:, Kh:]) and not np.array_equal(plain["d_X"][:, :Kh], g["d_X"][:, :Kh])   # the factor stops at Kh
    for k in ("dW", "dP"):
        assert np.array_equal(plain[k], g[k]), k                        # (the VALUES behind the activation are h's own)
    y = dl.backward(kind, torch.float32, *(v.astype(np.float32) for v in (a["h"], a["P"])), a["pos"], W.astype(np.float32),
                    tuple(v.astype(np.float32) for v in attn) if attn else None, a["keep"].astype(np.float32), p, seed.astype(np.float32), True, slope)
    for k, v in g.items():
        assert y[k].dtype == np.float32 and 0 < np.abs(y[k] - v).max() <= 1e-5 * np.abs(v).max(), k


# ---- route arithmetic ---------------------------------------------------------------------------------------------------------------------------
def test_padded_widths_of_the_tables():
    assert [dl.padded_k(c[1], c[2]) for c in dl.FWD_CASES] == [32, 32, 320, 64, 320]
    assert [c[3] * c[4] + 2 * c[3] for c in dl.FWD_CASES] == [3, 21, 104, 130, 128] and [dl.padded_f(c[3], c[4]) for c in dl.FWD_CASES] == [128, 128, 128, 256, 128]
    assert dl.FWD_CASES[4][1] % 4 == 3 and dl.FWD_CASES[2][0] == 129 and len(dl.GCN_FWD_FO) == len(dl.FWD_CASES)
    assert dl.tail_ws_bytes() == 2 * 256 * (128 * 128 + 256) * 4


def test_forward_cases_reach_the_tail_split_on_both_layouts():
    """the tail split needs a tail workspace and >= 8 k-tiles (Kp >= 256): (129, 250, 50) and (257, 251, 62) take it, the others do not,
    and nobody takes it without the workspace.  One round of tiles always costs less on 64-wide ones (choose_bn: 64 x 1.6 < 128), so
    every shape a unit test can afford runs the <..., 64> instances; the 128-wide ones need more than 512 tiles and stay with the
    full-size tests"""
    names = {}
    for (n, Kh, Pd, H, D), Fo in zip(dl.FWD_CASES, dl.GCN_FWD_FO):
        for tail in (False, True):
            names[("gat", n, tail)] = dl.gat_fwd_launches(n, Kh, Pd, H, D, tail)
            names[("gcn", n, tail)] = dl.gcn_fwd_launches(n, Kh, Pd, Fo, tail)
    fixed = {k for k, v in names.items() if len(v) == 2}
    assert fixed == {("gat", 129, True), ("gcn", 129, True), ("gat", 257, True), ("gcn", 257, True)}, fixed
    assert all(v[1].startswith("gemm_tail_fixup_kernel<") for k, v in names.items() if k in fixed)
    flat = {v[0] for v in names.values()}
    assert flat == {f"gemm_kernel<true, {b}, 4, 4, 64>" for b in ("true", "false")}, flat
    assert dl.choose_bn(128 * 200, 130, 1, False, 320) == 128 and dl.choose_bn(128 * 100, 130, 1, False, 320) == 64
    # on either side of the k-tile threshold of the rule itself
    assert dl.tail_split_slices(129, 104, 256, 64, True) == 2 and dl.tail_split_slices(129, 104, 224, 64, True) == 0
    assert dl.tail_split_slices(129, 104, 320, 64, False) == 0 and dl.tail_split_slices(128 * 512, 128, 320, 128, True) == 0    # (whole rounds: no tail)


def test_position_only_dx_cases_sit_on_both_sides_of_the_streaming_predicate():
    for n, Kh, Pd, H, D, streams in dl.BWD_POS_CASES:
        assert dl.dx_streams(Kh, Pd, 0) == streams and dl.dx_streams(Kh, Pd, 1) == 0
        c0 = dl.dx_c0(Kh, 0)
        assert c0 == Kh // 4 * 4 and c0 % 4 == 0 and dl.dx_c0(Kh, 1) == 0
        for masked in (False, True):
            names = dl.gat_dx_launches(n, Kh, Pd, H, D, 0, masked, False, False)
            assert names == (["gat_dx_pos_kernel"] if streams else ["gemm_kernel<true, false, 4, 4, 64>"]), names      # (65 and 72 columns: two 64-wide tiles)
    (_n, Kh1, Pd1, *_r), (_n2, Kh2, Pd2, *_r2), (_n3, Kh3, Pd3, *_r3) = dl.BWD_POS_CASES
    assert Kh1 % 4 == 3 and Pd1 <= 64 < Kh1 % 4 + Pd1                      # the straddling quad's feature columns push the range past 64
    assert Pd2 > 64 and Kh2 % 4 == 2                                       # wider than the kernel's 64 columns on its own
    assert Kh3 + Pd3 - Kh3 // 4 * 4 == 52 <= 64 and (Kh3, dl.padded_k(Kh3, Pd3)) == (Kh2, dl.padded_k(Kh1, Pd1))   # the same width class, streaming
    assert dl.dx_streams(250, 62, 0) == 1 and dl.dx_streams(250, 63, 0) == 0 and dl.dx_streams(250, 0, 0) == 0      # the threshold itself


def test_need_dh_cases_reach_the_epilogue_and_the_tail_fixup():
    fix, plain = set(), set()
    for n, Kh, Pd, H, D in dl.BWD_DH_CASES:
        for masked in (False, True):
            for act in (False, True):
                names = dl.gat_dx_launches(n, Kh, Pd, H, D, 1, masked, act, False)
                assert names[0].startswith("gemm_kernel<true, false, 4, 4, ")
                (fix if len(names) == 2 else plain).add((H, D))
                assert dl.gat_dx_launches(n, Kh, Pd, H, D, 1, masked, act, True) == ["split_pack_kernel", "split_pack_kernel", "gemm_nt_split_kernel<2, 3, 2, 1>"]
    assert plain == {(2, 24)} and fix == {(4, 63)}                         # Fp 128: 4 k-tiles, the GEMM's own epilogue; Fp 384: 12, the fix-up
    assert dl.padded_f(2, 24) == 128 and dl.padded_f(4, 63) == 384 and {c[2] for c in dl.BWD_DH_CASES} == {0, 16, 50}
    for n, Kh, Pd, H, D in dl.BWD_DH_CASES + [c[:5] for c in dl.BWD_POS_CASES]:
        assert dl.split_tn_eligible(dl.padded_f(H, D), dl.padded_k(Kh, Pd))        # Xt is there for every case (Fp % 128 == 0 by construction)
        assert dl.gat_dw_launches(n, Kh, Pd, H, D, False, True) == ["gemm_tn_split_kernel"]
        dw = dl.gat_dw_launches(n, Kh, Pd, H, D, True, False)
        assert len(dw) == 1 and dw[0].startswith("gemm_kernel<false, false, 4, 4, ") and not dw[0].endswith("160>"), dw
    assert not dl.split_tn_eligible(130, 64) and not dl.split_tn_eligible(128, 6) and dl.split_tn_eligible(128, 4)
    # gemm_tn_lds_kernel inside txe_gat_dense_bwd needs 2 Fp Kp n >= 2e10: out of a unit test's reach
    assert all(2.0 * dl.padded_f(H, D) * dl.padded_k(Kh, Pd) * n < 2e10 for n, Kh, Pd, H, D in dl.BWD_DH_CASES)
    assert dl.gemm_launches("tn", 1024, 320, 32768, dl.choose_splits(1024, 320, 32768)) == ["gemm_tn_lds_kernel"]


def test_gcn_cases_sit_on_both_sides_of_the_transposed_route():
    for n, Kh, Pd, Fo in dl.GCN_CASES:
        for masked in (False, True):
            for xd in (0, 1):
                assert not dl.gcn_dw_transposed(n, dl.padded_k(Kh, Pd), dl.gcn_padded_f(Fo), masked, xd)
                last = dl.gcn_bwd_launches(n, Kh, Pd, Fo, 1, masked, False, xd)[-1]
                assert last.startswith("gemm_kernel<false, false, 4, 4, "), last
    seen = set()
    for n, Kh, Pd, p, xd, transposed in dl.GCN_DWT_CASES:
        for Fo in dl.GCN_DWT_FO:
            Kp, Fop = dl.padded_k(Kh, Pd), dl.gcn_padded_f(Fo)
            assert dl.gcn_dw_transposed(n, Kp, Fop, p > 0, xd) == transposed, (n, Kh, Pd, p, xd, Fo)
            last = dl.gcn_bwd_launches(n, Kh, Pd, Fo, 0, p > 0, False, xd)[-1]
            assert (last == "gemm_tn_lds_kernel") == transposed, last
            seen.add((n, Kp, p > 0, xd, transposed))
    assert seen == {(4096, 320, False, 0, True), (4096, 288, False, 0, True), (4096, 160, False, 0, True), (4096, 256, False, 0, False), (4095, 320, False, 0, False),
                    (4096, 320, True, 0, False), (4096, 320, True, 1, True)}
    # the predicate's own thresholds: 160-column tiles must pad no more than 64-column ones; >= 8 k-tiles per slice, >= 2 slices
    assert [dl.gcn_dwt_splits(4096, kp, 64) > 0 for kp in (160, 256, 288, 320)] == [True, False, True, True]     # (288 pads to 320 either way)
    assert dl.gcn_dwt_splits(4096, 320, 64) == 16 and dl.gcn_dwt_splits(4096, 320, 512) == 16 and dl.gcn_dwt_splits(4095, 320, 64) == 0
    assert dl.gcn_dwt_splits(1 << 20, 320, 32) == 64 and dl.gcn_dwt_splits(4096, 320, 128 * 200) == 0


def test_preparation_cases_cover_their_variants():
    c = dl.PREP_CASES
    assert {x[4] for x in c} == {True, False} and {x[6] for x in c} == {0, 1} and {x[7] for x in c} == {True, False} and any(x[5] > 0 for x in c)
    assert all((x[1] + x[2]) % 32 != 0 for x in c if x[7])                 # a bias row needs a padding row
    assert any(x[1] % 2 == 1 and x[5] % 2 == 1 for x in c) and any(x[2] == 0 for x in c) and any(x[1] % 4 == 3 for x in c)
    assert dl.PREP_MAXL == 4
