"""The float64 references of tests/test_gpu_folded_layer_ops.py (tests/folded_layer_ref.py) against the oracle's own layers and readouts,
which the reference goldens pin -- gat_fold against orc.gat_layer + orc.weighted_mean_readout / mean_readout, below_then_fold against
orc.pgat_forward (one hidden layer) + readout, gcn_fold against orc.gcn_layer + readout: in float64 on batches A and C, to 1e-12 of the
tensor's largest entry.  Also: the branch-audit rule on the fp32 yardstick's own branches, what the four batches promise, and the
INSTANCE ARITHMETIC -- the case tables of the GPU file reach every kernel instance of the folded layer's host dispatch."""
import numpy as np
import pytest
import torch

import folded_layer_ref as fl
import message_passing_ref as mp
import txe_oracle as orc


def _close(got, want, what):
    got, want = got.detach().numpy(), want.detach().numpy()
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), what


def _csr(b):
    s, d = mp.in_csr_order(b["src"], b["dst"])
    return torch.from_numpy(s), torch.from_numpy(d), torch.from_numpy(b["graph_off"]), torch.from_numpy(b["pos"])


def _readout(goff, hn, pos, pw):
    return orc.weighted_mean_readout(goff, hn, pos, pw) if pw is not None else orc.mean_readout(goff, hn)


@pytest.mark.parametrize("bname", ["A", "C"])
@pytest.mark.parametrize("weighted", [True, False], ids=["wmr", "mr"])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_gat_fold_reference_is_the_oracle_layer_behind_its_readout(bname, weighted, p):
    b = fl.batch(bname)
    src, dst, goff, pos = _csr(b)
    n, E, Kt, D = b["n"], len(src), 14, 6
    rs = np.random.RandomState(5)
    X, W = torch.from_numpy(rs.standard_normal((n, Kt))), torch.from_numpy(rs.standard_normal((D, Kt)))
    al, ar = torch.from_numpy(rs.standard_normal(D)), torch.from_numpy(rs.standard_normal(D))
    pw = torch.from_numpy(fl.PW).double() if weighted else None
    keep = torch.from_numpy((rs.random_sample((n, Kt)) >= p).astype(np.float64)) if p else None
    akeep = torch.from_numpy((rs.random_sample(E) >= p).astype(np.float64)) if p else None
    sc = 1.0 / (1.0 - p)
    hn, parts = orc.gat_layer(src, dst, n, X, W, al.reshape(1, 1, D), ar.reshape(1, 1, D), 0.2, feat_keep=keep, feat_scale=sc,
                              attn_keep=akeep.reshape(E, 1, 1) if p else None, attn_scale=sc, return_parts=True)
    want = _readout(goff, hn.mean(1), pos, pw)
    r = fl.gat_fold(X, keep, sc, W, al, ar, src, dst, goff, pos, pw, 0.2, akeep, sc)
    assert r["hg"].dtype == torch.float64
    _close(r["hg"], want, "hg")
    _close(r["a12"], torch.cat([parts["a1"].reshape(n, 1), parts["a2"].reshape(n, 1)], 1), "a12")
    _close(r["alpha"], parts["alpha"].reshape(E), "alpha")
    _close(r["Z"] @ W.t(), want, "hg = Z W^T")
    w = fl.readout_weights(pos, pw, n, torch.float64)
    _close(r["wsum"], orc.segment_sum(goff, w), "wsum")
    # given branches that ARE the function's own change nothing; the logits as an input (A12_READY) neither
    own = (r["a12"][src, 0] + r["a12"][dst, 1] > 0).numpy().astype(np.int32)
    r2 = fl.gat_fold(X, keep, sc, W, al, ar, src, dst, goff, pos, pw, 0.2, akeep, sc, e_pos=own, a12=r["a12"])
    _close(r2["hg"], want, "hg, branches and logits given")


@pytest.mark.parametrize("bname", ["A", "C"])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_below_then_fold_reference_is_the_oracle_two_layer_stack(bname, p):
    b = fl.batch(bname)
    src, dst, goff, pos = _csr(b)
    n, E, K0, Hp, Dp, Pd, D = b["n"], len(src), 5, 4, 4, 3, 6
    rs = np.random.RandomState(6)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s))
    params = {"gat_layers.0.fc.weight": t(Hp * Dp, K0 + Pd), "gat_layers.0.attn_l": t(1, Hp, Dp), "gat_layers.0.attn_r": t(1, Hp, Dp),
              "gat_layers.1.fc.weight": t(D, Hp * Dp + Pd), "gat_layers.1.attn_l": t(1, 1, D), "gat_layers.1.attn_r": t(1, 1, D),
              "prop_position_embeddings.0.weight": t(3, Pd), "prop_position_embeddings.1.weight": t(3, Pd)}
    h = t(n, K0)
    sc = 1.0 / (1.0 - p)
    k = lambda *s: torch.from_numpy((rs.random_sample(s) >= p).astype(np.float64))
    masks = None
    keep_p = keep = akeep = None
    if p:
        keep_p, keep, akeep = k(E, Hp), k(n, Hp * Dp + Pd), k(E)
        masks = [dict(attn_keep=keep_p.unsqueeze(-1), attn_scale=sc), dict(feat_keep=keep, feat_scale=sc, attn_keep=akeep.reshape(E, 1, 1), attn_scale=sc)]
    graph = dict(src=src, dst=dst, pos=pos, num_nodes=n)
    hn, parts = orc.pgat_forward(params, graph, h, [Hp, 1], 1, masks=masks, return_parts=True)
    pw = torch.from_numpy(fl.PW).double()
    want = orc.weighted_mean_readout(goff, hn, pos, pw)
    W, al, ar = params["gat_layers.1.fc.weight"], params["gat_layers.1.attn_l"].reshape(D), params["gat_layers.1.attn_r"].reshape(D)
    fold = lambda Xn: fl.gat_fold(Xn, keep, sc, W, al, ar, src, dst, goff, pos, pw, 0.2, akeep, sc)
    r, Xn, alpha_p = fl.below_then_fold(parts[0]["ft"], parts[0]["a1"].squeeze(-1), parts[0]["a2"].squeeze(-1), src, dst, 0.2, keep_p, sc, 0.01, None,
                                        params["prop_position_embeddings.1.weight"], pos, fold)
    _close(r["hg"], want, "hg")
    _close(alpha_p, parts[0]["alpha"].squeeze(-1), "alpha of the layer below")
    _close(r["alpha"], parts[1]["alpha"].reshape(E), "alpha of the folded layer")
    # the activation's branches given as the stored X' has them: the same function
    r2, _x, _a = fl.below_then_fold(parts[0]["ft"], parts[0]["a1"].squeeze(-1), parts[0]["a2"].squeeze(-1), src, dst, 0.2, keep_p, sc, 0.01,
                                    (Xn[:, :Hp * Dp] > 0).numpy().astype(np.int32), params["prop_position_embeddings.1.weight"], pos, fold)
    _close(r2["hg"], want, "hg, activation branches given")


@pytest.mark.parametrize("bname", ["A", "C"])
@pytest.mark.parametrize("weighted,bias,p", [(True, True, 0.0), (False, False, 0.3), (True, False, 0.3), (False, True, 0.0)])
def test_gcn_fold_reference_is_the_oracle_layer_behind_its_readout(bname, weighted, bias, p):
    b = fl.batch(bname)
    src, dst, goff, pos = _csr(b)
    n, Kt, Fo = b["n"], 14, 6
    rs = np.random.RandomState(7)
    X, W = torch.from_numpy(rs.standard_normal((n, Kt))), torch.from_numpy(rs.standard_normal((Kt, Fo)))
    bv = torch.from_numpy(rs.standard_normal(Fo)) if bias else None
    pw = torch.from_numpy(fl.PW).double() if weighted else None
    keep = torch.from_numpy((rs.random_sample((n, Kt)) >= p).astype(np.float64)) if p else None
    sc = 1.0 / (1.0 - p)
    hn = orc.gcn_layer(src, dst, n, X, W, bv, orc.gcn_norm(dst, n, torch.float64), keep=keep, keep_scale=sc)
    want = _readout(goff, hn, pos, pw)
    r = fl.gcn_fold(X, keep, sc, W, bv, src, dst, goff, pos, pw)
    assert r["hg"].dtype == torch.float64
    _close(r["hg"], want, "hg")
    _close(r["Z"] @ W + (bv if bias else 0.0), want, "hg = Z W + b")


@pytest.mark.parametrize("bname", ["A", "B", "C"])
def test_fp32_yardstick_branches_stay_inside_the_audit_bound(bname):
    """with standard-normal inputs the branches the fp32 CPU run takes -- the sign of the fp32 sum a1[u] + a2[v] of ITS a12, the sign of
    ITS X' -- pass the audit against the float64 pre-activations (the bound the GPU file holds the device's stored state to)"""
    b = fl.batch(bname)
    src, dst, goff, pos = _csr(b)
    n, E, Hp, Dp, Pd, D = b["n"], len(src), 4, 16, 4, 6
    F_ = Hp * Dp
    rs = np.random.RandomState(8)
    a = {k: rs.standard_normal(s).astype(np.float32) for k, s in dict(ft=(n, Hp, Dp), a1=(n, Hp), a2=(n, Hp), P=(3, Pd), W=(D, F_ + Pd), al=(D,), ar=(D,)).items()}
    a["W"] /= np.sqrt(F_ + Pd)

    def run(dtype, act_pos, e_pos):
        t = {k: torch.from_numpy(v).to(dtype) for k, v in a.items()}
        fold = lambda Xn: fl.gat_fold(Xn, None, 1.0, t["W"], t["al"], t["ar"], src, dst, goff, pos, torch.from_numpy(fl.PW).to(dtype), 0.2, e_pos=e_pos)
        return fl.below_then_fold(t["ft"], t["a1"], t["a2"], src, dst, 0.2, None, 1.0, 0.01, act_pos, t["P"], pos, fold)
    r32, X32, _a = run(torch.float32, None, None)
    a12 = r32["a12"].numpy()
    e_pos = (a12[src.numpy(), 0] + a12[dst.numpy(), 1] > 0).astype(np.int32)
    _out, audit = fl.audited(lambda: run(torch.float64, (X32[:, :F_].numpy() > 0).astype(np.int32), e_pos))
    assert {r[0] for r in audit} == {"folded attention logits", "activation between the layers"}
    fl.audit_rule(audit)


def test_the_batches_hold_what_the_gpu_cases_rely_on():
    A, B, B15, C, E = (fl.batch(k) for k in ("A", "B", "B15", "C", "E"))
    deg = lambda b: (np.bincount(b["dst"], minlength=b["n"]), np.bincount(b["src"], minlength=b["n"]))
    # A: G < 16 (per-graph Z sweep); graphs on both sides of 64 nodes; the second 8-graph workgroup past the 512 LDS-staged nodes
    assert A["G"] == 15 and A["n"] == 992 and not fl.zsum_chunked(A["n"], A["G"])
    assert A["sizes"].min() < 64 < A["sizes"].max() and 64 in A["sizes"] and A["graph_off"][15] - A["graph_off"][8] == 785 > 512
    # B: chunked sweep, a last chunk of three graphs, the empty graphs, the special graphs
    assert B["G"] == 43 and B["G"] % 4 == 3 and fl.zsum_chunked(B["n"], B["G"]) and B["sizes"].max() == 16
    assert [i for i in range(43) if B["sizes"][i] == 0] == list(fl.B_EMPTY) and fl.B_EMPTY[-1] == 42
    assert B["sizes"][0] == 1 and B["sizes"][1] == 2 and B["sizes"][fl.B_NOT_HUB] == 10
    o = B["graph_off"][fl.B_NOT_HUB]
    outdeg_nh = deg(B)[1][o:o + 10]
    assert sorted(outdeg_nh.tolist()) == [1] * 5 + [2] * 4 + [7]             # sibling 5 has two out-edges but is no parent: not hub-shaped
    assert deg(B)[0].max() > 8 and deg(B)[1].max() > 8                      # heavy nodes on both sides
    assert B15["G"] == 15 and not fl.zsum_chunked(B15["n"], 15) and np.array_equal(B15["sizes"], B["sizes"][:15])
    assert np.array_equal(B15["src"], B["src"][:len(B15["src"])]) and np.array_equal(B15["pos"], B["pos"][:B15["n"]])
    # C: the hub, the 400 out-edges, nodes without in-edges, the circulant graph that overflows the heavy lists
    ind, outd = deg(C)
    assert C["G"] == 9 and ind.max() > 64 and outd.max() >= 400 and (ind == 0).any() and C["sizes"][-1] == 300
    o = C["graph_off"][8]
    assert (ind[o:] == 9).all() and (outd[o:] == 9).all() and 300 > 256
    # E: C with 45 empty graphs in a row
    assert E["G"] == 54 and E["n"] == C["n"] and (E["sizes"][4:49] == 0).all() and np.array_equal(E["pos"], C["pos"])
    assert np.array_equal(E["src"], C["src"]) and not fl.zsum_chunked(C["n"], C["G"])
    assert fl.zsum_chunked(E["n"], E["G"])                                  # (chunks of four EMPTY graphs, and a 300-node graph in a chunk)
    # the widened logits: a softmax that spans more than 180
    a12 = np.random.RandomState(0).standard_normal((A["n"], 2)).astype(np.float32)
    v = fl.widen_fold_logits(A, a12)
    e = orc._leaky(torch.from_numpy(a12[A["src"], 0] + a12[A["dst"], 1]), 0.2).numpy()[A["dst"] == v]
    assert e.max() - e.min() > 180.0
    with np.errstate(over="ignore"):
        assert np.exp(e.astype(np.float32)).max() == np.inf


# ---- instance arithmetic ----------------------------------------------------------------------------------------------------------------
def _sizes(bn):
    b = fl.batch(bn)
    return b["n"], b["G"]


def test_forward_cases_reach_every_instance_of_the_logits_and_z_sweeps():
    assert [fl.padded_k(Kh, Pd) for Kh, Pd, _kp in fl.FWD_WIDTHS] == [kp for _a, _b, kp in fl.FWD_WIDTHS] == [32, 256, 320, 1024, 2080, 2464, 2592]
    names = set()
    for Kh, Pd, bn in fl.FWD_CASES:
        for m in fl.MASKS:
            names |= set(fl.fwd_launches(*_sizes(bn), m))
    names |= {fl.zsum_kernel(*_sizes("B"), m, edot=True) for m in fl.MASKS}        # (the TXE_FUSED_EDOT cases, on B)
    T = ("true", "false")
    assert names == ({f"cl_logits_kernel<{m}>" for m in T} | {f"cl_zsum_kernel<{m}>" for m in T}
                     | {f"cl_zsum_chunk_kernel<{m}, {e}>" for m in T for e in T})
    # both sweeps at every width; nmap = ntile + 1 at ntile 4 (Kp 1024) and nmap = ntile beside it; tiles 1 .. 11, partial last tiles
    assert all({"A", "B"} <= {bn for Kh, Pd, bn in fl.FWD_CASES if fl.padded_k(Kh, Pd) == kp} for _a, _b, kp in fl.FWD_WIDTHS)
    assert fl.zsum_tiles(1024) == (4, 5) and fl.zsum_tiles(2080) == (9, 9) and fl.zsum_tiles(32) == (1, 1) and fl.zsum_tiles(2592) == (11, 11)
    assert {kp for kp in fl.FWD_OPTION_WIDTHS} <= {kp for _a, _b, kp in fl.FWD_WIDTHS} and len(fl.FWD_OPTION_WIDTHS) == 3


def test_backward_cases_reach_every_instance_of_the_dot_and_dx_sweeps():
    assert [fl.padded_k(Kh, Pd) for Kh, Pd, _kp in fl.BWD_WIDTHS] == [kp for _a, _b, kp in fl.BWD_WIDTHS]
    assert [kp // 4 for _a, _b, kp in fl.BWD_WIDTHS] == [8, 64, 72, 320, 328, 576, 584, 640, 648]      # both sides of every switch, in tiles of 8 vectors
    dot, dx = set(), set()
    for Kh, Pd, bn in fl.BWD_CASES:
        for m in fl.MASKS:
            d, x = fl.bwd_launches(fl.padded_k(Kh, Pd), m)
            dot.add(d); dx.add(x)
    for Kh, Pd, Fo, bn in fl.GCN_CASES:
        for m in fl.MASKS:
            dx.add(fl.bwd_launches(fl.padded_k(Kh, Pd), m, att=False, dot=False)[0])
    T = ("true", "false")
    assert dot == {f"cl_bwd_dot_kernel<{m}>" for m in T} | {f"cl_bwd_dot_row_kernel<{m}, {nt}>" for m in T for nt in (5, 9, 10)}
    assert dx == {f"cl_bwd_dx_kernel<{m}, {a}>" for m in T for a in T}
    # the switch points themselves
    for lo, hi in ((64, 65), (320, 321), (576, 577), (640, 641)):
        assert fl.bwd_dot_kernel(4 * lo, False) != fl.bwd_dot_kernel(4 * hi, False)
    assert {fl.padded_k(Kh, Pd) for Kh, Pd, Fo, bn in fl.GCN_CASES} == {32, 320, 2080} and {Fo for _a, _b, Fo, _c in fl.GCN_CASES} == {6, 250}


def test_fused_cases_reach_all_32_instances_and_every_tail():
    assert all(fl.fused_supported(Hp * Dp, Pd, Hp, Dp) for Hp, Dp, Pd in fl.FUSED_SHAPES)
    names = {fl.fused_kernel(m, Hp, Dp, ne) for Hp, Dp, Pd, bn, ne in fl.FUSED_CASES for m in fl.MASKS}
    T = ("true", "false")
    want = {f"gat_fused_bwd_kernel<{m}, {ni}, {nw}>" for m in T for ni in (1, 2, 3, 4) for nw in (1, 2, 4)}
    want |= {f"gat_fused_bwd_ego_kernel<{m}, {ni}>" for m in T for ni in (1, 2, 3, 4)}
    assert len(want) == 32 and names == want
    tails = {fl.padded_k(Hp * Dp, Pd) - Hp * Dp for Hp, Dp, Pd in fl.FUSED_SHAPES}
    assert {0, 16, 80, 128} <= tails                      # no tail; padding only; the MAG shape's; the widest the entry point accepts
    assert not fl.fused_supported(4 * 512, 129, 4, 512) and not fl.fused_supported(24, 4, 3, 8) and not fl.fused_supported(40, 0, 2, 20)
    # the <dZ, X> sweep of the fused cases: all four dot instances as well
    assert {fl.bwd_dot_kernel(fl.padded_k(Hp * Dp, Pd), False) for Hp, Dp, Pd in fl.FUSED_SHAPES} == \
        {"cl_bwd_dot_kernel<false>"} | {f"cl_bwd_dot_row_kernel<false, {nt}>" for nt in (5, 9, 10)}
    assert set(fl.FUSED_ON_BCE) <= set(fl.FUSED_SHAPES)
