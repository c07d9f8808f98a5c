"""The readout kernels (txe_readout.hip) and the matchers' training forms (txe_match.hip) against the oracle in FLOAT64, operator by
operator, at every edge of their dispatch: all nine readout_{fwd,bwd}_kernel<VEC,NI> instances (asserted through the library profiler)
and the second pass of their vector loop, egonets on both sides of the 64-node chunk, strided and misaligned inputs, the softplus /
sigmoid threshold; the second column pass, ties and NaN of the Sum / Max / Concat readouts; the bilinear pair and run forms past 512
columns (several passes of rowdot_runs_kernel, column tiles of runs_bwd_kernel); nn.Linear over the virtual concat at the MLP matcher's
MAG widths, with the split-K weight gradient, tanh, a missing second gradient, a strided input and an empty batch.

Reference: the oracle/txe_oracle.py function of the operation (F.linear for the linear layer) in float64 on the same inputs; yardstick:
the same function in fp32 on the CPU; gate: golden_util.gate_against_f64 with its defaults (2 x the yardstick's own error, floor 2e-5
and cap 1e-4 of the tensor's largest entry), for the output and for every gradient.  Every gate prints its figures
("[gate] operator what device-error yardstick-error", errors as fractions of the tensor's largest float64 entry).

Measured on the MI355X, largest device error / yardstick error per operator over all cases of this file (and the largest device error
itself; the floor is 2e-5):
    WeightedMeanReadout            1.9  (d_pw; largest device error 3.1e-6)
    MeanReadout                    2.0  (d_h, 2.2e-8 against 1.1e-8: under the floor; largest 7.4e-8)
    SumReadout                     1.0  (largest 5.8e-7)
    MaxReadout                     exact on both sides
    ConcatReadout                  2.0  (d_h, 1.8e-8: under the floor; largest 3.8e-8)
    BilinearPairFunction           4.8  (d_e2, 1.3e-6: under the floor); query-side form 4.0 (dW, 9.0e-8; largest 6.1e-7)
    BilinearRunsFunction           1.8  (dW; largest 8.9e-7); BilinearStackedRunsFunction the same figures
    LinearFunction                 5.2  (y, 1.7e-6: under the floor, the largest device error of the operator)
The 96 cases take 8 s on the MI355X, most of it the CPU references.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import txe_oracle as orc
from golden_util import gate_against_f64

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


# ---- the batch of sections 1 and 2 ------------------------------------------------------------------------------------------------
# (k grand-parents, m siblings): node counts 1, 2, 3, 4, 5 (the remainders of the 2- and 4-node unrolled sweeps), 63..68 and 127..129
# (both sides of one and two full 64-node chunks, and the look-ahead past a full chunk), 200; every position class empty somewhere
EGONETS = [(0, 0), (0, 1), (2, 0), (1, 2), (2, 2), (20, 42), (3, 60), (0, 64), (30, 35), (66, 0), (7, 60), (40, 86), (64, 63), (1, 127),
           (99, 100)]
assert [k + 1 + m for k, m in EGONETS] == [1, 2, 3, 4, 5, 63, 64, 65, 66, 67, 68, 127, 128, 129, 200]
SHAPES = (EGONETS * 5)[:71]             # G = 71: no multiple of the 4 egonets of a workgroup, 18 workgroups (xcd_remap permutes)
PW = np.array([[25.0], [-3.0], [0.4]], dtype=np.float32)       # class 0 takes the x > 20 branch of softplus / sigmoid
_BATCH = {}


def _batch():
    if not _BATCH:
        from taxoexpan_amd.graph import BatchedDGLGraph
        g = BatchedDGLGraph.from_egonet_shapes([s[0] for s in SHAPES], [s[1] for s in SHAPES])
        graph = orc.batch_egonets(SHAPES)
        goff = graph["graph_off"].numpy()
        assert g.number_of_nodes() == graph["num_nodes"] == goff[-1] and np.array_equal(g.ndata["pos"].numpy(), graph["pos"].numpy())
        _BATCH.update(csr=g.csr(_dev()), pos=g.ndata["pos"].to(_dev()), graph=graph, goff=goff, N=int(goff[-1]), G=len(SHAPES),
                      gid=np.repeat(np.arange(len(SHAPES)), np.diff(goff)))
    return _BATCH


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
def _gate(op, items):
    """items: (what, device, float64, fp32 yardstick) -- all gated, the whole case's figures printed, then one assertion"""
    errors, report = [], []
    for what, got, ref64, yard in items:
        gate_against_f64(got.detach().cpu().numpy() if torch.is_tensor(got) else got, ref64, yard, what, errors, report=report)
    for what, e_dev, e_yard in report:
        print(f"[gate] {op} {what} {e_dev:.3e} {e_yard:.3e}")
    assert not errors, (op, errors, report)


def _oracle(fn, dtype, arrays, w):
    """fn(*tensors) in `dtype` on the CPU with (out * w).sum().backward(): (out, [gradient of every array])"""
    ts = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in arrays]
    out = fn(*ts)
    (out * torch.from_numpy(w).to(dtype)).sum().backward()
    return out.detach().numpy(), [t.grad.numpy() for t in ts]


def _both(fn, arrays, w):
    return _oracle(fn, torch.float64, arrays, w), _oracle(fn, torch.float32, arrays, w)


def _profiled(fn):
    """fn() with the library profiler on: (fn's result, the names of the launches it recorded)"""
    from taxoexpan_amd import _lib
    lib = _lib.load()
    lib.txe_profile_reset()
    lib.txe_profile_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(64)
        ms, work, kind = ctypes.c_float(), ctypes.c_double(), ctypes.c_int()
        names = []
        for i in range(lib.txe_profile_count()):
            assert lib.txe_profile_get(i, buf, 64, ctypes.byref(ms), ctypes.byref(work), ctypes.byref(kind)) == 0
            names.append(buf.value.decode())
    finally:
        lib.txe_profile_enable(0)
        lib.txe_profile_reset()
    return out, names


def _laid_out(a, layout):
    """the array on the device as a leaf that wants a gradient: 'plain' contiguous; 'pad<k>' a column view of a buffer with k more
    columns; 'offset1' a view that starts one float into its buffer.  Everything of the buffer outside the view is NaN."""
    n, d = a.shape
    src = torch.from_numpy(a).to(_dev())
    if layout == "plain":
        t = src
    elif layout.startswith("pad"):
        base = torch.full((n, d + int(layout[3:])), float("nan"), device=_dev())
        base[:, :d] = src
        t = base[:, :d]
        assert t.stride() == (d + int(layout[3:]), 1)
    else:
        assert layout == "offset1"
        buf = torch.full((n * d + 1,), float("nan"), device=_dev())
        t = buf[1:].view(n, d)
        t.copy_(src)
        assert t.data_ptr() % 16 == 4 and t.stride() == (d, 1)
    return t.requires_grad_(True)


# ---- 1. MeanReadout / WeightedMeanReadout ---------------------------------------------------------------------------------------------
# (D, layout, the VEC the host must pick): every <VEC,NI> instance, the second pass of the t0 loop (D / VEC > 512: 2052, 1030, 515, and
# 600 once its layout forces VEC 1), row strides that keep or break the vector width, a base pointer aligned to 4 bytes only
RO_CASES = [(500, "plain", 4), (600, "plain", 4), (1100, "plain", 4), (2052, "plain", 4),
            (6, "plain", 2), (258, "plain", 2), (1030, "plain", 2),
            (33, "plain", 1), (129, "plain", 1), (257, "plain", 1), (515, "plain", 1),
            (600, "pad4", 4), (600, "pad1", 1), (600, "offset1", 1), (500, "pad4", 4), (500, "pad1", 1), (500, "offset1", 1)]


def _ni(D, vec):
    return 2 if D // vec <= 128 else (4 if D // vec <= 256 else 8)


def test_readout_cases_reach_all_nine_instances():
    """the table above names every readout_{fwd,bwd}_kernel<VEC,NI> instance (each case asserts that ITS instance ran)"""
    assert {(v, _ni(D, v)) for D, _lay, v in RO_CASES} == {(v, i) for v in (4, 2, 1) for i in (2, 4, 8)}
    assert {(D, v) for D, _lay, v in RO_CASES if D // v > 64 * 8} >= {(2052, 4), (1030, 2), (515, 1)}       # second t0 pass, each VEC


@pytest.mark.parametrize("weighted", [True, False], ids=["wmr", "mr"])
@pytest.mark.parametrize("D,layout,vec", RO_CASES, ids=[f"D{D}-{lay}" for D, lay, _v in RO_CASES])
def test_mean_readouts_against_float64(D, layout, vec, weighted):
    from taxoexpan_amd import ops
    b = _batch()
    rs = np.random.RandomState(1000 + D)
    h = rs.standard_normal((b["N"], D)).astype(np.float32)
    w = rs.standard_normal((b["G"], D)).astype(np.float32)
    goff, pos = b["graph"]["graph_off"], b["graph"]["pos"]
    if weighted:
        (hg64, (dh64, dpw64)), (hg32, (dh32, dpw32)) = _both(lambda h_, pw_: orc.weighted_mean_readout(goff, h_, pos, pw_), [h, PW], w)
    else:
        (hg64, (dh64,)), (hg32, (dh32,)) = _both(lambda h_: orc.mean_readout(goff, h_), [h], w)
    hd = _laid_out(h, layout)
    pwd = torch.from_numpy(PW).to(_dev()).requires_grad_(True) if weighted else None

    def run():
        out = ops.ReadoutFunction.apply(b["csr"], hd, b["pos"], pwd)
        (out * torch.from_numpy(w).to(_dev())).sum().backward()
        return out
    out, names = _profiled(run)
    ni = _ni(D, vec)
    for kn in ("readout_fwd_kernel", "readout_bwd_kernel"):        # the intended instance ran, and no other
        assert [n for n in names if n.startswith(kn)] == [f"{kn}<{vec}, {ni}>"], (names, vec, ni)
    hg, dh = out.detach().cpu().numpy(), hd.grad.cpu().numpy()
    assert np.isfinite(hg).all() and np.isfinite(dh).all()         # (nothing of the NaN padding around a strided / offset h got in)
    items = [("hg", hg, hg64, hg32), ("d_h", dh, dh64, dh32)]
    if weighted:
        items.append(("d_pw", pwd.grad, dpw64, dpw32))
    else:                                                          # every node of an egonet receives the same row, bit for bit
        first = b["goff"][:-1][b["gid"]]
        assert np.array_equal(dh, dh[first])
    _gate("WeightedMeanReadout" if weighted else "MeanReadout", items)


# ---- 2. SumReadout / MaxReadout / ConcatReadout --------------------------------------------------------------------------------------
MULTI = {1: ("SumReadout", lambda b: (lambda h_: orc.sum_readout(b["graph"]["graph_off"], h_))),
         2: ("MaxReadout", lambda b: (lambda h_: orc.max_readout(b["graph"]["graph_off"], h_))),
         3: ("ConcatReadout", lambda b: (lambda h_: orc.concat_readout(b["graph"]["graph_off"], h_, b["graph"]["pos"])))}


@pytest.mark.parametrize("mode", [1, 2, 3], ids=["sum", "max", "concat"])
@pytest.mark.parametrize("D,layout", [(37, "plain"), (512, "plain"), (513, "plain"), (1100, "plain"), (513, "pad3")])
def test_multi_readouts_against_float64(D, layout, mode):
    """D > 512: the second pass of the d0 loop (513: one live column in it); 'pad3': ld_h = D + 3"""
    from taxoexpan_amd import ops
    b = _batch()
    rs = np.random.RandomState(2000 + D + mode)
    h = rs.standard_normal((b["N"], D)).astype(np.float32)
    w = rs.standard_normal((b["G"], 3 * D if mode == 3 else D)).astype(np.float32)
    name, fn = MULTI[mode]
    (hg64, (dh64,)), (hg32, (dh32,)) = _both(fn(b), [h], w)
    hd = _laid_out(h, layout)
    out = ops.ReadoutMultiFunction.apply(b["csr"], hd, b["pos"], mode)
    (out * torch.from_numpy(w).to(_dev())).sum().backward()
    hg, dh = out.detach().cpu().numpy(), hd.grad.cpu().numpy()
    assert np.isfinite(hg).all() and np.isfinite(dh).all()
    if mode == 2:
        assert np.array_equal(hg.astype(np.float64), hg64)         # a maximum is exact
    _gate(name, [("hg", hg, hg64, hg32), ("d_h", dh, dh64, dh32)])


def _first_maximiser(seg):
    """per column of one egonet's rows: the first NaN if there is one, else the first largest entry"""
    isn = np.isnan(seg)
    return np.where(isn.any(0), isn.argmax(0), np.where(isn, -np.inf, seg).argmax(0))


def _max_backward_expected(h, w, goff):
    want = np.zeros_like(h)
    cols = np.arange(h.shape[1])
    for g in range(len(goff) - 1):
        am = _first_maximiser(h[goff[g]:goff[g + 1]])
        want[goff[g] + am, cols] = w[g]
    return want


@pytest.mark.parametrize("D", [37, 513])
def test_max_readout_ties_go_to_the_first_maximiser(D):
    """values from a grid of a few numbers with rows duplicated inside every egonet and all-negative columns: the forward value is the
    float64 maximum exactly; exactly one node per (egonet, column) -- the FIRST maximiser -- receives d_hg[g][d], all others exactly 0"""
    from taxoexpan_amd import ops
    b = _batch()
    rs = np.random.RandomState(31 + D)
    h = (np.round(rs.standard_normal((b["N"], D)) * 2.0) / 2.0).astype(np.float32)
    h[:, ::3] = -1.0 - np.abs(h[:, ::3])                           # all-negative columns (the running maximum must not start at 0)
    goff = b["goff"]
    for g in range(b["G"]):
        beg, n = goff[g], goff[g + 1] - goff[g]
        if n >= 4:
            h[beg + n - 1] = h[beg]                                # the first row again at the end of the egonet
            h[beg + n // 2] = h[beg + 1]
    w = (rs.standard_normal((b["G"], D)).astype(np.float32) + 3.0)  # (no zero: a stray copy of the gradient would show)
    hd = torch.from_numpy(h).to(_dev()).requires_grad_(True)
    out = ops.ReadoutMultiFunction.apply(b["csr"], hd, b["pos"], 2)
    (out * torch.from_numpy(w).to(_dev())).sum().backward()
    hg64 = orc.max_readout(b["graph"]["graph_off"], torch.from_numpy(h).double()).numpy()
    assert np.array_equal(out.detach().cpu().numpy().astype(np.float64), hg64)
    dh = hd.grad.cpu().numpy()
    ties = sum(int(((h[goff[g]:goff[g + 1]] == hg64[g]).sum(0) > 1).sum()) for g in range(b["G"]))
    assert ties > b["G"] * D // 2                                  # (the input does tie in most columns)
    assert np.array_equal(dh, _max_backward_expected(h, w, goff))
    assert ((dh != 0).reshape(b["N"], D).sum() == b["G"] * D)


@pytest.mark.parametrize("readout", ["mean", "wmean", "sum", "max", "concat"])
def test_readouts_propagate_nan_like_the_oracle(readout):
    """one NaN in h inside a 128-node egonet (second 64-node chunk): column d of that egonet's hg is NaN exactly where the oracle's is --
    the reference's weighted sums multiply by 0 / 1 weights, so ConcatReadout turns all three parts of the column NaN; torch.max
    propagates NaN, so MaxReadout does; everything else stays within the gate.  MaxReadout's argmax is the FIRST NaN of a column and its
    backward sends the gradient there (a second column with two NaNs)."""
    from taxoexpan_amd import ops
    b = _batch()
    D, g_nan = 37, 12
    goff = b["goff"]
    assert goff[g_nan + 1] - goff[g_nan] == 128
    rs = np.random.RandomState(77)
    h = rs.standard_normal((b["N"], D)).astype(np.float32)
    h[goff[g_nan] + 70, 5] = np.nan
    if readout == "max":
        h[goff[g_nan] + 90, 9] = np.nan
        h[goff[g_nan] + 10, 9] = np.nan
    w = (rs.standard_normal((b["G"], 3 * D if readout == "concat" else D)).astype(np.float32) + 3.0)
    tg, pos = b["graph"]["graph_off"], b["graph"]["pos"]
    fn = {"mean": lambda h_: orc.mean_readout(tg, h_), "wmean": lambda h_: orc.weighted_mean_readout(tg, h_, pos, torch.from_numpy(PW).to(h_.dtype)),
          "sum": lambda h_: orc.sum_readout(tg, h_), "max": lambda h_: orc.max_readout(tg, h_), "concat": lambda h_: orc.concat_readout(tg, h_, pos)}[readout]
    with torch.no_grad():
        hg64, hg32 = fn(torch.from_numpy(h).double()).numpy(), fn(torch.from_numpy(h)).numpy()
    hd = torch.from_numpy(h).to(_dev()).requires_grad_(True)
    if readout in ("mean", "wmean"):
        out = ops.ReadoutFunction.apply(b["csr"], hd, b["pos"], torch.from_numpy(PW).to(_dev()) if readout == "wmean" else None)
    else:
        out = ops.ReadoutMultiFunction.apply(b["csr"], hd, b["pos"], {"sum": 1, "max": 2, "concat": 3}[readout])
    hg = out.detach().cpu().numpy()
    n_nan = {"concat": 3, "max": 2}.get(readout, 1)
    assert int(np.isnan(hg64).sum()) == n_nan and not np.isnan(np.delete(hg64, g_nan, 0)).any()    # (what the oracle does)
    assert np.array_equal(np.isnan(hg), np.isnan(hg64)), (np.argwhere(np.isnan(hg)).tolist(), np.argwhere(np.isnan(hg64)).tolist())
    assert np.array_equal(np.isinf(hg), np.isinf(hg64))
    _gate(f"{readout}+NaN", [("hg (finite part)", np.nan_to_num(hg, nan=0.0), np.nan_to_num(hg64, nan=0.0), np.nan_to_num(hg32, nan=0.0))])
    if readout == "max":
        (out * torch.from_numpy(w).to(_dev())).sum().backward()
        assert np.array_equal(hd.grad.cpu().numpy(), _max_backward_expected(h, w, goff))


# ---- 3. the bilinear matcher's training forms -----------------------------------------------------------------------------------------
def _raw_scores_in_range(e1, e2, W):
    """an input condition of the case (not of the kernel): exp of the raw score stays finite and well conditioned in fp32"""
    raw = np.einsum("il,lr,ir->i", e1.astype(np.float64), W[0].astype(np.float64), e2.astype(np.float64))
    assert np.abs(raw).max() <= 20.0, np.abs(raw).max()


@pytest.mark.parametrize("query_grad", [True, False], ids=["pair", "query_side"])
@pytest.mark.parametrize("apply_exp", [False, True], ids=["bim", "lbm"])
@pytest.mark.parametrize("G,l,r", [(1, 5, 3), (37, 50, 23), (259, 1500, 250), (130, 513, 65)])
def test_bilinear_pair_against_float64(G, l, r, apply_exp, query_grad):
    """query_grad False: the query-side form (V = e2 W^T, elementwise d_e1) that training takes"""
    from taxoexpan_amd import ops
    rs = np.random.RandomState(3000 + G)
    e1 = (rs.standard_normal((G, l)) * 0.3).astype(np.float32)
    e2 = (rs.standard_normal((G, r)) * 0.3).astype(np.float32)
    W = (rs.standard_normal((1, l, r)) * (0.2 if l * r <= 50 * 23 else 0.05)).astype(np.float32)
    up = rs.standard_normal((G, 1)).astype(np.float32)
    _raw_scores_in_range(e1, e2, W)
    (s64, g64), (s32, g32) = _both(lambda a, b_, c: orc.bilinear_match(a, b_, c, apply_exp), [e1, e2, W], up)
    a, b_, c = (torch.from_numpy(t).to(_dev()).requires_grad_(True) for t in (e1, e2, W))
    b_.requires_grad_(query_grad)
    s = ops.BilinearPairFunction.apply(a, b_, c, apply_exp)
    (s * torch.from_numpy(up).to(_dev())).sum().backward()
    assert tuple(s.shape) == (G, 1) and (query_grad or b_.grad is None)
    items = [("scores", s, s64, s32), ("d_e1", a.grad, g64[0], g32[0]), ("dW", c.grad, g64[2], g32[2])]
    if query_grad:
        items.append(("d_e2", b_.grad, g64[1], g32[1]))
    _gate("BilinearPairFunction" + ("" if query_grad else "[query side]"), items)


RUN_LENS = [1, 33, 2, 16, 17, 300]          # a run of one, 16 / 17 on both sides of RB_NL, a long run


@pytest.mark.parametrize("form", ["runs", "stacked"])
@pytest.mark.parametrize("apply_exp", [False, True], ids=["bim", "lbm"])
@pytest.mark.parametrize("l", [512, 513, 1500])
def test_bilinear_run_forms_against_float64(l, apply_exp, form):
    """l = 512: one pass of rowdot_runs_kernel; 513: two, the second with one live column; 1500: three (partial sums parked in s, exp on
    the last pass only) and six column tiles of runs_bwd_kernel.  'runs': RepeatedRows.from_ids, runs known on the host; 'stacked': found
    on the device in the stacked matrix."""
    from taxoexpan_amd import ops
    r = 250
    rs = np.random.RandomState(4000 + l)
    ids = np.repeat(np.arange(len(RUN_LENS)), RUN_LENS)
    G = len(ids)
    table = (rs.standard_normal((len(RUN_LENS), r)) * 0.3).astype(np.float32)
    e1 = (rs.standard_normal((G, l)) * 0.3).astype(np.float32)
    W = (rs.standard_normal((1, l, r)) * 0.05).astype(np.float32)
    up = rs.standard_normal((G, 1)).astype(np.float32)
    e2 = table[ids]
    _raw_scores_in_range(e1, e2, W)
    (s64, g64), (s32, g32) = _both(lambda a, c: orc.bilinear_match(a, torch.from_numpy(e2).to(a.dtype), c, apply_exp), [e1, W], up)
    a, c = (torch.from_numpy(t).to(_dev()).requires_grad_(True) for t in (e1, W))
    if form == "runs":
        rr = ops.RepeatedRows.from_ids(torch.from_numpy(table).to(_dev()), ids)
        assert rr.rows.shape[0] == len(RUN_LENS) and np.diff(rr.run_off.cpu().numpy()).tolist() == RUN_LENS
        s = ops.BilinearRunsFunction.apply(a, c, apply_exp, rr.rows, rr.run_off)
    else:
        s = ops.BilinearStackedRunsFunction.apply(a, torch.from_numpy(e2).to(_dev()), c, apply_exp)
    (s * torch.from_numpy(up).to(_dev())).sum().backward()
    assert tuple(s.shape) == (G, 1)
    _gate("BilinearRunsFunction" if form == "runs" else "BilinearStackedRunsFunction",
          [("scores", s, s64, s32), ("d_e1", a.grad, g64[0], g32[0]), ("dW", c.grad, g64[1], g32[1])])


# ---- 4. LinearFunction ----------------------------------------------------------------------------------------------------------------
def _linear_inputs(G, l, r, O, bias, seed):
    rs = np.random.RandomState(seed)
    x1 = (rs.standard_normal((G, l)) * 0.5).astype(np.float32)
    x2 = (rs.standard_normal((G, r)) * 0.5).astype(np.float32) if r else None
    W = (rs.standard_normal((O, l + r)) / np.sqrt(l + r)).astype(np.float32)
    b = (rs.standard_normal((O,)) * 0.1).astype(np.float32) if bias else None
    w = rs.standard_normal((G, O)).astype(np.float32)
    return x1, x2, W, b, w


def _audit_branches(taken, pre64, what):
    """txe_oracle.BRANCH_AUDIT's rule (tests/test_gpu_routes.py): given relu branches may differ from the float64 pre-activation's own
    sign only where it is within rounding of 0 (1e-4 of the largest), on at most 1e-3 numel + 1 entries"""
    dis = (pre64 > 0) != taken
    worst = float(np.abs(pre64[dis]).max()) if dis.any() else 0.0
    assert worst <= 1e-4 * float(np.abs(pre64).max()) and int(dis.sum()) <= 1e-3 * pre64.size + 1, (what, int(dis.sum()), worst)


def _linear_reference(dtype, x1, x2, W, b, act, w, taken):
    """(y, pre-activation, {name: gradient}) of act([x1 | x2] W^T + b) in `dtype`; relu's GRADIENT runs through the given branches
    (taken, bool [G][O]) so that both sides differentiate the same piecewise-linear function, its forward value is the plain relu"""
    t = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in (("x1", x1), ("x2", x2), ("W", W), ("b", b)) if v is not None}
    pre = F.linear(torch.cat((t["x1"], t["x2"]), 1) if x2 is not None else t["x1"], t["W"], t.get("b"))
    if act == 1:
        y, yb = F.relu(pre), torch.where(torch.from_numpy(taken), pre, torch.zeros_like(pre))
    else:
        y = yb = torch.tanh(pre) if act == 2 else pre
    (yb * torch.from_numpy(w).to(dtype)).sum().backward()
    return y.detach().numpy(), pre.detach().numpy(), {k: v.grad.numpy() for k, v in t.items()}


def _linear_case(G, l, r, O, act, bias, seed, variant="plain"):
    from taxoexpan_amd import ops
    x1, x2, W, b, w = _linear_inputs(G, l, r, O, bias, seed)
    dev = _dev()
    x1d = _laid_out(x1, "pad3" if variant == "strided" else "plain")
    x2d = torch.from_numpy(x2).to(dev).requires_grad_(True) if x2 is not None else None
    Wd = torch.from_numpy(W).to(dev).requires_grad_(True)
    bd = torch.from_numpy(b).to(dev).requires_grad_(True) if bias else None
    if variant in ("x2_no_grad", "no_input_grad"):                 # dx2 == NULL with x2 present: dx1 alone, a product with N = l
        x2d.requires_grad_(False)
    if variant == "no_input_grad":
        x1d.requires_grad_(False)
    y = ops.LinearFunction.apply(x1d, x2d, Wd, bd, act)
    (y * torch.from_numpy(w).to(dev)).sum().backward()
    assert tuple(y.shape) == (G, O)
    yh = y.detach().cpu().numpy()
    taken = yh > 0
    y64, pre64, g64 = _linear_reference(torch.float64, x1, x2, W, b, act, w, taken)
    y32, pre32, g32 = _linear_reference(torch.float32, x1, x2, W, b, act, w, taken)
    if act == 1:
        _audit_branches(pre32 > 0, pre64, "fp32 oracle")           # the condition on the seeded inputs, with the fp32 oracle as the device
        _audit_branches(taken, pre64, "device")
    got = {"x1": x1d.grad, "x2": x2d.grad if x2d is not None else None, "W": Wd.grad, "b": bd.grad if bias else None}
    want = {"W"} | ({"b"} if bias else set()) | ({"x1"} if variant != "no_input_grad" else set()) | \
        ({"x2"} if (r and variant in ("plain", "strided")) else set())
    assert {k for k, v in got.items() if v is not None} == want
    assert all(bool(torch.isfinite(got[k]).all()) for k in want)
    _gate(f"LinearFunction[act {act}]", [("y", yh, y64, y32)] + [(f"d_{k}", got[k], g64[k], g32[k]) for k in sorted(want)])


@pytest.mark.parametrize("G,l,r,O,act,bias", [
    (1, 5, 0, 1, 0, False),             # the smallest case
    (517, 37, 23, 66, 1, True),         # the concat seam off every alignment
    (300, 1500, 250, 500, 1, True),     # MAG ConcatReadout + MLP matcher, first layer
    (300, 500, 0, 1, 0, True),          # its second layer
    (130, 24, 12, 16, 2, False),        # tanh
])
def test_linear_against_float64(G, l, r, O, act, bias):
    _linear_case(G, l, r, O, act, bias, seed=5000 + G + l)


# The first-layer widths with a batch at which the weight gradient dW [O][l + r] = dz^T [x1 | x2] runs split-K:
# choose_splits(M = O = 500, N = l + r = 1750, K = G) of txe_gemm.h on the 256 compute units (512 workgroup slots) of the MI355X.  N = 1750
# would take 160-wide tiles only from 2 M N K >= 2e10 (G >= 11,429); below that the 64-wide tiles win: 4 x 28 = 112 tiles, and with
# G = 1100 (35 k-tiles, at most ceil(1100 / 256) = 5 slices) S = 4 -- 448 workgroups in one round of 9 k-tiles each -- costs
# 11 x 0.55 + 0.28 = 6.3 against 20.4 for S = 1 and 10.3 for S = 5 (two rounds).  G = 1100: no multiple of the 128-row tile or of S x 32.
SPLIT_G, SPLIT_S = 1100, 4


def test_linear_split_k_weight_gradient_against_float64():
    from taxoexpan_amd import _lib
    l, r, O = 1500, 250, 500
    al = lambda n: (n + 255) // 256 * 256
    wsb = _lib.call("txe_linear_bwd_ws_bytes", SPLIT_G, l, r, O)
    assert wsb == al(SPLIT_G * O * 4) + al(SPLIT_S * O * (l + r) * 4), wsb         # the library does split this product, S = 4 ways
    _linear_case(SPLIT_G, l, r, O, 1, True, seed=5999)


@pytest.mark.parametrize("variant", ["strided", "x2_no_grad", "no_input_grad"])
def test_linear_variants_against_float64(variant):
    """at the 517 shape: x1 a column view with ld1 = l + 3 (NaN in the padding); no gradient wanted for x2 (dx2 == NULL, the input
    gradient's product has N = l); no gradient wanted for either input"""
    _linear_case(517, 37, 23, 66, 1, True, seed=5000 + 517 + 37, variant=variant)


@pytest.mark.parametrize("r", [23, 0])
def test_linear_on_an_empty_batch(r):
    """G = 0: outputs of the right shapes, dW and db exactly zero"""
    from taxoexpan_amd import ops
    dev, l, O = _dev(), 37, 66
    x1 = torch.zeros((0, l), device=dev, requires_grad=True)
    x2 = torch.zeros((0, r), device=dev, requires_grad=True) if r else None
    W = torch.randn((O, l + r), device=dev, requires_grad=True)
    b = torch.randn((O,), device=dev, requires_grad=True)
    y = ops.LinearFunction.apply(x1, x2, W, b, 1)
    assert tuple(y.shape) == (0, O)
    y.sum().backward()
    assert tuple(x1.grad.shape) == (0, l) and (x2 is None or tuple(x2.grad.shape) == (0, r))
    assert tuple(W.grad.shape) == (O, l + r) and tuple(b.grad.shape) == (O,)
    assert not W.grad.any() and not b.grad.any()
