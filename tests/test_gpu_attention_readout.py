"""The attention readout on the MI355X: ops.ReadoutAttnFunction (txe_readout_attn_fwd / _bwd, csrc/txe_readout.hip) operator by
operator against tests/attention_readout_ref.py in FLOAT64, then model_zoo.AttentionReadout inside TaxoExpan("...", "AR", "...") against
a float64 composite of the oracle's propagation, that reference and the oracle's matcher and loss, then the evaluation, inference,
training and checkpoint flows on tests/golden/toy_taxo.

Reference: the defining expression in torch float64 on the CPU; yardstick: the same expression in fp32 on the CPU; gate:
golden_util.gate_against_f64 with its defaults (2 x the yardstick's own error, floor 2e-5 and cap 1e-4 of the tensor's largest entry)
for hg, alpha and every gradient.  Every gate prints "[gate] operator what device-error yardstick-error" (fractions of the tensor's
largest float64 entry).

The batch is the one of tests/test_gpu_readout_match_ops.py (node counts 1..5, 63..68, 127..129, 200; G = 71).  The kernels keep the
scores of an egonet's first two 64-node chunks in LDS and score later chunks again (129 and 200 nodes take that path); one pass of
their column loop covers 64 * NI * VEC floats with NI = 2 (up to 128 vectors per row) or 8, so D = 2052 (VEC 4), 1030 (VEC 2) and 600
behind a row stride of 603 (VEC 1) each take a second pass, which reads alpha back instead of forming it again.

Measured on the MI355X, largest device error / yardstick error per tensor over the operator cases of this file (and the largest device
error itself; the floor is 2e-5, so every figure is under it):
    hg      1.3  (D 37, A 65; largest device error 2.4e-6, the u x 50 case, where the yardstick is at 2.3e-6)
    alpha   1.5  (D 37, A 65; largest 2.3e-6, the u x 50 case)
    d_h     1.02 (largest 9.5e-7)
    d_Y     3.5  (D 600 behind a row stride of 603 / one float into its buffer: 1.1e-6 against 3.1e-7; largest 3.9e-6, the u x 50 case)
    d_P     1.7  (saturated rows; largest 1.8e-6)
    d_u     1.6  (the u x 50 case, which is also the largest: 4.0e-6)
Models: PGAT + AR + BIM at most 2.1 (grad readout.gate_hidden.weight, 2.7e-7); PGCN + AR + MLP at most 13.9 (grad
readout.gate_hidden.bias, 2.6e-6 of the model's gradient scale against the fp32 composite's 1.9e-7: under the floor).
The 24 cases take 8 s on the MI355X, most of it the CPU references.
"""
import ctypes
import os
import shutil
import types

import numpy as np
import pytest
import torch

import attention_readout_ref as ref
import txe_oracle as orc
from golden_util import GOLDEN_DIR, gate_against_f64, gradient_scale_floor, load_case

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


# ---- the batch (copied from tests/test_gpu_readout_match_ops.py) ----------------------------------------------------------------------
EGONETS = [(0, 0), (0, 1), (2, 0), (1, 2), (2, 2), (20, 42), (3, 60), (0, 64), (30, 35), (66, 0), (7, 60), (40, 86), (64, 63), (1, 127),
           (99, 100)]
assert [k + 1 + m for k, m in EGONETS] == [1, 2, 3, 4, 5, 63, 64, 65, 66, 67, 68, 127, 128, 129, 200]
SHAPES = (EGONETS * 5)[:71]             # G = 71: no multiple of the 4 egonets of a workgroup, 18 workgroups (xcd_remap permutes)
_BATCH = {}


def _graph_of(shapes):
    from taxoexpan_amd.graph import BatchedDGLGraph
    return BatchedDGLGraph.from_egonet_shapes([s[0] for s in shapes], [s[1] for s in shapes])


def _batch():
    if not _BATCH:
        g = _graph_of(SHAPES)
        graph = orc.batch_egonets(SHAPES)
        goff = graph["graph_off"].numpy()
        assert g.number_of_nodes() == graph["num_nodes"] == goff[-1] and np.array_equal(g.ndata["pos"].numpy(), graph["pos"].numpy())
        _BATCH.update(csr=g.csr(_dev()), pos=g.ndata["pos"].to(_dev()), graph=graph, goff=goff, N=int(goff[-1]), G=len(SHAPES))
    return _BATCH


# ---- helpers --------------------------------------------------------------------------------------------------------------------------
def _gate(op, items, scale_floor=0.0):
    """items: (what, device, float64, fp32 yardstick) -- all gated, the whole case's figures printed, then one assertion"""
    errors, report = [], []
    for what, got, ref64, yard in items:
        gate_against_f64(got.detach().cpu().numpy() if torch.is_tensor(got) else got, ref64, yard, what, errors, report=report,
                         scale_floor=scale_floor)
    for what, e_dev, e_yard in report:
        print(f"[gate] {op} {what} {e_dev:.3e} {e_yard:.3e}")
    assert not errors, (op, errors, report)


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


def _draw(D, A, seed, u_scale=1.0, N=None):
    rs = np.random.RandomState(seed)
    N = _batch()["N"] if N is None else N
    h = rs.standard_normal((N, D)).astype(np.float32)
    Y = rs.standard_normal((N, A)).astype(np.float32)
    P = rs.standard_normal((3, A)).astype(np.float32)
    u = (rs.standard_normal((1, A)) * u_scale).astype(np.float32)
    return h, Y, P, u


def _references(goff_t, pos_t, arrays, w):
    """((hg, alpha), gradients) of the reference in float64 and in fp32; backward of <hg, w>"""
    fn = lambda h, Y, P, u: ref.attention_pool(goff_t, h, Y, pos_t, P, u)
    return ref.run(fn, torch.float64, arrays, [w, None]), ref.run(fn, torch.float32, arrays, [w, None])


def _device_run(csr, pos, hd, Yd, P, u, w):
    """forward and backward of <hg, w> on the device with the profiler on: (hg, alpha, Pd, ud, launch names)"""
    from taxoexpan_amd import ops
    Pd, ud = (torch.from_numpy(t).to(_dev()).requires_grad_(True) for t in (P, u))

    def run():
        hg, alpha = ops.ReadoutAttnFunction.apply(csr, hd, Yd, pos, Pd, ud)
        (hg * torch.from_numpy(w).to(_dev())).sum().backward()
        return hg, alpha
    (hg, alpha), names = _profiled(run)
    assert not alpha.requires_grad
    return hg.detach().cpu().numpy(), alpha.cpu().numpy(), Pd, ud, names


def _items(dev, r64, r32):
    """gate items of (hg, alpha, d_h, d_Y, d_P, d_u): device values, float64 reference, fp32 yardstick"""
    (o64, g64), (o32, g32) = r64, r32
    names = ["hg", "alpha", "d_h", "d_Y", "d_P", "d_u"]
    return [(n, d, a, b) for n, d, a, b in zip(names, dev, o64 + g64, o32 + g32)]


def _instance(vec, nvec):
    return f"<{vec}, {2 if nvec <= 128 else 8}>"


# ---- 1. the operator against float64 ------------------------------------------------------------------------------------------------
# (D, A, u scale, layout of h, layout of Y, the VEC the host must pick)
OP_CASES = [(600, 100, 1.0, "plain", "plain", 4),        # the MAG widths
            (8, 3, 50.0, "plain", "plain", 4),           # scores span about +-150: no max shift -> overflow; alphas underflow to exact zeros
            (37, 65, 1.0, "plain", "plain", 1),          # scalar loads, A across the 64-lane boundary
            (6, 1, 1.0, "plain", "plain", 2),
            (2052, 5, 1.0, "plain", "plain", 4),         # 513 vectors: a second pass of the column loop with one live vector
            (1030, 7, 1.0, "plain", "plain", 2),         # the same at VEC 2
            (600, 100, 1.0, "pad3", "plain", 1),         # ld_h = 603: VEC 1, 600 > 512 scalars: two passes
            (600, 100, 1.0, "offset1", "plain", 1),      # h starts 4 bytes into its buffer: only narrower loads are legal
            (600, 100, 1.0, "plain", "pad5", 4)]         # Y with a row stride larger than A


def test_operator_cases_reach_all_six_instances():
    assert {(v, D // v <= 128) for D, _A, _s, _lh, _ly, v in OP_CASES} == {(v, small) for v in (4, 2, 1) for small in (True, False)}
    assert {(D, v) for D, _A, _s, _lh, _ly, v in OP_CASES if D // v > 512} >= {(2052, 4), (1030, 2), (600, 1)}


@pytest.mark.parametrize("D,A,u_scale,h_layout,y_layout,vec", OP_CASES,
                         ids=[f"D{c[0]}-A{c[1]}-h_{c[3]}-Y_{c[4]}" for c in OP_CASES])
def test_operator_against_float64(D, A, u_scale, h_layout, y_layout, vec):
    b = _batch()
    h, Y, P, u = _draw(D, A, 7000 + D + A, u_scale)
    w = np.random.RandomState(D).standard_normal((b["G"], D)).astype(np.float32)
    r64, r32 = _references(b["graph"]["graph_off"], b["graph"]["pos"], [h, Y, P, u], w)
    hd, Yd = _laid_out(h, h_layout), _laid_out(Y, y_layout)
    hg, alpha, Pd, ud, names = _device_run(b["csr"], b["pos"], hd, Yd, P, u, w)
    inst = _instance(vec, D // vec)
    assert names == ["readout_attn_fwd_kernel" + inst, "readout_attn_bwd_kernel" + inst, "readout_attn_reduce_kernel"], names
    dev = [hg, alpha, hd.grad.cpu().numpy(), Yd.grad.cpu().numpy(), Pd.grad.cpu().numpy(), ud.grad.cpu().numpy()]
    assert all(np.isfinite(t).all() for t in dev)                  # (nothing of the NaN padding around a strided / offset view got in)
    if u_scale > 1.0:
        s = np.tanh(Y.astype(np.float64) + P.astype(np.float64)[b["graph"]["pos"].numpy()]) @ u.astype(np.float64).reshape(-1)
        assert s.max() > 100 and s.min() < -100                    # exp(s) alone overflows fp32
        assert (alpha == 0).sum() > 0 and (r64[0][1] < 1e-45).sum() > 0     # ... and some weights underflow to exact zeros
    sums = np.add.reduceat(alpha.astype(np.float64), b["goff"][:-1])
    assert np.abs(sums - 1.0).max() <= 1e-5
    _gate("ReadoutAttnFunction", _items(dev, r64, r32))


def test_saturated_gate_rows_have_exactly_zero_gradient():
    """rows of Y at +-30: t = +-1 in fp32 and float64 alike, so d_Y of those rows is exactly zero"""
    b = _batch()
    D, A = 37, 65
    h, Y, P, u = _draw(D, A, 7100)
    rows = np.arange(0, b["N"], 7)
    Y[rows] = np.where(np.arange(len(rows))[:, None] % 2 == 0, 30.0, -30.0).astype(np.float32)
    w = np.random.RandomState(1).standard_normal((b["G"], D)).astype(np.float32)
    r64, r32 = _references(b["graph"]["graph_off"], b["graph"]["pos"], [h, Y, P, u], w)
    hd, Yd = _laid_out(h, "plain"), _laid_out(Y, "plain")
    hg, alpha, Pd, ud, _names = _device_run(b["csr"], b["pos"], hd, Yd, P, u, w)
    dY = Yd.grad.cpu().numpy()
    assert not dY[rows].any() and not r64[1][1][rows].any() and np.abs(dY).max() > 0
    _gate("ReadoutAttnFunction[saturated]", _items([hg, alpha, hd.grad.cpu().numpy(), dY, Pd.grad.cpu().numpy(), ud.grad.cpu().numpy()], r64, r32))


@pytest.mark.parametrize("where", ["h", "Y"])
def test_non_finite_inputs_propagate_like_the_reference(where):
    """one NaN in h (second 64-node chunk of a 128-node egonet): only that column of that egonet's hg; one NaN in Y: that egonet's
    alpha and its whole hg row.  Every other egonet stays finite and within the gate."""
    from taxoexpan_amd import ops
    b = _batch()
    D, A, g_nan = 37, 65, 12
    goff = b["goff"]
    assert goff[g_nan + 1] - goff[g_nan] == 128
    h, Y, P, u = _draw(D, A, 7200)
    (h if where == "h" else Y)[goff[g_nan] + 70, 5] = np.nan
    with torch.no_grad():
        want = {dt: ref.attention_pool(b["graph"]["graph_off"], torch.from_numpy(h).to(dt), torch.from_numpy(Y).to(dt), b["graph"]["pos"],
                                       torch.from_numpy(P).to(dt), torch.from_numpy(u).to(dt)) for dt in (torch.float64, torch.float32)}
    hg64, al64 = (t.numpy() for t in want[torch.float64])
    hg32, al32 = (t.numpy() for t in want[torch.float32])
    hg, alpha = ops.ReadoutAttnFunction.apply(b["csr"], torch.from_numpy(h).to(_dev()), torch.from_numpy(Y).to(_dev()), b["pos"],
                                              torch.from_numpy(P).to(_dev()), torch.from_numpy(u).to(_dev()))
    hg, alpha = hg.cpu().numpy(), alpha.cpu().numpy()
    if where == "h":                                                    # (what the reference does)
        assert np.argwhere(np.isnan(hg64)).tolist() == [[g_nan, 5]] and not np.isnan(al64).any()
    else:
        assert np.isnan(hg64[g_nan]).all() and np.isnan(al64[goff[g_nan]:goff[g_nan + 1]]).all()
        assert int(np.isnan(hg64).sum()) == D and int(np.isnan(al64).sum()) == 128
    assert np.array_equal(np.isnan(hg), np.isnan(hg64)) and np.array_equal(np.isnan(alpha), np.isnan(al64))
    assert not np.isinf(hg).any() and not np.isinf(alpha).any()
    z = lambda t: np.nan_to_num(t, nan=0.0)
    _gate(f"ReadoutAttnFunction[NaN in {where}]", [("hg (finite part)", z(hg), z(hg64), z(hg32)), ("alpha (finite part)", z(alpha), z(al64), z(al32))])


def test_empty_segments_give_zero_rows_and_zero_contributions():
    """graph offsets with segments that hold no node -- first, in the middle, last -- beside segments of one and of 70 nodes"""
    goff = np.array([0, 0, 4, 4, 5, 75, 75], dtype=np.int32)
    N, D, A = 75, 12, 5
    h, Y, P, u = _draw(D, A, 7300, N=N)
    pos = np.random.RandomState(2).randint(0, 3, N)
    w = np.random.RandomState(3).standard_normal((6, D)).astype(np.float32)
    r64, r32 = _references(torch.from_numpy(goff.astype(np.int64)), torch.from_numpy(pos), [h, Y, P, u], w)
    csr = types.SimpleNamespace(graph_off=torch.from_numpy(goff).to(_dev()), n_graphs=6)
    hd, Yd = _laid_out(h, "plain"), _laid_out(Y, "plain")
    hg, alpha, Pd, ud, _names = _device_run(csr, torch.from_numpy(pos).to(_dev()), hd, Yd, P, u, w)
    assert not hg[[0, 2, 5]].any() and hg[[1, 3, 4]].any(1).all() and alpha[4] == 1.0
    _gate("ReadoutAttnFunction[empty segments]", _items([hg, alpha, hd.grad.cpu().numpy(), Yd.grad.cpu().numpy(), Pd.grad.cpu().numpy(),
                                                         ud.grad.cpu().numpy()], r64, r32))


def test_no_graphs_no_launch():
    from taxoexpan_amd import ops
    D, A = 8, 3
    csr = types.SimpleNamespace(graph_off=torch.zeros(1, dtype=torch.int32, device=_dev()), n_graphs=0)
    hd, Yd = (torch.zeros((0, k), device=_dev(), requires_grad=True) for k in (D, A))
    Pd, ud = torch.randn((3, A), device=_dev(), requires_grad=True), torch.randn((1, A), device=_dev(), requires_grad=True)

    def run():
        hg, alpha = ops.ReadoutAttnFunction.apply(csr, hd, Yd, torch.zeros(0, dtype=torch.int32, device=_dev()), Pd, ud)
        hg.sum().backward()
        return hg, alpha
    (hg, alpha), names = _profiled(run)
    assert names == [] and tuple(hg.shape) == (0, D) and tuple(alpha.shape) == (0,)
    assert tuple(hd.grad.shape) == (0, D) and tuple(Yd.grad.shape) == (0, A)
    assert tuple(Pd.grad.shape) == (3, A) and tuple(ud.grad.shape) == (1, A) and not Pd.grad.any() and not ud.grad.any()


def test_two_calls_are_bit_equal_and_a_sub_batch_equals_its_rows():
    b = _batch()
    D, A = 600, 100
    h, Y, P, u = _draw(D, A, 7400)
    w = np.random.RandomState(4).standard_normal((b["G"], D)).astype(np.float32)
    runs = []
    for _ in range(2):
        hd, Yd = _laid_out(h, "plain"), _laid_out(Y, "plain")
        hg, alpha, Pd, ud, _names = _device_run(b["csr"], b["pos"], hd, Yd, P, u, w)
        runs.append([hg, alpha] + [t.grad.cpu().numpy() for t in (hd, Yd, Pd, ud)])
    for x, y in zip(*runs):
        assert x.tobytes() == y.tobytes()
    # egonets 10..29 as a batch of their own: the same bits as their rows of the whole batch
    from taxoexpan_amd import ops
    lo, hi = b["goff"][10], b["goff"][30]
    sub = _graph_of(SHAPES[10:30])
    assert sub.number_of_nodes() == hi - lo
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    hg_s, alpha_s = ops.ReadoutAttnFunction.apply(sub.csr(_dev()), to(h[lo:hi]), to(Y[lo:hi]), sub.ndata["pos"].to(_dev()), to(P), to(u))
    assert hg_s.cpu().numpy().tobytes() == runs[0][0][10:30].tobytes()
    assert alpha_s.cpu().numpy().tobytes() == runs[0][1][lo:hi].tobytes()


def test_operator_refuses_host_tensors():
    from taxoexpan_amd import ops
    b = _batch()
    h, Y, P, u = (torch.from_numpy(t) for t in _draw(8, 3, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ReadoutAttnFunction.apply(b["csr"], h, Y.to(_dev()), b["pos"], P.to(_dev()), u.to(_dev()))


# ---- 2. the module inside the model ---------------------------------------------------------------------------------------------------
ATT = 6


def _readout_params(out_dim, seed):
    rs = np.random.RandomState(seed)
    return {"readout.gate_hidden.weight": (rs.standard_normal((ATT, out_dim)) / np.sqrt(out_dim)).astype(np.float32),
            "readout.gate_hidden.bias": (rs.standard_normal(ATT) * 0.1).astype(np.float32),
            "readout.gate_position.weight": rs.standard_normal((3, ATT)).astype(np.float32),
            "readout.gate_out.weight": rs.standard_normal((1, ATT)).astype(np.float32)}


def _mlp_params(spec, seed):
    rs = np.random.RandomState(seed)
    hid, wide = spec["hidden_dim"], spec["out_dim"] + spec["in_dim"]
    return {"match.ffn.0.weight": (rs.standard_normal((hid, wide)) / np.sqrt(wide)).astype(np.float32),
            "match.ffn.0.bias": (rs.standard_normal(hid) * 0.1).astype(np.float32),
            "match.ffn.2.weight": (rs.standard_normal((1, hid)) / np.sqrt(hid)).astype(np.float32),
            "match.ffn.2.bias": (rs.standard_normal(1) * 0.1).astype(np.float32)}


def _composite(dtype, spec, match, params, graph, x, q):
    """oracle propagation -> reference readout -> oracle matcher -> oracle InfoNCE in `dtype`: (scores, loss, {parameter: gradient})"""
    P = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in params.items()}
    xt, qt = torch.from_numpy(x).to(dtype), torch.from_numpy(q).to(dtype)
    if spec["prop"] == "PGAT":
        hn = orc.pgat_forward(P, graph, xt, spec["heads"], spec["num_layers"], prefix="graph_propagate.")
    else:
        hn = orc.pgcn_forward(P, graph, xt, spec["num_layers"], prefix="graph_propagate.")
    hg, _alpha = ref.attention_readout(graph["graph_off"], hn, graph["pos"], P["readout.gate_hidden.weight"], P["readout.gate_hidden.bias"],
                                       P["readout.gate_position.weight"], P["readout.gate_out.weight"])
    if match == "BIM":
        s = orc.bilinear_match(hg, qt, P["match.W.weight"], False)
    else:
        s = orc.mlp_match(hg, qt, P["match.ffn.0.weight"], P["match.ffn.0.bias"], P["match.ffn.2.weight"], P["match.ffn.2.bias"])
    loss = orc.info_nce_loss(s, spec["n_queries"])
    loss.backward()
    return s.detach().numpy(), np.asarray([float(loss.detach())]), {k: p.grad.numpy() for k, p in P.items()}


@pytest.mark.parametrize("case,prop,match", [("small_pgat_wmr_bim", "PGAT", "BIM"), ("small_pgcn_mr_bim", "PGCN", "MLP")])
def test_model_with_attention_readout_against_float64(case, prop, match):
    from taxoexpan_amd import TaxoExpan, model_zoo
    spec, _z, shapes, x, q, params, graph = load_case(case)
    assert spec["prop"] == prop
    params = {k: v for k, v in params.items() if k.startswith("graph_propagate.") or (match == "BIM" and k == "match.W.weight")}
    params.update(_readout_params(spec["out_dim"], 9000 + spec["seed"]))
    if match == "MLP":
        params.update(_mlp_params(spec, 9100 + spec["seed"]))
    model = TaxoExpan(prop, "AR", match, in_dim=spec["in_dim"], hidden_dim=spec["hidden_dim"], out_dim=spec["out_dim"],
                      pos_dim=spec["pos_dim"], num_layers=spec["num_layers"], heads=spec["heads"], feat_drop=0.1, attn_drop=0.1,
                      hidden_drop=0.1, out_drop=0.1, attention_dim=ATT)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    model = model.to(_dev()).eval()
    g = _graph_of(shapes)

    def run():
        scores = model(g, torch.from_numpy(x).to(_dev()), torch.from_numpy(q).to(_dev()))
        nq = spec["n_queries"]
        loss = torch.nn.functional.cross_entropy(scores.reshape(nq, -1), torch.zeros(nq, dtype=torch.long, device=_dev()), reduction="sum")
        loss.backward()
        return scores, loss
    (scores, loss), names = _profiled(run)
    assert sum(n.startswith("readout_attn_fwd_kernel") for n in names) == 1 and sum(n.startswith("readout_attn_bwd_kernel") for n in names) == 1
    assert isinstance(model.readout, model_zoo.AttentionReadout) and torch.is_tensor(g.ndata["a"]) and g.ndata["a"].shape == (graph["num_nodes"],)
    s64, l64, g64 = _composite(torch.float64, spec, match, params, graph, x, q)
    s32, l32, g32 = _composite(torch.float32, spec, match, params, graph, x, q)
    got = {k: p.grad for k, p in model.named_parameters()}
    assert set(got) == set(g64) and all(v is not None and bool(torch.isfinite(v).all()) for v in got.values())
    _gate(f"TaxoExpan({prop}, AR, {match})", [("scores", scores, s64, s32), ("loss", loss.detach().reshape(1), l64, l32)])
    _gate(f"TaxoExpan({prop}, AR, {match})", [("grad " + k, got[k], g64[k], g32[k]) for k in sorted(got)], scale_floor=gradient_scale_floor(g64))


def test_model_on_an_empty_batch():
    """no egonet at all: shapes flow through, gradients (where any arrive) are zeros, g.ndata['a'] is empty"""
    from taxoexpan_amd import TaxoExpan
    torch.manual_seed(3)
    model = TaxoExpan("PGAT", "AR", "BIM", in_dim=6, hidden_dim=8, out_dim=5, pos_dim=3, num_layers=1, heads=[2, 1], feat_drop=0.0,
                      attn_drop=0.0, hidden_drop=0.0, out_drop=0.0, attention_dim=4).to(_dev())
    g0 = _graph_of([])
    s0 = model(g0, torch.zeros(0, 6, device=_dev()), torch.zeros(0, 6, device=_dev()))
    assert tuple(s0.shape) == (0, 1) and tuple(g0.ndata["a"].shape) == (0,)
    if s0.requires_grad:
        s0.sum().backward()
    assert all(p.grad is None or bool(torch.all(p.grad == 0)) for p in model.parameters())


# ---- 3. the flows on the toy taxonomy ------------------------------------------------------------------------------------------------
def _toy(tmp_path, mode, **kw):
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    import random
    d = tmp_path / ("toy_" + mode)
    d.mkdir(exist_ok=True)
    for fn in os.listdir(os.path.join(GOLDEN_DIR, "toy_taxo")):
        shutil.copy(os.path.join(GOLDEN_DIR, "toy_taxo", fn), d)
    random.seed(0)
    opts = dict(mode=mode, sampling_mode=1 if mode == "train" else 0, negative_size=3, expand_factor=5, normalize_embed=True)
    opts.update(kw)
    return MaskedGraphDataset(MAGDataset("toy", str(d), raw=True), **opts)


def _toy_model(match="LBM", state=None):
    from taxoexpan_amd import TaxoExpan
    torch.manual_seed(11)
    m = TaxoExpan("PGAT", "AR", match, in_dim=8, hidden_dim=6, out_dim=5, pos_dim=3, num_layers=1, heads=[2, 1], feat_drop=0.0,
                  attn_drop=0.0, hidden_drop=0.0, out_drop=0.0, attention_dim=4).to(_dev())
    if state is not None:
        m.load_state_dict(state, strict=True)
    return m


def test_candidates_encoded_in_chunks_equal_one_batch_bit_for_bit(tmp_path):
    from taxoexpan_amd.evaluate import candidate_graphs
    from taxoexpan_amd.scoring import encode_candidates
    ds = _toy(tmp_path, "test", expand_factor=3)
    model = _toy_model().eval()
    cand = sorted(ds.all_positions)
    dtax = ds.device_taxonomy(_dev())
    one = encode_candidates(model, candidate_graphs(dtax, cand, ds.expand_factor, 3))
    chunks = candidate_graphs(dtax, cand, ds.expand_factor, 3, batch_size=17)
    assert isinstance(chunks, list) and len(chunks) == -(-len(cand) // 17) > 2
    many = encode_candidates(model, chunks)
    assert one.shape == many.shape == (len(cand), 5) and bool(torch.isfinite(one).all())
    assert torch.equal(one, many)


def test_evaluate_ranks_and_inferred_parents_equal_the_host_on_the_same_vectors(tmp_path):
    from taxoexpan_amd import scoring
    from taxoexpan_amd.evaluate import candidate_graphs, evaluate, infer
    ds = _toy(tmp_path, "test", expand_factor=100)
    model = _toy_model().eval()
    dtax = ds.device_taxonomy(_dev())
    _metrics, ranks, pos_off, queries = evaluate(model, ds, _dev(), seed=3)
    cand = sorted(ds.all_positions)
    index = {a: i for i, a in enumerate(cand)}
    hg = scoring.encode_candidates(model, candidate_graphs(dtax, cand, ds.expand_factor, 3))
    qf = ds.node_features[torch.as_tensor(queries, dtype=torch.long)].to(_dev())
    S = scoring.score_all(model.match, hg, qf).cpu().numpy()
    want = []
    for i, qn in enumerate(queries):
        want += orc.ranks_of_positives(S[i], [index[a] for a in ds.node2parents[qn] if a in index], True)
    assert len(queries) >= 5 and ranks.cpu().tolist() == want and int(pos_off[-1]) == len(want)
    # infer: every node of the graph is a candidate, in node order; best first, ties by ascending candidate
    rs = np.random.RandomState(5)
    names, vecs = [f"new_{i}" for i in range(9)], rs.standard_normal((9, 8)).astype(np.float32)
    out = infer(model, ds, (names, vecs), _dev(), topk=5)
    anchors = list(ds.graph.nodes)
    hg_all = scoring.encode_candidates(model, candidate_graphs(dtax, np.asarray(anchors, dtype=np.int64), ds.expand_factor, 0))
    S = scoring.score_all(model.match, hg_all, torch.from_numpy(vecs).to(_dev())).cpu().numpy()
    for (name, parents), row, n in zip(out, S, names):
        top = sorted(enumerate(row.tolist()), key=lambda e: -e[1])[:5]
        assert name == n and parents == [ds.vocab[anchors[i]] for i, _ in top]


def test_one_training_epoch_on_device_sampled_batches(tmp_path):
    from taxoexpan_amd import optim
    from taxoexpan_amd.data_loaders import DeviceBatchLoader
    from taxoexpan_amd.trainer import train_epoch
    model = _toy_model("BIM")
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    loader = DeviceBatchLoader(_toy(tmp_path, "train"), 16, _dev(), shuffle=True, seed=5, sampler="device")
    log = train_epoch(model, loader, optim.Adam(model.parameters(), lr=1e-3, amsgrad=True))
    assert log["n_batches"] == len(loader) > 1 and log["first_nonfinite"] == -1
    assert np.isfinite(log["losses"]).all() and np.isfinite(log["grad_norms"]).all() and (log["grad_norms"] > 0).all()
    moved = [k for k, v in model.state_dict().items() if not torch.equal(v, before[k])]
    assert {k for k in moved if k.startswith("readout.")} == {"readout.gate_hidden.weight", "readout.gate_hidden.bias",
                                                              "readout.gate_position.weight", "readout.gate_out.weight"}


def test_checkpoint_reloads_strictly_and_reproduces_the_ranks(tmp_path):
    from taxoexpan_amd import optim
    from taxoexpan_amd.data_loaders import DeviceBatchLoader
    from taxoexpan_amd.evaluate import evaluate
    from taxoexpan_amd.trainer import fit
    model = _toy_model()
    train = DeviceBatchLoader(_toy(tmp_path, "train"), 16, _dev(), shuffle=True, seed=5, sampler="device")
    valid = DeviceBatchLoader(_toy(tmp_path, "validation"), 16, _dev(), shuffle=True, seed=2, sampler="device")
    logs = fit(model, train, valid, optim.Adam(model.parameters(), lr=1e-3, amsgrad=True), 1, save_dir=tmp_path / "run", config={"name": "toy"})
    assert len(logs) == 1 and logs[0]["first_nonfinite"] == -1
    ck = torch.load(tmp_path / "run" / "checkpoint-epoch1.pth", map_location="cpu", weights_only=False)
    assert {k for k in ck["state_dict"] if k.startswith("readout.")} == {"readout.gate_hidden.weight", "readout.gate_hidden.bias",
                                                                          "readout.gate_position.weight", "readout.gate_out.weight"}
    fresh = _toy_model(state=ck["state_dict"])                               # strict=True
    ds = _toy(tmp_path, "test", expand_factor=100)
    m1, r1, off1, q1 = evaluate(model, ds, _dev(), seed=3)
    m2, r2, off2, q2 = evaluate(fresh, ds, _dev(), seed=3)
    assert torch.equal(r1.cpu(), r2.cpu()) and list(off1) == list(off2) and q1 == q2 and m1 == m2 and len(q1) >= 5
