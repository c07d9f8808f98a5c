"""The GAT and GCN message-passing kernels (txe_gat.hip, txe_gcn.hip) against FLOAT64, operator by operator, through the C ABI
(_lib.call: the test owns strides, alignment, ld_a, ld_da, n_pad and npw), at every edge of their host-side dispatch.

Reference: tests/message_passing_ref.py -- the one operation restated from oracle/txe_oracle.py's primitives (edge_softmax, scatter_sum,
_leaky, gcn_norm; tests/test_message_passing_ref_cpu.py holds it to orc.gat_layer / orc.gcn_layer) -- in float64 on the CPU, gradients
by autograd; yardstick: the same function in fp32 on the CPU; gate: golden_util.gate_against_f64 with its defaults, for the output, for
alpha and for every gradient.  Every gate prints "[gate] operator what device-error yardstick-error" (fractions of the tensor's largest
float64 entry); one assertion per case.  Attention dropout is the kernels' own counter-based mask, rng.keep_mask(seed, (E, H), p) in
destination-CSR order.  Backward cases use out_mode 0 (d_pre is the gradient with respect to the pre-activation output), so no
activation branch can differ between the two sides; the attention logit a_src + a_dst is ONE correctly rounded fp32 addition, whose sign
is the exact sum's: no branch audit is needed.

Graphs (message_passing_ref.py): a generic multigraph of 301 nodes and about 2,400 edges (in-degrees 0, 1, 2, 63, 64, 65, 128, 129, 200;
out-degrees 0, 1, 16, 17, 64, 65, 200; duplicates, self loops, the last node a hub, an isolated node; three destinations whose logits
span more than 180) and the batch of the 15 EGONETS of test_gpu_readout_match_ops.py (992 nodes).

Instance -> case (each case asserts ITS instance through the library profiler's launch names):
    gat_aggregate_fwd_kernel<4, 2|4|5|8, 0, false, 1>   FWD_CASES nvec 8, 128 | 132, 256 | 257, 320, 513, 600 | 321, 512, 641, 644
    gat_aggregate_fwd_kernel<2, 2|4|8, 0, false, 1>     (3, 6) | (2, 130), pad2 / offset2 layouts | (3, 342), layouts
    gat_aggregate_fwd_kernel<1, 2|4|8, 0, false, 1>     (3, 5) | (3, 43) | (5, 103), pad1 / offset1 layouts
    gat_aggregate_fwd_kernel<4, 2|4|5, 1|2|3, false, 1> test_forward_epilogues_against_float64 (nvec 128 | 256 | 320, 600)
    gat_aggregate_fwd_kernel<4, 5|8, 0..3, false, 2>, gat_aggregate_ego_kernel<2|3, 0..3>    test_other_forward_sweeps_at_the_walk_widths
    gat_bwd_edge_kernel<4|2|1, 2|4|8>, gat_bwd_edge_generic_kernel<4|2|1>, gat_bwd_node_kernel<4|2|1, 2|4|8>,
    gat_bwd_node_split_kernel<4|2|1>                     BWD_CASES (the names stand in the table)
    gcn_aggregate_kernel<4|2|1, 2|4|8>                   GCN_CASES, forward and backward

Measured on the MI355X, largest device error / yardstick error per operator over all cases of this file, and the largest device error
itself (fractions of the tensor's largest entry; the gate's floor is 2e-5):
    gat_aggregate_fwd (plain)      1.5  (out, 1.5e-7 against 1.0e-7: under the floor); largest 1.9e-6 (alpha with the widened logits: the
                                        fp32 rounding of a_src + a_dst near 95, which the yardstick shares)
    gat_aggregate_fwd (epilogues)  1.1  (out); largest 1.7e-7 (nx_a12)
    gat_aggregate_fwd (npw 2, walk) 1.1 (out); largest 1.9e-7 (nx_a12); out and alpha bit-equal to npw 1
    gat_aggregate_bwd              2.9  (d_ft, 3.4e-7 against 1.2e-7: under the floor); largest 9.0e-7 (d_a_src)
    gcn_norm / gcn_aggregate       2.5  (d_hw, 8.4e-7 against 3.4e-7: under the floor, the largest device error of the operator)
    head_mean                      1.0  (largest 8.1e-8); leaky_relu_bwd: bit-equal to the fp32 product
No case needed scale_floor.  The 133 cases take 8 s on the MI355X, most of it the CPU references; the slowest case 0.4 s.
"""
import numpy as np
import pytest
import torch

import message_passing_ref as mp
from test_gpu_readout_match_ops import EGONETS, _gate, _profiled

pytestmark = pytest.mark.gpu

ATTN_SLOPE, ACT_SLOPE, SEED = 0.2, 0.01, 4242
NAN = float("nan")


def _dev():
    return torch.device("cuda:0")


# ---- graphs, inputs, layouts ----------------------------------------------------------------------------------------------------------
_GRAPHS = {}


def _graph(name):
    if name not in _GRAPHS:
        from taxoexpan_amd.graph import BatchedDGLGraph, DGLGraph
        if name == "multigraph":
            src, dst = mp.generic_multigraph()
            n = mp.G1_N
            g = DGLGraph()
            g.add_nodes(n)
            g.add_edges(src, dst)
        else:
            assert mp.EGONETS == EGONETS
            src, dst, n = mp.egonet_batch()
            g = BatchedDGLGraph.from_egonet_shapes([s[0] for s in EGONETS], [s[1] for s in EGONETS])
            assert np.array_equal(g._src, src) and np.array_equal(g._dst, dst)
        csr = g.csr(_dev(), method="host")
        sc, dc = mp.in_csr_order(src, dst)
        assert csr.n_nodes == n and csr.n_edges == len(src) and np.array_equal(csr.col_src.cpu().numpy(), sc)
        rp = csr.rowptr_in.cpu().numpy()
        _GRAPHS[name] = dict(n=n, E=len(src), csr=csr, src=torch.from_numpy(sc), dst=torch.from_numpy(dc), rowptr=rp,
                             indeg=np.diff(rp), outdeg=np.diff(csr.rowptr_out.cpu().numpy()))
    return _GRAPHS[name]


def _place(a, layout, shape=None):
    """(view, base) on the device: 'plain' contiguous; 'pad<k>' a column view of a buffer with k more columns; 'offset<k>' a view that
    starts k floats into its buffer.  The view holds `a` (or stays NaN: an output), everything else of the buffer is NaN."""
    n, d = a.shape if a is not None else shape
    if layout == "plain":
        base = torch.full((n, d), NAN, device=_dev())
        view = base
    elif layout.startswith("pad"):
        k = int(layout[3:])
        base = torch.full((n, d + k), NAN, device=_dev())
        view = base[:, :d]
    else:
        assert layout.startswith("offset")
        k = int(layout[6:])
        base = torch.full((n * d + k,), NAN, device=_dev())
        view = base[k:].view(n, d)
        assert view.data_ptr() % 16 == (4 * k) % 16
    if a is not None:
        view.copy_(torch.from_numpy(a))
    return view, base


def _only_the_view_was_written(view, base, what):
    assert bool(torch.isfinite(view).all()), what
    assert int(torch.isnan(base).sum()) == base.numel() - view.numel(), what       # everything outside the view is still NaN


def _gat_inputs(gname, H, D):
    g = _graph(gname)
    rs = np.random.RandomState(1000 * H + D + (0 if gname == "multigraph" else 500000))
    ft = rs.standard_normal((g["n"], H * D)).astype(np.float32)
    a_s, a_d = rs.standard_normal((g["n"], H)).astype(np.float32), rs.standard_normal((g["n"], H)).astype(np.float32)
    if gname == "multigraph":
        mp.widen_logits(a_s)
    return ft, a_s, a_d


def _place_gat_inputs(ft, a_s, a_d, layout):
    """(ft, a_src, a_dst) views: layout 'row' = the model's (columns of one padded row, ld_a = the row pitch); anything else: ft in that
    layout, a_src | a_dst a separate [N][2H] array"""
    n, F = ft.shape
    H = a_s.shape[1]
    if layout == "row":
        pitch = (F + 2 * H + 3) // 4 * 4 + 4
        base = torch.full((n, pitch), NAN, device=_dev())
        base[:, :F] = torch.from_numpy(ft)
        base[:, F:F + H] = torch.from_numpy(a_s)
        base[:, F + H:F + 2 * H] = torch.from_numpy(a_d)
        return base[:, :F], base[:, F:F + H], base[:, F + H:F + 2 * H]
    a12 = torch.from_numpy(np.concatenate([a_s, a_d], 1)).to(_dev())
    return _place(ft, layout)[0], a12[:, :H], a12[:, H:]


def _keep(g, H, p, dtype):
    from taxoexpan_amd import rng
    return torch.from_numpy(rng.keep_mask(SEED, (g["E"], H), p)).to(dtype) if p > 0 else None


def _gat_ref(dtype, g, ft, a_s, a_d, H, D, p, out_mode, w=None):
    """(out [N][H*D], alpha [E][H], gradients of (ft, a_src, a_dst) under (out * w).sum() or None) of the GAT sweep in `dtype`"""
    ts = [torch.from_numpy(ft).to(dtype).reshape(g["n"], H, D), torch.from_numpy(a_s).to(dtype), torch.from_numpy(a_d).to(dtype)]
    if w is not None:
        ts = [t.requires_grad_(True) for t in ts]
    out, alpha = mp.gat_sweep(g["src"], g["dst"], g["n"], ts[0], ts[1], ts[2], ATTN_SLOPE, _keep(g, H, p, dtype), 1.0 / (1.0 - p),
                              ACT_SLOPE if out_mode == 1 else None)
    grads = None
    if w is not None:
        (out.flatten(1) * torch.from_numpy(w).to(dtype)).sum().backward()
        grads = [ts[0].grad.flatten(1).numpy(), ts[1].grad.numpy(), ts[2].grad.numpy()]
    return out.detach().flatten(1).numpy(), alpha.detach().numpy(), grads


def _alpha_sums(g, alpha):
    """per (destination, head): the sum of its in-edges' alpha, in float64"""
    out = np.zeros((g["n"], alpha.shape[1]))
    np.add.at(out, g["dst"].numpy(), np.asarray(alpha, dtype=np.float64))
    return out


def _fwd(g, ft, a_s, a_d, H, D, p, out_mode, out, alpha, npw=1, wa=None, kp=0, mask=None, nx_p=0.0, a12=None):
    from taxoexpan_amd import _lib
    csr = g["csr"]
    assert ft.stride(1) == 1 and out.stride(1) == 1 and a_s.stride(0) == a_d.stride(0)
    return _lib.call("txe_gat_aggregate_fwd", _lib.ptr(csr.rowptr_in), _lib.ptr(csr.col_src), g["n"], _lib.ptr(ft), ft.stride(0), _lib.ptr(a_s),
                     _lib.ptr(a_d), a_s.stride(0), H, D, ATTN_SLOPE, p, SEED, out_mode, ACT_SLOPE, _lib.ptr(out), out.stride(0), _lib.ptr(alpha),
                     _lib.ptr(wa), kp, _lib.ptr(mask), nx_p, _lib.ptr(a12), npw, _lib.stream_ptr())


# ---- 1. txe_gat_aggregate_fwd, one wave per node, plain epilogue ------------------------------------------------------------------------
# (H, D, input layout, output layout, the VEC the host must pick).  NI follows from nvec = H D / VEC: see _fwd_ni.
def _fwd_ni(vec, nvec):
    """the instance each width must reach (txe_gat_aggregate_fwd): 16-byte rows of 257..320 or 513..640 vectors take 5 per lane"""
    if vec == 4 and (256 < nvec <= 320 or 512 < nvec <= 640):
        return 5
    return 2 if nvec <= 128 else (4 if nvec <= 256 else 8)


_W4 = [(4, 8), (4, 128), (4, 132), (4, 256), (1, 1028), (4, 320), (1, 1284), (4, 512), (3, 684), (4, 600), (1, 2564), (4, 644)]
assert [h * d // 4 for h, d in _W4] == [8, 128, 132, 256, 257, 320, 321, 512, 513, 600, 641, 644]
FWD_CASES = [(H, D, "plain", "plain", 4) for H, D in _W4]
FWD_CASES += [(3, 6, "plain", "plain", 2), (2, 130, "plain", "plain", 2), (3, 342, "plain", "plain", 2)]          # nvec 9, 130, 513
FWD_CASES += [(3, 5, "plain", "plain", 1), (3, 43, "plain", "plain", 1), (5, 103, "plain", "plain", 1)]           # nvec 15, 129, 515
FWD_CASES += [(16, 4, "plain", "plain", 4), (5, 8, "plain", "plain", 4)]                                          # GAT_MAXH heads; past four
# one VEC-4 width per NI (2, 4, 5, 8) in the other layouts: the vector width kept (pad4), forced to 1 (pad1, offset1: input, output, both),
# forced to 2 (pad2 on the input; an 8-byte offset on the output)
for _H, _D in [(4, 128), (4, 132), (4, 320), (1, 1284)]:
    FWD_CASES += [(_H, _D, "pad4", "pad4", 4), (_H, _D, "pad1", "plain", 1), (_H, _D, "plain", "pad1", 1), (_H, _D, "offset1", "offset1", 1),
                  (_H, _D, "pad2", "plain", 2), (_H, _D, "plain", "offset2", 2)]
# a_src / a_dst as columns of ft's own padded row (ld_a = the row pitch, the model's layout)
FWD_CASES += [(4, 128, "row", "plain", 4), (4, 600, "row", "pad4", 4), (3, 6, "row", "plain", 2), (3, 5, "row", "plain", 1), (5, 8, "row", "plain", 4)]


def test_forward_cases_reach_every_plain_instance():
    got = {(v, _fwd_ni(v, H * D // v)) for H, D, _i, _o, v in FWD_CASES}
    assert got == {(4, 2), (4, 4), (4, 5), (4, 8), (2, 2), (2, 4), (2, 8), (1, 2), (1, 4), (1, 8)}
    two_pass = {(v, _fwd_ni(v, H * D // v)) for H, D, _i, _o, v in FWD_CASES if H * D // v > 64 * _fwd_ni(v, H * D // v)}
    assert two_pass >= {(4, 5), (4, 8), (2, 8), (1, 8)}                          # the second pass of the column loop, every VEC


@pytest.mark.parametrize("H,D,lin,lout,vec", FWD_CASES, ids=[f"H{H}-D{D}-{i}-{o}" for H, D, i, o, _v in FWD_CASES])
def test_forward_sweep_wave_per_node_against_float64(H, D, lin, lout, vec):
    """out_mode 0 | 1 x attention dropout 0 | 0.3, alpha kept: two of the four on either graph"""
    F = H * D
    kernel = f"gat_aggregate_fwd_kernel<{vec}, {_fwd_ni(vec, F // vec)}, 0, false, 1>"
    items = []
    for gname, combos in (("multigraph", [(0, 0.0), (1, 0.3)]), ("egonets", [(1, 0.0), (0, 0.3)])):
        g = _graph(gname)
        ft, a_s, a_d = _gat_inputs(gname, H, D)
        ftd, asd, add = _place_gat_inputs(ft, a_s, a_d, lin)
        for out_mode, p in combos:
            out, out_base = _place(None, lout, (g["n"], F))
            alpha = torch.full((g["E"] * H + 1,), NAN, device=_dev())
            _rc, names = _profiled(lambda: _fwd(g, ftd, asd, add, H, D, p, out_mode, out, alpha))
            assert names == [kernel], (names, kernel)
            tag = f"{gname} mode {out_mode} p {p}"
            _only_the_view_was_written(out, out_base, tag)                         # (plain mode: the columns behind H D too)
            assert bool(torch.isfinite(alpha[:-1]).all()) and bool(torch.isnan(alpha[-1])), tag
            o, al = out.cpu().numpy(), alpha[:-1].cpu().numpy().reshape(g["E"], H)
            assert not o[g["indeg"] == 0].any(), tag                              # no in-edge: an all-zero row, exactly
            o64, al64, _ = _gat_ref(torch.float64, g, ft, a_s, a_d, H, D, p, out_mode)
            o32, al32, _ = _gat_ref(torch.float32, g, ft, a_s, a_d, H, D, p, out_mode)
            s64 = _alpha_sums(g, al64)
            assert np.array_equal(s64 != 0, np.repeat((g["indeg"] > 0)[:, None], H, 1)) and np.abs(s64[g["indeg"] > 0] - 1).max() < 1e-12
            items += [(f"out [{tag}]", o, o64, o32), (f"alpha [{tag}]", al, al64, al32),
                      (f"alpha sums [{tag}]", _alpha_sums(g, al), s64, _alpha_sums(g, al32))]
    _gate("gat_aggregate_fwd", items)


# ---- 2. the forward epilogues (VEC 4 only: what the entry point accepts) --------------------------------------------------------------
# nvec 128, 256, 320, 600 -> gat_aggregate_fwd_kernel<4, 2 | 4 | 5 | 5 (two passes), M, false, 1>, M = 1 (nx_a12), 2 (nx_a12 + mask),
# 3 (nx_mask alone: the rows dropped); nx_kp = H D rounded up to 32 (= H D here: no column behind the features) and H D + 128
def _mask_bits(n, kp, p, seed):
    """(device mask words from txe_dropout_mask, their keep bits [n][kp] restated by rng.keep_mask_bits -- read back and compared)"""
    from taxoexpan_amd import _lib, rng
    mask = torch.empty((n, kp // 32), dtype=torch.int32, device=_dev())
    _lib.call("txe_dropout_mask", n, kp, p, seed, mask.data_ptr(), _lib.stream_ptr())
    keep = rng.keep_mask_bits(seed, n, kp, p)
    bits = ((mask.cpu().numpy().astype(np.int64)[:, :, None] >> np.arange(32)) & 1).reshape(n, -1)[:, :kp]
    assert np.array_equal(bits, keep.astype(np.int64))
    return mask, keep


def _epilogue_refs(g, ft, a_s, a_d, H, D, p, tail, keep, nx_p, wa):
    """per dtype: (the rows with the next layer's dropout applied, the plain rows, nx_a12)"""
    res = []
    for dtype in (torch.float64, torch.float32):
        o, _al, _ = _gat_ref(dtype, g, ft, a_s, a_d, H, D, p, 1)
        o = torch.from_numpy(o)
        k = torch.from_numpy(keep).to(dtype) if keep is not None else None
        dropped = (o * k[:, :H * D] * (1.0 / (1.0 - nx_p))).numpy() if k is not None else None
        x_next = torch.cat([o, torch.from_numpy(tail).to(dtype)], 1)
        a12 = mp.next_logits(x_next, k, 1.0 / (1.0 - nx_p), torch.from_numpy(wa).to(dtype)).numpy()
        res.append((dropped, o.numpy(), a12))
    return res


@pytest.mark.parametrize("mode", ["a12", "a12_mask", "rows_dropped"])
@pytest.mark.parametrize("kp_extra", [0, 128])
@pytest.mark.parametrize("H,D", [(4, 128), (4, 256), (4, 320), (4, 600)])
def test_forward_epilogues_against_float64(H, D, kp_extra, mode):
    g = _graph("multigraph")
    n, F = g["n"], H * D
    assert F % 32 == 0
    kp, p, nx_p = F + kp_extra, 0.3, (0.0 if mode == "a12" else 0.5)
    ft, a_s, a_d = _gat_inputs("multigraph", H, D)
    ftd, asd, add = _place_gat_inputs(ft, a_s, a_d, "plain")
    rs = np.random.RandomState(F + kp)
    tail = rs.standard_normal((n, kp - F)).astype(np.float32)                     # position columns of X' (the model pads them with zeros)
    wa = rs.standard_normal((2, kp)).astype(np.float32)
    mask, keep = _mask_bits(n, kp, nx_p, SEED + 1) if nx_p > 0 else (None, None)
    out = torch.full((n, kp), NAN, device=_dev())                                 # (the feature part: NaN until the sweep writes it)
    if mode != "rows_dropped":
        out[:, F:] = torch.from_numpy(tail)
    wad = torch.from_numpy(wa).to(_dev())
    a12 = torch.full((2 * n + 1,), NAN, device=_dev())
    alpha = torch.full((g["E"] * H,), NAN, device=_dev())
    with_a12 = mode != "rows_dropped"
    _rc, names = _profiled(lambda: _fwd(g, ftd, asd, add, H, D, p, 1, out, alpha, 1, wad if with_a12 else None, kp, mask, nx_p,
                                        a12 if with_a12 else None))
    M = {"a12": 1, "a12_mask": 2, "rows_dropped": 3}[mode]
    assert names == [f"gat_aggregate_fwd_kernel<4, {_fwd_ni(4, F // 4)}, {M}, false, 1>"], names
    o = out.cpu().numpy()
    (drop64, o64, a64), (drop32, o32, a32) = _epilogue_refs(g, ft, a_s, a_d, H, D, p, tail, keep, nx_p, wa)
    assert np.isfinite(o[:, :F]).all()
    if with_a12:
        assert np.array_equal(o[:, F:], tail)                                     # the columns behind the features: read, never written
        assert bool(torch.isnan(a12[-1])) and bool(torch.isfinite(a12[:-1]).all())
        _gate(f"gat_aggregate_fwd[{mode}]", [("out", o[:, :F], o64, o32), ("nx_a12", a12[:-1].cpu().numpy().reshape(n, 2), a64, a32)])
    else:
        assert np.isnan(o[:, F:]).all() and bool(torch.isnan(a12).all())
        assert not o[:, :F][keep[:, :F] == 0].any()                               # a dropped entry is 0, exactly; a kept one is not (unless the
        assert (o[:, :F] != 0)[(keep[:, :F] == 1) & (np.abs(o64) > 1e-30)].all()  # row itself is: no in-edge, or only underflown alpha kept)
        _gate(f"gat_aggregate_fwd[{mode}]", [("out", o[:, :F], drop64, drop32)])


# ---- 3. the other forward sweeps at the widths nobody compares them at -----------------------------------------------------------------
# H = 4, D = 512 | 516 | 768 (D / 4 = 128 | 129 | 192: gat_aggregate_ego_kernel<2 | 3 | 3, M>, the widest the walk accepts), on the egonet
# batch: npw 2 (gat_aggregate_fwd_kernel<4, 8 | 5 | 8, M, false, 2>) and the forced walk (npw 3 = a window size of the library's choice,
# 16) against npw 1 -- out and alpha bit for bit, nx_a12 (another summation order) within the gate against float64
@pytest.mark.parametrize("D", [512, 516, 768])
def test_other_forward_sweeps_at_the_walk_widths(D):
    H, p, nx_p = 4, 0.3, 0.5
    g = _graph("egonets")
    n, F = g["n"], H * D
    kp = (F + 50 + 31) // 32 * 32
    ft, a_s, a_d = _gat_inputs("egonets", H, D)
    ftd, asd, add = _place_gat_inputs(ft, a_s, a_d, "plain")
    rs = np.random.RandomState(D)
    tail = rs.standard_normal((n, kp - F)).astype(np.float32)
    wa = rs.standard_normal((2, kp)).astype(np.float32)
    wad = torch.from_numpy(wa).to(_dev())
    mask, keep = _mask_bits(n, kp, nx_p, SEED + 2)
    ni, nie = _fwd_ni(4, F // 4), (2 if D // 4 <= 128 else 3)
    modes = {"plain": 0, "a12": 1, "a12_mask": 2, "rows_dropped": 3}
    res = {}
    for npw in (1, 2, 3, 16):
        for mode, M in modes.items():
            out = torch.full((n, kp), NAN, device=_dev())
            out[:, F:] = torch.from_numpy(tail)
            alpha = torch.full((g["E"] * H + 1,), NAN, device=_dev())
            a12 = torch.full((2 * n,), NAN, device=_dev())
            with_a12, with_mask = M in (1, 2), M in (2, 3)
            _rc, names = _profiled(lambda: _fwd(g, ftd, asd, add, H, D, p, 1, out, alpha, npw, wad if with_a12 else None, kp,
                                                mask if with_mask else None, nx_p if with_mask else 0.0, a12 if with_a12 else None))
            want = f"gat_aggregate_fwd_kernel<4, {ni}, {M}, false, {npw}>" if npw <= 2 else f"gat_aggregate_ego_kernel<{nie}, {M}>"
            assert names == [want], (names, want)
            res[npw, mode] = (out.cpu().numpy(), alpha.cpu().numpy(), a12.cpu().numpy().reshape(n, 2))
    items = []
    refs = {True: _epilogue_refs(g, ft, a_s, a_d, H, D, p, tail, keep, nx_p, wa), False: _epilogue_refs(g, ft, a_s, a_d, H, D, p, tail, None, 0.0, wa)}
    for (npw, mode), (o, al, a12) in res.items():
        o1, al1, _a = res[1, mode]
        assert np.isfinite(o).all() and np.isfinite(al[:-1]).all() and np.isnan(al[-1]), (npw, mode)
        assert np.array_equal(o, o1) and np.array_equal(al, al1, equal_nan=True), (npw, mode)
        if mode.startswith("a12"):
            (_d64, _o64, a64), (_d32, _o32, a32) = refs[mode == "a12_mask"]
            items.append((f"nx_a12 [npw {npw} {mode}]", a12, a64, a32))
    (d64, o64, _a64), (d32, o32, _a32) = refs[True]
    items += [("out [npw 1 plain]", res[1, "plain"][0][:, :F], o64, o32), ("out [npw 1 rows_dropped]", res[1, "rows_dropped"][0][:, :F], d64, d32)]
    _gate("gat_aggregate_fwd[sweeps]", items)


def test_forced_walk_past_its_widest_row_is_an_argument_error():
    from taxoexpan_amd._lib import TxeError
    H, D = 4, 772
    g = _graph("egonets")
    ft, a_s, a_d = _gat_inputs("egonets", H, D)
    ftd, asd, add = _place_gat_inputs(ft, a_s, a_d, "plain")
    out = torch.full((g["n"], H * D), NAN, device=_dev())
    for npw in (3, 16):
        with pytest.raises(TxeError, match="TXE_ERR_ARG"):
            _fwd(g, ftd, asd, add, H, D, 0.0, 0, out, None, npw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                                           # (nothing was launched)


# ---- 4. txe_gat_aggregate_bwd ------------------------------------------------------------------------------------------------------
# (H, D, layouts of ft / d_pre / d_ft, the edge-side launch, the source-side launch).  Edge side: H <= 4 and nvec <= 512 ->
# gat_bwd_edge_kernel<VEC, NI>, else gat_bwd_edge_generic_kernel<VEC> (VEC from ft and d_pre); source side: 256 <= nvec <= 512 ->
# gat_bwd_node_split_kernel<VEC>, else gat_bwd_node_kernel<VEC, NI> (VEC from d_pre and d_ft).
E_, EG, ND, SP = "gat_bwd_edge_kernel", "gat_bwd_edge_generic_kernel", "gat_bwd_node_kernel", "gat_bwd_node_split_kernel"
BWD_CASES = [
    (4, 8, "plain", "plain", "plain", f"{E_}<4, 2>", f"{ND}<4, 2>"),              # nvec 8; H = 4 ...
    (5, 8, "plain", "plain", "plain", f"{EG}<4>", f"{ND}<4, 2>"),                 # ... against H = 5
    (4, 512, "plain", "plain", "plain", f"{E_}<4, 8>", f"{SP}<4>"),               # nvec 512: the widest of both
    (1, 2052, "plain", "plain", "plain", f"{EG}<4>", f"{ND}<4, 8>"),              # nvec 513: past both
    (4, 128, "plain", "plain", "plain", f"{E_}<4, 2>", f"{ND}<4, 2>"),            # nvec 128
    (4, 33, "row", "plain", "plain", f"{E_}<1, 4>", f"{ND}<1, 4>"),               # nvec 132 (VEC 1), a_src | a_dst in ft's row
    (4, 132, "row", "plain", "plain", f"{E_}<4, 4>", f"{ND}<4, 4>"),              # nvec 132 (VEC 4), the same
    (3, 340, "plain", "plain", "plain", f"{E_}<4, 4>", f"{ND}<4, 4>"),            # nvec 255: the last below the split kernel
    (4, 256, "plain", "plain", "plain", f"{E_}<4, 4>", f"{SP}<4>"),               # nvec 256: the first of the split kernel
    (4, 320, "pad4", "pad4", "pad4", f"{E_}<4, 8>", f"{SP}<4>"),                  # nvec 320
    (3, 6, "plain", "plain", "plain", f"{E_}<2, 2>", f"{ND}<2, 2>"),              # nvec 9
    (2, 130, "plain", "plain", "plain", f"{E_}<2, 4>", f"{ND}<2, 4>"),            # nvec 130
    (2, 258, "plain", "plain", "plain", f"{E_}<2, 8>", f"{SP}<2>"),               # nvec 258
    (3, 342, "plain", "plain", "plain", f"{EG}<2>", f"{ND}<2, 8>"),               # nvec 513
    (3, 5, "plain", "plain", "plain", f"{E_}<1, 2>", f"{ND}<1, 2>"),              # nvec 15
    (3, 43, "plain", "plain", "plain", f"{E_}<1, 4>", f"{ND}<1, 4>"),             # nvec 129
    (3, 101, "plain", "plain", "plain", f"{E_}<1, 8>", f"{SP}<1>"),               # nvec 303
    (5, 103, "plain", "plain", "plain", f"{EG}<1>", f"{ND}<1, 8>"),               # nvec 515
    (4, 128, "plain", "plain", "offset1", f"{E_}<4, 2>", f"{SP}<1>"),             # ft and d_pre 16-byte aligned, d_ft not: the two launches
    (4, 256, "plain", "plain", "pad2", f"{E_}<4, 4>", f"{SP}<2>"),                # of one call at different VEC (nvec 128 | 512, 256 | 512)
    (4, 128, "pad1", "plain", "plain", f"{E_}<1, 8>", f"{ND}<4, 2>"),             # ... and the other way round (nvec 512 | 128)
    (16, 4, "plain", "plain", "plain", f"{EG}<4>", f"{ND}<4, 2>"),                # GAT_MAXH heads
]


def test_backward_cases_reach_every_instance():
    edge, node = {c[5] for c in BWD_CASES}, {c[6] for c in BWD_CASES}
    assert edge == {f"{E_}<{v}, {i}>" for v in (4, 2, 1) for i in (2, 4, 8)} | {f"{EG}<{v}>" for v in (4, 2, 1)}
    assert node == {f"{ND}<{v}, {i}>" for v in (4, 2, 1) for i in (2, 4, 8)} | {f"{SP}<{v}>" for v in (4, 2, 1)}


@pytest.mark.parametrize("H,D,l_ft,l_dpre,l_dft,edge,node", BWD_CASES, ids=[f"H{c[0]}-D{c[1]}-{c[2]}-{c[3]}-{c[4]}" for c in BWD_CASES])
def test_backward_sweeps_against_float64(H, D, l_ft, l_dpre, l_dft, edge, node):
    """both graphs x attention dropout 0 | 0.3; alpha from the forward call of the same case; ld_da = H + 40 with n_pad 30 (multigraph)
    and n_pad 0 (egonets): exactly the n_pad floats behind d_a_dst[v][H - 1] become 0, the next keeps its NaN"""
    from taxoexpan_amd import _lib
    F, ld_da = H * D, H + 40
    items = []
    for gname, n_pad in (("multigraph", 30), ("egonets", 0)):
        g = _graph(gname)
        csr, n, E = g["csr"], g["n"], g["E"]
        ft, a_s, a_d = _gat_inputs(gname, H, D)
        ftd, asd, add = _place_gat_inputs(ft, a_s, a_d, l_ft)
        w = np.random.RandomState(F + n_pad).standard_normal((n, F)).astype(np.float32)
        dpre = _place(w, l_dpre)[0]
        for p in (0.0, 0.3):
            tag = f"{gname} p {p}"
            out = torch.empty((n, F), device=_dev())
            alpha = torch.full((E * H,), NAN, device=_dev())
            _fwd(g, ftd, asd, add, H, D, p, 0, out, alpha)
            dft, dft_base = _place(None, l_dft, (n, F))
            das, dad = torch.full((n, ld_da), NAN, device=_dev()), torch.full((n, ld_da), NAN, device=_dev())
            dz = torch.full((E * H + 1,), NAN, device=_dev())

            def run():
                return _lib.call("txe_gat_aggregate_bwd", _lib.ptr(csr.rowptr_in), _lib.ptr(csr.col_src), _lib.ptr(csr.rowptr_out), _lib.ptr(csr.col_dst),
                                 _lib.ptr(csr.pos_out), n, _lib.ptr(ftd), ftd.stride(0), _lib.ptr(asd), _lib.ptr(add), asd.stride(0), H, D, ATTN_SLOPE, p,
                                 SEED, _lib.ptr(alpha), _lib.ptr(dpre), dpre.stride(0), _lib.ptr(dft), dft.stride(0), _lib.ptr(das), _lib.ptr(dad), ld_da,
                                 _lib.ptr(dz), n_pad, _lib.stream_ptr())
            _rc, names = _profiled(run)
            assert names == [edge, node], (names, edge, node)
            _only_the_view_was_written(dft, dft_base, tag)
            assert bool(torch.isfinite(dz[:-1]).all()) and bool(torch.isnan(dz[-1])), tag
            d_ft, d_as, d_ad = dft.cpu().numpy(), das.cpu().numpy(), dad.cpu().numpy()
            assert np.isfinite(d_as[:, :H]).all() and np.isnan(d_as[:, H:]).all(), tag
            assert np.isfinite(d_ad[:, :H]).all() and not d_ad[:, H:H + n_pad].any() and np.isnan(d_ad[:, H + n_pad:]).all(), tag
            assert not d_ad[g["indeg"] == 0, :H].any(), tag                      # no in-edge: zero d_a_dst, exactly
            assert not d_ft[g["outdeg"] == 0].any() and not d_as[g["outdeg"] == 0, :H].any(), tag      # no out-edge: zero d_ft and d_a_src
            _o, _a, g64 = _gat_ref(torch.float64, g, ft, a_s, a_d, H, D, p, 0, w)
            _o, _a, g32 = _gat_ref(torch.float32, g, ft, a_s, a_d, H, D, p, 0, w)
            items += [(f"d_ft [{tag}]", d_ft, g64[0], g32[0]), (f"d_a_src [{tag}]", d_as[:, :H], g64[1], g32[1]),
                      (f"d_a_dst [{tag}]", d_ad[:, :H], g64[2], g32[2])]
    _gate("gat_aggregate_bwd", items)


# ---- 5. txe_gcn_norm, txe_gcn_aggregate_fwd, txe_gcn_aggregate_bwd -------------------------------------------------------------------
# (F, layout of the input (hw | d_pre), layout of the output (out | d_hw), VEC) -> gcn_aggregate_kernel<VEC, pick_ni(F / VEC)>, forward
# and backward; F / VEC > 512: the second pass of the column loop (2052, 1030, 515)
GCN_CASES = [(8, "plain", "plain", 4), (512, "plain", "plain", 4), (528, "plain", "plain", 4), (1024, "plain", "plain", 4), (2052, "plain", "plain", 4),
             (6, "plain", "plain", 2), (258, "plain", "plain", 2), (1030, "plain", "plain", 2),
             (5, "plain", "plain", 1), (129, "plain", "plain", 1), (515, "plain", "plain", 1),
             (528, "pad4", "pad4", 4), (528, "pad1", "plain", 1), (528, "plain", "offset1", 1), (528, "pad2", "plain", 2),
             (258, "pad2", "pad2", 2), (258, "plain", "pad1", 1), (258, "offset1", "plain", 1), (129, "pad3", "pad3", 1)]


def _gcn_ni(nvec):
    return 2 if nvec <= 128 else (4 if nvec <= 256 else 8)


def test_gcn_cases_reach_all_nine_instances():
    assert {(v, _gcn_ni(F // v)) for F, _i, _o, v in GCN_CASES} == {(v, i) for v in (4, 2, 1) for i in (2, 4, 8)}
    assert {(F, v) for F, _i, _o, v in GCN_CASES if F // v > 512} >= {(2052, 4), (1030, 2), (515, 1)}


def _gcn_ref(dtype, g, x, bias, act, w=None):
    xt = torch.from_numpy(x).to(dtype).requires_grad_(w is not None)
    bt = torch.from_numpy(bias).to(dtype).requires_grad_(w is not None) if bias is not None else None
    out = mp.gcn_sweep(g["src"], g["dst"], g["n"], xt, bt, ACT_SLOPE if act else None)
    if w is None:
        return out.detach().numpy()
    (out * torch.from_numpy(w).to(dtype)).sum().backward()
    return out.detach().numpy(), xt.grad.numpy(), bt.grad.numpy()


def _gcn_norm(g):
    from taxoexpan_amd import _lib
    import txe_oracle as orc
    norm = torch.full((g["n"] + 1,), NAN, device=_dev())
    _lib.call("txe_gcn_norm", _lib.ptr(g["csr"].rowptr_in), g["n"], _lib.ptr(norm), _lib.stream_ptr())
    assert bool(torch.isnan(norm[-1]))
    nd = norm[:-1].cpu().numpy()
    assert not nd[g["indeg"] == 0].any()                                          # in-degree 0: norm 0, not inf
    return norm, (nd[:, None], orc.gcn_norm(g["dst"], g["n"], torch.float64).numpy(), orc.gcn_norm(g["dst"], g["n"], torch.float32).numpy())


@pytest.mark.parametrize("F,lin,lout,vec", GCN_CASES, ids=[f"F{c[0]}-{c[1]}-{c[2]}" for c in GCN_CASES])
def test_gcn_sweeps_against_float64(F, lin, lout, vec):
    from taxoexpan_amd import _lib
    kernel = f"gcn_aggregate_kernel<{vec}, {_gcn_ni(F // vec)}>"
    items = []
    for gname, combos in (("multigraph", [(True, 1), (False, 0)]), ("egonets", [(True, 0), (False, 1)])):
        g = _graph(gname)
        csr, n = g["csr"], g["n"]
        norm, norm_item = _gcn_norm(g)
        items.append((f"norm [{gname}]",) + norm_item)
        rs = np.random.RandomState(F + n)
        x, bias, w = (rs.standard_normal(s).astype(np.float32) for s in ((n, F), (F,), (n, F)))
        xd = _place(x, lin)[0]
        bd = torch.from_numpy(bias).to(_dev())
        for with_bias, act in combos:
            tag = f"{gname} bias {int(with_bias)} act {act}"
            out, out_base = _place(None, lout, (n, F))
            _rc, names = _profiled(lambda: _lib.call("txe_gcn_aggregate_fwd", _lib.ptr(csr.rowptr_in), _lib.ptr(csr.col_src), n, _lib.ptr(xd), xd.stride(0),
                                                     _lib.ptr(norm), _lib.ptr(bd) if with_bias else None, act, ACT_SLOPE, F, _lib.ptr(out), out.stride(0),
                                                     _lib.stream_ptr()))
            assert names == [kernel], (names, kernel)
            _only_the_view_was_written(out, out_base, tag)
            o = out.cpu().numpy()
            b = bias if with_bias else None
            if not act:                                                           # in-degree 0: the output is the bias, exactly
                assert np.array_equal(o[g["indeg"] == 0], np.broadcast_to(bias if with_bias else np.zeros(F, np.float32), (int((g["indeg"] == 0).sum()), F))), tag
            items.append((f"out [{tag}]", o, _gcn_ref(torch.float64, g, x, b, act), _gcn_ref(torch.float32, g, x, b, act)))
        # backward: d_pre = w (has_act 0); d_hw in the output layout -- a plain one is widened so that columns lie behind roundup(F, 32)
        dpre = _place(w, lin)[0]
        pad32 = (F + 31) // 32 * 32
        dhw, dhw_base = _place(None, f"pad{pad32 - F + 8}" if lout == "plain" else lout, (n, F))
        zend = min(dhw.stride(0), pad32)
        wsb = _lib.call("txe_gcn_aggregate_bwd_ws_bytes", n, F)
        assert wsb == (n + 127) // 128 * F * 4
        ws = torch.empty(wsb, dtype=torch.uint8, device=_dev())
        db = torch.full((F + 1,), NAN, device=_dev())

        def bwd(d_bias, ws_bytes):
            return _lib.call("txe_gcn_aggregate_bwd", _lib.ptr(csr.rowptr_out), _lib.ptr(csr.col_dst), n, _lib.ptr(dpre), dpre.stride(0), _lib.ptr(norm), F,
                             _lib.ptr(dhw), dhw.stride(0), _lib.ptr(d_bias), _lib.ptr(ws) if d_bias is not None else None, ws_bytes, _lib.stream_ptr())
        _rc, names = _profiled(lambda: bwd(db, wsb))
        assert [k for k in names if k.startswith("gcn_aggregate")] == [kernel], (names, kernel)
        d_hw, d_b = dhw.cpu().numpy(), db.cpu().numpy()
        assert np.isfinite(d_hw).all() and np.isfinite(d_b[:F]).all() and np.isnan(d_b[F]), gname
        if dhw_base.dim() == 2:      # the columns [F, min(ld_dhw, roundup(F, 32))) are 0, the ones beyond keep their NaN
            rest = dhw_base.cpu().numpy()[:, F:]
            assert not rest[:, :zend - F].any() and np.isnan(rest[:, zend - F:]).all(), (gname, zend)
        else:                        # (an offset view: ld_dhw = F, nothing behind a row; the floats in front of the view stay NaN)
            assert bool(torch.isnan(dhw_base[:dhw_base.numel() - n * F]).all())
        assert not d_hw[g["outdeg"] == 0].any(), gname
        _o, dx64, db64 = _gcn_ref(torch.float64, g, x, bias, 0, w)
        _o, dx32, db32 = _gcn_ref(torch.float32, g, x, bias, 0, w)
        items += [(f"d_hw [{gname}]", d_hw, dx64, dx32), (f"d_bias [{gname}]", d_b[:F], db64, db32)]
        dhw.fill_(NAN)                                                            # d_bias = NULL: d_hw alone, no workspace asked for
        bwd(None, 0)
        torch.cuda.synchronize()
        assert np.array_equal(dhw.cpu().numpy(), d_hw)
        with pytest.raises(_lib.TxeError, match="TXE_ERR_WORKSPACE"):
            bwd(db, wsb - 4)
    _gate("gcn_aggregate", items)


# ---- 6. txe_head_mean_fwd / _bwd, txe_leaky_relu_bwd ------------------------------------------------------------------------------------
GRID_SPAN = 2048 * 256                     # threads of the largest grid: one element more takes a second trip of the grid-stride loop


@pytest.mark.parametrize("H", [1, 3, 4])
@pytest.mark.parametrize("D", [1, 5, 500])
def test_head_mean_against_float64(H, D):
    from taxoexpan_amd import _lib
    n = 301 if D > 1 else GRID_SPAN + 1                                            # (D = 1: n D = H-th part of n H D -- both past one grid)
    rs = np.random.RandomState(H * 1000 + D)
    x, dy = rs.standard_normal((n, H, D)).astype(np.float32), rs.standard_normal((n, D)).astype(np.float32)
    xd, dyd = torch.from_numpy(x).to(_dev()), torch.from_numpy(dy).to(_dev())
    y, dx = torch.full((n * D + 1,), NAN, device=_dev()), torch.full((n * H * D + 1,), NAN, device=_dev())
    _lib.call("txe_head_mean_fwd", _lib.ptr(xd), H, D, n, _lib.ptr(y), _lib.stream_ptr())
    _lib.call("txe_head_mean_bwd", _lib.ptr(dyd), H, D, n, _lib.ptr(dx), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[-1])) and bool(torch.isnan(dx[-1]))
    res = []
    for dtype in (torch.float64, torch.float32):
        xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
        out = mp.head_mean(xt)
        (out * torch.from_numpy(dy).to(dtype)).sum().backward()
        res.append((out.detach().numpy(), xt.grad.numpy()))
    _gate("head_mean", [("y", y[:-1].cpu().numpy().reshape(n, D), res[0][0], res[1][0]),
                        ("d_x", dx[:-1].cpu().numpy().reshape(n, H, D), res[0][1], res[1][1])])
    for name in ("txe_head_mean_fwd", "txe_head_mean_bwd"):                        # n = 0: TXE_OK, nothing touched
        assert _lib.call(name, None, H, D, 0, None, _lib.stream_ptr()) == 0


@pytest.mark.parametrize("n", [1, 1000, GRID_SPAN + 1])
def test_leaky_relu_bwd_against_its_definition(n):
    """d_pre = d_out * (out_act > 0 ? 1 : slope): exact in fp32 up to the one rounding of the product; out_act exactly 0 and -0.0 take
    the slope (F.leaky_relu's gradient at 0)"""
    from taxoexpan_amd import _lib
    rs = np.random.RandomState(n)
    act, dout = rs.standard_normal(n).astype(np.float32), rs.standard_normal(n).astype(np.float32)
    act[::7] = 0.0
    act[3::7] = -0.0
    ad, dd = torch.from_numpy(act).to(_dev()), torch.from_numpy(dout).to(_dev())
    dpre = torch.full((n + 1,), NAN, device=_dev())
    _lib.call("txe_leaky_relu_bwd", _lib.ptr(dd), _lib.ptr(ad), ACT_SLOPE, n, _lib.ptr(dpre), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(dpre[-1]))
    got = dpre[:-1].cpu().numpy()
    factor = np.where(act > 0, 1.0, np.float64(np.float32(ACT_SLOPE)))
    ref64 = dout.astype(np.float64) * factor
    ref32 = (dout * factor.astype(np.float32)).astype(np.float32)
    assert np.array_equal(got[act == 0], ref32[act == 0]) and np.array_equal(got[act > 0], dout[act > 0])
    _gate("leaky_relu_bwd", [("d_pre", got, ref64, ref32)])
    assert _lib.call("txe_leaky_relu_bwd", None, None, ACT_SLOPE, 0, None, _lib.stream_ptr()) == 0
