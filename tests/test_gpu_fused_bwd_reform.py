"""GPU: the fused backward's egonet walk with the X' rows of parents and siblings FORMED AGAIN from the Y rows it reads anyway
(gat_fused_bwd_ego_kernel<.., REFORM>, the default) against the walk that loads them (phases | TXE_WALK_NO_REFORM).

The two routes must agree bit for bit, which they can only do if the re-formed row IS the stored one: so every case first runs the
layer below's forward (txe_gat_aggregate_fwd: the walk, or one wave per node) on random Y rows -- that writes X' columns [0, F) and
alpha -- then the folded layer's forward on the device, then txe_gat_collapse_bwd_fused once per route on NaN-primed buffers, through
the C ABI as test_gpu_folded_layer_ops.py does.  What is compared, as raw bits: d_Y (all columns), the scratch dz_p, every parameter
gradient, and the WHOLE workspace -- it holds dal, the per-workgroup d_wa and position partials and hpart (and nothing that a run leaves
to chance: a route is also compared with a second run of itself).

Which instantiation ran cannot be seen in the launch names (they are the same on purpose); it is read off the algorithmic-byte figure
the library's profiler records for the launch, which the re-forming route lowers by 4 (N - G) F bytes."""
import ctypes

import numpy as np
import pytest
import torch

import folded_layer_ref as fl
from test_gpu_folded_layer_ops import (ACT_SLOPE, ATTN_SLOPE, NAN, SEED, VOCAB, _batch, _dev, _FoldState, _grad_buffers, _named, _nan,
                                       _pack_gat, _ptr, _up, _ws)
from test_gpu_message_passing_ops import _mask_bits

pytestmark = pytest.mark.gpu

FEAT_P = 0.3
REVERSED = 5                  # the egonet of the batch whose self loops come first in edge order: its siblings' in-lists are [self, hub]
SHAPES_HEAD = [(0, 0), (0, 4), (3, 0), (5, 7), (1, 1), (2, 3)]      # a single node, no parents, no siblings, the largest, ..., REVERSED


def egonets_with_parents_and_siblings(kind):
    """'egonets': 40 egonets of 0-5 parents and 0-7 siblings (SHAPES_HEAD first); 'big': one egonet of 70 nodes (more than the 64 the
    walk holds: the generic body); 'multi': an egonet with a doubled parent -> anchor edge and a sibling -> sibling edge (not hub-shaped)"""
    rs = np.random.RandomState(23)
    if kind == "egonets":
        shapes = SHAPES_HEAD + [(int(rs.randint(0, 6)), int(rs.randint(0, 8))) for _ in range(40 - len(SHAPES_HEAD))]
        parts = [fl._egonet(k, m) for k, m in shapes]
        graphs, pos = [p[0] for p in parts], [p[1] for p in parts]
        k, m = shapes[REVERSED]
        n, s, d = graphs[REVERSED]
        graphs[REVERSED] = (n, np.concatenate([s[k + m:], s[:k + m]]), np.concatenate([d[k + m:], d[:k + m]]))
        b = fl._finish(graphs, np.concatenate(pos))
        b["shapes"] = shapes
        return b
    if kind == "big":
        g, p = fl._egonet(20, 49)
        return fl._finish([g], np.asarray(p))
    (n, s, d), p = fl._egonet(3, 4)
    return fl._finish([(n, np.append(s, [0, 5]), np.append(d, [3, 6]))], np.asarray(p))


for _kind in ("egonets", "big", "multi"):
    fl.BATCHES.setdefault("reform_" + _kind, lambda _kind=_kind: egonets_with_parents_and_siblings(_kind))
BATCHES = ("reform_egonets", "reform_big", "reform_multi")
WIDTHS = [(16, 8), (512, 50)]         # (Dp, Pd): rows of 64 feature columns (NI = 1) and of 2,048 (NI = 2)


def _profiled_work(fn):
    """fn() with the library profiler on -> [(launch name, its algorithmic-work figure)]"""
    from taxoexpan_amd import _lib
    lib = _lib.load()
    lib.txe_profile_reset()
    lib.txe_profile_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(64)
        ms, work, kind = ctypes.c_float(), ctypes.c_double(), ctypes.c_int()
        recs = []
        for i in range(lib.txe_profile_count()):
            assert lib.txe_profile_get(i, buf, 64, ctypes.byref(ms), ctypes.byref(work), ctypes.byref(kind)) == 0
            recs.append((buf.value.decode(), work.value))
    finally:
        lib.txe_profile_enable(0)
        lib.txe_profile_reset()
    return recs


class _Case:
    """random Y rows, the layer below's forward (fwd_npw: txe_gat_aggregate_fwd's npw argument -- 8 = its egonet walk, 4 = one wave per
    node), the folded layer's forward; run() = one fused backward pass on fresh NaN buffers"""

    def __init__(self, bname, Dp, Pd, masked, pp, fwd_npw, Hp=4, inf_rows=(), keep_row=None, dropped=False):
        from taxoexpan_amd import _lib
        self.b = b = _batch(bname)
        csr = b["csr"]
        n, E, G, F_, D = b["n"], b["E"], b["G"], Hp * Dp, 6
        Kt, Kp = F_ + Pd, fl.padded_k(F_, Pd)
        rs = np.random.RandomState(900 + Dp + Hp)
        f = lambda *s: rs.standard_normal(s).astype(np.float32)
        self.inp = inp = dict(P=f(VOCAB, Pd), W=f(D, Kt) / np.float32(np.sqrt(Kt)), al=f(D) / np.float32(np.sqrt(D)), ar=f(D) / np.float32(np.sqrt(D)),
                              w=f(G, D), Hp=Hp, Dp=Dp, Kh=F_, Pd=Pd, D=D, Kt=Kt, Kp=Kp)
        self.ld = ld = F_ + 2 * Hp + 4
        Yp = np.full((n, ld), NAN, dtype=np.float32)
        Yp[:, :F_ + 2 * Hp] = f(n, F_ + 2 * Hp)
        for r in inf_rows:
            Yp[r, 3] = np.inf
        self.Yp = _up(Yp)
        X = np.full((n, Kp), NAN, dtype=np.float32)         # (the feature columns: the layer below's forward writes them)
        X[:, F_:Kt], X[:, Kt:] = inp["P"][b["pos"]], 0.0
        self.p = p = FEAT_P if (masked or keep_row is not None) else 0.0
        if keep_row is not None:                            # a keep mask of ONE row: every other row of Xd' is zero
            self.mask = torch.zeros((n, Kp // 32), dtype=torch.int32, device=_dev())
            self.mask[keep_row] = -1
        else:
            self.mask = _mask_bits(n, Kp, p, SEED)[0] if masked else None
        self.pw = np.array([[0.3], [-0.2], [0.5]], dtype=np.float32)
        self.pp = pp
        self.alpha_p = _nan(E, Hp)
        self.st = st = _FoldState(b, dict(inp, X=X), _pack_gat(inp), self.mask, p, self.pw, 0.0)
        yp = self.Yp.data_ptr()
        # dropped: the forward applies the next layer's feature dropout to the rows it stores (its NX == 3 form)
        nx = (None, Kp, self.mask.data_ptr(), p, None) if dropped else (None, 0, None, 0.0, None)
        _lib.call("txe_gat_aggregate_fwd", csr.rowptr_in.data_ptr(), csr.col_src.data_ptr(), n, yp, ld, yp + 4 * F_, yp + 4 * (F_ + Hp), ld, Hp, Dp,
                  ATTN_SLOPE, pp, SEED + 3, 1, ACT_SLOPE, st.X.data_ptr(), Kp, self.alpha_p.data_ptr(), *nx, fwd_npw, _lib.stream_ptr())
        st.forward()
        self.d_hg = _up(inp["w"])
        self.wsb = _lib.call("txe_gat_collapse_bwd_fused_ws_bytes", n, E, G, F_, Pd, D, VOCAB, Hp)
        self.x_skipped_bytes = 4.0 * (n - G) * F_

    def plan(self):
        from taxoexpan_amd import _lib
        b, csr = self.b, self.b["csr"]
        plan = torch.full((_lib.call("txe_egonet_walk_plan_bytes", b["n"]) // 4,), -1, dtype=torch.int32, device=_dev())
        _lib.call("txe_egonet_walk_plan", csr.rowptr_in.data_ptr(), csr.col_src.data_ptr(), csr.rowptr_out.data_ptr(), csr.col_dst.data_ptr(),
                  csr.pos_out.data_ptr(), csr.graph_off.data_ptr(), b["n"], b["G"], plan.data_ptr(), _lib.stream_ptr())
        return plan

    def run(self, extra=0, plan=None):
        """-> (every buffer the call wrote, [(launch name, work)] of the launches test_gpu_folded_layer_ops names)"""
        from taxoexpan_amd import _lib
        b, inp, st = self.b, self.inp, self.st
        n, E, Hp = b["n"], b["E"], inp["Hp"]
        d_Yp, dz_p = _nan(n, self.ld), _nan(E * Hp + 1)
        bufs, grads = _grad_buffers(inp, self.pw)
        below = _lib.GatFoldBelow(Yp=self.Yp.data_ptr(), ld_yp=self.ld, Hp=Hp, Dp=inp["Dp"], attn_slope_p=ATTN_SLOPE, attn_drop_p_p=self.pp,
                                  seed_p=SEED + 3, alpha_p=self.alpha_p.data_ptr(), d_Yp=d_Yp.data_ptr(), ld_dyp=self.ld, n_pad=0, dz_p=dz_p.data_ptr())
        ws = _ws(self.wsb)
        recs = _profiled_work(lambda: _lib.call(
            "txe_gat_collapse_bwd_fused", _lib.ref(b["gb"]), _lib.ref(st.layer), _lib.ref(below), None, _lib.ref(grads), self.d_hg.data_ptr(), inp["D"],
            ACT_SLOPE, _lib.FUSED_ALL | extra, None, 0, _ptr(plan), None, ws.data_ptr(), self.wsb, _lib.stream_ptr()))
        out = dict(d_Y=d_Yp, dz_p=dz_p, workspace=ws, **{k: v for k, v in bufs.items() if v is not None})
        return out, [r for r in recs if _named([r[0]])]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


def _sweep_work(recs):
    (w,) = [work for name, work in recs if name.startswith("gat_fused_bwd")]
    return w


def _both_routes(c, plan, what):
    """the default call and the call with TXE_WALK_NO_REFORM: the same launch names, the work figure apart by the rows not read, the same
    bits -> the default route's buffers"""
    from taxoexpan_amd import _lib
    on, recs_on = c.run(plan=plan)
    off, recs_off = c.run(_lib.WALK_NO_REFORM, plan=plan)
    names = [r[0] for r in recs_on]
    assert names == [r[0] for r in recs_off] == fl.fused_launches(c.inp["Kp"], c.mask is not None, 4, c.inp["Dp"]), (what, names)
    assert _sweep_work(recs_off) - _sweep_work(recs_on) == c.x_skipped_bytes, what
    _same_bits(on, off, what)
    return on


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("Dp,Pd", WIDTHS, ids=["F64", "F2048"])
@pytest.mark.parametrize("bname", BATCHES)
def test_reformed_rows_give_the_bits_of_loaded_rows(bname, Dp, Pd, masked):
    """every buffer of txe_gat_collapse_bwd_fused, route on against route off: attention dropout 0, 0.1 and 0.5 in the layer below (some
    coefficients exactly 0); with a walk plan (rows written by the forward walk) and without one (rows written by one wave per node);
    windows of at most 32 list positions cut the egonets of the 40-graph batch, so foreign hubs and the hub fix-up run"""
    for pp in (0.0, 0.1, 0.5):
        for planned in (False, True):
            c = _Case(bname, Dp, Pd, masked, pp, 8 if planned else 4)
            what = f"{bname} Dp {Dp} mask {int(masked)} attention dropout {pp} plan {int(planned)}"
            on = _both_routes(c, c.plan() if planned else None, what)
            if pp == 0.1:
                again, _r = c.run(plan=c.plan() if planned else None)
                _same_bits(on, again, what + ": run twice")
            F_ = 4 * Dp
            assert bool(torch.isfinite(on["d_Y"][:, :F_ + 8]).all()) and bool(torch.isnan(on["d_Y"][:, F_ + 8:]).all()), what


@pytest.mark.parametrize("fwd_npw", [8, 4], ids=["fwd_walk", "fwd_wave_per_node"])
def test_the_reformed_row_is_the_stored_row(fwd_npw):
    """The d_wa partials are sum_u da_u Xd'[u] with Xd'[u] = fscale keep[u] X'[u].  The C entry takes no da, so the one-hot is made on the
    other factor: a keep mask that keeps ONE row u (a parent; a sibling with in-list [hub, self]; a parent and a sibling of the egonet whose
    in-lists are [self, hub]).  The partials are then da_u fscale X'[u] alone -- of the stored row on one route, of the re-formed row on
    the other -- so a wrong coefficient or FMA order in that one row cannot hide in a sum over rows."""
    b = _batch("reform_egonets")
    off = b["graph_off"]
    k3, k5 = b["shapes"][3][0], b["shapes"][REVERSED][0]
    rows = {"parent": int(off[3]), "sibling": int(off[3]) + k3 + 1, "parent, reversed in-lists": int(off[REVERSED]),
            "sibling, reversed in-lists": int(off[REVERSED]) + k5 + 2}
    for what, u in rows.items():
        for pp in (0.0, 0.5):
            c = _Case("reform_egonets", 16, 8, True, pp, fwd_npw, keep_row=u)
            on = _both_routes(c, None, f"one-hot on the {what} (node {u}), attention dropout {pp}")
            assert bool((on["d_attn_l"][:6] != 0).any()), what          # (the row's da is not zero: the partials carry the row)


def test_a_row_of_y_that_is_not_finite():
    """Inf in the Y row of a parent and of a sibling: X' holds Inf / NaN there, and both routes leave the same non-finite pattern"""
    b = _batch("reform_egonets")
    off = b["graph_off"]
    rows = (int(off[3]) + 1, int(off[3]) + b["shapes"][3][0] + 3)
    for fwd_npw in (8, 4):
        c = _Case("reform_egonets", 16, 8, True, 0.1, fwd_npw, inf_rows=rows)
        assert not bool(torch.isfinite(c.st.X[rows[0], :64]).all())
        on = _both_routes(c, c.plan(), f"Inf in Y, forward {fwd_npw}")
        assert not bool(torch.isfinite(on["d_Y"][:, :72]).all())


def test_an_ineligible_call_takes_the_loading_walk():
    """two heads: no egonet walk at all, the bit changes nothing (names, work figure, bits).  Rows stored DROPPED by the forward (its
    NX == 3 form): the caller sets TXE_WALK_NO_REFORM, the launch names stay, the work figure is the loading walk's -- and the call without
    the bit, which takes the stored rows for the plain ones, gives other numbers: the bit is what keeps such a call right"""
    from taxoexpan_amd import _lib
    c = _Case("reform_egonets", 32, 8, True, 0.1, 4, Hp=2)
    a, ra = c.run()
    o, ro = c.run(_lib.WALK_NO_REFORM)
    assert [r[0] for r in ra] == [r[0] for r in ro] == fl.fused_launches(c.inp["Kp"], True, 2, 32)
    assert _sweep_work(ra) == _sweep_work(ro)
    _same_bits(a, o, "two heads")
    c = _Case("reform_egonets", 16, 8, True, 0.1, 4, dropped=True)
    plain = _Case("reform_egonets", 16, 8, True, 0.1, 4)
    assert not torch.equal(_bits(c.st.X), _bits(plain.st.X))
    o, ro = c.run(_lib.WALK_NO_REFORM)
    _r, rp = plain.run(_lib.WALK_NO_REFORM)
    assert [r[0] for r in ro] == [r[0] for r in rp] == fl.fused_launches(c.inp["Kp"], True, 4, 16)
    assert _sweep_work(ro) == _sweep_work(rp)
    a, ra = c.run()
    assert [r[0] for r in ra] == [r[0] for r in ro] and _sweep_work(ro) - _sweep_work(ra) == c.x_skipped_bytes
    assert not torch.equal(_bits(a["workspace"]), _bits(o["workspace"]))


def test_the_stack_takes_the_reforming_route_and_keeps_its_bits():
    """GATStackFunction (heads 4 -> 1, folded output layer, an activation between): ops.ROUTES['bwd_walk'] is 'reform' by default and
    'load' under ops._NO_REFORM_X / 'edges' under ops._NO_EGO_WALK; the launches and the hash of every output and gradient are the same
    on the first two"""
    from taxoexpan_amd import ops
    from test_gpu_stack_frame import HID, OUT, _stack
    # (a whole run on another route of the suite: no fused backward -> no note at all; no egonet walk -> 'edges' throughout)
    want = lambda route: None if ops._NO_FUSED_BWD else ("edges" if ops._NO_EGO_WALK else route)
    ops.ROUTES.pop("bwd_walk", None)
    on = _stack("gat", "collapse", [4, 1], [HID, OUT], pw=True)
    assert ops.ROUTES.get("bwd_walk") == want("reform")
    off = _stack("gat", "collapse", [4, 1], [HID, OUT], pw=True, switches=("_NO_REFORM_X",))
    assert ops.ROUTES.get("bwd_walk") == want("load")
    assert on == off
    _stack("gat", "collapse", [4, 1], [HID, OUT], pw=True, switches=("_NO_EGO_WALK",))
    assert ops.ROUTES.get("bwd_walk") == want("edges")
