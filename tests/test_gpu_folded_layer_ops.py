"""The output layer folded behind the mean readouts (csrc/txe_fold.hip, csrc/txe_fold_bwd.hip) against FLOAT64, entry point by entry point,
through the C ABI (_lib.call with _lib.GraphBatch, GatFoldLayer, FoldMatch, GatFoldGrads, GatFoldBelow, GcnFoldLayer, GcnFoldGrads: the
test owns X [N][Kp], every stride and every workspace), at every edge of the host-side dispatch.

Reference: tests/folded_layer_ref.py -- gat_fold, below_then_fold, gcn_fold restated from oracle/txe_oracle.py's primitives
(tests/test_folded_layer_ref_cpu.py holds them to orc.gat_layer / orc.pgat_forward / orc.gcn_layer + readout) -- in float64 on the CPU,
gradients by autograd; yardstick: the same function in fp32 on the CPU; gate: golden_util.gate_against_f64 with its defaults, once per
tensor per case.  Every gate prints "[gate] operator what device-error yardstick-error" (fractions of the tensor's largest float64
entry).  d_attn_r and d_a2 are judged with scale_floor = the largest entry of d_attn_l / d_a1 (a constant added to every in-edge of a
destination moves its softmax only through the leaky_relu's two slopes: the tensor is nearly zero on its own scale).

Inputs: X, the projections' outputs and every gradient seed standard normal; W / sqrt(Kt), attn_l and attn_r / sqrt(D) (the logits are
O(1), as with the model's Xavier initialisation: a saturated softmax would hide alpha behind 0 and 1).  Wp comes from txe_gat_pack_weights /
txe_gcn_pack_weights into a NaN-filled buffer, feature masks from txe_dropout_mask (read back and compared with rng.keep_mask_bits),
attention dropout is rng.keep_mask(seed, (E, H), p) in destination-CSR order.  The state a BACKWARD case reads (a12, alpha, coef, wsum,
gid, Z, hg, alpha_p, X') is the float64 forward's, rounded to fp32 and uploaded: every backward operator stands alone.  Leaky branches
are given to the reference as the kernels read them (the sign of the fp32 sum a1[u] + a2[v] of the stored a12; the sign of the stored
X') and audited: a given branch may differ from the float64 sign only where |x| <= 1e-4 of the largest, on at most 1e-3 numel + 1 entries.

NaN poisoning: the workspace is NaN before every call; outputs live in NaN-filled buffers (hg with ld_hg = D + 3, d_Yp with n_pad 0
and 2 and NaN columns behind them, a NaN guard behind every dense output): everything outside the view stays NaN, the documented zero
padding is zero.  EMPTY graphs are left out of the float64 comparison (a mean over no nodes has no value); their rows are pinned to what
the code defines: wsum 0, a zero row of Z, a zero row of hg for GAT, the bias for GCN (zero without one).

Batches (folded_layer_ref.py): A = the 15 egonets of the readout test (992 nodes; G < 16: the per-graph Z sweep; 785 nodes in the second
8-graph workgroup, past the 512 LDS-staged readout weights); B = 43 graphs of 0..16 nodes (the chunked Z sweep, a last chunk of three,
three empty graphs, one not hub-shaped); C = the generic batch of test_fused_backward_sweep_equals_unfused_chain plus a 300-node
circulant graph (every node heavy on both sides: the 256-entry heavy lists overflow); E = C with 45 empty graphs in a row.

Instance -> case (each case asserts ITS launch names through the library profiler; folded_layer_ref.py holds the arithmetic,
test_folded_layer_ref_cpu.py that the tables reach every instance):
    cl_logits_kernel<M>, cl_zsum_kernel<M> (A, C), cl_zsum_chunk_kernel<M, false> (B)       test_gat_fold_forward (fl.FWD_CASES)
    cl_zsum_chunk_kernel<M, true>, cl_fold_score_kernel                                     test_folded_matcher_rides_along (B)
    cl_bwd_dot_kernel<M> (Kp 32, 256, 2592), cl_bwd_dot_row_kernel<M, 5 | 9 | 10> (288, 1280 | 1312, 2304 | 2336, 2560),
    cl_bwd_dx_kernel<M, true>                                                               test_gat_fold_backward (fl.BWD_CASES)
    gat_fused_bwd_kernel<M, NI 1..4, NWH 1 | 2 | 4>, gat_fused_bwd_ego_kernel<M, NI 1..4>,
    gat_attn_bwd_reduce_a_kernel                                                            test_fused_backward (fl.FUSED_CASES)
    egonet_walk_plan_kernel, the phase flags, TXE_PH_DEFER, DW_BESIDE, DZ_GIVEN             test_fused_backward_routes_are_one_result
    cl_bwd_dx_kernel<M, false>, cl_zsum_* and cl_bwd_dot_* through the GCN entry points     test_gcn_fold (fl.GCN_CASES)

Measured on the MI355X, largest device error / yardstick error per operator over all cases of this file, and the largest device error
itself (fractions of the tensor's largest float64 entry; the gate's floor is 2e-5, and every ratio above 2 is of a tensor under it):
    txe_gat_collapse_fwd            2.5  (hg on B with attention dropout, 4.3e-7 against 1.7e-7); largest 2.8e-6 (wsum with the readout
                                         test's PW: log1pf(__expf(x)))
    txe_gat_collapse_bwd            4.6  (d_pw on A, masked, 4.8e-7 against 1.1e-7); largest 4.6e-6 (d_pw on A, masked)
    txe_gat_collapse_bwd_fused      3.8  (d_attn_r, unmasked, 1.6e-7 against 4.1e-8); largest 3.8e-6 (d_pw on B)
    txe_gat_collapse_fold_scores    1.7  (with e_part; scores without exp, 1.6e-7 against 9.0e-8: the largest device error of the two)
    txe_gcn_collapse_fwd / _bwd     2.1  (hg on A, masked, 1.1e-6 against 5.0e-7); largest 2.0e-6 (Z on A)
    TXE_FOLD_HG_SPLIT               hg 2.9 x the plain device product's error (8.2e-7 against 2.8e-7 on B); largest 1.0e-6 (A)
No case needed a scale_floor beyond the one d_attn_r / d_a2 get.  The 120 cases take 12 to 13 s on the MI355X, most of it the CPU references;
the slowest cases, test_fused_backward_against_float64 at its widest rows (H4-D772-P50-A, H4-D1024-P0-A), 0.4 s.
"""
import ctypes

import numpy as np
import pytest
import torch

import folded_layer_ref as fl
import message_passing_ref as mp
import txe_oracle as orc
from golden_util import gate_against_f64
from test_gpu_message_passing_ops import _mask_bits
from test_gpu_readout_match_ops import _profiled

pytestmark = pytest.mark.gpu

ATTN_SLOPE, ACT_SLOPE, SEED, VOCAB = 0.2, 0.01, 4242, 3
NAN = float("nan")
KERNELS = ("cl_", "gat_fused_bwd", "gat_attn_bwd_reduce_a", "egonet_walk_plan")      # the launches this file names (the GEMMs are not its subject)


def _dev():
    return torch.device("cuda:0")


def _gate(op, items):
    """items: (what, device, float64, fp32 yardstick[, scale_floor]) -- all gated with the defaults, the whole case's figures printed,
    then one assertion"""
    errors, report = [], []
    for it in items:
        what, got, ref64, yard = it[:4]
        gate_against_f64(got, ref64, yard, what, errors, report=report, scale_floor=it[4] if len(it) > 4 else 0.0)
    for what, e_dev, e_yard in report:
        print(f"[gate] {op} {what} {e_dev:.3e} {e_yard:.3e}")
    assert not errors, (op, errors, report)


def _audit(fn):
    """fn() with the oracle's branch audit on; the project's rule for given branches, then fn's result"""
    out, audit = fl.audited(fn)
    fl.audit_rule(audit)
    return out


# ---- batches on the device ------------------------------------------------------------------------------------------------------------------
_BATCHES = {}


def _batch(name):
    if name not in _BATCHES:
        from taxoexpan_amd import _lib
        from taxoexpan_amd.graph import DGLGraph, batch
        b = dict(fl.batch(name))
        graphs = []
        for n, s, d in b["graphs"]:
            g = DGLGraph()
            g.add_nodes(n)
            g.add_edges(s, d)
            graphs.append(g)
        bg = batch(graphs)
        csr = bg.csr(_dev(), method="host")
        sc, dc = mp.in_csr_order(b["src"], b["dst"])
        assert csr.n_nodes == b["n"] and csr.n_edges == len(sc) and csr.n_graphs == b["G"]
        assert np.array_equal(csr.col_src.cpu().numpy(), sc) and np.array_equal(csr.graph_off.cpu().numpy(), b["graph_off"])
        b.update(csr=csr, E=len(sc), s=torch.from_numpy(sc), d=torch.from_numpy(dc), goff=torch.from_numpy(b["graph_off"]),
                 post=torch.from_numpy(b["pos"]), posd=torch.from_numpy(b["pos"].astype(np.int32)).to(_dev()),
                 gid=np.repeat(np.arange(b["G"]), b["sizes"]).astype(np.int32), live=b["sizes"] > 0,
                 gb=_lib.GraphBatch(rowptr_in=csr.rowptr_in.data_ptr(), col_src=csr.col_src.data_ptr(), rowptr_out=csr.rowptr_out.data_ptr(),
                                    col_dst=csr.col_dst.data_ptr(), pos_out=csr.pos_out.data_ptr(), graph_off=csr.graph_off.data_ptr(),
                                    n_nodes=b["n"], n_edges=len(sc), G=b["G"]))
        _BATCHES[name] = b
    return _BATCHES[name]


# ---- device buffers ---------------------------------------------------------------------------------------------------------------------------
def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _nan(*shape):
    return torch.full(shape, NAN, device=_dev())


def _guarded(numel):
    """a dense output of `numel` floats with one NaN guard behind it"""
    return _nan(max(numel, 1) + 1)


def _take(buf, *shape):
    """the dense output as numpy; its guard (and nothing of the view) is still NaN"""
    numel = int(np.prod(shape))
    a = buf.cpu().numpy()
    assert np.isnan(a[numel:]).all() and np.isfinite(a[:numel]).all(), shape
    return a[:numel].reshape(shape)


def _ws(nbytes):
    return _nan(nbytes // 4 + 64)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _named(names):
    return [k for k in names if k.startswith(KERNELS)]


def _keep_attn(E, H, p, seed):
    from taxoexpan_amd import rng
    return rng.keep_mask(seed, (E, H), p) if p > 0 else None


def _t(a, dtype, grad=False):
    return None if a is None else torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(grad)


def _padded(a, Kp):
    out = np.zeros((a.shape[0], Kp), dtype=np.float32)
    out[:, :a.shape[1]] = a
    return out


def _np(t):
    return t.detach().numpy()


def _behind_activation(hl, h32):
    """the stored activated rows h32 as the output of the leaky_relu (ACT_SLOPE) below the folded layer: the VALUES are hl's -- exactly the
    numbers the device reads -- and the gradient with respect to hl is the one with respect to the pre-activation (the given branch's
    slope, the sign of the stored entry)"""
    a = orc._leaky(hl, ACT_SLOPE, torch.from_numpy(h32 > 0), tag="activation below the folded layer")
    return hl.detach() + (a - a.detach())


# ---- the folded GAT layer: inputs, reference, device calls -----------------------------------------------------------------------------------
def _gat_inputs(bname, Kh, Pd, D, seed):
    b = _batch(bname)
    rs = np.random.RandomState(seed)
    Kt = Kh + Pd
    f = lambda *s: rs.standard_normal(s).astype(np.float32)
    inp = dict(h=f(b["n"], Kh), P=f(VOCAB, Pd), W=f(D, Kt) / np.float32(np.sqrt(Kt)), al=f(D) / np.float32(np.sqrt(D)), ar=f(D) / np.float32(np.sqrt(D)),
               w=f(b["G"], D), Kh=Kh, Pd=Pd, D=D, Kt=Kt, Kp=fl.padded_k(Kh, Pd))
    inp["X"] = _padded(np.concatenate([inp["h"], inp["P"][b["pos"]]], 1), inp["Kp"])
    return inp


def _pack_gat(inp):
    from taxoexpan_amd import _lib
    D, Kt, Kp = inp["D"], inp["Kt"], inp["Kp"]
    Fp = _lib.call("txe_gat_padded_f", 1, D)
    Wd, ald, ard = _up(inp["W"]), _up(inp["al"]), _up(inp["ar"])
    Wp = _nan(Fp, Kp)
    _lib.call("txe_gat_pack_weights", Wd.data_ptr(), ald.data_ptr(), ard.data_ptr(), 1, D, Kt, Wp.data_ptr(), _lib.stream_ptr())
    wp = Wp.cpu().numpy()
    assert np.array_equal(wp[:D, :Kt], inp["W"]) and not wp[:, Kt:].any() and not wp[D + 2:].any()       # the documented zero padding
    return dict(Wp=Wp, W=Wd, al=ald, ar=ard)


def _gat_ref(dtype, b, inp, keep, p, akeep, ap, pw, e_pos=None, a12=None, act_on=False, w=None, dZ=None):
    """gat_fold in `dtype` on X = [act(h) | P[pos]]: (its dict as numpy, gradients under (hg * w).sum() -- or (Z * dZ).sum() -- or None).
    act_on: the first Kh columns are the output of a leaky_relu (ACT_SLOPE) with the branches of the stored X; d_X is then the gradient
    with respect to its pre-activation."""
    Kh, Pd, Kt = inp["Kh"], inp["Pd"], inp["Kt"]
    grad = w is not None or dZ is not None
    hl = _t(inp["h"], dtype, grad)
    P, W, al, ar, pwt = (_t(a, dtype, grad) for a in (inp["P"], inp["W"], inp["al"], inp["ar"], pw))
    hh = _behind_activation(hl, inp["h"]) if act_on else hl
    Pp = P[b["post"]]
    if grad:
        Pp.retain_grad()
    X = torch.cat((hh, Pp), 1)
    r = fl.gat_fold(X, _t(keep[:, :Kt], dtype) if keep is not None else None, 1.0 / (1.0 - p), W, al, ar, b["s"], b["d"], b["goff"], b["post"], pwt,
                    ATTN_SLOPE, _t(akeep[:, 0], dtype) if akeep is not None else None, 1.0 / (1.0 - ap), e_pos, _t(a12, dtype))
    g = None
    if grad:
        ((r["hg"] * _t(w, dtype)).sum() if dZ is None else (r["Z"] * _t(dZ, dtype)).sum()).backward()
        zero = lambda t_: _np(t_.grad) if t_.grad is not None else np.zeros(tuple(t_.shape))
        g = dict(d_X=np.concatenate([zero(hl), zero(Pp)], 1), dW=zero(W), d_attn_l=zero(al), d_attn_r=zero(ar), dP=zero(P),
                 d_pw=zero(pwt).reshape(-1) if pw is not None else None)
    return {k: _np(v) for k, v in r.items()}, g


def _branches(b, a12_32):
    """the folded layer's leaky branches as its kernels read them: the sign of the fp32 sum a1[u] + a2[v] of the stored fp32 logits"""
    a = np.asarray(a12_32, dtype=np.float32)
    return (a[b["s"].numpy(), 0] + a[b["d"].numpy(), 1] > 0).astype(np.int32)


class _FoldState:
    """the device side of one folded GAT layer: inputs, the buffers forward writes (NaN-filled) or the uploaded float64 state, the struct"""

    def __init__(self, b, inp, packed, mask, p, pw, ap, a12=None, state=None, want_hg=True):
        from taxoexpan_amd import _lib
        n, E, G, D, Kp = b["n"], b["E"], b["G"], inp["D"], inp["Kp"]
        self.b, self.inp, self.n, self.E, self.G, self.D, self.Kp = b, inp, n, E, G, D, Kp
        self.X, self.packed, self.mask = _up(inp["X"]) if n else _nan(1, Kp), packed, mask
        self.pw = _up(pw) if pw is not None else None
        self.a12, self.alpha, self.coef, self.wsum, self.Z = _guarded(2 * n), _guarded(E), _guarded(n), _guarded(G), _guarded(G * Kp)
        self.gid = torch.full((max(n, 1) + 1,), -7, dtype=torch.int32, device=_dev())
        self.hgb = _nan(max(G, 1), D + 3)
        if a12 is not None:
            self.a12[:2 * n] = _up(a12.astype(np.float32).reshape(-1))
        if state is not None:                      # the float64 forward, rounded to fp32
            for name, numel in (("a12", 2 * n), ("alpha", E), ("coef", n), ("wsum", G)):
                getattr(self, name)[:numel] = _up(state[name].astype(np.float32).reshape(-1))
            self.Z[:G * Kp] = _up(_padded(state["Z"].astype(np.float32), Kp).reshape(-1))
            self.hgb[:G, :D] = _up(state["hg"].astype(np.float32))
            self.gid[:n] = _up(b["gid"])
        self.layer = _lib.GatFoldLayer(X=self.X.data_ptr(), Kh=inp["Kh"], Pd=inp["Pd"], pos=b["posd"].data_ptr(), vocab=VOCAB, Wp=packed["Wp"].data_ptr(),
                                       W=packed["W"].data_ptr(), attn_l=packed["al"].data_ptr(), attn_r=packed["ar"].data_ptr(), D=D, feat_drop_p=p,
                                       mask=_ptr(mask), attn_slope=ATTN_SLOPE, attn_drop_p=ap, seed=SEED + 1, pw=_ptr(self.pw), a12=self.a12.data_ptr(),
                                       alpha=self.alpha.data_ptr(), coef=self.coef.data_ptr(), wsum=self.wsum.data_ptr(), gid=self.gid.data_ptr(),
                                       Z=self.Z.data_ptr(), hg=self.hgb.data_ptr() if want_hg else None, ld_hg=D + 3)

    def forward(self, flags=0, match=None, split=False):
        from taxoexpan_amd import _lib
        inp = self.inp
        wsb = _lib.call("txe_gat_collapse_ws_bytes", self.n, self.E, self.G, inp["Kh"], inp["Pd"], self.D, VOCAB)
        if split:
            wsb += _lib.call("txe_gat_collapse_split_ws_bytes", self.G, inp["Kh"], inp["Pd"], self.D)
        ws = _ws(wsb)
        _rc, names = _profiled(lambda: _lib.call("txe_gat_collapse_fwd", _lib.ref(self.b["gb"]), _lib.ref(self.layer), _lib.ref(match), flags, ws.data_ptr(),
                                                 wsb, _lib.stream_ptr()))
        return _named(names)

    def outputs(self, with_hg=True):
        """what forward wrote, as numpy: guards and everything outside the views still NaN, gid exact, the zero padding of Z zero"""
        n, E, G, D, Kp, Kt = self.n, self.E, self.G, self.D, self.Kp, self.inp["Kt"]
        out = dict(a12=_take(self.a12, n, 2), alpha=_take(self.alpha, E), coef=_take(self.coef, n), wsum=_take(self.wsum, G), Z=_take(self.Z, G, Kp))
        gid = self.gid.cpu().numpy()
        assert np.array_equal(gid[:n], self.b["gid"]) and gid[n] == -7
        assert not out["Z"][:, Kt:].any()
        hgb = self.hgb.cpu().numpy()
        if with_hg:
            assert np.isfinite(hgb[:G, :D]).all() and np.isnan(hgb[:, D:]).all() and np.isnan(hgb[G:]).all()
            out["hg"] = hgb[:G, :D]
        else:
            assert np.isnan(hgb).all()
        return out


def _forward_items(tag, b, out, r64, r32, Kt, keys=("a12", "alpha", "wsum", "Z", "hg")):
    """the gate's items of one forward run; the rows of EMPTY graphs pinned to what the code defines and left out of the comparison"""
    live = b["live"]
    items = []
    for k in keys:
        got, a64, a32 = out[k], r64[k], r32[k]
        if k == "Z":
            got = got[:, :Kt]
        if k in ("wsum", "Z", "hg"):
            assert not got[~live].any(), (tag, k)                                     # an empty graph: wsum 0, zero rows of Z and hg
            got, a64, a32 = got[live], a64[live], a32[live]
        items.append((f"{k} [{tag}]", got, a64, a32))
    return items


# ---- 2a. txe_gat_collapse_fwd --------------------------------------------------------------------------------------------------------------------
def _fwd_D(Kp, bname):
    return 250 if Kp <= 320 and bname != "C" else 6         # (the widest rows keep D = 6: the CPU reference, not the width under test, sets the time)


@pytest.mark.parametrize("Kh,Pd,bname", fl.FWD_CASES, ids=[f"Kp{fl.padded_k(c[0], c[1])}-{c[2]}" for c in fl.FWD_CASES])
def test_gat_fold_forward_against_float64(Kh, Pd, bname):
    """a12, alpha, wsum, Z, hg with and without the feature mask (p = 0.3), WeightedMeanReadout with the model's kind of weights; gid exact"""
    b = _batch(bname)
    D = _fwd_D(fl.padded_k(Kh, Pd), bname)
    inp = _gat_inputs(bname, Kh, Pd, D, 100 + Kh + Pd)
    packed = _pack_gat(inp)
    pw = np.array([[0.3], [-0.2], [0.5]], dtype=np.float32)
    items = []
    for masked in fl.MASKS:
        p = 0.3 if masked else 0.0
        mask, keep = _mask_bits(b["n"], inp["Kp"], p, SEED) if masked else (None, None)
        st = _FoldState(b, inp, packed, mask, p, pw, 0.0)
        names = st.forward()
        assert names == fl.fwd_launches(b["n"], b["G"], masked), names
        out = st.outputs()
        r64, _g = _gat_ref(torch.float64, b, inp, keep, p, None, 0.0, pw)
        r32, _g = _gat_ref(torch.float32, b, inp, keep, p, None, 0.0, pw)
        items += _forward_items(f"mask {int(masked)}", b, out, r64, r32, inp["Kt"])
    _gate("gat_collapse_fwd", items)


@pytest.mark.parametrize("option", ["mean_readout", "pw_softplus_branch", "attn_drop", "a12_ready", "hg_split", "z_only"])
@pytest.mark.parametrize("Kp", fl.FWD_OPTION_WIDTHS)
def test_gat_fold_forward_options_against_float64(Kp, option):
    """one option each, at three widths, on A and B: pw NULL (MeanReadout); the readout test's PW (class 0 on the x > 20 branch of
    softplus); attention dropout 0.2; TXE_FOLD_A12_READY with test-supplied logits whose softmax spans more than 180 at one destination
    (__expf without the running maximum would overflow); TXE_FOLD_HG_SPLIT (hg on the bf16 pipe, gated against float64 like the plain
    product and, with the plain device product of the same inputs as the yardstick, against that); hg NULL (forward stops at Z: the hg buffer keeps its NaN)"""
    from taxoexpan_amd import _lib
    Kh, Pd = next((a, c) for a, c, kp in fl.FWD_WIDTHS if kp == Kp)
    items = []
    for bname in ("A", "B"):
        b = _batch(bname)
        inp = _gat_inputs(bname, Kh, Pd, 6, 200 + Kp)
        packed = _pack_gat(inp)
        mask, keep = _mask_bits(b["n"], Kp, 0.3, SEED)
        pw = {"mean_readout": None, "pw_softplus_branch": fl.PW}.get(option, np.array([[0.3], [-0.2], [0.5]], dtype=np.float32))
        ap = 0.2 if option == "attn_drop" else 0.0
        akeep = _keep_attn(b["E"], 1, ap, SEED + 1)
        a12 = None
        if option == "a12_ready":
            a12 = np.random.RandomState(Kp).standard_normal((b["n"], 2)).astype(np.float32)
            v = fl.widen_fold_logits(b, a12)
        st = _FoldState(b, inp, packed, mask, 0.3, pw, ap, a12=a12, want_hg=option != "z_only")
        names = st.forward(flags=(_lib.FOLD_A12_READY if a12 is not None else 0) | (_lib.FOLD_HG_SPLIT if option == "hg_split" else 0),
                           split=option == "hg_split")
        assert names == fl.fwd_launches(b["n"], b["G"], True, a12_ready=a12 is not None), names
        out = st.outputs(with_hg=option != "z_only")
        r64, _g = _gat_ref(torch.float64, b, inp, keep, 0.3, akeep, ap, pw, a12=a12)
        r32, _g = _gat_ref(torch.float32, b, inp, keep, 0.3, akeep, ap, pw, a12=a12)
        if a12 is not None:
            assert np.array_equal(out["a12"], a12)                                 # given logits: read, never written
            e = orc._leaky(torch.from_numpy(a12[b["s"].numpy(), 0] + a12[b["d"].numpy(), 1]), ATTN_SLOPE).numpy()[b["d"].numpy() == v]
            assert e.max() - e.min() > 180.0
        keys = ("a12", "alpha", "wsum", "Z") + (("hg",) if option != "z_only" else ())
        items += _forward_items(f"{bname} {option}", b, out, r64, r32, inp["Kt"], keys)
        if option == "hg_split":
            # against the plain product: the same call without the flag; the bf16 route is held to the gate with the PLAIN DEVICE product
            # as its yardstick (no further from float64 than twice the fp32 MFMA route, floor 2e-5), and everything in front of hg is bit-equal
            plain = _FoldState(b, inp, packed, mask, 0.3, pw, ap)
            assert plain.forward() == names
            po = plain.outputs()
            for k in ("a12", "alpha", "coef", "wsum", "Z"):
                assert np.array_equal(po[k], out[k]), k
            live = b["live"]
            items.append((f"hg, split against plain [{bname}]", out["hg"][live], r64["hg"][live], po["hg"][live]))
            items.append((f"hg, plain [{bname}]", po["hg"][live], r64["hg"][live], r32["hg"][live]))
            small = _FoldState(b, inp, packed, mask, 0.3, pw, ap)
            with pytest.raises(_lib.TxeError, match="TXE_ERR_WORKSPACE"):              # the route is the caller's choice, not the buffer's size:
                small.forward(flags=_lib.FOLD_HG_SPLIT, split=False)                   # rejected before any launch
            torch.cuda.synchronize()
            for t in (small.a12, small.alpha, small.coef, small.wsum, small.Z, small.hgb):
                assert bool(torch.isnan(t).all())
    _gate(f"gat_collapse_fwd[{option}]", items)


def test_z_rows_do_not_depend_on_the_sweep_that_forms_them():
    """the first 15 graphs of B as a batch of their own (G < 16: cl_zsum_kernel, a wave per graph and tile) give the rows of Z they have
    in the 43-graph batch (cl_zsum_chunk_kernel, a wave per chunk of four graphs), bit for bit: per graph the same nodes in the same order"""
    Kh, Pd = 1000, 24
    big, small = _batch("B"), _batch("B15")
    inp = _gat_inputs("B", Kh, Pd, 6, 300)
    packed = _pack_gat(inp)
    n15 = small["n"]
    mask, _keep = _mask_bits(big["n"], inp["Kp"], 0.3, SEED)
    inp15 = dict(inp, X=inp["X"][:n15], h=inp["h"][:n15], w=inp["w"][:15])
    pw = fl.PW
    st, st15 = _FoldState(big, inp, packed, mask, 0.3, pw, 0.0), _FoldState(small, inp15, packed, mask[:n15].contiguous(), 0.3, pw, 0.0)
    assert st.forward() == ["cl_logits_kernel<true>", "cl_zsum_chunk_kernel<true, false>"]
    assert st15.forward() == ["cl_logits_kernel<true>", "cl_zsum_kernel<true>"]
    out, out15 = st.outputs(), st15.outputs()
    assert np.abs(out15["Z"]).max() > 0
    for k in ("a12", "alpha", "coef"):
        assert np.array_equal(out15[k], out[k][:len(out15[k])]), k
    assert np.array_equal(out15["wsum"], out["wsum"][:15]) and np.array_equal(out15["Z"], out["Z"][:15])


@pytest.mark.parametrize("n_graphs", [3, 0])
def test_gat_fold_forward_of_an_empty_batch(n_graphs):
    """N = 0 with G = 3 (the cl_wsum_kernel route: wsum 0, zero rows of Z and hg) and G = 0 (nothing launched): TXE_OK"""
    from taxoexpan_amd import _lib
    Kh, Pd, D, Kp = 250, 6, 6, 256
    zeros = torch.zeros(8, dtype=torch.int32, device=_dev())
    b = dict(n=0, E=0, G=n_graphs, posd=zeros, gid=np.zeros(0, np.int32),
             gb=_lib.GraphBatch(rowptr_in=zeros.data_ptr(), col_src=zeros.data_ptr(), rowptr_out=zeros.data_ptr(), col_dst=zeros.data_ptr(),
                                pos_out=zeros.data_ptr(), graph_off=zeros.data_ptr(), n_nodes=0, n_edges=0, G=n_graphs))
    rs = np.random.RandomState(1)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)
    inp = dict(X=np.zeros((0, Kp), np.float32), W=f(D, Kh + Pd), al=f(D), ar=f(D), Kh=Kh, Pd=Pd, D=D, Kt=Kh + Pd, Kp=Kp)
    st = _FoldState(b, inp, _pack_gat(inp), None, 0.0, fl.PW, 0.0)
    names = st.forward()
    assert names == (["cl_zsum_kernel<false>"] if n_graphs else []), names
    if n_graphs:
        out = st.outputs()
        assert not out["wsum"].any() and not out["Z"].any() and not out["hg"].any()
    else:
        for t in (st.a12, st.alpha, st.coef, st.wsum, st.Z, st.hgb):
            assert bool(torch.isnan(t).all())


# ---- 2b. txe_gat_collapse_bwd --------------------------------------------------------------------------------------------------------------------
def _grad_buffers(inp, pw):
    from taxoexpan_amd import _lib
    D, Kt, Pd = inp["D"], inp["Kt"], inp["Pd"]
    bufs = dict(dW=_guarded(D * Kt), d_attn_l=_guarded(D), d_attn_r=_guarded(D), dP=_guarded(VOCAB * Pd) if Pd else None,
                d_pw=_guarded(VOCAB) if pw is not None else None)
    return bufs, _lib.GatFoldGrads(**{k: _ptr(v) for k, v in bufs.items()})


def _param_grads(bufs, inp):
    D, Kt, Pd = inp["D"], inp["Kt"], inp["Pd"]
    out = dict(dW=_take(bufs["dW"], D, Kt), d_attn_l=_take(bufs["d_attn_l"], D), d_attn_r=_take(bufs["d_attn_r"], D))
    if bufs["dP"] is not None:
        out["dP"] = _take(bufs["dP"], VOCAB, Pd)
    if bufs["d_pw"] is not None:
        out["d_pw"] = _take(bufs["d_pw"], VOCAB)
    return out


def _param_items(tag, got, g64, g32):
    floor = float(np.abs(g64["d_attn_l"]).max())
    return [(f"{k} [{tag}]", got[k], g64[k], g32[k]) + ((floor,) if k == "d_attn_r" else ()) for k in ("dW", "d_attn_l", "d_attn_r", "dP", "d_pw") if k in got]


def _gat_backward_case(bname, Kh, Pd, masked, option=None):
    from taxoexpan_amd import _lib
    b = _batch(bname)
    n, E, G, D = b["n"], b["E"], b["G"], 6
    inp = _gat_inputs(bname, Kh, Pd, D, 400 + Kh + Pd)
    Kt, Kp = inp["Kt"], inp["Kp"]
    packed = _pack_gat(inp)
    p = 0.3 if masked else 0.0
    mask, keep = _mask_bits(n, Kp, p, SEED) if masked else (None, None)
    pw = None if option == "pw_none" else np.array([[0.3], [-0.2], [0.5]], dtype=np.float32)
    ap = 0.2 if option == "attn_drop" else 0.0
    akeep = _keep_attn(E, 1, ap, SEED + 1)
    act_on = option == "act_on"
    f64, _g = _gat_ref(torch.float64, b, inp, keep, p, akeep, ap, pw, act_on=act_on)
    e_pos = _branches(b, f64["a12"].astype(np.float32))
    r64, g64 = _audit(lambda: _gat_ref(torch.float64, b, inp, keep, p, akeep, ap, pw, e_pos=e_pos, act_on=act_on, w=inp["w"]))
    r32, g32 = _gat_ref(torch.float32, b, inp, keep, p, akeep, ap, pw, e_pos=e_pos, act_on=act_on, w=inp["w"])
    st = _FoldState(b, inp, packed, mask, p, pw, ap, state=f64)
    d_hg, d_X = _up(inp["w"]), _guarded(n * Kp)
    bufs, grads = _grad_buffers(inp, pw)
    wsb = _lib.call("txe_gat_collapse_ws_bytes", n, E, G, Kh, Pd, D, VOCAB)
    ws = _ws(wsb)
    _rc, names = _profiled(lambda: _lib.call("txe_gat_collapse_bwd", _lib.ref(b["gb"]), _lib.ref(st.layer), d_hg.data_ptr(), D, int(act_on), ACT_SLOPE,
                                             d_X.data_ptr(), _lib.ref(grads), ws.data_ptr(), wsb, _lib.stream_ptr()))
    assert _named(names) == fl.bwd_launches(Kp, masked), names
    dx = _take(d_X, n, Kp)
    assert not dx[:, Kt:].any()                                                      # the padding columns of d_X: zero
    tag = f"{bname} mask {int(masked)}" + (f" {option}" if option else "")
    return [(f"d_X [{tag}]", dx[:, :Kt], g64["d_X"], g32["d_X"])] + _param_items(tag, _param_grads(bufs, inp), g64, g32)


@pytest.mark.parametrize("Kh,Pd,bname", fl.BWD_CASES, ids=[f"Kp{fl.padded_k(c[0], c[1])}-{c[2]}" for c in fl.BWD_CASES])
def test_gat_fold_backward_against_float64(Kh, Pd, bname):
    """d_X, dW, d_attn_l, d_attn_r, dP, d_pw from the uploaded float64 state, with and without the feature mask"""
    _gate("gat_collapse_bwd", [it for masked in fl.MASKS for it in _gat_backward_case(bname, Kh, Pd, masked)])


@pytest.mark.parametrize("option", ["act_on", "pw_none", "attn_drop"])
def test_gat_fold_backward_options_against_float64(option):
    """one option each at Kp 288 on A: act_on 1 (slope 0.01: d_X's first Kh columns through leaky' of the stored X) beside act_on 0 of the
    plain cases, pw NULL (MeanReadout: no d_pw), attention dropout 0.2"""
    _gate(f"gat_collapse_bwd[{option}]", [it for masked in fl.MASKS for it in _gat_backward_case("A", 250, 38, masked, option)])


# ---- 2c. txe_gat_collapse_bwd_fused -------------------------------------------------------------------------------------------------------------
def _fused_inputs(bname, Hp, Dp, Pd, seed):
    b = _batch(bname)
    n, F_, D = b["n"], Hp * Dp, 6
    Kt = F_ + Pd
    rs = np.random.RandomState(seed)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)
    return dict(ft=f(n, F_), a1=f(n, Hp), a2=f(n, Hp), P=f(VOCAB, Pd), W=f(D, Kt) / np.float32(np.sqrt(Kt)), al=f(D) / np.float32(np.sqrt(D)),
                ar=f(D) / np.float32(np.sqrt(D)), w=f(b["G"], D), Hp=Hp, Dp=Dp, Kh=F_, Pd=Pd, D=D, Kt=Kt, Kp=fl.padded_k(F_, Pd))


def _fused_ref(dtype, b, inp, keep, p, pw, keep_p, pp, act_slope, act_pos=None, e_pos=None, w=None, dZ=None, extra_dW=None):
    """below_then_fold in `dtype`: (fold's dict, X', alpha_p as numpy, gradients under (hg * w).sum() -- or (Z * dZ).sum() with extra_dW
    [D][Kt] added to dW: TXE_FUSED_DZ_GIVEN -- or None)"""
    Hp, Dp, Kt = inp["Hp"], inp["Dp"], inp["Kt"]
    grad = w is not None or dZ is not None
    ft, a1, a2, P, W, al, ar, pwt = (_t(a, dtype, grad) for a in (inp["ft"], inp["a1"], inp["a2"], inp["P"], inp["W"], inp["al"], inp["ar"], pw))
    kt = _t(keep[:, :Kt], dtype) if keep is not None else None
    fold = lambda Xn: fl.gat_fold(Xn, kt, 1.0 / (1.0 - p), W, al, ar, b["s"], b["d"], b["goff"], b["post"], pwt, ATTN_SLOPE, e_pos=e_pos)
    r, Xn, alpha_p = fl.below_then_fold(ft.reshape(b["n"], Hp, Dp), a1, a2, b["s"], b["d"], ATTN_SLOPE, _t(keep_p, dtype), 1.0 / (1.0 - pp), act_slope,
                                        act_pos, P if inp["Pd"] else None, b["post"], fold)
    g = None
    if grad:
        ((r["hg"] * _t(w, dtype)).sum() if dZ is None else (r["Z"] * _t(dZ, dtype)).sum()).backward()
        zero = lambda t_: _np(t_.grad) if t_.grad is not None else np.zeros(tuple(t_.shape))
        g = dict(d_ft=zero(ft), d_a1=zero(a1), d_a2=zero(a2), dW=zero(W) + (extra_dW if extra_dW is not None else 0.0), d_attn_l=zero(al),
                 d_attn_r=zero(ar), dP=zero(P), d_pw=zero(pwt).reshape(-1))
    return {k: _np(v) for k, v in r.items()}, _np(Xn), _np(alpha_p), g


class _Fused:
    """one fused-backward case: inputs, both references, the uploaded float64 state; run() = one backward pass on fresh NaN buffers"""

    def __init__(self, bname, Hp, Dp, Pd, masked, act_slope=ACT_SLOPE, pp=0.0, seed=0, dZ=None, extra_dW=None, match=None):
        from taxoexpan_amd import _lib
        self.b = b = _batch(bname)
        self.inp = inp = _fused_inputs(bname, Hp, Dp, Pd, 500 + 7 * Hp + Dp + Pd + seed)
        n, E, G, F_, Kp = b["n"], b["E"], b["G"], Hp * Dp, inp["Kp"]
        self.p = p = 0.3 if masked else 0.0
        self.mask, keep = _mask_bits(n, Kp, p, SEED) if masked else (None, None)
        self.pw = pw = np.array([[0.3], [-0.2], [0.5]], dtype=np.float32)
        self.pp, self.act_slope, self.masked = pp, act_slope, masked
        keep_p = _keep_attn(E, Hp, pp, SEED + 3)
        f64, X64, ap64, _g = _fused_ref(torch.float64, b, inp, keep, p, pw, keep_p, pp, act_slope)
        X32 = X64.astype(np.float32)
        act_pos, e_pos = (X32[:, :F_] > 0).astype(np.int32), _branches(b, f64["a12"].astype(np.float32))
        if dZ is not None and callable(dZ):
            dZ = dZ(f64)
        self.dZ = dZ
        args = (keep, p, pw, keep_p, pp, act_slope, act_pos, e_pos, None if dZ is not None else inp["w"], dZ, extra_dW)
        _r, _x, _a, self.g64 = _audit(lambda: _fused_ref(torch.float64, b, inp, *args))
        _r, _x, _a, self.g32 = _fused_ref(torch.float32, b, inp, *args)
        self.f64 = f64
        # the device side: Yp = [ft | a1 | a2 | NaN], X' = the float64 forward's rounded to fp32 with its zero padding, alpha_p likewise
        self.ld = ld = (F_ + 2 * Hp + 2 + 3) // 4 * 4 + 4
        Yp = np.full((n, ld), NAN, dtype=np.float32)
        Yp[:, :F_], Yp[:, F_:F_ + Hp], Yp[:, F_ + Hp:F_ + 2 * Hp] = inp["ft"], inp["a1"], inp["a2"]
        self.Yp, self.alpha_p = _up(Yp), _up(ap64.astype(np.float32))
        self.packed = _pack_gat(inp)
        self.st = _FoldState(b, dict(inp, X=_padded(X32, Kp)), self.packed, self.mask, p, pw, 0.0, state=f64)
        self.d_hg = _up(inp["w"]) if dZ is None else _up(_padded(dZ.astype(np.float32), Kp))
        self.wsb = _lib.call("txe_gat_collapse_bwd_fused_ws_bytes", n, E, G, F_, Pd, inp["D"], VOCAB, Hp)
        self.match = match

    def run(self, phase_calls, n_pad=0, plan=None, chain=None, flush=False, dw_main=None, dw_slices=0, ws=None, check=True):
        """one backward pass: txe_gat_collapse_bwd_fused once per entry of phase_calls, all on ONE NaN-primed workspace and one set of
        NaN-filled outputs -> (outputs as numpy, launch names)"""
        from taxoexpan_amd import _lib
        b, inp, st = self.b, self.inp, self.st
        n, E, Hp, Dp, F_ = b["n"], b["E"], inp["Hp"], inp["Dp"], inp["Hp"] * inp["Dp"]
        d_Yp, dz_p = _nan(n, self.ld), _nan(E * Hp + 1)
        bufs, grads = _grad_buffers(inp, self.pw)
        below = _lib.GatFoldBelow(Yp=self.Yp.data_ptr(), ld_yp=self.ld, Hp=Hp, Dp=Dp, attn_slope_p=ATTN_SLOPE, attn_drop_p_p=self.pp, seed_p=SEED + 3,
                                  alpha_p=self.alpha_p.data_ptr(), d_Yp=d_Yp.data_ptr(), ld_dyp=self.ld, n_pad=n_pad, dz_p=dz_p.data_ptr())
        ws = _ws(self.wsb) if ws is None else ws
        given = self.dZ is not None
        ld_dhg = inp["Kp"] if given else inp["D"]

        def calls():
            for ph in phase_calls:
                edot = bool(ph & _lib.FUSED_EDOT)
                _lib.call("txe_gat_collapse_bwd_fused", _lib.ref(b["gb"]), _lib.ref(st.layer), _lib.ref(below), _lib.ref(self.match) if edot else None,
                          _lib.ref(grads), None if edot else self.d_hg.data_ptr(), ld_dhg, self.act_slope, ph, _ptr(dw_main), dw_slices, _ptr(plan), chain,
                          ws.data_ptr(), self.wsb, _lib.stream_ptr())
            if flush:
                _lib.call("txe_gat_tail_flush", chain, _lib.stream_ptr())
        _rc, names = _profiled(calls)
        if not check:
            return None, _named(names)
        dy = d_Yp.cpu().numpy()
        end = F_ + 2 * Hp
        assert np.isfinite(dy[:, :end]).all() and not dy[:, end:end + n_pad].any() and np.isnan(dy[:, end + n_pad:]).all()
        assert bool(torch.isnan(dz_p[-1]))
        out = dict(d_ft=dy[:, :F_], d_a1=dy[:, F_:F_ + Hp], d_a2=dy[:, F_ + Hp:end], **_param_grads(bufs, inp))
        return out, _named(names)

    def items(self, tag, out):
        g64, g32 = self.g64, self.g32
        floor = float(np.abs(g64["d_a1"]).max())
        its = [(f"{k} [{tag}]", out[k], g64[k], g32[k]) + ((floor,) if k == "d_a2" else ()) for k in ("d_ft", "d_a1", "d_a2")]
        return its + _param_items(tag, out, g64, g32)


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("Hp,Dp,Pd,bname,no_ego", fl.FUSED_CASES, ids=[f"H{c[0]}-D{c[1]}-P{c[2]}-{c[3]}" + ("-noego" if c[4] else "") for c in fl.FUSED_CASES])
def test_fused_backward_against_float64(Hp, Dp, Pd, bname, no_ego):
    """d_Yp = [d_ft | d_a1 | d_a2], dW, d_attn_l, d_attn_r, dP, d_pw against autograd of below_then_fold, with and without the feature
    mask; n_pad 0 (unmasked) and 2 (masked); the activation between the layers with slope 0.01"""
    from taxoexpan_amd import _lib
    items = []
    for masked in fl.MASKS:
        c = _Fused(bname, Hp, Dp, Pd, masked)
        out, names = c.run([_lib.FUSED_ALL | (_lib.FUSED_NO_EGO_WALK if no_ego else 0)], n_pad=2 if masked else 0)
        assert names == fl.fused_launches(c.inp["Kp"], masked, Hp, Dp, no_ego), names
        items += c.items(f"mask {int(masked)}", out)
    _gate("gat_collapse_bwd_fused", items)


@pytest.mark.parametrize("bname", ["A", "B"])
def test_fused_backward_routes_are_one_result(bname):
    """(4, 500, 50), masked: with a plan from txe_egonet_walk_plan and without one; run twice; the phases DZ, DW, SWEEP, REDUCE as four
    calls on one NaN-primed workspace; REDUCE | TXE_PH_DEFER with a chain, then txe_gat_tail_flush -- all bit-equal to TXE_FUSED_ALL;
    TXE_FUSED_DW_BESIDE (another split of the weight-gradient product) gated"""
    from taxoexpan_amd import _lib
    L = _lib
    c = _Fused(bname, 4, 500, 50, True)
    b, csr = c.b, c.b["csr"]
    base, names = c.run([L.FUSED_ALL])
    assert names == fl.fused_launches(c.inp["Kp"], True, 4, 500), names
    again, _n = c.run([L.FUSED_ALL])
    _same(base, again, "run twice")
    plan = torch.full((L.call("txe_egonet_walk_plan_bytes", b["n"]) // 4,), -1, dtype=torch.int32, device=_dev())
    _rc, pn = _profiled(lambda: L.call("txe_egonet_walk_plan", csr.rowptr_in.data_ptr(), csr.col_src.data_ptr(), csr.rowptr_out.data_ptr(), csr.col_dst.data_ptr(),
                                       csr.pos_out.data_ptr(), csr.graph_off.data_ptr(), b["n"], b["G"], plan.data_ptr(), L.stream_ptr()))
    assert pn == ["egonet_walk_plan_kernel"], pn
    planned, names_p = c.run([L.FUSED_ALL], plan=plan)
    assert names_p == names
    _same(base, planned, "walk plan")
    phased, names_4 = c.run([L.FUSED_DZ, L.FUSED_DW, L.FUSED_SWEEP, L.FUSED_REDUCE])
    assert names_4 == names
    _same(base, phased, "four phase calls")
    chain = ctypes.create_string_buffer(L.TAIL_CHAIN_BYTES)
    deferred, _n = c.run([L.FUSED_DZ | L.FUSED_DW | L.FUSED_SWEEP, L.FUSED_REDUCE | L.PH_DEFER], chain=ctypes.cast(chain, ctypes.c_void_p), flush=True)
    _same(base, deferred, "deferred final reductions")
    beside, _n = c.run([L.FUSED_ALL | L.FUSED_DW_BESIDE])
    _gate("gat_collapse_bwd_fused[routes]", c.items(f"{bname} all", base) + c.items(f"{bname} dw_beside", beside))


@pytest.mark.parametrize("bname", ["A", "B"])
@pytest.mark.parametrize("option", ["act_slope_1", "attn_drop_below", "dz_given_0", "dz_given_2"])
def test_fused_backward_options_against_float64(bname, option):
    """(4, 500, 50), masked: act_slope 1 (no activation between the layers) beside the 0.01 of the plain cases; attention dropout 0.2 in
    the layer below beside their 0; TXE_FUSED_DZ_GIVEN with dw_slices 0 and 2 -- the reference takes dZ [G][Kp] and the slices as inputs"""
    from taxoexpan_amd import _lib
    L = _lib
    b = _batch(bname)
    Kt, Kp, D = 2050, 2080, 6
    if option.startswith("dz_given"):
        rs = np.random.RandomState(9)
        dZ = rs.standard_normal((b["G"], Kt)).astype(np.float32)
        n_sl = int(option[-1])
        slices = rs.standard_normal((n_sl, D, Kp)).astype(np.float32)
        extra = slices.astype(np.float64).sum(0)[:, :Kt] if n_sl else None
        c = _Fused(bname, 4, 500, 50, True, dZ=dZ, extra_dW=extra)
        out, names = c.run([L.FUSED_ALL | L.FUSED_DZ_GIVEN], dw_main=_up(slices) if n_sl else None, dw_slices=n_sl)
    else:
        c = _Fused(bname, 4, 500, 50, True, act_slope=1.0 if option == "act_slope_1" else ACT_SLOPE, pp=0.2 if option == "attn_drop_below" else 0.0)
        out, names = c.run([L.FUSED_ALL])
    assert names == fl.fused_launches(Kp, True, 4, 500), names
    _gate(f"gat_collapse_bwd_fused[{option}]", c.items(bname, out))


# ---- 2c (TXE_FUSED_EDOT) and 2d: the folded matcher rides along ----------------------------------------------------------------------------------
def _e_part_ref(dtype, Tf, zrow, gid, X, keep, nt):
    """e_part[u][t] = <Tf[zrow[g(u)]], keep X[u]> over the 256 columns of tile t (no dropout scale: the consumers apply it)"""
    prod = torch.from_numpy(Tf[zrow[gid]]).to(dtype) * torch.from_numpy(X).to(dtype) * (torch.from_numpy(keep).to(dtype) if keep is not None else 1.0)
    pad = torch.zeros(prod.shape[0], nt * 256, dtype=dtype)
    pad[:, :prod.shape[1]] = prod
    return pad.reshape(prod.shape[0], nt, 256).sum(-1).numpy()


@pytest.mark.parametrize("masked", fl.MASKS, ids=["plain", "masked"])
@pytest.mark.parametrize("m_exp", [0, 1])
def test_folded_matcher_rides_along(masked, m_exp):
    """on B, (4, 500, 50): txe_gat_collapse_fwd with a FoldMatch (Tf, zrow with repeated rows, e_part; hg NULL) leaves
    <Tf[zrow[g]], keep X[u]> per node and tile; txe_gat_collapse_fold_scores sums the scores [exp] <Z_g, Tf[zrow[g]]> from them (an
    empty graph: raw score 0); txe_gat_collapse_bwd_fused with TXE_FUSED_EDOT runs from (m_ds, m_s, m_exp) and the float64 e_part and is
    gated against the reference run with dZ[g] = dsl_g Tf[zrow[g]], dsl = ds (x s for the exp matcher)"""
    from taxoexpan_amd import _lib
    L = _lib
    Hp, Dp, Pd = 4, 500, 50
    b = _batch("B")
    n, G, Kp, Kt = b["n"], b["G"], 2080, 2050
    nt = L.call("txe_gat_collapse_e_tiles", n, G, Hp * Dp, Pd)
    assert nt == fl.zsum_tiles(Kp)[0] == 9
    rs = np.random.RandomState(77 + m_exp)
    runs = 11
    Tf = _padded((rs.standard_normal((runs, Kt)) / np.sqrt(Kt)).astype(np.float32), Kp)
    zrow = np.sort(rs.randint(0, runs, G)).astype(np.int32)                         # runs of graphs that share a row of Tf
    assert len(set(zrow.tolist())) < G
    ds = rs.standard_normal(G).astype(np.float32)

    def dZ_of(f64):
        raw = (f64["Z"] * Tf[zrow][:, :Kt].astype(np.float64)).sum(1)
        s = np.exp(raw) if m_exp else raw
        dZ_of.s32 = s.astype(np.float32)
        dsl = ds.astype(np.float64) * (dZ_of.s32.astype(np.float64) if m_exp else 1.0)
        return dsl[:, None] * Tf[zrow][:, :Kt].astype(np.float64)
    c = _Fused("B", Hp, Dp, Pd, masked, dZ=dZ_of)
    p, keep = c.p, (_mask_bits(n, Kp, c.p, SEED)[1] if masked else None)
    X32 = c.st.inp["X"]
    Tfd, zrowd = _up(Tf), _up(zrow)
    # ---- forward: Z as without a matcher, e_part beside it ----
    fw = _FoldState(b, c.st.inp, c.packed, c.mask, p, c.pw, 0.0, want_hg=False)
    e_part = _guarded(n * nt)
    m_fwd = L.FoldMatch(e_part=e_part.data_ptr(), Tf=Tfd.data_ptr(), zrow=zrowd.data_ptr())
    names = fw.forward(match=m_fwd)
    assert names == fl.fwd_launches(n, G, masked, edot=True), names
    out = fw.outputs(with_hg=False)
    r64, _g = _gat_ref(torch.float64, b, dict(c.inp, h=X32[:, :Hp * Dp]), keep, p, None, 0.0, c.pw)
    r32, _g = _gat_ref(torch.float32, b, dict(c.inp, h=X32[:, :Hp * Dp]), keep, p, None, 0.0, c.pw)
    ep = _take(e_part, n, nt)
    items = _forward_items("edot forward", b, out, r64, r32, Kt, keys=("a12", "alpha", "wsum", "Z"))
    items.append(("e_part", ep, _e_part_ref(torch.float64, Tf, zrow, b["gid"], X32, keep, nt), _e_part_ref(torch.float32, Tf, zrow, b["gid"], X32, keep, nt)))
    # ---- 2d: the scores from e_part, with and without exp, scaled for the mask or not ----
    for ex in (0, 1):
        sb = _guarded(G)
        _rc, sn = _profiled(lambda: L.call("txe_gat_collapse_fold_scores", b["csr"].graph_off.data_ptr(), n, G, Hp * Dp, Pd, fw.coef.data_ptr(), fw.wsum.data_ptr(),
                                           e_part.data_ptr(), p, int(masked), ex, sb.data_ptr(), L.stream_ptr()))
        assert _named(sn) == ["cl_fold_score_kernel"], sn
        s = _take(sb, G)
        assert np.array_equal(s[~b["live"]], np.full(3, 1.0 if ex else 0.0, np.float32))      # an empty graph: raw score 0
        raw64 = (r64["Z"] * Tf[zrow][:, :Kt].astype(np.float64)).sum(1)
        raw32 = (r32["Z"] * Tf[zrow][:, :Kt]).sum(1, dtype=np.float32)
        f = (lambda a: np.exp(a)) if ex else (lambda a: a)
        items.append((f"scores exp {ex}", s[b["live"]], f(raw64)[b["live"]], f(raw32)[b["live"]]))
    if not masked:                                                                   # (masked = 0 with a drop probability: no scale)
        sb = _guarded(G)
        L.call("txe_gat_collapse_fold_scores", b["csr"].graph_off.data_ptr(), n, G, Hp * Dp, Pd, fw.coef.data_ptr(), fw.wsum.data_ptr(), e_part.data_ptr(), 0.3, 0,
               0, sb.data_ptr(), L.stream_ptr())
        items.append(("scores, p given but not masked", _take(sb, G)[b["live"]], raw64[b["live"]], raw32[b["live"]]))
    # ---- backward from (m_ds, m_s, m_exp) and the float64 e_part ----
    e64 = _up(_e_part_ref(torch.float64, Tf, zrow, b["gid"], X32, keep, nt).astype(np.float32))
    dsd, sd, zgid = _up(ds), _up(dZ_of.s32), torch.full((n + 1,), -7, dtype=torch.int32, device=_dev())
    c.match = L.FoldMatch(e_part=e64.data_ptr(), m_ds=dsd.data_ptr(), m_s=sd.data_ptr(), m_exp=m_exp, Tf=Tfd.data_ptr(), zrow=zrowd.data_ptr(), zgid=zgid.data_ptr())
    got, names = c.run([L.FUSED_ALL | L.FUSED_DZ_GIVEN | L.FUSED_EDOT])
    assert names == fl.fused_launches(Kp, masked, Hp, Dp, edot=True), names
    z = zgid.cpu().numpy()
    assert np.array_equal(z[:n], zrow[b["gid"]]) and z[n] == -7
    _gate("gat_collapse_bwd_fused[edot]", items + c.items(f"edot exp {m_exp}", got))


def test_folded_matcher_needs_the_chunked_sweep():
    """on A (G < 16: the per-graph Z sweep forms no e_part) txe_gat_collapse_e_tiles is 0, and the forward call with a FoldMatch, the score
    call and the TXE_FUSED_EDOT backward return TXE_ERR_ARG before any launch: every output buffer keeps its NaN."""
    from taxoexpan_amd import _lib
    L = _lib
    Hp, Dp, Pd = 4, 4, 4
    b = _batch("A")
    n, G = b["n"], b["G"]
    assert L.call("txe_gat_collapse_e_tiles", n, G, Hp * Dp, Pd) == 0 and L.call("txe_gat_collapse_e_tiles", 0, 16, 16, 4) == 0
    c = _Fused("A", Hp, Dp, Pd, False)
    Tfd, zrowd, e_part = _up(np.zeros((G, c.inp["Kp"]), np.float32)), _up(np.arange(G, dtype=np.int32)), torch.zeros(n * 2 + 1, device=_dev())
    fw = _FoldState(b, c.st.inp, c.packed, None, 0.0, c.pw, 0.0, want_hg=False)
    with pytest.raises(L.TxeError, match="TXE_ERR_ARG"):
        fw.forward(match=L.FoldMatch(e_part=e_part.data_ptr(), Tf=Tfd.data_ptr(), zrow=zrowd.data_ptr()))
    torch.cuda.synchronize()
    for t in (fw.a12, fw.alpha, fw.coef, fw.wsum, fw.Z):                              # (nothing was launched: not the logits, not the edge kernel)
        assert bool(torch.isnan(t).all())
    sb = _nan(G)
    with pytest.raises(L.TxeError, match="TXE_ERR_ARG"):
        L.call("txe_gat_collapse_fold_scores", b["csr"].graph_off.data_ptr(), n, G, Hp * Dp, Pd, fw.coef.data_ptr(), fw.wsum.data_ptr(), e_part.data_ptr(), 0.0, 0, 0,
               sb.data_ptr(), L.stream_ptr())
    ones, zgid = torch.ones(G, device=_dev()), torch.zeros(n, dtype=torch.int32, device=_dev())
    c.match = L.FoldMatch(e_part=e_part.data_ptr(), m_ds=ones.data_ptr(), m_s=ones.data_ptr(), m_exp=0, Tf=Tfd.data_ptr(), zrow=zrowd.data_ptr(), zgid=zgid.data_ptr())
    c.dZ = np.zeros((G, c.inp["Kt"]), np.float32)                                    # (ld_dhg = Kp, as TXE_FUSED_DZ_GIVEN wants it)
    with pytest.raises(L.TxeError, match="TXE_ERR_ARG"):
        c.run([L.FUSED_ALL | L.FUSED_DZ_GIVEN | L.FUSED_EDOT], check=False)
    torch.cuda.synchronize()
    assert bool(torch.isnan(sb).all())


# ---- 2e. txe_gcn_collapse_fwd / _bwd ------------------------------------------------------------------------------------------------------------
def _gcn_ref(dtype, b, inp, keep, p, bias, pw, act_on=False, w=None, dZ=None):
    Kt = inp["Kt"]
    grad = w is not None or dZ is not None
    hl = _t(inp["h"], dtype, grad)
    P, W, bt, pwt = (_t(a, dtype, grad) for a in (inp["P"], inp["Wg"], bias, pw))
    hh = _behind_activation(hl, inp["h"]) if act_on else hl
    Pp = P[b["post"]]
    if grad:
        Pp.retain_grad()
    r = fl.gcn_fold(torch.cat((hh, Pp), 1), _t(keep[:, :Kt], dtype) if keep is not None else None, 1.0 / (1.0 - p), W, bt, b["s"], b["d"], b["goff"], b["post"], pwt)
    g = None
    if grad:
        ((r["hg"] * _t(w, dtype)).sum() if dZ is None else (r["Z"] * _t(dZ, dtype)).sum()).backward()
        zero = lambda t_: _np(t_.grad) if t_.grad is not None else np.zeros(tuple(t_.shape))
        g = dict(d_X=np.concatenate([zero(hl), zero(Pp)], 1), dW=zero(W), dP=zero(P))
        if bias is not None:
            g["d_b"] = zero(bt)
        if pw is not None:
            g["d_pw"] = zero(pwt).reshape(-1)
    return {k: _np(v) for k, v in r.items()}, g


def _gcn_case(bname, Kh, Pd, Fo, masked, with_bias, with_pw, act_on, dz_given=False):
    from taxoexpan_amd import _lib
    L = _lib
    b = _batch(bname)
    csr, n, G = b["csr"], b["n"], b["G"]
    rs = np.random.RandomState(600 + Kh + Fo)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)
    Kt, Kp, Fop = Kh + Pd, fl.padded_k(Kh, Pd), (Fo + 31) // 32 * 32
    inp = dict(h=f(n, Kh), P=f(VOCAB, Pd), Wg=f(Kt, Fo) / np.float32(np.sqrt(Kt)), Kh=Kh, Pd=Pd, Kt=Kt, Kp=Kp)
    bias, w = f(Fo), f(G, Fo)
    dZ = f(G, Kt) if dz_given else None
    X = _padded(np.concatenate([inp["h"], inp["P"][b["pos"]]], 1), Kp)
    bias_ = bias if with_bias else None
    pw = np.array([[0.3], [-0.2], [0.5]], dtype=np.float32) if with_pw else None
    p = 0.3 if masked else 0.0
    mask, keep = _mask_bits(n, Kp, p, SEED) if masked else (None, None)
    tag = f"{bname} mask {int(masked)} bias {int(with_bias)} pw {int(with_pw)} act {int(act_on)}" + (" dz_given" if dz_given else "")
    # ---- device inputs ----
    Xd, Wd, bd, pwd = _up(X), _up(inp["Wg"]), _up(bias), (_up(pw) if with_pw else None)
    Wp = _nan((Kp + 127) // 128 * 128, Fop)
    L.call("txe_gcn_pack_weights", Wd.data_ptr(), Kt, Fo, Wp.data_ptr(), L.stream_ptr())
    wp = Wp.cpu().numpy()
    assert np.array_equal(wp[:Kt, :Fo], inp["Wg"]) and not wp[Kt:].any() and not wp[:, Fo:].any()
    norm = _guarded(n)
    L.call("txe_gcn_norm", csr.rowptr_in.data_ptr(), n, norm.data_ptr(), L.stream_ptr())
    coef, wsum, Z, hgb = _guarded(n), _guarded(G), _guarded(G * Kp), _nan(G, Fo + 3)
    gid = torch.full((n + 1,), -7, dtype=torch.int32, device=_dev())
    layer = L.GcnFoldLayer(X=Xd.data_ptr(), Kh=Kh, Pd=Pd, pos=b["posd"].data_ptr(), vocab=VOCAB, Wp=Wp.data_ptr(), Fo=Fo, bias=bd.data_ptr() if with_bias else None,
                           drop_p=p, mask=_ptr(mask), norm=norm.data_ptr(), pw=_ptr(pwd), coef=coef.data_ptr(), wsum=wsum.data_ptr(), gid=gid.data_ptr(),
                           Z=Z.data_ptr(), hg=hgb.data_ptr(), ld_hg=Fo + 3)
    wsb = L.call("txe_gcn_collapse_ws_bytes", n, G, Kh, Pd, Fo, VOCAB)
    # ---- forward ----
    ws = _ws(wsb)
    _rc, names = _profiled(lambda: L.call("txe_gcn_collapse_fwd", L.ref(b["gb"]), L.ref(layer), ws.data_ptr(), wsb, L.stream_ptr()))
    assert _named(names) == [fl.zsum_kernel(n, G, masked)], names
    r64, _g = _gcn_ref(torch.float64, b, inp, keep, p, bias_, pw)
    r32, _g = _gcn_ref(torch.float32, b, inp, keep, p, bias_, pw)
    live = b["live"]
    hg = hgb.cpu().numpy()
    assert np.isfinite(hg[:, :Fo]).all() and np.isnan(hg[:, Fo:]).all()
    g = gid.cpu().numpy()
    assert np.array_equal(g[:n], b["gid"]) and g[n] == -7
    Zh, wsh = _take(Z, G, Kp), _take(wsum, G)
    assert not Zh[:, Kt:].any() and not Zh[~live].any() and not wsh[~live].any()
    assert np.array_equal(hg[~live, :Fo], np.broadcast_to(bias if with_bias else np.zeros(Fo, np.float32), (int((~live).sum()), Fo)))   # an empty graph: the bias
    items = [(f"coef [{tag}]", _take(coef, n), r64["coef"], r32["coef"]), (f"wsum [{tag}]", wsh[live], r64["wsum"][live], r32["wsum"][live]),
             (f"Z [{tag}]", Zh[live, :Kt], r64["Z"][live], r32["Z"][live]), (f"hg [{tag}]", hg[live, :Fo], r64["hg"][live], r32["hg"][live])]
    # ---- backward from the uploaded float64 state ----
    coef[:n], wsum[:G] = _up(r64["coef"].astype(np.float32)), _up(r64["wsum"].astype(np.float32))
    Z[:G * Kp] = _up(_padded(r64["Z"].astype(np.float32), Kp).reshape(-1))
    _r, g64 = _audit(lambda: _gcn_ref(torch.float64, b, inp, keep, p, bias_, pw, act_on, None if dz_given else w, dZ)) if act_on else \
        _gcn_ref(torch.float64, b, inp, keep, p, bias_, pw, act_on, None if dz_given else w, dZ)
    _r, g32 = _gcn_ref(torch.float32, b, inp, keep, p, bias_, pw, act_on, None if dz_given else w, dZ)
    d_hg = _up(_padded(dZ, Kp)) if dz_given else _up(w)
    d_X, dW, d_b, dP, d_pw = _guarded(n * Kp), _guarded(Kt * Fo), _guarded(Fo), _guarded(VOCAB * Pd), (_guarded(VOCAB) if with_pw else None)
    grads = L.GcnFoldGrads(dW=dW.data_ptr(), d_b=d_b.data_ptr() if with_bias else None, dP=dP.data_ptr(), d_pw=_ptr(d_pw))
    ws = _ws(wsb)

    def bwd(ld):
        return L.call("txe_gcn_collapse_bwd", L.ref(b["gb"]), L.ref(layer), d_hg.data_ptr(), ld, int(act_on), ACT_SLOPE, d_X.data_ptr(), L.ref(grads), int(dz_given),
                      ws.data_ptr(), wsb, L.stream_ptr())
    if dz_given:
        with pytest.raises(L.TxeError, match="TXE_ERR_ARG"):                          # a dZ without the padded row pitch: rejected before any launch
            bwd(Kt)
        torch.cuda.synchronize()
        assert bool(torch.isnan(d_X).all())
    _rc, names = _profiled(lambda: bwd(Kp if dz_given else Fo))
    assert _named(names) == fl.bwd_launches(Kp, masked, att=False, dot=with_pw), names
    dx = _take(d_X, n, Kp)
    assert not dx[:, Kt:].any()
    items += [(f"d_X [{tag}]", dx[:, :Kt], g64["d_X"], g32["d_X"]), (f"dP [{tag}]", _take(dP, VOCAB, Pd), g64["dP"], g32["dP"])]
    if with_pw:
        items.append((f"d_pw [{tag}]", _take(d_pw, VOCAB), g64["d_pw"], g32["d_pw"]))
    if dz_given:
        assert bool(torch.isnan(dW).all()) and bool(torch.isnan(d_b).all())            # dW and d_b are the consumer's: not written
    else:
        items.append((f"dW [{tag}]", _take(dW, Kt, Fo), g64["dW"], g32["dW"]))
        if with_bias:
            items.append((f"d_b [{tag}]", _take(d_b, Fo), g64["d_b"], g32["d_b"]))
        else:
            assert bool(torch.isnan(d_b).all())
    return items


@pytest.mark.parametrize("Kh,Pd,Fo,bname", fl.GCN_CASES, ids=[f"Kp{fl.padded_k(c[0], c[1])}-Fo{c[2]}-{c[3]}" for c in fl.GCN_CASES])
def test_gcn_fold_against_float64(Kh, Pd, Fo, bname):
    """forward (coef, wsum, Z, hg; gid exact) and backward (d_X, dW, d_b, dP, d_pw) with and without the mask; bias, pw and act_on each on
    and off across the two runs of a case and the cases of the table"""
    flip = (fl.GCN_CASES.index((Kh, Pd, Fo, bname)) % 2) == 0                       # (A, B and C each see both patterns)
    items = _gcn_case(bname, Kh, Pd, Fo, False, flip, not flip, flip)
    items += _gcn_case(bname, Kh, Pd, Fo, True, not flip, flip, not flip)
    _gate("gcn_collapse", items)


@pytest.mark.parametrize("bname", ["A", "B"])
def test_gcn_fold_backward_with_dz_given(bname):
    """dz_given: d_hg IS dZ [G][Kp] -- dW and d_b are not written and keep their NaN; d_X, dP and d_pw are gated against the reference
    differentiated under (Z * dZ).sum(); a wrong ld_dhg is TXE_ERR_ARG"""
    _gate("gcn_collapse[dz_given]", _gcn_case(bname, 250, 50, 6, True, True, True, True, dz_given=True))
