"""The propagation layers' DENSE part (csrc/txe_project.hip: preparation launches, the projection Y = dropout(X) Wp^T, its backward) against
FLOAT64, entry point by entry point, through the C ABI (_lib.call: the test owns X [N][Kp], every stride and every workspace), at every
edge of the host-side dispatch.

Reference: tests/dense_layer_ref.py -- gat_dense, gcn_dense, build_x (tests/test_dense_layer_ref_cpu.py holds them to orc.gat_layer /
orc.gcn_layer / orc.pgat_forward) -- in float64 on the CPU, gradients by autograd (seeded through Y / hw); yardstick: the same function in
fp32 on the CPU; gate: golden_util.gate_against_f64 with its defaults, once per tensor per case.  Every gate prints "[gate] operator what
device-error yardstick-error" (fractions of the tensor's largest float64 entry).  No tensor needs a scale_floor: every gated gradient is
a direct product with a standard-normal seed.  The bf16-pipe routes (txe_gat_dense_fwd_split, _split_src, TXE_DENSE_DX_SPLIT, the
weight gradient from Xt) are held to the SAME gate: the project claims fp32 accuracy for them.  The activation's branch (act_on) is the
sign of the stored fp32 X that both sides read: no branch audit is needed.

Inputs: X (= [h | P[pos]]), d_Y / d_hw standard normal; W / sqrt(Kt); attn_l, attn_r / sqrt(D).  Wp comes from txe_gat_pack_weights /
txe_gcn_pack_weights into a NaN-filled buffer, masks from txe_dropout_mask (read back and compared with rng.keep_mask_bits); a
pre-dropped X from txe_gat_layers_prepare / txe_gcn_layers_prepare with x_dropped = 1 (compared with the host's X keep / (1 - p), exactly).
d_Y's padding columns [Fe, Fp) are zero, as txe.h requires.

NaN poisoning: the workspace is NaN before every call, and 64 NaN words behind the documented size stay NaN (the *_ws_bytes functions
are exactly enough); every output lives in a NaN-filled buffer with a NaN guard behind it; of d_X only the columns [c0, Kt) are written
(c0 = need_dh ? 0 : Kh / 4 * 4), everything else keeps its NaN.  The columns [Fe, Fp) of Y / [Fo, Fop) of hw are UNTOUCHED by all four
forward entry points (txe_gat_dense_fwd, txe_gat_dense_fwd_split, txe_gat_dense_fwd_split_src, txe_gcn_dense_fwd): they keep their NaN.
A rejected call launches nothing (profiler count 0) and leaves every output and the workspace NaN.

Instance -> case (each case asserts ITS launch names through the library profiler, as dense_layer_ref.py's restated choose_bn /
choose_splits / tail-split rule predict them; test_dense_layer_ref_cpu.py holds the tables to the routes):
    gemm_kernel<true, true, 4, 4, 64> (+ gemm_tail_fixup_kernel<64> at Kp 320 with a tail workspace), split_pack_multi_kernel,
    gemm_nt_split_kernel<2, 3, 2, 0>, gemm_kernel<true, false, 4, 4, 64> through txe_gcn_dense_fwd      test_forward (dl.FWD_CASES)
    gemm_kernel<true, false, 4, 4, 64> on Wp + c0 with mask_col0 = c0 and the column-split epilogue, no gat_dx_pos_kernel;
    gat_dx_pos_kernel beside it; gemm_tn_split_kernel from Xt, X == NULL                                 test_gat_backward_position_only
    gemm_kernel<true, false, ...> with mask and leaky' in its epilogue (Fp 128) or in gemm_tail_fixup_kernel (Fp 384);
    split_pack_kernel x 2 + gemm_nt_split_kernel<2, 3, 2, 1> (TXE_DENSE_DX_SPLIT)                        test_gat_backward_need_dh
    the phase flags, TXE_PH_DEFER + txe_gat_tail_flush                                                  test_gat_backward_phases_are_one_result
    gemm_kernel<true, true, ...> + gemm_kernel<false, false, ...> / gemm_tn_lds_kernel + reduce_splits_transposed_kernel
                                                                                                        test_gcn_backward, test_gcn_backward_transposed_route
    (gemm_tn_lds_kernel INSIDE txe_gat_dense_bwd needs 2 Fp Kp n >= 2e10 and the 128-wide tiles more than 512 tiles: both stay with
    the full-size tests)

Measured on the MI355X, largest device error / yardstick error per entry point over all cases of this file, and the largest device error
itself (fractions of the tensor's largest float64 entry; the gate's floor is 2e-5, and the two ratios above 2 are of tensors under it):
    txe_gat_pack_weights (folded rows)   2.0  ((250 + 50, H 4, D 24): 1.7e-7 against 8.7e-8); largest 1.7e-7
    txe_gat_dense_fwd                    1.9  (Y, mask in the loader, no tail workspace: 5.4e-7 against 2.9e-7); largest 6.4e-7
    txe_gat_dense_fwd_split / _split_src 1.6  (Y, p 0.3: 6.4e-7 against 3.9e-7 on both); largest 6.4e-7
    txe_gcn_dense_fwd                    2.1  (hw, p 0: 7.7e-7 against 3.7e-7); largest 7.7e-7
    txe_gat_dense_bwd, position only     1.9  (dW, masked, fp32 route: 4.9e-7 against 2.5e-7); largest 4.9e-7
    txe_gat_dense_bwd, need_dh           2.0  (d_X, TXE_DENSE_DX_SPLIT, masked: 5.5e-7 against 2.8e-7); largest 6.0e-7 (d_X, TXE_DENSE_DX_SPLIT)
    txe_gcn_dense_bwd                    1.4  (d_X, act_on: 2.3e-7 against 1.7e-7); largest 5.2e-7 (dW)
    txe_gcn_dense_bwd at n 4096          1.2 transposed (dW, Fo 500: 3.3e-7 against 2.7e-7), 1.6 plain (4.3e-7 against 2.8e-7); largest 4.3e-7
No case needed a scale_floor.  The 68 cases (565 gated tensors) take 4 s on the MI355X -- against the folded file's 12 to 13 s for 120: these
references are single products, the largest 4096 x 320 x 512 -- the slowest, test_packed_weights_of_both_families, 0.3 s.
"""
import ctypes

import numpy as np
import pytest
import torch

import dense_layer_ref as dl
from test_gpu_folded_layer_ops import _gate, _guarded, _nan, _padded, _ptr, _take, _up
from test_gpu_message_passing_ops import _mask_bits
from test_gpu_readout_match_ops import _profiled

pytestmark = pytest.mark.gpu

ACT_SLOPE, SEED, VOCAB, P_DROP = 0.01, 4242, 3, 0.3
GUARD = 64                                      # NaN words behind every workspace


def _dev():
    return torch.device("cuda:0")


def _L():
    from taxoexpan_amd import _lib
    return _lib


def _ws(nbytes):
    return _nan(nbytes // 4 + GUARD)


def _ws_intact(ws, nbytes):
    assert bool(torch.isnan(ws[(nbytes + 3) // 4:]).all()), "the words behind the workspace were written"


def _scale32(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))          # the kernels' drop_scale = 1.f / (1.f - p)


def _view(buf, rows, ld, c_lo, c_hi):
    """a [rows][ld] output of which only the columns [c_lo, c_hi) are written: those finite, everything else and the guard still NaN"""
    a = buf.cpu().numpy()
    assert np.isnan(a[rows * ld:]).all()
    a = a[:rows * ld].reshape(rows, ld)
    assert np.isfinite(a[:, c_lo:c_hi]).all(), "unwritten entries inside the view"
    assert np.isnan(a[:, :c_lo]).all() and np.isnan(a[:, c_hi:]).all(), "written entries outside the view"
    return a[:, c_lo:c_hi]


# ---- one layer's inputs -----------------------------------------------------------------------------------------------------------------------
class _Case:
    """inputs of one GAT (H, D) or GCN (Fo) layer on the host and the device; packed weights; on demand the mask and the pre-dropped X"""

    def __init__(self, kind, n, Kh, Pd, H=1, D=1, Fo=1, seed=0):
        L = _L()
        self.kind, self.n, self.Kh, self.Pd, self.H, self.D, self.Fo = kind, n, Kh, Pd, H, D, Fo
        self.Kt, self.Kp = Kh + Pd, dl.padded_k(Kh, Pd)
        rs = np.random.RandomState(1000 + seed + 7 * n + Kh + 3 * Pd)
        f = lambda *s: rs.standard_normal(s).astype(np.float32)
        Kt = self.Kt
        self.h, self.P, self.pos = f(n, Kh), f(VOCAB, Pd), rs.randint(0, VOCAB, n).astype(np.int32)
        self.X = _padded(np.concatenate([self.h, self.P[self.pos]], 1), self.Kp)
        self.Xd, self.posd, self.Pdev = _up(self.X) if n else _nan(1, self.Kp), _up(self.pos) if n else _nan(1), (_up(self.P) if Pd else None)
        if kind == "gat":
            self.F, self.Fe, self.Fp = H * D, H * D + 2 * H, dl.padded_f(H, D)
            self.W, self.al, self.ar = f(H * D, Kt) / np.float32(np.sqrt(Kt)), f(H, D) / np.float32(np.sqrt(D)), f(H, D) / np.float32(np.sqrt(D))
            self.Wd, self.ald, self.ard = _up(self.W), _up(self.al), _up(self.ar)
            self.Wp = _nan(self.Fp, self.Kp)
            L.call("txe_gat_pack_weights", self.Wd.data_ptr(), self.ald.data_ptr(), self.ard.data_ptr(), H, D, Kt, self.Wp.data_ptr(), L.stream_ptr())
        else:
            self.Fe, self.Fp = Fo, dl.gcn_padded_f(Fo)
            self.W = f(Kt, Fo) / np.float32(np.sqrt(Kt))
            self.Wd = _up(self.W)
            self.Wp = _nan(dl.round_up(self.Kp, 128), self.Fp)
            L.call("txe_gcn_pack_weights", self.Wd.data_ptr(), Kt, Fo, self.Wp.data_ptr(), L.stream_ptr())
        self.dY = f(n, self.Fe)
        self.dYd = _up(_padded(self.dY, self.Fp)) if n else torch.zeros(1, self.Fp, device=_dev())
        self._mask = self._dropped = self._xt = None
        self._refs = {}

    def attn(self):
        return (self.al, self.ar) if self.kind == "gat" else None

    def mask(self):
        if self._mask is None:
            self._mask = _mask_bits(self.n, self.Kp, P_DROP, SEED)
        return self._mask

    def dropped(self):
        """X with the dropout applied by the stack's preparation launch (x_dropped = 1): exactly X keep / (1 - p); the launch's mask and
        packed weights are those of txe_dropout_mask and txe_*_pack_weights, bit for bit"""
        if self._dropped is None:
            L = _L()
            mask, keep = self.mask()
            X, m2, Wp2 = _nan(self.n, self.Kp), torch.full_like(mask, -1), torch.full_like(self.Wp, float("nan"))
            hd = _up(self.h)
            if self.kind == "gat":
                d = L.GatPrepareDesc(h=hd.data_ptr(), ld_h=self.Kh, n_nodes=self.n, Kh=self.Kh, pos=self.posd.data_ptr(), P=_ptr(self.Pdev), Pd=self.Pd, X=X.data_ptr(),
                                     W=self.Wd.data_ptr(), attn_l=self.ald.data_ptr(), attn_r=self.ard.data_ptr(), H=self.H, D=self.D, Wp=Wp2.data_ptr(),
                                     feat_drop_p=P_DROP, seed=SEED, mask=m2.data_ptr(), x_dropped=1)
                L.call("txe_gat_layers_prepare", L.ref(d), 1, L.stream_ptr())
            else:
                d = L.GcnPrepareDesc(h=hd.data_ptr(), ld_h=self.Kh, n_nodes=self.n, Kh=self.Kh, pos=self.posd.data_ptr(), P=_ptr(self.Pdev), Pd=self.Pd, X=X.data_ptr(),
                                     W=self.Wd.data_ptr(), Fo=self.Fo, Wp=Wp2.data_ptr(), drop_p=P_DROP, seed=SEED, mask=m2.data_ptr(), x_dropped=1, bias_row=None)
                L.call("txe_gcn_layers_prepare", L.ref(d), 1, None, 0, None, L.stream_ptr())
            assert torch.equal(m2, mask) and torch.equal(Wp2, self.Wp)
            assert np.array_equal(X.cpu().numpy(), self.X * keep.astype(np.float32) * _scale32(P_DROP))
            self._dropped = X
        return self._dropped

    def xt(self, dropped):
        """X (plain or pre-dropped) packed contraction-major by txe_gat_dense_fwd_split: what the weight gradient takes on the bf16 pipe"""
        if self._xt is None:
            self._xt = {}
        if dropped not in self._xt:
            L = _L()
            nb = L.call("txe_gat_dense_split_xt_bytes", self.n, self.Kh, self.Pd, self.H, self.D)
            assert nb > 0 and dl.split_tn_eligible(self.Fp, self.Kp)
            Xt, Y = _nan(nb // 4 + 1), _nan(self.n, self.Fp)
            wsb = L.call("txe_gat_dense_split_ws_bytes", self.n, self.Kh, self.Pd, self.H, self.D)
            ws = _ws(wsb)
            X = self.dropped() if dropped else self.Xd
            L.call("txe_gat_dense_fwd_split", X.data_ptr(), self.n, self.Kh, self.Pd, self.Wp.data_ptr(), self.H, self.D, None, None, Xt.data_ptr(), Y.data_ptr(),
                   ws.data_ptr(), wsb, L.stream_ptr())
            torch.cuda.synchronize()
            _ws_intact(ws, wsb)
            assert bool(torch.isnan(Xt[-1]))
            self._xt[dropped] = Xt
        return self._xt[dropped]

    def fwd_ref(self, p):
        """(float64, fp32) of the projection's written columns, once per drop probability"""
        key = ("fwd", p)
        if key not in self._refs:
            out = []
            keep = self.mask()[1] if p > 0 else None
            for dtype in (torch.float64, torch.float32):
                t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
                X = dl.build_x(t(self.h), torch.from_numpy(self.pos).long(), t(self.P))
                k = t(keep[:, :self.Kt]) if keep is not None else None
                out.append((dl.gat_dense(X, t(self.W), t(self.al), t(self.ar), k, p) if self.kind == "gat" else dl.gcn_dense(X, t(self.W), k, p)).numpy())
            self._refs[key] = out
        return self._refs[key]

    def bwd_ref(self, p, act_on):
        key = ("bwd", p, act_on)
        if key not in self._refs:
            keep = self.mask()[1] if p > 0 else None
            self._refs[key] = [dl.backward(self.kind, dtype, self.h, self.P, self.pos, self.W, self.attn(), keep, p, self.dY, act_on, ACT_SLOPE)
                               for dtype in (torch.float64, torch.float32)]
        return self._refs[key]


def test_packed_weights_of_both_families():
    """txe_gat_pack_weights: rows < F exact, the 2H folded rows gated against float64, padding rows and columns zero (Wp NaN-primed);
    txe_gcn_pack_weights: exact, zero padding up to roundup(Kp, 128) rows"""
    items = []
    for n, Kh, Pd, H, D in dl.FWD_CASES:
        c = _Case("gat", 1, Kh, Pd, H, D)
        wp = c.Wp.cpu().numpy()
        assert np.array_equal(wp[:c.F, :c.Kt], c.W) and not wp[:, c.Kt:].any() and not wp[c.Fe:].any()
        wa = [dl.folded_rows(*(torch.from_numpy(a).to(dt) for a in (c.W, c.al, c.ar))).numpy() for dt in (torch.float64, torch.float32)]
        items.append((f"folded rows [{Kh}+{Pd} H{H} D{D}]", wp[c.F:c.Fe, :c.Kt], wa[0], wa[1]))
    _gate("gat_pack_weights", items)
    for (n, Kh, Pd, H, D), Fo in zip(dl.FWD_CASES, dl.GCN_FWD_FO):
        c = _Case("gcn", 1, Kh, Pd, Fo=Fo)
        wp = c.Wp.cpu().numpy()
        assert wp.shape == (dl.round_up(c.Kp, 128), dl.gcn_padded_f(Fo))
        assert np.array_equal(wp[:c.Kt, :Fo], c.W) and not wp[c.Kt:].any() and not wp[:, Fo:].any()


# ---- forward ------------------------------------------------------------------------------------------------------------------------------------
def _tail_ws(tail):
    L = _L()
    if not tail:
        return None, 0
    nb = L.call("txe_gemm_tail_ws_bytes")
    assert nb == dl.tail_ws_bytes()
    return _ws(nb), nb


@pytest.mark.parametrize("case", range(len(dl.FWD_CASES)), ids=["-".join(map(str, c)) for c in dl.FWD_CASES])
def test_forward_against_float64(case):
    """all four forward entry points at one shape: p 0 / 0.3, the mask in the loader or X pre-dropped and read plain, ws NULL or the
    tail workspace; _fwd_split with and without Xt_out; _fwd_split_src with ld_h = Kh and Kh + 3, with and without Xt_out -- its Xt
    bit-equal to _fwd_split's.  The columns [Fe, Fp) keep their NaN in every call."""
    L = _L()
    n, Kh, Pd, H, D = dl.FWD_CASES[case]
    Fo = dl.GCN_FWD_FO[case]
    items = []
    for kind in ("gat", "gcn"):
        c = _Case(kind, n, Kh, Pd, H, D, Fo)
        op = f"txe_{kind}_dense_fwd"
        for p, pre in ((0.0, False), (P_DROP, False), (P_DROP, True)):
            r64, r32 = c.fwd_ref(p)
            for tail in (False, True):
                X = c.dropped() if pre else c.Xd
                mask = c.mask()[0] if p > 0 and not pre else None
                Y, (ws, wsb) = _guarded(n * c.Fp), _tail_ws(tail)
                if kind == "gat":
                    fn = lambda: L.call(op, X.data_ptr(), n, Kh, Pd, c.Wp.data_ptr(), H, D, 0.0 if pre else p, _ptr(mask), Y.data_ptr(), _ptr(ws), wsb, L.stream_ptr())
                    want = dl.gat_fwd_launches(n, Kh, Pd, H, D, tail)
                else:
                    fn = lambda: L.call(op, X.data_ptr(), n, Kh, Pd, c.Wp.data_ptr(), Fo, 0.0 if pre else p, _ptr(mask), Y.data_ptr(), _ptr(ws), wsb, L.stream_ptr())
                    want = dl.gcn_fwd_launches(n, Kh, Pd, Fo, tail)
                _rc, names = _profiled(fn)
                assert names == want, (names, want)
                if tail:
                    _ws_intact(ws, wsb)
                items.append((f"{'Y' if kind == 'gat' else 'hw'} [p {p} pre {int(pre)} tail {int(tail)}]", _view(Y, n, c.Fp, 0, c.Fe), r64, r32))
        if kind == "gcn":
            _gate(op, items)
            continue
        _gate(op, items)
        items = []
        # ---- the bf16 pipe: X a plain operand (no dropout, or pre-dropped) ----
        wsb = L.call("txe_gat_dense_split_ws_bytes", n, Kh, Pd, H, D)
        xtb = L.call("txe_gat_dense_split_xt_bytes", n, Kh, Pd, H, D)
        assert xtb > 0
        xts = {}
        for p, pre in ((0.0, False), (P_DROP, True)):
            r64, r32 = c.fwd_ref(p)
            for with_xt in (False, True):
                X = c.dropped() if pre else c.Xd
                Y, ws, Xt = _guarded(n * c.Fp), _ws(wsb), (_nan(xtb // 4 + 1) if with_xt else None)
                _rc, names = _profiled(lambda: L.call("txe_gat_dense_fwd_split", X.data_ptr(), n, Kh, Pd, c.Wp.data_ptr(), H, D, None, None, _ptr(Xt), Y.data_ptr(),
                                                      ws.data_ptr(), wsb, L.stream_ptr()))
                assert names == dl.SPLIT_FWD, names
                _ws_intact(ws, wsb)
                if with_xt:
                    assert bool(torch.isnan(Xt[-1]))
                    xts[p] = Xt
                items.append((f"Y [split p {p} xt {int(with_xt)}]", _view(Y, n, c.Fp, 0, c.Fe), r64, r32))
        _gate("txe_gat_dense_fwd_split", items)
        items = []
        # ---- ... and from h, the position table and the keep mask: X never stored ----
        for p in (0.0, P_DROP):
            r64, r32 = c.fwd_ref(p)
            for extra, with_xt in ((0, True), (3, False), (3, True)):
                ld_h = Kh + extra
                hb = _nan(n, ld_h)
                hb[:, :Kh] = _up(c.h)
                Y, ws, Xt = _guarded(n * c.Fp), _ws(wsb), (_nan(xtb // 4 + 1) if with_xt else None)
                mask = c.mask()[0] if p > 0 else None
                _rc, names = _profiled(lambda: L.call("txe_gat_dense_fwd_split_src", hb.data_ptr(), ld_h, c.posd.data_ptr() if Pd else None, _ptr(c.Pdev), _ptr(mask), p,
                                                      n, Kh, Pd, c.Wp.data_ptr(), H, D, _ptr(Xt), Y.data_ptr(), ws.data_ptr(), wsb, L.stream_ptr()))
                assert names == dl.SPLIT_FWD, names
                _ws_intact(ws, wsb)
                if with_xt:
                    assert torch.equal(Xt.view(torch.int32), xts[p].view(torch.int32)), "Xt formed from (h, P, mask) differs from Xt packed from the stored X"
                items.append((f"Y [split_src p {p} ld_h +{extra} xt {int(with_xt)}]", _view(Y, n, c.Fp, 0, c.Fe), r64, r32))
        _gate("txe_gat_dense_fwd_split_src", items)
        items = []


# ---- txe_gat_dense_bwd ----------------------------------------------------------------------------------------------------------------------------
class _GatBwd:
    """one backward pass: NaN-filled outputs with guards, a NaN-primed workspace, txe_gat_dense_bwd once per entry of phase_calls"""

    def __init__(self, c, need_dh, act_on, p, x_dropped=False, split=False, xt=False, x_null=False, vocab=VOCAB, ws_delta=0, split_ws=None):
        L = _L()
        self.c, self.need_dh, self.act_on, self.p, self.x_dropped, self.split, self.xt, self.x_null = c, need_dh, act_on, p, x_dropped, split, xt, x_null
        self.vocab = vocab
        n, Kp = c.n, c.Kp
        self.d_X, self.dW, self.d_al, self.d_ar = _guarded(max(n, 1) * Kp), _guarded(c.F * c.Kt), _guarded(c.F), _guarded(c.F)
        self.dP = _guarded(VOCAB * c.Pd) if c.Pd else None
        self.base = L.call("txe_gat_dense_ws_bytes", n, c.Kh, c.Pd, c.H, c.D, min(vocab, VOCAB))
        self.wsb = self.base + (L.call("txe_gat_dense_bwd_split_ws_bytes", n, c.Kh, c.Pd, c.H, c.D) if (split if split_ws is None else split_ws) else 0) + ws_delta
        self.ws = _ws(self.wsb)

    def run(self, phase_calls=(dl.DENSE_ALL,), chain=None, flush=False, profiled=True):
        L, c = _L(), self.c
        X = None if self.x_null else (c.dropped() if self.x_dropped else c.Xd)
        Xt = c.xt(self.x_dropped) if self.xt else None
        mask = c.mask()[0] if self.p > 0 else None
        flag = dl.DENSE_DX_SPLIT if self.split else 0

        def calls():
            for ph in phase_calls:
                L.call("txe_gat_dense_bwd", _ptr(X), c.n, c.Kh, c.Pd, c.posd.data_ptr() if c.Pd else None, self.vocab, c.Wp.data_ptr(), c.Wd.data_ptr(),
                       c.ald.data_ptr(), c.ard.data_ptr(), c.H, c.D, self.p, _ptr(mask), c.dYd.data_ptr(), int(self.need_dh), int(self.act_on), ACT_SLOPE,
                       self.d_X.data_ptr(), self.dW.data_ptr(), self.d_al.data_ptr(), self.d_ar.data_ptr(), _ptr(self.dP), int(self.x_dropped), _ptr(Xt), ph | flag,
                       chain, self.ws.data_ptr(), self.wsb, L.stream_ptr())
            if flush:
                L.call("txe_gat_tail_flush", chain, L.stream_ptr())
        return _profiled(calls)[1] if profiled else calls()

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool(torch.isnan(t).all()) for t in (self.d_X, self.dW, self.d_al, self.d_ar, self.dP, self.ws) if t is not None)

    def outputs(self):
        c = self.c
        _ws_intact(self.ws, self.wsb)
        c0 = dl.dx_c0(c.Kh, self.need_dh)
        out = dict(dW=_take(self.dW, c.F, c.Kt), d_attn_l=_take(self.d_al, c.H, c.D), d_attn_r=_take(self.d_ar, c.H, c.D))
        if self.need_dh or c.Pd:
            out["d_X"] = _view(self.d_X, c.n, c.Kp, c0, c.Kt)
        else:
            assert bool(torch.isnan(self.d_X).all())
        if c.Pd:
            out["dP"] = _take(self.dP, VOCAB, c.Pd)
        return out

    def launches(self):
        c = self.c
        masked = self.p > 0
        return (dl.gat_dx_launches(c.n, c.Kh, c.Pd, c.H, c.D, self.need_dh, masked, self.act_on, self.split)
                + dl.gat_dw_launches(c.n, c.Kh, c.Pd, c.H, c.D, masked and not self.x_dropped, self.xt))

    def items(self, tag, out):
        c0 = dl.dx_c0(self.c.Kh, self.need_dh)
        g64, g32 = self.c.bwd_ref(self.p, self.act_on)
        its = []
        for k, v in out.items():
            a, b = (g64[k][:, c0:], g32[k][:, c0:]) if k == "d_X" else (g64[k], g32[k])
            its.append((f"{k} [{tag}]", v, a.reshape(v.shape), b.reshape(v.shape)))
        return its


@pytest.mark.parametrize("n,Kh,Pd,H,D,streams", dl.BWD_POS_CASES, ids=["-".join(map(str, c[:5])) + ("-stream" if c[5] else "-gemm") for c in dl.BWD_POS_CASES])
def test_gat_backward_position_only_against_float64(n, Kh, Pd, H, D, streams):
    """need_dh = 0: d_X[:, c0:Kt] (the straddling quad's feature columns [c0, Kh) included), dW, d_attn_l, d_attn_r, dP -- on the gemm_nn
    route with mask_col0 = c0 where the column range is wider than the streaming kernel's 64, on gat_dx_pos_kernel beside it; unmasked and
    masked; the weight gradient on the fp32 MFMA (mask in the loader / X pre-dropped) and from Xt on the bf16 pipe, with X and with X == NULL"""
    L = _L()
    assert L.call("txe_gat_dx_streams", Kh, Pd, 0) == streams == dl.dx_streams(Kh, Pd, 0)
    c = _Case("gat", n, Kh, Pd, H, D)
    items = []
    for p in (0.0, P_DROP):
        modes = [dict(), dict(xt=True), dict(xt=True, x_null=True)] if p == 0 else \
                [dict(), dict(x_dropped=True), dict(x_dropped=True, xt=True), dict(x_dropped=True, xt=True, x_null=True)]
        for m in modes:
            b = _GatBwd(c, 0, 0, p, **m)
            names = b.run()
            assert names == b.launches(), (names, b.launches())
            assert ("gat_dx_pos_kernel" in names) == bool(streams) and (names[0].startswith("gemm_kernel<true, false, ") or streams)
            assert (names[-1] == "gemm_tn_split_kernel") == bool(m.get("xt"))
            items += b.items(f"p {p} " + " ".join(sorted(m)), b.outputs())
    _gate("txe_gat_dense_bwd[position_only]", items)


@pytest.mark.parametrize("n,Kh,Pd,H,D", dl.BWD_DH_CASES, ids=["-".join(map(str, c)) for c in dl.BWD_DH_CASES])
def test_gat_backward_need_dh_against_float64(n, Kh, Pd, H, D):
    """need_dh = 1 on the fp32 MFMA (mask and leaky' factor in gemm_kernel's epilogue at Fp 128, in gemm_tail_fixup_kernel at Fp 384) and
    with TXE_DENSE_DX_SPLIT on the bf16 pipe: act_on x p; the activation factor reaches the columns < Kh only (the reference's); the
    weight gradient with the loader mask, and once per p from Xt"""
    c = _Case("gat", n, Kh, Pd, H, D)
    items = []
    for p in (0.0, P_DROP):
        for act_on in (0, 1):
            for split in (False, True):
                b = _GatBwd(c, 1, act_on, p, split=split, xt=bool(split and act_on), x_dropped=bool(split and act_on and p > 0))
                names = b.run()
                assert names == b.launches(), (names, b.launches())
                if split:
                    assert names[:3] == ["split_pack_kernel", "split_pack_kernel", "gemm_nt_split_kernel<2, 3, 2, 1>"]
                else:
                    assert ("gemm_tail_fixup_kernel<64>" in names or "gemm_tail_fixup_kernel<128>" in names) == (dl.padded_f(H, D) >= 256)
                items += b.items(f"p {p} act {act_on} split {int(split)}", b.outputs())
    _gate("txe_gat_dense_bwd[need_dh]", items)


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("which", ["position_only", "need_dh"])
def test_gat_backward_phases_are_one_result(which):
    """TXE_DENSE_DX, _DW, _REDUCE as three calls on one NaN-primed workspace, and TXE_DENSE_ALL | TXE_PH_DEFER into a chain followed by
    txe_gat_tail_flush: both bit-equal to one TXE_DENSE_ALL call (masked; the non-streaming position-only route, and need_dh with act_on)"""
    L = _L()
    c = _Case("gat", *(dl.BWD_POS_CASES[0][:5] if which == "position_only" else dl.BWD_DH_CASES[4]))
    kw = dict(need_dh=0, act_on=0) if which == "position_only" else dict(need_dh=1, act_on=1)
    base = _GatBwd(c, p=P_DROP, **kw)
    names = base.run()
    want = base.outputs()
    three = _GatBwd(c, p=P_DROP, **kw)
    assert three.run([dl.DENSE_DX, dl.DENSE_DW, dl.DENSE_REDUCE]) == names
    _same(want, three.outputs(), "three phase calls")
    chain = ctypes.create_string_buffer(L.TAIL_CHAIN_BYTES)
    deferred = _GatBwd(c, p=P_DROP, **kw)
    assert deferred.run([dl.DENSE_ALL | dl.PH_DEFER], chain=ctypes.cast(chain, ctypes.c_void_p), flush=False) == names
    torch.cuda.synchronize()
    assert bool(torch.isnan(deferred.dW).all()) and bool(torch.isnan(deferred.d_al).all())       # (phase B waits in the chain)
    L.call("txe_gat_tail_flush", ctypes.cast(chain, ctypes.c_void_p), L.stream_ptr())
    _same(want, deferred.outputs(), "deferred phase B")
    _gate(f"txe_gat_dense_bwd[phases_{which}]", base.items("all", want))


@pytest.mark.parametrize("need_dh", [0, 1])
def test_gat_backward_of_no_nodes(need_dh):
    """n_nodes = 0: dW, d_attn_l, d_attn_r and dP are exactly zero, d_X is untouched, nothing streams"""
    c = _Case("gat", 0, 250, 50, 2, 24)
    b = _GatBwd(c, need_dh, 0, 0.0)
    names = b.run()
    assert names == dl.gat_dw_launches(0, 250, 50, 2, 24, False, False), names
    torch.cuda.synchronize()
    assert bool(torch.isnan(b.d_X).all())
    for t, numel in ((b.dW, c.F * c.Kt), (b.d_al, c.F), (b.d_ar, c.F), (b.dP, VOCAB * c.Pd)):
        assert not _take(t, numel).any()
    _ws_intact(b.ws, b.wsb)


@pytest.mark.parametrize("what", ["ws_one_short", "dx_split_without_its_workspace", "vocab_9", "x_null_without_xt", "x_null_with_act_on",
                                  "x_null_xt_but_mask_in_the_loader"])
def test_gat_backward_rejections_launch_nothing(what):
    """each rejected call returns its documented code with ZERO launches (profiler count) and every output, and the workspace, still NaN"""
    L = _L()
    c = _Case("gat", *dl.BWD_DH_CASES[1])
    kw, code = {
        "ws_one_short": (dict(need_dh=1, act_on=0, p=P_DROP, ws_delta=-1), "TXE_ERR_WORKSPACE"),
        "dx_split_without_its_workspace": (dict(need_dh=1, act_on=0, p=P_DROP, split=True, split_ws=False), "TXE_ERR_WORKSPACE"),
        "vocab_9": (dict(need_dh=1, act_on=0, p=P_DROP, vocab=9), "TXE_ERR_ARG"),
        "x_null_without_xt": (dict(need_dh=0, act_on=0, p=0.0, x_null=True), "TXE_ERR_ARG"),
        "x_null_with_act_on": (dict(need_dh=1, act_on=1, p=0.0, x_null=True, xt=True), "TXE_ERR_ARG"),
        "x_null_xt_but_mask_in_the_loader": (dict(need_dh=0, act_on=0, p=P_DROP, x_null=True, xt=True), "TXE_ERR_ARG"),
    }[what]
    b = _GatBwd(c, **kw)
    if kw.get("xt"):
        c.xt(False)                                                      # (packed outside the profiled call)
    lib = L.load()
    lib.txe_profile_reset()
    lib.txe_profile_enable(1)
    try:
        with pytest.raises(L.TxeError, match=code):
            b.run(profiled=False)
        torch.cuda.synchronize()
        assert lib.txe_profile_count() == 0
    finally:
        lib.txe_profile_enable(0)
        lib.txe_profile_reset()
    assert b.untouched()


# ---- txe_gcn_dense_bwd ----------------------------------------------------------------------------------------------------------------------------
def _gcn_bwd(c, need_dh, act_on, p, x_dropped):
    """-> (items' outputs dict, launch names); txe_gcn_dense_ws_bytes is exactly enough"""
    L = _L()
    n, Kp, Kt, Fo = c.n, c.Kp, c.Kt, c.Fo
    d_X, dW, dP = _guarded(n * Kp), _guarded(Kt * Fo), (_guarded(VOCAB * c.Pd) if c.Pd else None)
    wsb = L.call("txe_gcn_dense_ws_bytes", n, c.Kh, c.Pd, Fo, VOCAB)
    ws = _ws(wsb)
    X = c.dropped() if x_dropped else c.Xd
    mask = c.mask()[0] if p > 0 else None
    _rc, names = _profiled(lambda: L.call("txe_gcn_dense_bwd", X.data_ptr(), n, c.Kh, c.Pd, c.posd.data_ptr() if c.Pd else None, VOCAB, c.Wp.data_ptr(), Fo, p,
                                          _ptr(mask), c.dYd.data_ptr(), int(need_dh), int(act_on), ACT_SLOPE, d_X.data_ptr(), dW.data_ptr(), _ptr(dP), int(x_dropped),
                                          ws.data_ptr(), wsb, L.stream_ptr()))
    _ws_intact(ws, wsb)
    out = dict(dW=_take(dW, Kt, Fo))
    if need_dh or c.Pd:
        out["d_X"] = _view(d_X, n, Kp, dl.dx_c0(c.Kh, need_dh), Kt)
    else:
        assert bool(torch.isnan(d_X).all())
    if c.Pd:
        out["dP"] = _take(dP, VOCAB, c.Pd)
    return out, names


def _gcn_items(c, tag, out, need_dh, act_on, p):
    c0 = dl.dx_c0(c.Kh, need_dh)
    g64, g32 = c.bwd_ref(p, bool(act_on and need_dh))
    return [(f"{k} [{tag}]", v, (g64[k][:, c0:] if k == "d_X" else g64[k]), (g32[k][:, c0:] if k == "d_X" else g32[k])) for k, v in out.items()]


@pytest.mark.parametrize("n,Kh,Pd,Fo", dl.GCN_CASES, ids=["-".join(map(str, c)) for c in dl.GCN_CASES])
def test_gcn_backward_against_float64(n, Kh, Pd, Fo):
    """d_X[:, c0:Kt], dW [Kt][Fo], dP: need_dh x act_on x p x x_dropped; the plain gemm_tn (then reduce_splits_sub) for dW"""
    c = _Case("gcn", n, Kh, Pd, Fo=Fo)
    items = []
    for need_dh in (0, 1):
        for act_on in ((0, 1) if need_dh else (0,)):
            for p, xd in ((0.0, 0), (P_DROP, 0), (P_DROP, 1)):
                out, names = _gcn_bwd(c, need_dh, act_on, p, xd)
                want = dl.gcn_bwd_launches(n, Kh, Pd, Fo, need_dh, p > 0, act_on, xd)
                assert names == want and names[-1].startswith("gemm_kernel<false, false, 4, 4, "), (names, want)
                items += _gcn_items(c, f"dh {need_dh} act {act_on} p {p} xd {xd}", out, need_dh, act_on, p)
    _gate("txe_gcn_dense_bwd", items)


@pytest.mark.parametrize("Fo", dl.GCN_DWT_FO)
@pytest.mark.parametrize("n,Kh,Pd,p,xd,transposed", dl.GCN_DWT_CASES, ids=[f"n{c[0]}-Kp{dl.padded_k(c[1], c[2])}-p{c[3]}-xd{c[4]}" for c in dl.GCN_DWT_CASES])
def test_gcn_backward_transposed_route(n, Kh, Pd, p, xd, transposed, Fo):
    """the predicate of the transposed dW route (gcn_dwt_splits: n >= 4096 and Kp tiling into 160-column tiles; a masked, not pre-dropped
    input falls back): which route ran, from the profiler's GEMM name and the restated predicate; dW gated on both"""
    c = _Case("gcn", n, Kh, Pd, Fo=Fo)
    assert dl.gcn_dw_transposed(n, c.Kp, c.Fp, p > 0, xd) == transposed
    out, names = _gcn_bwd(c, 0, 0, p, xd)
    assert names == dl.gcn_bwd_launches(n, Kh, Pd, Fo, 0, p > 0, 0, xd), names
    assert (names[-1] == "gemm_tn_lds_kernel") == transposed and (names[-1].startswith("gemm_kernel<false, false, 4, 4, ") or transposed)
    _gate("txe_gcn_dense_bwd[dW_transposed]" if transposed else "txe_gcn_dense_bwd[dW_plain_n4096]", _gcn_items(c, f"Fo {Fo}", out, 0, 0, p))


# ---- preparation and helpers ------------------------------------------------------------------------------------------------------------------------
def _gcn_prep_buffers(c, h_given, extra, with_bias, sentinel):
    """(h buffer or None, ld_h, X prefilled, Wp NaN, mask, bias at an address that is 4 mod 8, expected-host pieces)"""
    n, Kh, Kp = c.n, c.Kh, c.Kp
    ld_h = Kh + extra
    hb = None
    if h_given:
        hb = _nan(n, ld_h)
        hb[:, :Kh] = _up(c.h)
    X = _nan(n * Kp + 1)
    if not h_given:                                  # the layer below wrote the feature columns already
        xv = X[:n * Kp].view(n, Kp)
        xv[:, :Kh] = _up(sentinel)
    Wp = torch.full_like(c.Wp, float("nan"))
    mask = torch.full((n, Kp // 32), -1, dtype=torch.int32, device=_dev())
    bias = None
    if with_bias:
        bias = _nan(c.Fo + 1)[1:]
        bias.copy_(_up(np.arange(1, c.Fo + 1, dtype=np.float32) / 8))
        assert bias.data_ptr() % 8 == 4
    return hb, ld_h, X, Wp, mask, bias


@pytest.mark.parametrize("n,Kh,Pd,Fo,h_given,extra,xd,with_bias", dl.PREP_CASES, ids=["-".join(str(int(v)) for v in c) for c in dl.PREP_CASES])
@pytest.mark.parametrize("p", [0.0, P_DROP])
def test_gcn_layer_prepare_equals_layers_prepare(n, Kh, Pd, Fo, h_given, extra, xd, with_bias, p):
    """X, Wp and mask of txe_gcn_layer_prepare and of txe_gcn_layers_prepare: equal to each other and to the host's [h | P[pos] | 0]
    (x keep / (1 - p) when x_dropped; with h == NULL the feature columns -- the straddling quad's included -- untouched), W zero-padded
    with bias_row as row Kt, txe_dropout_mask's words; a NaN guard behind X"""
    L = _L()
    c = _Case("gcn", n, Kh, Pd, Fo=Fo)
    Kt, Kp = c.Kt, c.Kp
    sentinel = np.random.RandomState(5).standard_normal((n, Kh)).astype(np.float32)
    results = []
    for multi in (False, True):
        hb, ld_h, X, Wp, mask, bias = _gcn_prep_buffers(c, h_given, extra, with_bias, sentinel)
        args = dict(h=_ptr(hb), ld_h=ld_h, n_nodes=n, Kh=Kh, pos=c.posd.data_ptr() if Pd else None, P=_ptr(c.Pdev), Pd=Pd, X=X.data_ptr(), W=c.Wd.data_ptr(), Fo=Fo,
                    Wp=Wp.data_ptr(), drop_p=p, seed=SEED, mask=mask.data_ptr() if p > 0 else None, x_dropped=xd, bias_row=_ptr(bias))
        if multi:
            d = L.GcnPrepareDesc(**args)
            L.call("txe_gcn_layers_prepare", L.ref(d), 1, None, 0, None, L.stream_ptr())
        else:
            L.call("txe_gcn_layer_prepare", *[args[k] for k in ("h", "ld_h", "n_nodes", "Kh", "pos", "P", "Pd", "X", "W", "Fo", "Wp", "drop_p", "seed", "mask", "x_dropped",
                                                                "bias_row")], L.stream_ptr())
        torch.cuda.synchronize()
        results.append((X.cpu().numpy(), Wp.cpu().numpy(), mask.cpu().numpy()))
    (x1, w1, m1), (x2, w2, m2) = results
    assert np.array_equal(x1, x2, equal_nan=True) and np.array_equal(w1, w2) and np.array_equal(m1, m2)
    assert np.isnan(x1[-1])
    want = c.X.copy()
    if p > 0:
        words, keep = c.mask()
        assert np.array_equal(m1, words.cpu().numpy())
        if xd:
            want = want * keep.astype(np.float32) * _scale32(p)
    else:
        assert (m1 == -1).all()
    if not h_given:
        want[:, :Kh] = sentinel
    assert np.array_equal(x1[:-1].reshape(n, Kp), want)
    wp = c.Wp.cpu().numpy().copy()
    if with_bias:
        wp[Kt, :Fo] = np.arange(1, Fo + 1, dtype=np.float32) / 8
    assert np.array_equal(w1, wp)


def test_gcn_layers_prepare_of_a_stack():
    """two layers in one call equal two single calls; the norm written by the leading workgroups is bit-equal to txe_gcn_norm; six layers
    (more than PREP_MAXL = 4) take the second launch; bias_row with Kt % 32 == 0 is TXE_ERR_ARG"""
    L = _L()
    shapes = [(70, 13, 3, 36), (70, 36, 6, 5), (70, 5, 0, 7), (70, 250, 50, 100), (70, 7, 3, 5), (70, 100, 3, 66)]
    cases = [_Case("gcn", *s[:3], Fo=s[3], seed=i) for i, s in enumerate(shapes)]
    n = 70
    deg = np.random.RandomState(1).randint(0, 5, n)
    rowptr = _up(np.concatenate([[0], np.cumsum(deg)]).astype(np.int32))
    norm1, norm2 = _guarded(n), _guarded(n)
    L.call("txe_gcn_norm", rowptr.data_ptr(), n, norm1.data_ptr(), L.stream_ptr())

    def bufs(c):
        return _nan(n * c.Kp + 1), torch.full_like(c.Wp, float("nan")), torch.full((n, c.Kp // 32), -1, dtype=torch.int32, device=_dev()), _up(c.h)

    def desc(c, b, first):
        return L.GcnPrepareDesc(h=b[3].data_ptr(), ld_h=c.Kh, n_nodes=n, Kh=c.Kh, pos=c.posd.data_ptr() if c.Pd else None, P=_ptr(c.Pdev), Pd=c.Pd, X=b[0].data_ptr(),
                                W=c.Wd.data_ptr(), Fo=c.Fo, Wp=b[1].data_ptr(), drop_p=P_DROP, seed=SEED + (0 if first else 1), mask=b[2].data_ptr(), x_dropped=1,
                                bias_row=None)
    single = [bufs(c) for c in cases]
    for i, (c, b) in enumerate(zip(cases, single)):
        d = desc(c, b, i == 0)
        L.call("txe_gcn_layers_prepare", L.ref(d), 1, None, 0, None, L.stream_ptr())
    for k in (2, 6):
        multi = [bufs(c) for c in cases[:k]]
        arr = (L.GcnPrepareDesc * k)(*[desc(c, b, i == 0) for i, (c, b) in enumerate(zip(cases, multi))])
        norm2.fill_(float("nan"))
        L.call("txe_gcn_layers_prepare", ctypes.addressof(arr), k, rowptr.data_ptr(), n, norm2.data_ptr(), L.stream_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(_take(norm2, n), _take(norm1, n))
        for i, (a, b) in enumerate(zip(single, multi)):
            for t1, t2 in zip(a[:3], b[:3]):
                assert torch.equal(t1.view(torch.int32), t2.view(torch.int32)), (k, i)
            assert bool(torch.isnan(b[0][-1])) and bool(torch.isfinite(b[0][:-1]).all()) and bool(torch.isfinite(b[1]).all())
    c = _Case("gcn", 5, 30, 2, Fo=4)
    X, bias = _nan(5 * 32), _up(np.ones(4, np.float32))
    with pytest.raises(L.TxeError, match="TXE_ERR_ARG"):
        L.call("txe_gcn_layer_prepare", _up(c.h).data_ptr(), 30, 5, 30, c.posd.data_ptr(), c.Pdev.data_ptr(), 2, X.data_ptr(), c.Wd.data_ptr(), 4, c.Wp.data_ptr(), 0.0,
               SEED, None, 0, bias.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(X).all())


@pytest.mark.parametrize("n,Kh,Pd,ld_extra", [(33, 7, 3, 0), (33, 7, 3, 2), (65, 13, 0, 0), (129, 251, 62, 1), (40, 8, 4, 0)])
@pytest.mark.parametrize("h_given", [True, False], ids=["h", "h_null"])
def test_build_x(n, Kh, Pd, ld_extra, h_given):
    """txe_gat_build_x: [h | P[pos] | 0] exactly; odd Kh, odd ld_h, Pd 0; with h == NULL the columns [0, Kh) -- the feature part of the
    straddling quad included -- are untouched; a NaN guard behind X"""
    L = _L()
    c = _Case("gcn", n, Kh, Pd)
    ld_h = Kh + ld_extra
    hb = _nan(n, ld_h)
    hb[:, :Kh] = _up(c.h)
    X = _nan(n * c.Kp + 1)
    L.call("txe_gat_build_x", hb.data_ptr() if h_given else None, ld_h, n, Kh, c.posd.data_ptr() if Pd else None, _ptr(c.Pdev), Pd, X.data_ptr(), L.stream_ptr())
    x = X.cpu().numpy()
    assert np.isnan(x[-1])
    x = x[:-1].reshape(n, c.Kp)
    if h_given:
        assert np.array_equal(x, c.X)
    else:
        assert np.isnan(x[:, :Kh]).all() and np.array_equal(x[:, Kh:], c.X[:, Kh:])


def test_zero_cols():
    """txe_zero_cols: columns [c0, c1) of the first n_rows rows zero, everything else keeps its NaN (ld > c1); c0 == c1 is a no-op"""
    L = _L()
    x = _nan(9, 21)
    L.call("txe_zero_cols", x.data_ptr(), 21, 7, 5, 5, L.stream_ptr())
    assert bool(torch.isnan(x).all())
    L.call("txe_zero_cols", x.data_ptr(), 21, 7, 5, 18, L.stream_ptr())
    a = x.cpu().numpy()
    assert not a[:7, 5:18].any() and np.isnan(a[:7, :5]).all() and np.isnan(a[:7, 18:]).all() and np.isnan(a[7:]).all()
    with pytest.raises(L.TxeError, match="TXE_ERR_ARG"):
        L.call("txe_zero_cols", x.data_ptr(), 21, 7, 6, 5, L.stream_ptr())


@pytest.mark.parametrize("with_t2", [False, True])
def test_gather_add_rows(with_t2):
    """Y[v] = T[row[v]] (+ T2[row2[v]]): bit-equal to the fp32 sum, with repeated row indices and every ld wider than n_cols; a
    misaligned pointer or n_cols % 4 != 0 is TXE_ERR_ARG with no launch"""
    L = _L()
    rs = np.random.RandomState(3)
    n, nt, cols, ld_t, ld_t2, ld_y = 300, 17, 36, 40, 44, 48
    T, T2 = rs.standard_normal((nt, ld_t)).astype(np.float32), rs.standard_normal((VOCAB, ld_t2)).astype(np.float32)
    row, row2 = rs.randint(0, nt, n).astype(np.int32), rs.randint(0, VOCAB, n).astype(np.int32)
    assert len(set(row.tolist())) < n
    Td, T2d, rd, r2d, Y = _up(T), _up(T2), _up(row), _up(row2), _nan(n * ld_y + 1)

    def call(Tp, cols_, Yp):
        return L.call("txe_gather_add_rows", Tp, ld_t, rd.data_ptr(), T2d.data_ptr() if with_t2 else None, ld_t2, r2d.data_ptr() if with_t2 else None, n, cols_, Yp,
                      ld_y, L.stream_ptr())
    for bad in (lambda: call(Td.data_ptr() + 4, cols, Y.data_ptr()), lambda: call(Td.data_ptr(), cols, Y.data_ptr() + 8), lambda: call(Td.data_ptr(), cols - 2, Y.data_ptr())):
        lib = L.load()
        lib.txe_profile_reset()
        lib.txe_profile_enable(1)
        try:
            with pytest.raises(L.TxeError, match="TXE_ERR_ARG"):
                bad()
            assert lib.txe_profile_count() == 0
        finally:
            lib.txe_profile_enable(0)
            lib.txe_profile_reset()
    torch.cuda.synchronize()
    assert bool(torch.isnan(Y).all())
    _rc, names = _profiled(lambda: call(Td.data_ptr(), cols, Y.data_ptr()))
    assert names == ["gather_add_rows_kernel"]
    y = Y.cpu().numpy()
    assert np.isnan(y[-1])
    y = y[:-1].reshape(n, ld_y)
    want = T[row, :cols] + (T2[row2, :cols] if with_t2 else np.float32(0))
    assert np.array_equal(y[:, :cols], want) and np.isnan(y[:, cols:]).all()
