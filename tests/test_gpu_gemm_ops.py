"""The fp32 MFMA GEMM (csrc/txe_gemm.h, txe_gemm_tnlds.h, txe_gemm_{nt,nn,tn}.hip) against FLOAT64 at every edge of gemm_launch_layout's
dispatch, through txe_gemm_plain alone: the test owns every buffer, pitch and pointer offset.  tests/gemm_ref.py restates the dispatch
(vector widths, choose_bn, the k-slices, the tail-split choice, the LDS-direct kernel's eligibility list) and holds the case table;
tests/test_gemm_ref_cpu.py holds the table to the restatement.  The persistent kernel, the reducing epilogues and route bit 8 have
their own files (test_gpu_parity.py, test_gpu_log_partition.py / test_gpu_score_moments.py, test_gpu_split_gemm.py).

Every case: (1) the launches the library profiler records are the restatement's for the device's CU count; (2) the operands are views
inside NaN-filled buffers (NaN in the pitch padding, in front of the first element, behind the last row) and come back unchanged, C is
NaN-filled with a NaN guard: everything outside [M][N] stays NaN, everything inside is finite; (3) max |C - C64| / sum_k |a||b|
(test_gpu_split_gemm.py's measure; C64 = numpy float64 on the same fp32 operands; partial products summed by the test in float64) is at
most max(2 x the same figure of numpy's fp32 product, ABS_FLOOR), and each k-slice alone passes the same gate against its own range --
"[gate] case device yardstick" is printed per case; (4) a second call gives the same bytes.  Tolerance-free beside that: the five
vector-width pairs of one product give one C; a row range and a column range computed alone equal those entries of the whole (at the big
shape the whole runs on 128-wide tiles and the parts on 64-wide ones); route bits 2 and 4 give the bytes of route 0 slice by slice in TN
and NN; a workspace too small for the tail split gives the bytes of no workspace.  Once per layout (and on the LDS-direct kernel) +Inf,
NaN and -Inf beside a ragged k-tail: C's pattern of NaN / +Inf / -Inf is the float64 product's.

Instance -> case (gemm_ref.CASES by name; a name ending in -pitch has an -offset twin that reaches the same instance through a pointer
offset instead of the pitch):
    gemm_kernel<true, true, VA, VB, 64>       nt64-44-pitch, nt64-42-pitch, nt64-24-pitch, nt64-22-pitch, nt64-11-pitch
    gemm_kernel<true, false, VA, VB, 64>      nn64-44-pitch, nn64-42-pitch, nn64-24-pitch, nn64-22-pitch, nn64-11-pitch
    gemm_kernel<false, false, VA, VB, 64>     tn64-44-pitch, tn64-42-pitch, tn64-24-pitch, tn64-22-pitch, tn64-11-pitch
    gemm_kernel<..., VA, VB, 128>             nt128-VAVB, nn128-VAVB, tn128-VAVB (2950 x 1346 x 33), *128-split17 (17 slices)
    gemm_kernel<true, false, 4, 4, 160>       nn160-split (route 4), nn160-one-round (3850 x 2070 x 40, splits 1)
    gemm_kernel<false, false, 4, 4, 160>      tn160-split-route2, tnlds-back-ldc, tnlds-back-c-ptr, tn160-one-round
    gemm_tn_lds_kernel                        tnlds, tnlds-one-element-slice, tnlds-empty-slice, tnlds-two-tiles
    ... and back on gemm_kernel               tnlds-back-a-ptr (2, 4, 64), tnlds-back-ldb (4, 2, 64), tnlds-back-ldc, tnlds-back-c-ptr,
                                              tn160-split-route2 (4, 4, 160)
    gemm_tail_fixup_kernel<64>                nt-tail64, nn-tail64, tn-tail64, nt-tail-k255
    gemm_tail_fixup_kernel<128>               nt-tail128, nn-tail128, tn-tail128 (641 x 600 x 2048: 30 tiles in 16 slices)
    no tail split                             nt-tail-k224 (seven k-tiles), nn-tail-short-ws, tn-tail128-short-ws
    split-K edges                             {nt,nn,tn}-split-short-last, -one-element, -empty-slice, -auto (choose_splits)
    empty products                            {nt,nn,tn}-k0 (C = 0), nt-m0, tn-n0, nn-m0-split (nothing launched)
K = 255 has EIGHT k-tiles (the last one ragged), so gemm_launch_layout's rule nkt / 4 >= 2 cuts it into two slices of four like K = 256;
the first reduction that is one k-tile short is K = 224 (nt-tail-k224).

The 64-wide and the 128-wide instances DO agree bit for bit (every element is one chain of v_mfma_f32_32x32x2_f32 in k order whatever
the tile), so that comparison is kept (test_ranges_alone_equal_the_whole at the big shape).

What the file found: a row-contiguous operand (B of NN, both of TN) whose column count is no multiple of its vector width -- N = 130 under
16-byte loads, N = 65 under 8-byte ones -- took the hoisted fast loader on its ragged last tile, where the vector that straddles the
operand's edge was read from column 0 instead: wrong values in up to three valid rows / columns of C from the first whole k-tile on.
block_is_plain now leaves such a tile to the generic loader.  gemm_tn_lds_kernel multiplied zeroed A rows of a slice's ragged last
k-tile against B's re-read last row: 0 x Inf = NaN where gemm_kernel gives Inf; it zeroes B's rows as well now.

Measured on the MI355X (max |C - C64| / sum_k |a||b|; largest device figure per group, numpy's fp32 product beside it; the floor is 6e-7
and no case needed more than it):
    64-wide tiles (27 cases)                  2.7e-7 against 2.7e-7 (nn64-44-pitch); largest ratio 1.4 (nn64-24-pitch, 7.3e-8 against 5.2e-8)
    128-wide tiles, K = 33 (15 cases)         3.2e-7 against 3.1e-7
    160-wide tiles at splits 1                3.8e-7 against 3.4e-7 (nn160-one-round)
    single k-slices (98 gates)                3.5e-7 against 2.8e-7 (nt128-split17[8]); largest ratio 1.4
    split-K sums                              2.4e-7 against 2.5e-7
    tail splitting, K = 2048                  2.7e-7 against 7.8e-8 (tn-tail128-short-ws, plain k order: 3.5 x numpy's blocked sum, under the
                                              floor); with the 16 slices 4.6e-8
    special values (the finite rest)          2.1e-7 against 2.0e-7
The 109 cases take 4 s on the MI355X, none more than 0.2 s.
"""
import numpy as np
import pytest
import torch

import gemm_ref as gr
from gemm_ref import NN, NT, TN
from test_gpu_readout_match_ops import _profiled
from test_gpu_split_gemm import ABS_FLOOR

pytestmark = pytest.mark.gpu

TXE_ERR_ARG, TXE_ERR_WORKSPACE = "TXE_ERR_ARG", "TXE_ERR_WORKSPACE"


def _dev():
    return torch.device("cuda:0")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _up(buf):
    t = torch.from_numpy(buf).to(_dev())
    assert t.data_ptr() % 256 == 0                       # (the specs' offsets alone decide the pointers' alignment)
    return t


_WS = {}


def _ws():
    """the tail-splitting workspace, NaN-filled before every call"""
    from taxoexpan_amd import _lib
    if not _WS:
        nb = _lib.call("txe_gemm_tail_ws_bytes")
        assert nb == gr.tail_ws_bytes(_cus())
        _WS["t"] = torch.empty(nb // 4, dtype=torch.float32, device=_dev())
    _WS["t"].fill_(float("nan"))
    return _WS["t"]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


class _Run:
    """one case on the device: the operands uploaded once, call() = one txe_gemm_plain into a fresh NaN-filled C"""

    def __init__(self, cs, a=None, b=None, seed=0):
        self.cs, self.plan = cs, gr.plan(cs, _cus())
        if a is None:
            a, b = gr.logical(cs.M, cs.N, cs.K, seed)
        assert a.shape == (cs.M, cs.K) and b.shape == (cs.K, cs.N)            # (the kernels read what the case says, not what the arrays hold)
        self.a, self.b = a, b
        self.ops = gr.operands(cs, a, b)
        self.g = self.ops["g"]
        self.Ad, self.Bd = _up(self.ops["A"]), _up(self.ops["B"])

    def call(self, profiled=False, route=None):
        from taxoexpan_amd import _lib
        cs, p, g = self.cs, self.plan, self.g
        cbuf, cfirst = gr.c_buffer(cs, p.splits)
        Cd = _up(cbuf)
        ws = _ws() if cs.ws != "none" else None
        args = (cs.layout, self.Ad.data_ptr() + 4 * self.ops["a_first"], g.lda, self.Bd.data_ptr() + 4 * self.ops["b_first"], g.ldb,
                Cd.data_ptr() + 4 * cfirst, g.ldc, cs.M, cs.N, cs.K, p.splits, cs.route if route is None else route,
                ws.data_ptr() if ws is not None else None, p.ws_bytes, _lib.stream_ptr())
        if profiled:
            _rc, names = _profiled(lambda: _lib.call("txe_gemm_plain", *args))
        else:
            _lib.call("txe_gemm_plain", *args)
            names = None
        torch.cuda.synchronize()
        out = Cd.cpu().numpy()
        body, outside = gr.c_views(out, cfirst, cs, p.splits)
        return body, outside, names

    def product(self, route=None):
        """C [splits][M][N] after the poison checks"""
        body, outside, _ = self.call(route=route)
        assert np.isnan(outside).all()
        return np.ascontiguousarray(body[:, :, :self.cs.N])

    def operands_unchanged(self):
        return np.array_equal(_bits(self.Ad.cpu().numpy()), _bits(self.ops["A"])) and np.array_equal(_bits(self.Bd.cpu().numpy()), _bits(self.ops["B"]))


def _gate(what, got, a64, b64, a32, b32):
    """the accuracy gate of one product: (device figure, yardstick figure); asserts"""
    c64 = a64 @ b64
    scale = np.abs(a64) @ np.abs(b64)
    e_dev, e_yard = gr.measure(got, c64, scale), gr.measure(a32 @ b32, c64, scale)
    print(f"[gate] {what} {e_dev:.3e} {e_yard:.3e}")
    assert e_dev <= max(2.0 * e_yard, ABS_FLOOR), (what, e_dev, e_yard)
    return e_dev, e_yard


def test_the_table_reaches_every_instance_on_this_device():
    """gemm_ref.CASES planned for the device's own CU count: with the MI355X's 256 every instance has its case (on another count the
    cases still assert their own names, the coverage is the CPU test's)"""
    if _cus() != 256:
        return
    from test_gemm_ref_cpu import ALL_LAUNCHES
    assert {n for cs in gr.CASES for n in gr.plan(cs, 256).names} == ALL_LAUNCHES


@pytest.mark.parametrize("name", [c.name for c in gr.CASES])
def test_case_against_float64(name):
    cs = gr.BY_NAME[name]
    run = _Run(cs)
    p = run.plan
    body, outside, names = run.call(profiled=True)
    assert names == p.names, (names, p)                                        # 1. the intended instance ran, and nothing else
    assert np.isnan(outside).all()                                             # 2. nothing stored outside [M][N], guard and front intact
    got = body[:, :, :cs.N]
    assert np.isfinite(got).all()                                              #    and none of the NaN around the operands got in
    assert run.operands_unchanged()
    if cs.M == 0 or cs.N == 0:
        assert np.isnan(body).all()
        return
    a64, b64 = run.a.astype(np.float64), run.b.astype(np.float64)
    if cs.K == 0:
        assert not _bits(got).any()                                            # the empty sum: +0.0
    for z, (lo, hi) in enumerate(p.slices if p.splits > 1 else []):            # 3. each k-slice against its own range
        if hi <= lo:
            assert not _bits(got[z]).any(), (name, z)                          # an empty slice is stored as zeros: the caller adds them all
        else:
            _gate(f"{name}[{z}]", got[z], a64[:, lo:hi], b64[lo:hi], run.a[:, lo:hi], run.b[lo:hi])
    _gate(name, got.astype(np.float64).sum(0), a64, b64, run.a, run.b)
    again, outside2, _ = run.call()                                            # 4. repeatable
    assert np.array_equal(_bits(again), _bits(body)) and np.isnan(outside2).all()
    if "unsplit" in cs.tags:                                                   # a workspace that cannot hold the slices: the route without one
        bare = _Run(cs._replace(ws="none"), run.a, run.b)
        if bare.plan.bn == p.bn:
            assert bare.plan.names == p.names
        assert np.array_equal(_bits(bare.product()), _bits(got))


# ---- bit invariance: with no workspace and splits == 1 every element is one chain in k order ---------------------------------------------
@pytest.mark.parametrize("shape", ["small", "big"])
@pytest.mark.parametrize("layout", [NT, NN, TN], ids=["nt", "nn", "tn"])
def test_vector_widths_give_one_result(layout, shape):
    """the same product laid out for each of the five vector-width pairs (through the pitch and through a pointer offset)"""
    M, N, K = (130, 131, 67) if shape == "small" else gr.BIG
    a, b = gr.logical(M, N, K, 1)
    first, seen = None, set()
    for pair, specs in gr.VEC_SPECS.items():
        for sa, sb in specs if shape == "small" else specs[-1:]:
            run = _Run(gr.case("w", layout, M, N, K, sa, sb, "p4"), a, b)
            assert (run.plan.va, run.plan.vb) == pair
            seen.add(run.plan.names[0])
            c = run.product()
            first = c if first is None else first
            assert np.array_equal(_bits(c), _bits(first)), (pair, sa, sb)
    assert len(seen) == 5
    _gate(f"widths-{gr.LAYOUT_NAME[layout]}-{shape}", first[0], a.astype(np.float64), b.astype(np.float64), a, b)


@pytest.mark.parametrize("shape", ["small", "big"])
@pytest.mark.parametrize("layout", [NT, NN, TN], ids=["nt", "nn", "tn"])
def test_ranges_alone_equal_the_whole(layout, shape):
    """a row range and a column range of the product computed alone; at the big shape the whole is on 128-wide tiles and the parts on
    64-wide ones (on 256 CUs)"""
    M, N, K = (130, 131, 67) if shape == "small" else gr.BIG
    a, b = gr.logical(M, N, K, 2)
    whole_run = _Run(gr.case("whole", layout, M, N, K), a, b)
    whole = whole_run.product()[0]
    r0, c0, mc = M // 2 + 1, N // 3, min(M, 200)
    r1, c1 = min(M, r0 + 70), min(N, c0 + 129)
    rows = _Run(gr.case("rows", layout, r1 - r0, N, K, "p2", "p4"), a[r0:r1], b)
    cols = _Run(gr.case("cols", layout, mc, c1 - c0, K, "p4", "o8", "p1"), a[:mc], b[:, c0:c1])
    if shape == "big" and _cus() == 256:
        assert whole_run.plan.bn == 128 and rows.plan.bn == 64 and cols.plan.bn == 64
    assert np.array_equal(_bits(rows.product()[0]), _bits(whole[r0:r1]))
    assert np.array_equal(_bits(cols.product()[0]), _bits(whole[:cols.cs.M, c0:c1]))


@pytest.mark.parametrize("layout,M,N,K,S", [(TN, 132, 170, 70, 2), (TN, 300, 316, 1000, 3), (NN, 130, 200, 100, 3), (NN, 129, 322, 161, 2)],
                         ids=["tn-2", "tn-3", "nn-3", "nn-2"])
def test_route_bits_give_the_bytes_of_route_0(layout, M, N, K, S):
    """route 4 (128 x 160 tiles: gemm_tn_lds_kernel in TN, gemm_kernel<true, false, 4, 4, 160> in NN) and route 4 | 2 (TN on
    gemm_kernel<false, false, 4, 4, 160>) against route 0 (64- or 128-wide tiles), slice by slice"""
    a, b = gr.logical(M, N, K, 3)
    outs, names = {}, {}
    for route in (0, 4, 6):
        run = _Run(gr.case("r", layout, M, N, K, splits=S, route=route), a, b)
        names[route] = run.plan.names
        outs[route] = run.product()
        _b, _o, got_names = run.call(profiled=True)
        assert got_names == run.plan.names
    wide = "gemm_kernel<true, false, 4, 4, 160>" if layout == NN else "gemm_kernel<false, false, 4, 4, 160>"
    assert names[4] == (["gemm_tn_lds_kernel"] if layout == TN else [wide]) and names[6] == [wide] and names[0] != names[6]
    assert np.array_equal(_bits(outs[4]), _bits(outs[0])) and np.array_equal(_bits(outs[6]), _bits(outs[0]))


# ---- IEEE special values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,splits,route", [(NT, 1, 0), (NN, 1, 0), (TN, 1, 0), (TN, 2, 4), (TN, 2, 6), (NN, 2, 4)],
                         ids=["nt", "nn", "tn", "tn-lds", "tn-160", "nn-160"])
def test_special_values_propagate_like_float64(layout, splits, route):
    """row 5 of a holds +Inf and column 9 of b holds -Inf, both at the LAST k (beside the zero-filled rest of a ragged k-tile: a tail
    that is multiplied against them instead of selected away makes NaN), row 77 of a holds a NaN; O(1) otherwise"""
    M, N, K = 131, 70, 67
    a, b = gr.logical(M, N, K, 4)
    a[5, K - 1], a[77, 11], b[K - 1, 9] = np.inf, np.nan, -np.inf
    run = _Run(gr.case("ieee", layout, M, N, K, "p4", "p4", "p4", splits=splits, route=route), a, b)
    with np.errstate(invalid="ignore"):
        got = run.product().astype(np.float64).sum(0)
        c64 = a.astype(np.float64) @ b.astype(np.float64)
    for what, f in (("nan", np.isnan), ("+inf", lambda x: x == np.inf), ("-inf", lambda x: x == -np.inf)):
        assert np.array_equal(f(got), f(c64)), (what, np.argwhere(f(got) != f(c64))[:8])
    assert np.isnan(c64[77]).all() and np.isinf(c64[5]).all() and c64[5, 9] == -np.inf                # (the pattern is the intended one)
    keep_r, keep_c = np.setdiff1d(np.arange(M), [5, 77]), np.setdiff1d(np.arange(N), [9])
    a_, b_ = a[keep_r], b[:, keep_c]
    _gate(f"ieee-{gr.LAYOUT_NAME[layout]}-{splits}-{route}", got[np.ix_(keep_r, keep_c)], a_.astype(np.float64), b_.astype(np.float64), a_, b_)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from taxoexpan_amd import _lib
    lib = _lib.load()
    M, N, K = 40, 24, 48
    A, B = _up(np.ones(M * K, np.float32)), _up(np.ones(N * K, np.float32))
    C = torch.full((2 * M * N + 8,), float("nan"), device=_dev())
    need = _lib.call("txe_gemm_plain_split_ws_bytes", M, N, K)
    ws = torch.empty(need, dtype=torch.uint8, device=_dev())
    ok = dict(layout=0, A=A.data_ptr(), lda=K, B=B.data_ptr(), ldb=K, C=C.data_ptr(), ldc=N, M=M, N=N, K=K, splits=1, route=0,
              ws=None, wsb=0)
    bad = [("layout 3", dict(layout=3), TXE_ERR_ARG), ("M < 0", dict(M=-1), TXE_ERR_ARG), ("N < 0", dict(N=-1), TXE_ERR_ARG),
           ("K < 0", dict(K=-1), TXE_ERR_ARG), ("A null", dict(A=None), TXE_ERR_ARG), ("B null", dict(B=None), TXE_ERR_ARG),
           ("C null", dict(C=None), TXE_ERR_ARG), ("route 16", dict(route=16), TXE_ERR_ARG),
           ("route 8, layout 1", dict(route=8, layout=1, ws=ws.data_ptr(), wsb=need), TXE_ERR_ARG),
           ("route 8, splits 2", dict(route=8, splits=2, ws=ws.data_ptr(), wsb=need), TXE_ERR_ARG),
           ("route 8, workspace one byte short", dict(route=8, ws=ws.data_ptr(), wsb=need - 1), TXE_ERR_WORKSPACE)]
    lib.txe_profile_reset()
    lib.txe_profile_enable(1)
    try:
        for what, change, code in bad:
            v = dict(ok, **change)
            with pytest.raises(_lib.TxeError, match=code):
                _lib.call("txe_gemm_plain", v["layout"], v["A"], v["lda"], v["B"], v["ldb"], v["C"], v["ldc"], v["M"], v["N"], v["K"], v["splits"],
                          v["route"], v["ws"], v["wsb"], _lib.stream_ptr())
            torch.cuda.synchronize()
            assert lib.txe_profile_count() == 0, what
    finally:
        lib.txe_profile_enable(0)
        lib.txe_profile_reset()
    assert bool(torch.isnan(C).all())
