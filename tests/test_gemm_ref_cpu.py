"""tests/gemm_ref.py without a GPU: on 256 CUs its case table reaches every gemm_kernel instance, both 160-wide ones, the LDS-direct
kernel and both fix-up kernels; every reason that takes a TN product away from the LDS-direct kernel has exactly one case; the restated
k-slices tile [0, K); the operand builder poisons what it says it poisons; and the accuracy floor of tests/test_gpu_gemm_ops.py lies
above what an fp32 product summed in plain k order shows under its measure."""
import numpy as np
import pytest

import gemm_ref as gr
from gemm_ref import NN, NT, TN
from test_gpu_split_gemm import ABS_FLOOR

_TF = ("true", "false")
GEMM_KERNELS = {f"gemm_kernel<{_TF[not ak]}, {_TF[not bkc]}, {va}, {vb}, {bn}>"
                for ak, bkc in gr.KCONTIG.values() for va, vb in gr.VEC_PAIRS for bn in (64, 128)}
WIDE_KERNELS = {"gemm_kernel<true, false, 4, 4, 160>", "gemm_kernel<false, false, 4, 4, 160>"}
SPECIAL = {"gemm_tn_lds_kernel", "gemm_tail_fixup_kernel<64>", "gemm_tail_fixup_kernel<128>"}
ALL_LAUNCHES = GEMM_KERNELS | WIDE_KERNELS | SPECIAL


def _plans(cus=gr.CUS):
    return {c.name: gr.plan(c, cus) for c in gr.CASES}


def test_every_instance_has_its_case():
    assert len(GEMM_KERNELS) == 30
    plans = _plans()
    reached = {}
    for name, p in plans.items():
        for n in p.names:
            reached.setdefault(n, []).append(name)
    assert set(reached) == ALL_LAUNCHES, (ALL_LAUNCHES - set(reached), set(reached) - ALL_LAUNCHES)
    # ... and would be missed: every launch name but the few that many cases share is reached by a case that is NAMED after it
    for layout, lname in gr.LAYOUT_NAME.items():
        ak, bkc = gr.KCONTIG[layout]
        for va, vb in gr.VEC_PAIRS:
            k = f"gemm_kernel<{_TF[not ak]}, {_TF[not bkc]}, {va}, {vb}, "
            assert f"{lname}64-{va}{vb}-pitch" in reached[k + "64>"] and f"{lname}128-{va}{vb}" in reached[k + "128>"]
            if (va, vb) != (4, 4):                                             # both ways to the vector width
                assert f"{lname}64-{va}{vb}-offset" in reached[k + "64>"]
    for lname in gr.LAYOUT_NAME.values():                                      # tail splitting: every layout at both fix-up widths
        assert plans[f"{lname}-tail64"].names[1:] == ["gemm_tail_fixup_kernel<64>"] and plans[f"{lname}-tail128"].names[1:] == ["gemm_tail_fixup_kernel<128>"]
    for c in gr.CASES:
        if "unsplit" in c.tags:
            assert len(plans[c.name].names) == 1 and plans[c.name].S == 0 and c.ws != "none", c.name
    assert plans["nt-tail-k255"].S == 2 and plans["nt-tail-k224"].S == 0       # ceil(255 / 32) = 8 k-tiles: two slices of four; 7: none
    assert plans["nn160-one-round"].names == ["gemm_kernel<true, false, 4, 4, 160>"] and plans["nn160-one-round"].splits == 1
    assert plans["nn160-split"].names == ["gemm_kernel<true, false, 4, 4, 160>"] and plans["tn160-split-route2"].names == ["gemm_kernel<false, false, 4, 4, 160>"]


def test_vector_widths_both_ways():
    """gcd_vec / ptr_vec / the collapse, and the specs of the table: the pitch residues 0, 2, 1 and pointer offsets of 8 and 4 bytes"""
    assert [gr.gcd_vec(x) for x in (0, 4, 6, 7, 8)] == [4, 4, 2, 1, 4] and [gr.ptr_vec(x) for x in (0, 16, 8, 24, 4, 12)] == [4, 4, 2, 2, 1, 1]
    assert gr.vec_pair(8, 0, 8, 0) == (4, 4) and gr.vec_pair(8, 8, 6, 0) == (2, 2) and gr.vec_pair(8, 0, 7, 0) == (1, 1) and gr.vec_pair(8, 4, 8, 0) == (1, 1)
    for spec, res, off in (("p4", 0, 0), ("p2", 2, 0), ("p1", 1, 0), ("o8", 0, 2), ("o4", 0, 1)):
        for cols in (0, 1, 31, 64, 65, 130):
            ld, o = gr.pitch(spec, cols)
            assert ld > cols and (ld % 4 == res or (res == 1 and ld % 2 == 1)) and o == off
    for (va, vb), specs in gr.VEC_SPECS.items():
        for a, b in specs:
            c = gr.case("x", NT, 10, 10, 10, a, b)
            p = gr.plan(c)
            assert (p.va, p.vb) == (va, vb)
    ways = {(c.a, c.b) for c in gr.CASES}
    assert ways >= {s for specs in gr.VEC_SPECS.values() for s in specs}


def test_edges_of_the_shape_are_in_the_table():
    for what, pred in gr.EDGES.items():
        assert any(pred(c) for c in gr.CASES), what
    for c in gr.CASES:                                                         # the shapes past 600 x 600 x 2100 are the ones the table says
        if c.M > 600 or c.N > 600 or c.K > 2100:
            assert (c.M, c.N, c.K) in (gr.BIG, gr.WIDE, gr.TAIL128, gr.BIG_SPLIT[:3]), c.name
    # row-contiguous operands with a vector that straddles the operand's edge and a whole k-tile in front of it
    assert any(c.layout != NT and gr.plan(c).vb > 1 and c.N % gr.plan(c).vb and c.K >= 32 for c in gr.CASES)
    assert any(c.layout == TN and gr.plan(c).va > 1 and c.M % gr.plan(c).va and c.K >= 32 for c in gr.CASES)


def test_choose_bn_on_the_tables_own_shapes():
    """the arithmetic the table's comments state, on 256 CUs"""
    M, N, K = gr.BIG
    assert ((M + 127) // 128) * ((N + 63) // 64) == 528 and ((M + 127) // 128) * ((N + 127) // 128) == 264
    M, N, K = gr.WIDE
    assert ((M + 127) // 128) * ((N + 159) // 160) == 403 and ((M + 127) // 128) * ((N + 127) // 128) == 527
    M, N, K = gr.TAIL128
    p = gr.plan(gr.BY_NAME["nt-tail128"])
    assert p.bn == 128 and p.S == 16 and gr.plan(gr.case("x", NT, 640, N, K, ws="full")).bn == 64
    # on a device with fewer CUs the same cases plan other launches: the restatement follows the count
    assert gr.plan(gr.BY_NAME["nt128-44"], 512).bn == 64


def test_lds_fallback_reasons_have_one_case_each():
    single = {}
    for c in gr.CASES:
        p = gr.plan(c)
        if p.lds_reasons:
            assert p.names != ["gemm_tn_lds_kernel"]
            if len(p.lds_reasons) == 1:
                single.setdefault(p.lds_reasons[0], []).append(c.name)
    assert {k: len(v) for k, v in single.items()} == {"a_ptr": 1, "ldb": 1, "ldc": 1, "c_ptr": 1, "route2": 1}, single
    lds = [c for c in gr.CASES if gr.plan(c).names == ["gemm_tn_lds_kernel"]]
    assert {gr.plan(c).splits for c in lds} >= {2, 4} and any(hi <= lo for c in lds for lo, hi in gr.plan(c).slices)


def test_slices_cover_the_reduction_once():
    assert gr.slice_bounds(33, 2) == (32, [(0, 32), (32, 33)]) and gr.slice_bounds(65, 4)[1] == [(0, 32), (32, 64), (64, 65), (65, 65)]
    assert gr.slice_bounds(0, 1) == (32, [(0, 0)]) and gr.slice_bounds(200, 3) == (96, [(0, 96), (96, 192), (192, 200)])
    kinds = set()
    for c in gr.CASES:
        p = gr.plan(c)
        spans = p.slices if p.splits > 1 else (gr.tail_slices(c) if p.S else [])
        if not spans:
            continue
        assert len(spans) == (p.splits if p.splits > 1 else p.S) and p.ksplit % 32 == 0
        k = 0
        for lo, hi in spans:                                                   # contiguous, in order, nothing twice
            assert lo == min(k, c.K) and hi >= lo
            k = hi
        assert k == c.K, c.name
        lens = [hi - lo for lo, hi in spans]
        kinds |= {"short last"} if 0 < lens[-1] < lens[0] else set()
        kinds |= {"one element"} if 1 in lens else set()
        kinds |= {"empty"} if 0 in lens else set()
    assert kinds == {"short last", "one element", "empty"}
    auto = [c for c in gr.CASES if c.splits == "auto"]
    assert {c.layout for c in auto} == {NT, NN, TN} and all(gr.plan(c).splits == 8 for c in auto)      # choose_splits(128, 96, 2000) on 512 slots


def test_operand_builder_poisons_around_the_view():
    for c in (gr.BY_NAME["nn64-22-offset"], gr.BY_NAME["tn64-11-pitch"], gr.BY_NAME["nt-k0"], gr.BY_NAME["tn-k0"]):
        a, b = gr.logical(c.M, c.N, c.K)
        o = gr.operands(c, a, b)
        g = o["g"]
        for buf, first, (rows, cols), ld, off in ((o["A"], o["a_first"], gr.operand_shapes(c)[0], g.lda, g.a_off),
                                                  (o["B"], o["b_first"], gr.operand_shapes(c)[1], g.ldb, g.b_off)):
            assert first == gr.FRONT + off and np.isnan(buf[:first]).all() and np.isnan(buf[first + rows * ld:]).all() and buf.size - first - rows * ld == gr.GUARD
            body = buf[first:first + rows * ld].reshape(rows, ld)
            assert np.isfinite(body[:, :cols]).all() and np.isnan(body[:, cols:]).all() and (ld > cols)
        A = o["A"][o["a_first"]:o["a_first"] + gr.operand_shapes(c)[0][0] * g.lda].reshape(-1, g.lda)[:, :gr.operand_shapes(c)[0][1]]
        assert np.array_equal(A if c.layout != TN else A.T, a)
        buf, first = gr.c_buffer(c, 2)
        body, outside = gr.c_views(buf, first, c, 2)
        assert body.shape == (2, c.M, g.ldc) and outside.size == buf.size - 2 * c.M * c.N
    a1, b1 = gr.logical(5, 6, 7)
    a2, b2 = gr.logical(5, 6, 7)
    assert np.array_equal(a1, a2) and np.array_equal(b1, b2) and not np.array_equal(a1, gr.logical(5, 6, 7, 1)[0])


def test_floor_lies_above_an_fp32_product_in_k_order():
    """max |c - c64| / sum_k |a||b| of 4,000 fp32 dot products summed in k order (one rounded product, one rounded sum per k), at K = 33
    and at the table's largest K: 1.7e-7 .. 2.3e-7 up to K = 4000; numpy's own fp32 product (pairwise / blocked sums) about 1e-7"""
    kmax = max(c.K for c in gr.CASES)
    assert kmax == 2048
    rs = np.random.RandomState(5)
    for K in (33, kmax):
        a, b = rs.standard_normal((4000, K)).astype(np.float32), rs.standard_normal((4000, K)).astype(np.float32)
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        c64, scale = (a64 * b64).sum(1), (np.abs(a64) * np.abs(b64)).sum(1)
        e_k = gr.measure(gr.k_order_fp32(a, b), c64, scale)
        e_np = gr.measure(np.einsum("ik,ik->i", a, b), c64, scale)
        print(f"[floor] K {K} k-order {e_k:.3e} numpy {e_np:.3e}")
        assert e_k < ABS_FLOOR / 2 and e_np < ABS_FLOOR / 2
