"""The fp32 MFMA GEMM's host-side dispatch (csrc/txe_gemm.h: gemm_launch_layout, csrc/txe_gemm_tn.hip: gemm_tn_lds_launch, csrc/txe_match.hip:
txe_gemm_plain) restated in plain Python with the CU count as a parameter, an operand builder that puts every operand inside a NaN-filled
buffer, and the case table of tests/test_gpu_gemm_ops.py.  Nothing here needs a GPU: tests/test_gemm_ref_cpu.py holds the table to the
restatement (every kernel instance has its case) and the restatement to its own arithmetic.

For a case, plan() gives the launch names the library profiler must record, spelled as gemm_launch_v prints them
("gemm_kernel<true, false, 2, 4, 64>", "gemm_tail_fixup_kernel<64>", "gemm_tn_lds_kernel").  choose_bn and choose_splits are the
restatements of tests/dense_layer_ref.py (held to the source by that file's tests), called with this file's slot count.

A case names, per operand, HOW its vector width comes about:
    "p4"  pitch = 0 mod 4, pointer 16-byte aligned                  -> 4 floats per load
    "p2"  pitch = 2 mod 4                                           -> 2
    "p1"  odd pitch                                                 -> 1 (and the other operand drops to 1 with it)
    "o8"  pitch = 0 mod 4, pointer 8 bytes past a 16-byte boundary  -> 2
    "o4"  pitch = 0 mod 4, pointer 4 bytes past a 16-byte boundary  -> 1
    "c"   contiguous (pitch = columns), aligned                     -> whatever the column count gives (C only)
Every pitch but "c" is larger than the column count: there is NaN between the rows, in front of the first element and behind the last."""
from collections import namedtuple

import numpy as np

from dense_layer_ref import BK, BM, THREADS, choose_bn, choose_splits, round_up

CUS = 256
NT, NN, TN = 0, 1, 2
LAYOUT_NAME = {NT: "nt", NN: "nn", TN: "tn"}
KCONTIG = {NT: (True, True), NN: (True, False), TN: (False, False)}        # (AK, BKC) of gemm_launch_layout<AK, BKC>
ROUTE_NO_PERSIST, ROUTE_NO_TN_LDS, ROUTE_FORCE_BN160, ROUTE_BF16_PIPE = 1, 2, 4, 8
FRONT = 4            # NaN floats in front of every view (a multiple of 4: the pointer's alignment is the spec's offset alone)
GUARD = 64           # NaN floats behind every view


# ---- vector widths ----------------------------------------------------------------------------------------------------------------------------
def gcd_vec(x):
    """gcd_vec (txe_gemm.h)"""
    return 4 if x % 4 == 0 else (2 if x % 2 == 0 else 1)


def ptr_vec(addr):
    """ptr_vec (txe_gemm.h): addr in bytes"""
    return 4 if addr % 16 == 0 else (2 if addr % 8 == 0 else 1)


def vec_pair(lda, a_addr, ldb, b_addr):
    """vmat_vec of two plain operands and gemm_launch_layout's collapse: any 1 makes both 1"""
    va, vb = min(gcd_vec(lda), ptr_vec(a_addr)), min(gcd_vec(ldb), ptr_vec(b_addr))
    return (1, 1) if va == 1 or vb == 1 else (va, vb)


def pitch(spec, cols):
    """the smallest pitch of the spec's residue that leaves padding behind `cols` columns, and the view's offset in floats"""
    if spec == "c":
        return cols, 0
    if spec in ("p4", "o8", "o4"):
        return round_up(cols, 4) + 4, {"p4": 0, "o8": 2, "o4": 1}[spec]
    if spec == "p2":
        return round_up(cols + 1, 4) + 2, 0
    assert spec == "p1", spec
    return round_up(cols + 1, 2) + 1, 0


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------
# ws: "none" | "full" (txe_gemm_tail_ws_bytes()) | "short" (one partial tile less than the tail split of this case needs)
# splits: an int, or "auto" = choose_splits(M, N, K) of the device
Case = namedtuple("Case", "name layout M N K a b c splits route ws tags")


def case(name, layout, M, N, K, a="p4", b="p4", c="p4", splits=1, route=0, ws="none", tags=()):
    return Case(name, layout, M, N, K, a, b, c, splits, route, ws, tuple(tags))


def operand_shapes(cs):
    """(rows, cols) of A and B as stored: NT A[M][K] B[N][K], NN A[M][K] B[K][N], TN A[K][M] B[K][N]"""
    a = (cs.M, cs.K) if cs.layout != TN else (cs.K, cs.M)
    b = (cs.N, cs.K) if cs.layout == NT else (cs.K, cs.N)
    return a, b


Geometry = namedtuple("Geometry", "lda a_off ldb b_off ldc c_off")


def geometry(cs):
    (_ra, ca), (_rb, cb) = operand_shapes(cs)
    lda, ao = pitch(cs.a, ca)
    ldb, bo = pitch(cs.b, cb)
    ldc, co = pitch(cs.c, cs.N)
    return Geometry(lda, ao, ldb, bo, ldc, co)


def splits_of(cs, cus=CUS):
    return choose_splits(cs.M, cs.N, cs.K, 2 * cus) if cs.splits == "auto" else cs.splits


def slice_bounds(K, splits):
    """gemm_launch_layout's ksplit (the slice length rounded up to whole k-tiles, 32 for an empty product) and the k range of every slice
    as gemm_kernel clips it: [z ksplit, min(K, (z + 1) ksplit)), empty where it starts at or behind K"""
    splits = max(splits, 1)
    ksplit = round_up((K + splits - 1) // splits, BK) or BK
    return ksplit, [(min(K, z * ksplit), min(K, (z + 1) * ksplit)) for z in range(splits)]


def tail_ws_bytes(cus=CUS):
    """gemm_tail_ws_bytes (txe_gemm.h)"""
    return 2 * cus * (BM * 128 + THREADS) * 4


def tail_need(M, N, K, bn, cus=CUS):
    """the tail-split choice of gemm_launch_layout at splits == 1 with a workspace pointer: (S, bytes the partial tiles take); S < 2 = none"""
    slots = 2 * cus
    tiles = ((M + BM - 1) // BM) * ((N + bn - 1) // bn)
    r = tiles % slots
    nkt = (K + BK - 1) // BK
    S = min(slots // r if r else 0, nkt // 4, 16)
    return S, r * S * BM * bn * 4


Plan = namedtuple("Plan", "names va vb bn splits ksplit slices S ws_bytes lds_reasons")


def plan(cs, cus=CUS):
    """what txe_gemm_plain must do with the case on a device of `cus` compute units (route bit 8 is not restated: tests/test_gpu_split_gemm.py)"""
    assert 0 <= cs.route < 8 and cs.layout in KCONTIG
    g = geometry(cs)
    ak, bkc = KCONTIG[cs.layout]
    slots = 2 * cus
    splits = max(splits_of(cs, cus), 1)
    va, vb = vec_pair(g.lda, 4 * g.a_off, g.ldb, 4 * g.b_off)
    ksplit, slices = slice_bounds(cs.K, splits)
    M, N, K = cs.M, cs.N, cs.K
    if M <= 0 or N <= 0:
        return Plan([], va, vb, 0, splits, ksplit, slices, 0, 0, [])
    allow160 = (not bkc) and va == 4 and vb == 4                      # (txe_gemm_plain's epilogue is plain)
    tail_split = cs.ws != "none"
    bn = choose_bn(M, N, splits, tail_split, K, allow160, bool(cs.route & ROUTE_FORCE_BN160), slots)
    # the reasons a split-K TN product that asks for 128 x 160 tiles is not gemm_tn_lds_kernel's: what takes the 160-wide tiles away
    # (allow160), then gemm_tn_lds_launch's own list
    reasons = []
    if cs.layout == TN and splits > 1 and (cs.route & ROUTE_FORCE_BN160):
        reasons += [w for w, bad in (("a_ptr", (4 * g.a_off) % 16), ("lda", g.lda % 4), ("b_ptr", (4 * g.b_off) % 16), ("ldb", g.ldb % 4)) if bad]
        reasons += [w for w, bad in (("route2", cs.route & ROUTE_NO_TN_LDS), ("k0", K < 1), ("ldc", g.ldc % 4), ("c_ptr", (4 * g.c_off) % 16)) if bad]
    # gemm_persist_kernel: whole rounds of a plain short-K product (two rounds of tiles at least) -- not this table's subject
    if (splits == 1 and cs.ws != "none" and va == 4 and vb == 4 and N > 64 and not (cs.route & ROUTE_NO_PERSIST) and K % BK == 0 and 5 * BK <= K <= 512):
        ntiles = ((M + BM - 1) // BM) * ((N + 127) // 128)
        assert ntiles // slots < 2, f"{cs.name}: reaches the persistent kernel, which tests/test_gpu_parity.py pins"
    S, ws_bytes = 0, 0
    if cs.ws != "none":
        ws_bytes = tail_ws_bytes(cus)
        if splits == 1:
            S, need = tail_need(M, N, K, bn, cus)
            if cs.ws == "short":
                assert S >= 2 and need <= ws_bytes, f"{cs.name}: nothing to fall short of"
                ws_bytes = need - BM * bn * 4
            if S < 2 or need > ws_bytes:
                S = 0
    tf = lambda v: "true" if v else "false"
    if cs.layout == TN and bn == 160 and splits > 1 and va == 4 and vb == 4 and S == 0 and not reasons:
        return Plan(["gemm_tn_lds_kernel"], va, vb, bn, splits, ksplit, slices, 0, ws_bytes, reasons)
    names = [f"gemm_kernel<{tf(ak)}, {tf(bkc)}, {va}, {vb}, {bn}>"] + ([f"gemm_tail_fixup_kernel<{bn}>"] if S else [])
    return Plan(names, va, vb, bn, splits, ksplit, slices, S, ws_bytes, reasons)


def tail_slices(cs, cus=CUS):
    """the k ranges of a tail-split case's S slices (Tail.ksplit = ceil(nkt / S) k-tiles)"""
    p = plan(cs, cus)
    nkt = (cs.K + BK - 1) // BK
    ks = ((nkt + p.S - 1) // p.S) * BK if p.S else 0
    return [(min(cs.K, z * ks), min(cs.K, (z + 1) * ks)) for z in range(p.S)]


# ---- operands ---------------------------------------------------------------------------------------------------------------------------------
def logical(M, N, K, seed=0):
    """the product's operands as a [M][K] and b [K][N], standard normal in fp32 -- a function of the shape and the seed alone, so that the
    same product laid out in different ways has the same values"""
    rs = np.random.RandomState((1000003 * M + 1009 * N + K + 7919 * seed) % (2 ** 31))
    return rs.standard_normal((M, K)).astype(np.float32), rs.standard_normal((K, N)).astype(np.float32)


def embed(mat, ld, off):
    """a NaN-filled flat buffer with `mat` as the [rows][ld] view that starts FRONT + off floats in: (buffer, first element's index)"""
    rows, cols = mat.shape
    assert ld >= cols
    first = FRONT + off
    buf = np.full(first + rows * ld + GUARD, np.nan, np.float32)
    if rows:
        buf[first:first + rows * ld].reshape(rows, ld)[:, :cols] = mat
    return buf, first


def operands(cs, a, b):
    """the case's stored operands around the logical a [M][K], b [K][N]: dict(A, a_first, B, b_first, geometry)"""
    assert a.shape == (cs.M, cs.K) and b.shape == (cs.K, cs.N), (cs, a.shape, b.shape)
    g = geometry(cs)
    A, af = embed(a if cs.layout != TN else np.ascontiguousarray(a.T), g.lda, g.a_off)
    B, bf = embed(np.ascontiguousarray(b.T) if cs.layout == NT else b, g.ldb, g.b_off)
    return dict(A=A, a_first=af, B=B, b_first=bf, g=g)


def c_buffer(cs, splits):
    """NaN for `splits` partial products [M][ldc] behind FRONT + c_off floats, and the guard: (buffer, first element's index)"""
    g = geometry(cs)
    first = FRONT + g.c_off
    return np.full(first + splits * cs.M * g.ldc + GUARD, np.nan, np.float32), first


def c_views(buf, first, cs, splits):
    """(the [splits][M][ldc] view, everything of the buffer that is not inside one of the [M][N] products)"""
    g = geometry(cs)
    body = buf[first:first + splits * cs.M * g.ldc].reshape(splits, cs.M, g.ldc)
    outside = np.concatenate([buf[:first], body[:, :, cs.N:].ravel(), buf[first + splits * cs.M * g.ldc:]])
    return body, outside


def measure(c, c64, scale):
    """tests/test_gpu_split_gemm.py's per-element measure: max |c - c64| / sum_k |a||b|"""
    if c64.size == 0:
        return 0.0
    return float((np.abs(c.astype(np.float64) - c64) / np.maximum(scale, 1e-300)).max())


def k_order_fp32(a, b):
    """row-wise dot products sum_k a[i][k] b[i][k] in fp32, one rounded product and one rounded sum per k, in k order"""
    acc = np.zeros(a.shape[0], np.float32)
    for k in range(a.shape[1]):
        acc = acc + a[:, k] * b[:, k]
    return acc


# ---- the case table ---------------------------------------------------------------------------------------------------------------------------
# (VA, VB) -> the operand specs that give it, once through the pitches and once through a pointer offset under a pitch that is a multiple of 4
VEC_SPECS = {(4, 4): [("p4", "p4")], (4, 2): [("p4", "p2"), ("p4", "o8")], (2, 4): [("p2", "p4"), ("o8", "p4")],
             (2, 2): [("p2", "p2"), ("o8", "o8")], (1, 1): [("p1", "p4"), ("p4", "o4")]}
VEC_PAIRS = list(VEC_SPECS)

# 64-wide tiles: (M, N, K) per (layout, VA, VB) -- M and N off the tile (N <= 64, N = 65, M = 1, one row / column into the next tile), K % 32
# in {0, 1, 3, 31}, K < 32, one and two k-tiles; row-contiguous operands whose column count is no multiple of the vector (130 under 4, 65
# under 2: the last vector of a row straddles the operand's edge) with at least one whole k-tile
SMALL = {
    (NT, 4, 4): (130, 65, 67), (NT, 4, 2): (1, 60, 33), (NT, 2, 4): (129, 64, 31), (NT, 2, 2): (200, 100, 64), (NT, 1, 1): (77, 33, 95),
    (NN, 4, 4): (130, 130, 64), (NN, 4, 2): (100, 65, 33), (NN, 2, 4): (1, 129, 96), (NN, 2, 2): (257, 63, 35), (NN, 1, 1): (129, 65, 32),
    (TN, 4, 4): (130, 66, 65), (TN, 4, 2): (129, 65, 31), (TN, 2, 4): (131, 64, 64), (TN, 2, 2): (1, 200, 33), (TN, 1, 1): (200, 33, 99),
}
C_SPECS = ["p4", "p1", "p4", "c", "o8"]                     # per vector pair, in VEC_PAIRS order: vector stores, scalar stores (odd pitch, contiguous
                                                            # with N % 4 != 0 where it is, a pointer off by 8 bytes)
# 128-wide tiles: one product per layout in all five vector pairs.  With 256 CUs choose_bn takes 128 only when 64-wide tiles need a second
# round: 24 x 22 = 528 tiles of 64 columns against 24 x 11 of 128.  Ragged in M (6 rows in the last panel) and N (66 columns in the last
# tile, 1346 = 2 mod 4), K = 33: a whole k-tile and a one-element one
BIG = (2950, 1346, 33)
# ... and through split-K: 2 x 16 x 17 = 544 workgroups on 64-wide tiles, 272 on 128-wide ones
BIG_SPLIT = (256, 1024, 17 * 32 + 5, 17)
# 160-wide tiles at splits == 1: 31 x 13 = 403 tiles of 160 columns in one round where 31 x 17 = 527 of 128 need two
WIDE = (3850, 2070, 40)
# tail splitting on 128-wide tiles: 6 x 5 = 30 tiles; choose_bn's cost with a workspace puts them on 128 columns from M = 641 (six row
# panels) at K = 2048 -- one of the shapes past M, N <= 600
TAIL128 = (641, 600, 2048)


def _cases():
    out = []
    lay = LAYOUT_NAME
    for (layout, va, vb), (M, N, K) in SMALL.items():
        i = VEC_PAIRS.index((va, vb))
        for way, (a, b) in enumerate(VEC_SPECS[(va, vb)]):
            out.append(case(f"{lay[layout]}64-{va}{vb}-{'pitch' if way == 0 else 'offset'}", layout, M, N, K, a, b, C_SPECS[i], tags=("small", "plain")))
    for layout in (NT, NN, TN):
        for (va, vb), specs in VEC_SPECS.items():
            a, b = specs[-1] if (va, vb) in ((2, 2), (1, 1)) else specs[0]
            out.append(case(f"{lay[layout]}128-{va}{vb}", layout, *BIG, a, b, "p4" if (va, vb) != (2, 4) else "p1", tags=("big", "plain")))
        M, N, K, S = BIG_SPLIT
        out.append(case(f"{lay[layout]}128-split17", layout, M, N, K, "p4", "p4", "p4", splits=S, tags=("split",)))
    # 160-wide tiles
    out.append(case("nn160-split", NN, 130, 200, 100, splits=3, route=4, tags=("split", "route4")))
    out.append(case("tn160-split-route2", TN, 132, 170, 70, splits=2, route=6, tags=("split", "lds")))
    out.append(case("nn160-one-round", NN, *WIDE, tags=("wide", "plain")))
    out.append(case("tn160-one-round", TN, *WIDE, tags=("wide", "plain")))
    # gemm_tn_lds_kernel, and each single reason that sends the product back to gemm_kernel
    out.append(case("tnlds", TN, 132, 170, 70, splits=2, route=4, tags=("split", "lds", "route4")))
    out.append(case("tnlds-one-element-slice", TN, 130, 161, 33, splits=2, route=4, tags=("split", "lds")))
    out.append(case("tnlds-empty-slice", TN, 129, 66, 65, splits=4, route=4, tags=("split", "lds")))
    out.append(case("tnlds-two-tiles", TN, 300, 316, 200, splits=4, route=4, c="c", tags=("split", "lds")))
    out.append(case("tnlds-back-a-ptr", TN, 132, 170, 70, a="o8", splits=2, route=4, tags=("split", "lds")))
    out.append(case("tnlds-back-ldb", TN, 132, 170, 70, b="p2", splits=2, route=4, tags=("split", "lds")))
    out.append(case("tnlds-back-ldc", TN, 132, 170, 70, c="p2", splits=2, route=4, tags=("split", "lds")))
    out.append(case("tnlds-back-c-ptr", TN, 132, 170, 70, c="o8", splits=2, route=4, tags=("split", "lds")))
    # split-K in all three layouts: a short last slice, a slice of one element, an empty slice, the library's own slice count for a
    # weight-gradient-like shape (a long reduction into a small product)
    for layout, (a, b) in ((NT, ("p4", "p4")), (NN, ("p2", "p4")), (TN, ("p4", "o8"))):
        n = lay[layout]
        out.append(case(f"{n}-split-short-last", layout, 130, 70, 200, a, b, splits=3, tags=("split",)))
        out.append(case(f"{n}-split-one-element", layout, 129, 65, 33, a, b, "p1", splits=2, tags=("split",)))
        out.append(case(f"{n}-split-empty-slice", layout, 65, 130, 65, a, b, splits=4, tags=("split",)))
        out.append(case(f"{n}-split-auto", layout, 128, 96, 2000, "p4", "p4", "c", splits="auto", tags=("split", "auto")))
    # tail splitting: one partial round cut along k, both fix-up widths in every layout
    for layout in (NT, NN, TN):
        n = lay[layout]
        out.append(case(f"{n}-tail64", layout, 130, 65 if layout == NN else 60, 256, ws="full", tags=("tail",)))
        out.append(case(f"{n}-tail128", layout, *TAIL128, ws="full", tags=("tail",)))
    out.append(case("nt-tail-k255", NT, 130, 60, 255, ws="full", tags=("tail",)))            # eight k-tiles, the last one ragged: still two slices of four
    out.append(case("nt-tail-k224", NT, 130, 60, 224, ws="full", tags=("tail", "unsplit")))  # seven k-tiles: one short of two slices of four
    out.append(case("nn-tail-short-ws", NN, 130, 65, 256, ws="short", tags=("tail", "unsplit")))
    out.append(case("tn-tail128-short-ws", TN, *TAIL128, ws="short", tags=("tail", "unsplit")))
    # empty products
    for layout in (NT, NN, TN):
        out.append(case(f"{lay[layout]}-k0", layout, 130, 70, 0, tags=("empty",)))
    out.append(case("nt-m0", NT, 0, 70, 40, tags=("empty",)))
    out.append(case("tn-n0", TN, 70, 0, 40, tags=("empty",)))
    out.append(case("nn-m0-split", NN, 0, 70, 40, splits=2, tags=("empty",)))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# the issue's edges of M, N and K, each as a predicate some case must satisfy (tests/test_gemm_ref_cpu.py)
EDGES = {
    "N <= 64": lambda c: 0 < c.N <= 64, "N = 65": lambda c: c.N == 65, "M = 1": lambda c: c.M == 1,
    "K % 32 = 1": lambda c: c.K % 32 == 1, "K % 32 = 3": lambda c: c.K % 32 == 3, "K % 32 = 31": lambda c: c.K % 32 == 31,
    "K < 32": lambda c: 0 < c.K < 32, "K = 0 mod 32": lambda c: c.K > 0 and c.K % 32 == 0, "one k-tile": lambda c: 0 < c.K <= 32,
    "two k-tiles": lambda c: 32 < c.K <= 64, "odd ldc": lambda c: geometry(c).ldc % 2 == 1, "ldc > N": lambda c: geometry(c).ldc > c.N,
}
