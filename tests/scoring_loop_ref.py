"""Plain restatements of the all-candidate scoring and ranking loop (include/txe.h: txe_score_block, txe_score_positives,
txe_score_count_block, txe_score_topk_block, txe_topk_merge, txe_rank_block, txe_rank_finalize) in float64 and integers -- the reference
of tests/test_gpu_scoring_loop_ops.py.  Beside them the HOST PREDICATES its cases rely on, each restated from the C source it cites (for a
shape: the loaders, the tile width, the persistent kernel, the launch names the library's profiler must record), the two input
generators and the case tables.  Nothing here needs a GPU or imports the library: tests/test_scoring_loop_ref_cpu.py holds the functions
to the project's host code and the goldens, the exact generator to its claim, and the tables to the branches they are there for."""
import numpy as np

CUS = 256                         # the MI355X's compute units (device_cu_count, txe_profile.hip)
BM, BK, THREADS = 128, 32, 256    # txe_gemm.h: GEMM_BM, GEMM_BK, GEMM_THREADS
PS = 8                            # gemm_tile_epilogue: thresholds of a row staged in LDS (both tile widths, the bf16-pipe instance)
RANK_MAXP = 64                    # txe_rank.hip: positives per pass of rank_kernel's scalar path
RANK_ROUND = 4 * 256 * 4          # ... floats of a row per g0 round of its 16-byte path
TOPK_MAX = 8                      # txe_common.h
PERSIST_MAXK = 512                # txe_gemm.h: TXE_PERSIST_MAXK
INT_MAX = 0x7FFFFFFF              # an empty slot of txe_topk_merge
ERR_ARG, ERR_WORKSPACE = -1, -3


def round_up(x, m):
    return (x + m - 1) // m * m


# ---- the operations ---------------------------------------------------------------------------------------------------------------------------
def scores64(Q, U, apply_exp):
    """S[q][g] = <Q[q], U[g]> in float64, then exp (test_fast.py:116-123 / infer.py:95-99 on the projected candidates: txe.h's scoring
    loop).  Non-finite inputs take the literal sum of products (a BLAS may skip zero entries: inf x 0 must give NaN)."""
    Q, U = np.asarray(Q, dtype=np.float64), np.asarray(U, dtype=np.float64)
    with np.errstate(all="ignore"):
        if np.isfinite(Q).all() and np.isfinite(U).all():
            S = Q @ U.T
        else:
            S = np.stack([(q[None, :] * U).sum(1) for q in Q]) if len(Q) else np.zeros((0, len(U)))
        return np.exp(S) if apply_exp else S


def positives64(Q, Up, pos_off, apply_exp):
    """thr[j] = score(Q[q], Up[j]) for j in [pos_off[q], pos_off[q+1]): the staircase entries of scores64 (test_fast.py:121-123 on
    rearrange()'s positives)"""
    thr = np.zeros(int(pos_off[-1]))
    for q in range(len(pos_off) - 1):
        a, b = int(pos_off[q]), int(pos_off[q + 1])
        if b > a:
            thr[a:b] = scores64(Q[q:q + 1], Up[a:b], apply_exp)[0]
    return thr


def _better(a, b, larger):
    with np.errstate(invalid="ignore"):
        return (a > b) if larger else (a < b)         # strict; NaN on either side: False


def counts(S, pos_off, thr, larger):
    """counts[j] = #{g < G : S[q][g] strictly better than thr[j]} over ALL candidates (txe.h: txe_score_count_block); NaN never counts"""
    out = np.zeros(int(pos_off[-1]), dtype=np.int64)
    for q in range(len(pos_off) - 1):
        a, b = int(pos_off[q]), int(pos_off[q + 1])
        if b > a:
            out[a:b] = _better(S[q][None, :], np.asarray(thr[a:b])[:, None], larger).sum(1)
    return out


def finalize(pos_off, thr, cnt, larger):
    """ranks[j] = 1 + counts[j] - #{j' of the same query : thr[j'] strictly better than thr[j]} (metric.py:7-31: positives never count
    against each other)"""
    out = np.zeros(int(pos_off[-1]), dtype=np.int64)
    for q in range(len(pos_off) - 1):
        a, b = int(pos_off[q]), int(pos_off[q + 1])
        t = np.asarray(thr[a:b])
        for j in range(a, b):
            out[j] = 1 + int(cnt[j]) - int(_better(t, thr[j], larger).sum())
    return out


def ranks(S, pos_off, pos_idx, larger):
    """metric.py:7-31 after test_fast.py:16-22: rank(p) = 1 + #{g not a positive of q : S[q][g] strictly better than S[q][p]}"""
    out = np.zeros(int(pos_off[-1]), dtype=np.int64)
    for q in range(len(pos_off) - 1):
        P = np.asarray(pos_idx[int(pos_off[q]):int(pos_off[q + 1])], dtype=np.int64)
        neg = np.ones(S.shape[1], dtype=bool)
        neg[P] = False
        for i, p in enumerate(P):
            out[int(pos_off[q]) + i] = 1 + int(_better(S[q][neg], S[q][p], larger).sum())
    return out


def keys_of(S, larger):
    """the selection key: the score, negated when smaller is better; NaN ranks last (the key of -inf)"""
    key = np.array(S if larger else -np.asarray(S), dtype=np.float64)
    key[np.isnan(key)] = -np.inf
    return key


def topk(S, k, larger, idx_base=0):
    """infer.py:100-106 / test_fast.py:125-131: `sorted(enumerate(scores), key=-score)[:k]` -- Python's STABLE sort: better score first,
    equal scores by ascending candidate row; NaN last; rows shorter than k filled with -1 (key -inf).  -> (idx [nq][k], key [nq][k])"""
    key = keys_of(S, larger)
    nq, G = key.shape
    idx, out = np.full((nq, k), -1, dtype=np.int64), np.full((nq, k), -np.inf)
    for q in range(nq):
        o = np.argsort(-key[q], kind="stable")[:k]
        idx[q, :len(o)], out[q, :len(o)] = o + idx_base, key[q][o]
    return idx, out


def merge(keys, idx, k, idx_base=0):
    """txe_topk_merge: the same order over each row's (key, idx) entries -- better key first, equal keys by ascending idx; entries with
    idx == INT_MAX are empty; a NaN key counts as -inf; -1 / -inf behind the last real entry"""
    keys, idx = np.asarray(keys, dtype=np.float64), np.asarray(idx, dtype=np.int64)
    nq = keys.shape[0]
    oi, ok = np.full((nq, k), -1, dtype=np.int64), np.full((nq, k), -np.inf)
    for q in range(nq):
        ent = sorted(((-np.inf if np.isnan(kv) else float(kv), int(i)) for kv, i in zip(keys[q], idx[q]) if i != INT_MAX), key=lambda e: (-e[0], e[1]))[:k]
        for t, (kv, i) in enumerate(ent):
            oi[q, t], ok[q, t] = i + idx_base, kv
    return oi, ok


# ---- host predicates, restated ----------------------------------------------------------------------------------------------------------------
def gcd_vec(ld):
    """txe_gemm.h:1074"""
    return 4 if ld % 4 == 0 else (2 if ld % 2 == 0 else 1)


def ptr_vec(byte_off):
    """txe_gemm.h:1075-1078, for a pointer `byte_off` bytes behind a 256-byte aligned allocation"""
    return 4 if byte_off % 16 == 0 else (2 if byte_off % 8 == 0 else 1)


def vmat_vec(ld, off):
    """vmat_vec (txe_gemm.h:1079-1085) of a plain operand on a pitch of ld floats, `off` floats behind an aligned base"""
    return min(gcd_vec(ld), ptr_vec(4 * off))


def loader_pair(ld_q, off_q, ld_u, off_u):
    """gemm_launch_layout (txe_gemm.h:1183-1184): the two loaders' vector widths, both scalar when either is"""
    va, vb = vmat_vec(ld_q, off_q), vmat_vec(ld_u, off_u)
    return (1, 1) if va == 1 or vb == 1 else (va, vb)


def choose_bn(M, N, cus=CUS):
    """choose_bn (txe_gemm.h:1100-1133) as the scoring loop reaches it: splits == 1, no tail splitting (plain_k_order), no 160-wide
    tiles (NT products)"""
    if N <= 64:
        return 64
    slots = 2 * cus

    def cost(bn):
        blocks = ((M + BM - 1) // BM) * ((N + bn - 1) // bn)
        return float((blocks + slots - 1) // slots) * bn * (1.6 if bn == 64 else 1.0)
    return 64 if cost(64) < cost(128) else 128


def persist_plan(M, N, K, va, vb, tail, cus=CUS):
    """the persistent-kernel condition of gemm_launch_layout (txe_gemm.h:1192-1227) for txe_score_block (a plain epilogue with
    plain_k_order: never split along k).  None, or dict(name, nfull, rest, whole): `rest` leftover tiles ride as WHOLE tiles of the same
    launch (the `r > 0 && E.plain_k_order` branch)"""
    if not tail or (va, vb) != (4, 4) or N <= 64 or K % BK or K < 5 * BK or K > PERSIST_MAXK or M <= 0:
        return None
    slots = 2 * cus
    ntiles = ((M + BM - 1) // BM) * ((N + 127) // 128)
    nfull = ntiles // slots * slots
    if nfull < 2 * slots:
        return None
    dk = 8 if K >= 9 * BK else 4
    return dict(name=f"gemm_persist_kernel<true, true, {dk}, 4>", nfull=nfull, rest=ntiles - nfull, whole=ntiles - nfull > 0)


def topk_tiles(G):
    """txe_score_topk_tiles (txe_match.hip)"""
    return (G + 127) // 128


SPLIT_KERNEL = "gemm_nt_split_kernel<2, 3, 2, 2>"           # gemm_nt_split_epi_launch (txe_gemm_split.hip): the EPI == 2 instance


def gemm_name(va, vb, bn):
    return f"gemm_kernel<true, true, {va}, {vb}, {bn}>"


def launches(entry, route, nq, N, r, ld_q=None, off_q=0, ld_u=None, off_u=0, tail=False, cus=CUS):
    """the profiler names of one call.  entry "block" | "positives" | "count" | "topk"; route "mfma" (sws NULL) | "split" (the bf16 pipe
    packing per call) | "packed" (u_packed given); N = G, or n_pos for "positives".  (topk_floor_init_kernel, rank_kernel and
    rank_finalize_kernel record nothing.)"""
    if nq <= 0 or N <= 0:
        return []
    tailk = ["topk_merge_kernel"] if entry == "topk" else []
    if route != "mfma":
        return ["split_pack_kernel"] * (2 if route == "split" else 1) + [SPLIT_KERNEL] + tailk
    va, vb = loader_pair(ld_q if ld_q is not None else r, off_q, ld_u if ld_u is not None else r, off_u)
    if entry == "block":
        plan = persist_plan(nq, N, r, va, vb, tail, cus)
        if plan:
            return [plan["name"]]
    bn = 128 if entry == "topk" else choose_bn(nq, N, cus)             # force_bn128: the best-k scratch counts 128-wide tiles
    return [gemm_name(va, vb, bn)] + tailk


# ---- shapes that depend on the device's CU count -----------------------------------------------------------------------------------------------
def wide_shape(cus=CUS):
    """the smallest case at which choose_bn picks the 128-wide tile for the plain / count product AND for the pick product: nq = 2 cus
    queries (cus / 64 row panels), G ragged (64 j + 9), `p` positives for most queries.  -> (nq, G, p)"""
    nq = 2 * cus
    G = next(g for g in range(73, 1 << 22, 64) if choose_bn(nq, g, cus) == 128)
    p = next(p for p in range(17, 4096) if choose_bn(nq, sum(pos_counts(nq, G, "wide", p)), cus) == 128)
    return nq, G, p


def persist_shapes(cus=CUS):
    """txe_score_block on the persistent kernel: K = 160, 8 row panels, column tiles for nfull = 2 slots -- without a remainder, and
    with 16 leftover tiles that ride as whole tiles; G ragged inside its last tile.  -> [(nq, G, r, leftover tiles)]"""
    slots = 2 * cus
    nbn = 2 * slots // 8
    return [(1024, 128 * nbn - 40, 160, 0), (1024, 128 * (nbn + 2) - 40, 160, 16)]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
POS_CYCLE = [1, 8, 9, 17, 1, 0, 9, 8]      # positives per query: below, at and above PS = 8, the second LDS-less pass, none


def pos_counts(nq, G, pattern, wide_p=17):
    """positives per query.  "cycle": POS_CYCLE with NO positive in the first row of a tile (0, 128), the last row of a tile (127) and the
    last query; "cycle+300": one query with 300 besides (several 128-column tiles of the staircase); "wide": wide_p or wide_p + 1
    everywhere but those rows; "one": a single query with 9.  All clipped to G."""
    if pattern == "one":
        return [min(9, G)] * nq
    n = [(wide_p + q % 2) if pattern == "wide" else POS_CYCLE[q % len(POS_CYCLE)] for q in range(nq)]
    if nq >= 3:
        for q in (0, 127, 128, nq - 1):
            if q < nq:
                n[q] = 0
    if pattern == "cycle+300":
        n[nq // 2] = 300
    return [min(v, G) for v in n]


def positives(nq, G, pattern, seed, wide_p=17):
    """(pos_off int32 [nq + 1], pos_idx int32: distinct candidate rows per query)"""
    rs = np.random.RandomState(seed)
    n = pos_counts(nq, G, pattern, wide_p)
    idx = [rs.choice(G, size=k, replace=False) for k in n]
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int32), (np.concatenate(idx) if idx else np.zeros(0)).astype(np.int32)


def exact_inputs(nq, G, r, seed, thin=False, special=False, pos_off=None, pos_idx=None, zero_from=None):
    """Q [nq][r], U [G][r] fp32 whose entries are multiples of 1/4 with |x| <= 4: every product (a multiple of 1/16, at most 16) and every
    partial sum in any order is exact in fp32 (r <= 256: |sum| <= 4096 = 2^16 sixteenths), and on the bf16 pipe planes 1 and 2 of every
    element are zero.  thin (the exp cases): at most 5 non-zero entries per query, so |raw| <= 80 and distinct raw scores differ by at
    least 1/16 -- __expf cannot reorder or merge them.  Exact ties: a quarter of the candidate rows duplicated somewhere else, and the
    row of every query's first positive duplicated 64 rows on (another column tile of the 64-wide kernel).  special: a NaN candidate
    row, a +Inf query entry and a -Inf candidate entry.  zero_from: the columns from there on are zero (a zero-padded pitch)."""
    rs = np.random.RandomState(seed)
    Q = rs.randint(-16, 17, size=(nq, r)).astype(np.float32) / 4
    U = rs.randint(-16, 17, size=(G, r)).astype(np.float32) / 4
    if thin:
        keep = np.zeros((nq, r), dtype=bool)
        for q in range(nq):
            keep[q, rs.choice(r, size=min(5, r), replace=False)] = True
        Q *= keep
    if zero_from is not None:
        Q[:, zero_from:], U[:, zero_from:] = 0, 0
    for _ in range(G // 4):
        s, d = rs.randint(0, G, 2)
        U[d] = U[s]
    if pos_off is not None:
        for q in range(nq):
            if pos_off[q + 1] > pos_off[q]:
                p = int(pos_idx[pos_off[q]])
                U[(p + 64) % G] = U[p]
    if special:
        U[(G * 2) // 3] = np.nan
        Q[nq // 2, 0] = np.inf
        U[G // 3, r - 1] = -np.inf
    return Q, U


def generic_inputs(nq, G, r, seed, apply_exp, overflow=False):
    """seeded normal Q and U at the scale the matchers see (candidates x 0.05 under the exp: scores do not overflow).  overflow: four
    planted raw scores, 95 and 89.5 (exp = inf in fp32) and -110 and -106 (exp = 0 in fp32) -- (Q, U, [(q, g)] of the planted entries)"""
    rs = np.random.RandomState(seed)
    Q = rs.standard_normal((nq, r)).astype(np.float32)
    U = (rs.standard_normal((G, r)) * (0.05 if apply_exp else 1.0)).astype(np.float32)
    planted = []
    if overflow:                                        # column 0 belongs to the planted pairs alone
        Q[:, 0] = 0
        Q[:2], U[:4] = 0, 0
        Q[:2, 0] = 10.0
        U[:4, 0] = (9.5, -11.0, 8.95, -10.6)
        planted = [(q, g) for q in (0, 1) for g in (0, 1, 2, 3)]
    return Q, U, planted


# ---- case tables ------------------------------------------------------------------------------------------------------------------------------
# Every case: nq queries, G candidates, r columns; the pitches and pointer offsets (floats) of Q, U and S; the positives' pattern; which
# variants of the exact inputs it runs ("plain", "exp", "special" = NaN / Inf); `why`: the instance and the branch it is there for.
def _case(name, nq, G, r, ld_q, ld_u, off_q, off_u, ld_s, pos, variants, why, zero_from=None, off_s=0):
    return dict(name=name, nq=nq, G=G, r=r, ld_q=ld_q, ld_u=ld_u, off_q=off_q, off_u=off_u, ld_s=ld_s, off_s=off_s, pos=pos, variants=variants,
                why=why, zero_from=zero_from)


SCORE_CASES = [
    _case("1x1x1", 1, 1, 1, 1, 1, 0, 0, 1, "one", ("plain", "exp"), "loaders 1/1 (odd pitches); one query, one candidate, one column"),
    _case("127x3x10", 127, 3, 10, 12, 10, 0, 0, 3, "cycle", ("plain", "exp"), "loaders 4/2; G below one 16-byte chunk; ragged k-tile; scalar C stores (odd ld_s)"),
    _case("128x63x31", 128, 63, 31, 34, 32, 0, 0, 64, "cycle", ("plain", "exp", "special"),
          "loaders 2/4; a whole row panel; odd r; the recompute of a NaN / Inf tile under every epilogue"),
    _case("129x64x32", 129, 64, 32, 32, 32, 2, 2, 68, "cycle", ("plain", "exp"), "loaders 2/2 by an 8-byte base offset on 16-byte pitches; a second row panel of one row; N == 64"),
    _case("129x65x33", 129, 65, 33, 33, 36, 0, 0, 65, "cycle", ("plain", "exp"), "va == 1 collapses both loaders to 1/1; a second 64-column tile of one column"),
    _case("300x127x250", 300, 127, 250, 252, 256, 0, 0, 128, "cycle", ("plain", "exp", "special"), "loaders 4/4; r = 250 (ragged last k-tile); the bf16 pipe's long k-loop"),
    _case("300x129x256z", 300, 129, 256, 256, 256, 0, 0, 132, "cycle", ("plain", "exp"), "r = 256 on a zero-padded pitch (250 columns of data); a third 64-column tile of one column",
          zero_from=250),
    _case("300x1003x32", 300, 1003, 32, 32, 32, 0, 1, 1004, "cycle+300", ("plain", "exp", "special"),
          "vb == 1 (a 4-byte base offset) collapses both loaders; a query with 300 positives: 3 tiles of the staircase, 37 passes past PS; S from a misaligned base",
          off_s=1),
]
WIDE_CASE = dict(name="wide", r=12, pos="wide", variants=("plain", "exp"), why="the 128-wide tile of gemm_kernel under the plain, pick and count epilogues (sized by the CU count)")
TOPK_KS, IDX_BASE = (1, 5, 8), 7

# (a) generic inputs against float64 through the gate: (nq, G, r, ld_q, ld_u, ld_s, positives' pattern, overflow)
GENERIC_CASES = [(1, 1, 1, 1, 1, 1, "one", False), (127, 3, 10, 12, 10, 3, "cycle", False), (129, 65, 33, 33, 36, 65, "cycle", False),
                 (300, 129, 250, 252, 256, 132, "cycle", False), (300, 1003, 32, 32, 32, 1004, "cycle+300", True)]

# (c) txe_rank_block alone: (nq, G, ld_s, off_s, positives per query, why)
RANK_CASES = [
    (6, 3, 4, 0, [0, 1, 3, 3, 2, 1], "16-byte path, G < 4: no 16-byte chunk, only the ragged end"),
    (6, 4, 4, 0, [0, 1, 4, 4, 3, 1], "16-byte path, exactly one chunk"),
    (6, 5, 8, 0, [0, 1, 4, 5, 5, 1], "16-byte path, one chunk and a ragged end; 5 positives: a second group of four"),
    (5, 4095, 4096, 0, [0, 1, 4, 5, 9], "16-byte path, one g0 round short of full"),
    (5, 4097, 4100, 0, [0, 1, 4, 5, 9], "16-byte path, exactly one full g0 round (1,024 chunks) and a ragged end of one"),
    (5, 4101, 4104, 0, [0, 1, 4, 5, 9], "16-byte path, a second g0 round (1,025 chunks: 4,097 still ends in the first)"),
    (4, 1003, 1003, 0, [1, 64, 65, 130], "scalar path by an odd pitch: 65 and 130 positives take a second and a third pass"),
    (4, 1003, 1004, 1, [1, 64, 65, 130], "scalar path by a 4-byte base offset on a 16-byte pitch"),
    (1, 37, 40, 0, [9], "nq = 1"),
]
# txe_topk_merge alone: entries per row x rows; every k from 1 to 8
MERGE_CNTS, MERGE_NQ = (0, 1, 7, 64, 255, 256, 257, 1000), (1, 5)


def rank_path(ld_s, off_s):
    """rank_kernel (txe_rank.hip): the 16-byte single-sweep path, else the scalar one"""
    return "vec" if ld_s % 4 == 0 and (4 * off_s) % 16 == 0 else "scalar"


def edges(cus=CUS):
    """name -> reached, for every edge the tables are there for (tests/test_scoring_loop_ref_cpu.py asserts each)"""
    cs = SCORE_CASES
    pairs = {loader_pair(c["ld_q"], c["off_q"], c["ld_u"], c["off_u"]) for c in cs}
    raw = {(vmat_vec(c["ld_q"], c["off_q"]), vmat_vec(c["ld_u"], c["off_u"])) for c in cs}
    e = {f"loaders {a}/{b}": (a, b) in pairs for a, b in ((4, 4), (4, 2), (2, 4), (2, 2), (1, 1))}
    e["va == 1 collapses vb"] = any(a == 1 and b > 1 for a, b in raw)
    e["vb == 1 collapses va"] = any(b == 1 and a > 1 for a, b in raw)
    e["a loader narrowed by the pointer alone"] = any(gcd_vec(c["ld_q"]) == 4 and vmat_vec(c["ld_q"], c["off_q"]) < 4 for c in cs)
    for v in (1, 127, 128, 129, 300):
        e[f"nq {v}"] = any(c["nq"] == v for c in cs)
    for v in (1, 3, 63, 64, 65, 127, 129, 1003):
        e[f"G {v}"] = any(c["G"] == v for c in cs)
    for v in (1, 10, 31, 32, 33, 250):
        e[f"r {v}"] = any(c["r"] == v for c in cs)
    e["r 256 on a zero-padded pitch"] = any(c["r"] == 256 and c["zero_from"] for c in cs)
    e["64-wide tile: plain, pick, count"] = all(choose_bn(c["nq"], c["G"], cus) == 64 for c in cs)
    nq, G, p = wide_shape(cus)
    off, _ = positives(nq, G, "wide", 0, p)
    e["128-wide tile: plain, count"] = choose_bn(nq, G, cus) == 128
    e["128-wide tile: pick"] = choose_bn(nq, int(off[-1]), cus) == 128
    e["128-wide tile: best-k"] = all(launches("topk", "mfma", c["nq"], c["G"], c["r"])[0].endswith("128>") for c in cs)
    allpos = [pos_counts(c["nq"], c["G"], c["pos"]) for c in cs] + [pos_counts(nq, G, "wide", p)]
    for v in (0, 1, 8, 9, 17, 300):
        e[f"{v} positives"] = any(v in n for n in allpos)
    e["past PS thresholds at the 128-wide tile"] = p > PS
    big = [n for n in allpos if len(n) > 129]
    e["no positive in the first row of a tile"] = any(n[0] == 0 and n[128] == 0 for n in big)
    e["no positive in the last row of a tile"] = any(n[127] == 0 for n in big)
    e["no positive in the last query"] = all(n[-1] == 0 for n in big)
    e["positives across several staircase tiles"] = any(max(n) > 2 * 128 for n in allpos)
    e["NaN / Inf under every route"] = sum("special" in c["variants"] for c in cs) >= 2
    ps = persist_shapes(cus)
    plans = [persist_plan(m, n, k, 4, 4, True, cus) for m, n, k, _ in ps]
    e["persistent kernel, whole rounds only"] = plans[0] is not None and plans[0]["rest"] == 0
    e["persistent kernel, leftover tiles ride as whole tiles"] = plans[1] is not None and plans[1]["whole"] and plans[1]["rest"] == ps[1][3]
    e["no table case reaches the persistent kernel by accident"] = all(persist_plan(c["nq"], c["G"], c["r"], 4, 4, True, cus) is None for c in cs)
    rk = RANK_CASES
    for v in (3, 4, 5, 4095, 4097):
        e[f"rank 16-byte path G {v}"] = any(G == v and rank_path(ld, off) == "vec" for _, G, ld, off, _, _ in rk)
    e["rank 16-byte path, a second g0 round"] = any(G // 4 > RANK_ROUND // 4 and rank_path(ld, off) == "vec" for _, G, ld, off, _, _ in rk)
    for v in (0, 1, 4, 5, 9):
        e[f"rank 16-byte path {v} positives"] = any(v in n and rank_path(ld, off) == "vec" for _, _, ld, off, n, _ in rk)
    e["rank scalar path by an odd pitch"] = any(ld % 4 and off == 0 for _, _, ld, off, _, _ in rk)
    e["rank scalar path by the base pointer"] = any(ld % 4 == 0 and off % 4 for _, _, ld, off, _, _ in rk)
    for v in (1, 64, 65, 130):
        e[f"rank scalar path {v} positives"] = all(v in n for _, _, ld, off, n, _ in rk if rank_path(ld, off) == "scalar")
    e["rank nq 1"] = any(c[0] == 1 for c in rk)
    e["merge cnt"] = MERGE_CNTS == (0, 1, 7, 64, 255, 256, 257, 1000) and MERGE_NQ == (1, 5)
    return e
