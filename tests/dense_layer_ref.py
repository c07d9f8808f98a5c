"""Plain restatements of the propagation layers' DENSE part (csrc/txe_project.hip): the projection Y = dropout(X) Wp^T of a GATLayer with
its folded attention rows (model_zoo.py:82-85), hw = dropout(X) W of a GCNLayer (:35-37), the input concatenation [h | P[pos]]
(:214-215) -- the float64 reference (and, in fp32, the yardstick) of tests/test_gpu_dense_layer_ops.py; gradients come from autograd.
Beside them the case tables of that file and the HOST PREDICATES its cases rely on, each restated from the C source it cites: for a
shape, the route the library must take and the launch names its profiler must record.  Nothing here needs a GPU:
tests/test_dense_layer_ref_cpu.py holds the functions to the oracle's layers and the tables to the routes.

Every function is generic in dtype (the dtype of its tensors)."""
import numpy as np
import torch

CUS = 256                         # the MI355X's compute units (device_cu_count, txe_profile.hip)
SLOTS = 2 * CUS                   # two co-resident GEMM workgroups per CU
BM, BK, THREADS = 128, 32, 256    # txe_gemm.h:187
DXPOS_MAXC = 64                   # txe_dxpos.h:8
MAX_VOCAB = 8                     # txe_tail.h:10
PREP_MAXL = 4                     # txe_project.hip: layers per preparation launch
DENSE_DX, DENSE_DW, DENSE_REDUCE, DENSE_ALL, DENSE_DX_SPLIT, PH_DEFER = 1, 2, 4, 7, 16, 64


def round_up(x, m):
    return (x + m - 1) // m * m


def padded_k(Kh, Pd):
    return round_up(Kh + Pd, 32)              # txe_gat_padded_k


def padded_f(H, D):
    return round_up(H * D + 2 * H, 128)       # txe_gat_padded_f


def gcn_padded_f(Fo):
    return round_up(Fo, 32)                   # txe_gcn_padded_f


# ---- the operations ---------------------------------------------------------------------------------------------------------------------------
def _dropped(X, keep, p):
    return X if keep is None else X * keep * (1.0 / (1.0 - p))


def gat_dense(X, W, attn_l, attn_r, keep, p):
    """X [N][Kt], W [H D][Kt], attn_l / attn_r [H][D], keep [N][Kt] (0 / 1) or None -> Y[:, :F + 2H] = [ft | a1 | a2]"""
    H, D = attn_l.shape
    ft = _dropped(X, keep, p) @ W.t()                                        # model_zoo.py:82-83
    a1 = (ft.view(-1, H, D) * attn_l).sum(-1)                                # :84
    a2 = (ft.view(-1, H, D) * attn_r).sum(-1)                                # :85
    return torch.cat((ft, a1, a2), 1)


def gcn_dense(X, W, keep, p):
    """X [N][Kt], W [Kt][Fo] -> hw [N][Fo]"""
    return _dropped(X, keep, p) @ W                                          # model_zoo.py:35-37


def build_x(h, pos, P):
    """[h | P[pos]] (model_zoo.py:214-215); P None or zero columns wide: h"""
    return h if P is None or P.shape[1] == 0 else torch.cat((h, P[pos]), 1)


def folded_rows(W, attn_l, attn_r):
    """the 2H folded weight rows wa = [attn_l; attn_r] (x) W of txe_gat_pack_weights: a1 = h wa[:H]^T"""
    H, D = attn_l.shape
    Wv = W.view(H, D, -1)
    return torch.cat(((attn_l.unsqueeze(-1) * Wv).sum(1), (attn_r.unsqueeze(-1) * Wv).sum(1)), 0)


def behind_activation(hl, stored, slope):
    """hl [N][Kh] as the OUTPUT of a leaky_relu whose branches are the signs of the stored fp32 rows both sides read: the values are
    hl's, the gradient with respect to hl is the one with respect to the pre-activation (x leaky'(stored))"""
    pos = torch.as_tensor(np.asarray(stored) > 0)
    f = torch.where(pos, torch.ones((), dtype=hl.dtype), torch.full((), slope, dtype=hl.dtype))
    return hl.detach() + (hl - hl.detach()) * f


def backward(kind, dtype, h, P, pos, W, attn, keep, p, seed, act_on=False, act_slope=0.01):
    """gradients of (out * seed).sum(), out = gat_dense / gcn_dense ([act(h) | P[pos]]): dict(d_X [N][Kt] (with respect to the
    pre-activation on columns < Kh when act_on), dW, dP [vocab][Pd], and for "gat" d_attn_l, d_attn_r [H][D]) as numpy.
    h [N][Kh], P [vocab][Pd], W, seed, keep: numpy; attn = (attn_l, attn_r) [H][D] or None"""
    t = lambda a, g=True: torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(g)
    hl, Pt, Wt = t(h), t(P), t(W)
    hh = behind_activation(hl, h, act_slope) if act_on else hl
    Pp = Pt[torch.from_numpy(np.asarray(pos)).long()]
    Pp.retain_grad()
    X = torch.cat((hh, Pp), 1)
    kt = None if keep is None else t(keep[:, :X.shape[1]], False)
    if kind == "gat":
        al, ar = t(attn[0]), t(attn[1])
        out = gat_dense(X, Wt, al, ar, kt, p)
    else:
        out = gcn_dense(X, Wt, kt, p)
    (out * t(seed, False)).sum().backward()
    z = lambda v: v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))
    g = dict(d_X=np.concatenate([z(hl), z(Pp)], 1), dW=z(Wt), dP=z(Pt))
    if kind == "gat":
        g.update(d_attn_l=z(al), d_attn_r=z(ar))
    return g


# ---- host predicates, restated ----------------------------------------------------------------------------------------------------------------
def dx_streams(Kh, Pd, need_dh):
    """txe_gat_dx_streams (txe_project.hip:738-742)"""
    if need_dh or Pd < 1 or Kh < 1:
        return 0
    c0 = Kh // 4 * 4
    return 1 if (Kh + Pd - c0 <= DXPOS_MAXC and Kh - c0 + Pd <= DXPOS_MAXC) else 0


def dx_c0(Kh, need_dh):
    """first column of d_X that txe_gat_dense_bwd / txe_gcn_dense_bwd write: c0 = need_dh ? 0 : Kh/4*4 (txe_project.hip, both entry points)"""
    return 0 if need_dh else Kh // 4 * 4


def split_tn_eligible(M, N):
    """txe_gemm_split.h:131"""
    return M % 128 == 0 and N % 4 == 0 and M > 0 and N > 0


def gcn_dwt_splits(n, Kp, Fop, cus=CUS):
    """gcn_dwt_splits (txe_project.hip:480-489): k-slices of the transposed dW route of txe_gcn_dense_bwd, 0 = not eligible"""
    if n < 4096 or round_up(Kp, 160) > round_up(Kp, 64):
        return 0
    tiles = ((Fop + 127) // 128) * ((Kp + 159) // 160)
    S = (2 * cus) // tiles
    nkt = (n + BK - 1) // BK
    S = min(S, nkt // 8, 64)
    return S if S >= 2 else 0


def gcn_dw_transposed(n, Kp, Fop, masked, x_dropped):
    """txe_gcn_dense_bwd's `St > 0 && (x_dropped || !mask || drop_p <= 0)`: the transposed route has no masked loader"""
    return gcn_dwt_splits(n, Kp, Fop) > 0 and (bool(x_dropped) or not masked)


def choose_splits(M, N, K, slots=SLOTS):
    """choose_splits (txe_gemm.h:1312-1346)"""
    max_by_k = max((K + 255) // 256, 1)
    nkt = (K + BK - 1) // BK
    best, best_cost = 1, 1e30
    w160, w128, w64 = round_up(N, 160), round_up(N, 128), round_up(N, 64)
    if N > 64 and w160 < w128 and w160 <= w64 and 2.0 * M * N * K >= 2e10:
        tiles = ((M + BM - 1) // BM) * (w160 // 160)
        for s in range(2, min(64, max_by_k) + 1):
            rounds = (tiles * s + slots - 1) // slots
            kt = float((nkt + s - 1) // s)
            cost = rounds * (kt + 2.0) * 1.25 + 0.004 * nkt * s * 1.25
            if cost < best_cost:
                best_cost, best = cost, s
        if best > 1:
            return best
        best_cost = 1e30
    for bn in (64, 128):
        if bn == 64 and N <= 64:
            continue
        tiles = ((M + BM - 1) // BM) * ((N + bn - 1) // bn)
        for s in range(1, min(64, max_by_k) + 1):
            rounds = (tiles * s + slots - 1) // slots
            kt = float((nkt + s - 1) // s)
            cost = rounds * (kt + 2.0) * (0.55 if bn == 64 else 1.0) + 0.004 * nkt * s * (bn / 128.0)
            if cost < best_cost:
                best_cost, best = cost, s
    return best


def choose_bn(M, N, splits, tail_split=False, K=0, allow160=False, force160=False, slots=SLOTS):
    """choose_bn (txe_gemm.h:1100-1133)"""
    if allow160 and splits > 1 and force160:
        return 160
    if N <= 64:
        return 64
    w160, w128, w64 = round_up(N, 160), round_up(N, 128), round_up(N, 64)
    if allow160 and splits > 1 and 2.0 * M * N * K >= 2e10 and w160 < w128 and w160 <= w64:
        return 160
    if allow160 and splits == 1:
        nbm = (M + BM - 1) // BM
        t160, t128 = nbm * ((N + 159) // 160), nbm * ((N + 127) // 128)
        if t160 <= slots and t128 > slots and t160 * 5 >= slots * 3 and w160 <= w128:
            return 160

    def cost(bn):
        blocks = ((M + BM - 1) // BM) * ((N + bn - 1) // bn) * splits
        r = float((blocks + slots - 1) // slots)
        if tail_split and splits == 1 and blocks % slots != 0:
            frac = (blocks % slots) / slots
            kfloor = 4.0 * BK / K if K > 0 else 0.25
            r = float(blocks // slots) + max(frac, kfloor) + 0.1
        return r * bn * ((1.1 if splits > 1 else 1.6) if bn == 64 else 1.0)
    return 64 if cost(64) < cost(128) else 128


def tail_ws_bytes(cus=CUS):
    """gemm_tail_ws_bytes (txe_gemm.h:1165-1167)"""
    return 2 * cus * (BM * 128 + THREADS) * 4


def tail_split_slices(M, N, K, bn, tail, slots=SLOTS):
    """the tail-split rule of gemm_launch_layout (txe_gemm.h:1274-1286), splits == 1: the k-slices S of the last partial round of tiles
    (gemm_tail_fixup_kernel<bn> adds them), 0 = none"""
    if not tail:
        return 0
    tiles = ((M + BM - 1) // BM) * ((N + bn - 1) // bn)
    r = tiles % slots
    nkt = (K + BK - 1) // BK
    S = min(slots // r if r else 0, nkt // 4, 16)
    return S if S >= 2 and r * S * BM * bn * 4 <= tail_ws_bytes() else 0


def gemm_launches(layout, M, N, K, splits=1, tail=False, epi_extras=False, force160=False, loader_mask=False):
    """the profiler names of one product through gemm_launch_layout (txe_gemm.h:1173-1308), 16-byte aligned operands.
    layout "nt" | "nn" | "tn"; tail: a tail workspace is given; epi_extras: the epilogue carries a mask, an activation factor or a column
    split (no 160-wide tiles, no persistent kernel); loader_mask: a TN operand with the dropout mask in its loader (not LDS-direct)"""
    if M <= 0 or N <= 0:
        return []
    ak, bkc = {"nt": (True, True), "nn": (True, False), "tn": (False, False)}[layout]
    splits = max(splits, 1)
    allow160 = not bkc and not epi_extras
    bn = choose_bn(M, N, splits, tail, K, allow160, force160)
    if splits == 1 and tail and N > 64 and not epi_extras and K % BK == 0 and 5 * BK <= K <= 512:
        ntiles = ((M + BM - 1) // BM) * ((N + 127) // 128)                 # gemm_persist_kernel takes whole rounds from two rounds up:
        assert ntiles // SLOTS < 2, "a case table shape reached the persistent kernel: not restated here"
    S = tail_split_slices(M, N, K, bn, tail) if splits == 1 else 0
    if layout == "tn" and bn == 160 and splits > 1 and S == 0 and not loader_mask and not epi_extras:
        return ["gemm_tn_lds_kernel"]                                       # txe_gemm_tn.hip:11-28
    b = lambda v: "true" if v else "false"
    return [f"gemm_kernel<{b(ak)}, {b(bkc)}, 4, 4, {bn}>"] + ([f"gemm_tail_fixup_kernel<{bn}>"] if S else [])


# ---- what each entry point must launch ----------------------------------------------------------------------------------------------------------
def gat_fwd_launches(n, Kh, Pd, H, D, tail):
    """txe_gat_dense_fwd: NT, M = n, N = Fe, K = Kp (the mask rides in the A loader: no epilogue extras)"""
    return gemm_launches("nt", n, H * D + 2 * H, padded_k(Kh, Pd), 1, tail)


def gcn_fwd_launches(n, Kh, Pd, Fo, tail):
    """txe_gcn_dense_fwd: NN, M = n, N = Fo, K = Kp"""
    return gemm_launches("nn", n, Fo, padded_k(Kh, Pd), 1, tail)


SPLIT_FWD = ["split_pack_multi_kernel", "gemm_nt_split_kernel<2, 3, 2, 0>"]        # txe_gat_dense_fwd_split / _split_src: one pack launch, the product


def gat_dx_launches(n, Kh, Pd, H, D, need_dh, masked, act_on, split):
    """phase TXE_DENSE_DX of txe_gat_dense_bwd"""
    Kt, Fp, c0 = Kh + Pd, padded_f(H, D), dx_c0(Kh, need_dh)
    if n <= 0:
        return []
    if dx_streams(Kh, Pd, need_dh):
        return ["gat_dx_pos_kernel"]
    if split and need_dh:
        return ["split_pack_kernel", "split_pack_kernel", "gemm_nt_split_kernel<2, 3, 2, 1>"]
    if not (need_dh or Pd > 0) or Kt - c0 <= 0:
        return []
    cols_main = max(Kh - c0, 0)
    extras = masked or (act_on and need_dh) or cols_main < Kt - c0          # (c2 is always set: a column split unless Pd == 0 with need_dh)
    return gemm_launches("nn", n, Kt - c0, Fp, 1, True, extras)


def gat_dw_launches(n, Kh, Pd, H, D, masked_loader, xt_route):
    """phase TXE_DENSE_DW: the bf16 product on Xt, or split-K TN with M = Fp, N = Kp, K = n"""
    Fp, Kp = padded_f(H, D), padded_k(Kh, Pd)
    if xt_route and n > 0 and split_tn_eligible(Fp, Kp):
        return ["gemm_tn_split_kernel"]
    return gemm_launches("tn", Fp, Kp, n, choose_splits(Fp, Kp, n), False, False, False, masked_loader)


def gcn_bwd_launches(n, Kh, Pd, Fo, need_dh, masked, act_on, x_dropped):
    """txe_gcn_dense_bwd: d_X (NT on Wp's rows), then dW on one of its two routes"""
    Kt, Kp, Fop, c0 = Kh + Pd, padded_k(Kh, Pd), gcn_padded_f(Fo), dx_c0(Kh, need_dh)
    names = []
    if Kt - c0 > 0 and n > 0 and (need_dh or Pd > 0):
        cols_main = max(Kh - c0, 0)
        names += gemm_launches("nt", n, Kt - c0, Fop, 1, True, masked or (act_on and need_dh) or cols_main < Kt - c0)
    if gcn_dw_transposed(n, Kp, Fop, masked, x_dropped):
        return names + gemm_launches("tn", Fop, Kp, n, gcn_dwt_splits(n, Kp, Fop), False, False, True)
    return names + gemm_launches("tn", Kp, Fop, n, choose_splits(Kp, Fop, n), False, False, False, masked and not x_dropped)


# ---- case tables ------------------------------------------------------------------------------------------------------------------------------
# forward: (N, Kh, Pd, H, D) and the GCN width that goes with the same (N, Kh, Pd)
FWD_CASES = [(1, 1, 0, 1, 1), (33, 7, 3, 3, 5), (129, 250, 50, 4, 24), (300, 64, 0, 2, 63), (257, 251, 62, 1, 126)]
GCN_FWD_FO = [1, 5, 100, 66, 500]
# txe_gat_dense_bwd, position-only d_X: (N, Kh, Pd, H, D, streams)
BWD_POS_CASES = [(200, 251, 62, 2, 24, 0), (77, 250, 70, 2, 24, 0), (200, 250, 50, 2, 24, 1)]
# txe_gat_dense_bwd, need_dh = 1: (N, Kh, H, D) x Pd -- Fp 128: the GEMM's own epilogue; Fp 384: gemm_tail_fixup_kernel
BWD_DH_SHAPES = [(300, 64, 2, 24), (300, 64, 4, 63)]
BWD_DH_PD = [0, 16, 50]
BWD_DH_CASES = [(n, Kh, Pd, H, D) for n, Kh, H, D in BWD_DH_SHAPES for Pd in BWD_DH_PD]
# txe_gcn_dense_bwd: (N, Kh, Pd, Fo)
GCN_CASES = [(83, 13, 0, 66), (129, 250, 50, 100), (200, 251, 3, 36)]
# ... the transposed route's predicate: (N, Kh, Pd, p, x_dropped, transposed), each at Fo 36 and 500 (Kp 288: eligible -- 160- and 64-column
# tiles both pad it to 320 -- with a ragged second 160-column tile)
GCN_DWT_CASES = [(4096, 250, 50, 0.0, 0, True), (4096, 250, 38, 0.0, 0, True), (4096, 128, 32, 0.0, 0, True), (4096, 250, 6, 0.0, 0, False), (4095, 250, 50, 0.0, 0, False),
                 (4096, 250, 50, 0.3, 0, False), (4096, 250, 50, 0.3, 1, True)]
GCN_DWT_FO = [36, 500]
# preparation: (N, Kh, Pd, Fo, h given, extra ld_h, x_dropped, bias_row)
PREP_CASES = [(33, 7, 3, 5, True, 0, 0, False), (33, 7, 3, 5, True, 3, 1, True), (129, 250, 50, 100, False, 0, 0, True), (129, 250, 50, 100, False, 0, 1, False),
              (65, 13, 0, 66, True, 1, 1, True), (200, 251, 62, 36, True, 0, 1, False)]
