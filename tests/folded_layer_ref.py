"""Plain restatements of the output layer folded behind the mean readouts (csrc/txe_fold.hip, csrc/txe_fold_bwd.hip), built from
oracle/txe_oracle.py's own primitives (edge_softmax, scatter_sum, segment_sum, _leaky with given branches, gcn_norm, and -- in the CPU
test that holds these functions to the oracle -- weighted_mean_readout / mean_readout) -- the float64 reference (and, in fp32, the
yardstick) of tests/test_gpu_folded_layer_ops.py; the four batches that file runs them on; and the INSTANCE ARITHMETIC of the host
dispatch: for a shape, the kernel names the library must launch.  Nothing here needs a GPU: tests/test_folded_layer_ref_cpu.py holds
the functions to orc.gat_layer / orc.pgat_forward / orc.gcn_layer + readout, and the case tables to the instance lists.

Every function is generic in dtype (the dtype of its tensors).  Edges are (src -> dst) in DESTINATION-CSR order (mp.in_csr_order), where
the kernels keep alpha and hash the attention dropout.  Leaky branches may be GIVEN (0 / 1 arrays, as the kernels read them from stored
state): e_pos for the folded layer's attention logits, act_pos for the activation between the two layers."""
import numpy as np
import torch
import torch.nn.functional as F

import message_passing_ref as mp
import txe_oracle as orc


def _as_branch(pos):
    return None if pos is None else torch.as_tensor(np.asarray(pos) != 0)


def _dropped(X, keep, scale):
    return X if keep is None else X * keep * scale


def readout_weights(pos, pw, n, dtype):
    """w_v of the readout: softplus(pw[pos_v]) (WeightedMeanReadout, model_zoo.py:240-242) or 1 (MeanReadout, pw None)"""
    return F.softplus(pw[pos]).reshape(n) if pw is not None else torch.ones(n, dtype=dtype)


def _graph_rows(graph_off, coef, Xd, w):
    """(wsum [G], Z [G][K]): S_g = sum of the graph's w_v; Z[g] = sum_{u in g} coef_u Xd[u] / S_g; an EMPTY graph: S = 0 and a zero row"""
    wsum = orc.segment_sum(graph_off, w)
    S = torch.where(wsum > 0, wsum, torch.ones_like(wsum))
    return wsum, orc.segment_sum(graph_off, coef.unsqueeze(1) * Xd) / S.unsqueeze(1)


def gat_fold(X, keep, scale, W, attn_l, attn_r, src, dst, graph_off, pos, pw, attn_slope=0.2, attn_keep=None, attn_scale=1.0, e_pos=None,
             a12=None):
    """the one-head output GATLayer (model_zoo.py:80-104) behind Mean / WeightedMeanReadout (:227-242), in the association of
    include/txe.h: hg[g] = Z[g] W^T, Z[g] = sum_{u in g} c_u Xd[u], c_u = sum_{v: u -> v} w_v alpha'_uv / S_g.
    X [N][Kt]; keep [N][Kt] (0 / 1) or None, scale = 1 / (1 - p); W [D][Kt]; attn_l, attn_r [D]; attn_keep [E] (0 / 1) or None;
    pos [N] int64 and pw [vocab][1], or pw None; graph_off [G + 1] int64; a12 [N][2] given: the logits are an input (TXE_FOLD_A12_READY).
    -> dict(a12 [N][2], alpha [E], coef [N] (c~_u = sum_{v: u -> v} w_v alpha'_uv, the kernels' saved state), wsum [G], Z [G][Kt], hg [G][D])"""
    n = X.shape[0]
    Xd = _dropped(X, keep, scale)
    if a12 is None:
        ft = Xd @ W.t()                                                               # :83
        a12 = torch.stack([(ft * attn_l).sum(-1), (ft * attn_r).sum(-1)], 1)          # :84-85
    e = orc._leaky(a12[src, 0] + a12[dst, 1], attn_slope, _as_branch(e_pos), tag="folded attention logits")   # :106-109
    alpha = orc.edge_softmax(dst, n, e)                                               # :111-112
    a_drop = alpha if attn_keep is None else alpha * attn_keep * attn_scale           # :114
    w = readout_weights(pos, pw, n, X.dtype)
    coef = orc.scatter_sum(src, n, w[dst] * a_drop)
    wsum, Z = _graph_rows(graph_off, coef, Xd, w)
    return dict(a12=a12, alpha=alpha, coef=coef, wsum=wsum, Z=Z, hg=Z @ W.t())


def below_then_fold(ft, a1, a2, src, dst, attn_slope_p, keep_p, scale_p, act_slope, act_pos, P, pos, fold):
    """the composite txe_gat_collapse_bwd_fused differentiates: the GATLayer below's sweep (mp.gat_sweep with attention dropout) on its
    projection output Yp = [ft [N][Hp][Dp] | a1 [N][Hp] | a2 [N][Hp]], the activation between the layers (slope act_slope, branches
    act_pos [N][Hp Dp] or None = the plain function; act_slope 1: none), the concatenation with P[pos] (P [vocab][Pd] or None), then
    fold(X') = gat_fold on the remaining arguments.  -> (fold's dict, X' [N][Hp Dp + Pd], alpha_p [E][Hp])"""
    n = ft.shape[0]
    out, alpha_p = mp.gat_sweep(src, dst, n, ft, a1, a2, attn_slope_p, keep_p, scale_p)
    h = orc._leaky(out.flatten(1), act_slope, _as_branch(act_pos), tag="activation between the layers")
    Xn = h if P is None else torch.cat((h, P[pos]), 1)
    return fold(Xn), Xn, alpha_p


def gcn_fold(X, keep, scale, W, bias, src, dst, graph_off, pos, pw):
    """the output GCNLayer (model_zoo.py:35-47) behind the mean readouts: hg[g] = Z[g] W + b, Z[g] = sum_{u in g} c_u Xd[u],
    c_u = norm_u sum_{v: u -> v} w_v norm_v / S_g.  W [Kt][Fo], bias [Fo] or None -> dict(coef [N] (unnormalised), wsum, Z, hg)"""
    n = X.shape[0]
    Xd = _dropped(X, keep, scale)
    norm = orc.gcn_norm(dst, n, X.dtype).reshape(n)
    w = readout_weights(pos, pw, n, X.dtype)
    coef = norm * orc.scatter_sum(src, n, (w * norm)[dst])
    wsum, Z = _graph_rows(graph_off, coef, Xd, w)
    hg = Z @ W
    return dict(coef=coef, wsum=wsum, Z=Z, hg=hg if bias is None else hg + bias)


# ---- the batches ------------------------------------------------------------------------------------------------------------------------
# a batch: dict(graphs = per graph (n, src, dst) with local node ids in COO (edge-id) order, pos [N], and -- derived -- n, G, graph_off,
# src / dst of the whole batch in COO order).  The GPU test builds DGLGraph objects from `graphs` and batches them.
PW = np.array([[25.0], [-3.0], [0.4]], dtype=np.float32)       # class 0 takes the x > 20 branch of softplus / sigmoid (the readout test's)


def _finish(graphs, pos):
    sizes = np.array([g[0] for g in graphs], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)])
    src = np.concatenate([np.asarray(g[1], dtype=np.int64) + o for g, o in zip(graphs, off[:-1])])
    dst = np.concatenate([np.asarray(g[2], dtype=np.int64) + o for g, o in zip(graphs, off[:-1])])
    assert len(pos) == off[-1] and (len(src) == 0 or (src.max() < off[-1] and dst.max() < off[-1]))
    gid = np.repeat(np.arange(len(sizes)), sizes)
    assert np.array_equal(gid[src], gid[dst])                                        # edges stay inside their graph
    return dict(graphs=graphs, pos=np.asarray(pos, dtype=np.int64), n=int(off[-1]), G=len(sizes), graph_off=off, src=src, dst=dst, sizes=sizes)


def _egonet(k, m):
    n, s, d, p = orc.egonet_edges(k, m)
    return (n, np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64)), p


EMPTY = (0, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
B_EMPTY = (4, 20, 42)                          # the empty graphs of batch B (the last one ends the batch)
B_NOT_HUB = 9                                  # a 10-node egonet (3, 6) plus one sibling -> sibling edge: not hub-shaped
B_SHAPES = {0: (0, 0), 1: (1, 0), 7: (0, 15), 8: (10, 5), B_NOT_HUB: (3, 6), 30: (15, 0)}


def batch_a():
    """the 15 egonets of mp.EGONETS: 992 nodes, G < 16 (the per-graph Z sweep), graphs on both sides of 64 nodes; the second 8-graph
    workgroup of the edge-level kernels holds 785 nodes (past the 512 whose readout weights are staged in LDS)"""
    parts = [_egonet(k, m) for k, m in mp.EGONETS]
    b = _finish([p[0] for p in parts], np.concatenate([p[1] for p in parts]))
    s, d, n = mp.egonet_batch()
    assert n == b["n"] == 992 and np.array_equal(s, b["src"]) and np.array_equal(d, b["dst"])
    return b


def batch_b(first=None):
    """43 small graphs of 0..16 nodes (N <= 16 G, G >= 16: the chunked Z sweep; G % 4 == 3: a last chunk of three graphs): egonets (k, m),
    three EMPTY graphs (one of them last), a single-node graph, a parent + anchor graph, anchors with 16 out-edges and with 11 and 16
    in-edges (heavy nodes, degree > 8), and one 10-node graph that is not hub-shaped.  first = 15: its first 15 graphs alone."""
    rs = np.random.RandomState(11)
    graphs, pos = [], []
    for i in range(43):
        k, m = int(rs.randint(0, 7)), int(rs.randint(0, 9))                          # (drawn for every index: the list does not shift)
        if i in B_EMPTY:
            graphs.append(EMPTY)
            continue
        g, p = _egonet(*B_SHAPES.get(i, (k, m)))
        if i == B_NOT_HUB:
            g = (g[0], np.append(g[1], 5), np.append(g[2], 7))                        # sibling 5 -> sibling 7 (nodes 0..2 parents, 3 the anchor)
        graphs.append(g)
        pos.append(p)
    if first is not None:
        keep = [i for i in range(first) if i not in B_EMPTY]
        graphs, pos = graphs[:first], pos[:len(keep)]
    return _finish(graphs, np.concatenate(pos))


def batch_c(empties=0):
    """the generic batch of test_fused_backward_sweep_equals_unfused_chain (graphs of 1..90 nodes: a hub with in-degree > 64, a node with
    400 out-edges, nodes without in-edges, duplicate edges) plus one 300-node circulant graph u -> u + 1 .. u + 9: every node of it is
    heavy (degree 9 > 8) on both sides, 300 of them overflow the 256-entry heavy lists of its 8-graph workgroup.  empties = 45: batch E,
    45 empty graphs in a row behind the 7-node graph (a window of the egonet walk then holds more graphs than positions)."""
    rs = np.random.RandomState(3)
    graphs = []
    for n in [1, 2, 40, 7, 3, 90, 5, 33]:
        src, dst = [], []
        if n > 1:
            e = 3 * n
            src.append(rs.randint(0, n, e)); dst.append(rs.randint(1, n, e))          # node 0 of every graph: no in-edge but its self loop
        if n == 90:
            src.append(rs.randint(0, n, 100)); dst.append(np.full(100, 11))           # hub: in-degree > 64
            src.append(np.full(400, 17)); dst.append(rs.randint(0, n, 400))           # 400 out-edges: past the LDS-staged edge scalars
        if n != 33:
            src.append(np.arange(n)); dst.append(np.arange(n))                        # (the 33-node graph has nodes without any in-edge)
        graphs.append((n, np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)))
        if n == 7:
            graphs.extend([EMPTY] * empties)
    u = np.repeat(np.arange(300), 9)
    graphs.append((300, u, (u + np.tile(np.arange(1, 10), 300)) % 300))
    N = sum(g[0] for g in graphs)
    return _finish(graphs, rs.randint(0, 3, N))


BATCHES = {"A": batch_a, "B": batch_b, "B15": lambda: batch_b(15), "C": batch_c, "E": lambda: batch_c(45)}
_CACHE = {}


def batch(name):
    if name not in _CACHE:
        _CACHE[name] = BATCHES[name]()
    return _CACHE[name]


def audit_rule(audit):
    """the project's rule for given leaky branches, on the records orc.BRANCH_AUDIT collects: a given branch may differ from the float64
    sign only where |x| <= 1e-4 of the largest |x|, on at most 1e-3 numel + 1 entries"""
    assert len(audit) >= 1
    for tag, n_dis, worst, biggest, numel in audit:
        assert worst <= 1e-4 * biggest and n_dis <= 1e-3 * numel + 1, (tag, n_dis, worst, biggest, numel)


def audited(fn):
    """fn() with the oracle's branch audit on -> (fn's result, the audit records); the audit is off again afterwards"""
    orc.BRANCH_AUDIT = []
    try:
        return fn(), list(orc.BRANCH_AUDIT)
    finally:
        orc.BRANCH_AUDIT = None


def widen_fold_logits(b, a12):
    """a12 [N][2] (numpy, in place) for TXE_FOLD_A12_READY: the in-neighbours of the destination with the most in-edges get a1 = +90..95
    (every second one) or -450..-475 (-90..-95 behind the leaky_relu of slope 0.2), as mp.widen_logits does: that destination's softmax spans
    more than 180 -- without its running maximum __expf overflows fp32 there.  -> the destination"""
    indeg = np.bincount(b["dst"], minlength=b["n"])
    v = int(indeg.argmax())
    srcs = np.unique(b["src"][b["dst"] == v])
    assert len(srcs) >= 8
    r = np.random.RandomState(7).random_sample(len(srcs)).astype(np.float32)
    a12[srcs, 0] = np.where(np.arange(len(srcs)) % 2 == 0, 90.0 + 5.0 * r, -(450.0 + 25.0 * r))
    a12[v, 1] = 0.25
    return v


# ---- instance arithmetic: the kernel names the host must launch for a shape (the library profiler records these names) -------------------
def tf(flag):
    return "true" if flag else "false"


def padded_k(Kh, Pd):
    return (Kh + Pd + 31) // 32 * 32


def zsum_chunked(n, G):
    return n <= 16 * G and G >= 16


def zsum_kernel(n, G, masked, edot=False):
    if zsum_chunked(n, G):
        return f"cl_zsum_chunk_kernel<{tf(masked)}, {tf(edot)}>"
    assert not edot
    return f"cl_zsum_kernel<{tf(masked)}>"


def zsum_tiles(Kp):
    """(ntile, nmap): 256-column tiles of a row; wave slots per chunk of the chunked sweep -- one idle slot when ntile is a multiple of 4"""
    ntile = (Kp // 4 + 63) // 64
    return ntile, ntile + 1 if ntile % 4 == 0 else ntile


def fwd_launches(n, G, masked, a12_ready=False, edot=False):
    """the named launches of txe_gat_collapse_fwd (the edge-level kernel and the hg product carry no cl_ name)"""
    return ([] if a12_ready or n == 0 else [f"cl_logits_kernel<{tf(masked)}>"]) + [zsum_kernel(n, G, masked, edot)]


def bwd_dot_kernel(Kp, masked):
    nvec = Kp // 4
    nt = 5 if 64 < nvec <= 320 else 9 if 320 < nvec <= 576 else 10 if 576 < nvec <= 640 else 0
    return f"cl_bwd_dot_row_kernel<{tf(masked)}, {nt}>" if nt else f"cl_bwd_dot_kernel<{tf(masked)}>"


def bwd_launches(Kp, masked, att=True, dot=True):
    """the named cl_ launches of txe_gat_collapse_bwd (att) / txe_gcn_collapse_bwd (not att; dot: with readout weights)"""
    return ([bwd_dot_kernel(Kp, masked)] if dot else []) + [f"cl_bwd_dx_kernel<{tf(masked)}, {tf(att)}>"]


def fused_supported(Kh, Pd, Hp, Dp):
    F_ = Hp * Dp
    return Hp in (1, 2, 4) and F_ == Kh and F_ % 16 == 0 and F_ <= 4096 and padded_k(Kh, Pd) - F_ <= 128 and Pd <= 128 and Dp % 4 == 0


def fused_kernel(masked, Hp, Dp, no_ego_walk=False):
    """the sweep of txe_gat_collapse_bwd_fused: NI = 16-byte vectors per lane of a wave's quarter row, NWH = waves per head"""
    ni = (Hp * Dp // 16 + 63) // 64
    if Hp == 4 and not no_ego_walk:
        return f"gat_fused_bwd_ego_kernel<{tf(masked)}, {ni}>"
    return f"gat_fused_bwd_kernel<{tf(masked)}, {ni}, {4 // Hp}>"


def fused_launches(Kp, masked, Hp, Dp, no_ego_walk=False, edot=False):
    """the named launches of one TXE_FUSED_SWEEP (the <dZ, X> sweep, unless the forward pass left it in e_part; the fused sweep; the edge
    backward of the layer below with the first reduction stage)"""
    return ([] if edot else [bwd_dot_kernel(Kp, masked)]) + [fused_kernel(masked, Hp, Dp, no_ego_walk), "gat_attn_bwd_reduce_a_kernel"]


# ---- the case tables of tests/test_gpu_folded_layer_ops.py (here, so that the CPU test can hold them to the instance lists) ---------------
MASKS = (False, True)
# 2a. txe_gat_collapse_fwd: (Kh, Pd) -> Kp; every width on A and B, three of them on C as well; D = 6 at the widest rows
FWD_WIDTHS = [(10, 4, 32), (250, 6, 256), (250, 50, 320), (1000, 24, 1024), (2000, 50, 2080), (2400, 50, 2464), (2560, 32, 2592)]
FWD_ON_C = (32, 320, 2080)
FWD_OPTION_WIDTHS = (32, 320, 1024)              # the widths that also run the options (pw, attention dropout, A12_READY, HG_SPLIT, hg NULL)
FWD_CASES = [(Kh, Pd, bn) for Kh, Pd, Kp in FWD_WIDTHS for bn in ("A", "B") + (("C",) if Kp in FWD_ON_C else ())]
# 2b. txe_gat_collapse_bwd: every cl_bwd_dot instance and both sides of each switch (Kp / 4 = 64 | 65, 320 | 321, 576 | 577, 640 | 641)
BWD_WIDTHS = [(32, 0, 32), (250, 6, 256), (250, 38, 288), (1230, 50, 1280), (1262, 50, 1312), (2254, 50, 2304), (2286, 50, 2336),
              (2510, 50, 2560), (2542, 50, 2592)]
BWD_ON_BC = (288, 2336)
BWD_CASES = [(Kh, Pd, bn) for Kh, Pd, Kp in BWD_WIDTHS for bn in ("A",) + (("B", "C") if Kp in BWD_ON_BC else ())]
# 2c. txe_gat_collapse_bwd_fused: (Hp, Dp, Pd)
FUSED_SHAPES = [(4, 4, 4), (4, 256, 0), (4, 260, 50), (4, 500, 50), (4, 500, 0), (4, 512, 128), (4, 516, 1), (4, 600, 50), (4, 768, 0),
                (4, 772, 50), (4, 1024, 0), (2, 24, 4), (2, 520, 50), (2, 1032, 50), (2, 1544, 50), (1, 48, 4), (1, 1040, 50), (1, 2064, 50),
                (1, 3088, 50)]
FUSED_ON_BCE = [(4, 4, 4), (4, 500, 50), (2, 24, 4), (1, 48, 4)]
FUSED_CASES = [(Hp, Dp, Pd, "A", ne) for Hp, Dp, Pd in FUSED_SHAPES for ne in ((False, True) if Hp == 4 else (False,))]
FUSED_CASES += [(Hp, Dp, Pd, bn, False) for Hp, Dp, Pd in FUSED_ON_BCE for bn in ("B", "C", "E")]
# 2e. txe_gcn_collapse_fwd / _bwd: (Kh, Pd, Fo, batch)
GCN_CASES = [(10, 4, 6, "A"), (10, 4, 250, "B"), (250, 50, 250, "A"), (250, 50, 6, "B"), (250, 50, 6, "C"), (2000, 50, 6, "A"),
             (2000, 50, 6, "B")]
