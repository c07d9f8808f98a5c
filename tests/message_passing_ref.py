"""Plain restatements of ONE message-passing operation each, built from oracle/txe_oracle.py's own primitives (edge_softmax, scatter_sum,
_leaky, gcn_norm) -- the float64 reference (and, in fp32, the yardstick) of tests/test_gpu_message_passing_ops.py -- and the two graphs
that file runs them on.  Nothing here needs a GPU: tests/test_message_passing_ref_cpu.py holds these functions to orc.gat_layer /
orc.gcn_layer, which the reference goldens pin."""
import numpy as np
import torch

import txe_oracle as orc

# (k grand-parents, m siblings) of tests/test_gpu_readout_match_ops.py: node counts 1..5, 63..68, 127..129, 200
EGONETS = [(0, 0), (0, 1), (2, 0), (1, 2), (2, 2), (20, 42), (3, 60), (0, 64), (30, 35), (66, 0), (7, 60), (40, 86), (64, 63), (1, 127),
           (99, 100)]


def gat_sweep(src, dst, n, ft, a_src, a_dst, attn_slope=0.2, keep=None, scale=1.0, act_slope=None):
    """the GAT sweep (model_zoo.py:106-114, :95): ft [N][H][D], a_src / a_dst [N][H], edges (src -> dst) in any order, keep [E][H] the
    0 / 1 attention-dropout mask in that order -> (out [N][H][D], alpha [E][H])"""
    e = orc._leaky(a_src[src] + a_dst[dst], attn_slope)
    alpha = orc.edge_softmax(dst, n, e)
    a = alpha if keep is None else alpha * keep * scale
    out = orc.scatter_sum(dst, n, ft[src] * a.unsqueeze(-1))
    if act_slope is not None:
        out = orc._leaky(out, act_slope)
    return out, alpha


def gcn_sweep(src, dst, n, x, bias=None, act_slope=None):
    """the GCN sweep (model_zoo.py:39-49): out[v] = act(norm[v] * sum_{u -> v} norm[u] x[u] + bias), norm = in-degree^-1/2 (inf -> 0)"""
    norm = orc.gcn_norm(dst, n, x.dtype)
    out = orc.scatter_sum(dst, n, (x * norm)[src]) * norm
    if bias is not None:
        out = out + bias
    if act_slope is not None:
        out = orc._leaky(out, act_slope)
    return out


def next_logits(x_next, keep, scale, wa):
    """the folded attention logits of the next GATLayer: a12[v][r] = <dropout(X'[v]), wa[r]>, X' [N][kp], keep [N][kp] (0 / 1) or None"""
    xd = x_next if keep is None else x_next * keep * scale
    return xd @ wa.t()


def head_mean(x):
    """model_zoo.py:219 `.mean(1)`: x [N][H][D] -> [N][D]"""
    return x.mean(1)


def in_csr_order(src, dst):
    """the edges in destination-CSR order (stable by destination), where the kernels keep alpha and hash the attention dropout"""
    order = np.argsort(dst, kind="stable")
    return src[order], dst[order]


# ---- graph 1: one generic multigraph --------------------------------------------------------------------------------------------------
G1_N = 301                                   # no multiple of 4 (GAT_WAVES) or of 8
G1_IN = {10: 63, 11: 64, 12: 65, 13: 128, 14: 129, 15: 1, 16: 2, 17: 0, G1_N - 1: 200}   # in-degrees on both sides of one and two 64-edge chunks
G1_OUT = {20: 0, 21: 1, 22: 16, 23: 17, 24: 64, 25: 65, 26: 200}                         # out-degrees: SPLIT_LIGHT_DEG 16 | 17, a chunk, a hub
G1_LONE = 18                                 # neither in- nor out-edges
G1_WIDE = (10, 12, 16)                       # destinations whose softmax spans more than 180 (their sources: nodes 30..69)
G1_WIDE_SRC = np.arange(30, 70)


def generic_multigraph():
    """(src, dst) int64, in a shuffled COO order: G1_N nodes, about 2,400 edges; the nodes of G1_IN have exactly that in-degree, those of
    G1_OUT exactly that out-degree; duplicate edges, self loops, the last node a hub, node G1_LONE isolated"""
    rs = np.random.RandomState(20240)
    free = np.array([v for v in range(G1_N) if v not in G1_IN and v not in G1_OUT and v != G1_LONE])
    src_pool = np.concatenate([free, [v for v in G1_IN]])          # (a node of G1_OUT is a source only of its own edges)
    dst_pool = np.concatenate([free, [v for v in G1_OUT]])         # (a node of G1_IN a destination only of its own)
    src, dst = [], []
    for v, d in G1_IN.items():
        pool = G1_WIDE_SRC if v in G1_WIDE else src_pool
        src.append(rs.choice(pool, size=d) if d != 2 else pool[:2])  # (the two in-edges of node 16: one source of either sign)
        dst.append(np.full(d, v))
    for u, d in G1_OUT.items():
        src.append(np.full(d, u))
        dst.append(rs.choice(dst_pool, size=d))
    src.append(rs.choice(free, size=1100)); dst.append(rs.choice(free, size=1100))      # the bulk
    loops = rs.choice(free, size=60, replace=False)
    src.append(loops); dst.append(loops)                                                 # self loops
    src.append(src[-2][:40]); dst.append(dst[-2][:40])                                   # duplicates of bulk edges
    src.append(np.array([G1_N - 1, 17, 17, 13])); dst.append(np.array([20, 20, 21, 26]))  # the hub, the source-only node and a chunked node feed others
    src, dst = np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)
    perm = rs.permutation(len(src))
    src, dst = src[perm], dst[perm]
    indeg, outdeg = np.bincount(dst, minlength=G1_N), np.bincount(src, minlength=G1_N)
    assert all(indeg[v] == d for v, d in G1_IN.items()) and all(outdeg[u] == d for u, d in G1_OUT.items())
    assert indeg[G1_LONE] == 0 and outdeg[G1_LONE] == 0 and outdeg[17] > 0 and indeg[20] > 0 and len(src) <= 3000
    assert G1_N % 4 and len(set(zip(src.tolist(), dst.tolist()))) < len(src) and (src == dst).any()
    return src, dst


def widen_logits(a_src):
    """a_src [N][H] (numpy, in place): the sources of the G1_WIDE destinations get +90..95 (even ids) or -450..-475 (odd ids: -90..-95
    behind the leaky_relu of slope 0.2) -- a softmax without its running maximum overflows fp32 there, float64 does not"""
    rs = np.random.RandomState(7)
    for u in G1_WIDE_SRC:
        r = rs.random_sample(a_src.shape[1]).astype(np.float32)
        a_src[u] = (90.0 + 5.0 * r) if u % 2 == 0 else -(450.0 + 25.0 * r)
    return a_src


def egonet_batch():
    """(src, dst) int64 of the EGONETS batch in the dataset's edge order (parents -> anchor, anchor -> siblings, self loops), n"""
    g = orc.batch_egonets(EGONETS)
    return g["src"].numpy(), g["dst"].numpy(), int(g["num_nodes"])
