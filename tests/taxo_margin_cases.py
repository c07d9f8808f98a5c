"""Generated cases of the taxonomy-aware InfoNCE, shared by tests/test_taxo_margin_cpu.py and tests/test_gpu_taxo_margin.py:
small DAGs as parent CSRs with seeded score and anchor arrays, and per (case, gamma) the float64 restatement with the derived gates --
computed once and handed out unchanged.  No tests here."""
import functools

import numpy as np

EPS = 2.0 ** -24
GAMMAS = (0.0, 0.5, 4.0)


# ---- the taxonomies: name -> list of parent lists -----------------------------------------------------------------------------------

def _chain70():
    """0 <- 1 <- ... <- 69: anc(v) has v + 1 entries, beyond the 16-lane stride of txe_taxometric.hip and beyond any staging capacity"""
    return [[]] + [[v - 1] for v in range(1, 70)]


def _forest():
    """two binary trees of 7 nodes, 0..6 and 7..13: nodes of different trees share nothing (d = 1)"""
    tree = lambda o: [[]] + [[o + (v - 1) // 2] for v in range(1, 7)]
    return tree(0) + tree(7)


def _diamond():
    """node 4 has the parents 1 (depth 2) and 3 (depth 3): its depth is 4, the longest path; 6 is its sibling under 1, 7 a root alone"""
    return [[], [0], [0], [2], [1, 3], [4], [1], [], [5], [3]]


def _random40():
    rng = np.random.default_rng(40)
    par = [[], [], []]
    for v in range(3, 40):
        par.append(sorted(set(rng.integers(0, v, size=int(rng.integers(1, 3))).tolist())))
    return par


DAGS = {"chain70": _chain70, "forest": _forest, "diamond": _diamond, "random40": _random40}


@functools.lru_cache(maxsize=None)
def index(dag):
    from taxoexpan_amd.taxometric import TaxonomyIndex
    par = DAGS[dag]()
    ptr = np.concatenate([[0], np.cumsum([len(p) for p in par])])
    return TaxonomyIndex.from_parents(ptr, np.asarray([q for p in par for q in p], dtype=np.int64))


# ---- the cases ----------------------------------------------------------------------------------------------------------------------

# name -> (Q, C, dag, score spread, pitched, positives forced into the first rows)
SPECS = {
    "1x1": (1, 1, "random40", 1.0, False, ()),                 # no negative: loss 0 up to rounding, d_x 0
    "1x2": (1, 2, "diamond", 1.0, False, (4,)),                # the smallest group with a negative
    "3x32": (3, 32, "random40", 1.0, False, ()),               # the GW 32 / 64 boundary of the row function
    "3x33": (3, 33, "forest", 1.0, False, (4,)),
    "5x65": (5, 65, "chain70", 1.0, False, (69, 5, 64, 63)),   # rows that loop; closure rows of 70, 6, 65 and 64 entries
    "17x4": (17, 4, "diamond", 1.0, False, (4, 6, 3)),         # more groups than one workgroup's waves
    "130x6": (130, 6, "random40", 1.0, True, ()),              # ... and pitches above C
    "3x32wide": (3, 32, "random40", 30.0, False, ()),          # scores spread over +-30: the max shift matters
    "9x8chain": (9, 8, "chain70", 1.0, False, (69, 2, 66, 30)),
}
SHAPES = sorted(SPECS)


def _specials(idx, p, rng):
    """nodes in every relation to p that the taxonomy has: p itself, an ancestor, a descendant, a sibling, an unrelated node; then the
    two out-of-range ids"""
    from taxoexpan_amd.taxometric import _lca_depth
    n = idx.n_nodes
    anc = set(idx.ancestors(p).tolist())
    desc = {v for v in range(n) if p in idx.ancestors(v)}
    sib = [v for v in range(n) if v not in anc and v not in desc and set(idx.parents(v).tolist()) & set(idx.parents(p).tolist())]
    unrel = [v for v in range(n) if _lca_depth(idx, v, p) == 0]
    out = [p]
    for pool in (sorted(anc - {p}), sorted(desc - {p}), sib, unrel):
        if pool:
            out.append(int(pool[int(rng.integers(0, len(pool)))]))
    return out + [-1, n]


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(Q, C, dag, index, x fp32 [Q, ld_x], anchors int32 [Q, ld_a], ld_x, ld_dx, ld_a): row i's positive is anchors[i, 0]; the
    specials of the row's positive sit in its columns from 1 on, starting at a position that moves with the row, so that narrow
    shapes see all of them over their rows; the LAST row of a case of three rows or more has an out-of-range positive (-1 or n)"""
    Q, C, dag, spread, pitched, forced = SPECS[name]
    idx = index(dag)
    n = idx.n_nodes
    rng = np.random.default_rng(sum(map(ord, name)))
    ld_x, ld_dx, ld_a = (C + 3, C + 1, C + 2) if pitched else (C, C, C)
    x = np.full((Q, ld_x), np.nan, dtype=np.float32)
    x[:, :C] = (rng.standard_normal((Q, C)) * spread).astype(np.float32)
    anchors = np.full((Q, ld_a), 10 ** 9, dtype=np.int32)
    anchors[:, :C] = rng.integers(0, n, size=(Q, C))
    for i, p in enumerate(forced[:Q]):
        anchors[i, 0] = p
    for i in range(Q):
        sp = _specials(idx, int(anchors[i, 0]), rng)
        for j in range(min(C - 1, len(sp))):
            anchors[i, 1 + j] = sp[(i + j) % len(sp)]
    if Q >= 3:
        anchors[Q - 1, 0] = -1 if Q % 2 else n
    x.setflags(write=False)
    anchors.setflags(write=False)
    return dict(name=name, Q=Q, C=C, dag=dag, index=idx, x=x, anchors=anchors, ld_x=ld_x, ld_dx=ld_dx, ld_a=ld_a)


def pairs(name):
    """the (negative, positive) pairs of a case as host_taxonomic takes them: pred [Q (C - 1), 1], gold_off, gold_idx -- pairs whose
    negative or positive is out of range stay in (host_taxonomic answers relation 6 for them)"""
    c = case(name)
    a = c["anchors"][:, :c["C"]].astype(np.int64)
    pred = a[:, 1:].reshape(-1, 1)
    gold = np.repeat(a[:, 0], c["C"] - 1)
    return pred, np.arange(pred.shape[0] + 1), gold


@functools.lru_cache(maxsize=None)
def reference(name, gamma):
    """the float64 restatement of a case at `gamma` with the gates of tests/test_gpu_taxo_margin.py's docstring:
    dict(d, m, y fp32, loss, d_x, row_loss, e_row, row_gate, d_gate, dist_total)"""
    import torch
    import torch.nn.functional as F
    from taxoexpan_amd.loss import host_taxo_info_nce, host_taxo_margins
    c = case(name)
    Q, C = c["Q"], c["C"]
    x, a = c["x"][:, :C], c["anchors"][:, :C]
    d, m = host_taxo_margins(c["index"], a, gamma)
    loss, d_x, row = host_taxo_info_nce(x, a, c["index"], gamma)
    y = x + m                                                       # fp32: the rows both yardstick and kernel see
    y32 = torch.from_numpy(y.copy()).requires_grad_(True)
    zero = torch.zeros(Q, dtype=torch.long)
    lse32 = F.cross_entropy(y32, zero, reduction="none")            # = logsumexp(y) - y[:, 0], and y[:, 0] == x[:, 0]
    lse32.sum().backward()
    e_row = np.abs(lse32.detach().numpy().astype(np.float64) - row)
    x0 = x[:, 0].astype(np.float64)
    lse = row + x0
    row_gate = np.maximum(2 * e_row, (C + 16) * EPS * np.maximum(1.0, np.maximum(np.abs(lse), np.abs(x0))))
    d_gate = np.maximum(2 * np.abs(y32.grad.numpy().astype(np.float64) - d_x), 8 * EPS * np.maximum(1.0, np.abs(d_x)))
    dist_total = int(np.floor(d[:, 1:] * 2.0 ** 20).astype(np.int64).sum())
    out = dict(d=d, m=m, y=y, loss=loss, d_x=d_x, row_loss=row, e_row=e_row, row_gate=row_gate, d_gate=d_gate, dist_total=dist_total)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
