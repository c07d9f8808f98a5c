"""Shared builders of the near-negative tests (test_near_negatives_cpu.py, test_gpu_near_negatives.py): the three datasets the sampler
tests use, a literal Python statement of the rule (written from the rule's text, not from sampler.host_draw), and the slot ranges."""
import os
import random
import shutil

import numpy as np

from golden_util import GOLDEN_DIR

HARD_ROT_SLOT = 16383
_M = (1 << 64) - 1


def toy(tmp_path, **kw):
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    d = tmp_path / "toy"
    d.mkdir(exist_ok=True)
    for fn in os.listdir(os.path.join(GOLDEN_DIR, "toy_taxo")):
        shutil.copy(os.path.join(GOLDEN_DIR, "toy_taxo", fn), d)
    random.seed(0)
    opts = dict(mode="train", sampling_mode=1, negative_size=7, expand_factor=5, normalize_embed=True)
    opts.update(kw)
    return MaskedGraphDataset(MAGDataset("toy", str(d), raw=True), **opts)


def synthetic(tmp_path, **kw):
    """a few thousand nodes of the synthetic generator, written as raw files and read back like a real dataset"""
    from taxoexpan_amd import synthetic as syn
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    d = tmp_path / "syn"
    d.mkdir(exist_ok=True)
    tax = syn.make_taxonomy(3000, 4500, 16, seed=3)
    syn.write_raw(str(d), "syn", syn.taxonomy_edges(tax), tax.features.numpy())
    random.seed(0)
    opts = dict(mode="train", sampling_mode=1, negative_size=7, expand_factor=20)
    opts.update(kw)
    return MaskedGraphDataset(MAGDataset("syn", str(d), raw=True), **opts)


def hand(tmp_path, k=5):
    """0 -> 1 -> {2..9}: every query 2..9 has the one parent 1, whose one parent 0 is a root"""
    from taxoexpan_amd import synthetic as syn
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    d = tmp_path / "hand"
    d.mkdir(exist_ok=True)
    n = 10
    edges = [(0, 1)] + [(1, c) for c in range(2, n)]
    syn.write_raw(str(d), "hand", edges, np.random.RandomState(0).randn(n, 8).astype(np.float32))
    return MaskedGraphDataset(MAGDataset("hand", str(d), raw=True), mode="train", sampling_mode=1, negative_size=k, expand_factor=4)


# negative_size -> (table slots, near counts) of the lane-loop test: k = 1 (63 idle lanes beside the ballots), 64 (one full pass) and 65
# (a second pass with one live lane).  k = 1 has room for one source at a time: its near launch comes without a table.
LANE_LOOP_PLANS = {1: (1, (1, 0, 0)), 64: (3, (30, 1, 30)), 65: (3, (30, 2, 30))}


def lane_loop_routes(k, table):
    """the host_draw keywords of the three instantiations for negative_size k: pool; table + pool; near (+ table unless k = 1) + pool"""
    slots, counts = LANE_LOOP_PLANS[k]
    hard = dict(hard=table, hard_slots=slots)
    return dict(pool={}, table=hard, near=dict(near=counts, **({} if k == 1 else hard)))


def shuffled(n, seed):
    order = list(range(n))
    random.Random(seed).shuffle(order)
    return order


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


def rotation(seed, epoch, s, t, n):
    """r_X of the rule, in Python integers"""
    h = mix64(seed ^ mix64((epoch << 44) | (s << 20) | (HARD_ROT_SLOT << 6) | t))
    return ((h >> 32) * n) >> 32


def class_lists(ds, p):
    """(S, G, U) of the positive p from the dataset's masked graph, by the literal loops of the rule"""
    S = list(ds.graph.succ.get(p, ()))
    G = list(ds.graph.pred.get(p, ()))
    U = []
    for g in G:
        for c in ds.graph.succ.get(g, ()):
            U.append(c)
    return S, G, U


def slot_ranges(counts, h0=0):
    """[(first slot, one past the last)] of the sibling, grandparent and uncle slots"""
    out, at = [], h0
    for c in counts:
        out.append((at, at + c))
        at += c
    return out


def literal_near(ds, order, start, Q, epoch, seed, counts, positives, h0=0):
    """{(i, j): (class, node)} -- the ACCEPTED proposals of the Q queries at positions start .. of `order`, by the rule's text: class X
    proposes L_X[(r_X + e) % n_X] for e < min(c_X, n_X), kept iff it is a node, in the pool and not masked.  positives [Q]: the
    positive of every query (the pointer walk is not restated here)."""
    pool = set(ds.all_positions)
    n_nodes = int(ds.node_features.shape[0])
    out = {}
    for i in range(Q):
        s = start + i
        q = ds.node_list[order[s]]
        for x, ((lo, hi), L) in enumerate(zip(slot_ranges(counts, h0), class_lists(ds, int(positives[i])))):
            n = len(L)
            if n == 0:
                continue
            r = rotation(seed, epoch, s, 1 + x, n)
            for e in range(min(hi - lo, n)):
                a = L[(r + e) % n]
                if 0 <= a < n_nodes and a in pool and a not in ds.node2masks[q]:
                    out[(i, lo + e)] = (x, a)
    return out
