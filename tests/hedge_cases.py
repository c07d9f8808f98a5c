"""Shared case builders of the hedged-placement tests (test_hedge_cpu.py, test_gpu_hedge.py): small taxonomies as parent lists, the
brute-force descendant sets the index is checked against, and probability blocks."""
import numpy as np


def index_of(parents, n):
    """TaxonomyIndex of `parents` = {child: [parent, ...]} over n nodes"""
    from taxoexpan_amd.taxometric import TaxonomyIndex
    cnt = np.asarray([len(parents.get(v, ())) for v in range(n)], dtype=np.int64)
    idx = np.asarray([p for v in range(n) for p in parents.get(v, ())], dtype=np.int64)
    return TaxonomyIndex.from_parents(np.concatenate([[0], np.cumsum(cnt)]), idx)


def chain(n=5):
    return {v: [v - 1] for v in range(1, n)}, n


def star(n=6):
    return {v: [0] for v in range(1, n)}, n


def diamond():
    """0 -> {1, 2} -> 3 -> 4: node 3 has two parents, so 0 reaches 3 and 4 along two paths"""
    return {1: [0], 2: [0], 3: [1, 2], 4: [3]}, 5


def forest():
    """two roots: 0 -> {1, 2}, 3 -> {4, 5}, 5 -> 6"""
    return {1: [0], 2: [0], 4: [3], 5: [3], 6: [5]}, 7


def star_plus_chain(slice_len, seed=3):
    """3 * slice_len + 6 nodes whose subtree lists have 3 * slice_len + 5 entries (the root), slice_len + 1 (its child `b`), slice_len
    (b's only child `c`, with slice_len - 1 leaves) and 1 (every leaf, and one isolated node); node ids shuffled.
    Returns (parents, n, dict(root=, b=, c=, lone=))"""
    S = slice_len
    n = 3 * S + 6
    ids = np.random.RandomState(seed).permutation(n).tolist()
    root, b, c, lone = ids[0], ids[1], ids[2], ids[3]
    rest = ids[4:]
    parents = {b: [root], c: [b]}
    for v in rest[:S - 1]:
        parents[v] = [c]
    for v in rest[S - 1:]:
        parents[v] = [root]
    assert len(rest) - (S - 1) == 2 * S + 3
    return parents, n, dict(root=root, b=b, c=c, lone=lone)


def brute_sub(parents, n, cand):
    """per candidate column the sorted columns of the candidates among the node and its descendants: Python sets, a walk down the child
    lists over ALL nodes (so candidates below a dropped node still count)"""
    children = {v: set() for v in range(n)}
    for v, ps in parents.items():
        for p in ps:
            children[p].add(v)
    col = {int(a): i for i, a in enumerate(cand)}
    out = []
    for a in cand:
        seen, stack = {int(a)}, [int(a)]
        while stack:
            for w in children[stack.pop()]:
                if w not in seen:
                    seen.add(w)
                    stack.append(w)
        out.append(sorted(col[v] for v in seen if v in col))
    return out


def brute_depth(parents, n):
    """longest chain to a parentless node, 1 for a root"""
    memo = {}

    def d(v):
        if v not in memo:
            memo[v] = 1 + max((d(p) for p in parents.get(v, ())), default=0)
        return memo[v]
    return [d(v) for v in range(n)]


def probabilities(Q, G, seed=0, sharp=3.0):
    """P [Q, G] fp32, every row a distribution up to fp32 rounding, peaky enough that subtree masses spread over (0, 1)"""
    rs = np.random.RandomState(seed)
    e = np.exp(sharp * rs.standard_normal((Q, G)))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)
