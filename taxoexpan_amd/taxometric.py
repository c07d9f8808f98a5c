"""Taxonomy-aware evaluation: how far off is a predicted parent?  Wu & Palmer similarity of a prediction to the nearest
gold parent and the relation between the two (exact, too general, too specific, sibling, related, unrelated), on the taxonomy a
model predicts into.  All quantities are integers until the final quotient:

    depth(v)        1 for a node without parents, else 1 + the MAXIMUM depth of its parents (the longest chain to a parentless node)
    anc(v)          v and everything reachable upward, ascending by node id
    lca_depth(a, b) the maximum depth over anc(a) & anc(b); 0 when they share nothing (a forest)
    wup(a, b)       2 lca_depth(a, b) / (depth(a) + depth(b))

`TaxonomyIndex` holds depth and the ancestor closure (CSR) of a parent CSR, built on the host; `taxonomic_slots` evaluates every slot
(query, list position) of a [Q, K] prediction list against the query's gold parents in one launch of csrc/txe_taxometric.hip;
`host_taxonomic` is its numpy restatement.  There is no CPU fallback for device tensors and no device route for host arrays.
"""
import numpy as np
import torch

from . import _lib

EXACT, ANCESTOR, DESCENDANT, SIBLING, RELATED, UNRELATED, NONE = range(7)
RELATION_NAMES = ("exact", "ancestor", "descendant", "sibling", "related", "unrelated", "none")
MAX_CLOSURE = 2 ** 31          # the closure is addressed with int32 offsets


class TaxonomyIndex:
    """depth [n] int32, anc_ptr [n + 1] / anc_idx int32 (row v = anc(v), ascending, v included) and the parent CSR par_ptr / par_idx
    (int32, every row ascending and without repeats) of a DAG, as numpy arrays"""

    def __init__(self, depth, anc_ptr, anc_idx, par_ptr, par_idx):
        self.depth, self.anc_ptr, self.anc_idx, self.par_ptr, self.par_idx = depth, anc_ptr, anc_idx, par_ptr, par_idx
        self.n_nodes = int(depth.shape[0])

    @classmethod
    def from_parents(cls, par_ptr, par_idx):
        """par_ptr [n + 1], par_idx: the parents of node v are par_idx[par_ptr[v]:par_ptr[v + 1]].  ValueError: a malformed CSR, a parent id
        outside [0, n), a cycle (a self-loop included), a closure of 2^31 entries or more."""
        par_ptr = np.asarray(par_ptr, dtype=np.int64).reshape(-1)
        par_idx = np.asarray(par_idx, dtype=np.int64).reshape(-1)
        n = par_ptr.size - 1
        if n < 0 or n >= 2 ** 31 or par_ptr[0] != 0 or par_ptr[-1] != par_idx.size or np.any(np.diff(par_ptr) < 0):
            raise ValueError("TaxonomyIndex: par_ptr must be [n + 1] offsets, ascending from 0 to len(par_idx), n < 2^31")
        if par_idx.size and (par_idx.min() < 0 or par_idx.max() >= n):
            raise ValueError("TaxonomyIndex: a parent id lies outside [0, n)")
        child = np.repeat(np.arange(n, dtype=np.int64), np.diff(par_ptr))
        pairs = np.unique(np.stack([child, par_idx], 1), axis=0) if par_idx.size else np.zeros((0, 2), dtype=np.int64)
        child, parent = pairs[:, 0], pairs[:, 1]                       # rows ascending, repeats dropped
        n_par = np.bincount(child, minlength=n)
        par_ptr = np.concatenate([[0], np.cumsum(n_par)])
        # longest-path depth = the round of Kahn's peeling in which the node's last parent goes
        by_parent = np.argsort(parent, kind="stable")
        chd_idx = child[by_parent]
        chd_ptr = np.concatenate([[0], np.cumsum(np.bincount(parent, minlength=n))])
        depth = np.zeros(n, dtype=np.int64)
        left = n_par.copy()
        frontier = np.flatnonzero(left == 0)
        order, level = [], 0
        while frontier.size:
            level += 1
            depth[frontier] = level
            order.append(frontier)
            cnt = chd_ptr[frontier + 1] - chd_ptr[frontier]
            at = np.repeat(chd_ptr[frontier] - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(int(cnt.sum()))
            kids = chd_idx[at]
            touched, gone = np.unique(kids, return_counts=True)
            left[touched] -= gone
            frontier = touched[left[touched] == 0]
        if sum(f.size for f in order) != n:
            raise ValueError("TaxonomyIndex: the parent lists contain a cycle")
        # closure in topological order: anc(v) = {v} | the union of its parents' lists
        anc = [None] * n
        total = 0
        for v in (np.concatenate(order).tolist() if order else []):
            lo, hi = par_ptr[v], par_ptr[v + 1]
            if hi == lo:
                row = np.asarray([v], dtype=np.int32)
            else:
                row = np.unique(np.concatenate([anc[p] for p in parent[lo:hi].tolist()] + [np.asarray([v], dtype=np.int32)]))
            anc[v] = row
            total += row.size
            if total >= MAX_CLOSURE:
                raise ValueError("TaxonomyIndex: the ancestor closure has 2^31 entries or more")
        anc_ptr = np.concatenate([[0], np.cumsum([r.size for r in anc])]) if n else np.zeros(1, dtype=np.int64)
        anc_idx = np.concatenate(anc) if n else np.zeros(0, dtype=np.int32)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        return cls(i32(depth), i32(anc_ptr), i32(anc_idx), i32(par_ptr), i32(parent))

    @classmethod
    def from_dataset(cls, dataset):
        """the masked taxonomy `dataset.graph.pred` of a MaskedGraphDataset (held-out in-edges already dropped) over all
        `dataset.node_features.shape[0]` node ids -- the CSR dataset.device_taxonomy uploads"""
        n = int(dataset.node_features.shape[0])
        pred = dataset.graph.pred
        cnt = np.asarray([len(pred.get(i, ())) for i in range(n)], dtype=np.int64)
        idx = np.asarray([p for i in range(n) for p in pred.get(i, ())], dtype=np.int64)
        return cls.from_parents(np.concatenate([[0], np.cumsum(cnt)]), idx)

    def to(self, device):
        """the arrays as int32 tensors resident on `device`"""
        return DeviceTaxonomyIndex(self, device)

    def ancestors(self, v):
        return self.anc_idx[self.anc_ptr[v]:self.anc_ptr[v + 1]]

    def parents(self, v):
        return self.par_idx[self.par_ptr[v]:self.par_ptr[v + 1]]


class DeviceTaxonomyIndex:
    """a TaxonomyIndex resident on one device (`host` keeps the numpy arrays).  Empty arrays are padded to one element: the C entry
    point refuses NULL pointers."""

    def __init__(self, host, device):
        self.host, self.n_nodes, self.device = host, host.n_nodes, torch.device(device)
        up = lambda a: torch.from_numpy(a if a.size else np.zeros(1, dtype=np.int32)).to(self.device)
        self.depth, self.anc_ptr, self.anc_idx = up(host.depth), up(host.anc_ptr), up(host.anc_idx)
        self.par_ptr, self.par_idx = up(host.par_ptr), up(host.par_idx)

    def to(self, device):
        return self if torch.device(device) == self.device else DeviceTaxonomyIndex(self.host, device)


def _host_index(index):
    return index.host if isinstance(index, DeviceTaxonomyIndex) else index


def _lca_depth(index, a, b):
    common = np.intersect1d(index.ancestors(a), index.ancestors(b), assume_unique=True)
    return int(index.depth[common].max()) if common.size else 0


def _relation(index, a, b, l):
    if a == b:
        return EXACT
    if a in index.ancestors(b):
        return ANCESTOR
    if b in index.ancestors(a):
        return DESCENDANT
    if np.intersect1d(index.parents(a), index.parents(b)).size:
        return SIBLING
    return RELATED if l > 0 else UNRELATED


def host_taxonomic(index, pred, gold_off, gold_idx):
    """numpy restatement of txe_taxo_slots.  pred [Q, K] node ids, gold_off [Q + 1], gold_idx: query q's gold parents are
    gold_idx[gold_off[q]:gold_off[q + 1]].  Returns dict(lca_depth, best_gold, relation), each [Q, K] int32: per slot the gold j* (position
    in q's list) with the largest wup(pred, gold) -- compared exactly, l_j (d_a + d_j') against l_j' (d_a + d_j) in Python integers; ties by
    the smaller relation code, then the smaller j -- with its lca_depth and relation.  A prediction outside [0, n) or no usable gold (an
    empty list; gold ids outside [0, n) are skipped): lca_depth 0, best_gold -1, relation 6."""
    index = _host_index(index)
    pred = np.asarray(pred, dtype=np.int64)
    gold_off = np.asarray(gold_off, dtype=np.int64).reshape(-1)
    gold_idx = np.asarray(gold_idx, dtype=np.int64).reshape(-1)
    Q, K = pred.shape
    n = index.n_nodes
    off = np.clip(gold_off, 0, gold_idx.size)
    out = dict(lca_depth=np.zeros((Q, K), dtype=np.int32), best_gold=np.full((Q, K), -1, dtype=np.int32),
               relation=np.full((Q, K), NONE, dtype=np.int32))
    memo = {}
    for q in range(Q):
        golds = gold_idx[off[q]:off[q + 1]].tolist()
        for r in range(K):
            a = int(pred[q, r])
            if not 0 <= a < n:
                continue
            da = int(index.depth[a])
            best = None                                                    # (l, d_b, rel, j)
            for j, b in enumerate(golds):
                if not 0 <= b < n:
                    continue
                if (a, b) not in memo:
                    l = _lca_depth(index, a, b)
                    memo[(a, b)] = (l, _relation(index, a, b, l))
                l, rel = memo[(a, b)]
                db = int(index.depth[b])
                if best is not None:
                    lhs, rhs = l * (da + best[1]), best[0] * (da + db)
                if best is None or lhs > rhs or (lhs == rhs and rel < best[2]):
                    best = (l, db, rel, j)
            if best is not None:
                out["lca_depth"][q, r], out["best_gold"][q, r], out["relation"][q, r] = best[0], best[3], best[2]
    return out


def _check_lists(n, pred, gold_off, gold_idx):
    if pred.dim() != 2 or pred.shape[1] < 1:
        raise ValueError(f"taxonomic_slots takes pred [Q, K] with K >= 1, got {tuple(pred.shape)}")
    Q, K = pred.shape
    if Q * K >= 2 ** 31:
        raise ValueError("taxonomic_slots takes Q * K < 2^31 slots")
    gold_off = np.asarray(gold_off, dtype=np.int64).reshape(-1)
    gold_idx = np.asarray(gold_idx, dtype=np.int64).reshape(-1)
    if gold_off.size != Q + 1 or (Q and (gold_off[0] < 0 or gold_off[-1] > gold_idx.size or np.any(np.diff(gold_off) < 0))):
        raise ValueError("taxonomic_slots: gold_off must be [Q + 1] ascending offsets into gold_idx")
    if gold_idx.size >= 2 ** 31:
        raise ValueError("taxonomic_slots takes fewer than 2^31 gold entries")
    if gold_idx.size and (gold_idx.min() < 0 or gold_idx.max() >= n):
        raise ValueError(f"taxonomic_slots: a gold id lies outside [0, {n})")
    return gold_off, gold_idx


def taxonomic_slots(index_dev, pred, gold_off, gold_idx):
    """txe_taxo_slots on the current stream: ONE launch, nothing read back.  index_dev: TaxonomyIndex.to(device); pred [Q, K] integer
    device tensor of node ids (ids outside [0, n) give relation 6); gold_off [Q + 1] / gold_idx: host arrays (or tensors) -- a gold id
    outside [0, n) is a ValueError before any launch.  Returns dict(lca_depth, best_gold, relation), each [Q, K] int32 on the device."""
    if not isinstance(index_dev, DeviceTaxonomyIndex):
        raise TypeError("taxonomic_slots takes TaxonomyIndex.to(device)")
    if not torch.is_tensor(pred) or pred.device != index_dev.device or pred.device.type == "cpu":
        raise RuntimeError("taxonomic_slots takes a prediction tensor on the index's GPU (no CPU fallback; host_taxonomic is the numpy form)")
    if pred.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"pred must be int32 or int64, got {pred.dtype}")
    to_host = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else a
    gold_off, gold_idx = _check_lists(index_dev.n_nodes, pred, to_host(gold_off), to_host(gold_idx))
    dev = pred.device
    Q, K = pred.shape
    if pred.dtype == torch.int64:                                          # ids beyond int32 are out of range whatever n is
        pred = torch.where((pred >= 0) & (pred < 2 ** 31), pred, torch.full_like(pred, -1))
    pred32 = pred.to(torch.int32).contiguous()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1), dtype=np.int32)).to(dev, non_blocking=True)
    goff, gidx = up(gold_off), up(gold_idx)
    out = {k: torch.empty((Q, K), dtype=torch.int32, device=dev) for k in ("lca_depth", "best_gold", "relation")}
    with _lib.on_device(dev):
        _lib.call("txe_taxo_slots", _lib.ptr(index_dev.anc_ptr), _lib.ptr(index_dev.anc_idx), _lib.ptr(index_dev.depth),
                  _lib.ptr(index_dev.par_ptr), _lib.ptr(index_dev.par_idx), index_dev.n_nodes, _lib.ptr(pred32), Q, K, _lib.ptr(goff),
                  _lib.ptr(gidx), int(gold_idx.size), _lib.ptr(out["lca_depth"]), _lib.ptr(out["best_gold"]), _lib.ptr(out["relation"]),
                  _lib.stream_ptr())
    return out


def best_gold_nodes(best_gold, gold_off, gold_idx):
    """the node id of every slot's chosen gold, gold_idx[gold_off[q] + best_gold[q, r]]; -1 where best_gold is -1.  Device tensors in,
    device tensor out (gold_off / gold_idx are uploaded if they are host arrays); numpy in, numpy out."""
    if torch.is_tensor(best_gold):
        dev = best_gold.device
        off = torch.as_tensor(np.asarray(gold_off) if not torch.is_tensor(gold_off) else gold_off).to(device=dev, dtype=torch.int64)
        idx = torch.as_tensor(np.asarray(gold_idx) if not torch.is_tensor(gold_idx) else gold_idx).to(device=dev, dtype=torch.int64)
        if idx.numel() == 0:
            return torch.full_like(best_gold, -1, dtype=torch.int64)
        at = (off[:-1, None] + best_gold.long()).clamp(0, idx.numel() - 1)
        return torch.where(best_gold >= 0, idx[at], torch.full_like(at, -1))
    best_gold = np.asarray(best_gold, dtype=np.int64)
    off, idx = np.asarray(gold_off, dtype=np.int64), np.asarray(gold_idx, dtype=np.int64)
    if idx.size == 0:
        return np.full(best_gold.shape, -1, dtype=np.int64)
    return np.where(best_gold >= 0, idx[np.clip(off[:-1, None] + best_gold, 0, idx.size - 1)], -1)


def wu_palmer(index, pred, best_gold_node, lca_depth):
    """Wu & Palmer similarity per slot, float64: 2.0 * l / (d_pred + d_gold) from the integers -- one exact product and one correctly
    rounded quotient, so the device and numpy agree bit for bit -- and 0 where the slot has no gold (best_gold_node < 0: relation 6).
    index: a TaxonomyIndex with numpy operands, TaxonomyIndex.to(device) with tensors of that device."""
    if torch.is_tensor(pred):
        if not isinstance(index, DeviceTaxonomyIndex):
            raise TypeError("wu_palmer on tensors takes TaxonomyIndex.to(device)")
        depth, n = index.depth, index.n_nodes
        valid = (best_gold_node >= 0) & (pred >= 0) & (pred < n)
        da = depth[pred.long().clamp(0, max(n - 1, 0))].to(torch.float64)
        db = depth[best_gold_node.long().clamp(0, max(n - 1, 0))].to(torch.float64)
        w = 2.0 * lca_depth.to(torch.float64) / (da + db)
        return torch.where(valid, w, torch.zeros_like(w))
    index = _host_index(index)
    pred, node = np.asarray(pred, dtype=np.int64), np.asarray(best_gold_node, dtype=np.int64)
    n = index.n_nodes
    valid = (node >= 0) & (pred >= 0) & (pred < n)
    da = index.depth[np.clip(pred, 0, max(n - 1, 0))].astype(np.float64)
    db = index.depth[np.clip(node, 0, max(n - 1, 0))].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = 2.0 * np.asarray(lca_depth, dtype=np.float64) / (da + db)
    return np.where(valid, w, 0.0)


def summarize(relation, wup):
    """the scalar metrics of a [Q, K] evaluation (tensors or numpy arrays): wu_palmer = mean over queries of slot 0's value,
    wu_palmer_at_k = mean over queries of the best value in the list, taxonomic_k = K, rel_<name> = the share of queries by slot 0's
    relation (they sum to 1).  Means are sum / Q with one rounding, as metric._exact_mean; Q == 0 gives NaN."""
    Q, K = relation.shape
    if torch.is_tensor(relation):
        counts = torch.bincount(relation[:, 0].long(), minlength=7).cpu().tolist() if Q and K else [0] * 7
        s0 = float(wup[:, 0].sum().item()) if Q and K else 0.0
        sk = float(wup.max(dim=1).values.sum().item()) if Q and K else 0.0
    else:
        counts = np.bincount(np.asarray(relation)[:, 0], minlength=7).tolist() if Q and K else [0] * 7
        s0 = float(np.asarray(wup)[:, 0].sum()) if Q and K else 0.0
        sk = float(np.asarray(wup).max(axis=1).sum()) if Q and K else 0.0
    mean = lambda s: s / Q if Q and K else float("nan")
    out = dict(wu_palmer=mean(s0), wu_palmer_at_k=mean(sk), taxonomic_k=int(K))
    out.update({"rel_" + name: mean(float(c)) for name, c in zip(RELATION_NAMES, counts)})
    return out
