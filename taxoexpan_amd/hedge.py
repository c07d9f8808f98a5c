"""Hedged placement (Deng et al., "Hedging your bets", 2012): answer with the DEEPEST candidate whose subtree probability
reaches a threshold tau.  With calibrated p(parent | query) (calibrate.py) the answer is right about tau of the time and as specific as
the model can afford.  Everything lives in candidate-column space -- cand[0..G): distinct node ids, column g = cand[g]:

    sub(a)      the columns of all candidates in {a} | descendants(a) on the taxonomy, ascending, a included.  Descendants are the
                transpose of TaxonomyIndex's ancestor closure: a node reachable along two paths counts once, non-candidates are
                dropped, and candidates below a dropped node still count for the ancestors above it.
    depth[a]    TaxonomyIndex.depth of the candidate's node (longest chain)
    t[q, g]     fl32(beta z[q, g]), z = the score or its negative, beta = fl32(1 / T): what scoring.score_moments_fused forms
    p[q, g]     fl32(exp(float64(t[q, g]) - lse[q])), lse = that function's float64 value; 0 on a row whose lse is not finite
    mass[q, a]  the sum of p[q, d] over d in sub(a), in float64, in an order fixed by the list alone: the list is cut into consecutive
                slices of SLICE entries, every slice is summed left to right from 0.0, the slice sums are added left to right
    hedge[q, tau]  the column a with mass[q, a] >= tau (float64 compare) of the largest depth; ties: the larger mass, then the smaller
                column; -1 when none qualifies (a forest, a non-finite lse, G = 0), reported with its mass (NaN for -1) and depth (0)

`HedgeIndex` is built on the host; `.to(device)` keeps it resident.  `probabilities` / `subtree_mass` / `hedge_block` are the launches
of csrc/txe_hedge.hip, `hedged_parents` the driver over query blocks; `host_probabilities` / `host_subtree_mass` / `host_hedge` are the
numpy restatement.  There is no CPU fallback for device tensors and no device route for host arrays.
"""
import collections
import ctypes
import math
import types

import numpy as np
import torch

from . import _lib, scoring
from .taxometric import DeviceTaxonomyIndex

SLICE = _lib.HEDGE_SLICE                        # TXE_HEDGE_SLICE of include/txe.h: the unit of the summation order
MAX_THRESHOLDS = _lib.HEDGE_MAX_THRESHOLDS      # TXE_HEDGE_MAX_THRESHOLDS
QUERY_TILE = 64                                 # queries per wave of the sweep: blocks are rounded to it
MAX_ENTRIES = 2 ** 31                           # the lists are addressed with int32 offsets

Hedged = collections.namedtuple("Hedged", "node_col mass depth")       # each [Q, T]: int32 column (-1 = none), float64, int32


def check_thresholds(thresholds):
    """a float or a sequence of 1 to MAX_THRESHOLDS floats, each finite and in (0, 1], as a list of Python floats; else ValueError"""
    if isinstance(thresholds, (str, bytes, bool)) or thresholds is None:
        raise ValueError(f"hedge: thresholds must be a number or a sequence of numbers in (0, 1], got {thresholds!r}")
    try:
        vals = [thresholds] if np.ndim(thresholds) == 0 else list(np.asarray(thresholds).reshape(-1).tolist())
        vals = [float(v) for v in vals]
    except (TypeError, ValueError):
        raise ValueError(f"hedge: thresholds must be a number or a sequence of numbers in (0, 1], got {thresholds!r}") from None
    if not 1 <= len(vals) <= MAX_THRESHOLDS:
        raise ValueError(f"hedge: 1 to {MAX_THRESHOLDS} thresholds go in one sweep, got {len(vals)}")
    for v in vals:
        if not (math.isfinite(v) and 0.0 < v <= 1.0):
            raise ValueError(f"hedge: every threshold must be finite and in (0, 1], got {v!r}")
    return vals


class HedgeIndex:
    """sub_ptr [G + 1] / sub_idx (row a = sub(a), ascending, a included) and depth [G] of a candidate list on a TaxonomyIndex, plus the
    sweep's work list: item i = (item_row[i], item_slice[i], item_part[i]) in row order then slice order -- one item per SLICE entries
    of a row; item_part = -1 for a row of one slice, else the slice's position among the long rows' partial sums; long_row / long_ptr =
    the rows of more than SLICE entries and their ranges of positions.  All int32 numpy arrays."""

    def __init__(self, cand, sub_ptr, sub_idx, depth, item_row, item_slice, item_part, long_row, long_ptr):
        self.cand, self.sub_ptr, self.sub_idx, self.depth = cand, sub_ptr, sub_idx, depth
        self.item_row, self.item_slice, self.item_part, self.long_row, self.long_ptr = item_row, item_slice, item_part, long_row, long_ptr
        self.G, self.nnz = int(depth.shape[0]), int(sub_idx.shape[0])
        self.n_items, self.n_long, self.n_part = int(item_row.shape[0]), int(long_row.shape[0]), int(long_ptr[-1])

    @classmethod
    def build(cls, taxonomy_index, cand):
        """taxonomy_index: a taxometric.TaxonomyIndex (or its .to(device)); cand: the G distinct node ids of the candidate columns.
        ValueError: a duplicate candidate, an id outside [0, n), 2^31 list entries or more."""
        tix = taxonomy_index.host if isinstance(taxonomy_index, DeviceTaxonomyIndex) else taxonomy_index
        cand = np.asarray(cand, dtype=np.int64).reshape(-1)
        n, G = tix.n_nodes, int(cand.size)
        if G and (cand.min() < 0 or cand.max() >= n):
            raise ValueError(f"HedgeIndex: a candidate id lies outside [0, {n})")
        if np.unique(cand).size != G:
            raise ValueError("HedgeIndex: the candidate list holds a node twice")
        col_of = np.full(n, -1, dtype=np.int64)
        col_of[cand] = np.arange(G)
        # the closure's entries (node v, ancestor u) with both ends among the candidates, as (row = u's column, entry = v's column)
        anc_ptr = tix.anc_ptr.astype(np.int64)
        low = np.repeat(col_of, np.diff(anc_ptr))
        up = col_of[tix.anc_idx.astype(np.int64)] if tix.anc_idx.size else np.zeros(0, dtype=np.int64)
        keep = (low >= 0) & (up >= 0)
        row, ent = up[keep], low[keep]
        if row.size >= MAX_ENTRIES:
            raise ValueError("HedgeIndex: the subtree lists have 2^31 entries or more")
        # the transpose by a counting sort on the row: offsets = the prefix sum of the rows' counts; the stable pass keeps the entries,
        # sorted first, ascending inside every row
        sub_ptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=G))]) if G else np.zeros(1, dtype=np.int64)
        by_entry = np.argsort(ent, kind="stable")
        sub_idx = ent[by_entry][np.argsort(row[by_entry], kind="stable")]
        depth = tix.depth[cand] if G else np.zeros(0, dtype=np.int32)
        # the work list: a pure function of the rows' lengths
        n_slices = np.maximum((np.diff(sub_ptr) + SLICE - 1) // SLICE, 1)
        item_row = np.repeat(np.arange(G, dtype=np.int64), n_slices)
        first = np.concatenate([[0], np.cumsum(n_slices)])[:-1]
        item_slice = np.arange(item_row.size, dtype=np.int64) - np.repeat(first, n_slices)
        long_row = np.flatnonzero(n_slices > 1)
        long_ptr = np.concatenate([[0], np.cumsum(n_slices[long_row])])
        part_first = np.full(G, -1, dtype=np.int64)
        part_first[long_row] = long_ptr[:-1]
        item_part = np.where(part_first[item_row] >= 0, part_first[item_row] + item_slice, -1) if G else np.zeros(0, dtype=np.int64)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        return cls(cand, i32(sub_ptr), i32(sub_idx), i32(depth), i32(item_row), i32(item_slice), i32(item_part), i32(long_row), i32(long_ptr))

    def row(self, a):
        return self.sub_idx[self.sub_ptr[a]:self.sub_ptr[a + 1]]

    def to(self, device):
        """the arrays as int32 tensors resident on `device`"""
        return DeviceHedgeIndex(self, device)


class DeviceHedgeIndex:
    """a HedgeIndex resident on one device (`host` keeps the numpy arrays).  Empty arrays are padded to one element: the C entry point
    refuses NULL pointers."""
    _ARRAYS = ("sub_ptr", "sub_idx", "depth", "item_row", "item_slice", "item_part", "long_row", "long_ptr")

    def __init__(self, host, device):
        self.host, self.device = host, torch.device(device)
        self.G, self.nnz, self.n_items, self.n_long, self.n_part = host.G, host.nnz, host.n_items, host.n_long, host.n_part
        for k in self._ARRAYS:
            a = getattr(host, k)
            setattr(self, k, torch.from_numpy(a if a.size else np.zeros(1, dtype=np.int32)).to(self.device))

    def to(self, device):
        return self if torch.device(device) == self.device else DeviceHedgeIndex(self.host, device)


def _host_index(index):
    return index.host if isinstance(index, DeviceHedgeIndex) else index


# ---------------------------------------------------------------------------------------------------------------
# the numpy restatement
# ---------------------------------------------------------------------------------------------------------------
def host_probabilities(S, lse, temperature=1.0, larger_is_better=True):
    """p [Q, G] fp32 of a score array S [Q, G] and lse [Q] float64 (scoring.host_score_moments' or the device's): the module's
    definition of t and p, with zeros on every row whose lse is not finite"""
    beta = np.float32(scoring._beta_of(temperature))
    z = np.asarray(torch.as_tensor(S).detach().cpu(), dtype=np.float32)
    z = z if larger_is_better else -z
    lse = np.asarray(torch.as_tensor(lse).detach().cpu(), dtype=np.float64).reshape(-1)
    if lse.shape[0] != z.shape[0]:
        raise ValueError(f"host_probabilities: lse must hold one value per row of S, got {lse.shape[0]} for {z.shape[0]}")
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        t = (beta * z).astype(np.float32).astype(np.float64)
        p = np.exp(t - lse[:, None]).astype(np.float32)
    p[~np.isfinite(lse)] = 0.0
    return p


def host_subtree_mass(index, P):
    """mass [G, Q] float64 (candidate-major, as subtree_mass returns it) of probabilities P [Q, G]: per row its slices of SLICE entries
    summed left to right from 0.0 (np.cumsum adds one element at a time, in order), the slice sums added left to right"""
    index = _host_index(index)
    P64 = np.asarray(torch.as_tensor(P).detach().cpu(), dtype=np.float64)
    if P64.ndim != 2 or P64.shape[1] != index.G:
        raise ValueError(f"host_subtree_mass: P must be [Q, {index.G}], got {P64.shape}")
    PT = np.ascontiguousarray(P64.T)
    mass = np.zeros((index.G, P64.shape[0]), dtype=np.float64)
    for a in range(index.G):
        row = index.row(a)
        total = None
        for s0 in range(0, row.size, SLICE):
            part = np.cumsum(np.concatenate([np.zeros((1, PT.shape[1])), PT[row[s0:s0 + SLICE]]]), axis=0)[-1]
            total = part if total is None else total + part
        if total is not None:
            mass[a] = total
    return mass


def host_hedge(index, P, thresholds, mass=None):
    """Hedged(node_col [Q, T] int32, mass [Q, T] float64, depth [Q, T] int32) as numpy arrays from probabilities P [Q, G], or from a
    precomputed mass [G, Q] (then P may be None)"""
    index = _host_index(index)
    thr = check_thresholds(thresholds)
    mass = host_subtree_mass(index, P) if mass is None else np.asarray(mass, dtype=np.float64)
    G, Q = mass.shape
    col = np.full((Q, len(thr)), -1, dtype=np.int32)
    out_m = np.full((Q, len(thr)), np.nan, dtype=np.float64)
    out_d = np.zeros((Q, len(thr)), dtype=np.int32)
    for t, tau in enumerate(thr):
        ok = mass >= tau
        for q in range(Q):
            c = np.flatnonzero(ok[:, q])
            if not c.size:
                continue
            c = c[index.depth[c] == index.depth[c].max()]
            c = c[mass[c, q] == mass[c, q].max()]
            col[q, t], out_m[q, t], out_d[q, t] = c.min(), mass[c.min(), q], index.depth[c.min()]
    return Hedged(col, out_m, out_d)


# ---------------------------------------------------------------------------------------------------------------
# the launches
# ---------------------------------------------------------------------------------------------------------------
def _pitch(nq):
    return max((int(nq) + QUERY_TILE - 1) // QUERY_TILE * QUERY_TILE, QUERY_TILE)


def probabilities(S, lse, beta=1.0, larger_is_better=True, out=None):
    """txe_hedge_probs on the current stream: one launch.  S [nq, G] fp32 score block (rows on any pitch), lse [nq] float64, beta = the
    fp32 scale 1 / T.  Returns PT [G, nq] fp32, candidate-major: a view of a [G, pitch] buffer whose rows start 256-byte aligned (`out`:
    such a buffer to reuse, at least [G, nq rounded up to 64])."""
    from . import ops
    beta = ops._check_beta(beta)
    if not torch.is_tensor(S) or S.device.type == "cpu":
        raise RuntimeError("hedge.probabilities takes a score block on the GPU (no CPU fallback; host_probabilities is the numpy form)")
    if S.dim() != 2 or S.dtype != torch.float32 or (S.numel() and S.shape[1] > 1 and S.stride(1) != 1):
        raise ValueError("hedge.probabilities takes S [nq, G] fp32 with unit column stride")
    nq, G = S.shape
    if not torch.is_tensor(lse) or lse.dtype != torch.float64 or lse.shape != (nq,) or lse.device != S.device:
        raise ValueError("hedge.probabilities takes lse [nq] float64 on S's device")
    lse = lse.contiguous()
    ldq = _pitch(nq)
    if out is None:
        out = torch.empty((max(G, 1), ldq), dtype=torch.float32, device=S.device)
    elif out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] < G or out.shape[1] < ldq or not out.is_contiguous() or out.device != S.device:
        raise ValueError(f"hedge.probabilities: out must be a contiguous fp32 [>= {G}, >= {ldq}] buffer on S's device")
    if nq and G:
        with _lib.on_device(S.device):
            _lib.call("txe_hedge_probs", _lib.ptr(S), S.stride(0) if nq > 1 else max(S.stride(0), G), nq, G, _lib.ptr(lse), beta,
                      0 if larger_is_better else 1, _lib.ptr(out), out.stride(0), _lib.stream_ptr())
    return out[:G, :nq]


def _check_pt(index_dev, PT):
    if not isinstance(index_dev, DeviceHedgeIndex):
        raise TypeError("the sweep takes HedgeIndex.to(device)")
    if not torch.is_tensor(PT) or PT.device != index_dev.device or PT.device.type == "cpu":
        raise RuntimeError("the sweep takes probabilities on the index's GPU (no CPU fallback; host_subtree_mass / host_hedge are the numpy forms)")
    if PT.dim() != 2 or PT.dtype != torch.float32 or PT.shape[0] != index_dev.G or (PT.numel() and PT.shape[1] > 1 and PT.stride(1) != 1):
        raise ValueError(f"the sweep takes PT [G = {index_dev.G}, nq] fp32, candidate-major with unit query stride, got {tuple(PT.shape)}")
    nq = int(PT.shape[1])
    return nq, (PT.stride(0) if index_dev.G > 1 else max(PT.stride(0), nq))


def _sweep(ix, PT, ldq, nq, thr, mass, out):
    n_thr = len(thr)
    taus = (ctypes.c_double * max(n_thr, 1))(*thr)
    with _lib.on_device(ix.device):
        need = _lib.call("txe_hedge_sweep_ws_bytes", ix.n_items, ix.n_long, ix.n_part, nq, n_thr)
        ws = torch.empty(need, dtype=torch.uint8, device=ix.device)
        _lib.call("txe_hedge_sweep", _lib.ptr(ix.sub_ptr), _lib.ptr(ix.sub_idx), _lib.ptr(ix.depth), ix.G, ix.nnz, _lib.ptr(ix.item_row),
                  _lib.ptr(ix.item_slice), _lib.ptr(ix.item_part), ix.n_items, _lib.ptr(ix.long_row), _lib.ptr(ix.long_ptr), ix.n_long,
                  ix.n_part, _lib.ptr(PT), ldq, nq, ctypes.addressof(taus) if n_thr else None, n_thr, _lib.ptr(mass),
                  mass.stride(0) if mass is not None else 0, *((_lib.ptr(t) for t in out) if out is not None else (None, None, None)),
                  _lib.ptr(ws), need, _lib.stream_ptr())


def subtree_mass(index_dev, PT):
    """the full mass block (store mode): float64 [G, nq], candidate-major, bit-equal to host_subtree_mass on the same probabilities.
    For tests and moderate sizes: it is G x nq x 8 bytes.  PT: probabilities' result, or any fp32 [G, nq] with unit query stride."""
    nq, ldq = _check_pt(index_dev, PT)
    mass = torch.empty((index_dev.G, max(nq, 1)), dtype=torch.float64, device=index_dev.device)
    if nq and index_dev.G:
        _sweep(index_dev, PT, ldq, nq, [], mass, None)
    return mass[:, :nq]


def hedge_block(index_dev, PT, thresholds):
    """the reducing mode: Hedged(node_col, mass, depth), each [nq, T] on the device, bit-equal to host_hedge on the same probabilities;
    no mass matrix is written"""
    thr = check_thresholds(thresholds)
    nq, ldq = _check_pt(index_dev, PT)
    dev = index_dev.device
    out = Hedged(torch.full((nq, len(thr)), -1, dtype=torch.int32, device=dev),
                 torch.full((nq, len(thr)), float("nan"), dtype=torch.float64, device=dev),
                 torch.zeros((nq, len(thr)), dtype=torch.int32, device=dev))
    if nq and index_dev.G:
        _sweep(index_dev, PT, ldq, nq, thr, None, out)
    return out


def default_block(G, Q):
    """queries per block of hedged_parents: one fp32 score block and one probability block each at or below
    scoring.RETRIEVE_BLOCK_BYTES, a multiple of the sweep's query tile (at least one tile), no more than the queries need"""
    fit = scoring.RETRIEVE_BLOCK_BYTES // (4 * max(int(G), 1))
    return max(QUERY_TILE, min(fit // QUERY_TILE * QUERY_TILE, _pitch(Q)))


def hedged_parents(match, hg, queries, index_dev, thresholds, temperature=1.0, larger_is_better=True, block=None, lse=None):
    """The hedged parent of every query against ALL candidates hg [G, l] (already encoded), per threshold.  Per query block: lse from
    scoring.score_moments_fused (one call for all queries; `lse`: that float64 [Q] tensor if the caller has it), the score block by the
    matcher's store route (scoring.prepare_matcher(...).score; evaluate._score_blocks for a matcher without a fused route), one
    txe_hedge_probs launch and one sweep in hedge mode.  Returns Hedged(node_col, mass, depth), each [Q, T] on hg's device; node_col is
    the candidate COLUMN (index_dev.host.cand maps it to a node id), -1 = no column qualifies."""
    if not isinstance(index_dev, DeviceHedgeIndex):
        raise TypeError("hedged_parents takes HedgeIndex.to(device)")
    thr = check_thresholds(thresholds)
    beta = scoring._beta_of(temperature)
    dev = hg.device
    Q, G = int(queries.shape[0]), int(hg.shape[0])
    if index_dev.G != G:
        raise ValueError(f"hedged_parents: the index has {index_dev.G} candidate columns, hg has {G} rows")
    if block is None:
        block = default_block(G, Q)
    if isinstance(block, bool) or int(block) != block or int(block) < 1:
        raise ValueError(f"hedged_parents: block must be an integer >= 1, got {block!r}")
    block = int(block)
    T = len(thr)
    out = Hedged(torch.full((Q, T), -1, dtype=torch.int32, device=dev), torch.full((Q, T), float("nan"), dtype=torch.float64, device=dev),
                 torch.zeros((Q, T), dtype=torch.int32, device=dev))
    if Q == 0 or G == 0:
        return out
    with torch.no_grad():
        if lse is None:
            lse = scoring.score_moments_fused(match, hg, queries, larger_is_better, 1.0 / beta).lse
        nb = min(block, Q)
        pbuf = torch.empty((G, _pitch(nb)), dtype=torch.float32, device=dev)
        if scoring.fused_matcher_ok(match):
            pm = scoring.prepare_matcher(match, hg)
            sbuf = torch.empty((nb, (G + 3) // 4 * 4), dtype=torch.float32, device=dev)
            blocks = ((q0, pm.score(queries[q0:q0 + block], out=sbuf[:min(block, Q - q0), :G])) for q0 in range(0, Q, block))
        else:
            from .evaluate import _score_blocks
            blocks = ((q0, S.float().contiguous()) for q0, S in _score_blocks(types.SimpleNamespace(match=match), hg, queries, block))
        for q0, S in blocks:
            n = S.shape[0]
            PT = probabilities(S, lse[q0:q0 + n], beta, larger_is_better, out=pbuf)
            h = hedge_block(index_dev, PT, thr)
            for dst, src in zip(out, h):
                dst[q0:q0 + n] = src
    return out
