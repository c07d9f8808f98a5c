"""The training losses of the reference's model/loss.py on the device, each a HIP launch chain that leaves the sum-reduced loss AND its
gradient (no autograd graph of small torch kernels behind it, no read-back):

    info_nce_loss     loss.py:52-57 -- the loss of the PGAT+LBM training path (config "loss": "info_nce_loss"; trainer.py:52-56 regroups
                      the scores to [queries, 1 + negatives] and passes all-zero targets): one launch (csrc/txe_loss.hip)
    bce_loss          loss.py:21-29 -- the loss of nine of the reference's eleven configs: one launch (csrc/txe_pairloss.hip)
    square_exp_loss   loss.py:12-19: one launch
    margin_rank_loss  loss.py:31-50 without its `target.cpu()`, its regex over the label bytes and its itertools.product: five enqueued
                      steps on the stream, nothing read back
    host_bce_loss / host_square_exp_loss / host_margin_rank_loss   the numpy float64 restatements (the written definitions; the tests
                      compare against them)
    taxo_info_nce     an addition: info_nce_loss with a Wu & Palmer margin on every negative, from the anchors of the batch and a resident
                      taxonomy index (csrc/txe_taxoloss.hip; host_taxo_margins / host_taxo_info_nce: its numpy restatement)
    in_batch_info_nce an addition: every query of a batch against ALL of the batch's egonets, masked by the taxonomy (csrc/txe_inbatch.hip,
                      ops.InBatchNCEFunction; host_in_batch_nce: its float64 restatement)

The last three device losses take (output [B] or [B, 1], target [B] int32 / int64) as trainer.py:57-58 passes them.  An entry is a
positive iff its label is 1.  Only `nll_loss` (no config uses it) stays with torch."""
import numpy as np
import torch

from . import _lib


class _InfoNCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, target):
        x = output if (output.dtype == torch.float32 and output.stride(-1) == 1) else output.float().contiguous()
        B, C = x.shape
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        d_x = torch.empty((B, C), dtype=torch.float32, device=x.device)
        tgt = None
        if target is not None:
            tgt = target if (target.dtype == torch.int64 and target.is_contiguous()) else target.to(torch.int64).contiguous()
        _lib.call("txe_info_nce", x.data_ptr(), x.stride(0) if B > 1 else C, B, C, None if tgt is None else tgt.data_ptr(),
                  loss.data_ptr(), d_x.data_ptr(), C, _lib.stream_ptr())
        ctx.save_for_backward(d_x)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        (d_x,) = ctx.saved_tensors
        return _scaled(d_x, grad_loss), None


def _scaled(d_x, grad_loss):
    """the saved gradient times the upstream one; the cached unit constant of LossTensor.backward is recognised by its address"""
    unit = _UNIT.get(grad_loss.device)
    if unit is not None and grad_loss.data_ptr() == unit.data_ptr() and grad_loss.numel() == 1:
        return d_x                              # d_x * 1: the plain `loss.backward()` of trainer.py:60 (LossTensor.backward below)
    return d_x * grad_loss


_UNIT = {}      # device -> the constant 1.0 that `loss.backward()` starts from (never written after its creation)


class LossTensor(torch.Tensor):
    """The scalar loss.  `loss.backward()` without a gradient (trainer/trainer.py:60) makes autograd allocate a ones tensor and fill it
    (one ~5 us launch), and the loss function's backward then multiplies its saved gradient by that 1.0 (another): here the call starts
    from a cached device constant, which the loss functions' backward (_scaled) recognises by its address and answers with the saved
    gradient itself -- the same numbers, two launches fewer per step.  Any other use (an explicit gradient, arithmetic on the loss first,
    torch.autograd.backward / grad) takes the ordinary path."""

    def backward(self, gradient=None, retain_graph=None, create_graph=False, inputs=None):
        if gradient is None and self.numel() == 1 and self.is_cuda and not create_graph:
            gradient = _UNIT.get(self.device)
            if gradient is None:
                gradient = _UNIT[self.device] = torch.ones((), dtype=self.dtype, device=self.device)
            if gradient.dtype != self.dtype:
                gradient = None
        return super().backward(gradient, retain_graph, create_graph, inputs)


def info_nce_loss(output, target=None):
    """output: (batch_size, 1 + negative_size) scores; target: (batch_size,) long (all zeros in trainer.py:53; None means that).
    Returns sum-reduced cross entropy, like the reference."""
    if output.dim() != 2:
        raise ValueError("info_nce_loss expects a [batch, 1 + negatives] tensor")
    if not output.is_cuda:
        raise RuntimeError("taxoexpan_amd.loss.info_nce_loss runs on the MI355X only (no CPU path)")
    return _InfoNCE.apply(output, target).as_subclass(LossTensor)


# ---- taxonomy-aware InfoNCE: Wu & Palmer margins on the negatives --------------------------------------------------------

DIST_SCALE = 2 ** 20           # dist_total counts floor(d * 2^20) per negative


def _checked_gamma(gamma, who):
    try:
        g = float(gamma)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: gamma must be a finite number >= 0, got {gamma!r}") from None
    if isinstance(gamma, bool) or not np.isfinite(g) or g < 0:
        raise ValueError(f"{who}: gamma must be a finite number >= 0, got {gamma!r}")
    return g


class _TaxoInfoNCE(torch.autograd.Function):
    """txe_info_nce_taxo: forward leaves the loss and d_x; backward scales d_x"""

    @staticmethod
    def forward(ctx, output, anchors, index, gamma, dist_total):
        x = output if (output.dtype == torch.float32 and output.stride(-1) == 1) else output.float().contiguous()
        a = anchors if anchors.stride(-1) == 1 else anchors.contiguous()
        Q, C = x.shape
        dev = x.device
        with _lib.on_device(dev):
            loss = torch.empty((), dtype=torch.float32, device=dev)
            d_x = torch.empty((Q, C), dtype=torch.float32, device=dev)
            wsb = _lib.pure("txe_info_nce_taxo_ws_bytes", Q)
            ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
            _lib.call("txe_info_nce_taxo", x.data_ptr(), x.stride(0) if Q > 1 else C, Q, C, a.data_ptr(), a.stride(0) if Q > 1 else C,
                      index.anc_ptr.data_ptr(), index.anc_idx.data_ptr(), index.depth.data_ptr(), index.n_nodes, gamma, loss.data_ptr(),
                      d_x.data_ptr(), C, None, None if dist_total is None else dist_total.data_ptr(), ws.data_ptr(), wsb,
                      _lib.stream_ptr())
        ctx.save_for_backward(d_x)
        ctx.dtype = output.dtype
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        (d_x,) = ctx.saved_tensors
        d = _scaled(d_x, grad_loss)
        return (d if ctx.dtype == torch.float32 else d.to(ctx.dtype)), None, None, None, None


def taxo_info_nce(output, anchors, index, gamma, dist_total=None):
    """info_nce_loss with a taxonomic margin on every negative (an addition): a negative far from the true parent must be
    beaten by more.  output [Q, C]: the scores of Q groups, column 0 the positive (train_epoch's regrouping); anchors [Q, C] int32 on
    the same device: the taxonomy node every column's egonet is anchored at (a DeviceBatchLoader(attach_anchors=True) attaches it as
    g.anchors); index: TaxonomyIndex.to(device) (TypeError otherwise).  With d = 1 - wu_palmer(anchor, the group's positive) in float64
    (0 in column 0 and where either node lies outside the index), m = float32(gamma * d) and y = output + m:
        loss = sum over groups of logsumexp(y) - output[:, 0],    d loss / d output = softmax(y) - [column 0]
    csrc/txe_taxoloss.hip, one launch and a finish step; loss.host_taxo_info_nce is the written definition.  gamma: finite and >= 0
    (ValueError otherwise); 0 gives info_nce_loss's gradient bit for bit.  The margin is added to WHATEVER THE MODEL OUTPUTS -- for LBM
    that is exp(b), not b -- so the scale of gamma is the user's to choose against the scale of the scores.  A query with several
    parents is measured against the positive of its own group only (its other parents never appear as negatives: node2masks removes
    them).  No gradient flows into d.  dist_total: None, or an int64 [1] device counter that gains sum over the negatives of
    floor(d * 2^20) (train_epoch's mean_taxo_distance).  Returns the sum-reduced loss as a LossTensor."""
    from .taxometric import DeviceTaxonomyIndex
    if not isinstance(index, DeviceTaxonomyIndex):
        raise TypeError("taxo_info_nce takes TaxonomyIndex.to(device)")
    if not (torch.is_tensor(output) and torch.is_tensor(anchors)):
        raise TypeError("taxo_info_nce takes tensors")
    if not output.is_cuda:
        raise RuntimeError("taxoexpan_amd.loss.taxo_info_nce runs on the MI355X only (no CPU path; loss.host_taxo_info_nce is the restatement)")
    gamma = _checked_gamma(gamma, "taxo_info_nce")
    if output.dim() != 2 or output.shape[1] < 1:
        raise ValueError(f"taxo_info_nce takes scores [groups, 1 + negatives], got {tuple(output.shape)}")
    if tuple(anchors.shape) != tuple(output.shape):
        raise ValueError(f"one anchor per score: anchors {tuple(anchors.shape)} against scores {tuple(output.shape)}")
    if anchors.dtype != torch.int32:
        raise ValueError(f"anchors must be int32, got {anchors.dtype}")
    if not output.dtype.is_floating_point:
        raise ValueError(f"scores must be floating point, got {output.dtype}")
    if anchors.device != output.device or index.device != output.device:
        raise ValueError("scores, anchors and the taxonomy index must be on one device")
    if output.numel() >= 2 ** 31:
        raise ValueError("taxo_info_nce takes fewer than 2^31 scores")
    if dist_total is not None and not (torch.is_tensor(dist_total) and dist_total.dtype == torch.int64 and dist_total.numel() == 1
                                       and dist_total.device == output.device):
        raise ValueError("dist_total must be an int64 [1] tensor on the scores' device")
    return _TaxoInfoNCE.apply(output, anchors, index, gamma, dist_total).as_subclass(LossTensor)


def host_taxo_margins(index, anchors, gamma):
    """the margins of taxo_info_nce in numpy -- the written definition: (d float64 [Q, C], m float32 [Q, C]).  anchors [Q, C] node ids,
    column 0 the positive.  d = 1.0 - 2.0 * lca_depth / (depth_a + depth_p) from taxometric's own host helpers (the evaluation metric's
    integers: an exact product, one correctly rounded quotient, one subtraction); 0 in column 0 and where the anchor or the group's
    positive lies outside [0, n).  m = float32(float64(gamma) * d): one product, one cast."""
    from .taxometric import _host_index, _lca_depth
    index = _host_index(index)
    gamma = _checked_gamma(gamma, "host_taxo_margins")
    anchors = np.asarray(anchors)
    if anchors.ndim != 2 or anchors.shape[1] < 1:
        raise ValueError(f"anchors must be [groups, 1 + negatives], got {anchors.shape}")
    anchors = anchors.astype(np.int64)
    n = index.n_nodes
    d = np.zeros(anchors.shape, dtype=np.float64)
    memo = {}
    for i in range(anchors.shape[0]):
        p = int(anchors[i, 0])
        if not 0 <= p < n:
            continue
        for c in range(1, anchors.shape[1]):
            a = int(anchors[i, c])
            if not 0 <= a < n:
                continue
            if (a, p) not in memo:
                lca = np.float64(_lca_depth(index, a, p))
                memo[(a, p)] = 1.0 - 2.0 * lca / np.float64(int(index.depth[a]) + int(index.depth[p]))
            d[i, c] = memo[(a, p)]
    return d, (np.float64(gamma) * d).astype(np.float32)


def host_taxo_info_nce(x, anchors, index, gamma):
    """numpy float64 restatement of txe_info_nce_taxo -- the written definition: (loss, d_x [Q, C], row_loss [Q]) from
    y = x.astype(float32) + m in fp32 (host_taxo_margins' m), everything after that in float64"""
    x32 = np.asarray(x).astype(np.float32)
    _, m = host_taxo_margins(index, anchors, gamma)
    if x32.shape != m.shape:
        raise ValueError(f"one anchor per score: anchors {m.shape} against scores {x32.shape}")
    with np.errstate(over="ignore", invalid="ignore"):
        y = (x32 + m).astype(np.float64)
        mx = y.max(axis=1, keepdims=True)
        e = np.exp(y - mx)
        s = e.sum(axis=1, keepdims=True)
        row = mx[:, 0] + np.log(s[:, 0]) - x32[:, 0].astype(np.float64)
        d_x = e / s
        d_x[:, 0] -= 1.0
    return float(np.sum(row)), d_x, row


# ---- in-batch negatives -------------------------------------------------------------------------------------------------------------

def is_bilinear_matcher(match):
    """is `match` a BIM / LBM matcher?  scoring.prepare_matcher's rule: a bilinear weight `W` and the `apply_exp` switch (by attribute,
    not by class: the reference's own model with its import swapped passes too).  in_batch_info_nce and train_epoch(in_batch=True) ask it."""
    return hasattr(match, "W") and hasattr(match, "apply_exp")


def in_batch_info_nce(match, hg, queries, groups, valid_total=None, query_grad=False):
    """The in-batch loss of one training batch: every query against EVERY graph vector of the batch, not only its own
    1 + negative_size -- the other queries' egonets are negatives whose encoder work is already paid -- without the columns the taxonomy
    forbids (sampler.InBatchGroups: an anchor in node2masks[query] is the query's other parent, a sibling's positive or a descendant).
    match: a BIM / LBM matcher (TypeError otherwise); the cross entropy is taken over its output, b or exp(b), as info_nce_loss takes
    model(g, h, qf).  hg [G, l]: the graph vectors, e.g. encode_graph's (a DeferredGraphVector is materialised: the folded output layer
    never forms the hg this product needs).  queries [Q, r]: one row per query (a batch's `qf.rows`; an ops.RepeatedRows gives them).
    valid_total: None, or an int64 [1] device counter that gains the batch's valid pairs (train_epoch's mean_negatives).
    Returns the sum-reduced loss as a LossTensor; gradients reach hg and match.W, not the queries -- query rows that ask for a gradient
    are refused (ValueError) unless query_grad=True, which train_epoch passes when a feature_table.FeatureTable trains them."""
    from . import ops
    from .model_zoo import _graph_vector
    if not is_bilinear_matcher(match):
        raise TypeError(f"in_batch_info_nce takes a BIM / LBM matcher, got {type(match).__name__}")
    if isinstance(queries, ops.RepeatedRows):
        queries = queries.rows
    hg = _graph_vector(hg)
    if not (torch.is_tensor(hg) and torch.is_tensor(queries) and hg.dim() == 2 and queries.dim() == 2):
        raise ValueError("in_batch_info_nce takes graph vectors [G, l] and query rows [Q, r]")
    if not hg.is_cuda:
        raise RuntimeError("taxoexpan_amd.loss.in_batch_info_nce runs on the MI355X only (no CPU path; loss.host_in_batch_nce is the restatement)")
    return ops.InBatchNCEFunction.apply(hg, match.W.weight, queries, bool(match.apply_exp), groups, valid_total,
                                        bool(query_grad)).as_subclass(LossTensor)


def host_in_batch_valid(pos_col, anchor, qnode, mask_ptr=None, mask_idx=None):
    """valid [Q, G] bool of the in-batch rule: (g == pos_col[i]) or anchor[g] not in the mask row of qnode[i]"""
    pos_col, anchor, qnode = (np.asarray(a).astype(np.int64).reshape(-1) for a in (pos_col, anchor, qnode))
    if (mask_ptr is None) != (mask_idx is None):
        raise ValueError("mask_ptr and mask_idx come together")
    if pos_col.shape != qnode.shape:
        raise ValueError(f"one pos_col per query: {pos_col.shape} against {qnode.shape}")
    valid = np.ones((qnode.shape[0], anchor.shape[0]), dtype=bool)
    if mask_ptr is not None:
        mask_ptr, mask_idx = np.asarray(mask_ptr).astype(np.int64), np.asarray(mask_idx)
        for i, q in enumerate(qnode):
            valid[i] = ~np.isin(anchor, mask_idx[mask_ptr[q]:mask_ptr[q + 1]])
    valid[np.arange(qnode.shape[0]), pos_col] = True
    return valid


def host_in_batch_nce(S, pos_col, anchor, qnode, mask_ptr=None, mask_idx=None):
    """numpy float64 restatement of txe_inbatch_nce -- the written definition: (loss, dS [Q, G], n_valid [Q]).  A masked column's value
    is never used; dS is exactly 0 there."""
    S = np.asarray(S, dtype=np.float64)
    valid = host_in_batch_valid(pos_col, anchor, qnode, mask_ptr, mask_idx)
    if S.ndim != 2 or S.shape != valid.shape:
        raise ValueError(f"S must be [Q, G] = {valid.shape}, got {S.shape}")
    pos_col = np.asarray(pos_col).astype(np.int64).reshape(-1)
    rows = np.arange(S.shape[0])
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.where(valid, S, -np.inf)
        m = x.max(axis=1, keepdims=True) if S.shape[0] else np.zeros((0, 1))
        e = np.where(valid, np.exp(x - m), 0.0)
        s = e.sum(axis=1, keepdims=True)
        loss = float(np.sum(m[:, 0] + np.log(s[:, 0]) - S[rows, pos_col]))
        dS = e / s
        dS[rows, pos_col] -= 1.0
        dS = np.where(valid, dS, 0.0)
    return loss, dS, valid.sum(axis=1).astype(np.int64)


# ---- bce, square-exp and margin-rank ------------------------------------------------------------------------------------------------

_BCE, _SQUARE_EXP, _MARGIN_RANK = 0, 1, 2


class _LabelledLoss(torch.autograd.Function):
    """txe_bce_loss / txe_square_exp_loss / txe_margin_rank_loss: forward leaves the loss and d_x [B]; backward scales d_x"""

    @staticmethod
    def forward(ctx, output, target, kind, scalar):
        x = output.reshape(-1)                                        # [B] or [B, 1]: a view either way
        if not (x.dtype == torch.float32 and x.is_contiguous()):
            x = x.float().contiguous()
        lab = target if target.is_contiguous() else target.contiguous()
        B = x.shape[0]
        dev = x.device
        ctx.shape, ctx.dtype = output.shape, output.dtype
        with _lib.on_device(dev):
            d_x = torch.empty(B, dtype=torch.float32, device=dev)
            if B == 0:                                                # nothing to launch
                ctx.save_for_backward(d_x)
                return torch.zeros((), dtype=torch.float32, device=dev)
            loss = torch.empty((), dtype=torch.float32, device=dev)
            if kind == _BCE:
                _lib.call("txe_bce_loss", x.data_ptr(), lab.data_ptr(), lab.element_size(), B, loss.data_ptr(), d_x.data_ptr(),
                          _lib.stream_ptr())
            elif kind == _SQUARE_EXP:
                _lib.call("txe_square_exp_loss", x.data_ptr(), lab.data_ptr(), lab.element_size(), B, scalar, loss.data_ptr(),
                          d_x.data_ptr(), _lib.stream_ptr())
            else:
                wsb = _lib.pure("txe_margin_rank_loss_ws_bytes", B)   # a function of B alone
                ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
                _lib.call("txe_margin_rank_loss", x.data_ptr(), lab.data_ptr(), lab.element_size(), B, scalar, loss.data_ptr(),
                          d_x.data_ptr(), ws.data_ptr(), wsb, _lib.stream_ptr())
        ctx.save_for_backward(d_x)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        (d_x,) = ctx.saved_tensors
        d = _scaled(d_x, grad_loss).view(ctx.shape)
        return (d if ctx.dtype == torch.float32 else d.to(ctx.dtype)), None, None, None


def _labelled(name, output, target, kind, scalar):
    if not (torch.is_tensor(output) and torch.is_tensor(target)):
        raise TypeError(f"{name} takes tensors")
    if not output.is_cuda:
        raise RuntimeError(f"taxoexpan_amd.loss.{name} runs on the MI355X only (no CPU path; loss.host_{name} is the restatement)")
    if not (output.dim() == 1 or (output.dim() == 2 and output.shape[1] == 1)):
        raise ValueError(f"{name} takes scores [B] or [B, 1], got {tuple(output.shape)}")
    if target.dim() != 1 or target.shape[0] != output.shape[0]:
        raise ValueError(f"labels must be [B] with B = {output.shape[0]}, got {tuple(target.shape)}")
    if target.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"labels must be int32 or int64, got {target.dtype}")
    if target.device != output.device:
        raise ValueError("scores and labels must be on one device")
    if output.shape[0] >= 2 ** 31:
        raise ValueError(f"{name} takes B < 2^31")
    scalar = float(scalar)
    if not np.isfinite(scalar):
        raise ValueError(f"{name}: beta / margin must be finite, got {scalar}")
    return _LabelledLoss.apply(output, target, kind, scalar).as_subclass(LossTensor)


def bce_loss(output, target, beta=1.0):
    """model/loss.py:21-29.  output: [B] or [B, 1] scores (energies: smaller = more likely a true position, so the target is inverted,
    loss.py:26); target: [B] int32 / int64 in {0, 1}.  Returns sum over positives (label 1) of softplus(x) + sum over the others of
    softplus(-x) = F.binary_cross_entropy_with_logits(x, 1 - target, reduction="sum"), with d_x = sigmoid(x) - [no positive].  beta is
    accepted and unused, as in the reference.  B == 1 works (the reference's `squeeze()` makes a 0-dim tensor there and raises)."""
    return _labelled("bce_loss", output, target, _BCE, 0.0)


def square_exp_loss(output, target, beta=1.0):
    """model/loss.py:12-19: sum over label == 1 of x^2 + beta * sum over label == 0 of exp(-x); any other label contributes nothing (the
    reference masks with `== 0`).  exp overflows to Inf in fp32 as the torch expression does."""
    return _labelled("square_exp_loss", output, target, _SQUARE_EXP, beta)


def margin_rank_loss(output, target, margin=1.0):
    """model/loss.py:31-50 without its read-back.  Groups start at index 0 and at every i with target[i-1] == 0 and target[i] == 1
    (metric.obtain_ranks' rule); within a group every (positive p, negative n) pair -- label 1 against every other label -- contributes
    max(0, (x_p - x_n) + margin).  The gradient is integer-valued: +/- the number of active pairs of the entry, with the condition
    (x_p - x_n) + margin > 0 evaluated in fp32 exactly as written, so it is bit-equal to torch autograd's on the same pairs.
    DEVIATION from the reference: on label vectors whose every group is >= 1 ones followed by >= 1 zeros (what the samplers produce) the
    pairs are the reference's; on a vector that BEGINS WITH A ZERO ([0, 1, 0], [0, 0, 1, 0]) the reference's regex bookkeeping pairs
    nothing and returns 0, while this follows the group rule ([0, 1, 0]: the leading zero is a group of its own without a positive, and
    [1, 0] gives one pair)."""
    return _labelled("margin_rank_loss", output, target, _MARGIN_RANK, margin)


def _host_args(output, target):
    x = np.asarray(output)
    if not (x.ndim == 1 or (x.ndim == 2 and x.shape[1] == 1)):
        raise ValueError(f"scores must be [B] or [B, 1], got {x.shape}")
    x = x.reshape(-1).astype(np.float64)
    t = np.asarray(target)
    if t.ndim != 1 or t.shape[0] != x.shape[0]:
        raise ValueError(f"labels must be [B] with B = {x.shape[0]}, got {t.shape}")
    if t.dtype not in (np.int32, np.int64):
        raise ValueError(f"labels must be int32 or int64, got {t.dtype}")
    return x, t


def host_bce_loss(output, target, beta=1.0):
    """numpy float64 restatement of txe_bce_loss: (loss, d_x [B])"""
    x, t = _host_args(output, target)
    pos = t == 1
    with np.errstate(over="ignore", invalid="ignore"):
        z = np.where(pos, x, -x)
        loss = np.sum(np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z))) + np.where(np.isnan(z), np.nan, 0.0))
        e = np.exp(-np.abs(x))
        sig = np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        d = np.where(np.isnan(x), np.nan, sig - np.where(pos, 0.0, 1.0))
    return float(loss), d


def host_square_exp_loss(output, target, beta=1.0):
    """numpy float64 restatement of txe_square_exp_loss: (loss, d_x [B])"""
    x, t = _host_args(output, target)
    pos, neg = t == 1, t == 0
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-x[neg])
        loss = np.sum(x[pos] ** 2) + beta * np.sum(e)
        d = np.zeros_like(x)
        d[pos] = 2.0 * x[pos]
        d[neg] = -beta * e
    return float(loss), d


def group_starts(target):
    """the first index of every group of a label vector: 0 and every i with target[i-1] == 0 and target[i] == 1"""
    t = np.asarray(target)
    if t.shape[0] == 0:
        return np.zeros(0, dtype=np.int64)
    return np.flatnonzero(np.concatenate([[True], (t[:-1] == 0) & (t[1:] == 1)]))


def host_margin_pairs(target):
    """(positive indices, negative indices) of every pair of the group rule, group by group, positives outermost"""
    t = np.asarray(target)
    starts = group_starts(t)
    ends = np.append(starts[1:], t.shape[0])
    pi, ni = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for a, b in zip(starts, ends):
        idx = np.arange(a, b)
        p, n = idx[t[a:b] == 1], idx[t[a:b] != 1]
        pi.append(np.repeat(p, n.size))
        ni.append(np.tile(n, p.size))
    return np.concatenate(pi).astype(np.int64), np.concatenate(ni).astype(np.int64)


def host_margin_rank_loss(output, target, margin=1.0, dtype=np.float64):
    """numpy restatement of txe_margin_rank_loss: (loss, d_x [B]); dtype = the arithmetic of the hinge terms (float64: the definition;
    float32: the condition as the kernel evaluates it)"""
    x, t = _host_args(output, target)
    x = x.astype(dtype)
    pi, ni = host_margin_pairs(t)
    with np.errstate(invalid="ignore"):
        term = (x[pi] - x[ni]) + dtype(margin)
        active = term > 0
        loss = np.sum(np.where(~(term <= 0), term, dtype(0)).astype(np.float64))     # a NaN term stays (torch's clamp keeps it)
    d = np.zeros(x.shape[0], dtype=np.float64)
    np.add.at(d, pi[active], 1.0)
    np.add.at(d, ni[active], -1.0)
    return float(loss), d
