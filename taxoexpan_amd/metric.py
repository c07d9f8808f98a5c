"""model/metric.py of the reference on the flat rank layout the device ranking produces.

The reference passes `all_ranks` = a list (one entry per query) of lists of ranks; `ops.rank_block` / `scoring.rank_all_fused`
return one int32 tensor `ranks [n_positives]` plus the offsets `pos_off [Q+1]` of each query's positives.  Every function below
takes that pair and computes, on whatever device the ranks live, what the same-named reference function computes
(metric.py:62-96): macro_mr, micro_mr, hit_at_1/3/5, mrr_scaled_10, combined_metrics.  Results are Python floats.
`as_rank_lists` converts back to the reference's nested-list layout.

`obtain_ranks(outputs, targets, mode)` is metric.py:33-60 on a labelled batch (the Trainer's `pre_metric`): it returns a GroupedRanks
(ranks, pos_off), which every function below also takes as its single argument -- `metric(obtain_ranks(pred, label, mode=1))`.
Device tensors are ranked by csrc/txe_grouprank.hip, CPU tensors by a numpy restatement (_host_group_ranks).
"""
from typing import NamedTuple

import numpy as np
import torch

from . import _lib

METRIC_IDS = {"macro_mr": 0, "micro_mr": 1, "hit_at_1": 2, "hit_at_3": 3, "hit_at_5": 4, "mrr_scaled_10": 5, "combined_metrics": 6}


class GroupedRanks(NamedTuple):
    """obtain_ranks' result: ranks int32 [n_pos] (group by group, in entry order) and pos_off [n_groups + 1]"""
    ranks: torch.Tensor
    pos_off: torch.Tensor


def _unpack(ranks, pos_off):
    if isinstance(ranks, GroupedRanks) and pos_off is None:
        return ranks.ranks, ranks.pos_off
    return ranks, pos_off


def _check_batch(outputs, targets):
    s = outputs
    if s.dim() == 2 and s.shape[1] == 1:
        s = s[:, 0]
    if s.dim() != 1:
        raise ValueError(f"obtain_ranks takes scores [B] or [B, 1], got {tuple(outputs.shape)}")
    if s.dtype != torch.float32:
        raise ValueError(f"obtain_ranks ranks fp32 scores, got {s.dtype}")
    if targets.dim() != 1 or targets.shape[0] != s.shape[0]:
        raise ValueError(f"labels must be [B] with B = {s.shape[0]}, got {tuple(targets.shape)}")
    if targets.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"labels must be int32 or int64, got {targets.dtype}")
    if targets.device != s.device:
        raise ValueError("scores and labels must be on one device")
    if s.shape[0] >= 2 ** 31:
        raise ValueError("obtain_ranks takes B < 2^31")
    return s.contiguous(), targets.contiguous()


def _host_group_ranks(score, label, mode):
    """numpy restatement of txe_group_rank: groups start at 0 and at every 0 -> 1 transition; rank = 1 + the group's negatives
    strictly better in fp32 (a group without negatives: 1).  Returns (ranks int32 [n_pos], pos_off int32 [n_groups + 1])."""
    score = np.asarray(score, dtype=np.float32)
    label = np.asarray(label)
    B = len(label)
    if B == 0:                                           # the reference's single empty group
        return np.zeros(0, dtype=np.int32), np.zeros(2, dtype=np.int32)
    starts = np.flatnonzero(np.concatenate([[True], (label[:-1] == 0) & (label[1:] == 1)]))
    ends = np.append(starts[1:], B)
    ranks, pos_off = [], [0]
    for a, b in zip(starts, ends):
        s, pos = score[a:b], label[a:b] == 1
        neg = s[~pos]
        sp = s[pos][:, None]
        better = (neg[None, :] < sp) if mode == 0 else (neg[None, :] > sp)
        ranks.append(1 + better.sum(1))
        pos_off.append(pos_off[-1] + int(pos.sum()))
    return np.concatenate(ranks).astype(np.int32), np.asarray(pos_off, dtype=np.int32)


def _device_group_ranks(score, label, mode):
    """txe_group_rank on the current stream, nothing read back: (ranks [B], pos_off [B + 1], counts [2] = {n_groups, n_pos})"""
    B = int(score.shape[0])
    dev = score.device
    with _lib.on_device(dev):
        ranks = torch.empty(B, dtype=torch.int32, device=dev)
        pos_off = torch.empty(B + 1, dtype=torch.int32, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        wsb = _lib.pure("txe_group_rank_ws_bytes", B)
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
        _lib.call("txe_group_rank", _lib.ptr(score), _lib.ptr(label), label.element_size(), B, int(mode), _lib.ptr(ranks), _lib.ptr(pos_off),
                  _lib.ptr(counts), _lib.ptr(ws), wsb, _lib.stream_ptr())
    return ranks, pos_off, counts


def obtain_ranks(outputs, targets, mode=0):
    """model/metric.py:33-60: outputs = scores [B] or [B, 1] fp32, targets = labels [B] int32 / int64 ([1, .., 1, 0, .., 0] per query),
    mode 0: smaller is better, 1: larger is better.  Returns GroupedRanks(ranks int32 [n_pos], pos_off [n_groups + 1]) on the scores'
    device.  A group with no positive has an empty rank list (macro_mr is then NaN, as in the reference); a group with positives and no
    negatives -- outside the reference's domain, its numpy gives masked values -- ranks its positives 1."""
    if mode not in (0, 1):
        raise ValueError(f"mode must be 0 or 1, got {mode}")
    score, label = _check_batch(outputs.detach(), targets.detach())
    if score.device.type == "cpu":
        r, off = _host_group_ranks(score.numpy(), label.numpy(), mode)
        return GroupedRanks(torch.from_numpy(r), torch.from_numpy(off))
    if score.shape[0] == 0:
        return GroupedRanks(torch.zeros(0, dtype=torch.int32, device=score.device), torch.zeros(2, dtype=torch.int32, device=score.device))
    ranks, pos_off, counts = _device_group_ranks(score, label, mode)
    ng, npos = counts.cpu().tolist()
    return GroupedRanks(ranks[:npos], pos_off[:ng + 1])


def _f(ranks):
    return ranks.to(torch.float64)


def _counts(pos_off, device):
    off = torch.as_tensor(pos_off).to(device=device, dtype=torch.int64)
    return off, off[1:] - off[:-1]


def _exact_mean(v):
    """sum / n with one rounding, as numpy's mean of an integer array (a device mean multiplies by 1/n: one ulp off the reference)"""
    n = v.numel()
    return float(v.sum().item()) / n if n else float("nan")


def as_rank_lists(ranks, pos_off=None):
    """the reference's `all_ranks` (list of per-query rank lists), e.g. to call the reference's own metric functions"""
    ranks, pos_off = _unpack(ranks, pos_off)
    r = ranks.cpu().tolist()
    off = torch.as_tensor(pos_off).cpu().tolist()
    return [r[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def macro_mr(ranks, pos_off=None):
    """metric.py:62-64: mean over queries of the query's mean rank"""
    ranks, pos_off = _unpack(ranks, pos_off)
    off, cnt = _counts(pos_off, ranks.device)
    qid = torch.repeat_interleave(torch.arange(cnt.numel(), device=ranks.device), cnt)
    sums = torch.zeros(cnt.numel(), dtype=torch.float64, device=ranks.device).index_add_(0, qid, _f(ranks))
    return float((sums / cnt.to(torch.float64)).mean().item())


def micro_mr(ranks, pos_off=None):
    """metric.py:66-68: mean over all positives"""
    ranks, pos_off = _unpack(ranks, pos_off)
    return _exact_mean(_f(ranks))


def _hit(ranks, k):
    ranks, _ = _unpack(ranks, None)
    return _exact_mean((ranks <= k).to(torch.float64))


def hit_at_1(ranks, pos_off=None):
    return _hit(ranks, 1)


def hit_at_3(ranks, pos_off=None):
    return _hit(ranks, 3)


def hit_at_5(ranks, pos_off=None):
    return _hit(ranks, 5)


def mrr_scaled_10(ranks, pos_off=None):
    """metric.py:85-90: mean of 1 / ceil(rank / 10)"""
    ranks, pos_off = _unpack(ranks, pos_off)
    return float((1.0 / torch.ceil(_f(ranks) / 10.0)).mean().item())


def combined_metrics(ranks, pos_off=None):
    """metric.py:92-96 (early-stopping score)"""
    ranks, pos_off = _unpack(ranks, pos_off)
    return (macro_mr(ranks, pos_off) * (1.0 / max(mrr_scaled_10(ranks), 0.0001)) * (1.0 / max(hit_at_3(ranks), 0.0001)) *
            (1.0 / max(hit_at_1(ranks), 0.0001)))
