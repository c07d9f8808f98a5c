"""The training loop of the reference -- Trainer._train_epoch (trainer/trainer.py:41-94) and BaseTrainer.train / _save_checkpoint /
_resume_checkpoint (base/base_trainer.py:59-176) -- in the style of evaluate.validate: nothing per step returns to the host.

    StepLog       the device log of an epoch: per step the loss and the gradients' L2 norm, the running loss sum and the first step
                  whose loss or gradients were not finite, written by ONE launch per step (txe_step_log, csrc/txe_steplog.hip) between
                  `loss.backward()` and `optimizer.step()`; read back once per epoch.  guard() hands the optimizer launch of the step
                  the addresses of that norm and of that word (optim.Adam.step(guard=...)): clipping by the global norm and freezing
                  at the first non-finite step, with no launch, pass over the gradients or read-back added
    train_epoch   trainer.py:41-77 without `label.sum()` (:53), `loss.item()` (:64-65) or any other read-back inside the loop
    fit           base_trainer.py:59-107 + trainer.py:79-94: epochs of train_epoch + evaluate.validate, the LR schedule, monitoring,
                  early stopping, checkpoints with the reference's keys, resume -- and one addition: a diverged epoch ends the run;
                  averaged=True validates, monitors and checkpoints the averaged weights of optim.Adam(ema_decay=...)
    load_averaged a checkpoint's averaged weights ("ema_state_dict") into a model
    host_step_log the numpy restatement of txe_step_log (its written definition; the CPU tests use it)
"""
import inspect
import logging
import math
import os
import warnings

import numpy as np
import torch


def host_step_log(losses, grads_per_step, capacity=None):
    """What txe_step_log leaves after len(losses) steps: (loss_log fp32 [capacity], gnorm2_log fp64 [capacity], acc fp64 [2],
    first_bad int64 [1]).  grads_per_step[s] = the gradient arrays of step s (any shapes; none at all logs the loss alone).
    gnorm2 adds the fp64 squares of the fp32 elements one after the other, tensor after tensor in index order (the kernel adds the same
    numbers in its own fixed order: equal up to the reordering error of an fp64 sum, N * 2^-52 relative)."""
    n = len(losses)
    if len(grads_per_step) != n:
        raise ValueError("one list of gradients per step")
    capacity = n if capacity is None else int(capacity)
    if n > capacity:
        raise ValueError(f"{n} steps do not fit a log of capacity {capacity}")
    loss_log, gnorm2_log = np.zeros(capacity, dtype=np.float32), np.zeros(capacity, dtype=np.float64)
    acc, first_bad = np.zeros(2, dtype=np.float64), np.full(1, -1, dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(n):
            loss = np.float32(losses[s])
            flat = [np.asarray(g, dtype=np.float32).reshape(-1).astype(np.float64) for g in grads_per_step[s]]
            sq = np.concatenate(flat) ** 2 if flat else np.zeros(0)
            total = float(np.cumsum(sq)[-1]) if sq.size else 0.0          # cumsum: strictly sequential, unlike np.sum's pairwise blocks
            loss_log[s], gnorm2_log[s] = loss, total
            acc[0] += np.float64(loss)
            acc[1] += 1.0
            if first_bad[0] < 0 and not (np.isfinite(loss) and np.isfinite(sq).all()):
                first_bad[0] = s
    return loss_log, gnorm2_log, acc, first_bad


class StepLog:
    """The device log of up to `capacity` training steps (one epoch).  record() enqueues one txe_step_log on the current stream and
    returns nothing; read() is the one read-back.  All records of one log must be enqueued on one stream (the kernel's last workgroup
    updates the running sums with a plain read-modify-write)."""

    def __init__(self, device, capacity):
        from . import _lib
        self.device, self.capacity = torch.device(device), int(capacity)
        if self.capacity < 1:
            raise ValueError("StepLog needs a capacity of at least one step")
        if self.device.type != "cuda":
            raise RuntimeError("taxoexpan_amd.trainer.StepLog lives on the GPU (no CPU path; host_step_log is the restatement)")
        # one fp64 buffer, so that read() is ONE copy: [acc (2) | first_bad (1, as int64) | gnorm2 (capacity) | loss (capacity fp32) |
        # counter (1, as int64) | extra (2, as 4 int32)]
        c = self.capacity
        self._buf = torch.zeros(6 + c + (c + 1) // 2, dtype=torch.float64, device=self.device)
        self._acc, self._first_bad = self._buf[0:2], self._buf[2:3].view(torch.int64)
        self._gnorm2, self._loss = self._buf[3:3 + c], self._buf[3 + c:].view(torch.float32)[:c]
        # an int64 word the log itself never writes: a loss may add to it on the device (loss.in_batch_info_nce's valid_total); it comes
        # back with read() and is cleared by reset()
        self.counter = self._buf[-3:-2].view(torch.int64)
        # four int32 words of the same kind: train_epoch copies the sampler's near-negative counters of the epoch into them
        self.extra = self._buf[-2:].view(torch.int32)
        self._first_bad.fill_(-1)
        self._ws, self._ws_bytes = None, 0
        self._table = None
        self.n_recorded = 0
        self._lib = _lib

    def _workspace(self, n_chunks):
        need = self._lib.pure("txe_step_log_ws_bytes", n_chunks)
        if need > self._ws_bytes:                                   # zeroed: the ticket word starts at 0 and every launch leaves it there
            self._ws = torch.zeros((need + 7) // 8, dtype=torch.float64, device=self.device)
            self._ws_bytes = self._ws.numel() * 8
        return self._ws

    def record(self, loss, params):
        """log the step whose scalar `loss` (fp32, on the device) was just back-propagated into the `.grad` of `params` (parameters
        whose .grad is None are skipped); raises before any launch when the log is full"""
        import ctypes as C
        _lib = self._lib
        s = self.n_recorded
        if s >= self.capacity:
            raise IndexError(f"StepLog is full: step {s} of a log of capacity {self.capacity} (reset() starts the next epoch)")
        if not (torch.is_tensor(loss) and loss.numel() == 1 and loss.dtype == torch.float32 and loss.device == self.device):
            raise ValueError("StepLog.record needs the loss as one fp32 element on the log's device")
        grads = []
        for p in params:
            g = p.grad
            if g is None:
                continue
            if g.is_sparse or g.dtype != torch.float32 or g.device != self.device:
                raise RuntimeError("taxoexpan_amd.trainer.StepLog: dense fp32 gradients on the log's device only")
            grads.append(g if g.is_contiguous() else g.contiguous())
        addr = [g.data_ptr() for g in grads]
        numel = [g.numel() for g in grads]
        tab = self._table
        if tab is None or tab["addr"] != addr or tab["numel"] != numel:      # (set_to_none gradients are new tensors, usually at the old addresses)
            chunk = _lib.STEP_LOG_CHUNK
            tab = self._table = dict(addr=addr, numel=numel, g=(C.c_void_p * len(addr))(*addr), n=(C.c_longlong * len(numel))(*numel),
                                     n_chunks=sum(-(-n // chunk) for n in numel))
        ws = self._workspace(tab["n_chunks"])
        loss = loss.detach()
        with _lib.on_device(self.device):
            _lib.call("txe_step_log", loss.data_ptr(), len(addr), tab["g"], tab["n"], s, self.capacity, self._loss.data_ptr(),
                      self._gnorm2.data_ptr(), self._acc.data_ptr(), self._first_bad.data_ptr(), ws.data_ptr(), self._ws_bytes,
                      _lib.stream_ptr())
        self.n_recorded = s + 1

    def guard(self, step=None, gnorm2=True, first_bad=True):
        """the optim.StepGuard of a recorded step (default: the one recorded last) for the optimizer launch that follows record() on the
        same stream: gnorm2 = the address of that step's slot in the log's fp64 buffer, first_bad = the address of the log's word
        (either left out on request).  No device memory, no launch: two addresses and a reference to the buffer."""
        from .optim import StepGuard
        s = self.n_recorded - 1 if step is None else int(step)
        if not 0 <= s < self.n_recorded:
            raise IndexError(f"StepLog.guard: step {s} has not been recorded ({self.n_recorded} steps so far)")
        return StepGuard(gnorm2=self._gnorm2.data_ptr() + 8 * s if gnorm2 else None,
                         first_bad=self._first_bad.data_ptr() if first_bad else None, keep=(self._buf,))

    def read(self):
        """the epoch's one read-back: dict(loss fp32 [n], grad_norm fp64 [n], loss_sum, n_steps, first_nonfinite (-1: none), counter,
        extra int32 [4])"""
        host = self._buf.cpu().numpy()
        c, n = self.capacity, self.n_recorded
        return dict(loss=host[3 + c:].view(np.float32)[:n].copy(), grad_norm=np.sqrt(host[3:3 + n]), loss_sum=float(host[0]),
                    n_steps=int(host[1]), first_nonfinite=int(host[2:3].view(np.int64)[0]), counter=int(host[-3:-2].view(np.int64)[0]),
                    extra=host[-2:].view(np.int32).copy())

    def reset(self):
        """clear the log for the next epoch"""
        self._buf.zero_()
        self._first_bad.fill_(-1)
        self.n_recorded = 0


def _is_info_nce(loss_fn):
    return getattr(loss_fn, "__name__", "").startswith("info_nce")        # trainer.py:20 tests the config's loss NAME the same way


def train_epoch(model, loader, optimizer, loss_fn=None, group_size=None, log=None, max_grad_norm=None, freeze_on_nonfinite=False,
                in_batch=False, feature_table=None, taxo_margin=None, taxonomy_index=None):
    """trainer.py:41-77 on the device: model.train(), then per batch zero_grad, forward, loss, backward, ONE txe_step_log launch,
    optimizer.step() -- no .item(), .cpu() or synchronize between the first batch and the last (what `loader` does to build a batch is
    its own business), then one read-back of the log.
    loader: DeviceBatchLoader's (g, h, qf, label) or MaskedGraphDataLoader's (g, qf, label) batches, as evaluate.validate takes them.
    loss_fn (default loss.info_nce_loss): a function whose __name__ starts with "info_nce" gets the scores regrouped to
    [-1, group_size] and the target None (= all zeros, trainer.py:53-55); group_size defaults to 1 + loader.dataset.negative_size --
    sampling_mode 1 draws exactly that many anchors per query, so the shape is known without trainer.py:53's `label.sum()` -- and a batch
    that is no multiple of it raises ValueError.  Any other loss_fn gets (prediction, label) as trainer.py:57-58 passes them:
    loss.bce_loss, loss.square_exp_loss and loss.margin_rank_loss read the device labels as they are and keep the no-read-back promise;
    the reference's own margin_rank_loss (model/loss.py:31-50) does not -- it starts with `target.cpu()` and builds its pairs on the host.
    log: a StepLog to reuse (it is reset first; one too small for len(loader) steps raises ValueError before the first step); default:
    one of len(loader) steps.
    Returns dict(loss = the fp64 sum of the fp32 step losses / n_batches -- trainer.py:76's total_loss / len(data_loader) --, n_batches,
    losses fp32 [n_batches], grad_norms fp64 [n_batches], first_nonfinite = the first step with a non-finite loss or gradient, or -1).
    It never stops early: that would take a read-back per step.
    max_grad_norm / freeze_on_nonfinite (off by default: then the loop is launch for launch what it was): the optimizer launch of every
    step reads what the log launch before it wrote -- `optimizer.step(guard=log.guard())`, which optim.Adam takes and an optimizer whose
    step() has no `guard` does not (ValueError before the first step).
      max_grad_norm c: the gradients enter the update scaled by min(1, c / (norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s rule, with
        the norm the log has just formed (a group's own Adam(max_grad_norm=...) counts when c is None).  `.grad` is not rewritten and the
        returned grad_norms stay the norms BEFORE clipping -- what clip_grad_norm_ returns.
      freeze_on_nonfinite: from the first step s whose loss or gradients are not finite on, the optimizer launches return without a load
        or a store; after the read-back optimizer.discount_frozen_steps(n_batches - s) takes the skipped steps off the step counts.
        Model and optimizer are then exactly as after step s - 1 (the forward and backward passes of the later steps still ran).
    An optimizer that averages its parameters (optim.Adam(ema_decay=...)) does so inside the same optimizer launch; nothing here changes.
    A frozen run freezes the averages too: the launch that skips the update skips the average, and the discounted step counts let a
    warm-up schedule of the decay resume where the device stopped.
    in_batch (an addition; off: the loop is launch for launch what it was, the dict has no new key): every query is scored against EVERY
    egonet of its batch, not only its own 1 + negative_size -- per batch `hg = encode_graph(model, g, h, pos)`, then
    `loss.in_batch_info_nce(model.match, hg, qf.rows, g.in_batch)`, then backward, log and step as above.  The loader
    must attach `g.in_batch` (DeviceBatchLoader(sampler="device", in_batch=True)) and the matcher must be BIM / LBM; loss_fn cannot be
    given with it -- each a ValueError before the first optimizer step.  The dict gains mean_negatives = the valid negative columns per
    query, averaged over the epoch: the log's int64 counter word (StepLog.counter), which the loss launches add to and which comes
    back in the log's one read-back.
    feature_table (an addition; None: the loop is launch for launch what it was): a feature_table.FeatureTable that the loader gathers from
    (DeviceBatchLoader(feature_table=...)).  After zero_grad, feature_table.leaves(g, qf, h) makes the batch's node features and distinct
    query rows leaves; the log reads their gradients beside the parameters' -- the non-finite check covers them, and grad_norms then
    INCLUDE the per-occurrence feature gradients -- and feature_table.step(guard=...) runs right after optimizer.step(...).  Works with
    every loss_fn and with in_batch=True.  max_grad_norm (the argument's or a parameter group's) together with a table is a ValueError
    before the first step: the logged norm is over occurrences, not the table gradient's norm, and clipping the table is out of scope.
    freeze_on_nonfinite freezes the table with the model and discounts its steps as the optimizer's.  Averaged weights do not cover
    the table.
    taxo_margin (an addition; None: the loop is launch for launch what it was, the dict has no new key): gamma, a finite number >= 0 -- 0.0
    is a value and runs the new launch.  The loss call becomes `loss.taxo_info_nce(prediction.reshape(-1, group_size), g.anchors,
    index, gamma, dist_total=log.counter)`: InfoNCE whose negatives carry the margin gamma * (1 - Wu & Palmer similarity
    to the group's positive); forward, backward, log, guarded step, averaged weights, feature table and hard negatives stay as they
    are, and the folded route keeps running (no score matrix, no materialised hg).  taxonomy_index: TaxonomyIndex.to(device) of the
    loader's dataset; None builds TaxonomyIndex.from_dataset(loader.dataset).to(device) here (fit builds it once for all epochs).
    ValueError before the first optimizer step: together with in_batch=True (margins inside the in-batch loss are out of scope) or with
    a loss_fn, a loader that does not attach g.anchors (DeviceBatchLoader(sampler="device", attach_anchors=True)), a gamma that is not
    finite or negative, an index whose n_nodes differs from the dataset's.  The dict gains mean_taxo_distance = the mean of 1 - Wu &
    Palmer over the epoch's negatives, in steps of 2^-20: the log's int64 counter word / 2^20 / (groups * negatives per group).
    Near negatives (an addition; a loader without near slots: the loop is launch for launch what it was, the dict has no new key): when
    loader.sampler has near slots (DeviceBatchLoader(near_negatives=...) / set_near_negatives), the dict gains near_sibling_share,
    near_grandparent_share and near_uncle_share = the class's accepted proposals / its requested slots over the epoch (0.0 for a class
    without slots).  The sampler's three device counters are copied before the first batch and their growth is written into the log's
    `extra` words behind the last step, so they come back in the log's one read-back."""
    taxo = taxo_margin is not None
    if taxo:
        from .loss import _checked_gamma
        if in_batch:
            raise ValueError("train_epoch: taxo_margin cannot be combined with in_batch=True (margins inside the in-batch loss are out of scope)")
        if loss_fn is not None:
            raise ValueError("train_epoch: taxo_margin brings its own loss (loss.taxo_info_nce); loss_fn cannot be given with it")
        if getattr(loader, "attach_anchors", True) is False:
            raise ValueError("train_epoch: taxo_margin needs a loader that attaches g.anchors (DeviceBatchLoader(sampler='device', "
                             "attach_anchors=True))")
        taxo_margin = _checked_gamma(taxo_margin, "train_epoch: taxo_margin")
        n_data = getattr(getattr(getattr(loader, "dataset", None), "node_features", None), "shape", (None,))[0]
        if taxonomy_index is not None and n_data is not None and int(taxonomy_index.n_nodes) != int(n_data):
            raise ValueError(f"train_epoch: taxonomy_index has {taxonomy_index.n_nodes} nodes, the loader's dataset {n_data}")
    elif taxonomy_index is not None:
        raise ValueError("train_epoch: taxonomy_index is the index of taxo_margin; it cannot be given without it")
    if in_batch:
        if loss_fn is not None:
            raise ValueError("train_epoch: in_batch=True brings its own loss (loss.in_batch_info_nce); loss_fn cannot be given with it")
        from .loss import is_bilinear_matcher
        match = getattr(model, "match", None)
        if not is_bilinear_matcher(match):
            raise ValueError(f"train_epoch: in_batch=True needs a BIM / LBM matcher, the model has {type(match).__name__}")
        if getattr(loader, "in_batch", True) is False:
            raise ValueError("train_epoch: in_batch=True needs a loader that attaches g.in_batch (DeviceBatchLoader(in_batch=True))")
    if loss_fn is None:
        from .loss import info_nce_loss as loss_fn
    info_nce = _is_info_nce(loss_fn) and not in_batch
    if info_nce and group_size is None:
        k = getattr(getattr(loader, "dataset", None), "negative_size", None)
        if k is None:
            raise ValueError("train_epoch: group_size is needed (the loader has no dataset.negative_size to take it from)")
        group_size = 1 + int(k)
    if info_nce and int(group_size) < 1:
        raise ValueError(f"group_size must be positive, got {group_size}")
    from .optim import _checked_max_norm
    max_grad_norm = _checked_max_norm(max_grad_norm)
    clip = max_grad_norm is not None or any(g.get("max_grad_norm") is not None for g in optimizer.param_groups)
    guarded = clip or bool(freeze_on_nonfinite)
    if clip and feature_table is not None:
        raise ValueError("train_epoch: max_grad_norm cannot be combined with a feature_table (the step log's norm is over per-occurrence "
                         "gradients and is not the table gradient's norm; clipping the table is out of scope)")
    if guarded and "guard" not in inspect.signature(optimizer.step).parameters:
        raise ValueError(f"max_grad_norm / freeze_on_nonfinite need an optimizer whose step() takes `guard` (taxoexpan_amd.optim.Adam); "
                         f"{type(optimizer).__name__}.step does not")
    params = list(model.parameters())
    dev = params[0].device
    if log is None:
        log = StepLog(dev, max(1, len(loader)))
    else:
        if hasattr(loader, "__len__") and log.capacity < len(loader):
            raise ValueError(f"the StepLog holds {log.capacity} steps, the loader yields {len(loader)}")     # before any optimizer step
        log.reset()
    if in_batch:
        from .loss import in_batch_info_nce
        from .model import encode_graph
        valid_total, n_queries = log.counter, 0                        # (cleared with the log, read back with it)
    if taxo:
        from .loss import DIST_SCALE, taxo_info_nce
        from .taxometric import DeviceTaxonomyIndex, TaxonomyIndex
        if taxonomy_index is None:
            if getattr(loader, "dataset", None) is None:
                raise ValueError("train_epoch: taxo_margin needs taxonomy_index (the loader has no dataset to build it from)")
            taxonomy_index = TaxonomyIndex.from_dataset(loader.dataset)
        if not isinstance(taxonomy_index, DeviceTaxonomyIndex):
            taxonomy_index = taxonomy_index.to(dev)
        n_negatives = 0
    near_sampler = getattr(loader, "sampler", None)
    near = tuple(getattr(near_sampler, "near", None) or (0, 0, 0))
    if any(near) and hasattr(near_sampler, "_near"):                   # the counters as the epoch finds them (cumulative on the sampler)
        near_before, near_queries = near_sampler._near.clone(), 0
    else:
        near = (0, 0, 0)
    model.train()                                                      # trainer.py:42
    n_batches = 0
    for batch in loader:
        if len(batch) == 4:
            g, h, qf, label = batch
        else:
            g, qf, label = batch
            h = g.ndata.pop("x")                                       # trainer.py:48
        h = h.to(dev, non_blocking=True)
        qf = qf.to(dev, non_blocking=True) if torch.is_tensor(qf) else qf
        label = label.to(dev, non_blocking=True)
        if in_batch and getattr(g, "in_batch", None) is None:
            raise ValueError("train_epoch: in_batch=True, but a batch has no g.in_batch (DeviceBatchLoader(sampler='device', in_batch=True))")
        optimizer.zero_grad()                                          # trainer.py:50
        logged = params
        if feature_table is not None:
            h, qf, _ids, _qids = feature_table.leaves(g, qf, h)
            logged = params + [h, qf.rows]
        if in_batch:
            hg = encode_graph(model, g, h, g.ndata["pos"].to(dev))
            if feature_table is not None:
                loss = in_batch_info_nce(model.match, hg, qf.rows, g.in_batch, valid_total=valid_total, query_grad=True)
            else:
                loss = in_batch_info_nce(model.match, hg, getattr(qf, "rows", qf), g.in_batch, valid_total=valid_total)
            n_queries += g.in_batch.Q
        else:
            prediction = model(g, h, qf)
            if info_nce:
                if prediction.numel() % group_size:
                    raise ValueError(f"a batch of {prediction.numel()} scores is no multiple of group_size {group_size}")
                if taxo:
                    anchors = getattr(g, "anchors", None)
                    if anchors is None:
                        raise ValueError("train_epoch: taxo_margin, but a batch has no g.anchors (DeviceBatchLoader(sampler='device', "
                                         "attach_anchors=True))")
                    loss = taxo_info_nce(prediction.reshape(-1, group_size), anchors, taxonomy_index, taxo_margin, dist_total=log.counter)
                    n_negatives += (prediction.numel() // group_size) * (group_size - 1)
                else:
                    loss = loss_fn(prediction.reshape(-1, group_size), None)
            else:
                loss = loss_fn(prediction, label)
        loss.backward()                                                # trainer.py:60
        log.record(loss, logged)
        if guarded:                                                    # only what was asked for is passed
            guard = log.guard(gnorm2=clip, first_bad=bool(freeze_on_nonfinite))
            guard.max_grad_norm = max_grad_norm
            optimizer.step(guard=guard)
        else:
            guard = None
            optimizer.step()                                           # trainer.py:61
        if feature_table is not None:
            feature_table.step(guard=guard)
        n_batches += 1
        if any(near):
            near_queries += label.numel() // (1 + near_sampler.k)
    if any(near):                                                      # (this stream waited for every sampler launch of the epoch)
        log.extra[:3].copy_(near_sampler._near - near_before)
    rec = log.read()
    if freeze_on_nonfinite and rec["first_nonfinite"] >= 0:
        optimizer.discount_frozen_steps(n_batches - rec["first_nonfinite"])
        if feature_table is not None:
            feature_table.discount_frozen_steps(n_batches - rec["first_nonfinite"])
    out = dict(loss=rec["loss_sum"] / n_batches if n_batches else float("nan"), n_batches=n_batches, losses=rec["loss"],
               grad_norms=rec["grad_norm"], first_nonfinite=rec["first_nonfinite"])
    if in_batch:                                                       # (valid pairs - the positives) per query
        out["mean_negatives"] = (rec["counter"] - n_queries) / n_queries if n_queries else float("nan")
    if taxo:
        out["mean_taxo_distance"] = rec["counter"] / DIST_SCALE / n_negatives if n_negatives else float("nan")
    for name, slots, got in zip(("near_sibling_share", "near_grandparent_share", "near_uncle_share"), near, rec["extra"]):
        if any(near):                                                  # (a class without slots: 0 of 0 requested, reported as 0.0)
            out[name] = int(got) / (slots * near_queries) if slots * near_queries else 0.0
    return out


class TrainingDiverged(RuntimeError):
    """fit() met an epoch whose loss or gradients were not finite: .epoch (1-based), .step (0-based within the epoch), .logs (the
    per-epoch logs up to and including that epoch) and .checkpoint (the path of the last_finite.pth that fit wrote, or None)"""

    def __init__(self, epoch, step, logs=(), checkpoint=None):
        super().__init__(f"training diverged: non-finite loss or gradient at step {step} of epoch {epoch}")
        self.epoch, self.step, self.logs, self.checkpoint = epoch, step, list(logs), checkpoint


def _checkpoint_state(model, optimizer, epoch, monitor_best, config, averaged=False, feature_table=None):
    """averaged: one more key, "ema_state_dict" = the model's state_dict() with the averages swapped in, as copies (the swap goes back
    before anything else is read: "state_dict" and "optimizer" are the raw weights and the full state, as ever); feature_table: one more
    key, "feature_table" = its state_dict()"""
    state = {}
    if averaged:
        with optimizer.averaged_parameters():
            state["ema_state_dict"] = {k: v.detach().clone() for k, v in model.state_dict().items()}
    state.update({"arch": type(model).__name__, "epoch": epoch, "state_dict": model.state_dict(), "optimizer": optimizer.state_dict(),
                  "monitor_best": monitor_best, "config": config})
    if feature_table is not None:
        state["feature_table"] = feature_table.state_dict()
    return state


def load_averaged(model, path):
    """load the averaged weights that fit(averaged=True) wrote into the checkpoint `path` (its "ema_state_dict") into `model`, strictly;
    a checkpoint without them (written with averaged=False, or by the reference) raises ValueError.  Returns the checkpoint."""
    ckpt = torch.load(str(path), map_location="cpu", weights_only=False)
    if "ema_state_dict" not in ckpt:
        raise ValueError(f"{path} has no 'ema_state_dict': the checkpoint was written without averaged weights (fit(averaged=True))")
    model.load_state_dict(ckpt["ema_state_dict"], strict=True)
    return ckpt


def _save_checkpoint(save_dir, model, optimizer, epoch, monitor_best, config, save_best, averaged=False, feature_table=None):
    """base_trainer.py:126-149"""
    state = _checkpoint_state(model, optimizer, epoch, monitor_best, config, averaged, feature_table)
    os.makedirs(str(save_dir), exist_ok=True)
    torch.save(state, os.path.join(str(save_dir), f"checkpoint-epoch{epoch}.pth"))
    if save_best:
        torch.save(state, os.path.join(str(save_dir), "model_best.pth"))


def _checked_hard_negatives(cfg, train_loader):
    """fit's hard_negatives option as dict(size, slots, every, start), or None; ValueError for anything fit cannot run"""
    if cfg is None:
        return None
    from .sampler import DeviceAnchorSampler, _hard_size
    if not isinstance(cfg, dict) or not {"size", "slots"} <= set(cfg) or not set(cfg) <= {"size", "slots", "every", "start"}:
        raise ValueError(f"hard_negatives is None or dict(size=, slots=, every=1, start=1), got {cfg!r}")
    if not (isinstance(getattr(train_loader, "sampler", None), DeviceAnchorSampler) and hasattr(train_loader, "set_hard_negatives")):
        raise ValueError("hard_negatives needs a DeviceBatchLoader(sampler='device') over a sampling_mode 1 dataset (the host sampler and "
                         "the sampling_mode 0 group sampler draw from the pool only)")
    out = dict(every=1, start=1)
    out.update(cfg)
    for name, v in out.items():
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"hard_negatives[{name!r}] must be an integer, got {v!r}")
        out[name] = int(v)
    k = train_loader.sampler.k
    if not 0 <= out["slots"] <= k:
        raise ValueError(f"hard_negatives: slots must be in [0, negative_size = {k}], got {out['slots']}")
    out["size"] = _hard_size(out["size"], train_loader.sampler.n_pool)
    if out["size"] < out["slots"]:
        raise ValueError(f"hard_negatives: size {out['size']} is below slots {out['slots']}")
    if out["every"] < 1 or out["start"] < 1:
        raise ValueError(f"hard_negatives: every and start are at least 1, got {out['every']} and {out['start']}")
    return out


def _checked_near_negatives(cfg, train_loader, hard):
    """fit's near_negatives option as dict(siblings, grandparents, uncles, start), or None; ValueError for anything fit cannot run"""
    if cfg is None:
        return None
    from .sampler import DeviceAnchorSampler, _checked_near
    names = ("siblings", "grandparents", "uncles")
    if not isinstance(cfg, dict) or not set(cfg) <= set(names) | {"start"}:
        raise ValueError(f"near_negatives is None or dict(siblings=0, grandparents=0, uncles=0, start=0), got {cfg!r}")
    if not (isinstance(getattr(train_loader, "sampler", None), DeviceAnchorSampler) and hasattr(train_loader, "set_near_negatives")):
        raise ValueError("near_negatives needs a DeviceBatchLoader(sampler='device') over a sampling_mode 1 dataset (the host sampler and "
                         "the sampling_mode 0 group sampler draw from the pool only)")
    start = cfg.get("start", 0)
    if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or start < 0:
        raise ValueError(f"near_negatives['start'] must be an integer >= 0, got {start!r}")
    h0 = max(train_loader.sampler.hard_slots, hard["slots"] if hard is not None else 0)
    counts = _checked_near(tuple(cfg.get(n, 0) for n in names), train_loader.sampler.k, h0, "near_negatives")
    return dict(zip(names, counts), start=int(start))


def fit(model, train_loader, valid_loader, optimizer, epochs, metrics=None, monitor="min val_macro_mr", early_stop=math.inf,
        lr_scheduler=None, scheduler_metric=None, save_dir=None, save_period=1, resume=None, config=None, larger_is_better=True,
        loss_fn=None, group_size=None, train_epoch_fn=None, validate_fn=None, max_grad_norm=None, freeze_on_nonfinite=False,
        hard_negatives=None, averaged=False, in_batch=False, feature_table=None, taxo_margin=None, taxonomy_index=None,
        near_negatives=None):
    """BaseTrainer.train (base_trainer.py:59-107) around trainer.py:79-94.  Per epoch (1-based): train_epoch, then evaluate.validate on
    `valid_loader` (None: no validation) with its values merged into the epoch's log as val_<metric name>; then
      - lr_scheduler: a ReduceLROnPlateau is stepped with the log's `scheduler_metric` (default: the monitored metric; the reference
        picks val_metrics[0] or [2] by position, trainer.py:87-90), any other scheduler with a plain .step()
      - monitor "min <key>" / "max <key>" / "off": improved = `<=` / `>=` the best so far (a tie counts); an epoch that did not improve
        raises a count, and the run stops, without a checkpoint for that epoch, once the count exceeds early_stop; a key the log does
        not have warns once and turns monitoring off
      - every save_period epochs checkpoint-epoch{N}.pth under save_dir (None: nothing is written), and model_best.pth beside it when
        the epoch was the best so far; keys arch, epoch, state_dict, optimizer, monitor_best, config as base_trainer.py:134-142
    resume: such a checkpoint (this function's or the reference's): model, optimizer state, monitor_best and the start epoch are restored.
    Two deviations from the reference, both on purpose: (1) when the monitored key is missing, base_trainer.py:87-101 sets the count to 0
    and then still falls into its `else` branch, which raises it to 1 -- with early_stop = 0 the reference stops right there; here
    monitoring is switched off without counting, so the run goes on.  (2) _resume_checkpoint warns when the checkpoint's `arch` config
    differs and SKIPS the optimizer state when its optimizer `type` differs (base_trainer.py:164-174); fit has no config schema to compare,
    so both checks are dropped: the optimizer state is always loaded, and a mismatch surfaces as load_state_dict's own error.
    The one addition: an epoch whose step log shows a non-finite loss or gradient ends the run -- no validation, no scheduler step and no
    checkpoint for it -- with TrainingDiverged(epoch, step).  train_epoch itself runs the epoch to its end (see there).
    max_grad_norm / freeze_on_nonfinite go to train_epoch (see there; they are passed only when set).  With freeze_on_nonfinite the
    diverged epoch left model and optimizer as they were after its last finite step, and with a save_dir that state is written to
    last_finite.pth before TrainingDiverged is raised (.checkpoint names it): the keys of every other checkpoint, `epoch` = the epoch
    completed before the diverged one, so that `resume=` starts the diverged epoch again.
    loss_fn / group_size go to train_epoch (the device losses of taxoexpan_amd.loss -- info_nce, bce, square_exp, margin_rank -- keep an
    epoch free of read-backs; see there).  train_epoch_fn / validate_fn replace trainer.train_epoch / evaluate.validate (same call
    signatures); the loop control here makes no GPU call of its own.  Returns the list of per-epoch logs.
    hard_negatives: None (uniform negatives, as ever) or dict(size=H, slots=m, every=1, start=1): before every epoch e >= start with
    (e - start) % every == 0, sampler.mine_hard_negatives(model, train_loader.dataset, size=H, larger_is_better=larger_is_better) ranks
    the pool for every training query under the model as it stands, and train_loader.set_hard_negatives(table, m) makes the first m
    negative slots of every query draw from its H best (DeviceBatchLoader(sampler="device"), sampling_mode 1); before `start` the
    loader draws uniformly, between mining epochs it keeps the last table.  Checked before the first step (ValueError): the loader kind,
    0 <= slots <= negative_size, 1 <= size, size >= slots, every >= 1, start >= 1, no other key.  The table is not checkpointed: a
    resumed run mines at its first qualifying epoch.  The log of an epoch that mined gains hard_mined = True and hard_mean_count = the
    mean of the table's cnt; no other key changes.
    averaged (an addition; off: no new key, no new launch, the logs as they are): the optimizer must be an optim.Adam with an ema_decay
    in at least one group (ValueError before the first step otherwise).  validate_fn then runs inside
    optimizer.averaged_parameters(), so the val_* metrics -- and with them the monitor, the plateau scheduler and early stopping --
    follow the AVERAGED model, and every checkpoint (checkpoint-epochN.pth, model_best.pth, last_finite.pth) gains "ema_state_dict", the
    model's state_dict() taken inside that context, as copies (load_averaged reads it).  "state_dict" and "optimizer" stay the raw
    weights and the full optimizer state, the average included, so `resume=` continues exactly.  Hard-negative mining keeps ranking
    with the raw model, the one being trained: its negatives are meant to be hard for the weights that the next step updates.
    in_batch=True goes to train_epoch (see there; passed only when set): the epochs train on in-batch negatives and their logs gain
    mean_negatives; validation is unchanged, and hard negatives compose (they only change which anchors a batch holds).
    feature_table (an addition; None: nothing changes): a feature_table.FeatureTable, passed to train_epoch (see there; only when set).
    Before each validation feature_table.write_back() puts the table into the training dataset's node_features / kv, and
    feature_table.refresh(valid_loader) does the same for the validation loader's dataset and resident table, so that validation -- and
    anything that reads host features afterwards -- scores with the trained vectors.  Every checkpoint (checkpoint-epochN.pth,
    model_best.pth, last_finite.pth) gains "feature_table" = its state_dict(), and `resume=` restores it (a checkpoint without the key
    is a ValueError).  Averaged weights do not cover the table: with averaged=True the val_* metrics use the averaged model over the
    raw table.
    taxo_margin / taxonomy_index (an addition; None: nothing changes) go to train_epoch (see there; passed only when taxo_margin is set):
    the epochs train with loss.taxo_info_nce and their logs gain mean_taxo_distance.  The index is built ONCE here, before the first
    epoch (TaxonomyIndex.from_dataset(train_loader.dataset).to(the model's device)), when none is given.  Validation and checkpoints
    are unchanged: a run without the keyword loads them.
    near_negatives: None (nothing changes) or dict(siblings=0, grandparents=0, uncles=0, start=0): before the first epoch e >= start,
    train_loader.set_near_negatives(siblings, grandparents, uncles) makes that many negative slots of every query (behind the hard slots)
    propose a node of the positive's taxonomy neighbourhood; until then the loader draws what it drew.  Needs no model pass
    and no table, so start = 0 (the first epoch) is allowed.  Checked before the first step (ValueError): the loader kind, integer
    counts >= 0, start >= 0, no other key, hard slots (the loader's, or hard_negatives' slots) + the three counts <= negative_size.  The
    logs of the epochs with near slots gain near_sibling_share, near_grandparent_share and near_uncle_share (train_epoch), and the
    shares are logged at INFO level; no other key changes."""
    if averaged and not (hasattr(optimizer, "averaged_parameters") and any(g.get("ema_decay") is not None for g in optimizer.param_groups)):
        raise ValueError("fit(averaged=True) needs an optimizer with averaged_parameters() and an ema_decay in at least one parameter "
                         f"group (taxoexpan_amd.optim.Adam(ema_decay=...)); got {type(optimizer).__name__}")
    averaged = bool(averaged)
    hard = _checked_hard_negatives(hard_negatives, train_loader)
    near = _checked_near_negatives(near_negatives, train_loader, hard)
    if train_epoch_fn is None:
        train_epoch_fn = train_epoch
    if validate_fn is None:
        from .evaluate import validate as validate_fn
    if metrics is None:
        from .evaluate import VALIDATION_METRICS as metrics
    metrics = list(metrics)
    if monitor == "off":                                               # base_trainer.py:31-39
        mnt_mode, mnt_metric, mnt_best = "off", None, 0
    else:
        mnt_mode, mnt_metric = monitor.split()
        if mnt_mode not in ("min", "max"):
            raise ValueError(f"monitor must be 'off', 'min <key>' or 'max <key>', got {monitor!r}")
        mnt_best = math.inf if mnt_mode == "min" else -math.inf
    plateau = isinstance(lr_scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau)
    if plateau and scheduler_metric is None:
        if mnt_metric is None:
            raise ValueError("a ReduceLROnPlateau needs scheduler_metric when monitor is 'off'")
        scheduler_metric = mnt_metric
    start_epoch = 1
    if resume is not None:                                             # base_trainer.py:151-176
        ckpt = torch.load(str(resume), map_location="cpu", weights_only=False)
        start_epoch = ckpt["epoch"] + 1
        mnt_best = ckpt["monitor_best"]
        model.load_state_dict(ckpt["state_dict"])
        optimizer.load_state_dict(ckpt["optimizer"])
        if feature_table is not None:
            if "feature_table" not in ckpt:
                raise ValueError(f"{resume} has no 'feature_table': the checkpoint was written by a run that did not train the table")
            feature_table.load_state_dict(ckpt["feature_table"])
    logs = []
    not_improved_count = 0
    guard_args = {}
    if max_grad_norm is not None:
        guard_args["max_grad_norm"] = max_grad_norm
    if freeze_on_nonfinite:
        guard_args["freeze_on_nonfinite"] = True
    if in_batch:
        guard_args["in_batch"] = True
    if feature_table is not None:
        guard_args["feature_table"] = feature_table
    if taxo_margin is not None:
        from .loss import _checked_gamma
        _checked_gamma(taxo_margin, "fit: taxo_margin")
        if (taxonomy_index is None and not in_batch and loss_fn is None and getattr(train_loader, "attach_anchors", True) is not False
                and hasattr(train_loader, "dataset")):                # (a combination train_epoch refuses is left for it to refuse)
            from .taxometric import TaxonomyIndex
            taxonomy_index = TaxonomyIndex.from_dataset(train_loader.dataset).to(next(model.parameters()).device)
        guard_args["taxo_margin"] = taxo_margin
        if taxonomy_index is not None:
            guard_args["taxonomy_index"] = taxonomy_index
    for epoch in range(start_epoch, epochs + 1):
        mined = None
        if hard is not None and epoch >= hard["start"] and (epoch - hard["start"]) % hard["every"] == 0:
            from .sampler import mine_hard_negatives
            table = mine_hard_negatives(model, train_loader.dataset, train_loader.device, hard["size"], larger_is_better=larger_is_better,
                                        dtax=getattr(train_loader, "dtax", None))
            train_loader.set_hard_negatives(table, hard["slots"])
            mined = {"hard_mined": True, "hard_mean_count": float(table.cnt.double().mean().item())}
        if near is not None and epoch >= near["start"]:
            train_loader.set_near_negatives(near["siblings"], near["grandparents"], near["uncles"])
            near = None                                                # (set once: the loader keeps the counts)
        result = train_epoch_fn(model, train_loader, optimizer, loss_fn=loss_fn, group_size=group_size, **guard_args)
        log = {"epoch": epoch}
        log.update(result)
        if "near_sibling_share" in result:
            logging.getLogger(__name__).info("epoch %d: near negatives accepted -- siblings %.3f, grandparents %.3f, uncles %.3f", epoch,
                                             result["near_sibling_share"], result["near_grandparent_share"], result["near_uncle_share"])
        if mined is not None:
            log.update(mined)
        logs.append(log)
        if result.get("first_nonfinite", -1) >= 0:
            checkpoint = None
            if freeze_on_nonfinite and save_dir is not None:
                os.makedirs(str(save_dir), exist_ok=True)
                checkpoint = os.path.join(str(save_dir), "last_finite.pth")
                torch.save(_checkpoint_state(model, optimizer, epoch - 1, mnt_best, config, averaged, feature_table), checkpoint)
            raise TrainingDiverged(epoch, int(result["first_nonfinite"]), logs, checkpoint)
        if valid_loader is not None:                                   # trainer.py:80-82, base_trainer.py:71-72
            if feature_table is not None:                              # validation reads host features and its own resident table
                feature_table.write_back()
                feature_table.refresh(valid_loader)
            if averaged:
                with optimizer.averaged_parameters():
                    val = validate_fn(model, valid_loader, metrics=metrics, larger_is_better=larger_is_better)
            else:
                val = validate_fn(model, valid_loader, metrics=metrics, larger_is_better=larger_is_better)
            log.update({"val_" + name: v for name, v in zip(metrics, val["val_metrics"])})
        if lr_scheduler is not None:                                   # trainer.py:84-92
            if plateau:
                if scheduler_metric not in log:
                    raise ValueError(f"scheduler_metric {scheduler_metric!r} is not in the epoch's log {sorted(log)}")
                lr_scheduler.step(log[scheduler_metric])
            else:
                lr_scheduler.step()
        best = False
        if mnt_mode != "off":                                          # base_trainer.py:81-104
            if mnt_metric not in log:
                warnings.warn(f"Metric '{mnt_metric}' is not found. Model performance monitoring is disabled.")
                mnt_mode = "off"
            else:
                improved = log[mnt_metric] <= mnt_best if mnt_mode == "min" else log[mnt_metric] >= mnt_best
                if improved:
                    mnt_best, not_improved_count, best = log[mnt_metric], 0, True
                else:
                    not_improved_count += 1
                if not_improved_count > early_stop:
                    break
        if save_dir is not None and epoch % save_period == 0:         # base_trainer.py:106-107
            _save_checkpoint(save_dir, model, optimizer, epoch, mnt_best, config, best, averaged, feature_table)
    return logs
