"""Training-anchor sampling on the GPU for sampling_mode 1 (data_loader/dataset.py:334-381: one positive per query through the positive
pointer, exactly negative_size negatives): csrc/txe_sample.hip writes a batch straight into the packed index layout begin_device_batch
uploads, so the egonet builder behind it is unchanged.

What is reproduced: the positive walk exactly (the same pointer arithmetic over the same parent lists, so the positives of any sequence
of epoch orders equal the host sampler's), and the distribution of the negatives -- uniform over the distinct content of the reference's
5x queue (sorted(all_positions)), rejected while masked.  What is not: the `random`-module trace of the queue shuffles (a negative slot
is a counter-based hash of (seed, epoch, epoch position, slot, attempt), host_draw restates it bit for bit) and the negative-egonet
cache (dataset.py:390-400), which the device egonet builder never had either."""
import numpy as np
import torch

from . import _lib
from .rng import _mix64

TRIES = 64           # SAMPLE_TRIES of csrc/txe_sample.hip: rejections before a slot keeps its (masked) last draw


def _check(dataset):
    if dataset.mode == "test":
        raise ValueError("device sampling draws training negatives: mode 'test' emits all candidates (use evaluate())")
    if dataset.sampling_mode != 1:
        raise ValueError(f"device sampling implements sampling_mode 1 only, got {dataset.sampling_mode}")
    if dataset.negative_size < 1:
        raise ValueError(f"device sampling needs negative_size >= 1, got {dataset.negative_size}")


def _csr(n, rows):
    """{node: iterable of ids} -> (ptr [n+1], idx) int32, rows in the given order"""
    cnt = np.zeros(n, dtype=np.int64)
    for v, r in rows.items():
        cnt[v] = len(r)
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    idx = np.zeros(int(ptr[-1]), dtype=np.int32)
    for v, r in rows.items():
        idx[ptr[v]:ptr[v + 1]] = r
    return ptr, idx


def sampler_arrays(dataset):
    """The resident inputs of txe_sample_anchors as numpy int32 arrays, from a MaskedGraphDataset (no GPU needed):
    node_list, the query-parent CSR (par_ptr / par_idx, node2parents' order), the mask CSR (mask_ptr / mask_idx, node2masks[q] sorted),
    pool = sorted(all_positions), ptr = node2positive_pointer per node, and k = negative_size."""
    _check(dataset)
    n = int(dataset.node_features.shape[0])
    node_list = np.asarray(dataset.node_list, dtype=np.int32)
    par_ptr, par_idx = _csr(n, dataset.node2parents)
    if len(node_list) and (np.diff(par_ptr)[node_list] == 0).any():
        raise ValueError("a query without a parent cannot be sampled")
    mask_ptr, mask_idx = _csr(n, {q: sorted(m) for q, m in dataset.node2masks.items()})
    ptr = np.zeros(n, dtype=np.int32)
    for v, c in dataset.node2positive_pointer.items():
        ptr[v] = c
    pool = np.asarray(sorted(dataset.all_positions), dtype=np.int32)
    if len(pool) == 0:
        raise ValueError("device sampling needs a non-empty negative pool (all_positions)")
    return dict(node_list=node_list, par_ptr=par_ptr, par_idx=par_idx, mask_ptr=mask_ptr, mask_idx=mask_idx, pool=pool, ptr=ptr,
                k=int(dataset.negative_size))


def _ctr(epoch, s, j, t):
    u = lambda a: np.asarray(a).astype(np.uint64)
    return (u(epoch) << np.uint64(44)) | (u(s) << np.uint64(20)) | (u(j) << np.uint64(6)) | u(t)


def host_draw(arrays, order, start, Q, epoch, seed, ptr=None, repeated_queries=False):
    """numpy restatement of txe_sample_anchors for the Q queries at positions start .. start+Q-1 of `order` (indices into node_list).
    ptr: the positive pointers (int32 [n]), advanced in place; default a copy of arrays['ptr'].  Returns dict(anchors, exclude, query
    [B]; runs [Q] and offsets [Q+1] with repeated_queries; n_padded) -- the arrays the kernel writes, bit for bit."""
    k = arrays["k"]
    pool, mask_ptr, mask_idx = arrays["pool"], arrays["mask_ptr"], arrays["mask_idx"]
    ptr = arrays["ptr"].copy() if ptr is None else ptr
    s = np.arange(start, start + Q, dtype=np.int64)
    q = arrays["node_list"][np.asarray(order, dtype=np.int64)[s]].astype(np.int64)
    pos = np.empty(Q, dtype=np.int64)
    for i, v in enumerate(q):                                  # dataset.py:336-340, in order (a query appears once per epoch)
        b, n = arrays["par_ptr"][v], arrays["par_ptr"][v + 1] - arrays["par_ptr"][v]
        c = int(ptr[v])
        pos[i] = arrays["par_idx"][b + c]
        ptr[v] = (c + 1) % n
    with np.errstate(over="ignore"):
        j, t = np.arange(k)[None, :, None], np.arange(TRIES)[None, None, :]
        h = _mix64(np.uint64(seed) ^ _mix64(_ctr(epoch, s[:, None, None], j, t)))
        draws = pool[(((h >> np.uint64(32)) * np.uint64(len(pool))) >> np.uint64(32)).astype(np.int64)]      # [Q, k, TRIES]
    neg = np.empty((Q, k), dtype=np.int64)
    n_padded = 0
    for i, v in enumerate(q):
        row = mask_idx[mask_ptr[v]:mask_ptr[v + 1]]
        ok = ~np.isin(draws[i], row)
        first = np.where(ok.any(1), ok.argmax(1), TRIES - 1)
        n_padded += int((~ok.any(1)).sum())
        neg[i] = draws[i, np.arange(k), first]
    anchors = np.concatenate([pos[:, None], neg], 1).reshape(-1)
    exclude = np.concatenate([q[:, None], np.full((Q, k), -1, dtype=np.int64)], 1).reshape(-1)
    out = dict(anchors=anchors, exclude=exclude, query=np.repeat(q, 1 + k), n_padded=n_padded)
    if repeated_queries:
        out["runs"], out["offsets"] = q, np.arange(Q + 1, dtype=np.int64) * (1 + k)
    return out


class DeviceAnchorSampler:
    """sampler_arrays(dataset) resident on `device`, with the positive pointers (from node2positive_pointer when made; device sampling
    does NOT advance the host dict) and a padded-slot counter.  begin() launches the sampler and the egonet node count on one stream."""

    def __init__(self, dataset, device, seed=0, dtax=None):
        _check(dataset)
        self.dataset, self.device, self.seed = dataset, torch.device(device), int(seed)
        a = sampler_arrays(dataset)
        self.k, self.n_pool, self.n_queries = a["k"], len(a["pool"]), len(a["node_list"])
        up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(self.device)
        self.arrays = {name: up(v) for name, v in a.items() if name != "k"}
        self._padded = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.dtax = dtax if dtax is not None else dataset.device_taxonomy(self.device)
        torch.cuda.current_stream(self.device).synchronize()     # resident before a side stream reads them

    def upload_order(self, order, stream=None):
        """an epoch's order (indices into node_list) as an int32 device tensor, copied on `stream` (once per epoch)"""
        o = np.asarray(order, dtype=np.int64)
        if o.size and (o.min() < 0 or o.max() >= self.n_queries):
            raise ValueError("order holds an index outside the dataset")
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            return torch.from_numpy(o.astype(np.int32)).to(self.device)

    def launch(self, order_dev, start, Q, epoch, repeated_queries=True, stream=None):
        """txe_sample_anchors alone: the packed [4B + 1] int32 index arrays of the batch, written on `stream` (default: current)"""
        a = self.arrays
        B = Q * (1 + self.k)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)), _lib.on_device(self.device):
            packed = torch.empty(4 * B + 1, dtype=torch.int32, device=self.device)
            _lib.call("txe_sample_anchors", _lib.ptr(order_dev), int(order_dev.numel()), int(start), int(Q), _lib.ptr(a["node_list"]),
                      _lib.ptr(a["par_ptr"]), _lib.ptr(a["par_idx"]), _lib.ptr(a["mask_ptr"]), _lib.ptr(a["mask_idx"]), _lib.ptr(a["pool"]),
                      self.n_pool, _lib.ptr(a["ptr"]), self.k, self.seed, int(epoch), int(bool(repeated_queries)), _lib.ptr(packed),
                      _lib.ptr(self._padded), _lib.stream_ptr())
        return packed

    def begin(self, order_dev, start, Q, epoch, repeated_queries=True, stream=None, egonet_seed=0):
        """begin_device_batch's job for the Q queries at positions start .. start+Q-1 of the epoch order: sampled, egonet node counts
        launched, nothing waited for (data_loaders.finish_device_batch completes it)"""
        from .graph import device_egonet_begin
        dev = self.device
        side = stream if stream is not None else torch.cuda.current_stream(dev)
        B = Q * (1 + self.k)
        packed = self.launch(order_dev, start, Q, epoch, repeated_queries, side)
        with torch.cuda.stream(side):
            job = device_egonet_begin(self.dtax, packed[:B], packed[B:2 * B], expand_factor=self.dataset.expand_factor, seed=egonet_seed)
        return dict(job=job, packed=packed, B=B, side=side, dev=dev, n_runs=Q if repeated_queries else None)

    def padded(self):
        """negative slots that kept a masked draw since the sampler was made (synchronises the device)"""
        torch.cuda.synchronize(self.device)
        return int(self._padded.item())

    def pointers(self):
        """the positive pointers (int32 numpy [n_nodes]) after every launch so far (synchronises the device)"""
        torch.cuda.synchronize(self.device)
        return self.arrays["ptr"].cpu().numpy()


# ---- sampling_mode 0 (validation batches of the shipped configs): every parent, then at most k negatives ---------------------------------

def _check_groups(dataset):
    if dataset.mode == "test":
        raise ValueError("device sampling draws validation negatives: mode 'test' emits all candidates (use evaluate())")
    if dataset.sampling_mode != 0:
        raise ValueError(f"device group sampling implements sampling_mode 0 only, got {dataset.sampling_mode}")
    if dataset.negative_size < 1:
        raise ValueError(f"device sampling needs negative_size >= 1, got {dataset.negative_size}")


def group_sampler_arrays(dataset):
    """The resident inputs of txe_sample_groups as numpy int32 arrays, from a MaskedGraphDataset in sampling_mode 0 (no GPU needed):
    node_list, the query-parent CSR (node2parents' order), the mask CSR (node2masks[q] sorted), pool = sorted(all_positions), and
    k = negative_size.  (sampling_mode 0 has no positive pointer: every parent is emitted.)"""
    _check_groups(dataset)
    n = int(dataset.node_features.shape[0])
    node_list = np.asarray(dataset.node_list, dtype=np.int32)
    par_ptr, par_idx = _csr(n, dataset.node2parents)
    mask_ptr, mask_idx = _csr(n, {q: sorted(m) for q, m in dataset.node2masks.items()})
    pool = np.asarray(sorted(dataset.all_positions), dtype=np.int32)
    if len(pool) == 0:
        raise ValueError("device sampling needs a non-empty negative pool (all_positions)")
    return dict(node_list=node_list, par_ptr=par_ptr, par_idx=par_idx, mask_ptr=mask_ptr, mask_idx=mask_idx, pool=pool,
                k=int(dataset.negative_size))


def host_draw_groups(arrays, order, start, Q, epoch, seed, repeated_queries=False):
    """numpy restatement of txe_sample_groups for the Q queries at positions start .. start+Q-1 of `order` (indices into node_list):
    per query its parents (label 1, exclude = q), then the unmasked draws of the first round t whose k slot draws are not all masked, in
    slot order (label 0, exclude = -1); after TRIES empty rounds, slot 0 of the last round, counted in n_padded.  Returns dict(anchors,
    exclude, query, label [B]; runs [Q] and offsets [Q+1] with repeated_queries; n_padded) -- what the kernel writes, bit for bit."""
    k = arrays["k"]
    pool, mask_ptr, mask_idx = arrays["pool"], arrays["mask_ptr"], arrays["mask_idx"]
    par_ptr, par_idx = arrays["par_ptr"], arrays["par_idx"]
    s = np.arange(start, start + Q, dtype=np.int64)
    q = arrays["node_list"][np.asarray(order, dtype=np.int64)[s]].astype(np.int64)
    neg = [None] * Q
    pending = np.arange(Q)
    n_padded = 0
    for t in range(TRIES):                                     # round t for the queries whose earlier rounds were all masked
        if not len(pending):
            break
        with np.errstate(over="ignore"):
            h = _mix64(np.uint64(seed) ^ _mix64(_ctr(epoch, s[pending, None], np.arange(k)[None, :], t)))
            draws = pool[(((h >> np.uint64(32)) * np.uint64(len(pool))) >> np.uint64(32)).astype(np.int64)]     # [pending, k]
        left = []
        for r, i in enumerate(pending):
            row = mask_idx[mask_ptr[q[i]]:mask_ptr[q[i] + 1]]
            keep = draws[r][~np.isin(draws[r], row)]
            if len(keep):
                neg[i] = keep.astype(np.int64)
            elif t == TRIES - 1:
                neg[i] = draws[r][:1].astype(np.int64)
                n_padded += 1
            else:
                left.append(i)
        pending = np.asarray(left, dtype=np.int64)
    anchors, exclude, query, label, offsets = [], [], [], [], [0]
    for i, v in enumerate(q):
        par = par_idx[par_ptr[v]:par_ptr[v + 1]].astype(np.int64)
        n = len(par) + len(neg[i])
        anchors += [par, neg[i]]
        exclude += [np.full(len(par), v, dtype=np.int64), np.full(len(neg[i]), -1, dtype=np.int64)]
        query.append(np.full(n, v, dtype=np.int64))
        label += [np.ones(len(par), dtype=np.int64), np.zeros(len(neg[i]), dtype=np.int64)]
        offsets.append(offsets[-1] + n)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    out = dict(anchors=cat(anchors), exclude=cat(exclude), query=cat(query), label=cat(label), n_padded=n_padded)
    if repeated_queries:
        out["runs"], out["offsets"] = q, np.asarray(offsets, dtype=np.int64)
    return out


class DeviceGroupSampler:
    """group_sampler_arrays(dataset) resident on `device`, and a padded-query counter.  A batch's total B is known on the device only:
    sample() launches txe_sample_groups into buffers sized by the host-known capacity (sum of |parents| + Q k) and starts an
    asynchronous read-back of B into a pinned slot; egonet_begin() later waits for that read-back (long arrived when it is one loader
    step old) and begins the egonet node count on the B pairs.  The negative-egonet cache of the reference (dataset.py:390-400) is not
    reproduced: the device egonet builder never had one."""

    def __init__(self, dataset, device, seed=0, dtax=None):
        _check_groups(dataset)
        self.dataset, self.device, self.seed = dataset, torch.device(device), int(seed)
        a = group_sampler_arrays(dataset)
        self.k, self.n_pool, self.n_queries = a["k"], len(a["pool"]), len(a["node_list"])
        self._n_par = np.diff(a["par_ptr"]).astype(np.int64)[a["node_list"].astype(np.int64)]      # |parents| per node_list entry
        up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(self.device)
        self.arrays = {name: up(v) for name, v in a.items() if name != "k"}
        self._padded = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.dtax = dtax if dtax is not None else dataset.device_taxonomy(self.device)
        self._slots = []                                             # free pinned int32 read-back slots
        torch.cuda.current_stream(self.device).synchronize()

    def upload_order(self, order, stream=None):
        """an epoch's order (indices into node_list) as an int32 device tensor, copied on `stream` (once per epoch)"""
        o = np.asarray(order, dtype=np.int64)
        if o.size and (o.min() < 0 or o.max() >= self.n_queries):
            raise ValueError("order holds an index outside the dataset")
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            t = torch.from_numpy(o.astype(np.int32)).to(self.device)
        t.host_order = o
        return t

    def capacity(self, order, start, Q):
        """the largest B the Q queries at positions start .. start+Q-1 can give: their parents plus k negatives each"""
        o = np.asarray(order, dtype=np.int64)[start:start + Q]
        return int(self._n_par[o].sum()) + Q * self.k

    def launch(self, order_dev, start, Q, epoch, repeated_queries=True, stream=None):
        """txe_sample_groups alone, on `stream` (default: current): dict(packed [4 cap + 1] int32, labels [cap] int64, total [1] int32
        (B, on the device), cap).  packed's layout uses the stride B: packed[:4B + 1] is what begin_device_batch would upload."""
        a = self.arrays
        cap = self.capacity(order_dev.host_order, start, Q)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)), _lib.on_device(self.device):
            packed = torch.empty(4 * cap + 1, dtype=torch.int32, device=self.device)
            labels = torch.empty(max(cap, 1), dtype=torch.int64, device=self.device)
            total = torch.empty(2 + 3 * Q, dtype=torch.int32, device=self.device)         # [B | pad | ws 3Q + 1 ... ]
            _lib.call("txe_sample_groups", _lib.ptr(order_dev), int(order_dev.numel()), int(start), int(Q), _lib.ptr(a["node_list"]),
                      _lib.ptr(a["par_ptr"]), _lib.ptr(a["par_idx"]), _lib.ptr(a["mask_ptr"]), _lib.ptr(a["mask_idx"]), _lib.ptr(a["pool"]),
                      self.n_pool, self.k, self.seed, int(epoch), int(bool(repeated_queries)), cap, _lib.ptr(packed), _lib.ptr(labels),
                      _lib.ptr(total), _lib.ptr(total[1:]), _lib.ptr(self._padded), _lib.stream_ptr())
        return dict(packed=packed, labels=labels, total=total[:1], cap=cap, Q=Q)

    def sample(self, order_dev, start, Q, epoch, repeated_queries=True, stream=None):
        """launch() plus the asynchronous read-back of B into a pinned slot (nothing is waited for)"""
        side = stream if stream is not None else torch.cuda.current_stream(self.device)
        out = self.launch(order_dev, start, Q, epoch, repeated_queries, side)
        slot = self._slots.pop() if self._slots else torch.empty(1, dtype=torch.int32).pin_memory()
        with torch.cuda.stream(side):
            slot.copy_(out["total"], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        out.update(host_B=slot, ready=ev, side=side, repeated=bool(repeated_queries))
        return out

    def egonet_begin(self, sampled, egonet_seed=0):
        """begin_device_batch's job for a sample() result: waits for its B (one step old in DeviceBatchLoader: already there), then
        launches the egonet node count on the side stream.  Returns (pending for data_loaders.finish_device_batch, labels [B])."""
        from .graph import device_egonet_begin
        sampled["ready"].synchronize()
        B = int(sampled["host_B"][0])
        self._slots.append(sampled["host_B"])
        if not 0 < B <= sampled["cap"]:
            raise RuntimeError(f"txe_sample_groups gave a batch of {B} pairs for a capacity of {sampled['cap']}")
        packed, side = sampled["packed"], sampled["side"]
        with torch.cuda.stream(side):
            job = device_egonet_begin(self.dtax, packed[:B], packed[B:2 * B], expand_factor=self.dataset.expand_factor, seed=egonet_seed)
        pending = dict(job=job, packed=packed[:4 * B + 1], B=B, side=side, dev=self.device, n_runs=sampled["Q"] if sampled["repeated"] else None)
        return pending, sampled["labels"][:B]

    def padded(self):
        """queries that kept a masked negative since the sampler was made (synchronises the device)"""
        torch.cuda.synchronize(self.device)
        return int(self._padded.item())
