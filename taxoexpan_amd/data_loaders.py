"""data_loader/data_loaders.py of the reference, on the array-based dataset: the two collate functions (same names, same
outputs) and MaskedGraphDataLoader (same constructor arguments).  `data_path` is a raw dataset directory holding
`<name>.terms/.taxo/.terms.embed` or the `<name>.txe.npz` cache written by taxoexpan_amd.dataset.MAGDataset; the
reference's DGL pickles cannot be read without DGL (dataset.py says so when handed one)."""
import os
import itertools
import logging

import numpy as np
import torch
import torch.utils.data

from . import dataset as _ds
from .graph import batch

BATCH_GRAPH_NODE_LIMIT = 100000      # data_loaders.py:7: nodes per batched graph in large-batch mode


def _flatten(samples):
    """instances (tuples of [egonet, query feature, label] triplets) -> three parallel lists"""
    triplets = list(itertools.chain.from_iterable(samples))
    return [t[0] for t in triplets], [t[1] for t in triplets], [t[2] for t in triplets]


def collate_graph_and_node_small_batch(samples):
    """data_loaders.py:9-28: list of instances -> (batched graph, [B, d] query features, [B] labels)"""
    graphs, node_features, labels = _flatten(samples)
    return batch(graphs), torch.stack(node_features), torch.tensor(labels)


def collate_graph_and_node_large_batch(samples):
    """data_loaders.py:31-72: as above but cut into several batched graphs once a running node count passes
    BATCH_GRAPH_NODE_LIMIT (the egonet that crosses the limit stays in the batch it closes)"""
    graphs, node_features, labels = _flatten(samples)
    out_g, out_f, out_l = [], [], []
    start, nodes = 0, 0
    for i, g in enumerate(graphs):
        nodes += g.number_of_nodes()
        if nodes > BATCH_GRAPH_NODE_LIMIT and i > start:
            out_g.append(batch(graphs[start:i + 1]))
            out_f.append(torch.stack(node_features[start:i + 1]))
            out_l.append(torch.tensor(labels[start:i + 1]))
            start, nodes = i + 1, 0
    if start < len(graphs):
        out_g.append(batch(graphs[start:]))
        out_f.append(torch.stack(node_features[start:]))
        out_l.append(torch.tensor(labels[start:]))
    return out_g, out_f, out_l


def _open_dataset(data_path):
    if os.path.isdir(data_path):
        names = [f[:-len(".terms")] for f in os.listdir(data_path) if f.endswith(".terms")]
        if len(names) != 1:
            raise ValueError(f"{data_path}: expected exactly one <name>.terms file, found {sorted(names)}")
        name = names[0]
        cache = os.path.join(data_path, f"{name}.txe.npz")
        # (the optional existing partition, dataset.py:160-170: a changed split must invalidate the cache too)
        raw = [os.path.join(data_path, f) for f in (f"{name}.terms", f"{name}.taxo", f"{name}.terms.embed", f"{name}.terms.train",
                                                    f"{name}.terms.validation", f"{name}.terms.test")]
        # the cache written by the first raw load is used while it is newer than the raw files (the reference's pickle flow,
        # generate_dataset_binary.py): train / validation / test loaders and every rank parse the text files once, not 3 x world times
        if os.path.exists(cache) and all(os.path.getmtime(cache) >= os.path.getmtime(f) for f in raw if os.path.exists(f)):
            try:
                return _ds.MAGDataset(name=name, path=cache, raw=False)
            except Exception as exc:                  # unreadable cache: say so, fall back to the raw files (which rewrites it)
                logging.getLogger(__name__).warning("ignoring unreadable dataset cache %s (%r): re-reading the raw files", cache, exc)
        return _ds.MAGDataset(name=name, path=data_path, raw=True)
    return _ds.MAGDataset(name="", path=data_path, raw=False)


_COLLATE = {"small_batch": collate_graph_and_node_small_batch, "large_batch": collate_graph_and_node_large_batch}


class MaskedGraphDataLoader(torch.utils.data.DataLoader):
    """data_loaders.py:75-117 (same constructor arguments; `data_path` is a raw directory or a .txe.npz cache)"""

    def __init__(self, mode, data_path, sampling_mode=1, batch_size=10, batch_type="small_batch", negative_size=20, expand_factor=50,
                 shuffle=True, num_workers=8, cache_refresh_time=64, normalize_embed=False, test_topk=-1):
        if batch_type not in _COLLATE:
            raise AssertionError("batch_type arg must be either small_batch or large_batch")
        if mode not in ("train", "validation", "test"):
            raise AssertionError("mode must be one of train, validation, and test")
        self.mode, self.sampling_mode, self.batch_size_, self.batch_type = mode, sampling_mode, batch_size, batch_type
        self.negative_size, self.expand_factor, self.shuffle = negative_size, expand_factor, shuffle
        self.cache_refresh_time, self.normalize_embed = cache_refresh_time, normalize_embed
        self.dataset_ = _ds.MaskedGraphDataset(_open_dataset(data_path), mode=mode, sampling_mode=sampling_mode,
                                               negative_size=negative_size, expand_factor=expand_factor,
                                               cache_refresh_time=cache_refresh_time, normalize_embed=normalize_embed,
                                               test_topk=test_topk)
        collate = _COLLATE[batch_type]
        super().__init__(dataset=self.dataset_, batch_size=batch_size, shuffle=shuffle, collate_fn=collate, num_workers=num_workers,
                         pin_memory=torch.cuda.is_available())
        self.n_samples = len(self.dataset_)

    def __str__(self):
        return "\n\t".join([f"MaskedGraphDataLoader mode: {self.mode}", f"sampling_mode: {self.sampling_mode}",
                            f"batch_size: {self.batch_size_}", f"negative_size: {self.negative_size}",
                            f"expand_factor: {self.expand_factor}", f"cache_refresh_time: {self.cache_refresh_time}",
                            f"normalize_embed: {self.normalize_embed}"])


_PINNED = {}


def begin_device_batch(dtax, anchors, exclude, query_ids, expand_factor=50, seed=0, stream=None, repeated_queries=False):
    """First half of build_device_batch: the index arrays go up in one pinned copy and the egonets' node counts are computed, on
    `stream` (default: the current stream); nothing is waited for.  Returns the job finish_device_batch completes.
    repeated_queries: the batch's query features come back as ops.RepeatedRows -- the runs of equal consecutive query ids are found
    here, on the host, and only the distinct rows are gathered (BIM / LBM then project U rows instead of one per pair)."""
    from .graph import device_egonet_begin
    dev = dtax.device
    main = torch.cuda.current_stream(dev)
    side = stream if stream is not None else main
    # (the side stream does NOT wait for the caller's stream -- that would put the construction behind the running step again: the
    #  taxonomy arrays and the feature table must be complete before the first call; DeviceBatchLoader synchronises once when it is made)
    # the three index arrays travel in ONE pinned buffer and one copy (each small pageable upload costs ~60 us of host time); two
    # buffers per device take turns, each guarded by the event of its last upload (a loader keeps two batches in flight)
    B = len(anchors)
    ring = _PINNED.setdefault(str(dev), dict(k=0, slots=[None, None]))     # per device; the buffers grow to the largest batch seen
    ring["k"] ^= 1
    slot = ring["slots"][ring["k"]]
    if slot is None or slot[0].numel() < 4 * B + 1:               # [anchors | exclude | query ids | run offsets (<= B + 1)]
        if slot is not None and slot[1] is not None:
            slot[1].synchronize()                                 # (the smaller buffer's last upload has left it)
        cap = max(4 * B + 1, 2 * slot[0].numel() if slot is not None else 0)
        slot = ring["slots"][ring["k"]] = [torch.empty(cap, dtype=torch.int32).pin_memory(), None]
    host, uploaded = slot
    if uploaded is not None:
        uploaded.synchronize()
    hv = host.numpy()
    hv[:B] = anchors
    hv[B:2 * B] = exclude if exclude is not None else -1
    n_runs = 0
    if repeated_queries:                                          # distinct consecutive query ids + the first pair of every run
        q = np.asarray(query_ids).reshape(-1)
        start = np.flatnonzero(np.concatenate([[True], q[1:] != q[:-1]])) if B else np.zeros(0, dtype=np.int64)
        n_runs = len(start)
        hv[2 * B:2 * B + n_runs] = q[start]
        hv[3 * B:3 * B + n_runs] = start
        hv[3 * B + n_runs] = B
    else:
        hv[2 * B:3 * B] = query_ids
    with torch.cuda.stream(side):
        packed = host[:4 * B + 1].to(dev, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        job = device_egonet_begin(dtax, packed[:B], packed[B:2 * B] if exclude is not None else None, expand_factor=expand_factor, seed=seed)
        packed.record_stream(side)
    return dict(job=job, packed=packed, B=B, side=side, dev=dev, n_runs=n_runs if repeated_queries else None)


def finish_device_batch(pending, features, table=None):
    """Second half of build_device_batch: waits for the node count of the batch begun earlier (the one host synchronisation of the
    construction; behind work enqueued a whole step ago it returns at once), fills the node table and both CSR views and gathers the
    node / query features on the builder's stream; the CURRENT stream is made to wait for the finished batch, and every tensor of the
    batch is marked as used on it (caching-allocator safety).  Returns dict(g, x, pos, qf, n_nodes, n_edges).
    table (a feature_table.FeatureTable whose weight is `features`; needs repeated_queries): the table changes between batches, so the
    builder's stream waits for table.updated -- the event recorded behind the table's last step -- after the node table and the CSR
    views are filled and before the two gathers; the batch's rows are then the table after that step.  The graph gains g.query_ids,
    the int32 [U] ids of the gathered query rows (a view of the packed array)."""
    from .graph import device_egonet_finish
    side, dev, packed, B = pending["side"], pending["dev"], pending["packed"], pending["B"]
    main = torch.cuda.current_stream(dev)
    with torch.cuda.stream(side):
        U = pending["n_runs"]
        if table is None:
            g = device_egonet_finish(pending["job"], with_features=True)
            x = g.ndata.pop("x")
        else:
            if U is None:
                raise ValueError("a feature table needs repeated_queries=True (its query-side gradient is taken per distinct row)")
            g = device_egonet_finish(pending["job"], with_features=False)
            side.wait_event(table.updated)
            x = features.index_select(0, g.ndata["_id"].long())
            g.query_ids = packed[2 * B:2 * B + U]
        if U is None:
            qt = qf = features.index_select(0, packed[2 * B:3 * B])
        else:                                                     # only the distinct query rows are gathered
            from .ops import RepeatedRows
            qt = features.index_select(0, packed[2 * B:2 * B + U])
            qf = RepeatedRows(qt, packed[3 * B:3 * B + U + 1], B)
        from . import ops
        # the batch's walk plan (a view of its graphs like the CSR orders; the backward sweep of a four-head stack stages from it)
        plan = ops.walk_plan(g.csr(dev)) if not (ops._NO_EGO_WALK or ops._NO_WALK_PLAN) else None
    if side is not main:
        main.wait_stream(side)
        csr = g.csr(dev)
        packed.record_stream(main)
        for t in (x, qt, g.ndata["_id"], g.ndata["pos"], csr.rowptr_in, csr.col_src, csr.eid_in, csr.rowptr_out, csr.col_dst, csr.pos_out,
                  csr.graph_off) + ((plan,) if plan is not None else ()):
            t.record_stream(main)
    return dict(g=g, x=x, pos=g.ndata["pos"], qf=qf, n_nodes=g.number_of_nodes(), n_edges=g.number_of_edges())


def build_device_batch(dtax, anchors, exclude, query_ids, features, expand_factor=50, seed=0, stream=None, repeated_queries=False):
    """One training batch built ON the device (data_loaders.py:9-28 + dataset.py:404-437 without host egonet objects):
    graph.device_egonet_batch for the anchors, node features and query features gathered from the resident table.
    stream: build on that side stream -- the one host synchronisation of the construction (the array sizes) then waits for the
    builder's own few microseconds of work only, not for the training step still running on the caller's stream.  A loop that
    calls begin_device_batch for batch i+1 BEFORE it enqueues step i does not wait at all (DeviceBatchLoader does).
    Returns dict(g, x, pos, qf, n_nodes, n_edges)."""
    return finish_device_batch(begin_device_batch(dtax, anchors, exclude, query_ids, expand_factor, seed, stream, repeated_queries), features)


class DeviceBatchLoader:
    """`for batch in loader` over a MaskedGraphDataset in 'train' / 'validation' mode with the batches built on the GPU: the sampler
    (dataset.sample_anchors: the reference's positive pointer and negative sampling, host Python like data_loader/dataset.py:334-381)
    hands anchors to begin_device_batch / finish_device_batch.  Each batch is built on a side stream while the previous step runs,
    in two halves around the consumer's enqueue of that step: batch b+1 is BEGUN (sampled, uploaded, node counts launched) before
    batch b is handed out and FINISHED (arrays sized from the count, filled, features gathered) at the next `next()`, so the one host
    synchronisation of the construction finds its value already there.
    repeated_queries (default): the query features are an ops.RepeatedRows -- the sampler pairs one query with 1 + negative_size
    consecutive anchors, only the distinct rows are gathered and BIM / LBM project those (every other matcher of model_zoo densifies it;
    `.dense()` gives the reference's stacked [B, in_dim] tensor); False: the stacked tensor itself.  Yields (graph, node features, query features, labels) -- MaskedGraphDataLoader's small-batch
    tuple with the node features popped, all on `device`.
    sampler="host" (default): the anchors come from dataset.sample_anchors (the reference's `random`-module trace, host Python per pair).
    sampler="device" (sampling_mode 1, train / validation): sampler.DeviceAnchorSampler draws them on the side stream in one launch per
    batch -- no host work per pair, no upload per batch (the epoch order goes up once per epoch), labels a cached device tensor.  Its
    positives walk the same pointers as the host sampler, starting from the dataset's node2positive_pointer when the loader is made; the
    host dict is NOT advanced by device sampling.  Negatives follow the reference's distribution, not its `random` trace (sampler.py).
    hard_negatives / hard_slots (this sampler only; default off): a sampler.HardNegatives table whose rows fill the first hard_slots
    negative slots of every query (txe_sample_anchors' table slots); set_hard_negatives changes it between epochs.
    near_negatives (this sampler only; default None: the loader launches what it launched): dict(siblings=, grandparents=, uncles=), the
    negative slots behind the hard ones that propose a node of the positive's taxonomy neighbourhood -- another child of it, a parent of
    it, a child of one of its parents (txe_sample_anchors' near slots); a proposal that is masked, outside the pool or absent
    leaves its slot to the pool draw.  set_near_negatives changes the counts between epochs; sampler.near_counts() reads the accepted
    proposals.  The packed layout is unchanged, so in_batch, attach_anchors, the feature table and the hard table compose.
    in_batch=True (this sampler, repeated_queries=True; ValueError otherwise): every batch's graph carries `g.in_batch`, a
    sampler.InBatchGroups -- views of the sampler's index array and mask CSR for loss.in_batch_info_nce; the 4-tuple keeps its shape.
    attach_anchors=True (this sampler; ValueError otherwise; default off: the loader launches and yields what it did): every batch's graph
    carries `g.anchors`, the int32 [Q, 1 + negative_size] view of the sampler's anchors (positive first) that loss.taxo_info_nce reads;
    with in_batch=True as well, g.anchors and g.in_batch.anchor share storage.
    sampler="device" on a sampling_mode 0 dataset (validation batches of the shipped configs; train / validation): sampler.DeviceGroupSampler
    draws every parent and at most negative_size negatives per query, labels an int64 device tensor.  The batch size B is then known on
    the device only, so three batches are in flight: each next() after the first finishes batch b (its node count, read back one next()
    ago), begins the egonet count of batch b+1 (its B, read back one next() ago) and samples batch b+2 -- no next() waits on work it
    enqueued itself.
    feature_table (a feature_table.FeatureTable; needs repeated_queries=True, ValueError otherwise; default None: nothing changes): the
    loader gathers from table.weight, which the table's step rewrites between batches.  Batch b+1 is still BEGUN (sampled, uploaded, its
    node counts launched) while step b runs; its two gathers wait on the side stream for table.updated, so its rows are the table after
    step b (finish_device_batch).  Every graph gains g.query_ids, the int32 [U] ids of the distinct query rows."""

    def __init__(self, dataset, batch_size, device, shuffle=True, seed=0, drop_last=False, repeated_queries=True, sampler="host",
                 hard_negatives=None, hard_slots=0, in_batch=False, feature_table=None, attach_anchors=False, near_negatives=None):
        if sampler not in ("host", "device"):
            raise ValueError(f"sampler must be 'host' or 'device', got {sampler!r}")
        if feature_table is not None and not repeated_queries:
            raise ValueError("feature_table needs repeated_queries=True (the table's query-side gradient is taken per distinct query row)")
        if in_batch and not (sampler == "device" and dataset.sampling_mode == 1 and repeated_queries):
            raise ValueError("in_batch=True needs sampler='device', a sampling_mode 1 dataset and repeated_queries=True (the in-batch "
                             "groups are views of the device sampler's index array)")
        self.in_batch = bool(in_batch)
        if attach_anchors and not (sampler == "device" and dataset.sampling_mode == 1):
            raise ValueError("attach_anchors=True needs sampler='device' and a sampling_mode 1 dataset (g.anchors is a view of the device "
                             "sampler's index array, 1 + negative_size columns per query)")
        self.attach_anchors = bool(attach_anchors)
        if hard_negatives is not None and not (sampler == "device" and dataset.sampling_mode == 1):
            raise ValueError("hard negatives need sampler='device' on a sampling_mode 1 dataset")
        if near_negatives is not None and not (sampler == "device" and dataset.sampling_mode == 1):
            raise ValueError("near negatives need sampler='device' on a sampling_mode 1 dataset")
        self.repeated_queries = bool(repeated_queries)
        self.dataset, self.batch_size, self.device = dataset, int(batch_size), torch.device(device)
        self.shuffle, self.seed, self.drop_last = shuffle, int(seed), drop_last
        self.feature_table = feature_table
        if feature_table is None:
            self.dtax = dataset.device_taxonomy(self.device)
        else:                                                     # the table's storage IS the resident feature table
            dev = self.device if self.device.index is not None else torch.device(self.device.type, torch.cuda.current_device())
            if feature_table.device != dev or tuple(feature_table.weight.shape) != tuple(dataset.node_features.shape):
                raise ValueError("feature_table lives on another device or has another shape than the dataset's feature table")
            self.dtax = feature_table.dtax if feature_table.dataset is dataset else dataset.device_taxonomy(self.device)
            self.dtax.features = feature_table.weight
        self.features = self.dtax.features
        self._side = torch.cuda.Stream(device=self.device)
        self.sampler = None
        if sampler == "device" and dataset.sampling_mode == 0:
            from .sampler import DeviceGroupSampler
            self.sampler = DeviceGroupSampler(dataset, self.device, seed=self.seed, dtax=self.dtax)
        elif sampler == "device":
            from .sampler import DeviceAnchorSampler
            self.sampler = DeviceAnchorSampler(dataset, self.device, seed=self.seed, dtax=self.dtax)
            self._labels, self._pos_cols = {}, {}
        torch.cuda.current_stream(self.device).synchronize()      # the resident taxonomy / feature table are complete from here on
        self._epoch = 0
        if hard_negatives is not None:
            self.set_hard_negatives(hard_negatives, hard_slots)
        if near_negatives is not None:
            self.set_near_negatives(**near_negatives)

    def set_hard_negatives(self, table, slots=0):
        """from the next epoch's first batch on, the first `slots` negatives of every query come from `table` (sampler.HardNegatives,
        e.g. sampler.mine_hard_negatives; None: uniform draws again) -- DeviceAnchorSampler.set_hard_negatives.  ValueError on a loader
        whose sampler is 'host' or the sampling_mode 0 group sampler, for slots outside [0, negative_size] or a table of another row
        count; RuntimeError while an epoch is being iterated (two batches are in flight on the side stream)."""
        from .sampler import DeviceAnchorSampler
        if not isinstance(self.sampler, DeviceAnchorSampler):
            raise ValueError("hard negatives need sampler='device' on a sampling_mode 1 dataset (the host sampler and the sampling_mode 0 "
                             "group sampler draw from the pool only)")
        self.sampler.set_hard_negatives(table, slots)

    def set_near_negatives(self, siblings=0, grandparents=0, uncles=0):
        """from the next epoch's first batch on, that many negative slots of every query (behind the hard slots) propose a sibling, a
        grandparent, an uncle of the query -- DeviceAnchorSampler.set_near_negatives; all 0: the pool (and the table) alone again.
        ValueError on a loader whose sampler is 'host' or the sampling_mode 0 group sampler, for a count that is not an integer >= 0 or
        a sum with the hard slots above negative_size; RuntimeError while an epoch is being iterated."""
        from .sampler import DeviceAnchorSampler
        if not isinstance(self.sampler, DeviceAnchorSampler):
            raise ValueError("near negatives need sampler='device' on a sampling_mode 1 dataset (the host sampler and the sampling_mode 0 "
                             "group sampler draw from the pool only)")
        self.sampler.set_near_negatives(siblings, grandparents, uncles)

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        import random
        order = list(range(len(self.dataset)))
        if self.shuffle:
            random.Random(self.seed + self._epoch).shuffle(order)
        self._epoch += 1
        if self.sampler is not None:
            from .sampler import DeviceGroupSampler
            it = self._iter_groups if isinstance(self.sampler, DeviceGroupSampler) else self._iter_device
            yield from it(order, self._epoch - 1)
            return
        def begin(b):
            idx = order[b * self.batch_size:(b + 1) * self.batch_size]
            query, anchor, label, exclude = self.dataset.sample_anchors(idx)
            return label, begin_device_batch(self.dtax, anchor, exclude, query, expand_factor=self.dataset.expand_factor,
                                             seed=self.seed + 7919 * self._epoch + b, stream=self._side, repeated_queries=self.repeated_queries)
        # two batches in flight: batch b+1 is begun (sampled, uploaded, node counts launched) before the consumer gets batch b, so the
        # count's read-back has a whole step's enqueue to arrive and `finish` never waits
        nxt = begin(0) if len(self) else None
        for b in range(len(self)):
            label, pending = nxt
            batch = finish_device_batch(pending, self.features, self.feature_table)
            nxt = begin(b + 1) if b + 1 < len(self) else None
            yield batch["g"], batch["x"], batch["qf"], torch.as_tensor(label).to(self.device, non_blocking=True)

    def _label(self, Q):
        """[1, 0 x k] per query, int64 on the device, made once per batch size"""
        lab = self._labels.get(Q)
        if lab is None:
            lab = torch.zeros(Q, 1 + self.sampler.k, dtype=torch.int64, device=self.device)
            lab[:, 0] = 1
            lab = self._labels[Q] = lab.reshape(-1)
        return lab

    def _in_batch_groups(self, packed, Q):
        """sampler.InBatchGroups over the finished batch's packed index array: views, marked as used on the consumer's stream like the
        batch's other tensors; pos_col = i (1 + k), made once per batch size"""
        from .sampler import InBatchGroups
        pos_col = self._pos_cols.get(Q)
        if pos_col is None:
            pos_col = self._pos_cols[Q] = torch.arange(Q, dtype=torch.int32, device=self.device) * (1 + self.sampler.k)
        a = self.sampler.arrays
        groups = InBatchGroups.from_packed(packed, Q, self.sampler.k, pos_col, a["mask_ptr"], a["mask_idx"])
        groups.record_stream(torch.cuda.current_stream(self.device))
        return groups

    def _anchors(self, packed, Q):
        """the anchors of the finished batch as int32 [Q, 1 + k] (group-major, positive first): a view of packed[:B] -- the storage
        g.in_batch.anchor views too --, marked as used on the consumer's stream like the batch's other tensors"""
        C = 1 + self.sampler.k
        anchors = packed[:Q * C].view(Q, C)
        anchors.record_stream(torch.cuda.current_stream(self.device))
        return anchors

    def _iter_device(self, order, epoch):
        n, bs = len(order), self.batch_size
        order_dev = self.sampler.upload_order(order, self._side)     # once per epoch, on the side stream the launches use
        def begin(b):
            Q = min(bs, n - b * bs)
            return Q, self.sampler.begin(order_dev, b * bs, Q, epoch, self.repeated_queries, self._side,
                                         egonet_seed=self.seed + 7919 * self._epoch + b)
        self.sampler.in_epoch = True                                 # (set_hard_negatives / set_near_negatives refuse until the epoch's batches are out)
        try:
            nxt = begin(0) if len(self) else None
            for b in range(len(self)):
                Q, pending = nxt
                batch = finish_device_batch(pending, self.features, self.feature_table)
                nxt = begin(b + 1) if b + 1 < len(self) else None
                if self.in_batch:
                    batch["g"].in_batch = self._in_batch_groups(pending["packed"], Q)
                if self.attach_anchors:
                    batch["g"].anchors = self._anchors(pending["packed"], Q)
                yield batch["g"], batch["x"], batch["qf"], self._label(Q)
        finally:
            self.sampler.in_epoch = False

    def _iter_groups(self, order, epoch):
        """sampling_mode 0: sample b+2, begin the egonet count of b+1, finish b (see the class docstring)"""
        n, bs, nb = len(order), self.batch_size, len(self)
        order_dev = self.sampler.upload_order(order, self._side)
        main = torch.cuda.current_stream(self.device)
        sample = lambda b: self.sampler.sample(order_dev, b * bs, min(bs, n - b * bs), epoch, self.repeated_queries, self._side)
        begin = lambda b, sampled: self.sampler.egonet_begin(sampled, egonet_seed=self.seed + 7919 * self._epoch + b)
        sampled = [sample(b) for b in range(min(nb, 2))]
        nxt = begin(0, sampled.pop(0)) if nb else None
        for b in range(nb):
            pending, labels = nxt
            batch = finish_device_batch(pending, self.features, self.feature_table)
            if self._side is not main:
                labels.record_stream(main)
            nxt = begin(b + 1, sampled.pop(0)) if b + 1 < nb else None
            if b + 2 < nb:
                sampled.append(sample(b + 2))
            yield batch["g"], batch["x"], batch["qf"], labels
