"""GPU: the device anchor sampler (csrc/txe_sample.hip, taxoexpan_amd/sampler.py) against its numpy restatement (bit for bit), the host
sampler's positive walk, the mask, a uniformity test, and DeviceBatchLoader(sampler="device") against the in-line builder."""
import copy
import os
import random
import shutil

import numpy as np
import pytest
import torch

from golden_util import GOLDEN_DIR

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _toy(tmp_path, **kw):
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    d = tmp_path / "toy"
    d.mkdir(exist_ok=True)
    for fn in os.listdir(os.path.join(GOLDEN_DIR, "toy_taxo")):
        shutil.copy(os.path.join(GOLDEN_DIR, "toy_taxo", fn), d)
    random.seed(0)
    opts = dict(mode="train", sampling_mode=1, negative_size=7, expand_factor=5, normalize_embed=True)
    opts.update(kw)
    return MaskedGraphDataset(MAGDataset("toy", str(d), raw=True), **opts)


def _synthetic(tmp_path, **kw):
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


def _model(dev, in_dim):
    from taxoexpan_amd import TaxoExpan
    torch.manual_seed(0)
    return TaxoExpan("PGAT", "WMR", "LBM", in_dim=in_dim, hidden_dim=16, out_dim=16, pos_dim=4, num_layers=1, heads=[2, 1], feat_drop=0.1,
                     attn_drop=0.1, hidden_drop=0.1, out_drop=0.1).to(dev)


def _check_batch(packed, want, Q, k, repeated):
    B = Q * (1 + k)
    p = packed.cpu().numpy()
    assert np.array_equal(p[:B], want["anchors"]) and np.array_equal(p[B:2 * B], want["exclude"])
    if repeated:
        assert np.array_equal(p[2 * B:2 * B + Q], want["runs"]) and np.array_equal(p[3 * B:3 * B + Q + 1], want["offsets"])
    else:
        assert np.array_equal(p[2 * B:3 * B], want["query"])


@pytest.mark.parametrize("data,k", [("toy", 7), ("toy", 70), ("synthetic", 7), ("synthetic", 70)])
def test_device_draw_is_bit_equal_to_host_draw_over_three_epochs(tmp_path, data, k):
    """anchors, exclude, query ids and run offsets equal sampler.host_draw bit for bit (k = 70: the lane loop's second pass); every
    negative is a pool node outside the query's mask; no slot is padded; the pointers read back equal the restatement's"""
    from taxoexpan_amd.sampler import DeviceAnchorSampler, host_draw, sampler_arrays
    dev = _dev()
    ds = (_toy if data == "toy" else _synthetic)(tmp_path, negative_size=k)
    a = sampler_arrays(ds)
    sampler = DeviceAnchorSampler(ds, dev, seed=9)
    n, bs = len(ds), (16 if data == "toy" else 512)
    hptr = a["ptr"].copy()
    pool = set(a["pool"].tolist())
    for epoch in range(3):
        order = list(range(n))
        random.Random(epoch).shuffle(order)
        order_dev = sampler.upload_order(order)
        for start in range(0, n, bs):
            Q = min(bs, n - start)
            repeated = (start // bs + epoch) % 2 == 1
            packed = sampler.launch(order_dev, start, Q, epoch, repeated)
            want = host_draw(a, order, start, Q, epoch, 9, ptr=hptr, repeated_queries=repeated)
            _check_batch(packed, want, Q, k, repeated)
            anchors = want["anchors"].reshape(Q, 1 + k)
            for i in range(Q):
                q = ds.node_list[order[start + i]]
                assert all(x in pool and x not in ds.node2masks[q] for x in anchors[i, 1:].tolist())
    assert sampler.padded() == 0
    assert np.array_equal(sampler.pointers(), hptr)


def test_device_positives_follow_the_host_sampler_walk(tmp_path):
    """over three epoch orders the device positives are the host sample_anchors positives, and the device pointers end where the
    host dict ends"""
    from taxoexpan_amd.sampler import DeviceAnchorSampler
    dev = _dev()
    ds_dev, ds_host = _toy(tmp_path), _toy(tmp_path)
    sampler = DeviceAnchorSampler(ds_dev, dev, seed=1)
    n, k = len(ds_dev), 7
    for epoch in range(3):
        order = list(range(n))
        random.Random(10 + epoch).shuffle(order)
        packed = sampler.launch(sampler.upload_order(order), 0, n, epoch, repeated_queries=False)
        got = packed[:n * (1 + k)].cpu().numpy().reshape(n, 1 + k)[:, 0]
        _q, anchor, label, _e = ds_host.sample_anchors(order)
        assert got.tolist() == anchor[label == 1].tolist()
    ptr = sampler.pointers()
    assert all(ptr[v] == c for v, c in ds_host.node2positive_pointer.items())
    assert all(c == 0 for c in ds_dev.node2positive_pointer.values())       # device sampling leaves the host dict alone


def test_negative_draws_are_uniform_over_the_unmasked_pool(tmp_path):
    """one query, 6,000 negative slots in one launch: the accepted draws cover the query's unmasked pool uniformly (chi-square at a
    fixed seed -- deterministic, not a flaky statistical test)"""
    from scipy import stats
    from taxoexpan_amd.sampler import DeviceAnchorSampler, sampler_arrays
    dev = _dev()
    k = 6000
    ds = _toy(tmp_path, negative_size=k)
    a = sampler_arrays(ds)
    i = max(range(len(ds)), key=lambda j: len(ds.node2masks[ds.node_list[j]]))        # the most masked query: a pool with holes
    q = ds.node_list[i]
    allowed = sorted(set(a["pool"].tolist()) - ds.node2masks[q])
    assert 20 <= len(allowed) < len(a["pool"])
    sampler = DeviceAnchorSampler(ds, dev, seed=2024)
    packed = sampler.launch(sampler.upload_order([i]), 0, 1, 0, repeated_queries=True)
    neg = packed[1:1 + k].cpu().numpy()
    counts = np.array([np.count_nonzero(neg == v) for v in allowed])
    assert counts.sum() == k and sampler.padded() == 0
    chi2 = float(((counts - k / len(allowed)) ** 2 / (k / len(allowed))).sum())
    assert stats.chi2.sf(chi2, len(allowed) - 1) > 1e-3, chi2


def test_per_query_anchors_do_not_depend_on_the_batch_size(tmp_path):
    from taxoexpan_amd.sampler import DeviceAnchorSampler
    dev = _dev()
    ds = _toy(tmp_path)
    n, k = len(ds), 7
    order = list(range(n))
    random.Random(4).shuffle(order)
    per = []
    for bs in (16, 5):
        sampler = DeviceAnchorSampler(ds, dev, seed=6)          # both start from the dataset's pointers (device sampling leaves them)
        order_dev = sampler.upload_order(order)
        per.append(np.concatenate([sampler.launch(order_dev, s, min(bs, n - s), 1, False)[:min(bs, n - s) * (1 + k)].cpu().numpy()
                                   for s in range(0, n, bs)]))
    assert np.array_equal(per[0], per[1])


@pytest.mark.parametrize("repeated", [True, False])
def test_device_sampled_loader_equals_the_inline_builder_on_its_anchors(tmp_path, repeated):
    """every DeviceBatchLoader(sampler="device") batch of an epoch (the last one short) equals build_device_batch on the anchors host_draw
    gives for it -- ids, pos, both CSR views, node features, query features (RepeatedRows or stacked), labels -- with the caller's stream
    kept busy while next() builds"""
    from taxoexpan_amd import ops
    from taxoexpan_amd.data_loaders import DeviceBatchLoader, build_device_batch
    from taxoexpan_amd.sampler import host_draw, sampler_arrays
    dev = _dev()
    ds = _toy(tmp_path)
    a = sampler_arrays(ds)
    n, k, bs = len(ds), 7, 16
    loader = DeviceBatchLoader(ds, bs, dev, shuffle=True, seed=3, repeated_queries=repeated, sampler="device")
    model = _model(dev, 8).eval()
    busy = torch.randn(2048, 2048, device=dev)
    host = lambda t: t.cpu().numpy().copy()
    got = []
    for g, x, qf, labels in loader:
        busy = (busy @ busy) * 1e-3                                 # the caller's stream has work queued while next() builds
        pos = g.ndata["pos"]                                        # (the model takes it out of ndata)
        with torch.no_grad():
            pred = model(g, x, qf)
        csr = g.csr(dev)
        assert isinstance(qf, ops.RepeatedRows) == repeated
        got.append(dict(ids=host(g.ndata["_id"]), pos=host(pos), x=host(x), labels=host(labels), pred=host(pred),
                        qrows=host(qf.rows) if repeated else None, qoff=host(qf.run_off) if repeated else None, qf=host(ops.dense_rows(qf)),
                        csr=[host(t) for t in (csr.rowptr_in, csr.col_src, csr.eid_in, csr.rowptr_out, csr.col_dst, csr.pos_out, csr.graph_off)]))
    assert len(got) == len(loader) == -(-n // bs)
    order = list(range(n))
    random.Random(3).shuffle(order)
    hptr = a["ptr"].copy()
    for b, want in enumerate(got):
        Q = min(bs, n - b * bs)
        d = host_draw(a, order, b * bs, Q, 0, 3, ptr=hptr)
        ref = build_device_batch(loader.dtax, d["anchors"], d["exclude"], d["query"], loader.features, expand_factor=ds.expand_factor,
                                 seed=3 + 7919 + b, repeated_queries=repeated)
        g = ref["g"]
        csr = g.csr(dev)
        assert np.array_equal(host(g.ndata["_id"]), want["ids"]) and np.array_equal(host(ref["pos"]), want["pos"])
        for t, w in zip((csr.rowptr_in, csr.col_src, csr.eid_in, csr.rowptr_out, csr.col_dst, csr.pos_out, csr.graph_off), want["csr"]):
            assert np.array_equal(host(t), w)
        assert np.array_equal(host(ref["x"]), want["x"]) and np.array_equal(host(ops.dense_rows(ref["qf"])), want["qf"])
        if repeated:
            assert np.array_equal(host(ref["qf"].rows), want["qrows"]) and np.array_equal(host(ref["qf"].run_off), want["qoff"])
        assert want["labels"].dtype == np.int64 and want["labels"].tolist() == ([1] + [0] * k) * Q
        with torch.no_grad():
            np.testing.assert_array_equal(host(model(g, ref["x"], ref["qf"])), want["pred"])
        assert np.isfinite(want["pred"]).all()


def test_a_query_whose_mask_covers_the_pool_is_padded_with_valid_anchors(tmp_path):
    """root r -> q -> c1..c8: q's mask is every node, so its negatives can only be padded (dataset.py:370-375); the anchors stay valid node
    ids, the count says how many slots were padded (what host_draw counts), and the batch builds and runs a forward pass"""
    from taxoexpan_amd import synthetic as syn
    from taxoexpan_amd.data_loaders import DeviceBatchLoader
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    from taxoexpan_amd.sampler import host_draw, sampler_arrays
    dev = _dev()
    n, k = 10, 5
    edges = [(0, 1)] + [(1, c) for c in range(2, n)]
    feats = np.random.RandomState(0).randn(n, 8).astype(np.float32)
    syn.write_raw(str(tmp_path), "hand", edges, feats)
    ds = MaskedGraphDataset(MAGDataset("hand", str(tmp_path), raw=True), mode="train", sampling_mode=1, negative_size=k, expand_factor=4)
    assert len(ds) == n - 1 and set(ds.node2masks[1]) == set(range(n)) == ds.all_positions
    loader = DeviceBatchLoader(ds, 4, dev, shuffle=True, seed=5, sampler="device")
    model = _model(dev, 8).eval()
    for g, x, qf, labels in loader:
        ids = g.ndata["_id"].cpu().numpy()
        assert ids.min() >= 0 and ids.max() < n
        with torch.no_grad():
            pred = model(g, x, qf)
        assert pred.shape[0] == labels.shape[0] and torch.isfinite(pred).all()
    order = list(range(len(ds)))
    random.Random(5).shuffle(order)
    want = host_draw(sampler_arrays(ds), order, 0, len(ds), 0, 5)
    assert loader.sampler.padded() == want["n_padded"] == k


def test_training_steps_on_device_sampled_batches_equal_the_inline_built_ones(tmp_path):
    """five Adam + InfoNCE steps of PGAT on DeviceBatchLoader(sampler="device") batches give the losses, bit for bit, of the same steps of a
    twin model on build_device_batch of the same anchors (same dropout seeds), and they are finite"""
    from taxoexpan_amd.data_loaders import DeviceBatchLoader, build_device_batch
    from taxoexpan_amd.loss import info_nce_loss
    from taxoexpan_amd.optim import Adam
    from taxoexpan_amd.sampler import host_draw, sampler_arrays
    dev = _dev()
    ds = _synthetic(tmp_path, negative_size=15)
    a = sampler_arrays(ds)
    bs, k = 32, 15
    loader = DeviceBatchLoader(ds, bs, dev, shuffle=True, seed=3, sampler="device")
    m_a = _model(dev, 16).train()
    m_b = copy.deepcopy(m_a)
    opt_a, opt_b = Adam(m_a.parameters(), lr=1e-2, amsgrad=True), Adam(m_b.parameters(), lr=1e-2, amsgrad=True)
    order = list(range(len(ds)))
    random.Random(3).shuffle(order)
    hptr = a["ptr"].copy()

    def step(model, opt, g, x, qf, s):
        torch.manual_seed(100 + s)                                  # the dropout seeds (ops.new_seed) of both twins
        opt.zero_grad(set_to_none=True)
        loss = info_nce_loss(model(g, x, qf).reshape(bs, 1 + k))
        loss.backward()
        opt.step()
        return float(loss.detach())
    la, lb = [], []
    for s, (g, x, qf, labels) in enumerate(loader):
        if s == 5:
            break
        la.append(step(m_a, opt_a, g, x, qf, s))
        d = host_draw(a, order, s * bs, bs, 0, 3, ptr=hptr)
        ref = build_device_batch(loader.dtax, d["anchors"], d["exclude"], d["query"], loader.features, expand_factor=ds.expand_factor,
                                 seed=3 + 7919 + s, repeated_queries=True)
        lb.append(step(m_b, opt_b, ref["g"], ref["x"], ref["qf"], s))
    assert len(la) == 5 and la == lb and np.isfinite(la).all(), (la, lb)
