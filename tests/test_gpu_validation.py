"""GPU: the sampling_mode 0 device sampler (txe_sample_groups) against sampler.host_draw_groups bit for bit, its negatives' distribution,
DeviceBatchLoader(sampler="device") on a validation dataset against the in-line builder, the device obtain_ranks against the reference
fixture and the numpy restatement, and evaluate.validate against trainer.py:96-124 restated on the host."""
import random

import numpy as np
import pytest
import torch

from test_validation_cpu import METRICS, _cases, _synthetic, _toy, check_group_draw, check_metrics

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _read(out):
    """a DeviceGroupSampler.launch result as the host arrays of host_draw_groups"""
    B = int(out["total"].item())
    p = out["packed"].cpu().numpy()
    return B, p, out["labels"][:B].cpu().numpy()


@pytest.mark.parametrize("data,k", [("toy", 7), ("toy", 70), ("synthetic", 7), ("synthetic", 70), ("synthetic", 256)])
def test_device_group_draw_is_bit_equal_to_host_draw_groups(tmp_path, data, k):
    from taxoexpan_amd.sampler import DeviceGroupSampler, group_sampler_arrays, host_draw_groups
    dev = _dev()
    ds = (_toy if data == "toy" else _synthetic)(tmp_path, negative_size=k)
    a = group_sampler_arrays(ds)
    sampler = DeviceGroupSampler(ds, dev, seed=9)
    n = len(ds)
    for bs in (16, 512):
        for epoch in range(3):
            order = list(range(n))
            random.Random(epoch).shuffle(order)
            order_dev = sampler.upload_order(order)
            whole = {f: [] for f in ("anchors", "exclude", "query", "label")}
            for start in range(0, n, bs):
                Q = min(bs, n - start)
                repeated = (start // bs + epoch) % 2 == 1
                B, p, lab = _read(sampler.launch(order_dev, start, Q, epoch, repeated))
                want = host_draw_groups(a, order, start, Q, epoch, 9, repeated_queries=repeated)
                assert B == len(want["anchors"])
                assert np.array_equal(p[:B], want["anchors"]) and np.array_equal(p[B:2 * B], want["exclude"])
                assert lab.dtype == np.int64 and np.array_equal(lab, want["label"])
                if repeated:
                    assert np.array_equal(p[2 * B:2 * B + Q], want["runs"]) and np.array_equal(p[3 * B:3 * B + Q + 1], want["offsets"])
                else:
                    assert np.array_equal(p[2 * B:3 * B], want["query"])
                for f in whole:
                    whole[f].append(want[f])
            check_group_draw(ds, a, order, dict({f: np.concatenate(v) for f, v in whole.items()}, n_padded=0))
    assert sampler.padded() == 0


def test_group_negatives_are_uniform_over_the_unmasked_pool(tmp_path):
    """the most masked toy query, k = 6,000 slots in one launch: the survivors cover its unmasked pool uniformly (chi-square at a fixed
    seed), and their count is within 4 binomial sigma of k (1 - f_q), f_q = the masked share of the pool"""
    from scipy import stats
    from taxoexpan_amd.sampler import DeviceGroupSampler, group_sampler_arrays
    dev = _dev()
    k = 6000
    ds = _toy(tmp_path, negative_size=k)
    a = group_sampler_arrays(ds)
    i = max(range(len(ds)), key=lambda j: len(ds.node2masks[ds.node_list[j]] & ds.all_positions))
    q = ds.node_list[i]
    pool = a["pool"].tolist()
    allowed = sorted(set(pool) - ds.node2masks[q])
    f_q = 1.0 - len(allowed) / len(pool)
    assert f_q > 0 and len(allowed) >= 20
    sampler = DeviceGroupSampler(ds, dev, seed=2024)
    B, p, lab = _read(sampler.launch(sampler.upload_order([i]), 0, 1, 0, repeated_queries=True))
    neg = p[:B][lab == 0]
    mean, sd = k * (1 - f_q), (k * f_q * (1 - f_q)) ** 0.5
    assert abs(len(neg) - mean) <= 4 * sd, (len(neg), mean, sd)
    counts = np.array([np.count_nonzero(neg == v) for v in allowed])
    assert counts.sum() == len(neg) and sampler.padded() == 0
    e = len(neg) / len(allowed)
    chi2 = float(((counts - e) ** 2 / e).sum())
    assert stats.chi2.sf(chi2, len(allowed) - 1) > 1e-3, chi2


def _model(dev, in_dim, match="LBM"):
    from taxoexpan_amd import TaxoExpan
    torch.manual_seed(0)
    return TaxoExpan("PGAT", "WMR", match, in_dim=in_dim, hidden_dim=16, out_dim=16, pos_dim=4, num_layers=1, heads=[2, 1], feat_drop=0.1,
                     attn_drop=0.1, hidden_drop=0.1, out_drop=0.1).to(dev)


@pytest.mark.parametrize("repeated", [True, False])
def test_device_group_loader_equals_the_inline_builder_on_its_anchors(tmp_path, repeated):
    """every DeviceBatchLoader(sampler="device") batch of a validation epoch equals build_device_batch on host_draw_groups' anchors:
    graph arrays, x, qf.dense() and labels, with the caller's stream kept busy while next() builds"""
    from taxoexpan_amd import ops
    from taxoexpan_amd.data_loaders import DeviceBatchLoader, build_device_batch
    from taxoexpan_amd.sampler import group_sampler_arrays, host_draw_groups
    dev = _dev()
    ds = _toy(tmp_path)
    a = group_sampler_arrays(ds)
    n, bs = len(ds), 16
    loader = DeviceBatchLoader(ds, bs, dev, shuffle=True, seed=3, repeated_queries=repeated, sampler="device")
    busy = torch.randn(2048, 2048, device=dev)
    host = lambda t: t.cpu().numpy().copy()
    got = []
    for _epoch in range(2):
        for g, x, qf, labels in loader:
            busy = (busy @ busy) * 1e-3
            csr = g.csr(dev)
            assert isinstance(qf, ops.RepeatedRows) == repeated
            got.append(dict(ids=host(g.ndata["_id"]), pos=host(g.ndata["pos"]), x=host(x), labels=host(labels), qf=host(ops.dense_rows(qf)),
                            csr=[host(t) for t in (csr.rowptr_in, csr.col_src, csr.eid_in, csr.rowptr_out, csr.col_dst, csr.pos_out, csr.graph_off)]))
    nb = -(-n // bs)
    assert len(got) == 2 * nb == 2 * len(loader)
    for j, want in enumerate(got):
        epoch, b = divmod(j, nb)
        order = list(range(n))
        random.Random(3 + epoch).shuffle(order)
        Q = min(bs, n - b * bs)
        d = host_draw_groups(a, order, b * bs, Q, epoch, 3)
        ref = build_device_batch(loader.dtax, d["anchors"], d["exclude"], d["query"], loader.features, expand_factor=ds.expand_factor,
                                 seed=3 + 7919 * (epoch + 1) + b, repeated_queries=repeated)
        g = ref["g"]
        csr = g.csr(dev)
        assert np.array_equal(host(g.ndata["_id"]), want["ids"]) and np.array_equal(host(ref["pos"]), want["pos"])
        for t, w in zip((csr.rowptr_in, csr.col_src, csr.eid_in, csr.rowptr_out, csr.col_dst, csr.pos_out, csr.graph_off), want["csr"]):
            assert np.array_equal(host(t), w)
        assert np.array_equal(host(ref["x"]), want["x"]) and np.array_equal(host(ops.dense_rows(ref["qf"])), want["qf"])
        assert want["labels"].dtype == np.int64 and np.array_equal(want["labels"], d["label"])


def test_device_obtain_ranks_equals_the_reference_fixture():
    from taxoexpan_amd import metric
    dev = _dev()
    for c in _cases():
        gr = metric.obtain_ranks(torch.from_numpy(c["score"]).to(dev)[:, None], torch.from_numpy(c["label"]).to(dev), mode=int(c["mode"]))
        assert gr.ranks.is_cuda and gr.ranks.cpu().tolist() == c["ranks"].tolist() and gr.pos_off.cpu().tolist() == c["pos_off"].tolist()
        check_metrics(gr, c["metrics"])


def _fuzz(rng, B, dtype):
    """a labelled batch of B entries: groups of 1-8 positives and 0-400 negatives (a few long ones), ties, NaN, +-Inf, a leading negative run"""
    labels = [np.zeros(rng.randint(0, 5), dtype=dtype)]
    n = len(labels[0])
    while n < B:
        p = rng.randint(1, 9)
        m = rng.randint(0, 401) if rng.rand() > 0.01 else rng.randint(1000, 20000)
        labels += [np.ones(p, dtype=dtype), np.zeros(m, dtype=dtype)]
        n += p + m
    label = np.concatenate(labels)[:B]
    score = np.round(rng.randn(B) * 4).astype(np.float32) / np.float32(4)
    m = rng.rand(B)
    score[m < 0.01] = np.nan
    score[(m >= 0.01) & (m < 0.015)] = np.inf
    score[(m >= 0.015) & (m < 0.02)] = -np.inf
    return score, label


def test_device_obtain_ranks_equals_the_restatement_on_a_fuzz():
    from taxoexpan_amd import metric
    dev = _dev()
    rng = np.random.RandomState(7)
    for i, B in enumerate((2, 3, 64, 65, 1000, 4097, 100_003, 1 << 20)):
        for mode in (0, 1):
            dtype = np.int32 if (i + mode) % 2 else np.int64
            score, label = _fuzz(rng, B, dtype)
            r, off = metric._host_group_ranks(score, label, mode)
            s = torch.from_numpy(score).to(dev)
            gr = metric.obtain_ranks(s if i % 2 else s[:, None], torch.from_numpy(label).to(dev), mode=mode)
            assert np.array_equal(gr.ranks.cpu().numpy(), r) and np.array_equal(gr.pos_off.cpu().numpy(), off), (B, mode)


def test_device_obtain_ranks_on_one_group_of_355808():
    """test_fast.py:133/211's pre_metric(energy_scores, labels) at MAG-Full's candidate count: three positives, one group"""
    from taxoexpan_amd import metric
    dev = _dev()
    B = 355_808
    rng = np.random.RandomState(11)
    score = rng.randn(B).astype(np.float32)
    label = np.zeros(B, dtype=np.int64)
    label[:3] = 1
    for mode in (0, 1):
        r, off = metric._host_group_ranks(score, label, mode)
        gr = metric.obtain_ranks(torch.from_numpy(score).to(dev), torch.from_numpy(label).to(dev), mode=mode)
        assert gr.pos_off.cpu().tolist() == [0, 3] and np.array_equal(gr.ranks.cpu().numpy(), r)


class _Replay:
    """an epoch of batches kept for several passes: the model takes 'pos' out of g.ndata (model.py:58), so each pass puts it back"""

    def __init__(self, loader):
        self.batches = [(g, x, qf, lab, g.ndata["pos"]) for g, x, qf, lab in loader]

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for g, x, qf, lab, pos in self.batches:
            g.ndata["pos"] = pos
            yield g, x, qf, lab


def _host_valid_epoch(model, batches, metrics, mode):
    """trainer.py:96-124 restated on the host: the batch's model outputs, numpy ranks, the reference-formula metrics, the mean over batches"""
    from taxoexpan_amd import metric
    model.eval()
    total = np.zeros(len(metrics))
    ranks = []
    with torch.no_grad():
        for g, h, qf, label in batches:
            pred = model(g, h, qf)
            gr = metric.obtain_ranks(pred.cpu(), label.cpu(), mode=mode)
            ranks.append(gr)
            total += np.array([getattr(metric, m)(gr) for m in metrics])
    return (total / len(batches)).tolist(), ranks


@pytest.mark.parametrize("sampler,match", [("device", "LBM"), ("device", "BIM"), ("device", "MLP"), ("host", "LBM"), ("host", "MLP")])
def test_validate_equals_the_trainer_loop_on_the_host(tmp_path, sampler, match):
    from taxoexpan_amd import metric
    from taxoexpan_amd.data_loaders import DeviceBatchLoader
    from taxoexpan_amd.evaluate import validate
    dev = _dev()
    ds = _synthetic(tmp_path, negative_size=32)
    loader = DeviceBatchLoader(ds, 64, dev, shuffle=True, seed=1, sampler=sampler)
    batches = _Replay(loader)                                       # one epoch, kept: both sides see the same batches
    model = _model(dev, 16, match).train()
    got = validate(model, batches, metrics=METRICS, larger_is_better=True)
    assert model.training
    want, ranks = _host_valid_epoch(model, batches, METRICS, 1)
    model.train()
    assert got["n_batches"] == len(batches) == len(loader)
    assert got["n_groups"] == sum(int(r.pos_off.numel()) - 1 for r in ranks) == len(ds)
    assert got["n_positives"] == sum(int(r.ranks.numel()) for r in ranks)
    with torch.no_grad():                                           # the device ranks of each batch are the host's
        model.eval()
        for (g, x, qf, lab), r in zip(batches, ranks):
            gr = metric.obtain_ranks(model(g, x, qf), lab, mode=1)
            assert torch.equal(gr.ranks.cpu(), r.ranks) and torch.equal(gr.pos_off.cpu().long(), r.pos_off.long())
        model.train()
    for name, a, b in zip(METRICS, got["val_metrics"], want):
        assert np.isnan(a) == np.isnan(b), (name, a, b)
        if name in ("micro_mr", "hit_at_1", "hit_at_3", "hit_at_5"):
            # per batch bit-equal; the mean over batches is one fp64 sum in batch order on both sides
            assert a == b, (name, a, b)
        else:
            assert abs(a - b) <= 1e-12 * abs(b), (name, a, b)
    model.eval()
    assert validate(model, batches, metrics=("hit_at_1",), larger_is_better=False)["n_batches"] == len(batches)
    assert not model.training
