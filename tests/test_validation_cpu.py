"""CPU: metric.obtain_ranks on CPU tensors and the metric functions on its GroupedRanks against the reference's model/metric.py
(tests/golden/obtain_ranks.npz, tools/gen_validation_golden.py), the sampling_mode 0 restatement sampler.host_draw_groups, and the
argument checks of the new classes and C entry points, which answer before any device work."""
import ctypes
import os
import random
import shutil

import numpy as np
import pytest
import torch

from golden_util import GOLDEN_DIR

METRICS = ("macro_mr", "micro_mr", "hit_at_1", "hit_at_3", "hit_at_5", "mrr_scaled_10", "combined_metrics")
EXACT = {"micro_mr", "hit_at_1", "hit_at_3", "hit_at_5"}          # integer sums in fp64: bit-equal


def _cases():
    z = np.load(os.path.join(GOLDEN_DIR, "obtain_ranks.npz"))
    return [{f: z[f"{c}:{f}"] for f in ("score", "label", "mode", "ranks", "pos_off", "metrics")} for c in range(int(z["n_cases"]))]


def check_metrics(gr, want):
    """each metric of metric.py on a GroupedRanks vs the reference's value: bit-equal for micro_mr / hit_at_k, 1e-12 relative otherwise,
    NaN exactly where the reference gives NaN"""
    from taxoexpan_amd import metric
    for name, w in zip(METRICS, want):
        got = getattr(metric, name)(gr)
        assert np.isnan(got) == np.isnan(w), (name, got, w)
        if np.isnan(w):
            continue
        if name in EXACT:
            assert got == w, (name, got, w)
        else:
            assert abs(got - w) <= 1e-12 * abs(w), (name, got, w)


def test_fixture_covers_what_it_claims():
    cases = _cases()
    assert 25 <= len(cases) <= 40
    assert {c["label"].dtype for c in cases} == {np.dtype(np.int32), np.dtype(np.int64)} and {int(c["mode"]) for c in cases} == {0, 1}
    assert any(len(c["label"]) == 2 for c in cases) and any(c["label"][0] == 0 for c in cases)
    assert any(np.isnan(c["score"]).any() for c in cases) and any(np.isinf(c["score"]).any() for c in cases)
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "obtain_ranks.npz")) < 256 * 1024


@pytest.mark.parametrize("shape", ["flat", "column"])
def test_obtain_ranks_on_cpu_tensors_equals_the_reference(shape):
    from taxoexpan_amd import metric
    for c in _cases():
        s = torch.from_numpy(c["score"])
        gr = metric.obtain_ranks(s[:, None] if shape == "column" else s, torch.from_numpy(c["label"]), mode=int(c["mode"]))
        assert isinstance(gr, metric.GroupedRanks)
        assert gr.ranks.dtype == torch.int32
        assert gr.pos_off.tolist() == c["pos_off"].tolist() and gr.ranks.tolist() == c["ranks"].tolist()
        check_metrics(gr, c["metrics"])
        assert metric.as_rank_lists(gr) == metric.as_rank_lists(gr.ranks, gr.pos_off)
        # the (ranks, pos_off) calls are unchanged
        assert metric.hit_at_3(gr.ranks, gr.pos_off) == metric.hit_at_3(gr)


def test_obtain_ranks_refuses_what_it_does_not_rank():
    from taxoexpan_amd import metric
    s, lab = torch.zeros(4), torch.tensor([1, 0, 1, 0])
    for bad in ((s.double(), lab), (s[:, None].repeat(1, 2), lab), (s, lab.float()), (s, lab[:3])):
        with pytest.raises(ValueError):
            metric.obtain_ranks(*bad)
    with pytest.raises(ValueError):
        metric.obtain_ranks(s, lab, mode=2)
    gr = metric.obtain_ranks(torch.tensor([1.0, 2.0]), torch.tensor([1, 1]), mode=0)      # positives without negatives: rank 1
    assert gr.ranks.tolist() == [1, 1] and gr.pos_off.tolist() == [0, 2]


# ---- sampling_mode 0 restatement ---------------------------------------------------------------------------------------------------

def _toy(tmp_path, **kw):
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    d = tmp_path / "toy"
    d.mkdir(exist_ok=True)
    for fn in os.listdir(os.path.join(GOLDEN_DIR, "toy_taxo")):
        shutil.copy(os.path.join(GOLDEN_DIR, "toy_taxo", fn), d)
    random.seed(0)
    opts = dict(mode="validation", sampling_mode=0, negative_size=7, expand_factor=5, normalize_embed=True)
    opts.update(kw)
    return MaskedGraphDataset(MAGDataset("toy", str(d), raw=True), **opts)


def _synthetic(tmp_path, **kw):
    """the 3,000-node synthetic taxonomy of tests/test_gpu_device_sampler.py, in validation mode"""
    from taxoexpan_amd import synthetic as syn
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    d = tmp_path / "syn"
    d.mkdir(exist_ok=True)
    tax = syn.make_taxonomy(3000, 4500, 16, seed=3)
    syn.write_raw(str(d), "syn", syn.taxonomy_edges(tax), tax.features.numpy())
    random.seed(0)
    opts = dict(mode="validation", sampling_mode=0, negative_size=7, expand_factor=20)
    opts.update(kw)
    return MaskedGraphDataset(MAGDataset("syn", str(d), raw=True), **opts)


def check_group_draw(ds, arrays, order, d, repeated=False):
    """the layout of one host_draw_groups / device batch over all of `order`: per query its parents (exclude q, label 1), then 1 .. k
    unmasked pool nodes (exclude -1, label 0); offsets and labels consistent"""
    k = arrays["k"]
    pool = set(arrays["pool"].tolist())
    assert d["n_padded"] == 0
    assert len(d["anchors"]) == len(d["exclude"]) == len(d["query"]) == len(d["label"])
    o = 0
    offsets = [0]
    for idx in order:
        q = ds.node_list[idx]
        par = list(ds.node2parents[q])
        n = len(par)
        assert d["anchors"][o:o + n].tolist() == par and (d["exclude"][o:o + n] == q).all() and (d["label"][o:o + n] == 1).all()
        e = o + n
        while e < len(d["label"]) and d["label"][e] == 0 and d["query"][e] == q:
            e += 1
        neg = d["anchors"][o + n:e].tolist()
        assert 1 <= len(neg) <= k
        assert all(x in pool and x not in ds.node2masks[q] for x in neg)
        assert (d["exclude"][o + n:e] == -1).all() and (d["query"][o:e] == q).all()
        o = e
        offsets.append(o)
    assert o == len(d["anchors"])
    if repeated:
        assert d["offsets"].tolist() == offsets and d["runs"].tolist() == [ds.node_list[i] for i in order]


@pytest.mark.parametrize("data,k", [("toy", 7), ("toy", 70), ("synthetic", 7), ("synthetic", 70), ("synthetic", 256)])
def test_host_draw_groups_layout_and_batch_independence(tmp_path, data, k):
    from taxoexpan_amd.sampler import group_sampler_arrays, host_draw_groups
    ds = (_toy if data == "toy" else _synthetic)(tmp_path, negative_size=k)
    a = group_sampler_arrays(ds)
    n = len(ds)
    order = list(range(n))
    random.Random(5).shuffle(order)
    whole = host_draw_groups(a, order, 0, n, epoch=2, seed=11, repeated_queries=True)
    check_group_draw(ds, a, order, whole, repeated=True)
    for bs in (16, 5):                                        # batches of any size draw what the whole epoch draws
        parts = [host_draw_groups(a, order, s, min(bs, n - s), epoch=2, seed=11) for s in range(0, n, bs)]
        for f in ("anchors", "exclude", "query", "label"):
            assert np.array_equal(np.concatenate([p[f] for p in parts]), whole[f]), f
        assert sum(p["n_padded"] for p in parts) == 0
    other = host_draw_groups(a, order, 0, n, epoch=3, seed=11)
    assert not np.array_equal(other["anchors"], whole["anchors"]) or len(other["anchors"]) != len(whole["anchors"])


def test_group_sampler_refuses_what_it_does_not_implement(tmp_path):
    from taxoexpan_amd.sampler import DeviceAnchorSampler, DeviceGroupSampler, group_sampler_arrays, sampler_arrays
    for kw in (dict(sampling_mode=1), dict(negative_size=0), dict(mode="test")):
        ds = _toy(tmp_path, **kw)
        for make in (group_sampler_arrays, lambda d: DeviceGroupSampler(d, "cpu")):
            with pytest.raises(ValueError):
                make(ds)
    ds = _toy(tmp_path)
    for make in (sampler_arrays, lambda d: DeviceAnchorSampler(d, "cpu")):       # mode 1 sampler keeps refusing mode 0
        with pytest.raises(ValueError):
            make(ds)


def test_new_entry_points_check_their_arguments_without_a_gpu():
    from taxoexpan_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(order=p, n_order=4, start=0, Q=2, node_list=p, par_ptr=p, par_idx=p, n_par_idx=9, mask_ptr=p, mask_idx=p, pool=p, n_pool=3,
                k=2, seed=0, epoch=0, repeated=1, cap=8, packed=p, labels=p, total=p, ws=p, n_padded=p)
    src_f, span_f = [f for f, _ in _lib.SampleSource._fields_], [f for f, _ in _lib.SampleSpan._fields_]
    assert len(src_f) + len(span_f) + 6 == len(good)

    def call(**kw):                                              # txe_sample_anchors' two structs, then the plain arguments
        v = dict(good, **kw)
        src, span = _lib.SampleSource(**{f: v[f] for f in src_f}), _lib.SampleSpan(**{f: v[f] for f in span_f})
        return lib.txe_sample_groups(_lib.ref(src), _lib.ref(span), v["cap"], v["packed"], v["labels"], v["total"], v["ws"], v["n_padded"], None)
    for name in ("order", "node_list", "par_ptr", "par_idx", "mask_ptr", "mask_idx", "pool", "packed", "labels", "total", "ws", "n_padded"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(k=0), dict(k=1 << 14), dict(Q=-1), dict(n_pool=0), dict(start=-1), dict(start=3), dict(n_order=1), dict(epoch=-1),
                dict(epoch=1 << 20), dict(Q=(1 << 24) + 1, n_order=1 << 25, cap=1 << 25), dict(cap=1), dict(cap=1 << 29), dict(n_par_idx=-1)):
        assert call(**bad) == -1, bad
    assert call(Q=0) == 0
    assert lib.txe_sample_groups(None, None, 8, p, p, p, p, p, None) == -1                  # NULL structs
    ws = lib.txe_group_rank_ws_bytes(1000)
    assert ws > 1000 * 20 and lib.txe_group_rank_ws_bytes(0) == 0
    good = dict(score=p, labels=p, label_bytes=4, B=1000, mode=1, ranks=p, pos_off=p, counts=p, ws=p, ws_bytes=ws, stream=None)
    call = lambda **kw: lib.txe_group_rank(*dict(good, **kw).values())
    for name in ("score", "labels", "ranks", "pos_off", "counts", "ws"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(B=0), dict(B=-5), dict(label_bytes=2), dict(mode=2), dict(mode=-1)):
        assert call(**bad) == -1, bad
    assert call(ws_bytes=ws - 1) == -3
    good = dict(ranks=p, pos_off=p, counts=p, which=0x10, n_which=2, acc=p, stream=None)
    call = lambda **kw: lib.txe_group_metrics(*dict(good, **kw).values())
    for name in ("ranks", "pos_off", "counts", "acc"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(n_which=0), dict(n_which=17), dict(which=0x7), dict(which=0x70)):
        assert call(**bad) == -1, bad


def test_validate_refuses_unknown_metrics():
    from taxoexpan_amd.evaluate import validate
    model = torch.nn.Linear(2, 1)
    for bad in ((), ("macro_mr", "nope"), ("hit_at_1",) * 17):
        with pytest.raises(ValueError):
            validate(model, [], metrics=bad)
