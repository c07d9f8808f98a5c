"""CPU: the device anchor sampler's inputs (sampler.sampler_arrays), its numpy restatement (sampler.host_draw) and the argument checks of
txe_sample_anchors, which answer before any device work (include/txe.h)."""
import ctypes
import os
import random
import shutil

import numpy as np
import pytest

from golden_util import GOLDEN_DIR


def _toy(tmp_path, **kw):
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    for fn in os.listdir(os.path.join(GOLDEN_DIR, "toy_taxo")):
        shutil.copy(os.path.join(GOLDEN_DIR, "toy_taxo", fn), tmp_path)
    random.seed(0)
    opts = dict(mode="train", sampling_mode=1, negative_size=7, expand_factor=5, normalize_embed=True)
    opts.update(kw)
    return MaskedGraphDataset(MAGDataset("toy", str(tmp_path), raw=True), **opts)


def test_sampler_arrays_restate_the_dataset(tmp_path):
    from taxoexpan_amd.sampler import sampler_arrays
    ds = _toy(tmp_path)
    a = sampler_arrays(ds)
    assert a["k"] == 7
    assert all(v.dtype == np.int32 for name, v in a.items() if name != "k")
    assert a["node_list"].tolist() == list(ds.node_list)
    n = ds.node_features.shape[0]
    assert len(a["par_ptr"]) == len(a["mask_ptr"]) == n + 1 and len(a["ptr"]) == n
    for v in range(n):
        assert a["par_idx"][a["par_ptr"][v]:a["par_ptr"][v + 1]].tolist() == list(ds.node2parents.get(v, []))
        assert a["mask_idx"][a["mask_ptr"][v]:a["mask_ptr"][v + 1]].tolist() == sorted(ds.node2masks.get(v, []))
        assert a["ptr"][v] == ds.node2positive_pointer.get(v, 0)
    assert a["pool"].tolist() == sorted(ds.all_positions)


def test_sampler_refuses_what_it_does_not_implement(tmp_path):
    from taxoexpan_amd.sampler import DeviceAnchorSampler, sampler_arrays
    for kw in (dict(sampling_mode=0), dict(negative_size=0), dict(mode="test", sampling_mode=0)):
        ds = _toy(tmp_path, **kw)
        for make in (sampler_arrays, lambda d: DeviceAnchorSampler(d, "cpu")):
            with pytest.raises(ValueError):
                make(ds)
    ds = _toy(tmp_path)
    ds.mode = "test"                         # (MaskedGraphDataset itself refuses mode 'test' with sampling_mode 1)
    with pytest.raises(ValueError):
        DeviceAnchorSampler(ds, "cpu")


def test_host_draw_negatives_are_unmasked_deterministic_and_independent_of_batching(tmp_path):
    from taxoexpan_amd.sampler import host_draw, sampler_arrays
    ds = _toy(tmp_path)
    a = sampler_arrays(ds)
    n, k = len(ds), a["k"]
    order = list(range(n))
    random.Random(5).shuffle(order)
    whole = host_draw(a, order, 0, n, epoch=2, seed=11)
    assert whole["n_padded"] == 0 and len(whole["anchors"]) == n * (1 + k)
    anchors = whole["anchors"].reshape(n, 1 + k)
    query = whole["query"].reshape(n, 1 + k)
    pool = set(a["pool"].tolist())
    for i in range(n):
        q = ds.node_list[order[i]]
        assert (query[i] == q).all()
        assert anchors[i, 0] == ds.node2parents[q][ds.node2positive_pointer[q]]
        assert whole["exclude"][i * (1 + k)] == q and (whole["exclude"].reshape(n, 1 + k)[i, 1:] == -1).all()
        for x in anchors[i, 1:]:
            assert x in pool and x not in ds.node2masks[q]
    again = host_draw(a, order, 0, n, epoch=2, seed=11)
    assert all(np.array_equal(whole[f], again[f]) for f in ("anchors", "exclude", "query"))
    for bs in (16, 5):                                        # batches of any size draw what the whole epoch draws
        ptr = a["ptr"].copy()
        parts = [host_draw(a, order, s, min(bs, n - s), epoch=2, seed=11, ptr=ptr)["anchors"] for s in range(0, n, bs)]
        assert np.array_equal(np.concatenate(parts), whole["anchors"])
    other = host_draw(a, order, 0, n, epoch=3, seed=11)["anchors"].reshape(n, 1 + k)
    assert not np.array_equal(other[:, 1:], anchors[:, 1:])    # another epoch, other negatives
    reps = host_draw(a, order, 0, n, epoch=2, seed=11, repeated_queries=True)
    assert reps["runs"].tolist() == [ds.node_list[i] for i in order] and reps["offsets"].tolist() == list(range(0, n * (1 + k) + 1, 1 + k))


def test_host_draw_advances_the_pointers_like_the_host_sampler(tmp_path):
    from taxoexpan_amd.sampler import host_draw, sampler_arrays
    ds = _toy(tmp_path)
    a = sampler_arrays(ds)
    n = len(ds)
    ptr = a["ptr"].copy()
    for epoch in range(3):
        order = list(range(n))
        random.Random(epoch).shuffle(order)
        got = host_draw(a, order, 0, n, epoch, seed=1, ptr=ptr)["anchors"].reshape(n, -1)[:, 0]
        _q, anchor, label, _e = ds.sample_anchors(order)
        assert got.tolist() == anchor[label == 1].tolist()
    assert all(ptr[v] == c for v, c in ds.node2positive_pointer.items())


def test_sample_anchors_entry_point_checks_its_arguments_without_a_gpu():
    from taxoexpan_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert "txe_sample_anchors" in _lib.SIGNATURES and not [n for n in _lib.SIGNATURES if n.startswith("txe_sample_anchors_")]
    assert all(issubclass(getattr(_lib, n), ctypes.Structure) for n in ("SampleSource", "SampleSpan", "SampleHard", "SampleNear"))
    good = dict(order=p, n_order=4, start=0, Q=2, node_list=p, par_ptr=p, par_idx=p, n_par_idx=9, mask_ptr=p, mask_idx=p, pool=p, n_pool=3,
                pos_ptr=p, k=2, seed=0, epoch=0, repeated=1, packed=p, n_padded=p)
    src_f, span_f = [f for f, _ in _lib.SampleSource._fields_], [f for f, _ in _lib.SampleSpan._fields_]
    assert set(src_f) | set(span_f) | {"pos_ptr", "packed", "n_padded"} == set(good)

    def call(**kw):                                              # every value addressed to the field (or plain argument) that carries it
        v = dict(good, **kw)
        src, span = _lib.SampleSource(**{f: v[f] for f in src_f}), _lib.SampleSpan(**{f: v[f] for f in span_f})
        return lib.txe_sample_anchors(_lib.ref(src), _lib.ref(span), v["pos_ptr"], v["packed"], v["n_padded"], None, None, None)
    for name in ("order", "node_list", "par_ptr", "par_idx", "mask_ptr", "mask_idx", "pool", "pos_ptr", "packed", "n_padded"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(k=0), dict(k=-3), dict(k=1 << 14), dict(Q=-1), dict(n_pool=0), dict(start=-1), dict(start=3), dict(n_order=1),
                dict(epoch=-1), dict(epoch=1 << 20), dict(Q=(1 << 24) + 1, n_order=1 << 25), dict(Q=1 << 20, n_order=1 << 20, k=1 << 11),
                dict(n_par_idx=-1)):
        assert call(**bad) == -1, bad
    assert call(Q=0) == 0                                        # nothing to launch
    src, span = _lib.SampleSource(**{f: good[f] for f in src_f}), _lib.SampleSpan(**dict({f: good[f] for f in span_f}, Q=0))
    assert lib.txe_sample_anchors(None, _lib.ref(span), p, p, p, None, None, None) == -1         # a NULL struct
    assert lib.txe_sample_anchors(_lib.ref(src), None, p, p, p, None, None, None) == -1
