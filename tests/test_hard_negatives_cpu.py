"""CPU: hard-negative mining's host side -- the table's numpy restatement (sampler.host_hard_table), the draw's (sampler.host_draw with a
table), the checks of HardNegatives.from_numpy / set_hard_negatives / fit(hard_negatives=...), and the argument checks of
txe_sample_anchors with a txe_sample_hard, which answer before any device work (include/txe.h)."""
import ctypes
import os
import random
import shutil
import types

import numpy as np
import pytest
import torch

from golden_util import GOLDEN_DIR


def _toy(tmp_path, **kw):
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    for fn in os.listdir(os.path.join(GOLDEN_DIR, "toy_taxo")):
        shutil.copy(os.path.join(GOLDEN_DIR, "toy_taxo", fn), tmp_path)
    random.seed(0)
    opts = dict(mode="train", sampling_mode=1, negative_size=7, expand_factor=5, normalize_embed=True)
    opts.update(kw)
    return MaskedGraphDataset(MAGDataset("toy", str(tmp_path), raw=True), **opts)


def _masks(ds):
    """node2masks as candidate rows of the pool, CSR over node_list (what mining hands to select_k)"""
    from taxoexpan_amd.evaluate import _retrieval_masks
    pool = sorted(ds.all_positions)
    return pool, _retrieval_masks(ds, ds.node_list, {a: i for i, a in enumerate(pool)})


def _table(ds, size, seed=0, levels=None):
    """host_hard_table on a seeded random score matrix (levels: that many distinct values only, so that ties abound)"""
    from taxoexpan_amd.sampler import host_hard_table
    pool, (off, idx) = _masks(ds)
    rs = np.random.RandomState(seed)
    S = rs.randn(len(ds.node_list), len(pool)).astype(np.float32) if levels is None else \
        rs.randint(0, levels, (len(ds.node_list), len(pool))).astype(np.float32)
    return S, pool, off, idx, host_hard_table(S, pool, off, idx, size)


def test_host_draw_without_a_table_is_unchanged(tmp_path):
    from taxoexpan_amd.sampler import host_draw, sampler_arrays
    ds = _toy(tmp_path)
    a = sampler_arrays(ds)
    n = len(ds)
    order = list(range(n))
    random.Random(5).shuffle(order)
    for repeated in (False, True):
        p0, p1 = a["ptr"].copy(), a["ptr"].copy()
        old = host_draw(a, order, 3, 40, 2, 11, p0, repeated)
        new = host_draw(a, order, 3, 40, 2, 11, ptr=p1, repeated_queries=repeated, hard=None, hard_slots=0)
        assert old.keys() == new.keys() and np.array_equal(p0, p1)
        assert all(np.array_equal(old[f], new[f]) for f in old)


def test_hard_slots_come_from_the_table_and_the_rest_is_the_pool_draw(tmp_path):
    from taxoexpan_amd.sampler import host_draw, sampler_arrays
    ds = _toy(tmp_path)
    a = sampler_arrays(ds)
    n, k, m = len(ds), a["k"], 3
    _S, _pool, _off, _idx, (hidx, hcnt) = _table(ds, 100)
    assert (hcnt == 100).all()                                           # every query has at least 116 unmasked pool nodes
    order = list(range(n))
    random.Random(5).shuffle(order)
    p0, p1 = a["ptr"].copy(), a["ptr"].copy()
    plain = host_draw(a, order, 0, n, epoch=2, seed=11, ptr=p0)
    whole = host_draw(a, order, 0, n, epoch=2, seed=11, ptr=p1, hard=(hidx, hcnt), hard_slots=m)
    assert np.array_equal(p0, p1) and whole["n_padded"] == plain["n_padded"] == 0
    assert np.array_equal(whole["exclude"], plain["exclude"]) and np.array_equal(whole["query"], plain["query"])
    got, ref = whole["anchors"].reshape(n, 1 + k), plain["anchors"].reshape(n, 1 + k)
    assert np.array_equal(got[:, 0], ref[:, 0]) and np.array_equal(got[:, 1 + m:], ref[:, 1 + m:])
    for i in range(n):
        q = ds.node_list[order[i]]
        hard = got[i, 1:1 + m].tolist()
        assert len(set(hard)) == m and set(hard) <= set(hidx[order[i]].tolist()) and ds.node2masks[q].isdisjoint(hard)
        at = hidx[order[i]].tolist().index(hard[0])                      # consecutive entries of the row from the rotation on
        assert hard == [int(hidx[order[i], (at + j) % 100]) for j in range(m)]
    assert not np.array_equal(got[:, 1:1 + m], ref[:, 1:1 + m])
    for bs in (16, 5):                                                   # batches of any size draw what the whole epoch draws
        ptr = a["ptr"].copy()
        parts = [host_draw(a, order, s, min(bs, n - s), epoch=2, seed=11, ptr=ptr, hard=(hidx, hcnt), hard_slots=m)["anchors"]
                 for s in range(0, n, bs)]
        assert np.array_equal(np.concatenate(parts), whole["anchors"])
    other = host_draw(a, order, 0, n, epoch=3, seed=11, hard=(hidx, hcnt), hard_slots=m)["anchors"].reshape(n, 1 + k)
    assert not np.array_equal(other[:, 1], got[:, 1])                    # another epoch, another rotation
    reps = host_draw(a, order, 0, n, epoch=2, seed=11, repeated_queries=True, hard=(hidx, hcnt), hard_slots=m)
    assert np.array_equal(reps["anchors"], whole["anchors"]) and reps["offsets"].tolist() == list(range(0, n * (1 + k) + 1, 1 + k))
    for bad in (-1, k + 1):
        with pytest.raises(ValueError):
            host_draw(a, order, 0, n, epoch=2, seed=11, hard=(hidx, hcnt), hard_slots=bad)


def test_short_rows_give_as_many_hard_slots_as_they_hold(tmp_path):
    from taxoexpan_amd.sampler import host_draw, sampler_arrays
    ds = _toy(tmp_path)
    a = sampler_arrays(ds)
    n, k = len(ds), a["k"]
    _S, _pool, _off, _idx, (full, _cnt) = _table(ds, 6)
    hidx, hcnt = np.full((n, 6), -1, dtype=np.int32), np.zeros(n, dtype=np.int32)
    hidx[1::2, :2], hcnt[1::2] = full[1::2, :2], 2                       # even rows empty, odd rows two entries
    order = list(range(n))
    random.Random(8).shuffle(order)
    plain = host_draw(a, order, 0, n, epoch=1, seed=4)["anchors"].reshape(n, 1 + k)
    got = host_draw(a, order, 0, n, epoch=1, seed=4, hard=(hidx, hcnt), hard_slots=5)["anchors"].reshape(n, 1 + k)
    for i in range(n):
        if order[i] % 2 == 0:
            assert np.array_equal(got[i], plain[i])
        else:
            assert sorted(got[i, 1:3].tolist()) == sorted(hidx[order[i], :2].tolist()) and np.array_equal(got[i, 3:], plain[i, 3:])
    # an entry the query masks, a negative one inside the count and one above every pool id: those slots take the pool route
    i0 = order[0]
    q0 = ds.node_list[i0]
    bad = np.full((n, 6), -1, dtype=np.int32)
    bad[i0, :3] = [sorted(ds.node2masks[q0])[0], -1, int(a["pool"][-1]) + 1]
    cnt = np.zeros(n, dtype=np.int32)
    cnt[i0] = 3
    got = host_draw(a, order, 0, n, epoch=1, seed=4, hard=(bad, cnt), hard_slots=3)
    assert np.array_equal(got["anchors"].reshape(n, 1 + k), plain) and got["n_padded"] == 0


def test_host_hard_table_orders_masks_and_counts(tmp_path):
    from taxoexpan_amd.sampler import host_hard_table
    ds = _toy(tmp_path)
    S, pool, off, idx, (hidx, hcnt) = _table(ds, 128, seed=3, levels=5)  # five distinct scores: ties everywhere
    n = len(ds.node_list)
    assert hidx.shape == (n, 128) and hidx.dtype == np.int32 and hcnt.dtype == np.int32 and len(pool) == 134
    col = {a: i for i, a in enumerate(pool)}
    short = 0
    for i, q in enumerate(ds.node_list):
        unmasked = [a for a in pool if a not in ds.node2masks[q]]
        assert 116 <= len(unmasked) <= 129
        c = int(hcnt[i])
        assert c == min(128, len(unmasked)) and (hidx[i, c:] == -1).all() and (hidx[i, :c] >= 0).all()
        short += c < 128
        row = hidx[i, :c].tolist()
        assert len(set(row)) == c and ds.node2masks[q].isdisjoint(row) and set(row) <= set(pool)
        key = [(-float(S[i, col[a]]), col[a]) for a in row]
        assert key == sorted(key)                                        # best first, equal scores by ascending candidate row
        assert key == sorted((-float(S[i, col[a]]), col[a]) for a in unmasked)[:c]
    assert short > 0
    for size in (0, len(pool) + 1, 1.5):
        with pytest.raises(ValueError):
            host_hard_table(S, pool, off, idx, size)


def test_from_numpy_refuses_malformed_tables(tmp_path):
    from taxoexpan_amd.sampler import HardNegatives
    ds = _toy(tmp_path)
    n = len(ds.node_list)
    _S, pool, _off, _idx, (hidx, hcnt) = _table(ds, 8)
    t = HardNegatives.from_numpy(hidx, ds, "cpu")
    assert t.H == 8 and t.n_queries == n and t.idx.dtype == torch.int32 and t.cnt.dtype == torch.int32
    assert np.array_equal(t.numpy()[0], hidx) and np.array_equal(t.numpy()[1], hcnt)
    tail = hidx.copy()
    tail[0, 5:] = -1
    assert HardNegatives.from_numpy(tail, ds, "cpu").cnt[0].item() == 5
    q0 = ds.node_list[0]
    outside = next(v for v in range(ds.node_features.shape[0]) if v not in ds.all_positions)

    def changed(r, c, v):
        x = hidx.copy()
        x[r, c] = v
        return x
    for bad in (hidx[:-1], hidx[:, :0], hidx.reshape(-1), hidx.astype(np.float32), changed(0, 3, outside), changed(0, 3, -2),
                changed(0, 3, 10 ** 6), changed(0, 3, -1), changed(0, 3, hidx[0, 0]), changed(0, 3, sorted(ds.node2masks[q0] & set(pool))[0])):
        with pytest.raises(ValueError):
            HardNegatives.from_numpy(bad, ds, "cpu")


def _bare_sampler(k=7, n_queries=130):
    """a DeviceAnchorSampler without its device arrays: what set_hard_negatives reads"""
    from taxoexpan_amd.sampler import DeviceAnchorSampler
    s = DeviceAnchorSampler.__new__(DeviceAnchorSampler)
    s.k, s.n_queries, s.n_pool, s.device = k, n_queries, 134, torch.device("cpu")
    return s


def test_set_hard_negatives_refuses_what_it_cannot_use(tmp_path):
    from taxoexpan_amd.data_loaders import DeviceBatchLoader
    from taxoexpan_amd.sampler import DeviceGroupSampler, HardNegatives
    ds = _toy(tmp_path)
    _S, _pool, _off, _idx, (hidx, _cnt) = _table(ds, 8)
    t = HardNegatives.from_numpy(hidx, ds, "cpu")
    s = _bare_sampler()
    s.set_hard_negatives(t, 3)
    assert s.hard is t and s.hard_slots == 3
    s.set_hard_negatives(None, 0)
    assert s.hard is None and s.hard_slots == 0
    short = HardNegatives(t.idx[:-1], t.cnt[:-1])
    for table, slots in ((t, -1), (t, 8), (t, 2.5), (short, 2), ((hidx, _cnt), 2)):
        with pytest.raises(ValueError):
            s.set_hard_negatives(table, slots)
    s.in_epoch = True
    with pytest.raises(RuntimeError):
        s.set_hard_negatives(t, 3)
    assert s.hard is None
    for other in (None, DeviceGroupSampler.__new__(DeviceGroupSampler)):      # the host sampler, the sampling_mode 0 group sampler
        loader = DeviceBatchLoader.__new__(DeviceBatchLoader)
        loader.sampler = other
        with pytest.raises(ValueError):
            loader.set_hard_negatives(t, 3)
    loader = DeviceBatchLoader.__new__(DeviceBatchLoader)
    loader.sampler = _bare_sampler()
    loader.set_hard_negatives(t, 7)
    assert loader.sampler.hard is t and loader.sampler.hard_slots == 7
    with pytest.raises(ValueError):                                          # refused at construction, before any device work
        DeviceBatchLoader(ds, 16, "cpu", sampler="host", hard_negatives=t, hard_slots=3)


def test_fit_checks_the_hard_negative_option_before_any_step():
    from taxoexpan_amd.trainer import fit
    model = torch.nn.Linear(3, 2)
    opt = torch.optim.Adam(model.parameters(), lr=0.5)
    calls = []

    def train_epoch(model, loader, optimizer, loss_fn=None, group_size=None):
        calls.append(1)
        return dict(loss=1.0, n_batches=1, losses=np.ones(1, np.float32), grad_norms=np.ones(1), first_nonfinite=-1)
    run = lambda loader, cfg: fit(model, loader, None, opt, 2, monitor="off", train_epoch_fn=train_epoch, hard_negatives=cfg)
    device_loader = types.SimpleNamespace(sampler=_bare_sampler(), set_hard_negatives=lambda table, slots: None)
    host_loader = types.SimpleNamespace(sampler=None, set_hard_negatives=lambda table, slots: None)
    good = dict(size=8, slots=2)
    for loader, cfg in ((host_loader, good), ([None], good), (device_loader, dict(size=8, slots=8)), (device_loader, dict(size=2, slots=3)),
                        (device_loader, dict(size=0, slots=0)), (device_loader, dict(size=135, slots=2)), (device_loader, dict(size=8)),
                        (device_loader, dict(size=8, slots=2, every=0)), (device_loader, dict(size=8, slots=2, start=0)),
                        (device_loader, dict(size=8, slots=2, when=1)), (device_loader, (8, 2))):
        with pytest.raises(ValueError):
            run(loader, cfg)
    assert not calls
    assert len(run([None], None)) == 2 and len(calls) == 2                   # None: today's behaviour, on any loader


def test_hard_entry_point_checks_its_arguments_without_a_gpu():
    from taxoexpan_amd import _lib
    lib = _lib.load()
    assert "txe_sample_anchors" in _lib.SIGNATURES and "txe_sample_anchors_hard" not in _lib.SIGNATURES
    assert all(issubclass(getattr(_lib, n), ctypes.Structure) for n in ("SampleSource", "SampleSpan", "SampleHard", "SampleNear"))
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(order=p, n_order=4, start=0, Q=2, node_list=p, par_ptr=p, par_idx=p, n_par_idx=9, mask_ptr=p, mask_idx=p, pool=p, n_pool=3,
                pos_ptr=p, k=2, seed=0, epoch=0, repeated=1, packed=p, n_padded=p, hard_idx=p, hard_cnt=p, H=4, hard_slots=1)
    src_f, span_f = [f for f, _ in _lib.SampleSource._fields_], [f for f, _ in _lib.SampleSpan._fields_]
    assert len(src_f) + len(span_f) + 7 == len(good)

    def call(**kw):                                                          # the table form: a txe_sample_hard, no txe_sample_near
        v = dict(good, **kw)
        src, span = _lib.SampleSource(**{f: v[f] for f in src_f}), _lib.SampleSpan(**{f: v[f] for f in span_f})
        hard = _lib.SampleHard(idx=v["hard_idx"], cnt=v["hard_cnt"], H=v["H"], slots=v["hard_slots"])
        return lib.txe_sample_anchors(_lib.ref(src), _lib.ref(span), v["pos_ptr"], v["packed"], v["n_padded"], _lib.ref(hard), None, None)
    for name in ("order", "node_list", "par_ptr", "par_idx", "mask_ptr", "mask_idx", "pool", "pos_ptr", "packed", "n_padded", "hard_idx",
                 "hard_cnt"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(H=0), dict(H=-2), dict(hard_slots=-1), dict(hard_slots=3),
                dict(k=0), dict(k=-3), dict(k=1 << 14), dict(Q=-1), dict(n_pool=0), dict(start=-1), dict(start=3), dict(n_order=1),
                dict(epoch=-1), dict(epoch=1 << 20), dict(Q=(1 << 24) + 1, n_order=1 << 25), dict(Q=1 << 20, n_order=1 << 20, k=1 << 11),
                dict(n_par_idx=-1)):
        assert call(**bad) == -1, bad
    assert call(Q=0) == 0 and call(Q=0, hard_slots=2) == 0                   # nothing to launch
