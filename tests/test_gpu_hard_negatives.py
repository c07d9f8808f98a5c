"""GPU: hard-negative mining -- txe_sample_anchors' table instantiation against sampler.host_draw bit for bit, mine_hard_negatives against
sampler.host_hard_table on the model's own score matrix, the loader's and fit's use of the table."""
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


def _model(dev, match, readout="WMR"):
    """PGAT with the small_* golden dimensions on the toy's 8 features, seeded"""
    from taxoexpan_amd import TaxoExpan
    torch.manual_seed(0)
    return TaxoExpan("PGAT", readout, match, in_dim=8, hidden_dim=8, out_dim=7, pos_dim=5, num_layers=1, heads=[4, 1], feat_drop=0.0,
                     attn_drop=0.0, hidden_drop=0.0, out_drop=0.0).to(dev)


def _masks(ds):
    from taxoexpan_amd.evaluate import _retrieval_masks
    pool = sorted(ds.all_positions)
    return pool, _retrieval_masks(ds, ds.node_list, {a: i for i, a in enumerate(pool)})


def _random_table(ds, H, seed):
    """host_hard_table on seeded random scores, then rows i % 5 == 0 emptied and rows i % 5 == 1 cut to at most two entries"""
    from taxoexpan_amd.sampler import host_hard_table
    pool, (off, idx) = _masks(ds)
    S = np.random.RandomState(seed).randn(len(ds.node_list), len(pool)).astype(np.float32)
    hidx, hcnt = host_hard_table(S, pool, off, idx, H)
    hidx[0::5], hcnt[0::5] = -1, 0
    hidx[1::5, 2:], hcnt[1::5] = -1, np.minimum(hcnt[1::5], 2)
    return hidx, hcnt


def _unpack(packed, Q, k, repeated):
    B = Q * (1 + k)
    p = packed.cpu().numpy()
    out = dict(anchors=p[:B], exclude=p[B:2 * B])
    if repeated:
        out.update(runs=p[2 * B:2 * B + Q], offsets=p[3 * B:3 * B + Q + 1])
    else:
        out["query"] = p[2 * B:3 * B]
    return out


@pytest.mark.parametrize("k", [3, 70])
def test_hard_draw_is_bit_equal_to_host_draw(tmp_path, k):
    """every packed array and n_padded equal sampler.host_draw for hard_slots in {0, 1, k}, H in {1, 5, 64, 100}, both layouts, over the two
    batches of an epoch (the pointers advance), with empty rows and rows shorter than hard_slots (k = 70: the lane loop's second pass,
    hard slots in it for H = 100).  A twin sampler without a table runs the same launches: its output is the hard sampler's for
    hard_slots = 0, and its slots j >= hard_slots are the hard sampler's always."""
    from taxoexpan_amd.sampler import DeviceAnchorSampler, HardNegatives, host_draw, sampler_arrays
    dev = _dev()
    ds = _toy(tmp_path, negative_size=k)
    a = sampler_arrays(ds)
    n = len(ds)
    sampler, plain = DeviceAnchorSampler(ds, dev, seed=9), DeviceAnchorSampler(ds, dev, seed=9)
    hptr = a["ptr"].copy()
    n_padded = 0
    epoch = 0
    for H in (1, 5, 64, 100):
        hidx, hcnt = _random_table(ds, H, seed=H)
        table = HardNegatives(torch.from_numpy(hidx).to(dev), torch.from_numpy(hcnt).to(dev))
        for slots in (0, 1, k):
            for repeated in (True, False):
                sampler.set_hard_negatives(table, slots)
                order = list(range(n))
                random.Random(epoch).shuffle(order)
                order_dev = sampler.upload_order(order)
                for start, Q in ((0, 65), (65, n - 65)):
                    got = _unpack(sampler.launch(order_dev, start, Q, epoch, repeated), Q, k, repeated)
                    ref = _unpack(plain.launch(order_dev, start, Q, epoch, repeated), Q, k, repeated)
                    want = host_draw(a, order, start, Q, epoch, 9, ptr=hptr, repeated_queries=repeated, hard=(hidx, hcnt), hard_slots=slots)
                    n_padded += want["n_padded"]
                    for f in got:
                        assert np.array_equal(got[f], want[f]), (H, slots, repeated, start, f)
                    g2, r2 = got["anchors"].reshape(Q, 1 + k), ref["anchors"].reshape(Q, 1 + k)
                    assert np.array_equal(g2[:, 0], r2[:, 0]) and np.array_equal(g2[:, 1 + slots:], r2[:, 1 + slots:])
                    assert all(np.array_equal(got[f], ref[f]) for f in got if f != "anchors")
                    if slots == 0:
                        assert np.array_equal(g2, r2)
                    else:
                        rows = np.asarray(order)[start:start + Q]
                        m = np.minimum(slots, hcnt[rows])
                        for i in np.flatnonzero(m > 0):
                            assert set(g2[i, 1:1 + m[i]].tolist()) <= set(hidx[rows[i], :hcnt[rows[i]]].tolist())
                epoch += 1
    assert sampler.padded() == plain.padded() == n_padded
    assert np.array_equal(sampler.pointers(), hptr) and np.array_equal(plain.pointers(), hptr)


def test_a_masked_or_invalid_table_entry_takes_the_pool_route(tmp_path):
    """a table that names a node the query masks, a negative id inside the count, an id above every pool node and a count above the row
    width -- handed to the entry point without from_numpy's checks: those slots draw from the pool, as host_draw says, and no anchor is
    masked or outside the pool"""
    from taxoexpan_amd.sampler import DeviceAnchorSampler, HardNegatives, host_draw, sampler_arrays
    dev = _dev()
    ds = _toy(tmp_path)
    a = sampler_arrays(ds)
    n, k = len(ds), 7
    hidx, hcnt = _random_table(ds, 5, seed=1)
    for i in range(2, n, 5):                                             # (rows the helper left full)
        hidx[i, i % 5] = sorted(ds.node2masks[ds.node_list[i]])[0]
    hidx[3::5, 1] = -1
    hidx[4::5, 0] = int(a["pool"][-1]) + 1
    hcnt[3::5] = 9                                                       # above H = 5: read as 5
    sampler, plain = DeviceAnchorSampler(ds, dev, seed=2), DeviceAnchorSampler(ds, dev, seed=2)
    sampler.set_hard_negatives(HardNegatives(torch.from_numpy(hidx).to(dev), torch.from_numpy(hcnt).to(dev)), 5)
    order = list(range(n))
    random.Random(1).shuffle(order)
    order_dev = sampler.upload_order(order)
    got = _unpack(sampler.launch(order_dev, 0, n, 4, False), n, k, False)
    ref = _unpack(plain.launch(order_dev, 0, n, 4, False), n, k, False)
    want = host_draw(a, order, 0, n, 4, 2, hard=(hidx, hcnt), hard_slots=5)
    assert all(np.array_equal(got[f], want[f]) for f in got)
    g2, r2 = got["anchors"].reshape(n, 1 + k), ref["anchors"].reshape(n, 1 + k)
    pool = set(a["pool"].tolist())
    refused = 0
    for i in range(n):
        row, q = order[i], ds.node_list[order[i]]
        assert all(x in pool and x not in ds.node2masks[q] for x in g2[i, 1:].tolist())
        bad = {int(e) for e in hidx[row] if hcnt[row] and (e not in pool or e in ds.node2masks[q])}
        assert bad.isdisjoint(g2[i, 1:6].tolist())
        if bad:                                                          # the refused entry's slot is the twin's pool draw
            refused += 1
            assert sum(g2[i, 1 + j] == r2[i, 1 + j] for j in range(5)) >= len(bad)
    assert refused >= 3 * (n // 5) and np.array_equal(g2[:, 6:], r2[:, 6:]) and sampler.padded() == want["n_padded"] == 0


@pytest.mark.parametrize("match,readout", [("BIM", "WMR"), ("MLP", "CR")])
def test_mined_table_equals_the_host_table_of_the_models_scores(tmp_path, match, readout):
    """mine_hard_negatives(size=16) = host_hard_table on scoring.score_all's matrix for the same hg and queries (both select among the
    same fp32 values: the ids are equal exactly); every table score is >= every unmasked score outside the row; blocks of 48 queries and
    smaller-is-better give the corresponding tables; the model's mode is restored"""
    from taxoexpan_amd import scoring
    from taxoexpan_amd.sampler import _mining_inputs, host_hard_table, mine_hard_negatives
    dev = _dev()
    ds = _toy(tmp_path)
    model = _model(dev, match, readout).train()
    m = _mining_inputs(model, ds, dev)
    assert model.training
    with torch.no_grad():
        S = scoring.score_all(model.match, m["hg"], m["qf"]).cpu().numpy()
    pool, (off, idx) = _masks(ds)
    assert m["pool"].tolist() == pool and S.shape == (len(ds.node_list), len(pool)) and np.isfinite(S).all()
    want_idx, want_cnt = host_hard_table(S, pool, off, idx, 16)
    t = mine_hard_negatives(model, ds, dev, 16)
    assert model.training
    got_idx, got_cnt = t.numpy()
    assert got_idx.dtype == np.int32 and np.array_equal(got_idx, want_idx) and np.array_equal(got_cnt, want_cnt) and (got_cnt == 16).all()
    col = {a: i for i, a in enumerate(pool)}
    for i, q in enumerate(ds.node_list):
        inside = [col[a] for a in got_idx[i]]
        outside = [c for a, c in col.items() if a not in ds.node2masks[q] and c not in set(inside)]
        assert ds.node2masks[q].isdisjoint(got_idx[i].tolist()) and S[i, inside].min() >= S[i, outside].max()
    model.eval()
    blocks = mine_hard_negatives(model, ds, dev, 16, qblock=48)
    assert not model.training and np.array_equal(blocks.numpy()[0], want_idx)
    low = mine_hard_negatives(model, ds, dev, 16, larger_is_better=False)
    assert np.array_equal(low.numpy()[0], host_hard_table(-S, pool, off, idx, 16)[0])
    for size in (0, len(pool) + 1):
        with pytest.raises(ValueError):
            mine_hard_negatives(model, ds, dev, size)


def test_loader_draws_from_the_table(tmp_path):
    """DeviceBatchLoader(sampler="device", hard_negatives=t, hard_slots=3): the anchors of every batch are host_draw's (read off the
    egonets' centre nodes through the in-line builder), forward and backward are finite, set_hard_negatives raises inside an epoch and
    works after it"""
    from taxoexpan_amd.data_loaders import DeviceBatchLoader, build_device_batch
    from taxoexpan_amd.loss import info_nce_loss
    from taxoexpan_amd.sampler import HardNegatives, host_draw, host_hard_table, sampler_arrays
    dev = _dev()
    ds = _toy(tmp_path)
    a = sampler_arrays(ds)
    n, k, bs = len(ds), 7, 16
    pool, (off, idx) = _masks(ds)
    hidx, hcnt = host_hard_table(np.random.RandomState(3).randn(n, len(pool)).astype(np.float32), pool, off, idx, 12)
    t = HardNegatives.from_numpy(hidx, ds, dev)
    loader = DeviceBatchLoader(ds, bs, dev, shuffle=True, seed=3, sampler="device", hard_negatives=t, hard_slots=3)
    model = _model(dev, "BIM").train()
    order = list(range(n))
    random.Random(3).shuffle(order)
    hptr = a["ptr"].copy()
    host = lambda x: x.cpu().numpy()
    for b, (g, x, qf, labels) in enumerate(loader):
        if b == 1:
            with pytest.raises(RuntimeError):
                loader.set_hard_negatives(None, 0)
        Q = min(bs, n - b * bs)
        d = host_draw(a, order, b * bs, Q, 0, 3, ptr=hptr, hard=(hidx, hcnt), hard_slots=3)
        ref = build_device_batch(loader.dtax, d["anchors"], d["exclude"], d["query"], loader.features, expand_factor=ds.expand_factor,
                                 seed=3 + 7919 + b, repeated_queries=True)
        assert np.array_equal(host(g.ndata["_id"]), host(ref["g"].ndata["_id"])) and np.array_equal(host(x), host(ref["x"]))
        assert np.array_equal(host(g.csr(dev).graph_off), host(ref["g"].csr(dev).graph_off))
        hard = d["anchors"].reshape(Q, 1 + k)[:, 1:4]
        assert all(set(hard[i].tolist()) <= set(hidx[order[b * bs + i]].tolist()) for i in range(Q))
        model.zero_grad()
        loss = info_nce_loss(model(g, x, qf).reshape(Q, 1 + k))
        loss.backward()
        assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    assert b == len(loader) - 1 and loader.sampler.padded() == 0
    loader.set_hard_negatives(None, 0)
    assert loader.sampler.hard is None
    for bad in (-1, k + 1):
        with pytest.raises(ValueError):
            loader.set_hard_negatives(t, bad)
    with pytest.raises(ValueError):
        DeviceBatchLoader(_toy(tmp_path, mode="validation", sampling_mode=0), bs, dev, sampler="device").set_hard_negatives(t, 3)


class _Recording:
    """a loader that hands its batches on and keeps every batch's node ids"""

    def __init__(self, loader):
        self.loader, self.ids = loader, []
        self.dataset, self.sampler, self.device, self.dtax = loader.dataset, loader.sampler, loader.device, loader.dtax
        self.set_hard_negatives = loader.set_hard_negatives

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            self.ids.append(batch[0].ndata["_id"].cpu().numpy().copy())
            yield batch


def test_fit_mines_on_schedule(tmp_path):
    """fit(epochs=3, hard_negatives=dict(size=8, slots=2, every=2, start=2)): finite losses, hard_mined on epoch 2 alone, epoch 1's
    batches and losses those of a run without the option, epochs 2 and 3 other batches, nothing padded"""
    from taxoexpan_amd.data_loaders import DeviceBatchLoader
    from taxoexpan_amd.optim import Adam
    from taxoexpan_amd.trainer import fit
    dev = _dev()
    runs = []
    for cfg in (None, dict(size=8, slots=2, every=2, start=2)):
        loader = _Recording(DeviceBatchLoader(_toy(tmp_path), 16, dev, shuffle=True, seed=5, sampler="device"))
        model = _model(dev, "BIM")
        opt = Adam(model.parameters(), lr=1e-2, amsgrad=True)
        logs = fit(model, loader, None, opt, 3, monitor="off", hard_negatives=cfg)
        assert len(logs) == 3 and all(np.isfinite(l["losses"]).all() and l["first_nonfinite"] == -1 for l in logs)
        assert loader.sampler.padded() == 0
        runs.append((logs, loader.ids))
    (plain_logs, plain_ids), (logs, ids) = runs
    assert all("hard_mined" not in l and "hard_mean_count" not in l for l in plain_logs)
    assert [l.get("hard_mined", False) for l in logs] == [False, True, False] and logs[1]["hard_mean_count"] == 8.0
    assert set(logs[0]) == set(plain_logs[0]) and set(logs[1]) == set(plain_logs[1]) | {"hard_mined", "hard_mean_count"}
    nb = len(ids) // 3
    assert nb == 9 and len(plain_ids) == len(ids)
    assert all(np.array_equal(x, y) for x, y in zip(ids[:nb], plain_ids[:nb]))
    assert logs[0]["losses"].tobytes() == plain_logs[0]["losses"].tobytes()
    for e in (1, 2):                                                     # epoch 2 mined; epoch 3 keeps its table
        assert not all(np.array_equal(x, y) for x, y in zip(ids[e * nb:(e + 1) * nb], plain_ids[e * nb:(e + 1) * nb]))
