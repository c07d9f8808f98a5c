"""GPU: near negatives -- txe_sample_anchors' near instantiation against sampler.host_draw bit for bit, against the pool and table
instantiations where the rule says they agree, on malformed taxonomy arrays, and through DeviceBatchLoader / train_epoch."""
import numpy as np
import pytest
import torch

import near_negative_cases as cases

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _model(dev):
    """PGAT + WMR + LBM with the small_* golden dimensions on the toy's 8 features, seeded"""
    from taxoexpan_amd import TaxoExpan
    torch.manual_seed(0)
    return TaxoExpan("PGAT", "WMR", "LBM", in_dim=8, hidden_dim=8, out_dim=7, pos_dim=5, num_layers=1, heads=[4, 1], feat_drop=0.0,
                     attn_drop=0.0, hidden_drop=0.0, out_drop=0.0).to(dev)


def _unpack(packed, Q, k, repeated):
    B = Q * (1 + k)
    p = packed.cpu().numpy()
    out = dict(anchors=p[:B], exclude=p[B:2 * B])
    if repeated:
        out.update(runs=p[2 * B:2 * B + Q], offsets=p[3 * B:3 * B + Q + 1])
    else:
        out["query"] = p[2 * B:3 * B]
    return out


def _same(x, y, Q, k, repeated):
    """the arrays a launch writes (a packed buffer's unwritten gaps are not compared)"""
    x, y = _unpack(x, Q, k, repeated), _unpack(y, Q, k, repeated)
    return all(np.array_equal(x[f], y[f]) for f in x)


def _random_table(ds, H, seed):
    """a mined-style table (host_hard_table on seeded scores), rows i % 5 == 0 emptied"""
    from taxoexpan_amd.evaluate import _retrieval_masks
    from taxoexpan_amd.sampler import host_hard_table
    pool = sorted(ds.all_positions)
    off, idx = _retrieval_masks(ds, ds.node_list, {a: i for i, a in enumerate(pool)})
    hidx, hcnt = host_hard_table(np.random.RandomState(seed).randn(len(ds.node_list), len(pool)).astype(np.float32), pool, off, idx, H)
    hidx[0::5], hcnt[0::5] = -1, 0
    return hidx, hcnt


def _call_near(sampler, order_dev, start, Q, epoch, repeated, counts, table=None, hard_slots=0, tax=None):
    """txe_sample_anchors with an explicit txe_sample_near -- the near instantiation whatever the counts (DeviceAnchorSampler.launch hands
    one over only with a nonzero count) -- over `tax` = dict of int32 device tensors (par_ptr, par_idx, chd_ptr, chd_idx; default: the
    sampler's resident taxonomy); table None: hard = NULL"""
    from taxoexpan_amd import _lib
    from taxoexpan_amd.sampler import _span
    t = sampler.dtax
    tax = tax or dict(par_ptr=t.par_ptr, par_idx=t.par_idx, chd_ptr=t.chd_ptr, chd_idx=t.chd_idx)
    packed = torch.empty(4 * Q * (1 + sampler.k) + 1, dtype=torch.int32, device=sampler.device)
    hard = _lib.SampleHard(idx=_lib.ptr(table.idx), cnt=_lib.ptr(table.cnt), H=table.H, slots=hard_slots) if table is not None else None
    near = _lib.SampleNear(par_ptr=_lib.ptr(tax["par_ptr"]), par_idx=_lib.ptr(tax["par_idx"]), chd_ptr=_lib.ptr(tax["chd_ptr"]),
                           chd_idx=_lib.ptr(tax["chd_idx"]), n_nodes=int(tax["par_ptr"].numel()) - 1, n_par=int(tax["par_idx"].numel()),
                           n_chd=int(tax["chd_idx"].numel()), n_sib=counts[0], n_gpar=counts[1], n_unc=counts[2], counts=_lib.ptr(sampler._near))
    span = _span(order_dev, start, Q, epoch, sampler.seed, repeated)
    _lib.call("txe_sample_anchors", _lib.ref(sampler._src), _lib.ref(span), _lib.ptr(sampler.arrays["ptr"]), _lib.ptr(packed),
              _lib.ptr(sampler._padded), _lib.ref(hard), _lib.ref(near), _lib.stream_ptr())
    return packed


CASES = {"toy-k7": ("toy", 7, (2, 1, 2), 16), "toy-k70": ("toy", 70, (30, 2, 36), 16), "synthetic-k7": ("synthetic", 7, (2, 1, 2), 512),
         "synthetic-k70": ("synthetic", 70, (30, 2, 36), 512), "toy-one-batch-of-5": ("toy", 7, (2, 1, 2), None),
         "hand": ("hand", 7, (5, 1, 1), 4)}


@pytest.mark.parametrize("case", list(CASES))
def test_near_draw_is_bit_equal_to_host_draw_over_three_epochs(tmp_path, case):
    """anchors, exclude, query ids, run offsets, the pointers, n_padded and n_near equal sampler.host_draw over three epoch orders (the
    layouts alternate).  k = 70 with near = (30, 2, 36): the near slots cross lane 64, the lane loop's second pass.  One batch of 5
    queries: a partly filled workgroup.  The hand taxonomy 0 -> 1 -> {2..9}: every proposal but a sibling is masked."""
    from taxoexpan_amd.sampler import DeviceAnchorSampler, host_draw, near_arrays, sampler_arrays
    data, k, counts, bs = CASES[case]
    dev = _dev()
    ds = {"toy": cases.toy, "synthetic": cases.synthetic}[data](tmp_path, negative_size=k) if data != "hand" else cases.hand(tmp_path, k)
    a, tax, n = sampler_arrays(ds), near_arrays(ds), len(ds)
    sampler = DeviceAnchorSampler(ds, dev, seed=9)
    sampler.set_near_negatives(*counts)
    hptr = a["ptr"].copy()
    n_padded, n_near = 0, [0, 0, 0]
    for epoch in range(3):
        order = cases.shuffled(n, epoch)
        order_dev = sampler.upload_order(order)
        repeated = epoch % 2 == 0
        batches = [(3, 5)] if bs is None else [(s, min(bs, n - s)) for s in range(0, n, bs)]
        got = [sampler.launch(order_dev, s, Q, epoch, repeated) for s, Q in batches]
        for (s, Q), packed in zip(batches, got):
            want = host_draw(a, order, s, Q, epoch, 9, ptr=hptr, repeated_queries=repeated, near=counts, taxonomy=tax)
            n_padded += want["n_padded"]
            n_near = [x + y for x, y in zip(n_near, want["n_near"])]
            for f, v in _unpack(packed, Q, k, repeated).items():
                assert np.array_equal(v, want[f]), (epoch, s, f)
    assert sampler.padded() == n_padded and list(sampler.near_counts()) == n_near
    assert np.array_equal(sampler.pointers(), hptr)
    print(case, "accepted", n_near, "padded", n_padded)
    assert n_near[0] > 0 and (data == "hand" or bs is None or min(n_near) > 0)      # (15 queries may well accept no grandparent)


@pytest.mark.parametrize("k", [7, 70])
def test_zero_counts_give_the_older_entries_bytes(tmp_path, k):
    """all three counts 0 through the near instantiation (an explicit txe_sample_near): the pool instantiation's bytes without a table
    (hard = NULL), and the table instantiation's with a mined-style table and hard_slots = 3; the near counters stay 0"""
    from taxoexpan_amd.sampler import DeviceAnchorSampler, HardNegatives
    dev = _dev()
    ds = cases.toy(tmp_path, negative_size=k)
    n = len(ds)
    hidx, hcnt = _random_table(ds, 6, 1)
    table = HardNegatives(torch.from_numpy(hidx).to(dev), torch.from_numpy(hcnt).to(dev))
    new, old, new_hard, old_hard = (DeviceAnchorSampler(ds, dev, seed=4) for _ in range(4))
    old_hard.set_hard_negatives(table, 3)
    for epoch, repeated in ((0, True), (1, False)):
        order_dev = new.upload_order(cases.shuffled(n, epoch))
        for s, Q in ((0, 65), (65, n - 65)):
            got = _call_near(new, order_dev, s, Q, epoch, repeated, (0, 0, 0))
            assert _same(got, old.launch(order_dev, s, Q, epoch, repeated), Q, k, repeated)
            got = _call_near(new_hard, order_dev, s, Q, epoch, repeated, (0, 0, 0), table, 3)
            assert _same(got, old_hard.launch(order_dev, s, Q, epoch, repeated), Q, k, repeated)
    assert new.near_counts() == new_hard.near_counts() == (0, 0, 0)
    assert new.padded() == old.padded() and new_hard.padded() == old_hard.padded()
    assert np.array_equal(new.pointers(), old.pointers()) and np.array_equal(new_hard.pointers(), old_hard.pointers())


@pytest.mark.parametrize("k", list(cases.LANE_LOOP_PLANS))
def test_every_lane_stays_in_the_slot_loop_through_the_ballots(tmp_path, k):
    """negative_size 1, 64 and 65 (idle lanes beside one slot; one full pass; a second pass with one live lane) through all three
    instantiations -- pool, table, near (cases.LANE_LOOP_PLANS) -- against host_draw over two epochs, each in both layouts, as one batch of
    5 queries (a partly filled workgroup) and one batch of the rest: every array a launch writes, the pointers, padded() and near_counts()"""
    from taxoexpan_amd.sampler import DeviceAnchorSampler, HardNegatives, host_draw, near_arrays, sampler_arrays
    dev = _dev()
    ds = cases.toy(tmp_path, negative_size=k)
    a, tax, n = sampler_arrays(ds), near_arrays(ds), len(ds)
    hidx, hcnt = _random_table(ds, 6, 1)
    table = HardNegatives(torch.from_numpy(hidx).to(dev), torch.from_numpy(hcnt).to(dev))
    for route, kw in cases.lane_loop_routes(k, (hidx, hcnt)).items():
        sampler = DeviceAnchorSampler(ds, dev, seed=5)
        if "hard" in kw:
            sampler.set_hard_negatives(table, kw["hard_slots"])
        if "near" in kw:
            sampler.set_near_negatives(*kw["near"])
        assert (sampler._hard_arg is not None, sampler._near_arg is not None) == ("hard" in kw, "near" in kw)      # the instantiation meant
        hptr = a["ptr"].copy()
        n_padded, n_near = 0, [0, 0, 0]
        for epoch in range(2):
            order = cases.shuffled(n, epoch)
            order_dev = sampler.upload_order(order)
            for repeated in (True, False):
                for s, Q in ((0, 5), (5, n - 5)):
                    got = _unpack(sampler.launch(order_dev, s, Q, epoch, repeated), Q, k, repeated)
                    want = host_draw(a, order, s, Q, epoch, 5, ptr=hptr, repeated_queries=repeated, taxonomy=tax if "near" in kw else None, **kw)
                    n_padded += want["n_padded"]
                    n_near = [x + y for x, y in zip(n_near, want.get("n_near", [0, 0, 0]))]
                    for f, v in got.items():
                        assert np.array_equal(v, want[f]), (route, epoch, repeated, s, f)
        assert sampler.padded() == n_padded and list(sampler.near_counts()) == n_near, route
        assert np.array_equal(sampler.pointers(), hptr), route
        assert (sum(n_near) > 0) == (route == "near")


def test_near_slots_between_the_hard_slots_and_the_pool_slots(tmp_path):
    """a table with hard_slots = 3, near = (2, 1, 1), k = 15: slots [0, 3) are the table launch's, slots at or above 7
    the pool launch's, every array is host_draw's, and two samplers made alike launch equal bytes"""
    from taxoexpan_amd.sampler import DeviceAnchorSampler, HardNegatives, host_draw, near_arrays, sampler_arrays
    dev = _dev()
    k, counts = 15, (2, 1, 1)
    ds = cases.toy(tmp_path, negative_size=k)
    a, tax, n = sampler_arrays(ds), near_arrays(ds), len(ds)
    hidx, hcnt = _random_table(ds, 8, 2)
    table = HardNegatives(torch.from_numpy(hidx).to(dev), torch.from_numpy(hcnt).to(dev))
    near, twin, hard, plain = (DeviceAnchorSampler(ds, dev, seed=6) for _ in range(4))
    for s_ in (near, twin, hard):
        s_.set_hard_negatives(table, 3)
    near.set_near_negatives(*counts)
    twin.set_near_negatives(*counts)
    order = cases.shuffled(n, 7)
    order_dev = near.upload_order(order)
    got = near.launch(order_dev, 0, n, 2, True)
    assert _same(got, twin.launch(order_dev, 0, n, 2, True), n, k, True)   # no float, no order of arrival: equal bytes
    g = _unpack(got, n, k, True)
    want = host_draw(a, order, 0, n, 2, 6, repeated_queries=True, hard=(hidx, hcnt), hard_slots=3, near=counts, taxonomy=tax)
    assert all(np.array_equal(g[f], want[f]) for f in g)
    h = _unpack(hard.launch(order_dev, 0, n, 2, True), n, k, True)
    p = _unpack(plain.launch(order_dev, 0, n, 2, True), n, k, True)
    g2, h2, p2 = (x["anchors"].reshape(n, 1 + k) for x in (g, h, p))
    assert np.array_equal(g2[:, :4], h2[:, :4]) and np.array_equal(g2[:, 8:], p2[:, 8:]) and not np.array_equal(g2[:, 4:8], p2[:, 4:8])
    assert all(np.array_equal(g[f], p[f]) for f in g if f != "anchors")
    assert list(near.near_counts()) == want["n_near"] == list(twin.near_counts()) and near.padded() == want["n_padded"]


@pytest.mark.parametrize("bad", ["child_id_n_nodes", "child_id_negative", "row_end_before_start"])
def test_a_malformed_taxonomy_puts_no_invalid_id_into_a_batch(tmp_path, bad):
    """the child CSR handed to the entry point with every child id = n_nodes, every child id = -1, or descending row pointers (no row
    ends behind its start): ids are compared with their ranges before they address anything, so every anchor is a pool node, every
    sibling and uncle slot is its pool draw (the twin sampler's slot), no such proposal is counted, and the arrays are host_draw's"""
    from taxoexpan_amd.sampler import DeviceAnchorSampler, host_draw, near_arrays, sampler_arrays
    dev = _dev()
    ds = cases.toy(tmp_path)
    a, tax, n, k = sampler_arrays(ds), near_arrays(ds), len(ds), 7
    if bad == "child_id_n_nodes":
        tax["chd_idx"] = np.full_like(tax["chd_idx"], tax["n_nodes"])
    elif bad == "child_id_negative":
        tax["chd_idx"] = np.full_like(tax["chd_idx"], -1)
    else:
        tax["chd_ptr"] = tax["chd_ptr"][::-1].copy()
        assert tax["chd_ptr"].min() >= 0 and tax["chd_ptr"].max() == len(tax["chd_idx"]) and (np.diff(tax["chd_ptr"]) <= 0).all()
    dtax = {f: torch.from_numpy(tax[f]).to(dev) for f in ("par_ptr", "par_idx", "chd_ptr", "chd_idx")}
    sampler, plain = DeviceAnchorSampler(ds, dev, seed=3), DeviceAnchorSampler(ds, dev, seed=3)
    order = cases.shuffled(n, 2)
    order_dev = sampler.upload_order(order)
    g = _unpack(_call_near(sampler, order_dev, 0, n, 1, False, (2, 1, 2), tax=dtax), n, k, False)
    p = _unpack(plain.launch(order_dev, 0, n, 1, False), n, k, False)
    want = host_draw(a, order, 0, n, 1, 3, near=(2, 1, 2), taxonomy=tax)
    assert all(np.array_equal(g[f], want[f]) for f in g)
    g2, p2 = g["anchors"].reshape(n, 1 + k), p["anchors"].reshape(n, 1 + k)
    assert set(g2[:, 1:].ravel().tolist()) <= set(a["pool"].tolist())
    assert np.array_equal(g2[:, :3], p2[:, :3]) and np.array_equal(g2[:, 4:], p2[:, 4:])
    counts = sampler.near_counts()
    assert counts[0] == counts[2] == 0 and counts[1] == want["n_near"][1] > 0 and sampler.padded() == 0


class _Recording:
    """a loader that hands its batches on and keeps every batch's anchors"""

    def __init__(self, loader):
        self.loader, self.anchors = loader, []
        self.dataset, self.sampler, self.device, self.dtax = loader.dataset, loader.sampler, loader.device, loader.dtax
        self.in_batch, self.attach_anchors = loader.in_batch, loader.attach_anchors

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            self.anchors.append(batch[0].anchors.cpu().numpy().copy())
            yield batch


def test_loader_and_train_epoch_with_near_negatives(tmp_path):
    """DeviceBatchLoader(near_negatives=dict(siblings=2, grandparents=1, uncles=2)): two epochs of train_epoch on the toy set with a small
    PGAT + WMR + LBM model -- finite losses, the three shares reported, each in [0, 1] and equal to host_draw's accepted proposals /
    requested slots, every batch's anchors host_draw's.  A loader without the keyword: the anchors of host_draw() without `near`, and no
    new key in the log.  set_near_negatives inside an epoch raises RuntimeError."""
    from taxoexpan_amd.data_loaders import DeviceBatchLoader
    from taxoexpan_amd.optim import Adam
    from taxoexpan_amd.sampler import host_draw, near_arrays, sampler_arrays
    from taxoexpan_amd.trainer import train_epoch
    dev = _dev()
    counts, bs, k = (2, 1, 2), 16, 7
    names = ("near_sibling_share", "near_grandparent_share", "near_uncle_share")
    for near in (dict(siblings=2, grandparents=1, uncles=2), None):
        ds = cases.toy(tmp_path)
        a, tax, n = sampler_arrays(ds), near_arrays(ds), len(ds)
        loader = _Recording(DeviceBatchLoader(ds, bs, dev, shuffle=True, seed=3, sampler="device", attach_anchors=True, near_negatives=near))
        assert loader.sampler.near == (counts if near else (0, 0, 0))
        model = _model(dev)
        opt = Adam(model.parameters(), lr=1e-2)
        hptr = a["ptr"].copy()
        for epoch in range(2):
            loader.anchors = []
            log = train_epoch(model, loader, opt)
            assert log["n_batches"] == len(loader) == 9 and np.isfinite(log["losses"]).all() and log["first_nonfinite"] == -1
            order = cases.shuffled(n, 3 + epoch)
            accepted = [0, 0, 0]
            for b, got in enumerate(loader.anchors):
                Q = min(bs, n - b * bs)
                want = host_draw(a, order, b * bs, Q, epoch, 3, ptr=hptr, near=counts if near else None, taxonomy=tax)
                assert np.array_equal(got.reshape(-1), want["anchors"]), (epoch, b)
                accepted = [x + y for x, y in zip(accepted, want.get("n_near", [0, 0, 0]))]
            if near:
                shares = [log[f] for f in names]
                print("epoch", epoch, "shares", shares)
                assert all(0.0 <= v <= 1.0 for v in shares) and shares == [x / (c * n) for x, c in zip(accepted, counts)]
            else:
                assert not set(names) & set(log)
        assert loader.sampler.padded() == 0
    loader = DeviceBatchLoader(cases.toy(tmp_path), bs, dev, sampler="device", near_negatives=dict(uncles=3))
    for b, _batch in enumerate(loader):
        if b == 1:
            with pytest.raises(RuntimeError):
                loader.set_near_negatives(siblings=1)
    assert loader.sampler.near == (0, 0, 3)
    loader.set_near_negatives()
    assert loader.sampler.near == (0, 0, 0)
    with pytest.raises(ValueError):
        DeviceBatchLoader(cases.toy(tmp_path, mode="validation", sampling_mode=0), bs, dev, sampler="device").set_near_negatives(siblings=1)


@pytest.mark.parametrize("mode", ["in_batch", "taxo_margin"])
def test_near_negatives_compose_with_the_other_losses(tmp_path, mode):
    """one epoch with in_batch=True / taxo_margin=1.0 on near-negative batches: a finite loss, mean_negatives / mean_taxo_distance and the
    shares present (the packed layout those losses read is unchanged)"""
    from taxoexpan_amd.data_loaders import DeviceBatchLoader
    from taxoexpan_amd.optim import Adam
    from taxoexpan_amd.trainer import train_epoch
    dev = _dev()
    kw = dict(in_batch=True) if mode == "in_batch" else dict(attach_anchors=True)
    loader = DeviceBatchLoader(cases.toy(tmp_path), 16, dev, shuffle=True, seed=1, sampler="device",
                               near_negatives=dict(siblings=2, grandparents=1, uncles=2), **kw)
    model = _model(dev)
    log = train_epoch(model, loader, Adam(model.parameters(), lr=1e-2), **(dict(in_batch=True) if mode == "in_batch" else dict(taxo_margin=1.0)))
    assert np.isfinite(log["losses"]).all() and np.isfinite(log["loss"]) and log["first_nonfinite"] == -1
    key = "mean_negatives" if mode == "in_batch" else "mean_taxo_distance"
    assert np.isfinite(log[key]) and log[key] > 0
    assert all(0.0 < log[f] <= 1.0 for f in ("near_sibling_share", "near_grandparent_share", "near_uncle_share"))
