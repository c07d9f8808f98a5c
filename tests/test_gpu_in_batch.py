"""GPU: the in-batch loss -- txe_inbatch_nce (csrc/txe_inbatch.hip) against its float64 restatement on the generated cases of
tests/in_batch_cases.py, repeatability, the reduction to loss.info_nce_loss, ops.InBatchNCEFunction against torch float64 autograd, the
loader's g.in_batch, trainer.train_epoch(in_batch=True) and the C ABI's refusals.

Gates (derived, in the style of tests/test_gpu_pair_losses.py).  Yardstick e = |torch's fp32 cross_entropy on the same rows with -inf in
the masked columns - float64|.  Row loss: |HIP - f64| <= max(2 e_i, (n_valid_i + 16) 2^-24 max(1, |lse_i|, |S[i][pos]|)) -- n_valid
non-negative fp32 terms added in any order are at most n_valid 2^-24 relative off, the logarithm of the sum turns that into an absolute
error, and lse - S[pos] rounds at the size of its operands.  Total: the sum of the row gates.  Gradient, per element: max(2 e, 8 x 2^-24
x max(1, |d_f64|)), times max(1, |S|) under chain_exp.  n_valid and the zeros at masked entries: exact."""
import ctypes
import inspect
import os
import random
import shutil

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import in_batch_cases as cases
from golden_util import GOLDEN_DIR, gate_against_f64

pytestmark = pytest.mark.gpu

EPS = cases.EPS


def _dev():
    return torch.device("cuda:0")


def _up(a, dev):
    """a host array on the device; an empty one (a mask CSR without entries) as one unused element: its pointer must not be NULL"""
    if a is None:
        return None
    return torch.from_numpy(np.array(a) if len(a) else np.zeros(1, dtype=a.dtype)).to(dev)


def _raw(c, dev, chain_exp=0, masked=True, in_place=False, want_counts=True, S=None):
    """one raw txe_inbatch_nce call on a case: dict(rc, loss fp32, d [Q, G] fp32, n_valid, row_loss, total, pad_ok)"""
    from taxoexpan_amd import _lib
    lib = _lib.load()
    Q, G = c["Q"], c["G"]
    S_host = np.array(S if S is not None else (c["S"] if masked else c.get("S_plain", c["S"])))
    ld_s = S_host.shape[1]
    S_dev = _up(S_host, dev)
    ld_d = ld_s if in_place else G + 1
    d = S_dev if in_place else torch.full((Q, ld_d), 7.0, dtype=torch.float32, device=dev)
    t = {k: _up(c[k], dev) for k in ("pos_col", "anchor", "qnode")}
    mp, mi = (_up(c["mask_ptr"], dev), _up(c["mask_idx"], dev)) if masked else (None, None)
    loss = torch.full((1,), -5.0, dtype=torch.float32, device=dev)
    n_valid = torch.full((Q,), -1, dtype=torch.int32, device=dev) if want_counts else None
    total = torch.full((1,), 1000, dtype=torch.int64, device=dev) if want_counts else None
    wsb = lib.txe_inbatch_nce_ws_bytes(Q)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    rc = lib.txe_inbatch_nce(S_dev.data_ptr(), ld_s, Q, G, t["pos_col"].data_ptr(), t["anchor"].data_ptr(), t["qnode"].data_ptr(),
                             _lib.ptr(mp), _lib.ptr(mi), chain_exp, loss.data_ptr(), d.data_ptr(), ld_d, _lib.ptr(n_valid), _lib.ptr(total),
                             ws.data_ptr(), wsb, _lib.stream_ptr())
    torch.cuda.synchronize()
    d_host = d.cpu().numpy()
    pad = d_host[:, G:]
    return dict(rc=rc, loss=loss.cpu().numpy()[0], d=d_host[:, :G].copy(), pad_ok=bool(np.isnan(pad).all() if in_place else (pad == 7.0).all()),
                n_valid=None if n_valid is None else n_valid.cpu().numpy(), total=None if total is None else int(total.item()),
                row_loss=ws[:4 * Q].view(torch.float32).cpu().numpy())


def _check(c, ref, got, chain_exp, S, what):
    """one call against the float64 restatement under the gates of the module docstring"""
    valid = ref["valid"]
    assert got["rc"] == 0 and got["pad_ok"], what
    assert (got["n_valid"] == ref["n_valid"]).all() and got["total"] == 1000 + int(ref["n_valid"].sum()), what
    row_err = np.abs(got["row_loss"].astype(np.float64) - ref["row_loss"])
    tot_err = abs(float(got["loss"]) - ref["loss"])
    with np.errstate(invalid="ignore"):
        mag = np.where(valid, np.maximum(1.0, np.abs(S.astype(np.float64))), 1.0) if chain_exp else 1.0
        want_d = np.where(valid, ref["d"] * S.astype(np.float64), 0.0) if chain_exp else ref["d"]
    d_gate = ref["d_gate"] * mag
    d_err = np.abs(got["d"].astype(np.float64) - want_d)
    print(f"{what}: rows worst {float(np.max(row_err / ref['row_gate'])):.2f} of their gate (yardstick worst {float(ref['e_row'].max()):.2e}); "
          f"total |HIP - f64| = {tot_err:.3e} (gate {float(ref['row_gate'].sum()):.3e}); gradient worst {float(np.max(d_err / d_gate)):.2f} of its gate")
    assert (got["d"][~valid] == 0).all(), what                       # exact zeros, whatever the masked scores hold
    assert np.isfinite(got["loss"]) and np.isfinite(got["d"]).all(), what
    assert (row_err <= ref["row_gate"]).all(), (what, row_err, ref["row_gate"])
    assert tot_err <= ref["row_gate"].sum(), (what, tot_err)
    assert (d_err <= d_gate).all(), (what, float(np.max(d_err / d_gate)))


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("chain_exp", [0, 1])
@pytest.mark.parametrize("name", sorted(cases.SHAPES))
def test_kernel_equals_the_float64_restatement(name, chain_exp, masked):
    c, ref = cases.case(name), cases.reference(name, masked)
    S = (c["S"] if masked else c["S_plain"])[:, :c["G"]]
    got = _raw(c, _dev(), chain_exp, masked)
    _check(c, ref, got, chain_exp, S, f"{name} chain_exp={chain_exp} masked={masked}")
    for i, info in enumerate(c["rows"]):
        if info["all_masked"] and masked:                            # the row's loss is 0 up to rounding, its gradient 0, n_valid 1
            assert got["n_valid"][i] == 1 and (got["d"][i] == 0).all() and abs(got["row_loss"][i]) <= ref["row_gate"][i]


@pytest.mark.parametrize("name", ["3x12", "7x257", "4x1025", "1x65600"])
def test_two_calls_give_the_same_bytes_and_in_place_equals_out_of_place(name):
    c = cases.case(name)
    for chain_exp in (0, 1):
        a, b = _raw(c, _dev(), chain_exp), _raw(c, _dev(), chain_exp)
        assert a["loss"].tobytes() == b["loss"].tobytes() and a["d"].tobytes() == b["d"].tobytes()
        p = _raw(c, _dev(), chain_exp, in_place=True)
        assert p["rc"] == 0 and p["pad_ok"]
        assert p["loss"].tobytes() == a["loss"].tobytes() and p["d"].tobytes() == a["d"].tobytes()
    n = _raw(c, _dev(), 0, want_counts=False)                         # n_valid and valid_total are optional
    assert n["rc"] == 0 and n["loss"].tobytes() == _raw(c, _dev(), 0)["loss"].tobytes()


def test_every_foreign_column_masked_is_info_nce_loss():
    """with every foreign column masked the batch is the grouped InfoNCE: both device losses meet the same float64 value within the gates"""
    from taxoexpan_amd import loss
    from taxoexpan_amd.loss import host_in_batch_nce, host_in_batch_valid
    dev = _dev()
    c = cases.foreign_masked(5, 12)
    Q, k, G = c["Q"], c["k"], c["G"]
    args = (c["pos_col"], c["anchor"], c["qnode"], c["mask_ptr"], c["mask_idx"])
    valid = host_in_batch_valid(*args)
    l64, d64, n_valid = host_in_batch_nce(c["S"], *args)
    own = np.stack([c["S"][i, i * (1 + k):(i + 1) * (1 + k)] for i in range(Q)])
    x32 = torch.from_numpy(own).requires_grad_(True)
    row32 = F.cross_entropy(x32, torch.zeros(Q, dtype=torch.long), reduction="none")
    row32.sum().backward()
    x64 = torch.from_numpy(own).double()
    row64 = F.cross_entropy(x64, torch.zeros(Q, dtype=torch.long), reduction="none").numpy()
    d_own64 = np.stack([d64[i, i * (1 + k):(i + 1) * (1 + k)] for i in range(Q)])
    lse = row64 + own[:, 0]
    gate = np.maximum(2 * np.abs(row32.detach().numpy() - row64), (n_valid + 16) * EPS * np.maximum(1.0, np.maximum(np.abs(lse), np.abs(own[:, 0])))).sum()
    d_gate = np.maximum(2 * np.abs(x32.grad.numpy() - d_own64), 8 * EPS * np.maximum(1.0, np.abs(d_own64)))
    got = _raw(c, dev)
    grouped = torch.from_numpy(own).to(dev).requires_grad_(True)
    ref_loss = loss.info_nce_loss(grouped)
    ref_loss.backward()
    assert (got["n_valid"] == 1 + k).all() and (got["d"][~valid] == 0).all()
    assert abs(float(got["loss"]) - l64) <= gate and abs(float(ref_loss.detach()) - l64) <= gate
    d_own = np.stack([got["d"][i, i * (1 + k):(i + 1) * (1 + k)] for i in range(Q)])
    assert (np.abs(d_own - d_own64) <= d_gate).all() and (np.abs(grouped.grad.cpu().numpy() - d_own64) <= d_gate).all()


# ---- the autograd op ----------------------------------------------------------------------------------------------------------------

def _op_case(l, r, Q, k, seed=0):
    from taxoexpan_amd.sampler import InBatchGroups
    rng = np.random.default_rng(seed + l)
    G = Q * (1 + k)
    hg = (rng.standard_normal((G, l)) / np.sqrt(l)).astype(np.float32)
    W = (rng.standard_normal((1, l, r)) / np.sqrt(r)).astype(np.float32)            # b = q W^T hg^T ~ N(0, 1)
    q = rng.standard_normal((Q, r)).astype(np.float32)
    anchor = rng.integers(0, 40, size=G).astype(np.int32)
    qnode = rng.permutation(40)[:Q].astype(np.int32)
    rows = {int(v): np.sort(rng.choice(40, size=12, replace=False)) for v in qnode}
    mask_ptr = np.concatenate([[0], np.cumsum([len(rows.get(v, ())) for v in range(40)])]).astype(np.int32)
    mask_idx = np.concatenate([rows.get(v, np.zeros(0, dtype=np.int64)) for v in range(40)]).astype(np.int32)
    pos_col = (np.arange(Q) * (1 + k)).astype(np.int32)
    make = lambda dev: InBatchGroups.from_numpy(anchor, qnode, pos_col, mask_ptr, mask_idx, device=dev)
    return dict(hg=hg, W=W, q=q, args=(pos_col, anchor, qnode, mask_ptr, mask_idx), groups=make, Q=Q, G=G)


def _torch_expr(hg, W, q, valid, pos_col, apply_exp):
    B = (q @ W[0].t()) @ hg.t()
    S = torch.exp(B) if apply_exp else B
    x = torch.where(valid, S, torch.tensor(-np.inf, dtype=S.dtype))
    return F.cross_entropy(x, pos_col, reduction="sum")


@pytest.mark.parametrize("match", ["BIM", "LBM"])
@pytest.mark.parametrize("shape", [(12, 10, 3, 3), (500, 250, 4, 7)])
def test_autograd_op_equals_torch_float64(shape, match):
    from taxoexpan_amd import loss, model_zoo, ops
    from taxoexpan_amd.loss import host_in_batch_valid
    dev = _dev()
    l, r, Q, k = shape
    c = _op_case(*shape)
    apply_exp = match == "LBM"
    valid = torch.from_numpy(host_in_batch_valid(*c["args"]))
    pos = torch.from_numpy(c["args"][0].astype(np.int64))
    res = {}
    for dtype in (torch.float64, torch.float32):
        hg, W = (torch.from_numpy(c[n]).to(dtype).requires_grad_(True) for n in ("hg", "W"))
        out = _torch_expr(hg, W, torch.from_numpy(c["q"]).to(dtype), valid, pos, apply_exp)
        out.backward()
        res[dtype] = (float(out.detach()), hg.grad.numpy(), W.grad.numpy())
    hg, W = (torch.from_numpy(c[n]).to(dev).requires_grad_(True) for n in ("hg", "W"))
    q = torch.from_numpy(c["q"]).to(dev)
    groups = c["groups"](dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    got = ops.InBatchNCEFunction.apply(hg, W, q, apply_exp, groups, total)
    got.backward()
    assert got.shape == () and got.dtype == torch.float32 and int(total.item()) == int(valid.sum())
    l64, l32 = res[torch.float64][0], res[torch.float32][0]
    # a score is two chained dot products of r and l fp32 terms, a row's loss a sum over G of them: (l + r + G + 16) roundings at most
    tol = max(2 * abs(l32 - l64), (l + r + c["G"] + 16) * EPS * max(1.0, abs(l64)))
    print(f"{match} {shape}: |HIP - f64| = {abs(float(got.detach()) - l64):.3e} (tolerance {tol:.3e}, torch fp32 {abs(l32 - l64):.3e})")
    assert abs(float(got.detach()) - l64) <= tol
    errors, report = [], []
    gate_against_f64(hg.grad.cpu().numpy(), res[torch.float64][1], res[torch.float32][1], "d_hg", errors, report)
    gate_against_f64(W.grad.cpu().numpy(), res[torch.float64][2], res[torch.float32][2], "dW", errors, report)
    print(report)
    assert not errors, errors
    # through the public function: a LossTensor, the same bits; the queries get no gradient
    m = (model_zoo.LBM if apply_exp else model_zoo.BIM)(l, r).to(dev)
    with torch.no_grad():
        m.W.weight.copy_(W)
    hg2 = hg.detach().clone().requires_grad_(True)
    out = loss.in_batch_info_nce(m, hg2, q, groups)
    assert isinstance(out, loss.LossTensor) and torch.equal(out.detach(), got.detach())
    out.backward()
    assert torch.equal(hg2.grad, hg.grad) and torch.equal(m.W.weight.grad, W.grad)
    with pytest.raises(ValueError, match="no gradient"):
        loss.in_batch_info_nce(m, hg2, q.clone().requires_grad_(True), groups)
    with pytest.raises(TypeError):
        loss.in_batch_info_nce(torch.nn.Linear(2, 2), hg2, q, groups)                  # no BIM / LBM matcher
    with pytest.raises(ValueError):
        loss.in_batch_info_nce(m, hg2[:-1], q, groups)


# ---- loader and trainer ---------------------------------------------------------------------------------------------------------------

def _toy(tmp_path, mode="train", **kw):
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    d = tmp_path / "toy"
    d.mkdir(exist_ok=True)
    for fn in os.listdir(os.path.join(GOLDEN_DIR, "toy_taxo")):
        shutil.copy(os.path.join(GOLDEN_DIR, "toy_taxo", fn), d)
    random.seed(0)
    opts = dict(mode=mode, sampling_mode=1, negative_size=3, expand_factor=5, normalize_embed=True)
    opts.update(kw)
    return MaskedGraphDataset(MAGDataset("toy", str(d), raw=True), **opts)


def _loader(tmp_path, dev, batch_size=16, seed=5, **kw):
    from taxoexpan_amd.data_loaders import DeviceBatchLoader
    return DeviceBatchLoader(_toy(tmp_path), batch_size, dev, shuffle=True, seed=seed, sampler="device", **kw)


def _model(dev, match="LBM", state=None):
    from taxoexpan_amd import TaxoExpan
    torch.manual_seed(0)
    # (four heads of 16 and 4 position columns: a stack whose output layer folds into the matcher on the default route)
    m = TaxoExpan("PGAT", "WMR", match, in_dim=8, hidden_dim=16, out_dim=24, pos_dim=4, num_layers=1, heads=[4, 1], feat_drop=0.0,
                  attn_drop=0.0, hidden_drop=0.0, out_drop=0.0).to(dev)
    if state is not None:
        m.load_state_dict(state, strict=True)
    return m


def test_loader_attaches_the_groups_of_every_batch(tmp_path):
    from taxoexpan_amd.data_loaders import DeviceBatchLoader
    from taxoexpan_amd.loss import host_in_batch_nce
    dev = _dev()
    loader = _loader(tmp_path, dev, batch_size=8, in_batch=True)
    ds, k = loader.dataset, loader.dataset.negative_size
    n_batches = seen = 0
    order = list(range(len(ds)))
    random.Random(5).shuffle(order)                                   # the loader's first epoch (seed 5)
    for g, h, qf, label in loader:
        ib = g.in_batch
        Q, G = ib.Q, ib.G
        assert G == Q * (1 + k) == label.numel() and qf.rows.shape[0] == Q
        ids = g.ndata["_id"].cpu().numpy()
        pos = g.ndata["pos"].cpu().numpy()                           # (still there: no model has run on the batch)
        off = g.csr(dev).graph_off.cpu().numpy()
        host = ib.numpy()
        assert host["pos_col"].tolist() == [i * (1 + k) for i in range(Q)]
        assert len(off) == G + 1
        for col in range(G):                                         # an egonet's anchor is its one node at position 1 (parents 0, children 2)
            nodes, p = ids[off[col]:off[col + 1]], pos[off[col]:off[col + 1]]
            assert nodes[p == 1].tolist() == [host["anchor"][col]], col
        want_q = loader.features.index_select(0, ib.qnode.long())
        assert torch.equal(qf.rows, want_q)                          # the query ids are the rows the batch's query features were gathered by
        assert host["qnode"].tolist() == [ds.node_list[j] for j in order[seen:seen + Q]]
        seen += Q
        scores = torch.zeros(Q, G, device=dev)
        n_valid = torch.zeros(Q, dtype=torch.int32, device=dev)
        from taxoexpan_amd import _lib
        lib = _lib.load()
        wsb = lib.txe_inbatch_nce_ws_bytes(Q)
        ws, out = torch.zeros(wsb, dtype=torch.uint8, device=dev), torch.zeros(1, device=dev)
        assert lib.txe_inbatch_nce(scores.data_ptr(), G, Q, G, ib.pos_col.data_ptr(), ib.anchor.data_ptr(), ib.qnode.data_ptr(),
                                   ib.mask_ptr.data_ptr(), ib.mask_idx.data_ptr(), 0, out.data_ptr(), scores.data_ptr(), G, n_valid.data_ptr(),
                                   None, ws.data_ptr(), wsb, _lib.stream_ptr()) == 0
        want = [sum(1 for col, a in enumerate(host["anchor"]) if col == i * (1 + k) or int(a) not in set(ds.node2masks[int(host["qnode"][i])]))
                for i in range(Q)]
        assert n_valid.cpu().tolist() == want
        n_batches += 1
    assert n_batches == len(loader) > 2
    with pytest.raises(ValueError, match="in_batch"):
        DeviceBatchLoader(ds, 8, dev, sampler="host", in_batch=True)
    with pytest.raises(ValueError, match="in_batch"):
        DeviceBatchLoader(ds, 8, dev, sampler="device", in_batch=True, repeated_queries=False)
    plain = next(iter(_loader(tmp_path, dev, batch_size=8)))
    assert not hasattr(plain[0], "in_batch")


class _ArmedReplay:
    """batches fetched before, as a loader; with arm, torch's synchronisation check raises from the moment the first batch is handed out
    until the consumer comes back for a batch after the last -- exactly the body of train_epoch's loop, not its read-back behind it"""

    def __init__(self, batches, arm=True):
        self.batches, self.arm, self.armed_steps = batches, arm, 0

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        try:
            for g, h, qf, label, pos in self.batches:
                g.ndata["pos"] = pos                               # (the model takes it out)
                if self.arm:
                    torch.cuda.set_sync_debug_mode("error")
                    self.armed_steps += 1
                yield g, h, qf, label
        finally:
            torch.cuda.set_sync_debug_mode("default")


def test_train_epoch_in_batch_equals_the_hand_written_loop(tmp_path):
    from taxoexpan_amd import encode_graph, loss, ops, optim
    from taxoexpan_amd.trainer import StepLog, train_epoch
    dev = _dev()
    state = {k: v.clone() for k, v in _model(dev).state_dict().items()}
    a, b = _model(dev, state=state), _model(dev, state=state)
    opt_a, opt_b = (optim.Adam(m.parameters(), lr=1e-3, amsgrad=True) for m in (a, b))
    la, lb = _loader(tmp_path, dev, in_batch=True), _loader(tmp_path, dev, in_batch=True)
    k = la.dataset.negative_size
    got = train_epoch(a, la, opt_a, in_batch=True)
    b.train()
    want = []
    for g, h, qf, _label in lb:
        opt_b.zero_grad()
        hg = encode_graph(b, g, h, g.ndata["pos"].to(dev))
        out = loss.in_batch_info_nce(b.match, hg, qf.rows, g.in_batch)
        out.backward()
        opt_b.step()
        want.append(out.item())
    assert got["n_batches"] == len(la) and got["first_nonfinite"] == -1
    assert got["losses"].tolist() == want                             # bit-equal, step by step
    for (name, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), name
    assert got["mean_negatives"] > k and got["mean_negatives"] <= 16 * (1 + k) - 1
    # no host synchronisation inside train_epoch's own loop: batches fetched before (the loader's construction has a synchronisation of
    # its own) go through train_epoch(in_batch=True) with torch's check armed from the first batch handed out until the last is consumed
    batches = [(g, h, qf, label, g.ndata["pos"]) for g, h, qf, label in _loader(tmp_path, dev, in_batch=True)][:4]
    replay = _ArmedReplay(batches)
    train_epoch(a, _ArmedReplay(batches[:1], arm=False), opt_a, in_batch=True)                 # (first calls of this batch size's caches)
    torch.cuda.synchronize()
    try:
        rec = train_epoch(a, replay, opt_a, in_batch=True, log=StepLog(dev, 4))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert replay.armed_steps == 4 and rec["n_batches"] == 4 and rec["first_nonfinite"] == -1
    n_valid = sum(int(loss.host_in_batch_nce(np.zeros((b[0].in_batch.Q, b[0].in_batch.G)), **b[0].in_batch.numpy())[2].sum()) for b in batches)
    n_q = sum(b[0].in_batch.Q for b in batches)
    assert rec["mean_negatives"] == (n_valid - n_q) / n_q                                      # the log's counter word, exactly
    src = inspect.getsource(ops.InBatchNCEFunction) + inspect.getsource(loss.in_batch_info_nce)
    assert not any(w in src for w in (".item(", ".cpu(", ".tolist(", "synchronize", ".numpy("))
    # the default route is what it was
    ops.ROUTES.pop("match", None)
    plain = train_epoch(a, _loader(tmp_path, dev), opt_a)
    assert ops.ROUTES["match"] == "folded" and "mean_negatives" not in plain
    # refusals, each before the first optimizer step
    before = [p.detach().clone() for p in a.parameters()]
    with pytest.raises(ValueError, match="in_batch"):
        train_epoch(a, _loader(tmp_path, dev), opt_a, in_batch=True)                          # a loader without g.in_batch
    with pytest.raises(ValueError, match="in_batch"):
        train_epoch(a, [next(iter(_loader(tmp_path, dev)))], opt_a, in_batch=True)            # a plain list of batches without it
    with pytest.raises(ValueError, match="loss_fn"):
        train_epoch(a, la, opt_a, in_batch=True, loss_fn=loss.info_nce_loss)
    mlp = _model(dev, "MLP")
    with pytest.raises(ValueError, match="BIM / LBM"):
        train_epoch(mlp, la, optim.Adam(mlp.parameters(), lr=1e-3), in_batch=True)
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), before))


def test_fit_in_batch_logs_mean_negatives(tmp_path):
    """fit(in_batch=True) hands the flag to train_epoch: the epoch's log is train_epoch's own, mean_negatives included"""
    from taxoexpan_amd import optim
    from taxoexpan_amd.trainer import fit, train_epoch
    dev = _dev()
    state = {k: v.clone() for k, v in _model(dev).state_dict().items()}
    a, b = _model(dev, state=state), _model(dev, state=state)
    opt_a, opt_b = (optim.Adam(m.parameters(), lr=1e-3, amsgrad=True) for m in (a, b))
    logs = fit(a, _loader(tmp_path, dev, in_batch=True), None, opt_a, epochs=1, monitor="off", in_batch=True)
    want = train_epoch(b, _loader(tmp_path, dev, in_batch=True), opt_b, in_batch=True)
    assert len(logs) == 1 and logs[0]["epoch"] == 1
    assert logs[0]["mean_negatives"] == want["mean_negatives"] > 3                            # more than negative_size
    assert logs[0]["losses"].tolist() == want["losses"].tolist()
    plain = fit(a, _loader(tmp_path, dev), None, opt_a, epochs=1, monitor="off")
    assert "mean_negatives" not in plain[0]


def test_c_abi_refusals_launch_nothing():
    from taxoexpan_amd import _lib
    dev = _dev()
    lib = _lib.load()
    c = cases.case("3x12")
    Q, G = c["Q"], c["G"]
    S = _up(c["S"][:, :G], dev).contiguous()
    d = torch.full((Q, G), 7.0, device=dev)
    t = {k: _up(c[k], dev) for k in ("pos_col", "anchor", "qnode", "mask_ptr", "mask_idx")}
    loss = torch.full((1,), -5.0, device=dev)
    wsb = lib.txe_inbatch_nce_ws_bytes(Q)
    assert wsb >= 8 * Q and _lib.SIGNATURES["txe_inbatch_nce_ws_bytes"][1] == [ctypes.c_int]
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    good = dict(S=S.data_ptr(), ld_s=G, Q=Q, G=G, pos_col=t["pos_col"].data_ptr(), anchor=t["anchor"].data_ptr(), qnode=t["qnode"].data_ptr(),
                mask_ptr=t["mask_ptr"].data_ptr(), mask_idx=t["mask_idx"].data_ptr(), chain_exp=0, loss=loss.data_ptr(), d_out=d.data_ptr(),
                ld_d=G, n_valid=None, valid_total=None, ws=ws.data_ptr(), ws_bytes=wsb, stream=_lib.stream_ptr())
    bad = [dict(Q=-1), dict(G=0), dict(Q=1 << 16, G=1 << 15), dict(S=None), dict(pos_col=None), dict(anchor=None), dict(qnode=None),
           dict(loss=None), dict(d_out=None), dict(mask_ptr=None), dict(mask_idx=None), dict(ws_bytes=wsb - 1), dict(ws=None),
           dict(ld_s=G - 1), dict(ld_d=G - 1)]
    try:
        lib.txe_profile_enable(1)
        lib.txe_profile_reset()
        for change in bad:
            args = dict(good)
            args.update(change)
            assert lib.txe_inbatch_nce(*args.values()) == -1, change
        for exp_args in ((d.data_ptr(), G, -1, G), (d.data_ptr(), G, Q, 0), (d.data_ptr(), G - 1, Q, G), (None, G, Q, G)):
            assert lib.txe_inbatch_exp(*exp_args, _lib.stream_ptr()) == -1, exp_args
        assert lib.txe_inbatch_exp(None, G, 0, G, _lib.stream_ptr()) == 0                       # no rows: nothing to launch
        torch.cuda.synchronize()
        assert lib.txe_profile_count() == 0
    finally:
        lib.txe_profile_enable(0)
        lib.txe_profile_reset()
    assert (d == 7.0).all() and float(loss) == -5.0 and not ws.any()                            # nothing was written
    args = dict(good)
    args.update(Q=0)
    assert lib.txe_inbatch_nce(*args.values()) == 0
    torch.cuda.synchronize()
    assert float(loss) == 0.0 and (d == 7.0).all() and not ws.any()
    try:                                                                                        # (and the arguments were good: two launches)
        lib.txe_profile_enable(1)
        lib.txe_profile_reset()
        assert lib.txe_inbatch_nce(*good.values()) == 0
        torch.cuda.synchronize()
        assert lib.txe_profile_count() == 2
    finally:
        lib.txe_profile_enable(0)
        lib.txe_profile_reset()
    assert np.isfinite(float(loss)) and not (d == 7.0).any()
    # txe_inbatch_exp: in place over the [Q, G] block of a pitched buffer, within one fp32 ulp of the float64 exponential
    x = torch.from_numpy(np.random.default_rng(2).uniform(-6.0, 6.0, size=(Q, G)).astype(np.float32))
    B = torch.full((Q, G + 2), float("nan"), device=dev)
    B[:, :G] = x.to(dev)
    assert lib.txe_inbatch_exp(B.data_ptr(), G + 2, Q, G, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    want = np.exp(x.numpy().astype(np.float64))
    assert (np.abs(B[:, :G].cpu().numpy() - want) <= 2 * EPS * want).all() and torch.isnan(B[:, G:]).all()
