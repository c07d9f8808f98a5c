"""GPU: txe_step_log against trainer.host_step_log (lane, wave and chunk edges, an unaligned view, more tensors than one launch's table
holds), its non-finite detection and argument checks; trainer.train_epoch against the literal loop of trainer.py:41-77 bit for bit; 20
optimizer steps of the HIP path beside 20 steps of the CPU oracle in float64 and float32; trainer.fit end to end with checkpoints and
resume; and the divergence stop."""
import ctypes
import os
import random
import shutil
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_util import GOLDEN_DIR

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

pytestmark = pytest.mark.gpu

CHUNK = 4096                  # TXE_STEP_LOG_CHUNK: 4097 below straddles it, 300 * 37 + 5 ends inside the third chunk of its tensor
EDGES = [1, 63, 64, 65, 4097, 300 * 37 + 5]
TABLES = {"none": [], "one": [1], "edges": EDGES,
          "unaligned": [2 * CHUNK + 2, 5],                        # (whole chunks of a view that starts 4 bytes into its allocation)
          "two_launches": list(range(0, 55)) + [CHUNK + 1]}       # 56 tensors, one of them empty: more than one kernel-argument table


def _dev():
    return torch.device("cuda:0")


class _RawLog:
    """the arrays of one log and the raw txe_step_log call (return code, nothing raised)"""

    def __init__(self, dev, capacity, n_chunks):
        from taxoexpan_amd import _lib
        self.lib, self.capacity = _lib.load(), capacity
        self.loss = torch.zeros(capacity, dtype=torch.float32, device=dev)
        self.gnorm2 = torch.zeros(capacity, dtype=torch.float64, device=dev)
        self.acc = torch.zeros(2, dtype=torch.float64, device=dev)
        self.first_bad = torch.full((1,), -1, dtype=torch.int64, device=dev)
        self.ws_bytes = self.lib.txe_step_log_ws_bytes(n_chunks)
        self.ws = torch.zeros((self.ws_bytes + 7) // 8, dtype=torch.float64, device=dev)

    def step(self, loss_t, grads, s, **over):
        from taxoexpan_amd import _lib
        a = dict(loss=loss_t.data_ptr(), n=len(grads), g=(ctypes.c_void_p * len(grads))(*[g.data_ptr() for g in grads]),
                 numel=(ctypes.c_longlong * len(grads))(*[g.numel() for g in grads]), s=s, capacity=self.capacity, loss_log=self.loss.data_ptr(),
                 gnorm2=self.gnorm2.data_ptr(), acc=self.acc.data_ptr(), first_bad=self.first_bad.data_ptr(), ws=self.ws.data_ptr(),
                 ws_bytes=self.ws_bytes, stream=_lib.stream_ptr())
        a.update(over)
        return self.lib.txe_step_log(*a.values())

    def host(self):
        return tuple(t.cpu().numpy() for t in (self.loss, self.gnorm2, self.acc, self.first_bad))


def _draw(name, steps=6, seed=11):
    """fixed-seed losses and gradient tables (host arrays); gradients of very unequal scale so that the sum's order matters"""
    rng = np.random.RandomState(seed)
    sizes = TABLES[name]
    losses = (rng.rand(steps) * 30).astype(np.float32)
    grads = [[(rng.randn(n) * 10.0 ** rng.randint(-3, 4)).astype(np.float32) for n in sizes] for _ in range(steps)]
    return sizes, losses, grads


def _upload(name, host_grads, dev):
    """device copies of one step's gradients ("unaligned": its first tensor is a view one element into a larger allocation)"""
    out = []
    for i, g in enumerate(host_grads):
        if name == "unaligned" and i == 0:
            base = torch.zeros(g.size + 1, dtype=torch.float32, device=dev)
            base[1:] = torch.from_numpy(g).to(dev)
            out.append(base[1:])
            assert out[-1].data_ptr() % 16 == 4
        else:
            out.append(torch.from_numpy(g).to(dev))
    return out


def _run(name, dev, losses, grads, capacity=8):
    n_chunks = sum(-(-n // CHUNK) for n in TABLES[name])
    log = _RawLog(dev, capacity, n_chunks)
    for s, (l, gs) in enumerate(zip(losses, grads)):
        assert log.step(torch.tensor(l, dtype=torch.float32, device=dev), _upload(name, gs, dev), s) == 0
    torch.cuda.synchronize()
    return log.host()


@pytest.mark.parametrize("name", list(TABLES))
def test_step_log_kernel_equals_the_restatement(name):
    from taxoexpan_amd.trainer import host_step_log
    dev = _dev()
    sizes, losses, grads = _draw(name)
    N = sum(sizes)
    loss_log, gnorm2, acc, first_bad = _run(name, dev, losses, grads)
    w_loss, w_gnorm2, w_acc, w_bad = host_step_log(losses, grads, capacity=8)
    assert np.array_equal(loss_log, w_loss) and first_bad[0] == w_bad[0] == -1                  # exact
    for s in range(6):
        ref = float(np.sum(np.concatenate([g.astype(np.float64) for g in grads[s]]) ** 2)) if N else 0.0
        # N exactly representable squares added in another order: at most N * 2^-52 relative (derived, not tuned)
        assert abs(gnorm2[s] - ref) <= N * 2.0 ** -52 * ref, (name, s, gnorm2[s], ref)
        assert abs(gnorm2[s] - w_gnorm2[s]) <= 2 * N * 2.0 ** -52 * ref
    assert not gnorm2[6:].any() and not loss_log[6:].any()                                       # rows past the last step are untouched
    want = 0.0
    for l in losses:
        want += float(l)
    assert acc[0] == want == w_acc[0] and acc[1] == 6.0                                          # the fp64 sum of the fp32 losses, exactly
    again = _run(name, dev, losses, grads)
    for a, b in zip((loss_log, gnorm2, acc, first_bad), again):
        assert a.tobytes() == b.tobytes()                                                        # two runs: bit-identical


def test_step_log_finds_the_first_non_finite_step():
    dev = _dev()
    _sizes, losses, grads = _draw("edges")
    assert _run("edges", dev, losses, grads)[3][0] == -1
    g = [[a.copy() for a in step] for step in grads]
    g[3][-1][-1] = np.inf                                      # the last element of the last tensor (inside a tail chunk), step 3
    g[4][0][0] = np.nan                                        # a later bad step does not overwrite the first
    loss_log, gnorm2, acc, first_bad = _run("edges", dev, losses, g)
    assert first_bad[0] == 3 and np.isinf(gnorm2[3]) and np.isnan(gnorm2[4]) and np.isfinite(gnorm2[[0, 1, 2, 5]]).all()
    l = losses.copy()
    l[1] = np.nan                                              # a NaN loss at step 1 alone, every gradient finite
    loss_log, gnorm2, acc, first_bad = _run("edges", dev, l, grads)
    assert first_bad[0] == 1 and np.isnan(loss_log[1]) and np.isfinite(gnorm2[:6]).all()
    # ... and with the inf gradient of step 3 behind it: the first bad step stays
    loss_log, gnorm2, acc, first_bad = _run("edges", dev, l, g)
    assert first_bad[0] == 1 and np.isnan(loss_log[1]) and np.isnan(acc[0]) and acc[1] == 6.0
    g = [[a.copy() for a in step] for step in grads]
    g[2][4][CHUNK - 1] = -np.inf                               # the last element of a whole chunk
    assert _run("edges", dev, losses, g)[3][0] == 2
    assert _run("none", dev, np.asarray([1.0, np.inf, 2.0], dtype=np.float32), [[], [], []])[3][0] == 1


def test_step_log_argument_checks():
    from taxoexpan_amd import trainer
    dev = _dev()
    log = _RawLog(dev, 4, 3)
    loss = torch.ones((), device=dev)
    grads = [torch.ones(CHUNK + 1, device=dev), torch.ones(7, device=dev)]
    assert log.step(loss, grads, 4) == -1 and log.step(loss, grads, -1) == -1                    # s == capacity; s < 0
    for name in ("loss", "loss_log", "gnorm2", "acc", "first_bad", "ws", "g", "numel"):
        assert log.step(loss, grads, 0, **{name: None}) == -1, name
    assert log.step(loss, grads, 0, n=-1) == -1
    assert log.step(loss, grads, 0, ws_bytes=log.ws_bytes - 1) == -3
    torch.cuda.synchronize()
    l, g2, acc, bad = log.host()
    assert not l.any() and not g2.any() and not acc.any() and bad[0] == -1                       # nothing was launched
    assert log.step(loss, grads, 3) == 0                                                         # ... and the last row can be written
    torch.cuda.synchronize()
    assert log.host()[1][3] == CHUNK + 8 and log.host()[2].tolist() == [1.0, 1.0]
    # StepLog: parameters without a gradient are skipped; recording past the capacity raises on the host, before any launch
    p = [torch.nn.Parameter(torch.ones(5, device=dev)), torch.nn.Parameter(torch.ones(3, device=dev))]
    p[0].grad = torch.full((5,), 2.0, device=dev)
    sl = trainer.StepLog(dev, 2)
    sl.record(loss, p)
    sl.record(loss * 3, p)
    with pytest.raises(IndexError):
        sl.record(loss, p)
    with pytest.raises(ValueError):
        trainer.StepLog(dev, 2).record(loss.double(), p)
    r = sl.read()
    assert r["loss"].tolist() == [1.0, 3.0] and r["grad_norm"].tolist() == [20.0 ** 0.5] * 2 and r["loss_sum"] == 4.0
    assert r["n_steps"] == 2 and r["first_nonfinite"] == -1
    sl.reset()
    p[0].grad[4] = float("nan")
    sl.record(loss, p)
    r = sl.read()
    assert r["n_steps"] == 1 and r["first_nonfinite"] == 0 and r["loss"].tolist() == [1.0] and np.isnan(r["grad_norm"][0])


# ---- the epoch loop ----------------------------------------------------------------------------------------------------------------

def _toy(tmp_path, mode="train", **kw):
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    d = tmp_path / "toy"
    d.mkdir(exist_ok=True)
    for fn in os.listdir(os.path.join(GOLDEN_DIR, "toy_taxo")):
        shutil.copy(os.path.join(GOLDEN_DIR, "toy_taxo", fn), d)
    random.seed(0)
    opts = dict(mode=mode, sampling_mode=1 if mode == "train" else 0, negative_size=3, expand_factor=5, normalize_embed=True)
    opts.update(kw)
    return MaskedGraphDataset(MAGDataset("toy", str(d), raw=True), **opts)


def _loader(tmp_path, dev, mode="train", seed=5):
    from taxoexpan_amd.data_loaders import DeviceBatchLoader
    return DeviceBatchLoader(_toy(tmp_path, mode), 16, dev, shuffle=True, seed=seed, sampler="device")


def _model(dev, match="LBM", state=None):
    from taxoexpan_amd import TaxoExpan
    torch.manual_seed(0)
    m = TaxoExpan("PGAT", "WMR", match, in_dim=8, hidden_dim=6, out_dim=5, pos_dim=3, num_layers=1, heads=[2, 1], feat_drop=0.0,
                  attn_drop=0.0, hidden_drop=0.0, out_drop=0.0).to(dev)
    if state is not None:
        m.load_state_dict(state, strict=True)
    return m


def bce_like(prediction, label):
    return F.binary_cross_entropy_with_logits(prediction.reshape(-1), label.to(prediction.dtype), reduction="sum")


def _reference_loop(model, loader, optimizer, loss_fn, info_nce, dev):
    """trainer.py:41-77, statement for statement (the tensorboard writer and the logger left out)"""
    model.train()
    total_loss = 0
    losses = []
    for batch_example in loader:
        bg, h, nf, label = batch_example
        optimizer.zero_grad()
        prediction = model(bg, h, nf)
        if info_nce:
            n_batches = int(label.sum().detach())             # (trainer.py:53; a 0-dim tensor as a size is the same read-back)
            prediction = prediction.reshape(n_batches, -1)
            target = torch.zeros(n_batches, dtype=torch.long).to(dev)
            loss = loss_fn(prediction, target)
        else:
            loss = loss_fn(prediction, label)
        loss.backward()
        optimizer.step()
        losses.append(loss.item())
        total_loss += loss.item()
    return total_loss / len(loader), losses


@pytest.mark.parametrize("match,loss_name", [("LBM", "info_nce_loss"), ("BIM", "bce_like")])
def test_train_epoch_equals_the_hand_written_loop(tmp_path, match, loss_name):
    from taxoexpan_amd import loss as txe_loss, optim
    from taxoexpan_amd.trainer import train_epoch
    dev = _dev()
    loss_fn = txe_loss.info_nce_loss if loss_name == "info_nce_loss" else bce_like
    state = {k: v.clone() for k, v in _model(dev, match).state_dict().items()}
    a, b = _model(dev, match, state), _model(dev, match, state)
    opt_a, opt_b = (optim.Adam(m.parameters(), lr=1e-3, amsgrad=True) for m in (a, b))
    la, lb = _loader(tmp_path, dev), _loader(tmp_path, dev)
    for _epoch in range(2):
        got = train_epoch(a, la, opt_a, loss_fn=loss_fn)
        want_loss, want_losses = _reference_loop(b, lb, opt_b, loss_fn, loss_name.startswith("info_nce"), dev)
        assert got["n_batches"] == len(la) == 9 and got["first_nonfinite"] == -1
        assert got["losses"].dtype == np.float32 and got["losses"].tolist() == want_losses          # bit-equal, step by step
        assert got["loss"] == want_loss
        assert got["grad_norms"].shape == (9,) and np.isfinite(got["grad_norms"]).all() and (got["grad_norms"] > 0).all()
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), k
    assert a.training
    if loss_name == "info_nce_loss":
        from taxoexpan_amd.trainer import StepLog
        before = [p.detach().clone() for p in a.parameters()]
        with pytest.raises(ValueError, match="holds 2 steps"):                 # a log too small for the epoch: refused before any step
            train_epoch(a, la, opt_a, log=StepLog(dev, 2))
        assert all(torch.equal(p, q) for p, q in zip(a.parameters(), before))
        with pytest.raises(ValueError, match="multiple"):
            train_epoch(a, la, opt_a, group_size=5)


def _recorded_batches(tmp_path, dev, n):
    """n training batches of the toy loader, kept: the device tuple, and the oracle's view of it on the host"""
    from taxoexpan_amd import ops
    loader = _loader(tmp_path, dev)
    out = []
    while len(out) < n:
        for g, x, qf, label in loader:
            csr = g.csr(dev)
            deg = (csr.rowptr_in[1:] - csr.rowptr_in[:-1]).long()
            host = dict(src=csr.col_src.long().cpu(), dst=torch.repeat_interleave(torch.arange(deg.numel(), device=dev), deg).cpu(),
                        pos=g.ndata["pos"].long().cpu(), graph_off=csr.graph_off.long().cpu(), num_nodes=int(deg.numel()),
                        x=x.cpu().clone(), qf=ops.dense_rows(qf).cpu().clone(), label=label.cpu().clone())
            out.append(((g, x, qf, label, g.ndata["pos"]), host))
            if len(out) == n:
                break
    return out


class _Replay:
    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for g, x, qf, label, pos in self.batches:
            g.ndata["pos"] = pos                               # (the model takes it out)
            yield g, x, qf, label


def _oracle_losses(batches, state, dtype, lr):
    import txe_oracle as orc
    P = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in state.items()}
    opt = torch.optim.Adam(list(P.values()), lr=lr, amsgrad=True)
    losses = []
    for b in batches:
        opt.zero_grad()
        s, _hg, _hn = orc.taxoexpan_forward(P, b, b["x"].to(dtype), b["qf"].to(dtype), "PGAT", "WMR", "LBM", [2, 1], 1, None)
        assert int(b["label"].sum()) * 4 == s.shape[0]
        loss = orc.info_nce_loss(s, s.shape[0] // 4)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return np.asarray(losses, dtype=np.float64)


def test_twenty_steps_beside_the_oracle(tmp_path):
    """20 optimizer steps on the same 20 batches (dropout 0, Adam amsgrad, lr 1e-3: the float64 oracle stays finite there, checked on
    the CPU when the test was written, and asserted below): the HIP path through train_epoch, the CPU oracle in float64 with
    torch.optim.Adam (the reference), the same oracle in float32 (the yardstick).  Gate, as for the single-step gradients: max over the
    steps of the HIP loss's relative error <= max(2 x the fp32 oracle's, 1e-5).
    Measured on an MI355X: the fp32 oracle 1.8e-7, the HIP path 1.3e-7 (profiles/NOTES.md), so the 1e-5 floor is the gate."""
    from taxoexpan_amd import optim
    from taxoexpan_amd.trainer import train_epoch
    dev = _dev()
    lr = 1e-3
    rec = _recorded_batches(tmp_path, dev, 20)
    model = _model(dev)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    got = train_epoch(model, _Replay([r[0] for r in rec]), optim.Adam(model.parameters(), lr=lr, amsgrad=True), group_size=4)
    assert got["n_batches"] == 20 and got["first_nonfinite"] == -1
    ref = _oracle_losses([r[1] for r in rec], state, torch.float64, lr)
    assert np.isfinite(ref).all(), ref
    f32 = _oracle_losses([r[1] for r in rec], state, torch.float32, lr)
    yardstick = float(np.max(np.abs(f32 - ref) / np.abs(ref)))
    err = float(np.max(np.abs(got["losses"].astype(np.float64) - ref) / np.abs(ref)))
    print(f"\n20 steps: fp32 oracle vs float64 oracle {yardstick:.3e}, HIP vs float64 oracle {err:.3e} (max relative loss error over the steps)")
    assert err <= max(2 * yardstick, 1e-5), f"HIP {err:.3e} against the float64 oracle; the fp32 oracle's own error is {yardstick:.3e}"
    assert abs(ref[-1] - ref[0]) > 1e-3 * ref[0]               # (the parameters did move: 20 steps, not 20 times the first)


def _advance(loader, epochs):
    for _ in range(epochs):
        for _batch in loader:
            pass


def _fit_setup(tmp_path, dev, skip_epochs=0):
    """model, optimizer, scheduler and both toy loaders as a fresh process would build them; skip_epochs: the loaders' epoch counters
    and the device sampler's positive pointers are not restorable from outside, so a resumed run draws (and drops) that many epochs"""
    from taxoexpan_amd import optim
    model = _model(dev)
    opt = optim.Adam(model.parameters(), lr=1e-3, amsgrad=True)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=0)
    train, valid = _loader(tmp_path, dev), _loader(tmp_path, dev, mode="validation", seed=2)
    _advance(train, skip_epochs)
    _advance(valid, skip_epochs)
    return model, opt, sched, train, valid


def test_fit_end_to_end_with_checkpoints_and_resume(tmp_path):
    """3 epochs on the toy loaders.  The resumed run builds fresh loaders and draws two epochs from them first: DeviceBatchLoader's epoch
    counter and the device sampler's positive pointers cannot be set from outside (a limitation of the loader, not of fit)."""
    from taxoexpan_amd.evaluate import VALIDATION_METRICS, validate
    from taxoexpan_amd.trainer import fit
    dev = _dev()
    model, opt, sched, train, valid = _fit_setup(tmp_path, dev)
    logs = fit(model, train, valid, opt, 3, lr_scheduler=sched, save_dir=tmp_path / "run", config={"name": "toy"})
    assert [l["epoch"] for l in logs] == [1, 2, 3] and all(l["n_batches"] == 9 and l["first_nonfinite"] == -1 for l in logs)
    assert sorted(os.listdir(tmp_path / "run")) == ["checkpoint-epoch1.pth", "checkpoint-epoch2.pth", "checkpoint-epoch3.pth", "model_best.pth"]
    best = torch.load(tmp_path / "run" / "model_best.pth", map_location="cpu", weights_only=False)
    assert sorted(best) == ["arch", "config", "epoch", "monitor_best", "optimizer", "state_dict"] and best["arch"] == "TaxoExpan"
    e = best["epoch"]
    assert best["monitor_best"] == logs[e - 1]["val_macro_mr"] == min(l["val_macro_mr"] for l in logs)
    fresh = _model(dev, state=best["state_dict"])              # strict=True
    _m, _o, _s, _t, valid2 = _fit_setup(tmp_path, dev)
    _advance(valid2, e - 1)                                    # the validation batches of epoch e
    again = validate(fresh, valid2, metrics=VALIDATION_METRICS)
    assert again["val_metrics"] == [logs[e - 1]["val_" + m] for m in VALIDATION_METRICS]
    # resume from epoch 2: epoch 3 again, bit for bit
    model_r, opt_r, sched_r, train_r, valid_r = _fit_setup(tmp_path, dev, skip_epochs=2)
    logs_r = fit(model_r, train_r, valid_r, opt_r, 3, lr_scheduler=sched_r, save_dir=tmp_path / "resumed",
                 resume=tmp_path / "run" / "checkpoint-epoch2.pth")
    assert len(logs_r) == 1 and logs_r[0]["epoch"] == 3
    assert logs_r[0]["losses"].tobytes() == logs[2]["losses"].tobytes() and logs_r[0]["grad_norms"].tobytes() == logs[2]["grad_norms"].tobytes()
    assert logs_r[0]["loss"] == logs[2]["loss"] and all(logs_r[0]["val_" + m] == logs[2]["val_" + m] for m in VALIDATION_METRICS)
    for (k, p), q in zip(model.named_parameters(), model_r.parameters()):
        assert torch.equal(p, q), k
    assert torch.load(tmp_path / "resumed" / "checkpoint-epoch3.pth", map_location="cpu", weights_only=False)["monitor_best"] == \
        torch.load(tmp_path / "run" / "checkpoint-epoch3.pth", map_location="cpu", weights_only=False)["monitor_best"]


def test_fit_stops_after_a_diverged_epoch(tmp_path):
    from taxoexpan_amd import loss as txe_loss
    from taxoexpan_amd.trainer import TrainingDiverged, fit
    dev = _dev()
    model, opt, _sched, train, valid = _fit_setup(tmp_path, dev)
    calls = {"n": 0}

    def info_nce_then_inf(output, target=None):
        loss = txe_loss.info_nce_loss(output, target)
        calls["n"] += 1
        return loss * float("inf") if calls["n"] == 3 else loss          # step 2 of epoch 1

    with pytest.raises(TrainingDiverged) as e:
        fit(model, train, valid, opt, 3, save_dir=tmp_path / "run", loss_fn=info_nce_then_inf)
    assert (e.value.epoch, e.value.step) == (1, 2) and len(e.value.logs) == 1
    assert calls["n"] == 9                                       # the epoch ran to its end: train_epoch never stops early
    assert np.isinf(e.value.logs[0]["losses"][2]) and np.isfinite(e.value.logs[0]["losses"][:2]).all()
    assert not os.path.isdir(tmp_path / "run") or os.listdir(tmp_path / "run") == []
