"""CPU: trainer.host_step_log (the written definition of txe_step_log) on a hand-made case, the loop control of trainer.fit with scripted
train_epoch / validate stubs (monitor, ties, early stop, ReduceLROnPlateau on a named metric, an unknown monitor, the divergence stop),
and the checkpoint round trip with a torch.nn.Linear and torch.optim.Adam (file names and keys of base_trainer.py:134-149, resume)."""
import math
import os
import warnings

import numpy as np
import pytest
import torch


# ---- host_step_log -----------------------------------------------------------------------------------------------------------------

def _hand_made():
    """5 steps, gradient tensors of 1, 7 and 300 elements; an inf gradient element at step 2, a NaN loss at step 4"""
    rng = np.random.RandomState(5)
    losses = [np.float32(x) for x in (3.25, 2.7182817, 1.1, 0.3, np.nan)]
    grads = [[rng.randn(n).astype(np.float32) for n in (1, 7, 300)] for _ in range(5)]
    grads[2][2][123] = np.inf
    return losses, grads


def test_host_step_log_equals_its_definition_on_a_hand_made_case():
    from taxoexpan_amd.trainer import host_step_log
    losses, grads = _hand_made()
    loss_log, gnorm2, acc, first_bad = host_step_log(losses, grads)
    assert loss_log.dtype == np.float32 and gnorm2.dtype == np.float64 and acc.dtype == np.float64 and first_bad.dtype == np.int64
    assert loss_log.shape == (5,) and gnorm2.shape == (5,) and acc.shape == (2,) and first_bad.shape == (1,)
    assert np.array_equal(loss_log[:4], np.asarray(losses[:4], dtype=np.float32)) and np.isnan(loss_log[4])
    assert first_bad[0] == 2                                   # the inf gradient of step 2, not the NaN loss of step 4
    for s in (0, 1, 3):
        # every square of an fp32 element is exact in fp64; a sequential python-float sum in index order is the definition.
        # Exact equality with np.sum, as the issue words it, cannot hold beside "sums sequentially in index order": np.sum adds the
        # 300-element tensor pairwise (blocks of 8 accumulators) and differs from the sequential sum in the last bits on all three of
        # these steps.  So: exact against the sequential sum, np.sum within the reordering bound N * 2^-52 -- and exact against np.sum
        # in the next test, on values where every partial sum is exact whatever the order.
        want = 0.0
        for g in grads[s]:
            for v in g.astype(np.float64):
                want += float(v) * float(v)
        assert gnorm2[s] == want, s
        flat = np.concatenate([g.astype(np.float64) for g in grads[s]])
        assert abs(gnorm2[s] - np.sum(flat ** 2)) <= 308 * 2.0 ** -52 * gnorm2[s]
    assert np.isinf(gnorm2[2]) and np.isfinite(gnorm2[4])
    assert acc[1] == 5.0 and np.isnan(acc[0])


def test_host_step_log_sums_equal_numpy_exactly_where_every_order_is_exact():
    """gradients that are small multiples of 1/8: every partial sum of squares is an exact fp64 number, so np.sum's order gives the
    same bits as the sequential sum -- on the issue's sizes 1, 7 and 300"""
    from taxoexpan_amd.trainer import host_step_log
    rng = np.random.RandomState(2)
    losses = [np.float32(v) for v in (0.5, 0.25, 4.0)]
    grads = [[(rng.randint(-64, 65, size=n) / 8.0).astype(np.float32) for n in (1, 7, 300)] for _ in losses]
    loss_log, gnorm2, acc, first_bad = host_step_log(losses, grads, capacity=8)
    assert loss_log.shape == (8,) and first_bad[0] == -1
    for s in range(3):
        assert gnorm2[s] == sum(np.sum(g.astype(np.float64) ** 2) for g in grads[s])
    assert acc.tolist() == [4.75, 3.0] and not gnorm2[3:].any() and not loss_log[3:].any()
    # the first bad step stays; no gradients at all logs the loss only; too many steps are refused
    l2, g2, a2, f2 = host_step_log([np.inf, 1.0, np.nan], [[], [], []])
    assert f2[0] == 0 and g2.tolist() == [0.0, 0.0, 0.0] and a2[1] == 3.0
    with pytest.raises(ValueError):
        host_step_log([1.0, 2.0], [[], []], capacity=1)
    with pytest.raises(ValueError):
        host_step_log([1.0, 2.0], [[]])


def test_step_log_and_train_epoch_refuse_the_host():
    from taxoexpan_amd import trainer
    with pytest.raises(RuntimeError, match="no CPU path"):
        trainer.StepLog("cpu", 4)
    with pytest.raises(ValueError):
        trainer.StepLog("cpu", 0)
    model = torch.nn.Linear(2, 1)
    with pytest.raises(ValueError, match="group_size"):          # an InfoNCE epoch needs the group size before anything runs
        trainer.train_epoch(model, [], torch.optim.SGD(model.parameters(), lr=0.1))


# ---- fit: loop control with stubs --------------------------------------------------------------------------------------------------

class _Script:
    """train_epoch / validate stand-ins that replay scripted values and count their calls"""

    def __init__(self, val, names=("macro_mr", "hit_at_1"), bad_epoch=None):
        self.val, self.names, self.bad_epoch = val, names, bad_epoch
        self.trained = self.validated = 0

    def train_epoch(self, model, loader, optimizer, loss_fn=None, group_size=None):
        self.trained += 1
        bad = self.trained == self.bad_epoch
        return dict(loss=1.0 / self.trained, n_batches=4, losses=np.ones(4, np.float32), grad_norms=np.ones(4), first_nonfinite=2 if bad else -1)

    def validate(self, model, loader, metrics=None, larger_is_better=True):
        assert list(metrics) == list(self.names)
        v = self.val[self.validated]
        self.validated += 1
        return dict(val_metrics=list(v) if isinstance(v, (list, tuple)) else [v] * len(self.names), n_batches=1, n_groups=1, n_positives=1)


def _fit(script, epochs, **kw):
    from taxoexpan_amd.trainer import fit
    model = kw.pop("model", None) or torch.nn.Linear(3, 2)
    opt = kw.pop("optimizer", None) or torch.optim.Adam(model.parameters(), lr=0.5)
    logs = fit(model, [None], [None], opt, epochs, metrics=script.names, train_epoch_fn=script.train_epoch, validate_fn=script.validate, **kw)
    return logs, model, opt


def _files(d):
    return sorted(os.listdir(d)) if os.path.isdir(d) else []


def test_fit_min_monitor_ties_and_early_stop(tmp_path):
    # epoch:        1    2    3 (tie)  4    5    6 (count 3 > early_stop 2: stop, unsaved)
    s = _Script([5.0, 4.0, 4.0, 4.5, 4.5, 4.5, 1.0, 1.0])
    logs, _m, _o = _fit(s, 8, monitor="min val_macro_mr", early_stop=2, save_dir=tmp_path / "a")
    assert [l["epoch"] for l in logs] == [1, 2, 3, 4, 5, 6] and s.trained == 6 and s.validated == 6
    assert logs[2]["val_macro_mr"] == 4.0 and logs[2]["val_hit_at_1"] == 4.0 and logs[0]["loss"] == 1.0
    assert _files(tmp_path / "a") == [f"checkpoint-epoch{e}.pth" for e in (1, 2, 3, 4, 5)] + ["model_best.pth"]
    best = torch.load(tmp_path / "a" / "model_best.pth", weights_only=False)
    assert best["epoch"] == 3 and best["monitor_best"] == 4.0            # the tie of epoch 3 counted as improved
    assert torch.load(tmp_path / "a" / "checkpoint-epoch5.pth", weights_only=False)["monitor_best"] == 4.0
    # early_stop = 3: the count reaches 3 at epoch 6 and does not exceed it -- the run goes on and improves at 7
    s = _Script([5.0, 4.0, 4.0, 4.5, 4.5, 4.5, 1.0, 1.0])
    logs, _m, _o = _fit(s, 8, monitor="min val_macro_mr", early_stop=3)
    assert len(logs) == 8


def test_fit_max_monitor_and_save_period(tmp_path):
    s = _Script([(9.0, 0.1), (9.0, 0.3), (9.0, 0.3), (9.0, 0.2), (9.0, 0.2)])
    logs, _m, _o = _fit(s, 5, monitor="max val_hit_at_1", early_stop=1, save_dir=tmp_path, save_period=2)
    assert len(logs) == 5                                               # stops at epoch 5 (count 2 > 1)
    assert _files(tmp_path) == ["checkpoint-epoch2.pth", "checkpoint-epoch4.pth", "model_best.pth"]
    assert torch.load(tmp_path / "model_best.pth", weights_only=False)["epoch"] == 2    # epoch 3 was best too, but is no save epoch
    with pytest.raises(ValueError):
        _fit(_Script([1.0]), 1, monitor="best val_macro_mr")


def test_fit_feeds_reduce_lr_on_plateau_the_named_metric():
    # macro_mr keeps improving, hit_at_1 plateaus from epoch 2 on: only a scheduler fed hit_at_1 by NAME cuts the rate
    val = [(10.0 - e, 0.5 if e else 0.4) for e in range(6)]
    for name, want in (("val_hit_at_1", 0.05), (None, 0.5)):
        model = torch.nn.Linear(3, 2)
        opt = torch.optim.Adam(model.parameters(), lr=0.5)
        sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="max" if name else "min", factor=0.1, patience=2)
        _fit(_Script(val), 6, model=model, optimizer=opt, monitor="min val_macro_mr", lr_scheduler=sched, scheduler_metric=name)
        assert opt.param_groups[0]["lr"] == pytest.approx(want), name
    # any other scheduler: a plain step per epoch
    model = torch.nn.Linear(3, 2)
    opt = torch.optim.Adam(model.parameters(), lr=0.5)
    _fit(_Script(val), 3, model=model, optimizer=opt, lr_scheduler=torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5))
    assert opt.param_groups[0]["lr"] == pytest.approx(0.0625)
    with pytest.raises(ValueError, match="scheduler_metric"):
        opt = torch.optim.Adam(model.parameters(), lr=0.5)
        _fit(_Script(val), 2, optimizer=opt, monitor="off", lr_scheduler=torch.optim.lr_scheduler.ReduceLROnPlateau(opt))
    with pytest.raises(ValueError, match="val_nope"):
        opt = torch.optim.Adam(model.parameters(), lr=0.5)
        _fit(_Script(val), 2, optimizer=opt, lr_scheduler=torch.optim.lr_scheduler.ReduceLROnPlateau(opt), scheduler_metric="val_nope")


def test_fit_unknown_monitor_warns_once_and_stops_monitoring(tmp_path):
    s = _Script([3.0, 4.0, 5.0, 6.0])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        logs, _m, _o = _fit(s, 4, monitor="min val_missing", early_stop=0, save_dir=tmp_path)
    assert len([x for x in w if "val_missing" in str(x.message)]) == 1
    assert len(logs) == 4                                               # no early stop without a monitor
    assert _files(tmp_path) == [f"checkpoint-epoch{e}.pth" for e in (1, 2, 3, 4)]       # ... and no model_best
    s = _Script([3.0, 4.0])
    logs, _m, _o = _fit(s, 2, monitor="off", early_stop=0, save_dir=tmp_path / "off")
    assert len(logs) == 2 and "model_best.pth" not in _files(tmp_path / "off")


def test_fit_stops_on_a_diverged_epoch_without_a_checkpoint(tmp_path):
    from taxoexpan_amd.trainer import TrainingDiverged
    s = _Script([3.0, 2.0, 1.0, 1.0], bad_epoch=3)
    with pytest.raises(TrainingDiverged) as e:
        _fit(s, 5, save_dir=tmp_path)
    assert (e.value.epoch, e.value.step) == (3, 2) and [l["epoch"] for l in e.value.logs] == [1, 2, 3]
    assert s.trained == 3 and s.validated == 2                          # the diverged epoch is not validated
    assert _files(tmp_path) == ["checkpoint-epoch1.pth", "checkpoint-epoch2.pth", "model_best.pth"]


# ---- checkpoints -------------------------------------------------------------------------------------------------------------------

def _sgd_epochs(seed):
    """a train_epoch stand-in that really trains a Linear on the CPU: two Adam steps per epoch on data drawn from the epoch's number"""
    count = {"epoch": seed}

    def train(model, loader, optimizer, loss_fn=None, group_size=None):
        count["epoch"] += 1
        g = torch.Generator().manual_seed(count["epoch"])
        losses = []
        for _ in range(2):
            x, y = torch.randn(8, 3, generator=g), torch.randn(8, 2, generator=g)
            optimizer.zero_grad()
            loss = ((model(x) - y) ** 2).sum()
            loss.backward()
            optimizer.step()
            losses.append(float(loss.detach()))
        return dict(loss=sum(losses) / 2, n_batches=2, losses=np.asarray(losses, np.float32), grad_norms=np.ones(2), first_nonfinite=-1)
    return train


def test_checkpoint_round_trip_and_resume(tmp_path):
    from taxoexpan_amd.trainer import fit
    val = [5.0, 6.0, 4.0, 7.0]                                          # improved at epochs 1 and 3
    names = ("macro_mr",)
    torch.manual_seed(3)
    init = torch.nn.Linear(3, 2).state_dict()

    def run(epochs, d, resume=None, skip=0):
        model = torch.nn.Linear(3, 2)
        model.load_state_dict(init)
        opt = torch.optim.Adam(model.parameters(), lr=0.05, amsgrad=True)
        s = _Script(val[skip:], names)
        logs = fit(model, [None], [None], opt, epochs, metrics=names, save_dir=d, resume=resume, config={"arch": {"type": "Linear"}},
                   train_epoch_fn=_sgd_epochs(skip), validate_fn=s.validate)
        return logs, model, opt

    logs, model, opt = run(4, tmp_path / "full")
    assert _files(tmp_path / "full") == [f"checkpoint-epoch{e}.pth" for e in (1, 2, 3, 4)] + ["model_best.pth"]
    ck = torch.load(tmp_path / "full" / "checkpoint-epoch2.pth", weights_only=False)
    assert sorted(ck) == ["arch", "config", "epoch", "monitor_best", "optimizer", "state_dict"]      # base_trainer.py:135-142
    assert ck["arch"] == "Linear" and ck["epoch"] == 2 and ck["monitor_best"] == 5.0 and ck["config"] == {"arch": {"type": "Linear"}}
    best = torch.load(tmp_path / "full" / "model_best.pth", weights_only=False)
    assert best["epoch"] == 3 and best["monitor_best"] == 4.0          # written at epochs 1 and 3 only: epoch 4 did not touch it
    ck3 = torch.load(tmp_path / "full" / "checkpoint-epoch3.pth", weights_only=False)
    assert all(torch.equal(best["state_dict"][k], ck3["state_dict"][k]) for k in ck3["state_dict"])
    # resume from epoch 2: epochs 3 and 4 run again, from the same parameters, optimizer state and monitor_best
    logs_r, model_r, opt_r = run(4, tmp_path / "resumed", resume=tmp_path / "full" / "checkpoint-epoch2.pth", skip=2)
    assert [l["epoch"] for l in logs_r] == [3, 4] and [l["loss"] for l in logs_r] == [l["loss"] for l in logs[2:]]
    assert all(torch.equal(a, b) for a, b in zip(model.parameters(), model_r.parameters()))
    sa, sb = opt.state_dict()["state"], opt_r.state_dict()["state"]
    assert sa.keys() == sb.keys()
    for k in sa:
        assert all(torch.equal(torch.as_tensor(sa[k][f]), torch.as_tensor(sb[k][f])) for f in ("step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"))
    assert _files(tmp_path / "resumed") == ["checkpoint-epoch3.pth", "checkpoint-epoch4.pth", "model_best.pth"]
    assert torch.load(tmp_path / "resumed" / "checkpoint-epoch4.pth", weights_only=False)["monitor_best"] == 4.0
    # monitor_best came from the checkpoint: resumed at epoch 3 with a value between the old best (5.0) and +inf, epoch 3 is NOT best
    model = torch.nn.Linear(3, 2)
    opt = torch.optim.Adam(model.parameters(), lr=0.05, amsgrad=True)
    fit(model, [None], [None], opt, 3, metrics=names, save_dir=tmp_path / "worse", resume=tmp_path / "full" / "checkpoint-epoch2.pth",
        train_epoch_fn=_sgd_epochs(2), validate_fn=_Script([5.5], names).validate)
    assert _files(tmp_path / "worse") == ["checkpoint-epoch3.pth"]


def test_step_log_entry_point_checks_its_arguments_without_a_gpu():
    """every refusal of txe_step_log comes before any device work (host buffers stand in for the device pointers: never read)"""
    import ctypes
    from taxoexpan_amd import _lib
    lib = _lib.load()
    assert lib.txe_step_log_ws_bytes(0) == lib.txe_step_log_ws_bytes(1) == 24 and lib.txe_step_log_ws_bytes(256) == 16 + 8 * 256
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    p += -p % 16                                             # a 16-byte aligned address inside the buffer
    ptrs = (ctypes.c_void_p * 2)(p, p)
    numel = (ctypes.c_longlong * 2)(_lib.STEP_LOG_CHUNK + 1, 7)
    good = dict(loss=p, n=2, g=ptrs, numel=numel, s=0, capacity=4, loss_log=p, gnorm2=p, acc=p, first_bad=p, ws=p, ws_bytes=0, stream=None)
    call = lambda **kw: lib.txe_step_log(*dict(good, **kw).values())
    for name in ("loss", "g", "numel", "loss_log", "gnorm2", "acc", "first_bad", "ws"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(s=4), dict(s=-1), dict(capacity=0), dict(n=-1), dict(numel=(ctypes.c_longlong * 2)(5, -1)),
                dict(g=(ctypes.c_void_p * 2)(p, None)), dict(ws=p + 8)):
        assert call(**bad) == -1, bad
    assert call() == -3 and call(ws_bytes=lib.txe_step_log_ws_bytes(3) - 1) == -3        # three chunks: 4,097 + 7 elements
    assert call(numel=(ctypes.c_longlong * 2)(5, 0), g=(ctypes.c_void_p * 2)(p, None), ws_bytes=23) == -3   # an empty tensor needs no pointer
