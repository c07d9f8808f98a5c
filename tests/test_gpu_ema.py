"""GPU: the averaged weights.  txe_adam_step_ema through the C ABI -- p, m, v, vmax bit-equal to txe_adam_step (the average never
perturbs the step), e bit-equal to optim.host_ema_update in float32 fed the device's own new p (aligned, a misaligned tensor, only e
misaligned, 26 tensors = two launches), ema == NULL against txe_adam_step_guarded, the frozen step, the active clip; txe_tensor_swap
on NaN payloads, infinities, -0.0 and denormals; optim.Adam(ema_decay=...) with averaged_parameters(), state-dict round trips and the
warm-up schedule; train_epoch's freeze; fit(averaged=True) with checkpoints, resume and load_averaged.

Every comparison is bit for bit: against the unchanged entry points, against the float32 restatement (the kernel operation for
operation; tests/test_ema_cpu.py gates that restatement against float64), or against a run that never averaged."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

from test_gpu_guarded_step import (CASES, HYPER, SIZES, UNALIGNED, _assert_same_bits, _dev_array, _gnorm2, _host_draw, _inf_from_call, _scalars,
                                   _Tensors)
from test_gpu_trainer import _dev, _model, _recorded_batches, _Replay

pytestmark = pytest.mark.gpu

DECAY = 0.9
MANY = SIZES + [UNALIGNED] + [1 + 37 * k for k in range(20)]               # 26 tensors: two launches, tensor 5 misaligned


class _EmaTensors(_Tensors):
    """_Tensors with the average e (a copy of p) and the txe_adam_step_ema call; e_unaligned: tensors whose e ALONE sits 4 bytes into
    its allocation"""

    def __init__(self, host_p, dev, unaligned=(), e_unaligned=()):
        super().__init__(host_p, dev, unaligned)
        self.e = [_dev_array(a.copy(), dev, i in self.unaligned or i in set(e_unaligned)) for i, a in enumerate(host_p)]

    def step_ema(self, host_g, step, ams, wd, decay=DECAY, ema=True, gnorm2=None, first_bad=None, max_grad_norm=0.0):
        g = [_dev_array(a, self.dev, i in self.unaligned) for i, a in enumerate(host_g)]
        rc = self.lib.txe_adam_step_ema(len(self.p), self._tab(self.p), self._tab(g), self._tab(self.m), self._tab(self.v),
                                        self._tab(self.x) if ams else None, self._tab(self.e) if ema else None, self.n, HYPER["lr"], HYPER["beta1"],
                                        HYPER["beta2"], HYPER["eps"], wd, step, decay, None if gnorm2 is None else gnorm2.data_ptr(),
                                        None if first_bad is None else first_bad.data_ptr(), max_grad_norm, self._lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        return g

    def host_e(self):
        return [t.cpu().numpy().copy() for t in self.e]


def _assert_e(got, want, what):
    for i, (x, y) in enumerate(zip(got, want)):
        assert x.tobytes() == y.tobytes(), f"{what}: the average of tensor {i} ({x.size} elements) differs"


@pytest.mark.parametrize("ams,wd", CASES)
@pytest.mark.parametrize("layout", ["six", "e_alone_misaligned", "two_launches"])
def test_kernel_leaves_the_step_alone_and_averages_like_the_restatement(ams, wd, layout):
    from taxoexpan_amd.optim import host_ema_update
    dev = _dev()
    sizes = MANY if layout == "two_launches" else SIZES + [UNALIGNED]
    host_p, host_g = _host_draw(sizes, seed=21, steps=3)
    plain = _Tensors(host_p, dev, unaligned=[5])
    ema = _EmaTensors(host_p, dev, unaligned=[5], e_unaligned=[2, 4] if layout == "e_alone_misaligned" else [])
    if layout == "e_alone_misaligned":
        assert ema.e[2].data_ptr() % 16 == 4 and ema.p[2].data_ptr() % 16 == 0 and ema.m[2].data_ptr() % 16 == 0
    want_e = [a.copy() for a in host_p]
    for s in (1, 2, 3):
        plain.step(host_g[s - 1], s, ams, wd, guarded=False)
        ema.step_ema(host_g[s - 1], s, ams, wd)
        got = ema.host()
        _assert_same_bits(got, plain.host(), f"{layout}, step {s}")
        want_e = [host_ema_update(e, p, DECAY, np.float32) for e, p in zip(want_e, got["p"])]
        _assert_e(ema.host_e(), want_e, f"{layout}, step {s}")
    assert all((e != p).any() for e, p in zip(want_e, got["p"])) and all((e != p0).any() for e, p0 in zip(want_e, host_p))


@pytest.mark.parametrize("ams,wd", CASES)
def test_null_ema_is_the_guarded_entry_point(ams, wd):
    """guard active (clip at a third of the norm), inactive (first_bad -1, norm below the threshold) and both pointers NULL; the decay
    is not looked at"""
    dev = _dev()
    sizes = SIZES + [UNALIGNED]
    host_p, host_g = _host_draw(sizes, seed=22)
    for name in ("active", "inactive", "null"):
        a, b = _Tensors(host_p, dev, unaligned=[5]), _EmaTensors(host_p, dev, unaligned=[5])
        for s in (1, 2):
            g2 = _gnorm2(host_g[s - 1])
            gnorm2, first_bad = _scalars(dev, g2, -1) if name != "null" else (None, None)
            c = 0.0 if name == "null" else math.sqrt(g2) * (1.0 / 3.0 if name == "active" else 2.0)
            a.step(host_g[s - 1], s, ams, wd, True, gnorm2, first_bad, c)
            b.step_ema(host_g[s - 1], s, ams, wd, decay=float("nan"), ema=False, gnorm2=gnorm2, first_bad=first_bad, max_grad_norm=c)
            _assert_same_bits(b.host(), a.host(), f"{name}, step {s}")
        _assert_e(b.host_e(), host_p, name)                      # e was not passed: untouched


@pytest.mark.parametrize("ams", [True, False])
def test_frozen_step_leaves_the_average_alone(ams):
    dev = _dev()
    host_p, host_g = _host_draw(MANY, seed=23)
    t = _EmaTensors(host_p, dev, unaligned=[5])
    t.step_ema(host_g[0], 1, ams, 0.01)
    before, before_e = t.host(), t.host_e()
    assert all((e != p0).any() for e, p0 in zip(before_e, host_p))
    bad = [g.copy() for g in host_g[1]]
    for i, g in enumerate(bad):
        g[0], g[-1] = np.nan, np.inf if i % 2 else -np.inf
    gnorm2, first_bad = _scalars(dev, float("nan"), 0)
    t.step_ema(bad, 2, ams, 0.01, gnorm2=gnorm2, first_bad=first_bad, max_grad_norm=1.0)
    t.step_ema(bad, 2, ams, 0.01, first_bad=first_bad)
    _assert_same_bits(t.host(), before, "frozen")
    _assert_e(t.host_e(), before_e, "frozen")
    first_bad.fill_(-1)                                          # ... and -1 lets the (finite) step through: e moves, in both launches
    t.step_ema(host_g[1], 2, ams, 0.01, first_bad=first_bad)
    after, after_e = t.host(), t.host_e()
    assert all((a != b).any() for a, b in zip(after["p"], before["p"])) and all((a != b).any() for a, b in zip(after_e, before_e))
    assert all(np.isfinite(e).all() for e in after_e)


@pytest.mark.parametrize("ams,wd", CASES)
def test_active_clip_reaches_the_average_through_p(ams, wd):
    """the norm is 3 times the threshold: p is the clipped step's (bit-equal to txe_adam_step_guarded), and e the restatement of THAT p"""
    from taxoexpan_amd.optim import host_ema_update
    dev = _dev()
    sizes = SIZES + [UNALIGNED]
    host_p, host_g = _host_draw(sizes, seed=24)
    guarded, free, ema = _Tensors(host_p, dev, unaligned=[5]), _Tensors(host_p, dev, unaligned=[5]), _EmaTensors(host_p, dev, unaligned=[5])
    want_e = [a.copy() for a in host_p]
    for s in (1, 2):
        g2 = _gnorm2(host_g[s - 1])
        gnorm2, first_bad = _scalars(dev, g2, -1)
        c = math.sqrt(g2) / 3.0
        guarded.step(host_g[s - 1], s, ams, wd, True, gnorm2, first_bad, c)
        free.step(host_g[s - 1], s, ams, wd, guarded=False)
        ema.step_ema(host_g[s - 1], s, ams, wd, gnorm2=gnorm2, first_bad=first_bad, max_grad_norm=c)
        got = ema.host()
        _assert_same_bits(got, guarded.host(), f"step {s}")
        want_e = [host_ema_update(e, p, DECAY, np.float32) for e, p in zip(want_e, got["p"])]
        _assert_e(ema.host_e(), want_e, f"step {s}")
    assert any(a.tobytes() != b.tobytes() for a, b in zip(got["m"], free.host()["m"]))           # the clip acted


def test_tensor_swap_moves_words():
    from taxoexpan_amd import _lib
    dev = _dev()
    lib = _lib.load()
    rng = np.random.RandomState(25)
    special = np.array([0x7fc00001, 0xffc12345, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff, 0x7f800001], dtype=np.uint32)
    host_a, host_b = [], []
    for n in MANY:
        a, b = rng.randn(n).astype(np.float32).view(np.uint32), rng.randn(n).astype(np.float32).view(np.uint32)
        for k, w in enumerate(special):                          # two NaN payloads, +-Inf, -0.0, denormals, a signalling NaN
            a[(7 * k) % n] = w
            b[(11 * k + n // 2) % n] = w
        host_a.append(a)
        host_b.append(b)
    A = [_dev_array(a.view(np.float32), dev, i == 5) for i, a in enumerate(host_a)]
    B = [_dev_array(b.view(np.float32), dev, i in (5, 3)) for i, b in enumerate(host_b)]       # pair 3: only b misaligned
    n = (ctypes.c_longlong * len(MANY))(*MANY)

    def tab(ts):
        return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    def words(ts):
        return [t.cpu().numpy().view(np.uint32) for t in ts]

    assert lib.txe_tensor_swap(len(MANY), tab(A), tab(B), n, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(words(A), words(B))):
        assert np.array_equal(a, host_b[i]) and np.array_equal(b, host_a[i]), i
    assert lib.txe_tensor_swap(len(MANY), tab(A), tab(B), n, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(words(A), words(B))):
        assert np.array_equal(a, host_a[i]) and np.array_equal(b, host_b[i]), i


# ---- the optimizer -----------------------------------------------------------------------------------------------------------------

STEPS = 3


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    """3 recorded training batches of the toy loader and the model's initial state (dropout 0 everywhere)"""
    dev = _dev()
    rec = _recorded_batches(tmp_path_factory.mktemp("toy"), dev, STEPS)
    state = {k: v.detach().clone() for k, v in _model(dev).state_dict().items()}
    return dev, [r[0] for r in rec], state


def _fresh(toy, **adam):
    from taxoexpan_amd import optim
    dev, _batches, state = toy
    model = _model(dev, state=state)
    return model, optim.Adam(model.parameters(), lr=1e-3, amsgrad=True, **adam)


def _one_step(model, opt, batch):
    from taxoexpan_amd.loss import info_nce_loss
    g, x, qf, _label = next(iter(_Replay([batch])))
    model.train()
    opt.zero_grad()
    loss = info_nce_loss(model(g, x, qf).reshape(-1, 4), None)
    loss.backward()
    opt.step()
    return loss


def _forward(model, batch):
    g, x, qf, _label = next(iter(_Replay([batch])))
    model.eval()
    with torch.no_grad():
        return model(g, x, qf).clone()


def _params(model):
    return [p.detach().cpu().numpy().copy() for p in model.parameters()]


def _emas(model, opt):
    return [opt.state[p]["ema"].detach().cpu().numpy().copy() for p in model.parameters()]


def _assert_same_state(model_a, opt_a, model_b, opt_b, ema=False):
    for (k, p), q in zip(model_a.named_parameters(), model_b.parameters()):
        assert torch.equal(p, q), k
        sa, sb = opt_a.state[p], opt_b.state[q]
        assert float(sa["step"]) == float(sb["step"]), k
        for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq") + (("ema",) if ema else ()):
            assert sa[key].cpu().numpy().tobytes() == sb[key].cpu().numpy().tobytes(), (k, key)


def test_optimizer_averages_beside_an_unchanged_step(toy):
    from taxoexpan_amd.optim import host_ema_update
    dev, batches, state = toy
    model, opt = _fresh(toy, ema_decay=DECAY)
    plain_model, plain_opt = _fresh(toy)
    want = _params(model)                                          # the average starts as the parameter before its first update
    for b in batches:
        _one_step(model, opt, b)
        _one_step(plain_model, plain_opt, b)
        want = [host_ema_update(e, p, DECAY, np.float32) for e, p in zip(want, _params(model))]
    _assert_same_state(model, opt, plain_model, plain_opt)
    for (k, _p), e, w in zip(model.named_parameters(), _emas(model, opt), want):
        assert e.tobytes() == w.tobytes(), k
    assert "ema" not in plain_opt.state[next(iter(plain_model.parameters()))]
    raw, avg = _params(model), _emas(model, opt)
    raw_out = _forward(model, batches[0])
    with opt.averaged_parameters():
        for (k, _p), p, e in zip(model.named_parameters(), _params(model), avg):
            assert p.tobytes() == e.tobytes(), k               # every parameter's bytes are the average's
        inside = _forward(model, batches[0])
        loaded = {k: v.detach().clone() for k, v in model.state_dict().items()}
        for (k, _p), e in zip(model.named_parameters(), avg):
            loaded[k] = torch.from_numpy(e).to(dev)                # the averages as read from the optimizer before the swap
        fresh = _model(dev, state=loaded)
        assert torch.equal(inside, _forward(fresh, batches[0]))   # bit for bit the forward of a model that was never anything else
        assert not torch.equal(inside, raw_out)
        with pytest.raises(RuntimeError, match="average"):
            opt.step()
        with pytest.raises(RuntimeError, match="nest"):
            with opt.averaged_parameters():
                pass
        for p, e in zip(_params(model), avg):
            assert p.tobytes() == e.tobytes()                      # ... and neither refusal swapped anything
    for p, r in zip(_params(model), raw):
        assert p.tobytes() == r.tobytes()
    assert torch.equal(_forward(model, batches[0]), raw_out)
    with pytest.raises(KeyError):
        with opt.averaged_parameters():
            raise KeyError("the body fails")
    for p, r, e, a in zip(_params(model), raw, _emas(model, opt), avg):
        assert p.tobytes() == r.tobytes() and e.tobytes() == a.tobytes()
    # a further step after the swaps = a further step of a run that never swapped
    never_model, never_opt = _fresh(toy, ema_decay=DECAY)
    for b in batches:
        _one_step(never_model, never_opt, b)
    _one_step(model, opt, batches[0])
    _one_step(never_model, never_opt, batches[0])
    _assert_same_state(model, opt, never_model, never_opt, ema=True)


def test_state_dict_round_trip(toy):
    from taxoexpan_amd import optim
    dev, batches, _state = toy
    model, opt = _fresh(toy, ema_decay=DECAY)
    for b in batches[:2]:
        _one_step(model, opt, b)
    sd = copy.deepcopy(opt.state_dict())                          # (state_dict() hands out the live tensors: a checkpoint would copy them)
    assert all(sorted(st) == ["ema", "exp_avg", "exp_avg_sq", "max_exp_avg_sq", "step"] for st in sd["state"].values())
    twin = _model(dev, state={k: v.detach().clone() for k, v in model.state_dict().items()})
    twin_opt = optim.Adam(twin.parameters(), lr=1e-3, amsgrad=True, ema_decay=DECAY)
    twin_opt.load_state_dict(sd)
    _one_step(model, opt, batches[2])
    _one_step(twin, twin_opt, batches[2])
    _assert_same_state(model, opt, twin, twin_opt, ema=True)
    # a state without an average (a run that did not average) into an averaging optimizer: the average starts from the current parameter
    from taxoexpan_amd.optim import host_ema_update
    plain_model, plain_opt = _fresh(toy)
    for b in batches[:2]:
        _one_step(plain_model, plain_opt, b)
    late = _model(dev, state={k: v.detach().clone() for k, v in plain_model.state_dict().items()})
    late_opt = optim.Adam(late.parameters(), lr=1e-3, amsgrad=True, ema_decay=DECAY)
    late_opt.load_state_dict(copy.deepcopy(plain_opt.state_dict()))
    assert all("ema" not in st for st in late_opt.state.values())
    start = _params(late)
    _one_step(late, late_opt, batches[2])
    _one_step(plain_model, plain_opt, batches[2])
    _assert_same_state(late, late_opt, plain_model, plain_opt)
    for e, p0, p1 in zip(_emas(late, late_opt), start, _params(late)):
        assert e.tobytes() == host_ema_update(p0, p1, DECAY, np.float32).tobytes()


def test_warmup_schedule(toy):
    from taxoexpan_amd.optim import host_ema_update
    _dev_, batches, _state = toy
    model, opt = _fresh(toy, ema_decay=0.999, ema_warmup=True)
    want = _params(model)
    for b, d in zip(batches, (2.0 / 11.0, 3.0 / 12.0, 4.0 / 13.0)):
        _one_step(model, opt, b)
        want = [host_ema_update(e, p, d, np.float32) for e, p in zip(want, _params(model))]
        for e, w in zip(_emas(model, opt), want):
            assert e.tobytes() == w.tobytes(), d


def test_train_epoch_freezes_the_averages_with_the_run(toy):
    """the loss is inf from its 3rd call on (step s = 2): parameters, moments, averages and step counts are those of a run stopped
    after step 1 -- with warm-up, so that the NEXT step's decay (4/13 of update 3, not 5/14) shows the discounted count"""
    from taxoexpan_amd.optim import host_ema_update
    from taxoexpan_amd.trainer import train_epoch
    _dev_, batches, _state = toy
    adam = dict(ema_decay=0.999, ema_warmup=True)
    model, opt = _fresh(toy, **adam)
    loss_fn, _calls = _inf_from_call(3)
    got = train_epoch(model, _Replay(batches), opt, loss_fn=loss_fn, group_size=4, freeze_on_nonfinite=True)
    assert got["first_nonfinite"] == 2 and got["n_batches"] == STEPS
    two_model, two_opt = _fresh(toy, **adam)
    train_epoch(two_model, _Replay(batches[:2]), two_opt, group_size=4)
    _assert_same_state(model, opt, two_model, two_opt, ema=True)
    assert all(float(st["step"]) == 2 for st in opt.state.values())
    before = _emas(model, opt)
    train_epoch(model, _Replay(batches[2:]), opt, group_size=4)
    for e, b, p in zip(_emas(model, opt), before, _params(model)):
        assert e.tobytes() == host_ema_update(b, p, 4.0 / 13.0, np.float32).tobytes()


def test_fit_averaged(toy, tmp_path):
    from taxoexpan_amd.trainer import fit, load_averaged
    dev, batches, _state = toy
    seen = []

    def spy_validate(model, loader, metrics, larger_is_better):
        """records the first parameter's bytes; the metric is a function of them, so the log shows which weights were validated"""
        first = next(iter(model.parameters())).detach().double().cpu().numpy().copy()
        seen.append(first)
        return {"val_metrics": [float(np.abs(first).sum())]}

    kw = dict(metrics=["spy"], monitor="min val_spy", group_size=4, validate_fn=spy_validate, averaged=True)
    model, opt = _fresh(toy, ema_decay=DECAY)
    logs = fit(model, _Replay(batches), "valid", opt, 2, save_dir=tmp_path / "run", **kw)
    assert [l["epoch"] for l in logs] == [1, 2] and len(seen) == 2
    first_e = opt.state[next(iter(model.parameters()))]["ema"].detach().double().cpu().numpy()
    first_p = next(iter(model.parameters())).detach().double().cpu().numpy()
    assert seen[1].tobytes() == first_e.tobytes() and seen[1].tobytes() != first_p.tobytes()      # the spy saw the average ...
    assert logs[1]["val_spy"] == float(np.abs(first_e).sum()) != float(np.abs(first_p).sum())     # ... and the log follows it
    ck = torch.load(tmp_path / "run" / "checkpoint-epoch2.pth", map_location="cpu", weights_only=False)
    assert sorted(ck) == ["arch", "config", "ema_state_dict", "epoch", "monitor_best", "optimizer", "state_dict"]
    for (k, p), e in zip(model.named_parameters(), _emas(model, opt)):
        assert ck["ema_state_dict"][k].numpy().tobytes() == e.tobytes(), k
        assert ck["state_dict"][k].numpy().tobytes() == p.detach().cpu().numpy().tobytes(), k
    assert "ema_state_dict" in torch.load(tmp_path / "run" / "model_best.pth", map_location="cpu", weights_only=False)
    # resume from epoch 1 + one more epoch = the uninterrupted run
    model_r, opt_r = _fresh(toy, ema_decay=DECAY)
    logs_r = fit(model_r, _Replay(batches), "valid", opt_r, 2, resume=tmp_path / "run" / "checkpoint-epoch1.pth", **kw)
    assert [l["epoch"] for l in logs_r] == [2] and logs_r[0]["losses"].tobytes() == logs[1]["losses"].tobytes()
    assert logs_r[0]["val_spy"] == logs[1]["val_spy"]
    _assert_same_state(model, opt, model_r, opt_r, ema=True)
    # load_averaged: the averaged model; a checkpoint written without averaging has none
    avg_model = _model(dev)
    load_averaged(avg_model, tmp_path / "run" / "checkpoint-epoch2.pth")
    for (k, q), e in zip(avg_model.named_parameters(), _emas(model, opt)):
        assert q.detach().cpu().numpy().tobytes() == e.tobytes(), k
    with opt.averaged_parameters():
        assert torch.equal(_forward(model, batches[0]), _forward(avg_model, batches[0]))
    plain_model, plain_opt = _fresh(toy, ema_decay=DECAY)
    fit(plain_model, _Replay(batches), None, plain_opt, 1, monitor="off", group_size=4, save_dir=tmp_path / "plain")
    ck = torch.load(tmp_path / "plain" / "checkpoint-epoch1.pth", map_location="cpu", weights_only=False)
    assert sorted(ck) == ["arch", "config", "epoch", "monitor_best", "optimizer", "state_dict"]
    with pytest.raises(ValueError, match="ema_state_dict"):
        load_averaged(_model(dev), tmp_path / "plain" / "checkpoint-epoch1.pth")


def test_fit_averaged_needs_an_averaging_optimizer(toy):
    from taxoexpan_amd.trainer import fit
    dev, batches, state = toy
    model, opt = _fresh(toy)
    with pytest.raises(ValueError, match="ema_decay"):
        fit(model, _Replay(batches), None, opt, 1, monitor="off", group_size=4, averaged=True)
    for k, p in model.named_parameters():
        assert torch.equal(p, state[k]), k
    assert len(opt.state) == 0


def test_fit_freezes_and_saves_the_averages(toy, tmp_path):
    """last_finite.pth of an averaged run carries the averages of the last finite step"""
    from taxoexpan_amd.trainer import TrainingDiverged, fit, train_epoch
    _dev_, batches, _state = toy
    model, opt = _fresh(toy, ema_decay=DECAY)
    loss_fn, _calls = _inf_from_call(3)
    with pytest.raises(TrainingDiverged) as e:
        fit(model, _Replay(batches), None, opt, 1, monitor="off", save_dir=tmp_path / "run", loss_fn=loss_fn, group_size=4,
            freeze_on_nonfinite=True, averaged=True)
    ck = torch.load(e.value.checkpoint, map_location="cpu", weights_only=False)
    two_model, two_opt = _fresh(toy, ema_decay=DECAY)
    train_epoch(two_model, _Replay(batches[:2]), two_opt, group_size=4)
    for (k, p), a in zip(two_model.named_parameters(), _emas(two_model, two_opt)):
        assert ck["ema_state_dict"][k].numpy().tobytes() == a.tobytes(), k
        assert ck["state_dict"][k].numpy().tobytes() == p.detach().cpu().numpy().tobytes(), k
