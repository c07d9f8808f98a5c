"""CPU: optim.host_guarded_adam (the written definition of txe_adam_step_guarded) against a plain numpy Adam / AMSGrad step, its clip
coefficient at the edges and its frozen call; the argument checks of optim.Adam(max_grad_norm=...), StepGuard and the new C entry point
(they return before any launch); discount_frozen_steps on a state built by hand; and trainer.fit forwarding max_grad_norm /
freeze_on_nonfinite to its train_epoch and writing last_finite.pth for a diverged epoch."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch


def _draw(n=301, seed=3, second_step=True):
    rng = np.random.RandomState(seed)
    p, g = rng.randn(n).astype(np.float32), (rng.randn(n) * 10.0 ** rng.randint(-3, 3, n)).astype(np.float32)
    if second_step:                                          # moments of an earlier step; vmax >= v, as AMSGrad keeps it
        m, v = (0.1 * rng.randn(n)).astype(np.float32), (rng.rand(n) ** 2).astype(np.float32)
        vmax = np.maximum(v, rng.rand(n).astype(np.float32))
    else:
        m, v, vmax = (np.zeros(n, np.float32) for _ in range(3))
    return p, g, m, v, vmax


def _plain_adam(p, g, m, v, vmax, lr, b1, b2, eps, wd, step, dtype):
    """torch.optim.Adam's single-tensor update in plain numpy, independent of the restatement's helpers.  In float32 the kernel fuses
    three products into their sums (fmaf); here each of those is formed in float64 -- where the product of two fp32 numbers is exact --
    and rounded to fp32 once (this differs from fmaf only when the fp64 sum lands on an fp32 tie: not on these fixed draws)"""
    f = dtype
    w = np.float64
    p, g, m, v = (a.astype(f) for a in (p, g, m, v))
    omb1, omb2, b2_ = f(1 - b1), f(1 - b2), f(b2)
    g = (w(f(wd)) * p.astype(w) + g.astype(w)).astype(f)
    m = (w(omb1) * (g - m).astype(w) + m.astype(w)).astype(f)
    v = (g.astype(w) * (omb2 * g).astype(w) + (b2_ * v).astype(w)).astype(f)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    if vmax is not None:
        vmax = np.maximum(vmax.astype(f), v)
    d = np.sqrt(v if vmax is None else vmax) / f(math.sqrt(bc2)) + f(eps)
    return p - f(lr / bc1) * m / d, m, v, vmax


@pytest.mark.parametrize("amsgrad", [True, False])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("step", [1, 2])
def test_host_guarded_adam_without_a_guard_is_a_plain_adam_step(amsgrad, wd, step):
    from taxoexpan_amd.optim import host_guarded_adam
    p, g, m, v, vmax = _draw(second_step=step > 1)
    hyper = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=wd, step=step)
    before = [a.copy() for a in (p, g, m, v, vmax)]
    got32 = host_guarded_adam(p, g, m, v, vmax if amsgrad else None, dtype=np.float32, **hyper)
    got64 = host_guarded_adam(p, g, m, v, vmax if amsgrad else None, dtype=np.float64, **hyper)
    assert all(np.array_equal(a, b) for a, b in zip((p, g, m, v, vmax), before))                 # no argument is changed
    want64 = _plain_adam(p, g, m, v, vmax if amsgrad else None, 1e-2, 0.9, 0.999, 1e-8, wd, step, np.float64)
    want32 = _plain_adam(p, g, m, v, vmax if amsgrad else None, 1e-2, 0.9, 0.999, 1e-8, wd, step, np.float32)
    for name, a32, a64, w32, w64 in zip("p m v vmax".split(), got32, got64, want32, want64):
        if a32 is None:
            assert name == "vmax" and not amsgrad and a64 is None
            continue
        assert a32.dtype == np.float32 and a64.dtype == np.float64
        assert a32.tobytes() == w32.tobytes(), name                                              # float32: bit for bit
        # float64: one formula, the scalars (1 - beta1, lr / bc1, ...) formed the same way: equal, or apart by fp64 rounding alone
        np.testing.assert_allclose(a64, w64, rtol=1e-12, atol=1e-300, err_msg=name)
    # a coefficient of exactly 1 (the norm is below the threshold) changes no bit; neither does a first_bad of -1
    same = host_guarded_adam(p, g, m, v, vmax if amsgrad else None, gnorm2=4.0, first_bad=-1, max_grad_norm=3.0, dtype=np.float32, **hyper)
    assert all((a is None and b is None) or a.tobytes() == b.tobytes() for a, b in zip(same, got32))


def test_clip_coefficient_edges():
    """norm 0: coefficient 1; norm exactly max_grad_norm: below 1 by the 1e-6 term; just above: c / (norm + 1e-6); NaN: 1; +Inf: 0"""
    from taxoexpan_amd.optim import host_guarded_adam
    p, g, m, v, vmax = _draw(n=64)

    def run(gnorm2, c, dtype=np.float32, grad=g):
        return host_guarded_adam(p, grad, m, v, vmax, lr=1e-2, step=3, gnorm2=gnorm2, max_grad_norm=c, dtype=dtype)

    def scaled(coef, dtype=np.float32):
        return host_guarded_adam(p, (g.astype(dtype) * dtype(coef)), m, v, vmax, lr=1e-2, step=3, dtype=dtype)

    plain = scaled(1.0)
    for got in (run(0.0, 0.5), run(0.2499, 0.5), run(float("nan"), 0.5)):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, plain))
    at = 0.5 / (0.5 + 1e-6)                                  # sqrt(0.25) is exact
    assert at < 1.0 and np.float32(at) < np.float32(1.0)
    for dtype in (np.float32, np.float64):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(run(0.25, 0.5, dtype), scaled(at, dtype)))
        assert any(a.tobytes() != b.tobytes() for a, b in zip(run(0.25, 0.5, dtype), scaled(1.0, dtype)))
        above = 0.5 / (math.sqrt(0.2500001) + 1e-6)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(run(0.2500001, 0.5, dtype), scaled(above, dtype)))
        big = 0.5 / (math.sqrt(2500.0) + 1e-6)               # a hundred times the threshold
        assert all(a.tobytes() == b.tobytes() for a, b in zip(run(2500.0, 0.5, dtype), scaled(big, dtype)))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(run(float("inf"), 0.5), scaled(0.0)))
    with pytest.raises(ValueError):
        run(1.0, None)
    with pytest.raises(ValueError):
        run(1.0, 0.0)
    with pytest.raises(ValueError):
        host_guarded_adam(p, g, m, v, vmax, dtype=np.float16)


@pytest.mark.parametrize("amsgrad", [True, False])
def test_a_frozen_call_returns_its_inputs_unchanged(amsgrad):
    from taxoexpan_amd.optim import host_guarded_adam
    p, g, m, v, vmax = _draw()
    g[5], g[7] = np.nan, np.inf
    for first_bad in (0, 3):
        for kw in (dict(), dict(gnorm2=float("nan"), max_grad_norm=1.0)):
            got = host_guarded_adam(p, g, m, v, vmax if amsgrad else None, first_bad=first_bad, step=4, **kw)
            assert got[0].tobytes() == p.tobytes() and got[1].tobytes() == m.tobytes() and got[2].tobytes() == v.tobytes()
            assert (got[3].tobytes() == vmax.tobytes()) if amsgrad else got[3] is None
            assert got[0] is not p
    assert np.isnan(host_guarded_adam(p, g, m, v, vmax, first_bad=-1)[0][5])         # -1: the step is taken, NaN and all


def test_adam_and_step_guard_check_max_grad_norm():
    from taxoexpan_amd import optim
    w = torch.nn.Parameter(torch.zeros(3))
    plain = optim.Adam([w])                                  # not asked for: the groups and the state_dict are what they were
    assert "max_grad_norm" not in plain.param_groups[0] and "max_grad_norm" not in plain.defaults
    assert plain.state_dict()["param_groups"][0].keys() == {"lr", "betas", "eps", "weight_decay", "amsgrad", "params"}
    assert optim.Adam([w], max_grad_norm=2).param_groups[0]["max_grad_norm"] == 2.0
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match="max_grad_norm"):
            optim.Adam([w], max_grad_norm=bad)
        with pytest.raises(ValueError, match="max_grad_norm"):
            optim.StepGuard(max_grad_norm=bad)
    # the state_dict keeps torch's layout: the new key sits in the param group, and a group saved without it loads as None
    opt = optim.Adam([w], lr=0.1, max_grad_norm=0.5)
    sd = opt.state_dict()
    assert sorted(sd) == ["param_groups", "state"] and sd["param_groups"][0]["max_grad_norm"] == 0.5
    old = torch.optim.Adam([w], lr=0.1).state_dict()
    assert "max_grad_norm" not in old["param_groups"][0]
    opt.__setstate__({"state": {}, "param_groups": [dict(old["param_groups"][0], params=[w])], "defaults": opt.defaults})
    assert opt.param_groups[0]["max_grad_norm"] is None
    torch.optim.Adam([w], lr=0.1).load_state_dict(sd)                                 # ... and torch's class takes ours
    # a threshold without a norm to clip by is refused before anything is launched (no GPU is touched: the check comes first)
    w.grad = torch.ones(3)
    with pytest.raises(RuntimeError, match="no guard"):
        optim.Adam([w], max_grad_norm=1.0).step()
    with pytest.raises(RuntimeError, match="no guard"):
        optim.Adam([w], max_grad_norm=1.0).step(guard=optim.StepGuard(first_bad=1234))
    with pytest.raises(RuntimeError, match="no guard"):
        optim.Adam([w]).step(guard=optim.StepGuard(first_bad=1234, max_grad_norm=1.0))


def test_discount_frozen_steps():
    from taxoexpan_amd import optim
    ws = [torch.nn.Parameter(torch.zeros(n)) for n in (3, 1, 2)]
    opt = optim.Adam(ws, amsgrad=True)
    for w, k in zip(ws, (9.0, 2.0, 0.0)):
        opt.state[w] = dict(step=torch.tensor(k), exp_avg=torch.ones_like(w), exp_avg_sq=torch.ones_like(w), max_exp_avg_sq=torch.ones_like(w))
    opt.discount_frozen_steps(0)
    assert [float(opt.state[w]["step"]) for w in ws] == [9.0, 2.0, 0.0]
    opt.discount_frozen_steps(3)
    assert [float(opt.state[w]["step"]) for w in ws] == [6.0, 0.0, 0.0]             # never below 0
    assert all(torch.is_tensor(opt.state[w]["step"]) and opt.state[w]["step"].dtype == torch.float32 for w in ws)
    assert all(torch.equal(opt.state[w][k], torch.ones_like(w)) for w in ws for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"))
    opt.state[ws[0]]["step"] = 5                                                      # a plain number, as old checkpoints hold
    opt.discount_frozen_steps(7)
    assert opt.state[ws[0]]["step"] == 0
    with pytest.raises(ValueError):
        opt.discount_frozen_steps(-1)


def test_guarded_entry_point_checks_its_arguments_without_a_gpu():
    """every refusal of txe_adam_step_guarded comes before any launch (a host buffer stands in for the device pointers: never read)"""
    from taxoexpan_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 8)()
    a = ctypes.addressof(buf)
    tab, numel = (ctypes.c_void_p * 2)(a, a), (ctypes.c_longlong * 2)(5, 7)
    good = dict(n=2, p=tab, g=tab, m=tab, v=tab, x=tab, numel=numel, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, step=1, gnorm2=a,
                first_bad=a, max_grad_norm=1.0, stream=None)
    call = lambda **kw: lib.txe_adam_step_guarded(*dict(good, **kw).values())
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(max_grad_norm=bad) == -1, bad
        assert call(max_grad_norm=bad, first_bad=None) == -1, bad
    for name in ("p", "g", "m", "v", "numel"):
        assert call(**{name: None}) == -1, name
        assert call(**{name: None}, gnorm2=None, first_bad=None) == -1, name
    assert call(n=-1) == -1 and call(step=0) == -1 and call(b1=1.0) == -1 and call(b2=-0.1) == -1
    assert call(numel=(ctypes.c_longlong * 2)(5, -1)) == -1 and call(p=(ctypes.c_void_p * 2)(None, a)) == -1
    assert call(x=(ctypes.c_void_p * 2)(a, None)) == -1
    # nothing to update: no launch, whatever the guard; and max_grad_norm is not looked at without a gnorm2
    assert call(n=0) == 0 and call(n=0, gnorm2=None, max_grad_norm=float("nan")) == 0
    assert call(numel=(ctypes.c_longlong * 2)(0, 0), gnorm2=None, max_grad_norm=-1.0) == 0


# ---- fit ---------------------------------------------------------------------------------------------------------------------------

class _Epochs:
    """a train_epoch stand-in that records what fit passes it; epoch `bad_epoch` reports a non-finite step 2"""

    def __init__(self, bad_epoch=None, strict=False):
        self.bad_epoch, self.calls = bad_epoch, []
        if strict:                                           # the old signature: fit must not pass what was not asked for
            self.fn = lambda model, loader, optimizer, loss_fn=None, group_size=None: self._run({})
        else:
            self.fn = lambda model, loader, optimizer, loss_fn=None, group_size=None, **kw: self._run(kw)

    def _run(self, kw):
        self.calls.append(kw)
        bad = len(self.calls) == self.bad_epoch
        return dict(loss=1.0, n_batches=4, losses=np.ones(4, np.float32), grad_norms=np.ones(4), first_nonfinite=2 if bad else -1)


def _validate(model, loader, metrics=None, larger_is_better=True):
    return dict(val_metrics=[1.0] * len(metrics), n_batches=1, n_groups=1, n_positives=1)


def _fit(epochs_fn, n, **kw):
    from taxoexpan_amd.trainer import fit
    model = torch.nn.Linear(3, 2)
    opt = torch.optim.Adam(model.parameters(), lr=0.5)
    return fit(model, [None], [None], opt, n, metrics=("macro_mr",), train_epoch_fn=epochs_fn.fn, validate_fn=_validate, **kw), model, opt


def test_fit_forwards_the_guard_arguments():
    e = _Epochs(strict=True)
    _fit(e, 2)                                               # nothing asked for: the old call, keyword for keyword
    assert e.calls == [{}, {}]
    e = _Epochs()
    _fit(e, 2, max_grad_norm=0.25)
    assert e.calls == [dict(max_grad_norm=0.25)] * 2
    e = _Epochs()
    _fit(e, 1, freeze_on_nonfinite=True)
    assert e.calls == [dict(freeze_on_nonfinite=True)]
    e = _Epochs()
    _fit(e, 1, max_grad_norm=3.0, freeze_on_nonfinite=True)
    assert e.calls == [dict(max_grad_norm=3.0, freeze_on_nonfinite=True)]


def test_fit_writes_last_finite_for_a_diverged_epoch(tmp_path):
    from taxoexpan_amd.trainer import TrainingDiverged
    with pytest.raises(TrainingDiverged) as e:
        _fit(_Epochs(bad_epoch=3), 5, save_dir=tmp_path / "run", freeze_on_nonfinite=True, config={"name": "x"})
    assert (e.value.epoch, e.value.step) == (3, 2)
    assert e.value.checkpoint == os.path.join(str(tmp_path / "run"), "last_finite.pth")
    assert sorted(os.listdir(tmp_path / "run")) == ["checkpoint-epoch1.pth", "checkpoint-epoch2.pth", "last_finite.pth", "model_best.pth"]
    ck = torch.load(e.value.checkpoint, weights_only=False)
    assert sorted(ck) == ["arch", "config", "epoch", "monitor_best", "optimizer", "state_dict"]
    assert ck["epoch"] == 2 and ck["arch"] == "Linear" and ck["monitor_best"] == 1.0 and ck["config"] == {"name": "x"}
    assert sorted(ck["optimizer"]) == ["param_groups", "state"]
    # the first epoch diverges: `epoch` 0, so that a resumed run starts at epoch 1
    with pytest.raises(TrainingDiverged) as e:
        _fit(_Epochs(bad_epoch=1), 5, save_dir=tmp_path / "first", freeze_on_nonfinite=True)
    assert torch.load(e.value.checkpoint, weights_only=False)["epoch"] == 0
    resumed = _Epochs()
    logs, _m, _o = _fit(resumed, 2, resume=e.value.checkpoint)
    assert [l["epoch"] for l in logs] == [1, 2]
    # without the flag, or without a save_dir, nothing is written and .checkpoint is None (the state is not the last finite one)
    with pytest.raises(TrainingDiverged) as e:
        _fit(_Epochs(bad_epoch=1), 5, save_dir=tmp_path / "plain")
    assert e.value.checkpoint is None and not os.path.exists(tmp_path / "plain" / "last_finite.pth")
    with pytest.raises(TrainingDiverged) as e:
        _fit(_Epochs(bad_epoch=1), 5, freeze_on_nonfinite=True)
    assert e.value.checkpoint is None


def test_train_epoch_refuses_an_optimizer_without_a_guard_before_any_step():
    from taxoexpan_amd import trainer
    model = torch.nn.Linear(2, 1)
    before = [p.detach().clone() for p in model.parameters()]
    for kw in (dict(max_grad_norm=1.0), dict(freeze_on_nonfinite=True)):
        with pytest.raises(ValueError, match="guard"):
            trainer.train_epoch(model, [], torch.optim.Adam(model.parameters(), lr=0.1), group_size=4, **kw)
    with pytest.raises(ValueError, match="max_grad_norm"):
        trainer.train_epoch(model, [], torch.optim.Adam(model.parameters(), lr=0.1), group_size=4, max_grad_norm=0.0)
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), before))
    assert trainer.TrainingDiverged(1, 2).checkpoint is None
