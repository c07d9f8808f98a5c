"""GPU: txe_adam_step_guarded through the C ABI -- bit-equal to txe_adam_step while the guard is inactive, frozen by first_bad (26
tensors: two launches; NaN and Inf gradients), clipping against optim.host_guarded_adam in float64 beside the fp32 literal route
(clip_grad_norm_, then torch.optim.Adam), the clip coefficient's edges bit for bit against the float32 restatement -- and the loop:
trainer.train_epoch(max_grad_norm=..., freeze_on_nonfinite=...) and trainer.fit with last_finite.pth and resume.

Gate of the clipping tests, the project's usual one (golden_util.gate_against_f64 with its defaults): max |HIP - f64| <= 2 x max |fp32
literal route - f64|, floored at 2e-5 of the tensor's largest float64 entry.  Every gate prints its pair.  Measured on the MI355X
(profiles/NOTES.md): kernel test, worst tensor and buffer over all cases: HIP 2.4e-7, literal route 2.5e-7 of the largest entry (both
in exp_avg_sq at step 2); loop test, worst parameter after 6 clipped steps: HIP 1.7e-7, literal loop 1.7e-7 -- the 2e-5 floor decides
everywhere."""
import ctypes
import math

import numpy as np
import pytest
import torch

from golden_util import gate_against_f64
from test_gpu_trainer import _dev, _model, _recorded_batches, _Replay

pytestmark = pytest.mark.gpu

# 3: one partial float4; 1023 / 1024 / 1025: the workgroup's chunk less one, exactly, plus one (a second workgroup with one element);
# 4097: five workgroups, the last with one element; 1030 (below): a view 4 bytes into its allocation, which takes the scalar path
SIZES = [3, 1023, 1024, 1025, 4097]
UNALIGNED = 1030
CASES = [(True, 0.0), (False, 0.0), (True, 0.01), (False, 0.01)]          # (amsgrad, weight_decay)
HYPER = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)
BUFFERS = ("p", "m", "v", "x")


def _host_draw(sizes, seed, steps=2):
    """parameters, and per step one gradient per tensor (of very unequal scale from tensor to tensor)"""
    rng = np.random.RandomState(seed)
    p = [rng.randn(n).astype(np.float32) for n in sizes]
    g = [[(rng.randn(n) * 10.0 ** rng.randint(-2, 2)).astype(np.float32) for n in sizes] for _ in range(steps)]
    return p, g


def _gnorm2(grads):
    return float(sum(np.sum(g.astype(np.float64) ** 2) for g in grads))


def _dev_array(a, dev, unaligned):
    if not unaligned:
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    base = torch.zeros(a.size + 1, dtype=torch.float32, device=dev)
    base[1:] = torch.from_numpy(a).to(dev)
    assert base[1:].data_ptr() % 16 == 4
    return base[1:]


class _Tensors:
    """device copies of a parameter set with zero moments, and the raw entry points (return code, nothing raised)"""

    def __init__(self, host_p, dev, unaligned=()):
        from taxoexpan_amd import _lib
        self._lib, self.lib, self.dev, self.unaligned = _lib, _lib.load(), dev, set(unaligned)
        self.p = [_dev_array(a, dev, i in self.unaligned) for i, a in enumerate(host_p)]
        self.m, self.v, self.x = ([_dev_array(np.zeros_like(a), dev, i in self.unaligned) for i, a in enumerate(host_p)] for _ in range(3))
        self.n = (ctypes.c_longlong * len(host_p))(*[a.size for a in host_p])

    @staticmethod
    def _tab(ts):
        return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    def step(self, host_g, step, ams, wd, guarded, gnorm2=None, first_bad=None, max_grad_norm=0.0):
        g = [_dev_array(a, self.dev, i in self.unaligned) for i, a in enumerate(host_g)]
        args = [len(self.p), self._tab(self.p), self._tab(g), self._tab(self.m), self._tab(self.v), self._tab(self.x) if ams else None, self.n,
                HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], wd, step]
        if guarded:
            rc = self.lib.txe_adam_step_guarded(*args, None if gnorm2 is None else gnorm2.data_ptr(),
                                                None if first_bad is None else first_bad.data_ptr(), max_grad_norm, self._lib.stream_ptr())
        else:
            rc = self.lib.txe_adam_step(*args, self._lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        return g

    def host(self):
        return {k: [t.cpu().numpy().copy() for t in getattr(self, k)] for k in BUFFERS}


def _assert_same_bits(a, b, what):
    for k in BUFFERS:
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert x.tobytes() == y.tobytes(), f"{what}: buffer {k} of tensor {i} ({x.size} elements) differs"


def _scalars(dev, gnorm2, first_bad):
    return torch.tensor([gnorm2], dtype=torch.float64, device=dev), torch.tensor([first_bad], dtype=torch.int64, device=dev)


@pytest.mark.parametrize("ams,wd", CASES)
def test_inactive_guard_is_bit_equal_to_the_unguarded_step(ams, wd):
    """first_bad = -1 and a norm below the threshold (coefficient 1, and g * 1.0f is g): the same bits as txe_adam_step, over two steps
    (the second with other bias corrections); so are both pointers NULL, and either pointer alone"""
    dev = _dev()
    sizes = SIZES + [UNALIGNED]
    host_p, host_g = _host_draw(sizes, seed=1)
    runs = {name: _Tensors(host_p, dev, unaligned=[5]) for name in ("plain", "guarded", "null", "only_bad", "only_norm")}
    for s in (1, 2):
        g2 = _gnorm2(host_g[s - 1])
        gnorm2, first_bad = _scalars(dev, g2, -1)
        c = 2.0 * math.sqrt(g2)                                # the norm is half the threshold
        runs["plain"].step(host_g[s - 1], s, ams, wd, guarded=False)
        runs["guarded"].step(host_g[s - 1], s, ams, wd, True, gnorm2, first_bad, c)
        runs["null"].step(host_g[s - 1], s, ams, wd, True)
        runs["only_bad"].step(host_g[s - 1], s, ams, wd, True, None, first_bad, float("nan"))       # max_grad_norm is ignored without gnorm2
        runs["only_norm"].step(host_g[s - 1], s, ams, wd, True, gnorm2, None, c)
        assert gnorm2.item() == g2 and first_bad.item() == -1                                       # read, never written
        want = runs["plain"].host()
        assert all(np.isfinite(a).all() for a in want["p"]) and any((a != b).any() for a, b in zip(want["p"], host_p))
        for name in ("guarded", "null", "only_bad", "only_norm"):
            _assert_same_bits(runs[name].host(), want, f"{name}, step {s}")
        if not ams:
            assert all(not a.any() for a in want["x"])         # plain Adam never touches max_exp_avg_sq


@pytest.mark.parametrize("ams", [True, False])
def test_frozen_step_touches_nothing(ams):
    """first_bad = 0, gradients with NaN and Inf in them (ordinary data), 26 tensors = two launches: every buffer of every tensor keeps
    its bits, with and without a gnorm2 pointer (whose NaN is never used), from a state that one real step has made non-trivial"""
    dev = _dev()
    sizes = SIZES + [UNALIGNED] + [1 + 37 * k for k in range(20)]
    assert len(sizes) == 26
    host_p, host_g = _host_draw(sizes, seed=2)
    t = _Tensors(host_p, dev, unaligned=[5])
    t.step(host_g[0], 1, ams, 0.01, guarded=False)
    before = t.host()
    bad = [g.copy() for g in host_g[1]]
    for i, g in enumerate(bad):
        g[0], g[-1] = np.nan, np.inf if i % 2 else -np.inf
    gnorm2, first_bad = _scalars(dev, float("nan"), 0)
    t.step(bad, 2, ams, 0.01, True, gnorm2, first_bad, 1.0)
    _assert_same_bits(t.host(), before, "frozen, with a norm")
    t.step(bad, 2, ams, 0.01, True, None, first_bad, 0.0)
    _assert_same_bits(t.host(), before, "frozen, without a norm")
    assert first_bad.item() == 0 and math.isnan(gnorm2.item())
    first_bad.fill_(7)                                         # any step >= 0, not only 0
    t.step(bad, 2, ams, 0.01, True, gnorm2, first_bad, 1.0)
    _assert_same_bits(t.host(), before, "frozen at step 7")
    first_bad.fill_(-1)                                        # ... and -1 lets the (finite) step through again, in both launches
    t.step(host_g[1], 2, ams, 0.01, True, None, first_bad, 0.0)
    after = t.host()
    assert all((a != b).any() for a, b in zip(after["p"], before["p"]))


def _literal_route(host_p, dev, ams, wd):
    ps = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev)) for a in host_p]
    return ps, torch.optim.Adam(ps, lr=HYPER["lr"], betas=(HYPER["beta1"], HYPER["beta2"]), eps=HYPER["eps"], weight_decay=wd, amsgrad=ams)


@pytest.mark.parametrize("ams,wd", CASES)
def test_active_clip_against_the_float64_restatement(ams, wd):
    """the norm is 3 times the threshold at step 1 and 100 times at step 2.  Reference: host_guarded_adam in float64, iterated on its
    own state; yardstick: clip_grad_norm_ then torch.optim.Adam in fp32 on the device, on its own state; gate: see the module docstring"""
    from taxoexpan_amd.optim import host_guarded_adam
    dev = _dev()
    sizes = SIZES + [UNALIGNED]
    host_p, host_g = _host_draw(sizes, seed=3)
    hip = _Tensors(host_p, dev, unaligned=[5])
    lit_p, lit_opt = _literal_route(host_p, dev, ams, wd)
    ref = dict(p=[a.astype(np.float64) for a in host_p], m=[np.zeros(n) for n in sizes], v=[np.zeros(n) for n in sizes],
               x=[np.zeros(n) for n in sizes])
    errors, report = [], []
    for s, factor in ((1, 3.0), (2, 100.0)):
        g2 = _gnorm2(host_g[s - 1])
        c = math.sqrt(g2) / factor
        gnorm2, first_bad = _scalars(dev, g2, -1)
        grads = hip.step(host_g[s - 1], s, ams, wd, True, gnorm2, first_bad, c)
        assert all(np.array_equal(g.cpu().numpy(), h) for g, h in zip(grads, host_g[s - 1]))        # the gradients are not rewritten
        for p, g in zip(lit_p, host_g[s - 1]):
            p.grad = torch.from_numpy(g.copy()).to(dev)
        total = torch.nn.utils.clip_grad_norm_(lit_p, c)
        assert abs(float(total) - math.sqrt(g2)) <= 1e-5 * math.sqrt(g2)
        lit_opt.step()
        for i in range(len(sizes)):
            ref["p"][i], ref["m"][i], ref["v"][i], x = host_guarded_adam(
                ref["p"][i], host_g[s - 1][i], ref["m"][i], ref["v"][i], ref["x"][i] if ams else None, weight_decay=wd, step=s, gnorm2=g2,
                max_grad_norm=c, dtype=np.float64, **HYPER)
            if ams:
                ref["x"][i] = x
        got = hip.host()
        for i, p in enumerate(lit_p):
            st = lit_opt.state[p]
            yard = dict(p=p.detach(), m=st["exp_avg"], v=st["exp_avg_sq"], x=st["max_exp_avg_sq"] if ams else None)
            for k in BUFFERS[:4 if ams else 3]:
                gate_against_f64(got[k][i], ref[k][i], yard[k].cpu().numpy(), f"step {s} tensor {i} ({sizes[i]}) {k}", errors, report)
    worst = max(report, key=lambda r: r[1])
    print(f"\n[gate] guarded adam ams={ams} wd={wd}: worst HIP error {worst[1]:.3e} ({worst[0]}; yardstick there {worst[2]:.3e}), "
          f"worst yardstick error {max(r[2] for r in report):.3e} (fractions of the tensor's largest float64 entry)")
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("ams,wd", CASES)
def test_clip_coefficient_edges_bit_for_bit(ams, wd):
    """gnorm2 = 0: coefficient 1; gnorm2 = max_grad_norm^2 exactly (0.25 and 0.5: the square root is exact): the coefficient is
    0.5 / (0.5 + 1e-6) < 1.  Both against the float32 restatement, which is the kernel operation for operation: the same bits"""
    from taxoexpan_amd.optim import host_guarded_adam
    dev = _dev()
    sizes = SIZES + [UNALIGNED]
    host_p, host_g = _host_draw(sizes, seed=4)
    for g2, clipped in ((0.0, False), (0.25, True)):
        hip = _Tensors(host_p, dev, unaligned=[5])
        want = dict(p=[a.copy() for a in host_p], m=[np.zeros(n, np.float32) for n in sizes], v=[np.zeros(n, np.float32) for n in sizes],
                    x=[np.zeros(n, np.float32) for n in sizes])
        free = {k: [a.copy() for a in v] for k, v in want.items()}
        for s in (1, 2):
            gnorm2, first_bad = _scalars(dev, g2, -1)
            hip.step(host_g[s - 1], s, ams, wd, True, gnorm2, first_bad, 0.5)
            for state, kw in ((want, dict(gnorm2=g2, max_grad_norm=0.5)), (free, dict())):
                for i in range(len(sizes)):
                    state["p"][i], state["m"][i], state["v"][i], x = host_guarded_adam(
                        state["p"][i], host_g[s - 1][i], state["m"][i], state["v"][i], state["x"][i] if ams else None, weight_decay=wd,
                        step=s, dtype=np.float32, **HYPER, **kw)
                    if ams:
                        state["x"][i] = x
            _assert_same_bits(hip.host(), want, f"gnorm2 {g2}, step {s}")
        differs = any(a.tobytes() != b.tobytes() for a, b in zip(want["m"], free["m"]))
        assert differs == clipped                              # 0: the unclipped step exactly; max^2: below it by the 1e-6 term


# ---- the loop ----------------------------------------------------------------------------------------------------------------------

STEPS = 6


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    """6 recorded training batches of the toy loader and the model's initial state (dropout 0 everywhere: no seeds to keep in step)"""
    dev = _dev()
    rec = _recorded_batches(tmp_path_factory.mktemp("toy"), dev, STEPS)
    state = {k: v.detach().clone() for k, v in _model(dev).state_dict().items()}
    return dev, [r[0] for r in rec], state


def _fresh(toy, **adam):
    from taxoexpan_amd import optim
    dev, batches, state = toy
    model = _model(dev, state=state)
    return model, optim.Adam(model.parameters(), lr=1e-3, amsgrad=True, **adam)


def _opt_state(opt):
    return [(float(st["step"]), st["exp_avg"], st["exp_avg_sq"], st["max_exp_avg_sq"]) for st in (opt.state[p] for p in opt.param_groups[0]["params"])]


def _assert_same_run(model_a, opt_a, model_b, opt_b):
    for (k, p), q in zip(model_a.named_parameters(), model_b.parameters()):
        assert torch.equal(p, q), k
    for a, b in zip(_opt_state(opt_a), _opt_state(opt_b)):
        assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))


def test_train_epoch_with_a_clip_that_never_acts_changes_no_bit(toy):
    from taxoexpan_amd.trainer import train_epoch
    _dev_, batches, _state = toy
    model_a, opt_a = _fresh(toy)
    model_b, opt_b = _fresh(toy)
    model_c, opt_c = _fresh(toy, max_grad_norm=1e6)            # the threshold as the optimizer's own
    plain = train_epoch(model_a, _Replay(batches), opt_a, group_size=4)
    got = train_epoch(model_b, _Replay(batches), opt_b, group_size=4, max_grad_norm=1e6, freeze_on_nonfinite=True)
    own = train_epoch(model_c, _Replay(batches), opt_c, group_size=4)
    assert plain["first_nonfinite"] == -1 and plain["grad_norms"].max() < 1e6
    for r in (got, own):
        assert r["losses"].tobytes() == plain["losses"].tobytes() and r["grad_norms"].tobytes() == plain["grad_norms"].tobytes()
        assert r["first_nonfinite"] == -1 and r["n_batches"] == STEPS
    _assert_same_run(model_a, opt_a, model_b, opt_b)
    _assert_same_run(model_a, opt_a, model_c, opt_c)
    assert all(s[0] == STEPS for s in _opt_state(opt_b))


def test_train_epoch_clips_like_the_literal_loop(toy):
    """every step clips (c = a quarter of the smallest norm of an unclipped epoch; asserted on the clipped epoch's own norms).  Subject:
    train_epoch(max_grad_norm=c).  Yardstick: the literal loop -- backward, clip_grad_norm_, the unguarded optim.Adam.step() -- on the
    same batches.  Reference: host_guarded_adam in float64 iterated on the literal loop's recorded (unclipped) gradients."""
    from taxoexpan_amd import optim
    from taxoexpan_amd.loss import info_nce_loss
    from taxoexpan_amd.optim import host_guarded_adam
    from taxoexpan_amd.trainer import StepLog, train_epoch
    dev, batches, state = toy
    probe_model, probe_opt = _fresh(toy)
    c = 0.25 * float(train_epoch(probe_model, _Replay(batches), probe_opt, group_size=4)["grad_norms"].min())

    class Recording(optim.Adam):
        """optim.Adam that keeps a copy of the gradients as they are AFTER each step"""
        seen = None

        def step(self, closure=None, guard=None):
            out = super().step(closure, guard=guard)
            self.seen.append([p.grad.detach().clone() for p in self.param_groups[0]["params"]])
            return out

    model = _model(dev, state=state)
    opt = Recording(model.parameters(), lr=1e-3, amsgrad=True)
    opt.seen = []
    got = train_epoch(model, _Replay(batches), opt, group_size=4, max_grad_norm=c)
    assert got["first_nonfinite"] == -1 and (got["grad_norms"] > c).all(), (c, got["grad_norms"])
    # the returned norms are the norms before clipping: bit-equal to a log, with no optimizer anywhere near it, of the same gradients
    # (and the gradients themselves were still unscaled after the step)
    log = StepLog(dev, STEPS)
    holders = [torch.nn.Parameter(torch.empty_like(g)) for g in opt.seen[0]]
    for grads in opt.seen:
        for h, g in zip(holders, grads):
            h.grad = g
        log.record(torch.zeros((), device=dev), holders)
    assert log.read()["grad_norm"].tobytes() == got["grad_norms"].tobytes()
    # the literal loop, recording its gradients before it clips them
    lit = _model(dev, state=state)
    lit_opt = optim.Adam(lit.parameters(), lr=1e-3, amsgrad=True)
    lit.train()
    recorded = []
    for g, x, qf, _label in _Replay(batches):
        lit_opt.zero_grad()
        loss = info_nce_loss(lit(g, x, qf).reshape(-1, 4), None)
        loss.backward()
        recorded.append([p.grad.detach().cpu().numpy().copy() for p in lit.parameters()])
        torch.nn.utils.clip_grad_norm_(lit.parameters(), c)
        lit_opt.step()
    names = [k for k, _ in lit.named_parameters()]
    ref = [dict(p=state[k].cpu().numpy().astype(np.float64), m=0.0 * state[k].cpu().numpy().astype(np.float64)) for k in names]
    for r in ref:
        r["v"], r["x"] = r["m"].copy(), r["m"].copy()
    for s, grads in enumerate(recorded):
        g2 = float(sum(np.sum(g.astype(np.float64) ** 2) for g in grads))
        for r, g in zip(ref, grads):
            r["p"], r["m"], r["v"], r["x"] = host_guarded_adam(r["p"], g, r["m"], r["v"], r["x"], lr=1e-3, step=s + 1, gnorm2=g2, max_grad_norm=c,
                                                               dtype=np.float64)
    errors, report = [], []
    for k, r, p, q in zip(names, ref, model.parameters(), lit.parameters()):
        gate_against_f64(p.detach().cpu().numpy(), r["p"], q.detach().cpu().numpy(), k, errors, report)
    worst = max(report, key=lambda r: r[1])
    print(f"\n[gate] clipped loop, {STEPS} steps: worst HIP error {worst[1]:.3e} ({worst[0]}; yardstick there {worst[2]:.3e}), worst yardstick "
          f"error {max(r[2] for r in report):.3e} (fractions of the parameter's largest float64 entry)")
    assert not errors, "\n".join(errors)
    # ... and the clip mattered: the unclipped epoch ended somewhere else
    assert any(not torch.equal(p, q) for p, q in zip(model.parameters(), probe_model.parameters()))


def _inf_from_call(n):
    """info_nce_loss times inf from its n-th call on (a host counter: no read-back)"""
    from taxoexpan_amd.loss import info_nce_loss
    calls = {"n": 0}

    def info_nce_then_inf(output, target=None):
        loss = info_nce_loss(output, target)
        calls["n"] += 1
        return loss * float("inf") if calls["n"] >= n else loss
    return info_nce_then_inf, calls


def test_train_epoch_freezes_at_the_first_nonfinite_step(toy):
    from taxoexpan_amd.trainer import train_epoch
    _dev_, batches, _state = toy
    model, opt = _fresh(toy)
    loss_fn, calls = _inf_from_call(4)
    got = train_epoch(model, _Replay(batches), opt, loss_fn=loss_fn, group_size=4, freeze_on_nonfinite=True)
    assert got["first_nonfinite"] == 3 and got["n_batches"] == STEPS and calls["n"] == STEPS         # the epoch still runs to its end
    assert np.isfinite(got["losses"][:3]).all() and np.isinf(got["losses"][3:]).all()
    three_model, three_opt = _fresh(toy)
    three = train_epoch(three_model, _Replay(batches[:3]), three_opt, group_size=4)
    assert three["losses"].tobytes() == got["losses"][:3].tobytes()
    _assert_same_run(model, opt, three_model, three_opt)                                             # parameters, moments and step counts
    assert all(s[0] == 3 for s in _opt_state(opt))
    # without the flag: today's behaviour, the NaN goes through every later step
    model, opt = _fresh(toy)
    loss_fn, _calls = _inf_from_call(4)
    got = train_epoch(model, _Replay(batches), opt, loss_fn=loss_fn, group_size=4)
    assert got["first_nonfinite"] == 3 and all(s[0] == STEPS for s in _opt_state(opt))
    assert any(not torch.isfinite(p).all() for p in model.parameters())


def test_fit_freezes_saves_and_resumes(toy, tmp_path):
    from taxoexpan_amd import optim
    from taxoexpan_amd.trainer import TrainingDiverged, fit
    dev, batches, state = toy
    model, opt = _fresh(toy)
    loss_fn, _calls = _inf_from_call(4)
    with pytest.raises(TrainingDiverged) as e:
        fit(model, _Replay(batches), None, opt, 2, monitor="off", save_dir=tmp_path / "run", loss_fn=loss_fn, group_size=4,
            freeze_on_nonfinite=True)
    assert (e.value.epoch, e.value.step) == (1, 3) and e.value.checkpoint == str(tmp_path / "run" / "last_finite.pth")
    assert all(torch.isfinite(p).all() for p in model.parameters())
    ck = torch.load(e.value.checkpoint, map_location="cpu", weights_only=False)
    assert ck["epoch"] == 0 and sorted(ck) == ["arch", "config", "epoch", "monitor_best", "optimizer", "state_dict"]
    fresh = _model(dev)
    fresh.load_state_dict(ck["state_dict"], strict=True)
    fresh_opt = optim.Adam(fresh.parameters(), lr=1e-3, amsgrad=True)
    fresh_opt.load_state_dict(ck["optimizer"])
    for (k, p), q in zip(model.named_parameters(), fresh.parameters()):
        assert torch.equal(p, q), k
    assert all(float(st["step"]) == 3 for st in fresh_opt.state.values())
    # one further epoch from the checkpoint, the wrapper gone: it starts at epoch 1 again and ends finite
    again = _model(dev)
    again_opt = optim.Adam(again.parameters(), lr=1e-3, amsgrad=True)
    logs = fit(again, _Replay(batches), None, again_opt, 1, monitor="off", group_size=4, resume=e.value.checkpoint, freeze_on_nonfinite=True)
    assert [l["epoch"] for l in logs] == [1] and logs[0]["first_nonfinite"] == -1
    assert all(torch.isfinite(p).all() for p in again.parameters())
    assert all(float(st["step"]) == 3 + STEPS for st in again_opt.state.values())
    assert any(not torch.equal(p, q) for p, q in zip(again.parameters(), fresh.parameters()))


def test_a_foreign_optimizer_is_refused_before_any_step(toy):
    from taxoexpan_amd.trainer import train_epoch
    _dev_, batches, state = toy
    model = _model(_dev_, state=state)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, amsgrad=True)
    with pytest.raises(ValueError, match="guard"):
        train_epoch(model, _Replay(batches), opt, group_size=4, max_grad_norm=1.0)
    for k, p in model.named_parameters():
        assert torch.equal(p, state[k]), k
    assert len(opt.state) == 0
