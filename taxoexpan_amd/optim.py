"""`torch.optim.Adam` as the reference configures it (train.py:36 `config.initialize('optimizer', torch.optim, ...)`,
config.mag.json:66-73: Adam, lr 1e-3, weight_decay 0, amsgrad true), stepped by ONE HIP launch over all parameter tensors
(txe_adam_step).  Same constructor arguments, same `state_dict()` layout (step / exp_avg / exp_avg_sq / max_exp_avg_sq per
parameter), so optimizer checkpoints written by base_trainer.py:104-121 load into either class.  There is no CPU path.

The guarded step (txe_adam_step_guarded) is the same launch behind two device scalars that an earlier launch on the same stream wrote --
trainer.StepLog's squared gradient norm of the step and its first-non-finite word: clipping by the global norm without a norm pass or
a scaling pass, and a step that leaves parameters and moments alone once the run has diverged, both without a read-back.
    StepGuard          what step(guard=...) takes: the two device addresses and the tensors that keep them alive
    host_guarded_adam  the numpy restatement of the kernel, in float32 (operation for operation) or float64 (the reference of the gates)

Averaged weights (an addition: the reference has no weight averaging).  Adam(ema_decay=d) keeps state["ema"], an exponential moving
average of every parameter, formed by the thread that has just updated the element (txe_adam_step_ema: one more 4-byte load and store
per element in the same launch, no second pass, and frozen with the step when the guard freezes it).
    ema_decay_at       the effective decay of one step (constant, or the warm-up schedule min(d, (1 + step) / (10 + step)))
    host_ema_update    the numpy restatement of the average, in float32 (operation for operation) or float64
    Adam.averaged_parameters()   a context in which the parameters ARE the averages (one txe_tensor_swap in, one out): validate,
                       evaluate, infer or take a state_dict() inside it"""
import contextlib
import ctypes as C
import math

import numpy as np
import torch

from . import _lib


class StepGuard:
    """gnorm2: the device address of one fp64 -- the squared global L2 norm of the gradients of the step about to be taken -- or None;
    first_bad: the device address of one int64 that is >= 0 once a step was not finite, or None; keep: whatever owns that memory.
    Both values must have been written by work enqueued earlier on the stream that step() is called on."""
    __slots__ = ("gnorm2", "first_bad", "max_grad_norm", "keep")

    def __init__(self, gnorm2=None, first_bad=None, max_grad_norm=None, keep=()):
        """max_grad_norm: the clip threshold for this step; None takes each parameter group's own `max_grad_norm`"""
        self.gnorm2, self.first_bad, self.max_grad_norm, self.keep = gnorm2, first_bad, _checked_max_norm(max_grad_norm), tuple(keep)


def _checked_max_norm(max_grad_norm):
    if max_grad_norm is None:
        return None
    if isinstance(max_grad_norm, bool) or not (math.isfinite(max_grad_norm) and max_grad_norm > 0.0):
        raise ValueError(f"max_grad_norm must be None or finite and > 0, got {max_grad_norm!r}")
    return float(max_grad_norm)


def _checked_ema_decay(ema_decay):
    if ema_decay is None:
        return None
    if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float, np.floating)) or not 0.0 < ema_decay < 1.0:     # (NaN compares false)
        raise ValueError(f"ema_decay must be None or a float with 0 < ema_decay < 1, got {ema_decay!r}")
    return float(ema_decay)


def ema_decay_at(decay, step, warmup=False):
    """the decay that update number `step` (1-based: the number the kernel gets as `step`) averages with: `decay`, or with warm-up
    min(decay, (1 + step) / (10 + step)) -- 2/11, 3/12, ... until the cap, so that the first steps do not pin the average to the
    initial weights"""
    decay = float(decay)
    if not warmup:
        return decay
    step = int(step)
    if step < 1:
        raise ValueError("step counts from 1")
    return min(decay, (1.0 + step) / (10.0 + step))


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, max_grad_norm=None, ema_decay=None,
                 ema_warmup=False):
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("invalid Adam hyper-parameter")        # the checks of torch.optim.Adam.__init__
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        if _checked_max_norm(max_grad_norm) is not None:            # an added key of the param groups, as torch's optimizers add theirs;
            defaults["max_grad_norm"] = float(max_grad_norm)        # absent (read as None) when not asked for: groups and state_dict as ever
        if _checked_ema_decay(ema_decay) is not None:               # the same rule: two more keys only when averaging was asked for
            defaults["ema_decay"], defaults["ema_warmup"] = float(ema_decay), bool(ema_warmup)
        super().__init__(params, defaults)
        self._tables = {}
        self._averaged = False

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("amsgrad", False)
            group.setdefault("max_grad_norm", None)
            group.setdefault("ema_decay", None)
            group.setdefault("ema_warmup", False)
        self._tables = {}
        self._averaged = False

    def load_state_dict(self, state_dict):
        """torch's, with one addition: param groups saved WITHOUT an ema_decay key (a run that did not average, or the reference's
        torch.optim.Adam) leave this optimizer's own ema_decay / ema_warmup in place -- the average then starts from the current
        parameters at the next step.  Groups saved with the key load it like every other hyper-parameter."""
        mine = [(g.get("ema_decay"), g.get("ema_warmup", False)) for g in self.param_groups]
        super().load_state_dict(state_dict)
        for group, saved, (decay, warmup) in zip(self.param_groups, state_dict["param_groups"], mine):
            if "ema_decay" not in saved and decay is not None:
                group["ema_decay"], group["ema_warmup"] = decay, warmup

    def discount_frozen_steps(self, n):
        """take back `n` steps that the host counted and the device skipped (a guarded step with *first_bad >= 0 changes nothing, but
        step() cannot know that without a read-back): every parameter's state["step"] -= n, never below 0"""
        n = int(n)
        if n < 0:
            raise ValueError(f"discount_frozen_steps needs n >= 0, got {n}")
        for st in self.state.values():
            if "step" in st:
                st["step"] = torch.clamp(st["step"] - n, min=0) if torch.is_tensor(st["step"]) else max(st["step"] - n, 0)

    def _init_state(self, p, amsgrad, ema=False):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if amsgrad:
                st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if ema and "ema" not in st:                                # with the other state, or at the first step after a checkpoint without
            st["ema"] = p.detach().clone(memory_format=torch.preserve_format)       # an average: the parameter before this update
        return st

    def _averaged_pairs(self):
        """(parameter, its average) for every parameter that has one, the average normalised as step() normalises the moments"""
        pairs = []
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p)
                if st is None or "ema" not in st:
                    continue
                e = st["ema"]
                if not (e.is_contiguous() and e.dtype == torch.float32 and e.device == p.device):
                    e = st["ema"] = e.to(device=p.device, dtype=torch.float32).contiguous()
                if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous():
                    raise RuntimeError("taxoexpan_amd.optim.Adam: dense contiguous fp32 parameters on the GPU only")
                pairs.append((p, e))
        return pairs

    @torch.no_grad()
    def swap_averaged(self):
        """exchange every parameter that has a state["ema"] with it, bit for bit, in ONE txe_tensor_swap: after an odd number of calls
        the model computes with the averages (and state["ema"] holds the raw weights), after an even number all is as it was.  The
        swapped parameters' `_version` is raised, so that whatever memoises on a parameter (ops' int32 / prefetch / fold tokens, the
        prepared bilinear side) sees a written tensor.  step() refuses to run while the averages are in."""
        pairs = self._averaged_pairs()
        if pairs:
            with _lib.on_device(pairs[0][0].device):
                _lib.call("txe_tensor_swap", len(pairs), self._ptr_array([p for p, _ in pairs]), self._ptr_array([e for _, e in pairs]),
                          (C.c_longlong * len(pairs))(*[p.numel() for p, _ in pairs]), _lib.stream_ptr())
            for p, e in pairs:
                torch.autograd.graph.increment_version(p)
                torch.autograd.graph.increment_version(e)
        self._averaged = not self._averaged

    @contextlib.contextmanager
    def averaged_parameters(self):
        """`with optimizer.averaged_parameters(): validate(model, ...)` -- the parameters are the averages inside (swap_averaged on
        entry) and the raw weights again afterwards (swapped back on exit, also when the body raises).  Entering it twice, or calling
        step() inside it, raises RuntimeError: that step would average the averages."""
        if self._averaged:
            raise RuntimeError("taxoexpan_amd.optim.Adam: the averaged parameters are already swapped in (averaged_parameters() does not nest)")
        self.swap_averaged()
        try:
            yield self
        finally:
            self.swap_averaged()

    @staticmethod
    def _ptr_array(tensors):
        return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])

    @torch.no_grad()
    def step(self, closure=None, guard=None):
        """guard (a StepGuard, e.g. trainer.StepLog.guard()): None and no group with a max_grad_norm is txe_adam_step as ever.  With a
        guard the launch reads guard.first_bad (set: a diverged run's steps change nothing) and, for a group whose max_grad_norm --
        or the guard's, which goes first -- is set, guard.gnorm2 (every gradient is scaled by min(1, max_grad_norm / (norm + 1e-6)) on
        its way into the update; `.grad` itself is not written).  state["step"] is counted either way: see discount_frozen_steps.
        A group with an ema_decay goes through txe_adam_step_ema, guard or not: the same update, and state["ema"] averaged in the same
        launch with ema_decay_at(decay, this step's count, warm-up) -- a frozen step leaves it alone, and the discounted counts let the
        warm-up schedule resume where the device stopped."""
        if self._averaged:
            raise RuntimeError("taxoexpan_amd.optim.Adam: step() while the averaged parameters are swapped in would average the averages "
                               "(leave averaged_parameters() first)")
        for group in self.param_groups:
            if (group.get("max_grad_norm") is not None or (guard is not None and guard.max_grad_norm is not None)) and \
                    (guard is None or guard.gnorm2 is None):
                raise RuntimeError("taxoexpan_amd.optim.Adam: max_grad_norm is set, but step() got no guard with the gradients' norm to "
                                   "clip by (trainer.StepLog.guard() after record())")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            ams = bool(group["amsgrad"])
            decay = group.get("ema_decay")
            ema = decay is not None
            by_step = {}                                   # parameters that skipped updates (grad None) keep their own count
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse or p.dtype != torch.float32 or not p.is_cuda:
                    raise RuntimeError("taxoexpan_amd.optim.Adam: dense fp32 parameters on the GPU only")
                st = self._init_state(p, ams, ema)
                by_step.setdefault(int(st["step"]), []).append(p)
            for step, ps in by_step.items():
                key = (gi, ema, tuple(id(p) for p in ps))
                tab = self._tables.get(key)
                if tab is None or any(t.data_ptr() != a for t, a in zip(tab["tensors"], tab["addr"])):
                    sts = [self.state[p] for p in ps]
                    for p, st in zip(ps, sts):
                        for k in ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if ams else ()) + (("ema",) if ema else ()):
                            if not (st[k].is_contiguous() and st[k].dtype == torch.float32 and st[k].device == p.device):
                                st[k] = st[k].to(device=p.device, dtype=torch.float32).contiguous()
                    if any(not p.is_contiguous() for p in ps):
                        raise RuntimeError("taxoexpan_amd.optim.Adam: parameters must be contiguous")
                    tensors = list(ps) + [st["exp_avg"] for st in sts] + [st["exp_avg_sq"] for st in sts] + \
                        ([st["max_exp_avg_sq"] for st in sts] if ams else []) + ([st["ema"] for st in sts] if ema else [])
                    tab = dict(tensors=tensors, addr=[t.data_ptr() for t in tensors], p=self._ptr_array(ps),
                               m=self._ptr_array([st["exp_avg"] for st in sts]), v=self._ptr_array([st["exp_avg_sq"] for st in sts]),
                               x=self._ptr_array([st["max_exp_avg_sq"] for st in sts]) if ams else None,
                               e=self._ptr_array([st["ema"] for st in sts]) if ema else None,
                               n=(C.c_longlong * len(ps))(*[p.numel() for p in ps]))
                    self._tables[key] = tab
                grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in ps]
                hyper = (float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]),
                         float(group["weight_decay"]), step + 1)
                clip = None if guard is None else (guard.max_grad_norm if guard.max_grad_norm is not None else group.get("max_grad_norm"))
                if ema:
                    _lib.call("txe_adam_step_ema", len(ps), tab["p"], self._ptr_array(grads), tab["m"], tab["v"], tab["x"], tab["e"], tab["n"],
                              *hyper, ema_decay_at(decay, step + 1, group.get("ema_warmup", False)),
                              guard.gnorm2 if clip is not None else None, None if guard is None else guard.first_bad,
                              0.0 if clip is None else float(clip), _lib.stream_ptr())
                elif guard is None:
                    _lib.call("txe_adam_step", len(ps), tab["p"], self._ptr_array(grads), tab["m"], tab["v"], tab["x"], tab["n"], *hyper,
                              _lib.stream_ptr())
                else:
                    _lib.call("txe_adam_step_guarded", len(ps), tab["p"], self._ptr_array(grads), tab["m"], tab["v"], tab["x"], tab["n"],
                              *hyper, guard.gnorm2 if clip is not None else None, guard.first_bad, 0.0 if clip is None else float(clip),
                              _lib.stream_ptr())
                for p in ps:
                    self.state[p]["step"] += 1
        return loss


def _fma(a, b, c, dtype):
    """a * b + c rounded once to `dtype` (fmaf); float64: the plain expression"""
    if dtype == np.float64:
        return a * b + c
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    prod = a * b                                               # exact: 24 + 24 bits
    s = prod + c
    # one rounding to fp64 and a second one to fp32 can differ from the single rounding of fmaf when the fp64 sum is inexact and lands on
    # an fp32 tie: round the fp64 sum to ODD instead (Knuth's two-sum gives the error term), after which the rounding to fp32 is fmaf's
    bb = s - prod
    err = (prod - (s - bb)) + (c - bb)
    with np.errstate(invalid="ignore"):
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def host_ema_update(ema, p_new, decay, dtype=np.float32):
    """One tensor's average after one step, on the host: the new `ema` as a `dtype` array; no argument is changed.  `decay` is the
    effective decay of the step (ema_decay_at), p_new the parameter AFTER the step's update.
    dtype float32 is the kernel operation for operation: one_minus_d = (float)(1 - decay), the fp32 difference p_new - e, then
    e = fma(one_minus_d, p_new - e, e).  dtype float64 is the plain recurrence e = decay e + (1 - decay) p_new, nothing rounded to fp32."""
    dtype = np.dtype(dtype).type
    if dtype not in (np.float32, np.float64):
        raise ValueError("host_ema_update runs in float32 or float64")
    decay = float(decay)
    if not 0.0 <= decay < 1.0:
        raise ValueError(f"the effective decay of a step is in [0, 1), got {decay!r}")
    e, p = np.array(ema, dtype=dtype), np.array(p_new, dtype=dtype)
    with np.errstate(all="ignore"):
        if dtype == np.float64:
            return decay * e + (1.0 - decay) * p
        return _fma(np.float32(1.0 - decay), p - e, e, dtype)


def host_guarded_adam(p, g, m, v, vmax, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1, gnorm2=None, first_bad=None,
                      max_grad_norm=None, dtype=np.float32):
    """One tensor's txe_adam_step_guarded on the host: returns the new (p, m, v, vmax) as `dtype` arrays and changes no argument.
    vmax None selects plain Adam (None is returned in its place); `step` >= 1 is the count of this update; gnorm2 (the squared global
    norm, a float), first_bad (an int) and max_grad_norm are the values the kernel reads, None = a NULL pointer.
      first_bad >= 0: the inputs come back unchanged.
      coef64 = max_grad_norm / (sqrt(gnorm2) + 1e-6) in fp64;  coef = coef64 if coef64 < 1 else 1  (NaN norm: 1, +Inf norm: 0)
      g' = fma(weight_decay, p, coef g);  m = fma(1-beta1, g' - m, m);  v = fma(g', (1-beta2) g', beta2 v);  vmax = max(vmax, v)
      p -= (lr / (1-beta1^step)) m / (sqrt(vmax or v) / sqrt(1-beta2^step) + eps)
    dtype float32 is the kernel operation for operation: the scalars rounded to fp32 as the C entry point rounds them, coef rounded to
    fp32, every product and sum in fp32 with the fused multiply-adds where the kernel has them (the division and the square root are
    correctly rounded on the device, as numpy's are).  dtype float64 is the same definition with nothing rounded to fp32 on the way: the
    reference that the gates measure the kernel and the fp32 literal route (clip_grad_norm_, then torch.optim.Adam) against."""
    dtype = np.dtype(dtype).type
    if dtype not in (np.float32, np.float64):
        raise ValueError("host_guarded_adam runs in float32 or float64")
    if step < 1:
        raise ValueError("step counts from 1")
    ams = vmax is not None
    p, g, m, v = (np.array(a, dtype=dtype) for a in (p, g, m, v))
    x = np.array(vmax, dtype=dtype) if ams else None
    if first_bad is not None and int(first_bad) >= 0:
        return p, m, v, x
    if gnorm2 is not None and _checked_max_norm(max_grad_norm) is None:
        raise ValueError("a gnorm2 needs the max_grad_norm to clip to")
    f = dtype
    bc1, bc2 = 1.0 - math.pow(beta1, step), 1.0 - math.pow(beta2, step)
    omb1, b2, omb2, eps_, wd, step_size, bc2_sqrt = f(1.0 - beta1), f(beta2), f(1.0 - beta2), f(eps), f(weight_decay), f(lr / bc1), f(math.sqrt(bc2))
    with np.errstate(all="ignore"):
        if gnorm2 is not None:
            coef64 = np.float64(max_grad_norm) / (np.sqrt(np.float64(gnorm2)) + np.float64(1e-6))
            g = g * (f(coef64) if coef64 < 1.0 else f(1.0))
        g = _fma(wd, p, g, dtype)
        m = _fma(omb1, g - m, m, dtype)
        v = _fma(g, omb2 * g, b2 * v, dtype)
        if ams:
            x = np.fmax(x, v)                                  # fmaxf
        d = np.sqrt(x if ams else v) / bc2_sqrt + eps_
        p = p - step_size * m / d
    return p.astype(dtype), m.astype(dtype), v.astype(dtype), (x.astype(dtype) if ams else None)
