#!/usr/bin/env python3
"""One training epoch (trainer.py:41-77) on a MAG-CS-shaped masked dataset (synthetic.make_named_taxonomy("mag_cs", seed=47) written as
raw files and read back; train mode, sampling_mode 1, 31 negatives, batches of 128 queries = 4,096 egonets: bench.py's step;
bench.make_model("pgat"), optim.Adam(amsgrad) at bench.LR), two legs alternating in one process on DeviceBatchLoader(sampler="device"):
  (a) trainer.train_epoch: one txe_step_log launch per step, nothing read back inside the loop, one read-back per epoch;
  (b) the reference-style loop: `label.sum()` read back to reshape the scores, a torch.zeros target, `loss.item()` twice per step.
Prints per leg and epoch the wall time and the time per step, then the step-log kernel's own average (and the Adam kernel's, for scale)
from the library's profile hooks over --profile-steps steps of leg (a).
--guard adds a third alternating leg
  (g) trainer.train_epoch(max_grad_norm=1e30, freeze_on_nonfinite=True): clip and freeze on, the clip never active (the same bits);
then profiles (a) and (g) twice each, alternating -- adam_kernel<true> beside adam_guarded_kernel<true>, and the library's launches per
step of both legs -- and last times the frozen tail of a diverged epoch: every loss times inf, so every optimizer launch of leg (g)
returns at once (parameters and moments are checked to be untouched).

--loss {info_nce,bce,square_exp,margin_rank} (default info_nce: everything above, unchanged) puts another loss into both legs: (a) gets
the device loss (loss.bce_loss / square_exp_loss / margin_rank_loss: still nothing read back), (b) the torch expression of the same loss
as tools/loss_timing.py writes it -- for margin_rank the literal route with its label read-back and host pair construction -- and keeps
its two `loss.item()`.  --guard goes with info_nce only.

--ema DECAY (info_nce only, beside --guard or without it) adds two more alternating legs on the same model and optimizer state:
  (e) train_epoch with the optimizer's ema_decay = DECAY: the average formed inside the Adam launch (txe_adam_step_ema);
  (l) the yardstick: ema_decay off, and torch._foreach_lerp_ over cloned parameters after every optimizer step -- what
      torch.optim.swa_utils.AveragedModel does with an EMA rule: one more pass over all parameters, one more launch per step;
then profiles the three legs twice each, alternating -- adam_kernel<true> of (a) and (l) beside adam_ema_kernel<true> of (e), the
library's launches per step -- and times the lerp launch of (l) on its own with device events.

    python tools/train_epoch_timing.py [--epochs 3] [--profile-steps 50] [--guard] [--ema DECAY] [--loss info_nce]"""
import argparse
import ctypes
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import loss_timing  # noqa: E402  (tools/loss_timing.py: the torch expressions of the labelled losses)
from taxoexpan_amd import loss as txe_loss  # noqa: E402
from taxoexpan_amd import _lib, synthetic as syn  # noqa: E402
from taxoexpan_amd.data_loaders import DeviceBatchLoader  # noqa: E402
from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset  # noqa: E402
from taxoexpan_amd.loss import info_nce_loss  # noqa: E402
from taxoexpan_amd.optim import Adam  # noqa: E402
from taxoexpan_amd.trainer import train_epoch  # noqa: E402

BS, K = bench.N_QUERIES, bench.NEG


def masked_mag_cs_train(directory):
    tax = syn.make_named_taxonomy("mag_cs", seed=47)
    syn.write_raw(directory, "magcs", syn.taxonomy_edges(tax), tax.features.numpy())
    random.seed(0)
    raw = MAGDataset("magcs", directory, raw=True)
    return MaskedGraphDataset(raw, mode="train", sampling_mode=1, negative_size=K, expand_factor=50, normalize_embed=True)


DEVICE_LOSS = {"bce": txe_loss.bce_loss, "square_exp": txe_loss.square_exp_loss, "margin_rank": txe_loss.margin_rank_loss}
TORCH_LOSS = {"bce": loss_timing.torch_bce, "square_exp": loss_timing.torch_square_exp, "margin_rank": loss_timing.torch_margin_literal}


def reference_style_epoch(model, loader, optimizer, dev, loss_name="info_nce"):
    """trainer.py:41-77 as written: two host round trips per step"""
    model.train()
    total_loss, n = 0, 0
    for bg, h, nf, label in loader:
        optimizer.zero_grad()
        prediction = model(bg, h, nf)
        if loss_name == "info_nce":
            n_batches = int(label.sum().detach())
            prediction = prediction.reshape(n_batches, -1)
            target = torch.zeros(n_batches, dtype=torch.long).to(dev)
            loss = info_nce_loss(prediction, target)
        else:
            loss = TORCH_LOSS[loss_name](prediction.reshape(-1, 1), label)      # trainer.py:57-58
        loss.backward()
        optimizer.step()
        loss.item()                                          # trainer.py:64 (the tensorboard scalar)
        total_loss += loss.item()
        n += 1
    return total_loss / n, n


class _First:
    """the first n batches of a loader"""

    def __init__(self, loader, n):
        self.loader, self.n, self.dataset = loader, min(n, len(loader)), loader.dataset

    def __len__(self):
        return self.n

    def __iter__(self):
        for i, b in enumerate(self.loader):
            if i == self.n:
                return
            yield b


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


GUARD = dict(max_grad_norm=1e30, freeze_on_nonfinite=True)


def info_nce_times_inf(output, target=None):
    return info_nce_loss(output, target) * float("inf")


def profiled_kernels(model, loader, opt, steps, **kw):
    """average duration by kernel name over `steps` steps of train_epoch (HIP events around every launch of the library)"""
    lib = _lib.load()
    lib.txe_profile_reset()
    lib.txe_profile_enable(1)
    train_epoch(model, _First(loader, steps), opt, **kw)
    torch.cuda.synchronize()
    lib.txe_profile_enable(0)
    buf = ctypes.create_string_buffer(64)
    ms, work, kind = ctypes.c_float(), ctypes.c_double(), ctypes.c_int()
    by = {}
    for i in range(lib.txe_profile_count()):
        lib.txe_profile_get(i, buf, 64, ctypes.byref(ms), ctypes.byref(work), ctypes.byref(kind))
        by.setdefault(buf.value.decode(), []).append((1e3 * ms.value, work.value))
    lib.txe_profile_reset()
    return {k: (float(np.mean([u for u, _ in v])), float(np.median([u for u, _ in v])), len(v), v[0][1]) for k, v in by.items()}


def guard_report(model, loader, opt, steps, g_s):
    """adam_kernel<true> of leg (a) beside adam_guarded_kernel<true> of leg (g), two alternating rounds; then the frozen tail"""
    print(f"(g) {min(g_s):.3f}-{max(g_s):.3f} ms/step (median {float(np.median(g_s)):.3f})")
    for r in range(2):
        for leg, kw, name in (("a", {}, "adam_kernel<true>"), ("g", GUARD, "adam_guarded_kernel<true>")):
            prof = profiled_kernels(model, loader, opt, steps, **kw)
            mean, med, n, work = prof[name]
            launches = sum(v[2] for v in prof.values()) / steps
            print(f"round {r} leg ({leg}): {name}: mean {mean:.2f} us, median {med:.2f} us over {n} launches = {work / (1e-6 * med) / 1e12:.2f} TB/s "
                  f"at the median; {launches:.1f} library launches per step", flush=True)
    before = [p.detach().clone() for p in model.parameters()]
    moments = [opt.state[p]["exp_avg_sq"].clone() for p in model.parameters()]
    counts = [float(opt.state[p]["step"]) for p in model.parameters()]
    n = min(60, len(loader))
    train_epoch(model, _First(loader, 10), opt, loss_fn=info_nce_times_inf, group_size=1 + K, **GUARD)       # (first calls of the non-finite route)
    t, r = timed(lambda: train_epoch(model, _First(loader, n), opt, loss_fn=info_nce_times_inf, group_size=1 + K, **GUARD))
    prof = profiled_kernels(model, loader, opt, min(steps, n), loss_fn=info_nce_times_inf, group_size=1 + K, **GUARD)
    assert r["first_nonfinite"] == 0 and all(torch.equal(p, q) for p, q in zip(model.parameters(), before))
    assert all(torch.equal(opt.state[p]["exp_avg_sq"], q) for p, q in zip(model.parameters(), moments))
    assert [float(opt.state[p]["step"]) for p in model.parameters()] == counts
    mean, med, k, _work = prof["adam_guarded_kernel<true>"]
    print(f"frozen tail: {n} steps of a diverged epoch (every loss inf, freeze on): {1e3 * t / n:.3f} ms/step; the frozen "
          f"adam_guarded_kernel<true>: mean {mean:.2f} us, median {med:.2f} us over {k} launches (no traffic); parameters, moments and step "
          f"counts untouched", flush=True)


class LerpAfterStep:
    """leg (l): the optimizer with its averaging off, and after every step avg = lerp(avg, p, 1 - decay) over clones of the parameters
    (torch._foreach_lerp_, the update of swa_utils.get_ema_multi_avg_fn); train_epoch sees param_groups, zero_grad and step"""

    def __init__(self, opt, decay):
        self.opt, self.weight = opt, 1.0 - decay
        self.params = [p for g in opt.param_groups for p in g["params"]]
        self.avg = [p.detach().clone() for p in self.params]

    @property
    def param_groups(self):
        return self.opt.param_groups

    def zero_grad(self):
        self.opt.zero_grad()

    @torch.no_grad()
    def lerp(self):
        torch._foreach_lerp_(self.avg, [p.detach() for p in self.params], self.weight)

    def step(self):
        self.opt.step()
        self.lerp()


def set_ema(opt, decay):
    """averaging on (a decay) or off (None) for every group: optim.Adam reads the key at every step, and keeps state["ema"] while off"""
    for g in opt.param_groups:
        g["ema_decay"] = decay


def ema_report(model, loader, opt, lerp_opt, decay, steps, e_s, l_s):
    print(f"(e) {min(e_s):.3f}-{max(e_s):.3f} ms/step (median {float(np.median(e_s)):.3f}), (l) {min(l_s):.3f}-{max(l_s):.3f} ms/step "
          f"(median {float(np.median(l_s)):.3f})")
    for r in range(2):
        for leg, name in (("a", "adam_kernel<true>"), ("e", "adam_ema_kernel<true>"), ("l", "adam_kernel<true>")):
            set_ema(opt, decay if leg == "e" else None)
            prof = profiled_kernels(model, loader, lerp_opt if leg == "l" else opt, steps)
            mean, med, n, work = prof[name]
            launches = sum(v[2] for v in prof.values()) / steps
            print(f"round {r} leg ({leg}): {name}: mean {mean:.2f} us, median {med:.2f} us over {n} launches, {work / 1e6:.2f} MB = "
                  f"{work / (1e-6 * med) / 1e12:.2f} TB/s at the median; {launches:.1f} library launches per step"
                  + (" (+ 1 torch launch: the lerp)" if leg == "l" else ""), flush=True)
    set_ema(opt, None)
    for _ in range(20):
        lerp_opt.lerp()
    us = []
    for _ in range(200):                                     # the lerp launch alone, back to back with nothing: device events around each
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        lerp_opt.lerp()
        t1.record()
        t1.synchronize()
        us.append(1e3 * t0.elapsed_time(t1))
    n = sum(p.numel() for p in lerp_opt.params)
    print(f"torch._foreach_lerp_ over {len(lerp_opt.params)} tensors, {n} elements ({12.0 * n / 1e6:.2f} MB read + written), events around "
          f"each call: mean {float(np.mean(us)):.2f} us, median {float(np.median(us)):.2f} us over {len(us)} calls", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=50)
    ap.add_argument("--guard", action="store_true", help="add leg (g): clip (never active) and freeze on; see the module docstring")
    ap.add_argument("--ema", type=float, default=None, metavar="DECAY",
                    help="add legs (e) and (l): the average inside the Adam launch, and a foreach lerp after every step; see the module docstring")
    ap.add_argument("--loss", choices=["info_nce", "bce", "square_exp", "margin_rank"], default="info_nce")
    args = ap.parse_args()
    if args.guard and args.loss != "info_nce":
        ap.error("--guard goes with --loss info_nce only")
    if args.ema is not None and (args.loss != "info_nce" or not 0.0 < args.ema < 1.0):
        ap.error("--ema takes a decay in (0, 1) and goes with --loss info_nce only")
    kw = {} if args.loss == "info_nce" else {"loss_fn": DEVICE_LOSS[args.loss]}       # (info_nce: the calls are what they were)
    if kw:
        print(f"loss: {args.loss} -- (a) the device loss, (b) its torch expression", flush=True)
    assert torch.cuda.is_available(), "train_epoch_timing.py times the MI355X: no GPU found"
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        ds = masked_mag_cs_train(d)
        print(f"dataset: {ds.node_features.shape[0]} nodes, {len(ds)} training queries (built in {time.perf_counter() - t0:.1f} s)", flush=True)
    torch.manual_seed(47)
    model = bench.make_model("pgat", dev)
    opt = Adam(model.parameters(), lr=bench.LR, weight_decay=0, amsgrad=True)
    loader = DeviceBatchLoader(ds, BS, dev, shuffle=True, seed=0, sampler="device")
    n_grad = sum(p.numel() for p in model.parameters())
    print(f"{len(loader)} steps per epoch, {BS} queries x {1 + K} egonets per step, {n_grad} gradient elements per step", flush=True)
    train_epoch(model, _First(loader, 30), opt, **kw)        # warm-up of both legs (first-call costs, allocator)
    reference_style_epoch(model, _First(loader, 30), opt, dev, args.loss)
    if args.guard:
        train_epoch(model, _First(loader, 30), opt, **GUARD)
    lerp_opt = None
    if args.ema is not None:
        set_ema(opt, args.ema)
        train_epoch(model, _First(loader, 30), opt)
        set_ema(opt, None)
        lerp_opt = LerpAfterStep(opt, args.ema)
        train_epoch(model, _First(loader, 30), lerp_opt)
    a_s, b_s, g_s, e_s, l_s = [], [], [], [], []
    for e in range(args.epochs):
        ta, ra = timed(lambda: train_epoch(model, loader, opt, **kw))
        if args.ema is not None:
            set_ema(opt, args.ema)
            te, re_ = timed(lambda: train_epoch(model, loader, opt))
            set_ema(opt, None)
            tl, rl = timed(lambda: train_epoch(model, loader, lerp_opt))
            assert re_["first_nonfinite"] == -1 and rl["first_nonfinite"] == -1, "the model diverged: the timing is void"
            e_s.append(1e3 * te / re_["n_batches"])
            l_s.append(1e3 * tl / rl["n_batches"])
        if args.guard:
            tg, rg = timed(lambda: train_epoch(model, loader, opt, **GUARD))
            assert rg["first_nonfinite"] == -1, "the model diverged: the timing is void"
            g_s.append(1e3 * tg / rg["n_batches"])
        tb, (lb, nb) = timed(lambda: reference_style_epoch(model, loader, opt, dev, args.loss))
        assert ra["first_nonfinite"] == -1 and np.isfinite(lb), "the model diverged: the timing is void"
        a_s.append(1e3 * ta / ra["n_batches"])
        b_s.append(1e3 * tb / nb)
        print(f"epoch {e}: (a) train_epoch {1e3 * ta:.1f} ms = {a_s[-1]:.3f} ms/step (loss {ra['loss']:.3f}, |g| {ra['grad_norms'][-1]:.3f}) | "
              + (f"(g) guarded {1e3 * tg:.1f} ms = {g_s[-1]:.3f} ms/step | " if args.guard else "")
              + (f"(e) EMA in the launch {1e3 * te:.1f} ms = {e_s[-1]:.3f} ms/step | (l) foreach lerp after the step {1e3 * tl:.1f} ms = "
                 f"{l_s[-1]:.3f} ms/step | " if args.ema is not None else "")
              + f"(b) reference-style loop {1e3 * tb:.1f} ms = {b_s[-1]:.3f} ms/step (loss {lb:.3f})", flush=True)
    prof = profiled_kernels(model, loader, opt, args.profile_steps, **kw)
    loss_kernels = {"bce": ("bce_loss_kernel",), "square_exp": ("square_exp_loss_kernel",),
                    "margin_rank": ("group_flags_kernel", "group_scan", "group_index_kernel<0>", "margin_pairs_kernel", "margin_finish_kernel")}
    for name in ("step_log_kernel", "adam_kernel<true>") + loss_kernels.get(args.loss, ()):
        if name in prof:
            mean, med, n, work = prof[name]
            print(f"{name}: mean {mean:.2f} us, median {med:.2f} us over {n} launches; {work / 1e6:.2f} MB compulsory per launch "
                  f"= {work / (1e-6 * med) / 1e12:.2f} TB/s at the median")
    if args.guard:
        guard_report(model, loader, opt, args.profile_steps, g_s)
    if args.ema is not None:
        ema_report(model, loader, opt, lerp_opt, args.ema, args.profile_steps, e_s, l_s)
    print(f"summary: (a) {min(a_s):.3f}-{max(a_s):.3f} ms/step (median {float(np.median(a_s)):.3f}), (b) {min(b_s):.3f}-{max(b_s):.3f} ms/step "
          f"(median {float(np.median(b_s)):.3f}); (a) <= (b) in every epoch: {all(a <= b for a, b in zip(a_s, b_s))}")


if __name__ == "__main__":
    main()
