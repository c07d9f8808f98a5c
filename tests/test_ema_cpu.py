"""CPU: the averaged weights' host side -- optim.Adam's ema_decay / ema_warmup arguments, optim.ema_decay_at, optim.host_ema_update in
float32 against float64 under a derived bound, and the argument checks of txe_adam_step_ema / txe_tensor_swap that need no GPU.

The float32 bound.  One step of e = fma(1 - d, p - e, e) in fp32, with M the largest |p| or |e| met: the fp32 difference errs by at
most 2^-24 * 2M, the rounded 1 - d adds at most 2^-24 * 2M, the fma's rounding at most 2^-24 * M, and the errors of earlier steps
contract by d < 1: after T steps |e32 - e64| <= T * 5 * 2^-24 * M < T * 2^-21 * M.  Worst case over the cases below: 0.08 of it."""
import ctypes

import numpy as np
import pytest
import torch

T_STEPS = 8


@pytest.mark.parametrize("bad", [0.0, 1.0, -0.1, 1.5, float("nan"), True])
def test_constructor_refuses_a_decay_outside_the_open_unit_interval(bad):
    from taxoexpan_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match="ema_decay"):
        optim.Adam([p], ema_decay=bad)


def test_constructor_takes_a_decay_and_adds_keys_only_when_asked():
    from taxoexpan_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    opt = optim.Adam([p], ema_decay=0.999)
    assert opt.param_groups[0]["ema_decay"] == 0.999 and opt.param_groups[0]["ema_warmup"] is False
    assert optim.Adam([p], ema_decay=0.5, ema_warmup=True).param_groups[0]["ema_warmup"] is True
    plain = optim.Adam([p], lr=1e-3, amsgrad=True)
    assert sorted(plain.param_groups[0]) == sorted(["params", "lr", "betas", "eps", "weight_decay", "amsgrad"])
    sd = plain.state_dict()
    assert sorted(sd) == ["param_groups", "state"] and sd["state"] == {}
    assert sorted(sd["param_groups"][0]) == sorted(["params", "lr", "betas", "eps", "weight_decay", "amsgrad"])
    # a state written before the option existed loads, and reads as "no averaging"
    opt.__setstate__({"state": {}, "param_groups": [dict(params=[p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)],
                      "defaults": plain.defaults})
    assert opt.param_groups[0]["ema_decay"] is None and opt.param_groups[0]["ema_warmup"] is False


def test_loading_groups_saved_without_the_option_keeps_the_optimizers_own():
    from taxoexpan_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    plain, half = optim.Adam([p], amsgrad=True), optim.Adam([p], amsgrad=True, ema_decay=0.5)
    opt = optim.Adam([p], amsgrad=True, ema_decay=0.9, ema_warmup=True)
    opt.load_state_dict(plain.state_dict())
    assert opt.param_groups[0]["ema_decay"] == 0.9 and opt.param_groups[0]["ema_warmup"] is True
    opt.load_state_dict(half.state_dict())                         # saved with the key: it loads like every hyper-parameter
    assert opt.param_groups[0]["ema_decay"] == 0.5 and opt.param_groups[0]["ema_warmup"] is False
    plain.load_state_dict(half.state_dict())
    assert plain.param_groups[0]["ema_decay"] == 0.5


def test_ema_decay_at():
    from taxoexpan_amd.optim import ema_decay_at
    assert all(ema_decay_at(0.999, s) == 0.999 and ema_decay_at(0.999, s, False) == 0.999 for s in (1, 2, 10, 10 ** 6))
    want = [(1.0 + s) / (10.0 + s) for s in range(1, 6)]
    assert want[:3] == [2.0 / 11.0, 3.0 / 12.0, 4.0 / 13.0]
    assert [ema_decay_at(0.999, s, True) for s in range(1, 6)] == want
    prev = 0.0
    for s in range(1, 20000):
        d = ema_decay_at(0.999, s, True)
        assert prev <= d <= 0.999
        prev = d
    assert ema_decay_at(0.999, 8989, True) < 0.999 and ema_decay_at(0.999, 8990, True) == 0.999       # (1 + s) / (10 + s) = 0.999 at s = 8990
    assert ema_decay_at(0.5, 8, True) == 0.5 and ema_decay_at(0.5, 7, True) == 8.0 / 17.0
    with pytest.raises(ValueError):
        ema_decay_at(0.9, 0, True)


@pytest.mark.parametrize("decay", [0.5, 0.9, 0.999, 0.9999])
@pytest.mark.parametrize("n", [3, 1025, 4097])
def test_host_ema_update_float32_against_float64(decay, n):
    from taxoexpan_amd.optim import host_ema_update
    rng = np.random.RandomState(1000 + n)
    worst = 0.0
    for scale in (1e-2, 1e-1, 1.0, 1e1):
        p = (rng.randn(n) * scale).astype(np.float32)
        e32, e64 = p.copy(), p.astype(np.float64)
        M = float(np.abs(p).max())
        for _s in range(T_STEPS):
            p = (p + rng.randn(n).astype(np.float32) * np.float32(0.1 * scale)).astype(np.float32)        # gradient-like moves
            e32 = host_ema_update(e32, p, decay, np.float32)
            e64 = host_ema_update(e64, p, decay, np.float64)
            assert e32.dtype == np.float32 and e64.dtype == np.float64
            M = max(M, float(np.abs(p).max()), float(np.abs(e32).max()), float(np.abs(e64).max()))
        err, bound = float(np.abs(e32.astype(np.float64) - e64).max()), T_STEPS * 2.0 ** -21 * M
        worst = max(worst, err / bound)
        assert err <= bound, (decay, n, scale, err, bound)
    print(f"\n[gate] host_ema_update decay={decay} n={n}: worst |e32 - e64| = {worst:.3f} of T * 2^-21 * M")


def test_host_ema_update_definition_and_fixed_point():
    from taxoexpan_amd.optim import host_ema_update
    rng = np.random.RandomState(7)
    p = rng.randn(1025).astype(np.float32)
    e = p.copy()
    for d in (0.0, 0.5, 0.999):
        for _ in range(3):
            e = host_ema_update(e, p, d)
        assert e.tobytes() == p.tobytes()                          # a constant parameter and e == p: p - e = 0, fma(., 0, e) = e
    e0 = rng.randn(5)
    q = rng.randn(5)
    assert np.array_equal(host_ema_update(e0, q, 0.75, np.float64), 0.75 * e0 + 0.25 * q)
    # float32 by hand: (float)(1 - d), the fp32 difference, one rounding of the exact product-sum (all exact in fp64 for these values)
    a, b = np.float32(3.0), np.float32(1.0)
    omd = np.float32(1.0 - 0.9)
    want = np.float32(np.float64(omd) * np.float64(a - b) + np.float64(b))
    assert host_ema_update(np.array([b]), np.array([a]), 0.9)[0] == want
    keep_e, keep_p = e0.copy(), q.copy()
    host_ema_update(e0, q, 0.5)
    assert np.array_equal(e0, keep_e) and np.array_equal(q, keep_p)                # no argument is changed
    for bad in (1.0, -0.5, float("nan")):
        with pytest.raises(ValueError):
            host_ema_update(e0, q, bad)
    with pytest.raises(ValueError):
        host_ema_update(e0, q, 0.5, np.float16)


def test_c_abi_argument_checks_need_no_gpu():
    from taxoexpan_amd import _lib
    assert "txe_adam_step_ema" in _lib.SIGNATURES and "txe_tensor_swap" in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, "txe_adam_step_ema") and hasattr(lib, "txe_tensor_swap")
    one = (ctypes.c_void_p * 1)(None)                              # a non-NULL table (never read: the decay is checked first)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    for d in (1.0, -0.5, float("nan")):
        assert lib.txe_adam_step_ema(0, None, None, None, None, None, one, None, *hyper, d, None, None, 0.0, None) == -1
        assert lib.txe_adam_step_ema(1, one, one, one, one, None, one, None, *hyper, d, None, None, 0.0, None) == -1
    # ema == NULL: the decay is not looked at (nothing to do for 0 tensors -> 0)
    assert lib.txe_adam_step_ema(0, None, None, None, None, None, None, None, *hyper, 7.0, None, None, 0.0, None) == 0
    assert lib.txe_adam_step_ema(0, None, None, None, None, None, one, None, *hyper, 0.0, None, None, 0.0, None) == 0
    assert lib.txe_adam_step_ema(-1, None, None, None, None, None, one, None, *hyper, 0.5, None, None, 0.0, None) == -1
    assert lib.txe_tensor_swap(-1, None, None, None, None) == -1
    assert lib.txe_tensor_swap(0, None, None, None, None) == 0
    assert lib.txe_tensor_swap(1, None, None, None, None) == -1
    n = (ctypes.c_longlong * 1)(5)
    assert lib.txe_tensor_swap(1, one, one, n, None) == -1         # a NULL pointer of a non-empty pair
    n[0] = -1
    assert lib.txe_tensor_swap(1, one, one, n, None) == -1
    n[0] = 0
    assert lib.txe_tensor_swap(1, one, one, n, None) == 0          # an empty pair is skipped


def test_fit_refuses_averaging_without_an_averaging_optimizer():
    """before any step: nothing of the model, the loaders or the device is touched"""
    from taxoexpan_amd import optim
    from taxoexpan_amd.trainer import fit
    p = torch.nn.Parameter(torch.zeros(3))
    for opt in (torch.optim.Adam([p]), optim.Adam([p])):
        with pytest.raises(ValueError, match="ema_decay"):
            fit(None, None, None, opt, 1, averaged=True)
