"""CPU: feature_table.host_sparse_adam_rows (the written definition of txe_rowgrad_group + txe_sparse_adam_rows) against torch.optim.Adam,
np.add.at and optim.host_guarded_adam; what it must leave alone; the argument checks of the new C entry points (they return before any
launch); the binding table against the header; the option checks of FeatureTable's users that need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from feature_table_cases import CASES, D_VALUES, N_ROWS, draw_case, draw_state

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYPER = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)


@pytest.mark.parametrize("amsgrad", [False, True])
def test_float64_restatement_is_torch_adam_when_every_row_occurs_once(amsgrad):
    """5 steps, every row exactly once per step (split over the two sides, shuffled): dense torch.optim.Adam in float64 on the same
    gradients; the tolerance is the one test_guarded_step_cpu.py holds host_guarded_adam's float64 to (rtol 1e-12, atol 1e-300)"""
    from taxoexpan_amd.feature_table import host_sparse_adam_rows
    rng = np.random.RandomState(5)
    n, d = 23, 7
    w0 = rng.randn(n, d).astype(np.float32)
    p = torch.nn.Parameter(torch.from_numpy(w0.astype(np.float64)))
    opt = torch.optim.Adam([p], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, amsgrad=amsgrad)
    w, m, v = w0.astype(np.float64), np.zeros((n, d)), np.zeros((n, d))
    x = np.zeros((n, d)) if amsgrad else None
    for step in range(1, 6):
        perm = rng.permutation(n)
        ids_a, ids_b = perm[:14], perm[14:]
        d_a, d_b = rng.randn(14, d).astype(np.float32), rng.randn(n - 14, d).astype(np.float32)
        dense = np.zeros((n, d))
        dense[ids_a], dense[ids_b] = d_a, d_b
        p.grad = torch.from_numpy(dense)
        opt.step()
        w, m, v, x = host_sparse_adam_rows(w, m, v, x, ids_a, d_a, ids_b, d_b, step=step, dtype=np.float64, **HYPER)
        st = opt.state[p]
        np.testing.assert_allclose(w, p.detach().numpy(), rtol=1e-12, atol=1e-300, err_msg=f"weight, step {step}")
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-300)
        if amsgrad:
            np.testing.assert_allclose(x, st["max_exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("case", [c for c in CASES if c not in ("both_empty",)])
def test_float64_row_sums_are_add_at(case):
    """with duplicates: the float64 sums in the kernel's order against np.add.at (plain left-to-right) -- equal to fp64 reordering
    error, and exactly equal while no segment is split (L <= 64: the same order)"""
    from taxoexpan_amd.feature_table import host_row_sums, SPLIT
    c = draw_case(case, 7)
    rows, sums = host_row_sums(c["ids_a"], c["d_a"], c["ids_b"], c["d_b"], N_ROWS, np.float64)
    ids = np.concatenate([c["ids_a"], c["ids_b"]]).astype(np.int64)
    g = np.concatenate([c["d_a"], c["d_b"]], 0).astype(np.float64)
    ok = (ids >= 0) & (ids < N_ROWS)
    want = np.zeros((N_ROWS, 7))
    np.add.at(want, ids[ok], g[ok])
    assert rows.tolist() == sorted(set(ids[ok].tolist()))
    longest = max(np.bincount(ids[ok], minlength=1)) if ok.any() else 0
    if longest <= SPLIT:
        assert np.array_equal(sums, want[rows])
    else:
        np.testing.assert_allclose(sums, want[rows], rtol=0, atol=longest * 2.0 ** -52 * np.abs(g).sum(0).max())
    touched = np.zeros(N_ROWS, bool)
    touched[rows] = True
    assert not want[~touched].any()


@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_float32_restatement_is_host_guarded_adam_on_its_row_sums(case, amsgrad):
    from taxoexpan_amd.feature_table import host_row_sums, host_sparse_adam_rows
    from taxoexpan_amd.optim import host_guarded_adam
    c = draw_case(case, 7)
    w, m, v, x = draw_state(7, amsgrad)
    got = host_sparse_adam_rows(w, m, v, x, c["ids_a"], c["d_a"], c["ids_b"], c["d_b"], step=3, trainable=c.get("trainable"), **HYPER)
    rows, sums = host_row_sums(c["ids_a"], c["d_a"], c["ids_b"], c["d_b"], N_ROWS, np.float32)
    assert sums.dtype == np.float32
    if c.get("trainable") is not None:
        keep = c["trainable"][rows] != 0
        rows, sums = rows[keep], sums[keep]
    want = [a.copy() for a in (w, m, v)] + [None if x is None else x.copy()]
    if len(rows):
        upd = host_guarded_adam(w[rows], sums, m[rows], v[rows], None if x is None else x[rows], weight_decay=0.0, step=3,
                                dtype=np.float32, **HYPER)
        for dst, src in zip(want, upd):
            if dst is not None:
                dst[rows] = src
    for name, a, b in zip("weight exp_avg exp_avg_sq max_exp_avg_sq".split(), got, want):
        assert (a is None and b is None) or (a.dtype == np.float32 and a.tobytes() == b.tobytes()), name
    # rows that do not occur (or are not trainable) come back bit-unchanged
    rest = np.ones(N_ROWS, bool)
    rest[rows] = False
    for a, b in zip(got, (w, m, v, x)):
        assert a is None or a[rest].tobytes() == b[rest].tobytes()
    if len(rows):
        assert not np.array_equal(got[0][rows], w[rows])


def test_what_the_restatement_leaves_alone():
    """first_bad >= 0: every array bit-unchanged; out-of-range ids change nothing; no argument is written"""
    from taxoexpan_amd.feature_table import host_sparse_adam_rows
    c = draw_case("all_distinct", 7)
    w, m, v, x = draw_state(7, True)
    before = [a.copy() for a in (w, m, v, x, c["d_a"], c["d_b"])]
    for first_bad in (0, 5):
        got = host_sparse_adam_rows(w, m, v, x, c["ids_a"], c["d_a"], c["ids_b"], c["d_b"], step=2, first_bad=first_bad, **HYPER)
        assert all(a.tobytes() == b.tobytes() and a is not b for a, b in zip(got, (w, m, v, x)))
    moved = host_sparse_adam_rows(w, m, v, x, c["ids_a"], c["d_a"], c["ids_b"], c["d_b"], step=2, first_bad=-1, **HYPER)
    assert moved[0].tobytes() != w.tobytes()
    rng = np.random.RandomState(1)
    bad_a = np.where(rng.rand(len(c["ids_a"])) < 0.5, -1 - rng.randint(0, 5, len(c["ids_a"])), N_ROWS + rng.randint(0, 9, len(c["ids_a"])))
    bad_b = np.full(len(c["ids_b"]), 2 ** 31 - 1)
    got = host_sparse_adam_rows(w, m, v, x, bad_a, c["d_a"], bad_b, c["d_b"], step=2, **HYPER)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, (w, m, v, x)))
    # mixed: the in-range occurrences give what they give alone
    mixed = host_sparse_adam_rows(w, m, v, x, c["ids_a"], c["d_a"], bad_b, c["d_b"], step=2, **HYPER)
    alone = host_sparse_adam_rows(w, m, v, x, c["ids_a"], c["d_a"], np.zeros(0, np.int64), np.zeros((0, 7), np.float32), step=2, **HYPER)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(mixed, alone))
    assert all(a.tobytes() == b.tobytes() for a, b in zip((w, m, v, x, c["d_a"], c["d_b"]), before))
    with pytest.raises(ValueError):
        host_sparse_adam_rows(w, m, v, x, c["ids_a"], c["d_a"], c["ids_b"], c["d_b"], step=0)


def test_the_float64_restatement_stays_within_the_gradient_gate_of_the_float32_one():
    """the cases the GPU test compares bit for bit are well conditioned: float32 against float64, held to the gate with the float32
    result as its own yardstick's bound (max error <= 1e-4 of the largest entry)"""
    from taxoexpan_amd.feature_table import host_sparse_adam_rows
    for case in CASES:
        for d in D_VALUES:
            c = draw_case(case, d)
            for amsgrad in (False, True):
                w, m, v, x = draw_state(d, amsgrad)
                args = (w, m, v, x, c["ids_a"], c["d_a"], c["ids_b"], c["d_b"])
                got32 = host_sparse_adam_rows(*args, step=3, trainable=c.get("trainable"), dtype=np.float32, **HYPER)
                got64 = host_sparse_adam_rows(*args, step=3, trainable=c.get("trainable"), dtype=np.float64, **HYPER)
                for name, a, b in zip("weight exp_avg exp_avg_sq max_exp_avg_sq".split(), got32, got64):
                    if a is None:
                        continue
                    err, scale = float(np.abs(a - b).max()), float(np.abs(b).max())
                    assert err <= 1e-4 * scale, (case, d, amsgrad, name, err / scale)


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """every refusal comes before any launch (a host buffer stands in for the device pointers: never read)"""
    from taxoexpan_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    need = lib.txe_rowgrad_ws_bytes(5, 3)
    assert need > 0 and lib.txe_rowgrad_ws_bytes(0, 0) > 0 and lib.txe_rowgrad_ws_bytes(-4, 3) == lib.txe_rowgrad_ws_bytes(0, 3)
    assert lib.txe_rowgrad_ws_bytes(2 ** 31 - 1, 2 ** 31 - 1) == 0
    group = dict(ids_a=a, n_a=5, ids_b=a, n_b=3, n_rows=37, ws=a, ws_bytes=need, stream=None)
    g = lambda **kw: lib.txe_rowgrad_group(*dict(group, **kw).values())
    assert g(n_a=-1) == -1 and g(n_b=-1) == -1 and g(n_rows=-1) == -1
    assert g(ids_a=None) == -1 and g(ids_b=None) == -1 and g(ws=None) == -1 and g(ws_bytes=need - 1) == -1 and g(ws_bytes=0) == -1
    assert g(n_a=2 ** 31 - 1, n_b=2 ** 31 - 1) == -1
    assert g(n_a=0, n_b=0, ids_a=None, ids_b=None, ws=None, ws_bytes=0) == 0                  # both sides empty: nothing to launch
    adam = dict(w=a, m=a, v=a, x=a, ld_w=7, n_rows=37, d=7, d_a=a, ld_a=7, n_a=5, d_b=a, ld_b=10, n_b=3, ws=a, ws_bytes=need, trainable=None,
                lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, step=1, first_bad=None, stream=None)
    s = lambda **kw: lib.txe_sparse_adam_rows(*dict(adam, **kw).values())
    assert s(n_a=-1) == -1 and s(n_b=-1) == -1 and s(n_rows=-1) == -1 and s(d=0) == -1
    assert s(d_a=None) == -1 and s(d_b=None) == -1 and s(w=None) == -1 and s(m=None) == -1 and s(v=None) == -1
    assert s(ld_a=6) == -1 and s(ld_b=6) == -1 and s(ld_w=6) == -1
    assert s(ws=None) == -1 and s(ws_bytes=need - 1) == -1
    assert s(step=0) == -1 and s(step=-3) == -1 and s(b1=1.0) == -1 and s(b2=-0.1) == -1
    assert s(n_a=2 ** 31 - 1, n_b=2 ** 31 - 1) == -1
    # an empty side needs neither its pointer nor a pitch; both empty: nothing to launch, ws not looked at -- but step is still checked
    assert s(n_a=0, n_b=0, d_a=None, d_b=None, ld_a=0, ld_b=0, ws=None, ws_bytes=0) == 0
    assert s(n_a=0, n_b=0, d_a=None, d_b=None, ws=None, ws_bytes=0, step=0) == -1
    run = dict(src=a, ld_src=7, run_off=a, U=2, G=5, r=7, dst=a, ld_dst=7, stream=None)
    r = lambda **kw: lib.txe_rows_run_sum(*dict(run, **kw).values())
    assert r(U=-1) == -1 and r(G=-1) == -1 and r(r=0) == -1 and r(ld_src=6) == -1 and r(ld_dst=6) == -1
    assert r(src=None) == -1 and r(run_off=None) == -1 and r(dst=None) == -1 and r(U=0, run_off=None, dst=None) == 0


def test_binding_table_and_header_agree_on_the_new_symbols():
    from taxoexpan_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "txe.h")).read(), flags=re.S)
    lib = _lib.load()
    cmap = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t, "double": ctypes.c_double}
    for name in ("txe_rowgrad_ws_bytes", "txe_rowgrad_group", "txe_sparse_adam_rows", "txe_rows_run_sum"):
        m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, name
        args = [x.strip() for x in m.group(2).replace("\n", " ").split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is cmap[m.group(1)] and len(args) == len(argtypes), name
        for arg, t in zip(args, argtypes):
            assert t is (ctypes.c_void_p if "*" in arg else cmap[arg.rsplit(" ", 1)[0].replace("const ", "").strip()]), (name, arg)
        assert hasattr(lib, name)
    assert not [k for k in re.findall(r"TXE_\w+", text) if "ROWGRAD" in k]        # no new TXE_* constant: test_cabi pins their count


def test_options_are_checked_before_any_gpu_work():
    from taxoexpan_amd import trainer
    from taxoexpan_amd.feature_table import FeatureTable
    with pytest.raises(RuntimeError, match="no CPU path"):
        FeatureTable(object(), "cpu", lr=1e-3)
    model = torch.nn.Linear(2, 1)
    before = [p.detach().clone() for p in model.parameters()]

    class _Opt(torch.optim.Adam):
        def step(self, closure=None, guard=None):
            raise AssertionError("no step may be taken")

    with pytest.raises(ValueError, match="feature_table"):
        trainer.train_epoch(model, [], _Opt(model.parameters(), lr=0.1), group_size=4, max_grad_norm=1.0, feature_table=object())
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), before))


def test_repeated_rows_on_the_host_keep_their_torch_backward():
    """ops.RepeatedRows.dense() takes the run-sum backward (txe_rows_run_sum) for rows ON THE DEVICE that ask for a gradient; host rows
    are expanded and differentiated by torch as ever"""
    from taxoexpan_amd import ops
    rows = torch.arange(6.0).reshape(3, 2).requires_grad_(True)
    rr = ops.RepeatedRows(rows, torch.tensor([0, 2, 3, 6], dtype=torch.int32), 6)
    dense = rr.dense()
    assert torch.equal(dense.detach(), rows.detach().repeat_interleave(torch.tensor([2, 1, 3]), dim=0))
    dense.backward(torch.ones(6, 2))
    assert rows.grad.tolist() == [[2.0, 2.0], [1.0, 1.0], [3.0, 3.0]]
