"""CPU: the numpy restatements of the bce, square-exp and margin-rank losses (loss.host_*) against tests/golden/losses.npz -- what the
reference's own model/loss.py returns, loss and autograd gradient, in float64 (tools/gen_loss_golden.py) --, the documented deviation of
the margin-rank group rule, the group rule against metric._host_group_ranks' groups, and the argument errors."""
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN_DIR

FUNCTIONS = ("bce_loss", "square_exp_loss", "margin_rank_loss")


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN_DIR, "losses.npz"))
    return {k: z[k] for k in z.files}


def _case(golden, name):
    return {k[len(name) + 2:]: v for k, v in golden.items() if k.startswith(name + "__")}


def _host(fn, c):
    from taxoexpan_amd import loss
    scalar = float(c["margin"]) if fn == "margin_rank_loss" else float(c["beta"])
    return getattr(loss, "host_" + fn)(c["x"], c["label"], scalar)


def test_fixture_holds_the_cases_the_tests_need(golden):
    names = list(golden["cases"])
    sizes = {n: golden[n + "__x"].shape[0] for n in names}
    assert {1, 63, 64, 65, 1025, 203} <= set(sizes.values())
    assert {golden[n + "__label"].dtype for n in names} == {np.dtype(np.int32), np.dtype(np.int64)}
    assert any(float(golden[n + "__beta"]) == 0.5 and float(golden[n + "__margin"]) == 0.7 for n in names)
    assert golden["b1__label"].tolist() == [1] and golden["g3x200__label"].tolist() == [1] * 3 + [0] * 200
    for n in names:                                                    # the reference raises in one place only: its bce at B == 1
        for fn in FUNCTIONS:
            assert int(golden[f"{n}__{fn}_ok"]) == (0 if (fn == "bce_loss" and sizes[n] == 1) else 1), (n, fn)
            assert golden[f"{n}__{fn}_grad64"].dtype == np.float64 and golden[f"{n}__{fn}_grad32"].dtype == np.float32


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_restatement_equals_the_reference_in_float64(golden, fn):
    for name in golden["cases"]:
        c = _case(golden, name)
        if name.startswith("dev_") and fn == "margin_rank_loss":
            continue                                                   # the documented deviation: its own test below
        loss, d = _host(fn, c)
        assert d.dtype == np.float64 and d.shape == c["x"].shape
        if not int(c[fn + "_ok"]):
            continue                                                   # (bce at B == 1: the reference raises; the GPU test checks the definition)
        want, want_d = float(c[fn + "_loss64"]), c[fn + "_grad64"]
        assert abs(loss - want) <= 1e-12 * abs(want), (name, loss, want)
        if fn == "margin_rank_loss":
            assert np.array_equal(d, want_d), name                     # integers, exactly
            assert np.array_equal(d, c[fn + "_grad32"].astype(np.float64)), name
        else:
            assert np.max(np.abs(d - want_d), initial=0.0) <= 1e-12, (name, np.max(np.abs(d - want_d)))


def test_restatements_take_a_column_and_both_label_widths(golden):
    from taxoexpan_amd import loss
    c = _case(golden, "b65")
    for fn in FUNCTIONS:
        f = getattr(loss, "host_" + fn)
        a = f(c["x"], c["label"].astype(np.int32))
        b = f(c["x"].reshape(-1, 1), c["label"].astype(np.int64))
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
    # B == 1 (the reference's bce raises there): the definition, softplus(x) for a positive (target 1 - 1 = 0)
    x = _case(golden, "b1")["x"]
    l, d = loss.host_bce_loss(x, np.array([1]))
    assert abs(l - np.log1p(np.exp(float(x[0])))) <= 1e-15 * max(1.0, l) and abs(d[0] - 1.0 / (1.0 + np.exp(-float(x[0])))) <= 1e-15
    # B == 0
    for fn in FUNCTIONS:
        l, d = getattr(loss, "host_" + fn)(np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int64))
        assert l == 0.0 and d.shape == (0,)


def test_margin_rank_deviation_on_vectors_that_begin_with_a_zero(golden):
    """[0, 1, 0] and [0, 0, 1, 0]: the reference's regex bookkeeping pairs nothing (the fixture records its 0); the group rule makes the
    leading zeros a group of their own without a positive and pairs the [1, 0] that follows"""
    from taxoexpan_amd import loss
    for name, p, n in (("dev_010", 1, 2), ("dev_0010", 2, 3)):
        c = _case(golden, name)
        assert float(c["margin_rank_loss_loss64"]) == 0.0 and not c["margin_rank_loss_grad64"].any()          # the reference
        x = c["x"].astype(np.float64)
        term = (x[p] - x[n]) + 1.0
        l, d = loss.host_margin_rank_loss(c["x"], c["label"])
        want_d = np.zeros(len(x))
        if term > 0:
            want_d[p], want_d[n] = 1.0, -1.0
        assert l == max(term, 0.0) and np.array_equal(d, want_d)
        assert loss.group_starts(c["label"]).tolist() == [0, p]
    # at least one of the two is active with the fixture's scores, so the deviation is visible in the value, not only in the pairs
    assert any(loss.host_margin_rank_loss(golden[n + "__x"], golden[n + "__label"])[0] > 0 for n in ("dev_010", "dev_0010"))
    # inside the domain the issue's three hand cases
    for lab, pairs in (([1, 0, 1], [(0, 1)]), ([1, 0, 0, 1, 1], [(0, 1), (0, 2)]), ([1, 0, 0, 1, 1, 0], [(0, 1), (0, 2), (3, 5), (4, 5)])):
        pi, ni = loss.host_margin_pairs(np.asarray(lab))
        assert list(zip(pi.tolist(), ni.tolist())) == pairs


def test_group_rule_is_the_ranking_rule(golden):
    """the groups of host_margin_rank_loss = the groups of metric._host_group_ranks, on the fixture's label vectors and on vectors
    outside the reference's domain (labels other than 0 / 1, leading zeros, no zero at all)"""
    from taxoexpan_amd import loss
    from taxoexpan_amd.metric import _host_group_ranks
    rng = np.random.RandomState(3)
    labels = [golden[n + "__label"] for n in golden["cases"]]
    labels += [rng.randint(0, 3, size=n).astype(np.int64) for n in (2, 7, 64, 130)] + [np.ones(5, dtype=np.int32), np.zeros(4, dtype=np.int32)]
    for lab in labels:
        x = rng.randn(len(lab)).astype(np.float32)
        ranks, pos_off = _host_group_ranks(x, lab, 1)
        starts = loss.group_starts(lab)
        ends = np.append(starts[1:], len(lab))
        assert len(pos_off) == len(starts) + 1
        assert [int((lab[a:b] == 1).sum()) for a, b in zip(starts, ends)] == np.diff(pos_off).tolist()
        # mode 1 rank - 1 = the group's negatives strictly larger = the pairs with x_p - x_n < 0: with margin 0 the active pairs are the
        # OTHER ones, so per positive: active = negatives of the group - (rank - 1) - ties
        pi, ni = loss.host_margin_pairs(lab)
        _l, d = loss.host_margin_rank_loss(x, lab, margin=0.0)
        pos_idx = np.flatnonzero(lab == 1)
        for k, p in enumerate(pos_idx):
            mine = ni[pi == p]
            assert d[p] == len(mine) - (ranks[k] - 1) - int((x[mine] == x[p]).sum())


def test_argument_errors():
    from taxoexpan_amd import _lib, loss
    x, t = np.zeros(4, dtype=np.float32), np.zeros(4, dtype=np.int64)
    for f in (loss.host_bce_loss, loss.host_square_exp_loss, loss.host_margin_rank_loss):
        with pytest.raises(ValueError):
            f(x.reshape(2, 2), t)
        with pytest.raises(ValueError):
            f(x, t[:3])
        with pytest.raises(ValueError):
            f(x, t.astype(np.float32))
    for f in (loss.bce_loss, loss.square_exp_loss, loss.margin_rank_loss):
        with pytest.raises(RuntimeError, match="no CPU path"):        # a CPU tensor, as info_nce_loss
            f(torch.zeros(4), torch.zeros(4, dtype=torch.int64))
    # the C entry points refuse before any device work (host memory, never read)
    lib = _lib.load()
    import ctypes
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    f32 = ctypes.c_float
    for args in ((None, a, 8, 4, a, a), (a, None, 8, 4, a, a), (a, a, 8, 4, None, a), (a, a, 8, 4, a, None), (a, a, 8, 0, a, a), (a, a, 2, 4, a, a)):
        assert lib.txe_bce_loss(*args, None) == -1
        assert lib.txe_square_exp_loss(*args[:4], f32(1.0), *args[4:], None) == -1
        assert lib.txe_margin_rank_loss(*args[:4], f32(1.0), *args[4:], a, 1 << 20, None) == -1
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert lib.txe_square_exp_loss(a, a, 8, 4, f32(bad), a, a, None) == -1
        assert lib.txe_margin_rank_loss(a, a, 8, 4, f32(bad), a, a, a, 1 << 20, None) == -1
    assert lib.txe_margin_rank_loss(a, a, 8, 4, f32(1.0), a, a, None, 1 << 20, None) == -1
    need = lib.txe_margin_rank_loss_ws_bytes(4)
    assert need > 0 and lib.txe_margin_rank_loss_ws_bytes(0) == 0
    assert lib.txe_margin_rank_loss(a, a, 8, 4, f32(1.0), a, a, a, need - 1, None) == -3
    assert not any(buf)                                               # nothing was written
    sizes = [lib.txe_margin_rank_loss_ws_bytes(b) for b in (1, 64, 65, 1025, 1 << 18)]
    assert sizes == sorted(sizes) and sizes == [lib.txe_margin_rank_loss_ws_bytes(b) for b in (1, 64, 65, 1025, 1 << 18)]
