"""GPU: loss.bce_loss / square_exp_loss / margin_rank_loss (csrc/txe_pairloss.hip) against the reference's own values
(tests/golden/losses.npz, tools/gen_loss_golden.py) and the float64 restatements (loss.host_*): shapes at the lane, tile and workgroup
edges, both label widths, a strided column, special values, run-to-run determinism, autograd, the number of launches, the absence of a
host synchronisation, the training loop and the C ABI's refusals.

Gates (derived, not tuned).  Loss: with e_ref = |the reference's fp32 value - its float64 value| (0 where the fixture has no such case),
|HIP - f64| <= max(2 e_ref, (n_terms + 16) 2^-24 loss_f64): n_terms non-negative fp32 terms added in any order are at most n_terms 2^-24
relative off, plus a few ulp per term; n_terms = B (bce, square_exp) or the number of pairs (margin_rank).  Gradient, per element:
max(2 x the reference fp32 gradient's error, 4 x 2^-24 x max(1, |d_f64|)).  Margin-rank gradient: bit-equal to the reference's fp32 one."""
import ctypes
import inspect
import os
import random
import shutil
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_util import GOLDEN_DIR, gate_against_f64

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

pytestmark = pytest.mark.gpu

FUNCTIONS = ("bce_loss", "square_exp_loss", "margin_rank_loss")
EPS = 2.0 ** -24
MARGIN_LAUNCHES = 5                # flags, scan, index, pairs, finish


def _dev():
    return torch.device("cuda:0")


_GOLDEN = {}


def _golden():
    if not _GOLDEN:
        z = np.load(os.path.join(GOLDEN_DIR, "losses.npz"))
        _GOLDEN.update({k: z[k] for k in z.files})
    return _GOLDEN


def _case(name):
    return {k[len(name) + 2:]: v for k, v in _golden().items() if k.startswith(name + "__")}


def _pairs(label):
    """the group rule, written out: groups start at 0 and at every 0 -> 1 step; every (label 1, label != 1) pair of a group"""
    label = np.asarray(label)
    pi, ni, start = [], [], 0
    for i in range(1, len(label) + 1):
        if i == len(label) or (label[i - 1] == 0 and label[i] == 1):
            pos = [j for j in range(start, i) if label[j] == 1]
            neg = [j for j in range(start, i) if label[j] != 1]
            for p in pos:
                for n in neg:
                    pi.append(p)
                    ni.append(n)
            start = i
    return np.asarray(pi, dtype=np.int64), np.asarray(ni, dtype=np.int64)


def _torch_expr(fn, x, label, scalar, pairs=None):
    """the torch expression of each loss, from its definition (x [B] of any float dtype on any device, label [B])"""
    if fn == "bce_loss":
        return F.binary_cross_entropy_with_logits(x, (1 - label).to(x.dtype), reduction="sum")
    if fn == "square_exp_loss":
        return (x[label == 1] ** 2).sum() + scalar * torch.exp(-1.0 * x[label == 0]).sum()
    pi, ni = pairs if pairs is not None else _pairs(label.cpu().numpy())
    pi, ni = torch.as_tensor(pi, device=x.device), torch.as_tensor(ni, device=x.device)
    return torch.clamp_min((x[pi] - x[ni]) + scalar, 0).sum()


def _n_terms(fn, label):
    return len(_pairs(label)[0]) if fn == "margin_rank_loss" else len(label)


def _device_loss(fn, x, label, scalar, dev, column=False):
    """(loss fp32 as float, d_x fp32 numpy [B], the LossTensor) of one call; column: x is handed over as column 0 of a [B, 2] buffer
    whose other column is NaN"""
    from taxoexpan_amd import loss
    if column:
        buf = torch.full((len(x), 2), float("nan"), dtype=torch.float32, device=dev)
        buf[:, 0] = torch.from_numpy(x).to(dev)
        out = buf[:, 0:1].requires_grad_(True)
        assert out.shape == (len(x), 1) and out.stride(0) == 2
    else:
        out = torch.from_numpy(x).to(dev).requires_grad_(True)
    got = getattr(loss, fn)(out, torch.from_numpy(label).to(dev), scalar)
    (g,) = torch.autograd.grad(got, out)
    assert g.shape == out.shape and g.dtype == torch.float32
    return float(got.detach().cpu()), g.detach().reshape(-1).cpu().numpy(), got


def _check(fn, name, x, label, scalar, dev, ref=None, column=False):
    """one case against the float64 value: the fixture's (ref = the case's dict) or the restatement's"""
    from taxoexpan_amd import loss
    h_loss, h_d = getattr(loss, "host_" + fn)(x, label, scalar)
    if ref is not None and int(ref[fn + "_ok"]):
        l64, d64 = float(ref[fn + "_loss64"]), ref[fn + "_grad64"]
        e_ref, e_d = abs(float(ref[fn + "_loss32"]) - l64), np.abs(ref[fn + "_grad32"].astype(np.float64) - d64)
    else:
        l64, d64, e_ref, e_d = h_loss, h_d, 0.0, np.zeros(len(x))
    got, d, _t = _device_loss(fn, x, label, scalar, dev, column)
    n = _n_terms(fn, label)
    bound = max(2 * e_ref, (n + 16) * EPS * abs(l64))
    d_bound = np.maximum(2 * e_d, 4 * EPS * np.maximum(1.0, np.abs(d64)))
    d_err = np.abs(d.astype(np.float64) - d64)
    worst = float(np.max(d_err / d_bound, initial=0.0))
    print(f"{fn} {name} B={len(x)} {label.dtype}: |HIP - f64| = {abs(got - l64):.3e} (bound {bound:.3e}, reference fp32 {e_ref:.3e}); "
          f"gradient worst {float(np.max(d_err, initial=0.0)):.3e} = {worst:.2f} of its bound")
    assert abs(got - l64) <= bound, (fn, name, got, l64, bound)
    assert (d_err <= d_bound).all(), (fn, name, worst)
    if fn == "margin_rank_loss":
        want = ref[fn + "_grad32"] if ref is not None else h_d.astype(np.float32)
        assert torch.equal(torch.from_numpy(d), torch.from_numpy(want)), (fn, name)      # bit-exact integers
    return got, d


def _fixture_cases():
    return [n for n in ("b1", "b63", "b64", "b65", "b65_params", "b1025", "b1025_i32_params", "g3x200", "g3x200_i32_params")]


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_kernel_equals_the_reference_on_the_fixture_cases(fn):
    dev = _dev()
    assert set(_fixture_cases()) <= set(_golden()["cases"])
    for name in _fixture_cases():
        c = _case(name)
        scalar = float(c["margin"]) if fn == "margin_rank_loss" else float(c["beta"])
        _check(fn, name, c["x"], c["label"], scalar, dev, ref=c)
        other = c["label"].astype(np.int64 if c["label"].dtype == np.int32 else np.int32)       # the other label width: the same bits
        a = _device_loss(fn, c["x"], c["label"], scalar, dev)
        b = _device_loss(fn, c["x"], other, scalar, dev)
        assert np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes() and a[1].tobytes() == b[1].tobytes(), (fn, name)


def _extra_shapes():
    rng = np.random.RandomState(77)
    straddle = ([1] + [0] * 30) * 5                                    # 155 entries: groups 2 and 4 lie across the tile edges 64 and 128
    dom63 = _case("b63")["label"].tolist()
    dom64 = _case("b64")["label"].tolist()
    shapes = {"straddle": straddle, "two_pos_straddle": [1, 0] * 31 + [1, 1, 0, 0, 0], "starts_on_last_lane": dom63 + [1],
              "starts_on_a_new_tile": dom64 + [1], "all_positive": [1] * 70, "all_negative": [0] * 70, "other_labels": [1, 2, 0, 1, 3, 0, 0, 1, 1, 5]}
    return {k: (np.asarray(v), (rng.randn(len(v)) * 2.0).astype(np.float32)) for k, v in shapes.items()}


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_kernel_equals_the_restatement_on_edge_shapes(fn):
    dev = _dev()
    scalar = 0.5                                                       # (exact in fp32: restatement and kernel use the same number)
    for name, (label, x) in _extra_shapes().items():
        if fn == "bce_loss" and name == "other_labels":
            continue                                                   # bce's contract is {0, 1}
        for width in (np.int32, np.int64):
            _check(fn, name, x, label.astype(width), scalar, dev)
        a, da = _check(fn, name + "[column]", x, label.astype(np.int64), scalar, dev, column=True)
        b, db, _t = _device_loss(fn, x, label.astype(np.int64), scalar, dev)
        assert a == b and da.tobytes() == db.tobytes()
    # the shapes do what their names say
    assert len(_pairs(_extra_shapes()["starts_on_last_lane"][0])[0]) == len(_pairs(_case("b63")["label"])[0])
    assert len(_pairs([1] * 70)[0]) == 0 and len(_pairs([0] * 70)[0]) == 0 and len(_pairs(([1] + [0] * 30) * 5)[0]) == 150


def _klass(v):
    v = float(v)
    return "nan" if np.isnan(v) else ("+inf" if v == np.inf else ("-inf" if v == -np.inf else "finite"))


def test_special_values():
    from taxoexpan_amd import loss
    dev = _dev()
    label = np.asarray([1, 0, 0, 1, 1, 0, 0, 0], dtype=np.int64)
    base = np.asarray([0.3, -1.2, 2.0, 0.1, -0.7, 1.5, 0.2, -0.4], dtype=np.float32)

    def run(fn, x, scalar=1.0):
        got, d, _t = _device_loss(fn, x, label, scalar, dev)
        want = _torch_expr(fn, torch.from_numpy(x), torch.from_numpy(label), scalar)
        assert _klass(got) == _klass(want), (fn, x.tolist(), got, float(want))
        return got, d

    # +-1e4: bce stays finite and equals the restatement under the gate
    x = base.copy()
    x[0], x[1], x[2], x[3] = 1e4, -1e4, 1e4, -1e4
    got, d = run("bce_loss", x)
    h, hd = loss.host_bce_loss(x, label)
    assert np.isfinite(got) and np.isfinite(d).all() and abs(got - h) <= (len(x) + 16) * EPS * h
    assert (np.abs(d - hd) <= 4 * EPS * np.maximum(1.0, np.abs(hd))).all()
    _check("bce_loss", "+-1e4", x, label, 1.0, dev)
    # x = -100 on a negative: exp overflows in fp32
    x = base.copy()
    x[1] = -100.0
    got, d = run("square_exp_loss", x)
    assert got == np.inf and d[1] == -np.inf and np.isfinite(np.delete(d, 1)).all()
    # a NaN score in each loss (on a negative and on a positive): the loss is NaN
    for at in (1, 0):
        x = base.copy()
        x[at] = np.nan
        for fn in FUNCTIONS:
            got, d = run(fn, x)
            assert np.isnan(got), (fn, at)
            if fn == "margin_rank_loss":
                assert np.isfinite(d).all()                             # NaN never compares true: no pair of it is active
    # +Inf against +Inf in one pair is NaN too; a NaN in a group without a pair is not seen
    x = base.copy()
    x[0] = x[1] = np.inf
    assert np.isnan(run("margin_rank_loss", x)[0])
    lab1 = np.asarray([1, 1, 1], dtype=np.int64)
    g, _d, _t = _device_loss("margin_rank_loss", np.asarray([np.nan, 1.0, 2.0], dtype=np.float32), lab1, 1.0, dev)
    assert g == 0.0


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_two_calls_give_the_same_bits(fn):
    dev = _dev()
    for name in ("g3x200", "b1025"):                                   # 3 + 200: the positives receive counts from four tiles
        c = _case(name)
        runs = [_device_loss(fn, c["x"], c["label"], 1.0, dev) for _ in range(3)]
        for r in runs[1:]:
            assert np.float32(r[0]).tobytes() == np.float32(runs[0][0]).tobytes() and r[1].tobytes() == runs[0][1].tobytes()


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_autograd(fn):
    from taxoexpan_amd import loss
    dev = _dev()
    c = _case("b65")
    f = getattr(loss, fn)
    lab = torch.from_numpy(c["label"]).to(dev)
    _l, d, _t = _device_loss(fn, c["x"], c["label"], 1.0, dev)
    d = torch.from_numpy(d).to(dev)
    for shape in ((65,), (65, 1)):
        x = torch.from_numpy(c["x"]).to(dev).reshape(shape).requires_grad_(True)
        out = f(x, lab)
        assert isinstance(out, loss.LossTensor) and out.dim() == 0 and out.dtype == torch.float32
        out.backward()                                                 # the cached unit constant
        assert x.grad.shape == shape and torch.equal(x.grad.reshape(-1), d)
        x.grad = None
        (2.5 * f(x, lab)).backward()
        assert torch.equal(x.grad.reshape(-1), 2.5 * d)
        (g,) = torch.autograd.grad(f(x, lab), x, grad_outputs=torch.tensor(-3.0, device=dev))
        assert torch.equal(g.reshape(-1), -3.0 * d)
    # B == 0: a zero loss and an empty gradient; B == 1
    x0 = torch.zeros(0, device=dev, requires_grad=True)
    out = f(x0, torch.zeros(0, dtype=torch.int64, device=dev))
    out.backward()
    assert float(out) == 0.0 and x0.grad.shape == (0,) and isinstance(out, loss.LossTensor)
    x1 = torch.tensor([[0.3]], device=dev, requires_grad=True)
    out = f(x1, torch.ones(1, dtype=torch.int32, device=dev))
    out.backward()
    want, want_d = getattr(loss, "host_" + fn)(np.asarray([0.3], dtype=np.float32), np.ones(1, dtype=np.int32))
    assert abs(float(out) - want) <= 17 * EPS * want and abs(float(x1.grad) - want_d[0]) <= 4 * EPS
    # a half-precision score vector is made fp32 and gets a gradient of its own dtype; shape errors
    xh = torch.from_numpy(c["x"]).to(dev).half().requires_grad_(True)
    f(xh, lab).backward()
    assert xh.grad.dtype == torch.float16 and xh.grad.shape == (65,)
    with pytest.raises(ValueError):
        f(torch.zeros(4, 2, device=dev), torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        f(torch.zeros(4, device=dev), torch.zeros(3, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        f(torch.zeros(4, device=dev), torch.zeros(4, device=dev))


def test_launches_and_no_host_synchronisation():
    from taxoexpan_amd import _lib, loss
    dev = _dev()
    lib = _lib.load()
    c = _case("b1025")
    x, lab = torch.from_numpy(c["x"]).to(dev), torch.from_numpy(c["label"]).to(dev)
    for fn in FUNCTIONS:
        getattr(loss, fn)(x, lab)                                      # (first call: the workspace size is asked once and cached)
    torch.cuda.synchronize()
    counts = {}
    try:
        lib.txe_profile_enable(1)
        for fn in FUNCTIONS:
            lib.txe_profile_reset()
            getattr(loss, fn)(x, lab)
            counts[fn] = lib.txe_profile_count()
    finally:
        lib.txe_profile_enable(0)
        lib.txe_profile_reset()
    assert counts == {"bce_loss": 1, "square_exp_loss": 1, "margin_rank_loss": MARGIN_LAUNCHES}
    # no synchronisation: torch's own sync check is armed around forward and backward of each loss
    xs = x.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for fn in FUNCTIONS:
            getattr(loss, fn)(xs, lab).backward()
            getattr(loss, fn)(xs.reshape(-1, 1), lab.int()).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    src = inspect.getsource(loss._LabelledLoss) + inspect.getsource(loss._labelled) + inspect.getsource(loss._scaled)
    assert not any(w in src for w in (".item(", ".cpu(", ".tolist(", "synchronize", ".numpy("))
    # the workspace is a function of B alone: the entry point takes nothing else
    assert _lib.SIGNATURES["txe_margin_rank_loss_ws_bytes"][1] == [ctypes.c_int]
    assert lib.txe_margin_rank_loss_ws_bytes(1025) == lib.txe_margin_rank_loss_ws_bytes(1025) > 1025 * 28


def test_c_abi_refusals_write_nothing():
    from taxoexpan_amd import _lib
    dev = _dev()
    lib = _lib.load()
    B = 70
    x = torch.randn(B, device=dev)
    lab = torch.zeros(B, dtype=torch.int64, device=dev)
    lab[::7] = 1
    loss_t = torch.full((1,), 123.0, device=dev)
    d = torch.full((B,), 456.0, device=dev)
    need = lib.txe_margin_rank_loss_ws_bytes(B)
    ws = torch.full((need,), 7, dtype=torch.uint8, device=dev)
    X, LAB, LOSS, D, WS, S = x.data_ptr(), lab.data_ptr(), loss_t.data_ptr(), d.data_ptr(), ws.data_ptr(), _lib.stream_ptr()
    f32 = ctypes.c_float
    for args in ((None, LAB, 8, B, LOSS, D), (X, None, 8, B, LOSS, D), (X, LAB, 8, B, None, D), (X, LAB, 8, B, LOSS, None), (X, LAB, 8, 0, LOSS, D),
                 (X, LAB, 8, -3, LOSS, D), (X, LAB, 2, B, LOSS, D), (X, LAB, 16, B, LOSS, D)):
        assert lib.txe_bce_loss(*args, S) == -1
        assert lib.txe_square_exp_loss(*args[:4], f32(1.0), *args[4:], S) == -1
        assert lib.txe_margin_rank_loss(*args[:4], f32(1.0), *args[4:], WS, need, S) == -1
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert lib.txe_square_exp_loss(X, LAB, 8, B, f32(bad), LOSS, D, S) == -1
        assert lib.txe_margin_rank_loss(X, LAB, 8, B, f32(bad), LOSS, D, WS, need, S) == -1
    assert lib.txe_margin_rank_loss(X, LAB, 8, B, f32(1.0), LOSS, D, None, need, S) == -1
    assert lib.txe_margin_rank_loss(X, LAB, 8, B, f32(1.0), LOSS, D, WS, need - 1, S) == -3
    assert lib.txe_margin_rank_loss(X, LAB, 8, B, f32(1.0), LOSS, D, WS, 0, S) == -3
    torch.cuda.synchronize()
    assert float(loss_t) == 123.0 and bool((d == 456.0).all()) and bool((ws == 7).all())
    # ... and the same arguments without the fault are taken
    assert lib.txe_margin_rank_loss(X, LAB, 8, B, f32(1.0), LOSS, D, WS, need, S) == 0
    torch.cuda.synchronize()
    from taxoexpan_amd.loss import host_margin_rank_loss
    want, want_d = host_margin_rank_loss(x.cpu().numpy(), lab.cpu().numpy(), 1.0, dtype=np.float32)
    assert abs(float(loss_t) - want) <= (60 * 10 + 16) * EPS * want and np.array_equal(d.cpu().numpy().astype(np.float64), want_d)


# ---- the training loop ---------------------------------------------------------------------------------------------------------------

def _toy(tmp_path):
    from taxoexpan_amd.dataset import MAGDataset, MaskedGraphDataset
    d = tmp_path / "toy"
    d.mkdir(exist_ok=True)
    for fn in os.listdir(os.path.join(GOLDEN_DIR, "toy_taxo")):
        shutil.copy(os.path.join(GOLDEN_DIR, "toy_taxo", fn), d)
    random.seed(0)
    return MaskedGraphDataset(MAGDataset("toy", str(d), raw=True), mode="train", sampling_mode=1, negative_size=3, expand_factor=5,
                              normalize_embed=True)


def _loader(tmp_path, dev, seed=5):
    from taxoexpan_amd.data_loaders import DeviceBatchLoader
    return DeviceBatchLoader(_toy(tmp_path), 16, dev, shuffle=True, seed=seed, sampler="device")


def _model(dev, state=None):
    from taxoexpan_amd import TaxoExpan
    torch.manual_seed(0)
    m = TaxoExpan("PGAT", "WMR", "BIM", in_dim=8, hidden_dim=6, out_dim=5, pos_dim=3, num_layers=1, heads=[2, 1], feat_drop=0.0,
                  attn_drop=0.0, hidden_drop=0.0, out_drop=0.0).to(dev)
    if state is not None:
        m.load_state_dict(state, strict=True)
    return m


def _hand_written_epoch(model, loader, optimizer, fn, scalar):
    """trainer.py:41-77 with the torch expression of the loss on the device (margin-rank: the pair indices built on the host from the
    labels, as the reference does); returns per step (fp32 loss, the same expression in float64, n_terms)"""
    model.train()
    out = []
    for bg, h, nf, label in loader:
        optimizer.zero_grad()
        prediction = model(bg, h, nf)
        lab = label.cpu().numpy()
        pairs = _pairs(lab) if fn == "margin_rank_loss" else None
        loss = _torch_expr(fn, prediction.reshape(-1), label, scalar, pairs)
        loss.backward()
        optimizer.step()
        l64 = _torch_expr(fn, prediction.detach().reshape(-1).double(), label, scalar, pairs)
        out.append((loss.item(), l64.item(), len(pairs[0]) if pairs is not None else len(lab)))
    return out


def test_train_epoch_with_margin_rank_equals_the_hand_written_loop(tmp_path):
    """two epochs; the integer gradient makes both backward passes start from the same bits, so the parameters stay bit-equal"""
    from taxoexpan_amd import loss, optim
    from taxoexpan_amd.trainer import train_epoch
    dev = _dev()
    state = {k: v.clone() for k, v in _model(dev).state_dict().items()}
    a, b = _model(dev, state), _model(dev, state)
    opt_a, opt_b = (optim.Adam(m.parameters(), lr=1e-3, amsgrad=True) for m in (a, b))
    la, lb = _loader(tmp_path, dev), _loader(tmp_path, dev)
    for epoch in range(2):
        got = train_epoch(a, la, opt_a, loss_fn=loss.margin_rank_loss)
        want = _hand_written_epoch(b, lb, opt_b, "margin_rank_loss", 1.0)
        assert got["n_batches"] == len(want) == len(la) and got["first_nonfinite"] == -1
        for s, (l32, l64, n) in enumerate(want):
            bound = max(2 * abs(l32 - l64), (n + 16) * EPS * abs(l64))
            assert n > 0 and abs(float(got["losses"][s]) - l64) <= bound, (epoch, s, got["losses"][s], l32, l64, bound)
        for (k, p), q in zip(a.named_parameters(), b.parameters()):
            assert torch.equal(p, q), (epoch, k)
    assert any(float(p.detach().abs().sum()) != float(state[k].abs().sum()) for k, p in a.named_parameters())    # the parameters did move


def test_first_bce_step_beside_the_float64_oracle(tmp_path):
    """the first step of the toy loader with loss.bce_loss: the loss under the loss gate, and every parameter gradient under the
    project's gradient gate (golden_util.gate_against_f64: <= 2 x the fp32 yardstick's error against float64, floored at 2e-5) -- float64
    and the yardstick are the CPU oracle's forward with the torch expression of bce behind it"""
    import txe_oracle as orc
    from taxoexpan_amd import loss, ops
    dev = _dev()
    model = _model(dev)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    g, x, qf, label = next(iter(_loader(tmp_path, dev)))
    csr = g.csr(dev)
    deg = (csr.rowptr_in[1:] - csr.rowptr_in[:-1]).long()
    host = dict(src=csr.col_src.long().cpu(), dst=torch.repeat_interleave(torch.arange(deg.numel(), device=dev), deg).cpu(),
                pos=g.ndata["pos"].long().cpu(), graph_off=csr.graph_off.long().cpu(), num_nodes=int(deg.numel()))
    xh, qh, lh = x.cpu().clone(), ops.dense_rows(qf).cpu().clone(), label.cpu().clone()

    def oracle(dtype):
        P = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in state.items()}
        s, _hg, _hn = orc.taxoexpan_forward(P, host, xh.to(dtype), qh.to(dtype), "PGAT", "WMR", "BIM", [2, 1], 1, None)
        l = _torch_expr("bce_loss", s.reshape(-1), lh, 1.0)
        l.backward()
        return float(l.detach()), {k: p.grad.numpy() for k, p in P.items()}

    l64, g64 = oracle(torch.float64)
    l32, g32 = oracle(torch.float32)
    model.train()
    model.zero_grad()
    out = loss.bce_loss(model(g, x, qf), label)
    out.backward()
    got = float(out.detach().cpu())
    n = int(lh.numel())
    bound = max(2 * abs(l32 - l64), (n + 16) * EPS * abs(l64))
    print(f"\nfirst bce step: B = {n}, |HIP - f64| = {abs(got - l64):.3e}, fp32 oracle {abs(l32 - l64):.3e}, bound {bound:.3e}")
    assert abs(got - l64) <= bound, (got, l32, l64)
    errors, report = [], []
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        gate_against_f64(p.grad.detach().cpu().numpy(), g64[k], g32[k], k, errors, report)
    for what, e_got, e_yard in report:
        print(f"  {what}: HIP {e_got:.3e}, fp32 oracle {e_yard:.3e} of the largest float64 entry")
    assert not errors, errors
