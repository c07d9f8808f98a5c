"""GPU: the trainable feature table.
  - txe_rowgrad_group + txe_sparse_adam_rows through the C ABI against feature_table.host_sparse_adam_rows in float32, bit for bit, and a
    second call on the same inputs gives equal bytes; the grouping itself against a stable numpy sort; first_bad freezes all four arrays
  - d_h and the distinct query rows' gradient of one training step against the float64 oracle's autograd (golden_util.gate_against_f64
    with its defaults, the fp32 oracle as the yardstick), on the default route of three model families; the same for the in-batch loss
    (ops.InBatchNCEFunction with query_grad=True): the op against torch float64 autograd, then a whole in-batch step
  - DeviceBatchLoader(feature_table=...): every batch's rows are the table as it stands when the batch is handed out
  - trainer.train_epoch(feature_table=...) against the float64 restatement iterated on the recorded per-occurrence gradients; two runs
    give equal bytes, also with in_batch=True; a planted NaN freezes model and table; trainer.fit checkpoints, restores and writes the
    table back
The sum of a row's occurrences has ONE order (csrc/txe_rowgrad.hip), so the kernel tests compare bytes, not tolerances; that the compared
cases are well conditioned is checked on the CPU (test_feature_table_cpu.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from feature_table_cases import CASES, D_VALUES, N_ROWS, draw_case, draw_state
from golden_util import gate_against_f64, load_case
from test_gpu_parity import _build_model, _graph
from test_gpu_trainer import _dev, _model, _toy

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

pytestmark = pytest.mark.gpu

HYPER = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)
NAMES = ("weight", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")


def _pitched(a, pitch, dev):
    """a [n, d] on the device as the [:, :d] view of an [n, pitch] allocation filled with NaN beside it (a read past d would show)"""
    n, d = a.shape
    base = torch.full((max(n, 1), pitch), float("nan"), dtype=torch.float32, device=dev)
    base[:n, :d] = torch.from_numpy(a).to(dev)
    return base[:n, :d]


class _Call:
    """device copies of one case and the two raw entry points (return codes, nothing raised)"""

    def __init__(self, case, state, dev, grad_pitch_extra=0, table_pitch_extra=0):
        from taxoexpan_amd import _lib
        self._lib, self.lib, self.dev = _lib, _lib.load(), dev
        d = state[0].shape[1]
        self.d = d
        self.ids = [torch.from_numpy(case[k].astype(np.int32)).to(dev) for k in ("ids_a", "ids_b")]
        self.grads = [_pitched(case[k], d + grad_pitch_extra, dev) for k in ("d_a", "d_b")]
        self.state = [None if a is None else _pitched(a, d + table_pitch_extra, dev) for a in state]
        self.trainable = None if case.get("trainable") is None else torch.from_numpy(case["trainable"]).to(dev)
        self.n = [int(t.numel()) for t in self.ids]
        self.ws_bytes = self.lib.txe_rowgrad_ws_bytes(*self.n)
        self.ws = torch.zeros(self.ws_bytes // 4 + 1, dtype=torch.int32, device=dev)

    def group(self):
        p = lambda t: t.data_ptr() if t.numel() else None
        return self.lib.txe_rowgrad_group(p(self.ids[0]), self.n[0], p(self.ids[1]), self.n[1], N_ROWS, self.ws.data_ptr(), self.ws_bytes,
                                          self._lib.stream_ptr())

    def adam(self, step, first_bad=None):
        w, m, v, x = self.state
        p = lambda t: t.data_ptr() if t is not None and t.numel() else None
        return self.lib.txe_sparse_adam_rows(w.data_ptr(), m.data_ptr(), v.data_ptr(), None if x is None else x.data_ptr(), w.stride(0), N_ROWS,
                                             self.d, p(self.grads[0]), self.grads[0].stride(0), self.n[0], p(self.grads[1]),
                                             self.grads[1].stride(0), self.n[1], self.ws.data_ptr(), self.ws_bytes, p(self.trainable),
                                             HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], step,
                                             None if first_bad is None else first_bad.data_ptr(), self._lib.stream_ptr())

    def host(self):
        torch.cuda.synchronize()
        return [None if t is None else t.cpu().numpy().copy() for t in self.state]


@pytest.mark.parametrize("d", D_VALUES)
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_equals_the_float32_restatement_bit_for_bit(case, d):
    """weight, exp_avg, exp_avg_sq and max_exp_avg_sq after one step (the table's third), amsgrad on and off, gradient pitch d and d + 3
    (with d + 3 the table's pitch is d + 3 as well: d = 513 then takes 16-byte accesses with an element tail, d = 7 8-byte ones)"""
    from taxoexpan_amd.feature_table import host_sparse_adam_rows
    dev = _dev()
    c = draw_case(case, d)
    for amsgrad in (False, True):
        state = draw_state(d, amsgrad)
        want = host_sparse_adam_rows(*state, c["ids_a"], c["d_a"], c["ids_b"], c["d_b"], step=3, trainable=c.get("trainable"), **HYPER)
        for extra in (0, 3):
            runs = []
            for _ in range(2):
                call = _Call(c, state, dev, grad_pitch_extra=extra, table_pitch_extra=extra)
                assert call.group() == 0 and call.adam(3) == 0
                runs.append(call.host())
            for name, a, b, w in zip(NAMES, runs[0], runs[1], want):
                assert (a is None and w is None) or a.tobytes() == w.tobytes(), (case, d, amsgrad, extra, name,
                                                                                  None if a is None else float(np.abs(a - w).max()))
                assert a is None or a.tobytes() == b.tobytes(), (name, "second call")
    if case not in ("both_empty",):
        assert want[0].tobytes() != state[0].tobytes()                       # (the step moved something)


def test_table_pitch_alone_and_unaligned_gradients():
    """d = 250 at pitch 250 (8-byte aligned rows: the training shape), and gradients that start 4 bytes into their allocation (element
    accesses) -- the same bytes as the restatement"""
    from taxoexpan_amd.feature_table import host_sparse_adam_rows
    dev = _dev()
    c = draw_case("mixed_lengths", 250)
    state = draw_state(250, True)
    want = host_sparse_adam_rows(*state, c["ids_a"], c["d_a"], c["ids_b"], c["d_b"], step=2, **HYPER)
    call = _Call(c, state, dev)
    assert call.state[0].stride(0) == 250 and call.state[0].data_ptr() % 16 == 0
    flat = torch.zeros(c["d_a"].size + 1, dtype=torch.float32, device=dev)
    flat[1:] = torch.from_numpy(c["d_a"]).to(dev).reshape(-1)
    call.grads[0] = flat[1:].view(-1, 250)
    assert call.grads[0].data_ptr() % 8 == 4
    assert call.group() == 0 and call.adam(2) == 0
    for name, a, w in zip(NAMES, call.host(), want):
        assert a.tobytes() == w.tobytes(), name


@pytest.mark.parametrize("case", ["out_of_range", "same_id_both_sides", "mixed_lengths", "a_empty", "all_distinct"])
def test_grouping_is_the_stable_sort_by_row(case):
    """the workspace after txe_rowgrad_group (include/txe.h has the layout): keys sorted, an out-of-range id keyed n_rows, occurrence
    indices ascending within a row (a's before b's), one head per distinct key"""
    dev = _dev()
    c = draw_case(case, 1)
    call = _Call(c, draw_state(1, False), dev)
    assert call.group() == 0
    torch.cuda.synchronize()
    ws = call.ws.cpu().numpy()
    ids = np.concatenate([c["ids_a"], c["ids_b"]])
    n = len(ids)
    keys = np.where((ids >= 0) & (ids < N_ROWS), ids, N_ROWS)
    order = np.argsort(keys, kind="stable")
    e = -(-max(n, 1) // 64) * 64
    heads = np.flatnonzero(np.concatenate([[True], keys[order][1:] != keys[order][:-1]]))
    assert ws[0] == len(heads)
    assert np.array_equal(ws[64:64 + n], keys[order]) and np.array_equal(ws[64 + e:64 + e + n], order)
    assert np.array_equal(ws[64 + 2 * e:64 + 2 * e + len(heads)], heads)


@pytest.mark.parametrize("amsgrad", [False, True])
def test_first_bad_freezes_all_four_arrays(amsgrad):
    dev = _dev()
    c = draw_case("mixed_lengths", 7)
    state = draw_state(7, amsgrad)
    call = _Call(c, state, dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)                      # first_bad = 0
    assert call.group() == 0 and call.adam(1, first_bad=bad) == 0
    for a, b in zip(call.host(), state):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()
    bad.fill_(-1)                                                            # -1: the step is taken
    assert call.adam(1, first_bad=bad) == 0
    assert call.host()[0].tobytes() != state[0].tobytes()


def test_run_sum_is_the_left_to_right_sum_of_each_run():
    from taxoexpan_amd import ops
    dev = _dev()
    rng = np.random.RandomState(3)
    cnt = np.array([1, 4, 33, 2, 70])
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    rows = torch.from_numpy(rng.randn(len(cnt), 250).astype(np.float32)).to(dev).requires_grad_(True)
    d_out = (rng.randn(int(cnt.sum()), 250) * 10.0 ** rng.randint(-3, 3, (int(cnt.sum()), 1))).astype(np.float32)
    rr = ops.RepeatedRows(rows, torch.from_numpy(off).to(dev), int(cnt.sum()))
    dense = rr.dense()
    assert torch.equal(dense.detach(), rows.detach().repeat_interleave(torch.from_numpy(cnt).to(dev), dim=0))
    dense.backward(torch.from_numpy(d_out).to(dev))
    want = np.zeros((len(cnt), 250), np.float32)
    for u in range(len(cnt)):
        s = d_out[off[u]].copy()
        for i in range(off[u] + 1, off[u + 1]):
            s = s + d_out[i]
        want[u] = s
    assert rows.grad.cpu().numpy().tobytes() == want.tobytes()


# ---- the model's gradients to its inputs ---------------------------------------------------------------------------------------------

def _oracle_input_grads(spec, params, graph, x, q_rows, cnt, dtype):
    """(d x, d distinct query rows) of the oracle's training step in `dtype`"""
    import txe_oracle as orc
    P = {k: torch.from_numpy(v).to(dtype) for k, v in params.items()}
    xc = torch.from_numpy(x).to(dtype).requires_grad_(True)
    qc = torch.from_numpy(q_rows).to(dtype).requires_grad_(True)
    qd = qc.repeat_interleave(torch.from_numpy(cnt), dim=0)
    if spec["match"] == "MLP":                                               # (taxoexpan_forward has the bilinear matchers only)
        hn = orc.pgat_forward(P, graph, xc, spec["heads"], spec["num_layers"], prefix="graph_propagate.")
        hg = orc.concat_readout(graph["graph_off"], hn, graph["pos"])
        s = orc.mlp_match(hg, qd, P["match.ffn.0.weight"], P["match.ffn.0.bias"], P["match.ffn.2.weight"], P["match.ffn.2.bias"])
    else:
        s, _hg, _hn = orc.taxoexpan_forward(P, graph, xc, qd, spec["prop"], spec["readout"], spec["match"], spec["heads"],
                                            spec["num_layers"], None)
    orc.info_nce_loss(s, spec["n_queries"]).backward()
    return xc.grad.numpy(), qc.grad.numpy()


@pytest.mark.parametrize("name", ["small_pgat_wmr_lbm", "mag_pgat_wmr_lbm_q8x32", "small_pgcn_mr_bim", "small_pgat_cr_mlp"])
def test_input_gradients_of_a_training_step_match_the_float64_oracle(name):
    """d_h (x = features[_id]) and the gradient of the DISTINCT query rows, on whatever route the model takes by itself when both ask
    for a gradient (train mode, dropout 0)"""
    from taxoexpan_amd import ops
    spec, z, shapes, x, q, params, graph = load_case(name)
    spec = dict(spec, dropout=(0.0, 0.0))
    dev = _dev()
    G, nq = q.shape[0], spec["n_queries"]
    rep = G // nq if spec.get("repeat_queries") else 1                       # the trainer's layout: one row per query, `rep` pairs each
    q_rows, cnt = q[::rep].copy(), np.full(G // rep, rep, dtype=np.int64)
    assert np.array_equal(np.repeat(q_rows, rep, axis=0), q)
    model = _build_model(spec, params).train()
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)).to(dev)
    target = torch.zeros(nq, dtype=torch.long, device=dev)

    def step(x_in, rows_in):
        ops.ROUTES.clear()
        scores = model(_graph(shapes), x_in, ops.RepeatedRows(rows_in, off, G))
        torch.nn.functional.cross_entropy(scores.reshape(nq, -1), target, reduction="sum").backward()
        return dict(ops.ROUTES)

    frozen = step(torch.from_numpy(x).to(dev), torch.from_numpy(q_rows).to(dev))       # the step as it is without a table
    xg = torch.from_numpy(x).to(dev).requires_grad_(True)
    rows = torch.from_numpy(q_rows).to(dev).requires_grad_(True)
    routes = step(xg, rows)
    assert xg.grad is not None and rows.grad is not None, routes
    # the route taken BY ITSELF: a bilinear matcher leaves the folded / runs forms, which have no query gradient, for the GEMM form, and
    # the stack then runs as it runs under that matcher route without a table; the MLP matcher and its stack keep their route
    if spec["match"] in ("BIM", "LBM"):
        assert routes.get("match") == "pair" and frozen.get("match") in ("folded", "runs", "pair"), (routes, frozen)
    else:
        assert routes.get("match") == frozen.get("match") and routes.get("stack") == frozen.get("stack"), (routes, frozen)
    assert routes.get("stack") in ("collapse", frozen.get("stack")), (routes, frozen)
    dx64, dq64 = _oracle_input_grads(spec, params, graph, x, q_rows, cnt, torch.float64)
    dx32, dq32 = _oracle_input_grads(spec, params, graph, x, q_rows, cnt, torch.float32)
    errors, report = [], []
    gate_against_f64(xg.grad.cpu().numpy(), dx64, dx32, "d_h", errors, report)
    gate_against_f64(rows.grad.cpu().numpy(), dq64, dq32, "d query rows", errors, report)
    print(f"\n[gate] {name} (match {routes.get('match')}, stack {routes.get('stack')}; without a table: match {frozen.get('match')}, stack "
          f"{frozen.get('stack')}): " +
          ", ".join(f"{w}: HIP {a:.3e}, fp32 oracle {b:.3e}" for w, a, b in report))
    assert not errors, "\n".join(errors)


# ---- the in-batch loss with a gradient to the query rows ------------------------------------------------------------------------------

@pytest.mark.parametrize("match", ["BIM", "LBM"])
@pytest.mark.parametrize("shape", [(12, 10, 3, 3), (500, 250, 4, 7)])
def test_in_batch_op_hands_the_query_rows_their_gradient(shape, match):
    """ops.InBatchNCEFunction(query_grad=True) against torch float64 autograd of the same expression (test_gpu_in_batch.py's cases and
    expression): d_q = dV W beside d_hg and dW, under exp (LBM) and without; d_hg, dW and the loss keep the bits they have without it"""
    from taxoexpan_amd import loss, model_zoo
    from taxoexpan_amd.loss import host_in_batch_valid
    from test_gpu_in_batch import _op_case, _torch_expr
    dev = _dev()
    l, r, Q, k = shape
    c = _op_case(*shape)
    apply_exp = match == "LBM"
    valid = torch.from_numpy(host_in_batch_valid(*c["args"]))
    pos = torch.from_numpy(c["args"][0].astype(np.int64))
    res = {}
    for dtype in (torch.float64, torch.float32):
        hg, W, q = (torch.from_numpy(c[n]).to(dtype).requires_grad_(True) for n in ("hg", "W", "q"))
        _torch_expr(hg, W, q, valid, pos, apply_exp).backward()
        res[dtype] = (hg.grad.numpy(), W.grad.numpy(), q.grad.numpy())
    m = (model_zoo.LBM if apply_exp else model_zoo.BIM)(l, r).to(dev)
    with torch.no_grad():
        m.W.weight.copy_(torch.from_numpy(c["W"]))
    groups = c["groups"](dev)
    hg = torch.from_numpy(c["hg"]).to(dev).requires_grad_(True)
    q = torch.from_numpy(c["q"]).to(dev).requires_grad_(True)
    out = loss.in_batch_info_nce(m, hg, q, groups, query_grad=True)
    out.backward()
    assert q.grad is not None and q.grad.shape == (Q, r)
    errors, report = [], []
    for what, got, i in (("d_hg", hg.grad, 0), ("dW", m.W.weight.grad, 1), ("d_q", q.grad, 2)):
        gate_against_f64(got.cpu().numpy(), res[torch.float64][i], res[torch.float32][i], what, errors, report)
    print(f"\n[gate] in-batch op {match} {shape}: " + ", ".join(f"{w}: HIP {a:.3e}, torch fp32 {b:.3e}" for w, a, b in report))
    assert not errors, "\n".join(errors)
    # without the flag and without a gradient asked for: the same loss, d_hg and dW, bit for bit
    m2 = (model_zoo.LBM if apply_exp else model_zoo.BIM)(l, r).to(dev)
    with torch.no_grad():
        m2.W.weight.copy_(torch.from_numpy(c["W"]))
    hg2 = torch.from_numpy(c["hg"]).to(dev).requires_grad_(True)
    out2 = loss.in_batch_info_nce(m2, hg2, torch.from_numpy(c["q"]).to(dev), groups)
    out2.backward()
    assert torch.equal(out2.detach(), out.detach()) and torch.equal(hg2.grad, hg.grad) and torch.equal(m2.W.weight.grad, m.W.weight.grad)
    with pytest.raises(ValueError, match="no gradient"):                     # ... and the flag is what lets such queries in
        loss.in_batch_info_nce(m2, hg2, q, groups)


def _synthetic_groups(Q, G, seed):
    """host arrays (pos_col, anchor, qnode, mask_ptr, mask_idx) of an in-batch layout over 40 made-up node ids: query i's positive is
    column i G / Q, its mask row names 12 of the ids"""
    rng = np.random.default_rng(seed)
    anchor = rng.integers(0, 40, size=G).astype(np.int32)
    qnode = rng.permutation(40)[:Q].astype(np.int32)
    rows = {int(v): np.sort(rng.choice(40, size=12, replace=False)) for v in qnode}
    mask_ptr = np.concatenate([[0], np.cumsum([len(rows.get(v, ())) for v in range(40)])]).astype(np.int32)
    mask_idx = np.concatenate([rows.get(v, np.zeros(0, dtype=np.int64)) for v in range(40)]).astype(np.int32)
    return (np.arange(Q) * (G // Q)).astype(np.int32), anchor, qnode, mask_ptr, mask_idx


@pytest.mark.parametrize("name", ["small_pgat_wmr_lbm", "mag_pgat_wmr_lbm_q8x32", "small_pgcn_mr_bim"])
def test_input_gradients_of_an_in_batch_step_match_the_float64_oracle(name):
    """x.grad and the query rows' gradient of one in-batch step as train_epoch(in_batch=True, feature_table=...) takes it -- encode_graph,
    loss.in_batch_info_nce(query_grad=True) -- against the oracle's encoder in float64 under the in-batch expression"""
    import txe_oracle as orc
    from taxoexpan_amd import encode_graph, loss
    from taxoexpan_amd.loss import host_in_batch_valid
    from taxoexpan_amd.sampler import InBatchGroups
    from test_gpu_in_batch import _torch_expr
    spec, z, shapes, x, q, params, graph = load_case(name)
    spec = dict(spec, dropout=(0.0, 0.0))
    dev = _dev()
    G, Q = q.shape[0], spec["n_queries"]
    q_rows = q[::G // Q].copy()                                              # one row per query
    args = _synthetic_groups(Q, G, seed=len(name))
    valid = torch.from_numpy(host_in_batch_valid(*args))
    pos_col = torch.from_numpy(args[0].astype(np.int64))
    apply_exp = spec["match"] == "LBM"
    res = {}
    for dtype in (torch.float64, torch.float32):
        P = {k: torch.from_numpy(v).to(dtype) for k, v in params.items()}
        xc = torch.from_numpy(x).to(dtype).requires_grad_(True)
        qc = torch.from_numpy(q_rows).to(dtype).requires_grad_(True)
        _s, hg, _hn = orc.taxoexpan_forward(P, graph, xc, qc.repeat_interleave(G // Q, dim=0), spec["prop"], spec["readout"], spec["match"],
                                            spec["heads"], spec["num_layers"], None)
        _torch_expr(hg, P["match.W.weight"], qc, valid, pos_col, apply_exp).backward()
        res[dtype] = (xc.grad.numpy(), qc.grad.numpy())
    model = _build_model(spec, params).train()
    g = _graph(shapes)
    xg = torch.from_numpy(x).to(dev).requires_grad_(True)
    rows = torch.from_numpy(q_rows).to(dev).requires_grad_(True)
    hg = encode_graph(model, g, xg, g.ndata["pos"].to(dev))
    loss.in_batch_info_nce(model.match, hg, rows, InBatchGroups.from_numpy(args[1], args[2], args[0], args[3], args[4], device=dev),
                           query_grad=True).backward()
    assert xg.grad is not None and rows.grad is not None
    errors, report = [], []
    gate_against_f64(xg.grad.cpu().numpy(), res[torch.float64][0], res[torch.float32][0], "d_h", errors, report)
    gate_against_f64(rows.grad.cpu().numpy(), res[torch.float64][1], res[torch.float32][1], "d query rows", errors, report)
    print(f"\n[gate] in-batch step {name}: " + ", ".join(f"{w}: HIP {a:.3e}, fp32 oracle {b:.3e}" for w, a, b in report))
    assert not errors, "\n".join(errors)


# ---- loader, trainer, fit ----------------------------------------------------------------------------------------------------------

def _table_and_loader(tmp_path, dev, lr, seed=5, **kw):
    from taxoexpan_amd.data_loaders import DeviceBatchLoader
    from taxoexpan_amd.feature_table import FeatureTable
    ds = _toy(tmp_path)
    table = FeatureTable(ds, dev, lr=lr, **kw)
    return ds, table, DeviceBatchLoader(ds, 16, dev, shuffle=True, seed=seed, sampler="device", feature_table=table)


class _Take:
    """the first n batches of a loader, with an optional edit of batch `at`"""

    def __init__(self, loader, n, at=None, edit=None):
        self.loader, self.n, self.at, self.edit, self.dataset = loader, n, at, edit, loader.dataset

    def __len__(self):
        return self.n

    def __iter__(self):
        for i, batch in enumerate(self.loader):
            if i >= self.n:
                break
            if i == self.at:
                self.edit(batch)
            yield batch


def test_loader_serves_the_table_as_it_stands(tmp_path):
    from taxoexpan_amd.data_loaders import DeviceBatchLoader
    from taxoexpan_amd.loss import info_nce_loss
    dev = _dev()
    ds, table, loader = _table_and_loader(tmp_path, dev, lr=0.05)
    with pytest.raises(ValueError, match="repeated_queries"):
        DeviceBatchLoader(ds, 16, dev, sampler="device", repeated_queries=False, feature_table=table)
    assert loader.features is table.weight and loader.dtax.features is table.weight
    first = table.weight.detach().clone()
    model = _model(dev).train()
    steps = 0
    for g, x, qf, _label in _Take(loader, 4):
        # the batch's rows are the table after the previous step, bit for bit (the side stream waited for it)
        assert torch.equal(x, table.weight.index_select(0, g.ndata["_id"].long()))
        assert g.query_ids.dtype == torch.int32 and g.query_ids.shape == (qf.rows.shape[0],)
        assert torch.equal(qf.rows, table.weight.index_select(0, g.query_ids.long()))
        x, qf, ids_a, ids_b = table.leaves(g, qf, x)
        assert ids_a is g.ndata["_id"] and ids_b is g.query_ids and x.requires_grad and qf.rows.requires_grad
        info_nce_loss(model(g, x, qf).reshape(-1, 4), None).backward()
        table.step()
        steps += 1
    assert steps == 4 and table.step_count == 4
    torch.cuda.synchronize()
    moved = (table.weight != first).any(dim=1)
    assert moved.any() and not moved.all()                                   # lazy: rows that never occurred are as they were
    assert torch.equal(table.exp_avg[~moved], torch.zeros_like(table.exp_avg[~moved]))
    # a loader without a table is what it was: no query_ids, its own resident copy
    plain = DeviceBatchLoader(_toy(tmp_path), 16, dev, shuffle=True, seed=5, sampler="device")
    g, _x, _qf, _l = next(iter(plain))
    assert not hasattr(g, "query_ids") and plain.feature_table is None


def _recording_table(tmp_path, dev, lr, in_batch=False, **kw):
    """(dataset, table, loader); the table keeps (ids_a, d_a, ids_b, d_b) of every step"""
    from taxoexpan_amd.data_loaders import DeviceBatchLoader
    from taxoexpan_amd.feature_table import FeatureTable

    class Recording(FeatureTable):
        def step(self, guard=None):
            x, rows, ids_a, ids_b = self._leaves
            self.seen.append(tuple(t.detach().cpu().numpy().copy() for t in (ids_a, x.grad, ids_b, rows.grad)))
            return super().step(guard=guard)

    ds = _toy(tmp_path)
    table = Recording(ds, dev, lr=lr, **kw)
    table.seen = []
    return ds, table, DeviceBatchLoader(ds, 16, dev, shuffle=True, seed=5, sampler="device", feature_table=table, in_batch=in_batch)


def _epoch(tmp_path, dev, state, n=3, lr=0.02, amsgrad=True, at=None, edit=None, **kw):
    from taxoexpan_amd import optim
    from taxoexpan_amd.trainer import train_epoch

    class RecordingAdam(optim.Adam):
        def step(self, closure=None, guard=None):
            self.seen.append([p.grad.detach().cpu().numpy().copy() for p in self.param_groups[0]["params"]])
            return super().step(closure, guard=guard)

    ds, table, loader = _recording_table(tmp_path, dev, lr, in_batch=bool(kw.get("in_batch")), amsgrad=amsgrad)
    model = _model(dev, state=state)
    opt = RecordingAdam(model.parameters(), lr=1e-3, amsgrad=True)
    opt.seen = []
    out = train_epoch(model, _Take(loader, n, at, edit), opt, group_size=None if kw.get("in_batch") else 4, feature_table=table, **kw)
    torch.cuda.synchronize()
    return model, opt, table, out


def _table_bytes(table):
    return [None if t is None else t.detach().cpu().numpy().tobytes() for t in (table.weight, table.exp_avg, table.exp_avg_sq, table.max_exp_avg_sq)]


def test_train_epoch_trains_the_table_like_the_float64_restatement(tmp_path):
    from taxoexpan_amd.feature_table import host_sparse_adam_rows
    from taxoexpan_amd.optim import host_guarded_adam
    dev = _dev()
    state = {k: v.detach().clone() for k, v in _model(dev).state_dict().items()}
    first = _toy(tmp_path).node_features.numpy().copy()
    model, opt, table, out = _epoch(tmp_path, dev, state)
    assert out["n_batches"] == 3 and out["first_nonfinite"] == -1 and table.step_count == 3 and len(table.seen) == 3
    # the table: float64 and float32 restatements iterated on the recorded per-occurrence gradients
    ref = {np.float64: None, np.float32: None}
    for dtype in ref:
        w, m, v, x = first.astype(dtype), np.zeros_like(first, dtype=dtype), np.zeros_like(first, dtype=dtype), np.zeros_like(first, dtype=dtype)
        for s, (ids_a, d_a, ids_b, d_b) in enumerate(table.seen):
            w, m, v, x = host_sparse_adam_rows(w, m, v, x, ids_a, d_a, ids_b, d_b, lr=0.02, step=s + 1, dtype=dtype)
        ref[dtype] = (w, m, v, x)
    errors, report = [], []
    for name, t, r64, r32 in zip(NAMES, (table.weight, table.exp_avg, table.exp_avg_sq, table.max_exp_avg_sq), ref[np.float64], ref[np.float32]):
        gate_against_f64(t.cpu().numpy(), r64, r32, "table " + name, errors, report)
        assert t.cpu().numpy().tobytes() == r32.tobytes(), name              # ... and the float32 restatement is the kernel itself
    # the model's parameters: host_guarded_adam in float64 iterated on the recorded gradients, as test_gpu_guarded_step.py holds them
    names = [k for k, _ in model.named_parameters()]
    for i, k in enumerate(names):
        for dtype, keep in ((np.float64, "r64"), (np.float32, "r32")):
            p = state[k].cpu().numpy().astype(dtype)
            m, v, x = np.zeros_like(p), np.zeros_like(p), np.zeros_like(p)
            for s, grads in enumerate(opt.seen):
                p, m, v, x = host_guarded_adam(p, grads[i], m, v, x, lr=1e-3, step=s + 1, dtype=dtype)
            if dtype == np.float64:
                r64 = p
            else:
                r32 = p
        gate_against_f64(dict(model.named_parameters())[k].detach().cpu().numpy(), r64, r32, k, errors, report)
    print("\n[gate] " + ", ".join(f"{w}: HIP {a:.3e}, fp32 {b:.3e}" for w, a, b in report))
    assert not errors, "\n".join(errors)
    assert (table.weight.cpu().numpy() != first).any()
    # grad_norms include the per-occurrence feature gradients
    for s in range(3):
        g2 = sum(float(np.sum(g.astype(np.float64) ** 2)) for g in opt.seen[s]) + \
            sum(float(np.sum(table.seen[s][i].astype(np.float64) ** 2)) for i in (1, 3))
        assert abs(out["grad_norms"][s] ** 2 - g2) <= 1e-9 * g2
    # two runs give equal bytes
    model_b, opt_b, table_b, out_b = _epoch(tmp_path, dev, state)
    assert _table_bytes(table) == _table_bytes(table_b) and out["losses"].tobytes() == out_b["losses"].tobytes()
    for (k, p), q in zip(model.named_parameters(), model_b.parameters()):
        assert torch.equal(p, q), k


def test_train_epoch_in_batch_trains_the_table(tmp_path):
    """train_epoch(in_batch=True, feature_table=t), 3 steps: the table moves, equals the restatement iterated on the recorded
    per-occurrence gradients (float32: the same bytes; float64: the gate), the query side contributes, and two runs give equal bytes"""
    from taxoexpan_amd.feature_table import host_sparse_adam_rows
    dev = _dev()
    state = {k: v.detach().clone() for k, v in _model(dev).state_dict().items()}
    first = _toy(tmp_path).node_features.numpy().copy()
    model, opt, table, out = _epoch(tmp_path, dev, state, in_batch=True)
    assert out["n_batches"] == 3 and out["first_nonfinite"] == -1 and table.step_count == 3 and out["mean_negatives"] > 3
    assert all(np.abs(seen[3]).max() > 0 and np.abs(seen[1]).max() > 0 for seen in table.seen)       # both sides carry a gradient
    ref = {}
    for dtype in (np.float64, np.float32):
        w, m, v, x = first.astype(dtype), np.zeros_like(first, dtype=dtype), np.zeros_like(first, dtype=dtype), np.zeros_like(first, dtype=dtype)
        for s, (ids_a, d_a, ids_b, d_b) in enumerate(table.seen):
            w, m, v, x = host_sparse_adam_rows(w, m, v, x, ids_a, d_a, ids_b, d_b, lr=0.02, step=s + 1, dtype=dtype)
        ref[dtype] = (w, m, v, x)
    errors, report = [], []
    for name, t, r64, r32 in zip(NAMES, (table.weight, table.exp_avg, table.exp_avg_sq, table.max_exp_avg_sq), ref[np.float64], ref[np.float32]):
        gate_against_f64(t.cpu().numpy(), r64, r32, "table " + name, errors, report)
        assert t.cpu().numpy().tobytes() == r32.tobytes(), name
    assert not errors, "\n".join(errors)
    assert (table.weight.cpu().numpy() != first).any()
    model_b, opt_b, table_b, out_b = _epoch(tmp_path, dev, state, in_batch=True)
    assert _table_bytes(table) == _table_bytes(table_b) and out["losses"].tobytes() == out_b["losses"].tobytes()
    for (k, p), q in zip(model.named_parameters(), model_b.parameters()):
        assert torch.equal(p, q), k
    # ... and it is another run than the grouped loss gives
    _m, _o, grouped, _out = _epoch(tmp_path, dev, state)
    assert _table_bytes(grouped) != _table_bytes(table)


def test_train_epoch_refuses_a_clip_and_freezes_on_a_planted_nan(tmp_path):
    from taxoexpan_amd import optim
    from taxoexpan_amd.trainer import train_epoch
    dev = _dev()
    state = {k: v.detach().clone() for k, v in _model(dev).state_dict().items()}
    ds, table, loader = _table_and_loader(tmp_path, dev, lr=0.02)
    model = _model(dev, state=state)
    before = table.weight.detach().clone()
    for opt, kw in ((optim.Adam(model.parameters(), lr=1e-3), dict(max_grad_norm=1.0)),
                    (optim.Adam(model.parameters(), lr=1e-3, max_grad_norm=2.0), dict())):
        with pytest.raises(ValueError, match="feature_table"):
            train_epoch(model, _Take(loader, 3), opt, group_size=4, feature_table=table, **kw)
    assert torch.equal(table.weight, before) and table.step_count == 0
    for k, p in model.named_parameters():
        assert torch.equal(p, state[k]), k
    with pytest.raises(ValueError, match="clip"):
        table.step(guard=optim.StepGuard(gnorm2=1234, max_grad_norm=1.0))

    def plant(batch):
        batch[2].rows[0, 0] = float("nan")                                   # one query row's features, in the gathered copy

    model, opt, table, out = _epoch(tmp_path, dev, state, n=4, at=2, edit=plant, freeze_on_nonfinite=True)
    assert out["first_nonfinite"] == 2 and out["n_batches"] == 4
    two_model, two_opt, two_table, two = _epoch(tmp_path, dev, state, n=2)
    assert two["losses"].tobytes() == out["losses"][:2].tobytes()
    assert _table_bytes(table) == _table_bytes(two_table)                    # the table froze with the model at step 2 ...
    for (k, p), q in zip(model.named_parameters(), two_model.parameters()):
        assert torch.equal(p, q), k
    assert table.step_count == 2 and all(float(st["step"]) == 2 for st in opt.state.values())       # ... and both counts were discounted
    assert torch.isfinite(table.weight).all()


def test_fit_checkpoints_restores_and_writes_back_the_table(tmp_path):
    from taxoexpan_amd import optim
    from taxoexpan_amd.data_loaders import DeviceBatchLoader
    from taxoexpan_amd.evaluate import evaluate
    from taxoexpan_amd.feature_table import FeatureTable
    from taxoexpan_amd.trainer import fit
    dev = _dev()
    ds, table, loader = _table_and_loader(tmp_path, dev, lr=0.05, amsgrad=True)
    valid_ds = _toy(tmp_path, "validation")
    valid = DeviceBatchLoader(valid_ds, 16, dev, shuffle=False, sampler="device")
    model = _model(dev)
    opt = optim.Adam(model.parameters(), lr=1e-3, amsgrad=True)
    first = ds.node_features.clone()
    logs = fit(model, loader, valid, opt, 1, monitor="off", save_dir=tmp_path / "run", feature_table=table)
    assert len(logs) == 1 and logs[0]["first_nonfinite"] == -1 and table.step_count == len(loader)
    # written back before the validation: the host table, the rows kv serves, the validation loader's dataset and resident copy
    host = table.weight.cpu()
    assert torch.equal(ds.node_features, host) and not torch.equal(host, first)
    assert np.array_equal(ds.kv[[str(i) for i in range(host.shape[0])]], host.numpy())
    assert torch.equal(valid_ds.node_features, host) and torch.equal(valid.features, table.weight)
    # the checkpoint round-trips the table bit for bit, into a table built from an untrained dataset
    ck = torch.load(tmp_path / "run" / "checkpoint-epoch1.pth", map_location="cpu", weights_only=False)
    assert "feature_table" in ck and ck["feature_table"]["step"] == len(loader)
    fresh = FeatureTable(_toy(tmp_path), dev, lr=1.0)
    assert not torch.equal(fresh.weight, table.weight)
    fresh.load_state_dict(ck["feature_table"])
    assert _table_bytes(fresh) == _table_bytes(table) and fresh.step_count == table.step_count
    assert (fresh.lr, fresh.betas, fresh.eps, fresh.amsgrad) == (table.lr, table.betas, table.eps, table.amsgrad)
    assert fresh.dtax.features is fresh.weight
    with pytest.raises(ValueError, match="shape"):
        fresh.load_state_dict(dict(ck["feature_table"], weight=ck["feature_table"]["weight"][:-1]))
    # resume restores it through fit; a checkpoint without a table is refused
    again_ds, again_table, again_loader = _table_and_loader(tmp_path, dev, lr=0.05, amsgrad=True)
    again = _model(dev)
    again_opt = optim.Adam(again.parameters(), lr=1e-3, amsgrad=True)
    fit(again, again_loader, None, again_opt, 1, monitor="off", resume=tmp_path / "run" / "checkpoint-epoch1.pth", feature_table=again_table)
    assert _table_bytes(again_table) == _table_bytes(table)                  # (epoch 1 was done: nothing more was trained)
    torch.save({k: v for k, v in ck.items() if k != "feature_table"}, tmp_path / "no_table.pth")
    with pytest.raises(ValueError, match="feature_table"):
        fit(again, again_loader, None, again_opt, 1, monitor="off", resume=tmp_path / "no_table.pth", feature_table=again_table)
    # the same model evaluated on the untrained features and on the written-back ones: the trained vectors are what evaluate serves
    untrained = evaluate(model, _toy(tmp_path, "validation"), dev, nll=True)[0]
    trained = evaluate(model, valid_ds, dev, nll=True)[0]
    assert np.isfinite(trained["nll"]) and trained["nll"] != untrained["nll"]
