"""GPU: the two propagation stacks' launch sequences and result bits, pinned against a recording of themselves.

tests/golden/stack_launches.json (written by tools/gen_stack_launch_golden.py, which runs run_case() below twice per case) holds, per
case, the ordered names of the launches the library's profiler records in forward and in backward, and a sha256 of the bytes of every
returned tensor and every gradient.  A tensor whose two recording runs disagreed bit for bit (a reduction whose order the hardware
decides) is recorded as "unstable" and only its launches are pinned here; the float64 / golden tests cover its values.

Every case is one branch of GATStackFunction / GCNStackFunction (ops.py): how the stack ends ('none' / 'mean' / 'layers' / 'collapse' /
'collapse_z'), which backward the folded layer takes, the table route of GatheredRows, the alternative routes behind ops._NO_*, an
empty batch.  Shapes: 24 egonets of 3-9 nodes, raw width 40, position width 8, vocabulary 3, hidden 16 (x 4 heads: the folded layer
reads 64 + 8 columns, for which txe_gat_fused_bwd_supported answers 1 and the fused-logits condition holds) or 10 (no fused
backward), output width 12."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stack_launches.json")
IN_DIM, POS_DIM, VOCAB, HID, OUT, DROP = 40, 8, 3, 16, 12, 0.1
SEED = 20261019
UNSTABLE = "unstable"
UNSTABLE_CAP = 0.1          # at most one recorded tensor in ten may be unstable


def _dev():
    return torch.device("cuda:0")


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def _profiled(fn):
    """fn() with the library profiler on: (fn's result, the names of the launches it recorded)"""
    from taxoexpan_amd import _lib
    lib = _lib.load()
    lib.txe_profile_reset()
    lib.txe_profile_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(64)
        ms, work, kind = ctypes.c_float(), ctypes.c_double(), ctypes.c_int()
        names = []
        for i in range(lib.txe_profile_count()):
            assert lib.txe_profile_get(i, buf, 64, ctypes.byref(ms), ctypes.byref(work), ctypes.byref(kind)) == 0
            names.append(buf.value.decode())
    finally:
        lib.txe_profile_enable(0)
        lib.txe_profile_reset()
    return out, names


_SHARED = {}


def _graph(empty=False):
    """a fresh batch (PGAT / PGCN pop ndata['pos']) of the shared shapes: 24 egonets of 3-9 nodes; the node features and query rows"""
    from taxoexpan_amd.graph import BatchedDGLGraph
    if empty:
        return BatchedDGLGraph.from_egonet_shapes([], [])
    if "shapes" not in _SHARED:
        rs = np.random.RandomState(SEED)
        n = rs.randint(3, 10, size=24)
        k = rs.randint(0, 3, size=24)
        gen = torch.Generator().manual_seed(SEED)
        _SHARED["shapes"] = (k, n - 1 - k)
        _SHARED["x"] = torch.randn(int(n.sum()), IN_DIM, generator=gen)
        _SHARED["q"] = torch.randn(6, IN_DIM, generator=gen)
        _SHARED["table"] = torch.randn(60, IN_DIM, generator=gen)
        _SHARED["index"] = torch.from_numpy(rs.randint(0, 60, size=int(n.sum())))
    return BatchedDGLGraph.from_egonet_shapes(*_SHARED["shapes"])


def _leaf(gen, *shape, scale=0.3):
    return (torch.randn(*shape, generator=gen) * scale).to(_dev()).requires_grad_(True)


def _gat_params(heads, dims, pos_dim):
    gen = torch.Generator().manual_seed(SEED + 1)
    named, kin = [], IN_DIM
    for l, (H, D) in enumerate(zip(heads, dims)):
        named += [(f"W{l}", _leaf(gen, H * D, kin + pos_dim)), (f"al{l}", _leaf(gen, 1, H, D)), (f"ar{l}", _leaf(gen, 1, H, D)),
                  (f"P{l}", _leaf(gen, VOCAB, pos_dim) if pos_dim else None)]
        kin = H * D
    return named


def _gcn_params(dims, pos_dim):
    gen = torch.Generator().manual_seed(SEED + 2)
    named, kin = [], IN_DIM
    for l, D in enumerate(dims):
        named += [(f"W{l}", _leaf(gen, kin + pos_dim, D)), (f"b{l}", _leaf(gen, D)), (f"P{l}", _leaf(gen, VOCAB, pos_dim) if pos_dim else None)]
        kin = D
    return named


def _record(forward, named, returned=lambda out: [("out", out)], may_refuse=False):
    """profiled forward, profiled backward of sum(out * fixed weights): launch names and the hashes of the outputs and of every gradient.
    may_refuse: a stack that is RUN on zero rows is refused by the library's argument checks before anything is launched (model_zoo
    never runs one where it can answer with zeros itself); what is pinned is that it stays a TxeError and not something worse."""
    from taxoexpan_amd import _lib
    try:
        out, fwd = _profiled(forward)
    except _lib.TxeError:
        if not may_refuse:
            raise
        return {"fwd": [], "bwd": [], "tensors": {}, "refused": "TxeError"}
    outs = returned(out)
    tensors = {k: _sha(t) for k, t in outs}
    bwd = []
    main = outs[0][1]
    if main.requires_grad:
        gen = torch.Generator().manual_seed(SEED + 3)
        w = torch.randn(main.shape, generator=gen).to(main.device)
        _, bwd = _profiled(lambda: (main * w).sum().backward())
        for k, p in named:
            if p is not None and p.requires_grad:
                tensors["d_" + k] = _sha(p.grad) if p.grad is not None else "none"
    return {"fwd": fwd, "bwd": bwd, "tensors": tensors}


def _stack(kind, final, heads=None, dims=None, pos_dim=POS_DIM, pw=False, h_grad=False, grad=True, table=False, slopes=None, drop=DROP,
           switches=()):
    """one apply_stack call on the shared batch"""
    from taxoexpan_amd import ops
    dev = _dev()
    g = _graph()
    csr = g.csr(dev)
    pos = g.ndata["pos"].to(dev)
    if table:
        h = ops.GatheredRows(_SHARED["table"].to(dev), _SHARED["index"].to(dev))
    else:
        h = _SHARED["x"].to(dev).requires_grad_(h_grad)
    gen = torch.Generator().manual_seed(SEED + 4)
    pw_t = _leaf(gen, VOCAB, 1, scale=1.0) if pw else None
    collapse = final in ("collapse", "collapse_z")
    if kind == "gat":
        named = _gat_params(heads, dims, pos_dim)
        cfg = ops.GATConfig(heads, dims, [pos_dim] * len(heads), VOCAB if pos_dim else 0, 0.2, None if final == "none" else 0.01, drop, drop,
                            final, SEED)
        fn = ops.GATStackFunction
    else:
        named = _gcn_params(dims, pos_dim)
        cfg = ops.GCNConfig(dims, VOCAB if pos_dim else 0, slopes, [drop] * len(dims), SEED)
        cfg.final = final
        fn = ops.GCNStackFunction
    args = (h, pos if pos_dim else None, pos if (collapse and pw) else None, pw_t) + tuple(p for _, p in named)
    olds = {s: getattr(ops, s) for s in switches}
    for s in switches:
        setattr(ops, s, True)
    try:
        with torch.set_grad_enabled(grad):
            return _record(lambda: ops.apply_stack(fn, csr, cfg, *args), named + [("h", None if table else h), ("pw", pw_t)])
    finally:
        for s, v in olds.items():
            setattr(ops, s, v)


def _model(prop, heads=None, bias=True, switches=(), grad_ready=False, empty=False, routes=None, readout="WMR", match="BIM"):
    """TaxoExpan(prop, WMR, BIM) on the shared batch with repeating queries (ops.RepeatedRows: 6 rows x 4), or on an empty batch"""
    from taxoexpan_amd import TaxoExpan, ops
    dev = _dev()
    torch.manual_seed(SEED + 5)
    model = TaxoExpan(prop, readout, match, in_dim=IN_DIM, hidden_dim=HID, out_dim=OUT, pos_dim=POS_DIM, num_layers=1, heads=heads,
                      feat_drop=DROP, attn_drop=DROP, hidden_drop=DROP, out_drop=DROP).to(dev).train()
    if not bias:
        model.graph_propagate.layers[-1].bias = None
    g = _graph(empty)
    if empty:
        x, q = torch.zeros(0, IN_DIM, device=dev), torch.zeros(0, IN_DIM, device=dev)
    else:
        x = _SHARED["x"].to(dev)
        q = ops.RepeatedRows(_SHARED["q"].to(dev), torch.arange(0, 25, 4, dtype=torch.int32, device=dev), 24)
    named = list(model.named_parameters())
    ids = {id(p): k for k, p in named}
    ready = []
    olds = {s: getattr(ops, s) for s in switches}
    old_ready = ops._GRAD_READY
    for s in switches:
        setattr(ops, s, True)
    if grad_ready:
        ops._GRAD_READY = lambda l, grads, pids: ready.append([l, len(grads), [ids.get(i, "none") for i in pids]])
    try:
        torch.manual_seed(SEED + 6)                # (the stack's dropout seed: ops.new_seed draws from torch's CPU generator)
        ops.ROUTES.clear()
        rec = _record(lambda: model(g, x, q), named, lambda s: [("scores", s)], may_refuse=empty)
        if routes is not None:
            got = {k: ops.ROUTES.get(k) for k in routes}
            assert got == routes, got
        rec["routes"] = {k: ops.ROUTES.get(k) for k in ("match", "stack", "stack_bwd", "fold")}
    finally:
        ops._GRAD_READY = old_ready
        for s, v in olds.items():
            setattr(ops, s, v)
    if grad_ready:
        rec["grad_ready"] = ready
    return rec


def _layer(cls, empty=True):
    """one model_zoo.GATLayer / GCNLayer module on the empty batch: a stack that runs with no rows"""
    from taxoexpan_amd import model_zoo as mz
    dev = _dev()
    torch.manual_seed(SEED + 7)
    if cls == "GATLayer":
        m = mz.GATLayer(IN_DIM, OUT, 3, DROP, DROP).to(dev).train()
    else:
        m = mz.GCNLayer(IN_DIM, OUT, torch.nn.functional.leaky_relu, DROP).to(dev).train()
    g = _graph(empty)
    x = torch.zeros(0, IN_DIM, device=dev)
    torch.manual_seed(SEED + 6)
    return _record(lambda: m(g, x), list(m.named_parameters()), may_refuse=True)


FOLDED = {"match": "folded", "stack": "collapse_z+edot"}
GCN_FOLDED = {"match": "folded", "stack": "collapse_z"}
CASES = {
    "gat_none_1layer_h3": lambda: _stack("gat", "none", [3], [OUT], pos_dim=0),
    "gat_mean_heads_4_2": lambda: _stack("gat", "mean", [4, 2], [HID, OUT], h_grad=True),
    "gat_mean_heads_4_1": lambda: _stack("gat", "mean", [4, 1], [HID, OUT]),
    "gat_collapse_1layer": lambda: _stack("gat", "collapse", [1], [OUT], pw=True),
    "gat_collapse_fused_pw": lambda: _stack("gat", "collapse", [4, 1], [HID, OUT], pw=True),
    "gat_collapse_fused": lambda: _stack("gat", "collapse", [4, 1], [HID, OUT]),
    "gat_collapse_unfused_shape_pw": lambda: _stack("gat", "collapse", [4, 1], [10, OUT], pw=True),
    "gat_collapse_unfused_shape": lambda: _stack("gat", "collapse", [4, 1], [10, OUT]),
    "gat_collapse_no_fused_bwd_pw": lambda: _stack("gat", "collapse", [4, 1], [HID, OUT], pw=True, switches=("_NO_FUSED_BWD",)),
    "pgat_wmr_bim_folded": lambda: _model("PGAT", [4, 1], routes=FOLDED),
    "pgat_folded_no_fused_logits": lambda: _model("PGAT", [4, 1], switches=("_NO_FUSED_LOGITS",), routes=FOLDED),
    "pgat_folded_no_tail_chain": lambda: _model("PGAT", [4, 1], switches=("_NO_TAIL_CHAIN",), routes=FOLDED),
    "pgat_folded_no_side_stream": lambda: _model("PGAT", [4, 1], switches=("_NO_SIDE_STREAM",), routes=FOLDED),
    "pgat_folded_grad_ready": lambda: _model("PGAT", [4, 1], grad_ready=True, routes=FOLDED),
    "gat_nograd_table_mean": lambda: _stack("gat", "mean", [4, 2], [HID, OUT], grad=False, table=True, drop=0.0),
    "gat_nograd_table_collapse": lambda: _stack("gat", "collapse", [4, 1], [HID, OUT], pw=True, grad=False, table=True, drop=0.0),
    "gcn_layers_2_activated": lambda: _stack("gcn", "layers", dims=[HID, OUT], slopes=[0.01, 0.01], h_grad=True),
    "gcn_one_activated_layer": lambda: _stack("gcn", "layers", dims=[OUT], slopes=[0.01], pos_dim=0),
    "gcn_collapse_pw": lambda: _stack("gcn", "collapse", dims=[HID, OUT], slopes=[0.01, None], pw=True),
    "gcn_collapse": lambda: _stack("gcn", "collapse", dims=[HID, OUT], slopes=[0.01, None]),
    "pgcn_bim_collapse_z_bias": lambda: _model("PGCN", routes=GCN_FOLDED),
    "pgcn_bim_collapse_z_no_bias": lambda: _model("PGCN", bias=False, routes=GCN_FOLDED),
    "gcn_nograd_table_layers": lambda: _stack("gcn", "layers", dims=[HID, OUT], slopes=[0.01, 0.01], grad=False, table=True, drop=0.0),
    "gcn_nograd_table_collapse": lambda: _stack("gcn", "collapse", dims=[HID, OUT], slopes=[0.01, None], pw=True, grad=False, table=True, drop=0.0),
    "empty_pgat_folding": lambda: _model("PGAT", [4, 1], empty=True),
    "empty_pgat_heads_4_2": lambda: _model("PGAT", [4, 2], empty=True),
    "empty_pgcn": lambda: _model("PGCN", empty=True),
    "empty_gat_layer": lambda: _layer("GATLayer"),
    "empty_gcn_layer": lambda: _layer("GCNLayer"),
}


def run_case(name):
    return CASES[name]()


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_shapes_take_the_branches_they_are_meant_to():
    """asked of the library's own predicates, not guessed"""
    from taxoexpan_amd import _lib
    assert _lib.call("txe_gat_fused_bwd_supported", 4 * HID, POS_DIM, 4, HID) == 1
    assert _lib.call("txe_gat_fused_bwd_supported", 4 * 10, POS_DIM, 4, 10) == 0
    kp = _lib.call("txe_gat_padded_k", 4 * HID, POS_DIM)
    assert HID % 4 == 0 and kp - 4 * HID <= 128                       # the fused-logits condition of GATStackFunction.forward
    assert _lib.call("txe_gat_collapse_e_tiles", int(_graph().csr(_dev()).n_nodes), 24, 4 * HID, POS_DIM) > 0
    assert (HID + POS_DIM) % 32 != 0                                  # the folded GCN layer's bias row has a padding column to ride in


def test_the_fixture_covers_every_case_and_is_mostly_stable():
    fx = _fixture()
    assert sorted(fx) == sorted(CASES)
    hashes = [v for c in fx.values() for v in c["tensors"].values()]
    assert sum(v == UNSTABLE for v in hashes) <= UNSTABLE_CAP * len(hashes)


@pytest.mark.parametrize("name", sorted(CASES))
def test_launches_and_bits_are_the_recorded_ones(name):
    want = _fixture()[name]
    got = run_case(name)
    assert got["fwd"] == want["fwd"]
    assert got["bwd"] == want["bwd"]
    assert got.get("routes") == want.get("routes")
    assert got.get("grad_ready") == want.get("grad_ready")
    assert got.get("refused") == want.get("refused")
    assert sorted(got["tensors"]) == sorted(want["tensors"])
    for k, v in want["tensors"].items():
        if v != UNSTABLE:
            assert got["tensors"][k] == v, k
