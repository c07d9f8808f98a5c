"""GPU parity at BASELINE.json's full sizes, and of the fused stack's per-layer intermediates.

* the whole training step of the three bench workloads (configs[1] PGAT+WMR+LBM, configs[4] PGCN+MR+BIM, configs[3]'s model PGAT
  num_layers=2 heads [4,4,1]) on the 4,096-egonet MAG-CS batch bench.py times -- training mode, dropout 0.1 -- against the CPU oracle
  run on the SAME full batch with the identical hash-generated dropout masks: scores, graph vectors, loss and every parameter gradient
  (reference: model_zoo.py:80-114,210-220, trainer/trainer.py:45-60, loss.py:52-57);
* the per-layer attention coefficients and layer outputs the reference goldens carry (`layer{l}_alpha`, `layer{l}_out`, captured from
  the unmodified model_zoo.GATLayer by oracle/gen_golden.py) against the buffers of the fused / folded stack: a compensating pair of
  errors inside the stack cannot hide behind correct final scores.
Tolerance: 1e-4 relative on logits / hidden states (north star).  Gradients are measured against the oracle run in FLOAT64, with the same
oracle in torch fp32 as the yardstick: for every gradient tensor max |HIP - f64| <= max(2 x max |fp32 oracle - f64|, 2e-5 max |f64|)
and <= 1e-4 max |f64| unless fp32 itself cannot (measured: ~1e-6 on both sides; the test prints the table).  The oracle is handed the branch each leaky_relu
took on the device (`_device_branches`), so all three differentiate the same piecewise-linear function;
* BASELINE configs[2] at its size: every MAG-CS candidate's graph vector, the whole score matrix and the ranks against the oracle,
  and a 30,000-egonet MAG-Full chunk."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_cases as gc
import txe_oracle as orc
from golden_util import load_case

pytestmark = pytest.mark.gpu

MAG = dict(in_dim=250, hidden_dim=500, out_dim=500, pos_dim=50, feat_drop=0.1, attn_drop=0.1, hidden_drop=0.1, out_drop=0.1)
WORKLOADS = {      # bench.py --workload name -> (propagation, readout, match, num_layers, heads)
    "pgat": ("PGAT", "WMR", "LBM", 1, [4, 1]),
    "pgcn": ("PGCN", "MR", "BIM", 1, None),
    "pgat2": ("PGAT", "WMR", "LBM", 2, [4, 4, 1]),
    "semeval": ("PGAT", "WMR", "LBM", 1, [4, 1]),      # BASELINE configs[0]: config.wordnet.json's dimensions on the SemEval-Noun shape
}
SEMEVAL = dict(in_dim=300, hidden_dim=600, out_dim=300, pos_dim=50, feat_drop=0.1, attn_drop=0.1, hidden_drop=0.1, out_drop=0.1)
N_QUERIES, NEG = 128, 31


def _dev():
    return torch.device("cuda:0")


def _close(got, ref, rtol, atol_rel, msg, errors):
    """|got - ref| <= rtol |ref| + atol_rel max|ref| + 2e-6 for EVERY entry -- no allowance for outliers: the oracle differentiates
    the same linear piece of every leaky_relu as the device did (`_device_branches`), so what is left is fp32 summation order."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (msg, got.shape, ref.shape)
    diff = np.abs(got - ref)
    tol = rtol * np.abs(ref) + atol_rel * np.abs(ref).max() + 2e-6
    bad = diff > tol
    if bad.any():
        errors.append(f"{msg}: {int(bad.sum())} of {bad.size} entries off, worst |diff| {diff.max():.3e} (max |ref| {np.abs(ref).max():.3e})")


def _device_branches(kind, states, src, dst, masks):
    """the branch every leaky_relu of the DEVICE forward pass took, added to the oracle's per-layer mask dicts (txe_oracle._leaky):
    leaky_relu' jumps at 0, and a pre-activation within rounding of 0 lands on the other side in another summation order -- the fp32
    oracle differs from its own float64 run by ~2e-3 of a tensor's largest entry on such rows.  With the branches given, both sides
    differentiate the same piecewise-linear function and every gradient entry is held to the plain tolerance.
      attention logits (model_zoo.py:106-109): z = a1[src] + a2[dst] from the projection's a1 / a2 columns (the folded output layer:
        its a12 buffer) -- the same fp32 add the kernel does;
      inter-layer activation (model_zoo.py:216 / :49): the sign of the activated row the layer wrote into the next layer's input
        (entries the next layer's dropout zeroed carry no gradient either way)."""
    L = len(states)
    for l, st in enumerate(states):
        if kind == "PGAT":
            H, F_ = st.H, st.H * st.D
            if l < L - 1 or st.cl is None:                            # (model_zoo._NO_FOLD: the output layer runs unfolded, like the others)
                a1, a2 = st.Y[:, F_:F_ + H].cpu().numpy(), st.Y[:, F_ + H:F_ + 2 * H].cpu().numpy()
            else:
                a12 = st.cl.a12.cpu().numpy()
                a1, a2 = a12[:, 0:1], a12[:, 1:2]
            z = a1[src] + a2[dst]                                     # float32 + float32, like the kernels
            masks[l]["e_pos"] = torch.from_numpy(z > 0).unsqueeze(-1)
            width = F_
        else:
            width = st.Fo
        if l < L - 1:
            masks[l]["act_pos"] = (states[l + 1].X[:, :width] > 0).cpu()
    return masks


def _masks(kind, P, heads, num_layers, N, E, seed, eid_in, pf, pa):
    """the keep masks the kernels regenerate from `seed` (taxoexpan_amd/rng.py restates the device hash), in the oracle's form"""
    from taxoexpan_amd import rng
    out = []
    for l in range(num_layers + 1):
        if kind == "PGAT":
            kt = P[f"graph_propagate.gat_layers.{l}.fc.weight"].shape[1]
            H = heads[l]
            m_csr = rng.keep_mask(seed + 16 * l + 1, (E, H), pa)              # destination-CSR order
            m_eid = np.empty_like(m_csr)
            m_eid[eid_in] = m_csr
            out.append(dict(feat_keep=torch.from_numpy(rng.keep_mask_bits(seed + 16 * l, N, kt, pf)), feat_scale=1.0 / (1.0 - pf),
                            attn_keep=torch.from_numpy(m_eid).unsqueeze(-1), attn_scale=1.0 / (1.0 - pa)))
        else:
            kt = P[f"graph_propagate.layers.{l}.weight"].shape[0]
            p = pf if l < num_layers else 0.1                                   # out_drop of the config (model.py:30-31), 0.1 as well
            out.append(dict(keep=torch.from_numpy(rng.keep_mask_bits(seed + 16 * l, N, kt, p)), keep_scale=1.0 / (1.0 - p)))
    return out


def _expected_routes(prop, form):
    """the routes the step must take with the library's switches as they are (TXE_TEST_ROUTE flips one for a whole run): the DEFAULT for
    the three PGAT workloads is the one bench.py times -- stack 'collapse_z+edot', matcher 'folded' on the e_part scores, backward
    'fused+edot' -- and a test that silently ran anything else is a test of something else"""
    from taxoexpan_amd import model_zoo as mz, ops
    runs_ok = form == "rows" or not ops._NO_QUERY_RUNS
    can_fold = not (ops._NO_MATCH_FOLD or mz._NO_FOLD) and (prop != "PGAT" or not ops._NO_FUSED_BWD)
    fold = runs_ok and can_fold
    edot = fold and prop == "PGAT" and not ops._NO_FOLD_EDOT and form != "hook"
    match = "folded" if fold else (("runs" if form == "rows" else "stacked") if runs_ok else "pair")
    if mz._NO_FOLD:
        stack = "mean" if prop == "PGAT" else "layers"
    else:
        stack = ("collapse_z" + ("+edot" if edot else "")) if fold else "collapse"
    fold_kind = ("edot" if edot else "inline") if fold else None      # (the matcher's job is only handed to the stack for the sweep to carry T)
    if not fold and form == "hook" and can_fold:                        # the hook's .detach() ran the stack up to Z; hg = Z W^T materialised afterwards
        stack, fold_kind = "collapse_z", "materialised"
    bwd = "fused+edot" if edot else (("collapse" if not mz._NO_FOLD else "layers") if prop == "PGAT" else None)
    return dict(match=match, stack=stack, fold=fold_kind, stack_bwd=bwd)


def _graph_vectors_from_capture(prop, states, model, D):
    """hg [G, D] from the folded output layer's saved Z (nothing in the step is touched: no hook, no materialisation)"""
    st = states[-1]
    if st.cl is None:
        return None
    Z = st.cl.Z.detach()
    if prop == "PGAT":
        if st.cl.hg is not None:
            return st.cl.hg.detach().cpu().numpy()
        return (Z.double() @ st.Wp[:D].detach().double().t()).float().cpu().numpy()
    return (Z.double() @ st.Wp[:Z.shape[1], :D].double() + st.b.detach().double()).float().cpu().numpy()


@pytest.mark.parametrize("workload,form", [("pgat", "stacked"), ("pgat", "rows"), ("pgat", "hook"), ("pgcn", "stacked"), ("pgat2", "stacked"),
                                           ("semeval", "stacked"), ("semeval", "rows"), ("pgcn", "rows"), ("pgcn", "hook")])
def test_full_size_training_step_matches_oracle(workload, form, monkeypatch):
    """form: how the queries arrive / who else looks at the graph vector --
      'stacked': the reference collate's [G, r] matrix (data_loaders.py:9-28), nothing else touches the step: THE ROUTE bench.py TIMES;
      'rows':    ops.RepeatedRows (DeviceBatchLoader(repeated_queries=True));
      'hook':    a forward hook on the readout that logs `out.detach()` (what gen_golden.py does to the reference): the fold stays, its
                 query-side job cannot ride in the sweep any more (the in-line kernels).
    The routes are ASSERTED (_expected_routes); scores, graph vectors, loss and every gradient entry against the oracle."""
    from taxoexpan_amd import TaxoExpan, ops, synthetic as syn
    prop, readout, match, num_layers, heads = WORKLOADS[workload]
    dev = _dev()
    # (bench.py times `pgat2` -- BASELINE configs[3] -- on the MAG-Full-shaped taxonomy, `pgat` / `pgcn` on the MAG-CS one; `semeval` is
    #  configs[0]'s shape: 64 queries x 32 = 2,048 egonets, d = 300 -- its 350-column layer input ends 2 columns short of the padded row,
    #  so the streaming d_X kernel's weight slab runs past it: clamped column vectors)
    dims = SEMEVAL if workload == "semeval" else MAG
    n_queries = 64 if workload == "semeval" else N_QUERIES
    tax = syn.make_named_taxonomy({"pgat2": "mag_full", "semeval": "semeval_noun"}.get(workload, "mag_cs"), seed=47)
    g, qf, _labels = syn.training_batch(tax, n_queries, NEG, seed=1000)          # batch 0 of bench.py's rank 0
    assert g.batch_size == n_queries * 32
    x = g.ndata.pop("x")
    pos = g.ndata["pos"].clone()
    torch.manual_seed(47)
    model = TaxoExpan(prop, readout, match, **dict(dims, num_layers=num_layers, heads=heads)).to(dev).train()
    seed = 987654321
    monkeypatch.setattr(ops, "new_seed", lambda: seed)
    caps = {}
    if form == "hook":
        model.readout.register_forward_hook(lambda m, i, o: caps.__setitem__("hg", o.detach().cpu().numpy()))
    q_dev = qf.to(dev)
    if form == "rows":
        q_arg = ops.RepeatedRows(q_dev[::32].contiguous(), torch.arange(0, n_queries * 32 + 1, 32, dtype=torch.int32, device=dev), n_queries * 32)
        assert torch.equal(q_arg.dense(), q_dev)
    else:
        q_arg = q_dev
    with ops.debug_capture() as runs:
        scores = model(g, x.to(dev), q_arg)
    assert len(runs) == 1
    _csr_dev, _cfg, states = runs[0]
    want = _expected_routes(prop, form)
    taken = dict(runs.routes)
    for kind in ("match", "stack", "fold"):
        assert taken.get(kind) == want[kind], (kind, taken, want)
    if "hg" not in caps:
        caps["hg"] = _graph_vectors_from_capture(prop, states, model, dims["out_dim"])
    src_np, dst_np = np.asarray(g._src), np.asarray(g._dst)
    branches = _device_branches("PGAT" if prop == "PGAT" else "PGCN", states, src_np, dst_np, [{} for _ in states])   # (before backward frees anything)
    loss = F.cross_entropy(scores.reshape(n_queries, -1), torch.zeros(n_queries, dtype=torch.long, device=dev), reduction="sum")
    ops.ROUTES.pop("stack_bwd", None)
    loss.backward()
    torch.cuda.synchronize()
    assert ops.ROUTES.get("stack_bwd") == want["stack_bwd"], (ops.ROUTES, want)

    # ---- the oracle on the same egonets, same parameters, same masks ----
    csr = g.csr("cpu")
    N, E = csr.n_nodes, csr.n_edges
    P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}      # THE REFERENCE: float64
    P32 = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.state_dict().items()}     # the yardstick: the same oracle in fp32
    graph = dict(src=torch.from_numpy(np.asarray(g._src)).long(), dst=torch.from_numpy(np.asarray(g._dst)).long(), pos=pos.long(),
                 graph_off=csr.graph_off.long(), num_nodes=N)
    masks = _masks("PGAT" if prop == "PGAT" else "PGCN", P, heads, num_layers, N, E, seed, csr.eid_in.numpy(), 0.1, 0.1)
    for mk, br in zip(masks, branches):
        mk.update(br)
    monkeypatch.setattr(orc, "BRANCH_AUDIT", [])
    s_ref, hg_ref, _ = orc.taxoexpan_forward(P, graph, x.double(), qf.double(), prop, readout, match, heads, num_layers, masks)
    # the device's branch pattern may differ from the oracle's own only where the pre-activation is within rounding of 0: a wrongly
    # signed LARGE logit / activation on the device would otherwise be handed to the oracle and cancel out of the comparison
    audit = list(orc.BRANCH_AUDIT)
    assert len(audit) >= 1, audit
    for tag, n_dis, worst, biggest, numel in audit:
        assert worst <= 1e-4 * biggest and n_dis <= 1e-3 * numel, (tag, n_dis, worst, biggest, numel)
    l_ref = orc.info_nce_loss(s_ref, n_queries)
    l_ref.backward()
    s_32, hg_32, _ = orc.taxoexpan_forward(P32, graph, x, qf, prop, readout, match, heads, num_layers, masks)    # (same masks, same branches)
    orc.info_nce_loss(s_32, n_queries).backward()

    errors = []
    if caps["hg"] is not None:
        _close(caps["hg"], hg_ref.detach().numpy(), 1e-4, 2e-5, "hg", errors)
    else:
        from taxoexpan_amd import model_zoo as mz
        assert mz._NO_FOLD                                                       # (only the unfolded test route has no saved Z to read hg from)
    _close(scores.detach().cpu().numpy(), s_ref.detach().numpy(), 1e-4, 2e-5, "scores", errors)
    np.testing.assert_allclose(loss.item(), l_ref.item(), rtol=1e-4)
    # gradients: the north star's "within 1e-4 fp32".  Reference = the float64 oracle; yardstick = the SAME oracle in torch fp32 (what the
    # reference's own arithmetic gives).  Every gradient tensor: max |HIP - f64| <= 2 x max |fp32 oracle - f64| (no worse than fp32
    # arithmetic in another summation order; both are maxima over thousands of entries), floored at 2e-5 of the tensor's largest entry (a
    # tensor the fp32 oracle happens to get to 1e-7 must not fail the device at 2e-7) -- and <= 1e-4 of the tensor's largest entry unless
    # fp32 arithmetic itself cannot reach that (golden_util.gate_against_f64)
    report = []
    scale_floor = 1e-3 * max(float(P[k].grad.abs().max()) for k in P)          # (a tensor whose exact gradient is ~0 is judged on the model's scale)
    for k, p in model.named_parameters():
        ref = P[k].grad.numpy()
        scale = max(float(np.abs(ref).max()), scale_floor)
        e_hip = float(np.abs(p.grad.cpu().double().numpy() - ref).max())
        e_32 = float(np.abs(P32[k].grad.double().numpy() - ref).max())
        report.append((k, e_hip / scale, e_32 / scale))
        if not (e_hip <= max(2.0 * e_32, 2e-5 * scale) and e_hip <= max(1e-4 * scale, 2.0 * e_32)):
            errors.append(f"grad {k}: max |HIP - f64| = {e_hip / scale:.3e} of max |ref|, the fp32 oracle's {e_32 / scale:.3e}")
    print(f"\n[{workload}-{form}] gradient error vs the float64 oracle, as a fraction of the tensor's largest entry (HIP | fp32 oracle):")
    for k, a, b in report:
        print(f"    {k:60s} {a:.3e} | {b:.3e}")
    assert not errors, "\n".join(errors)


GAT_GOLDENS = [n for n, s in gc.CASES.items() if s["prop"] == "PGAT" and not s.get("dropout") and s["readout"] in ("WMR", "MR")]


@pytest.mark.parametrize("name", GAT_GOLDENS)
def test_fused_stack_intermediates_match_reference_goldens(name):
    """layer{l}_alpha (model_zoo.py:112-114, edge-id order) and layer{l}_out (GATLayer.forward's return, :95-104; every 5th node row
    for the MAG-dimension cases) of the reference run against the fused stack: hidden layers through the aggregation kernel's
    activated output (the next layer's padded input), the folded output layer through its attention buffer and, unfolded, `h.tensor()`"""
    from taxoexpan_amd import TaxoExpan, model_zoo, ops
    from taxoexpan_amd.graph import BatchedDGLGraph
    if model_zoo._NO_FOLD:
        pytest.skip("model_zoo._NO_FOLD: the folded output layer this test looks into is switched off")
    spec, z, shapes, x, q, params, graph = load_case(name)
    dev = _dev()
    model = TaxoExpan(spec["prop"], spec["readout"], spec["match"], in_dim=spec["in_dim"], hidden_dim=spec["hidden_dim"], out_dim=spec["out_dim"],
                      pos_dim=spec["pos_dim"], num_layers=spec["num_layers"], heads=spec["heads"], feat_drop=0.1, attn_drop=0.1,
                      hidden_drop=0.1, out_drop=0.1)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    model = model.to(dev).eval()
    g = BatchedDGLGraph.from_egonet_shapes([s[0] for s in shapes], [s[1] for s in shapes])
    with ops.debug_capture() as runs:
        scores = model(g, torch.from_numpy(x).to(dev), torch.from_numpy(q).to(dev))       # grad mode on: the stack keeps its state
    assert len(runs) == 1
    csr, cfg, states = runs[0]
    L = len(states)
    eid = csr.eid_in.long()
    step = gc.row_steps(spec)[1]
    for l, st in enumerate(states):
        H, D = st.H, st.D
        want_alpha = torch.from_numpy(z[f"layer{l}_alpha"]).reshape(-1, H)
        want_out = torch.from_numpy(z[f"layer{l}_out"]).reshape(-1, H * D)
        if l < L - 1:
            alpha = torch.empty_like(want_alpha)
            alpha[eid.cpu()] = st.alpha.cpu()
            nxt = states[l + 1]
            got_out = nxt.X[:, :H * D].cpu()[::step]                                        # = leaky_relu(out), slope 0.01
            np.testing.assert_allclose(got_out.numpy(), F.leaky_relu(want_out, 0.01).numpy(), rtol=1e-4, atol=2e-5, err_msg=f"layer {l} out")
        else:                                                                                # folded one-head output layer
            assert cfg.final in ("collapse", "collapse_z") and st.cl is not None
            alpha = torch.empty_like(want_alpha)
            alpha[eid.cpu()] = st.cl.alpha.cpu().reshape(-1, 1)
            hn = g.ndata["h"].tensor().detach().cpu()[::step]                              # the same layer, unfolded: N x out_dim
            np.testing.assert_allclose(hn.numpy(), want_out.numpy(), rtol=1e-4, atol=2e-5, err_msg=f"layer {l} out (unfolded)")
        np.testing.assert_allclose(alpha.numpy(), want_alpha.numpy(), rtol=1e-4, atol=2e-6, err_msg=f"layer {l} alpha")
    np.testing.assert_allclose(scores.detach().cpu().numpy(), z["scores"], rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("heads,hidden,drop,layers,empties", [([4, 1], 500, 0.1, 1, 0), ([4, 1], 8, 0.0, 1, 0), ([2, 1], 24, 0.2, 1, 0), ([1, 1], 32, 0.2, 1, 0),
                                                              ([4, 1], 600, 0.1, 1, 0), ([3, 4, 1], 12, 0.1, 2, 0), ([4, 1], 100, 0.0, 1, 0),
                                                              # 45 EMPTY graphs in the batch: a window of the egonet walk then holds more
                                                              # graphs than positions and takes the generic body as a whole
                                                              ([4, 1], 500, 0.1, 1, 45), ([4, 1], 8, 0.0, 1, 45)])
def test_fused_backward_sweep_equals_unfused_chain(heads, hidden, drop, layers, empties, monkeypatch):
    """txe_gat_collapse_bwd_fused (d_X' formed on the fly inside the layer below's source-side sweep) against the unfused chain
    txe_gat_collapse_bwd -> txe_gat_aggregate_bwd of the SAME forward pass (same saved state, same dropout seeds): every gradient,
    on generic batched multigraphs (a hub with in-degree > 64 and a node with ~400 out-edges, nodes without in-edges, graphs of
    1..90 nodes) -- head layouts of 1 / 2 / 4 heads (one, two, four waves per head), row widths up to 2,400 columns"""
    from taxoexpan_amd import model_zoo as mz, ops
    from taxoexpan_amd.graph import DGLGraph, batch
    dev = _dev()
    rs = np.random.RandomState(3)
    graphs = []
    for n in [1, 2, 40, 7, 3, 90, 5, 33]:
        g = DGLGraph()
        g.add_nodes(n)
        if n > 1:
            e = 3 * n
            g.add_edges(rs.randint(0, n, e), rs.randint(1, n, e))            # node 0 of every graph: no in-edge but the self loop below
        if n == 90:
            g.add_edges(rs.randint(0, n, 100), np.full(100, 11))              # hub: in-degree > 64
            g.add_edges(np.full(400, 17), rs.randint(0, n, 400))              # 400 out-edges: past the LDS-staged edge scalars
        if n != 33:
            g.add_edges(g.nodes(), g.nodes())                                 # (the 33-node graph has nodes without any in-edge)
        graphs.append(g)
        if n == 7:
            graphs.extend(DGLGraph() for _ in range(empties))                 # (graphs without nodes, in the middle of the batch)
    bg = batch(graphs)
    N = bg.number_of_nodes()
    pos = torch.from_numpy(rs.randint(0, 3, N)).to(dev)
    x = torch.randn(N, 10, generator=torch.Generator().manual_seed(0)).to(dev)
    coef = torch.randn(len(graphs), 6, generator=torch.Generator().manual_seed(1)).to(dev)
    torch.manual_seed(5)
    prop = mz.PGAT(10, hidden, 6, 4, num_layers=layers, heads=heads, activation=F.leaky_relu, feat_drop=drop, attn_drop=drop).to(dev)
    ro = mz.WeightedMeanReadout().to(dev)
    prop.train(drop > 0)
    seed = 4242
    monkeypatch.setattr(ops, "new_seed", lambda: seed)
    results = []
    for fused in (True, False):
        monkeypatch.setattr(ops, "_NO_FUSED_BWD", not fused)
        for p in list(prop.parameters()) + list(ro.parameters()):
            p.grad = None
        xg = x.clone().requires_grad_(True)
        bg.ndata["pos"] = pos
        with ops.debug_capture() as runs:
            bg.ndata["h"] = prop(bg, xg)
            hg = ro(bg, pos)
            hg = hg.tensor() if isinstance(hg, mz.DeferredGraphVector) else hg     # (grad mode: the readout only describes its work)
        _csr, _cfg, states = runs[0]
        assert ops._fused_bwd_ok(_csr, states[-1], states[-2]) == (fused and heads[-2] in (1, 2, 4) and (heads[-2] * hidden) % 16 == 0)
        (hg * coef).sum().backward()
        results.append((hg.detach().cpu().numpy(), xg.grad.cpu().numpy(),
                        {k: p.grad.cpu().numpy() for k, p in list(prop.named_parameters()) + list(ro.named_parameters())}))
    (a, dxa, ga), (b, dxb, gb) = results
    np.testing.assert_array_equal(a, b)                                      # same forward
    errors = []
    _close(dxa, dxb, 2e-4, 2e-5, "d_x", errors)
    for k in ga:
        _close(ga[k], gb[k], 2e-4, 2e-5, "grad " + k, errors)
    assert not errors, "\n".join(errors)


# ================================================================================================================
# BASELINE configs[2]: the all-candidate inference loop AT ITS SIZE against the oracle (test_fast.py:99-140,149-218)
# ================================================================================================================
def _oracle_encode(P, features, ids, pos, node_off, heads=(4, 1), chunk=2048, select=None):
    """encode_graph (test_fast.py:25-28) of the egonets [node_off[g], node_off[g+1]) with the oracle, `chunk` egonets at a time.
    The egonet layout is dataset.py:404-437's: k grand-parents (pos 0), the anchor, m siblings (pos 2).  select: egonet indices."""
    sel = np.arange(len(node_off) - 1) if select is None else np.asarray(select)
    out = []
    with torch.no_grad():
        for c0 in range(0, len(sel), chunk):
            gs = sel[c0:c0 + chunk]
            rows = np.concatenate([np.arange(node_off[g], node_off[g + 1]) for g in gs])
            p = pos[rows]
            shapes = []
            for g in gs:
                pg = pos[node_off[g]:node_off[g + 1]]
                k, m = int((pg == 0).sum()), int((pg == 2).sum())
                assert k + 1 + m == len(pg) and pg[k] == 1
                shapes.append((k, m))
            graph = orc.batch_egonets(shapes)
            assert np.array_equal(graph["pos"].numpy(), p)
            hn = orc.pgat_forward(P, graph, features[torch.from_numpy(ids[rows]).long()], list(heads), 1, prefix="graph_propagate.")
            out.append(orc.weighted_mean_readout(graph["graph_off"], hn, graph["pos"], P["readout.position_weights.weight"]))
    return torch.cat(out)


def _rank_brackets(S_ref, pos_off, pos_idx, delta):
    """metric.py:7-31 on the oracle's scores with a relative band: [rank if every near-tie goes the positive's way, rank if none does]"""
    lo, hi = [], []
    for q in range(len(pos_off) - 1):
        p = pos_idx[pos_off[q]:pos_off[q + 1]]
        row = S_ref[q].astype(np.float64)
        neg = np.delete(row, p)
        for c in p:
            s = row[c]
            lo.append(1 + int((neg > s * (1 + delta)).sum()))
            hi.append(1 + int((neg > s * (1 - delta)).sum()))
    return np.asarray(lo), np.asarray(hi)


def test_mag_cs_inference_matches_oracle_at_full_size():
    """configs[2] on the MAG-CS shape: ALL 24,754 candidate egonets through the eval route the scripts take here (device-built egonets
    whose features stay rows of the taxonomy table -> table projection once -> rows formed inside the sweep -> folded output layer)
    against the oracle's encode_graph on the same egonets (every graph vector, 1e-4); then the whole 2,450 x 24,754 score matrix
    (factored GEMM + fused exp) against the oracle's scores at 1e-4, and the ranks of every true parent, three ways:
    (a) materialised = fused = metric.py:7-31 evaluated on the device scores, integer for integer;
    (b) END TO END with the model as initialised (random weights: a query's 24 k LBM scores lie within ~1e-2 of each other, ~1e-6
        apart, and the two encoders differ by ~1e-6): every rank inside the band the oracle's scores leave when gaps below 2.5x the
        MEASURED score error may fall either way -- a band, because an exact-rank assert would test noise there;
    (c) the SCORING LOOP + RANKING PINNED: same graph vectors on both sides (the oracle's, uploaded) and the matcher's weight scaled so
        that a query's log-scores spread over several units (std 2; what a trained matcher looks like) -- against metric.py:7-31 on the
        oracle's float64 scores: >= 99 % of the ranks EXACT, every other one inside the 2.5-eps band, materialised and fused alike."""
    from taxoexpan_amd import TaxoExpan, graph as G, ops, synthetic as syn
    from taxoexpan_amd.evaluate import candidate_graphs
    from taxoexpan_amd.scoring import encode_candidates, rank_all_fused, score_all
    import bench
    dev = _dev()
    tax = syn.make_named_taxonomy("mag_cs", seed=47)
    cand, _val, test = syn.split_candidates(tax)
    assert len(cand) > 24000 and len(test) > 2400
    torch.manual_seed(47)
    model = TaxoExpan("PGAT", "WMR", "LBM", **dict(MAG, num_layers=1, heads=[4, 1])).to(dev).eval()
    dtax = G.DeviceTaxonomy(tax.par_ptr, tax.par_idx, tax.chd_ptr, tax.chd_idx, tax.features, dev)
    g = candidate_graphs(dtax, cand, 50, 7)
    hg = encode_candidates(model, g)
    ids, pos = g.ndata["_id"].cpu().numpy(), g.ndata["pos"].cpu().numpy()
    node_off = g.csr(dev).graph_off.cpu().numpy()
    assert len(node_off) == len(cand) + 1 and node_off[-1] == len(ids) > 80000
    P = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    hg_ref = _oracle_encode(P, tax.features, ids, pos, node_off)
    errors = []
    _close(hg.cpu().numpy(), hg_ref.numpy(), 1e-4, 2e-5, "hg (all MAG-CS candidates)", errors)
    assert not errors, errors
    queries = tax.features[torch.from_numpy(test)]
    S = score_all(model.match, hg, queries.to(dev))
    S_ref = torch.exp(queries @ (hg_ref @ P["match.W.weight"][0]).t()).numpy()          # the factored form of test_fast.py:121-123
    assert S.shape == S_ref.shape == (len(test), len(cand))
    np.testing.assert_allclose(S.cpu().numpy(), S_ref, rtol=1e-4, atol=1e-30)
    pos_off, pos_idx = bench._positives(tax, cand, test)
    Sg = S.cpu().numpy()
    eps = float(np.max(np.abs(Sg.astype(np.float64) - S_ref) / S_ref))                   # measured, <= 1e-4 by the assert above
    off_t, idx_t = torch.tensor(pos_off, dtype=torch.int32), torch.tensor(pos_idx, dtype=torch.int32)
    r_mat = ops.rank_block(S, off_t, idx_t, True).cpu().numpy()
    r_fused = rank_all_fused(model.match, hg, queries.to(dev), pos_off, pos_idx).cpu().numpy()
    assert np.array_equal(r_mat, r_fused)
    # (a) metric.py:7-31 evaluated on the DEVICE scores is exactly what both device paths return
    lo0, hi0 = _rank_brackets(Sg, pos_off, pos_idx, 0.0)
    assert np.array_equal(lo0, hi0) and np.array_equal(r_mat, lo0)
    # (b) against the ORACLE's scores: scores that agree to eps relative can only reorder pairs closer than 2 eps, so every rank lies in
    # the band the oracle's scores leave when gaps below 2.5 eps may fall either way.  (With random weights the 24,736 LBM scores of
    # a query sit within a few 1e-2 of each other -- spacing ~1e-6 relative -- so only part of the ranks is pinned to one value.)
    lo, hi = _rank_brackets(S_ref, pos_off, pos_idx, 2.5 * eps)
    assert ((r_mat >= lo) & (r_mat <= hi)).all(), np.nonzero((r_mat < lo) | (r_mat > hi))[0][:10]
    width = (hi - lo).astype(np.float64)
    assert np.median(width) <= 8 and width.max() <= 0.01 * len(cand), (np.median(width), width.max(), eps)
    lo_x, hi_x = _rank_brackets(S_ref, pos_off, pos_idx, 0.0)                            # the oracle's own ranks
    assert np.abs(r_mat - lo_x).max() <= width.max() and np.corrcoef(r_mat, lo_x)[0, 1] > 0.999999
    # (c) scoring + ranking alone, pinned to exact ranks (model/metric.py:7-31, test_fast.py:116-140)
    W64 = P["match.W.weight"][0].double()
    Z = queries.double() @ (hg_ref.double() @ W64).t()                                   # log-scores, float64
    scale = 2.0 / float(Z.std())
    with torch.no_grad():
        model.match.W.weight.mul_(scale)
    S64 = torch.exp(Z * scale).numpy()
    hg_same = hg_ref.to(dev)
    S2 = score_all(model.match, hg_same, queries.to(dev))
    S2h = S2.cpu().numpy()
    eps2 = float(np.max(np.abs(S2h.astype(np.float64) - S64) / S64))
    assert eps2 <= 1e-4, eps2
    assert float(np.log(S64.max() / S64.min())) > 10.0                                   # the scores DO spread now
    r2 = ops.rank_block(S2, off_t, idx_t, True).cpu().numpy()
    r2f = rank_all_fused(model.match, hg_same, queries.to(dev), pos_off, pos_idx).cpu().numpy()
    assert np.array_equal(r2, r2f)
    want, _ = _rank_brackets(S64, pos_off, pos_idx, 0.0)                                 # metric.py:7-31 on the float64 scores
    exact = float((r2 == want).mean())
    lo2, hi2 = _rank_brackets(S64, pos_off, pos_idx, 2.5 * eps2)
    assert exact >= 0.99, (exact, eps2)
    assert ((r2 >= lo2) & (r2 <= hi2)).all(), np.nonzero((r2 < lo2) | (r2 > hi2))[0][:10]


def test_mag_full_30000_chunk_matches_oracle():
    """configs[2]'s `-b 30000` on the MAG-Full shape: the first chunk of 30,000 candidate egonets (431,416-row feature table projected
    once, rows formed in the sweep) against the oracle on a strided sample of 5,000 of them (every 6th egonet, graph vectors at 1e-4),
    and their scores against 512 test queries"""
    from taxoexpan_amd import TaxoExpan, graph as G, synthetic as syn
    from taxoexpan_amd.scoring import encode_candidates, score_all
    dev = _dev()
    tax = syn.make_named_taxonomy("mag_full", seed=47)
    cand, _val, test = syn.split_candidates(tax)
    torch.manual_seed(47)
    model = TaxoExpan("PGAT", "WMR", "LBM", **dict(MAG, num_layers=1, heads=[4, 1])).to(dev).eval()
    dtax = G.DeviceTaxonomy(tax.par_ptr, tax.par_idx, tax.chd_ptr, tax.chd_idx, tax.features, dev)
    g = G.device_egonet_batch(dtax, cand[:30000], expand_factor=50, seed=7, with_features="lazy", index_base=0)
    hg = encode_candidates(model, g)
    assert hg.shape == (30000, 500)
    ids, pos = g.ndata["_id"].cpu().numpy(), g.ndata["pos"].cpu().numpy()
    node_off = g.csr(dev).graph_off.cpu().numpy()
    sel = np.arange(0, 30000, 6)
    P = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    hg_ref = _oracle_encode(P, tax.features, ids, pos, node_off, select=sel)
    errors = []
    _close(hg.cpu().numpy()[sel], hg_ref.numpy(), 1e-4, 2e-5, "hg (MAG-Full chunk, strided sample)", errors)
    assert not errors, errors
    queries = tax.features[torch.from_numpy(test[:512])]
    S = score_all(model.match, hg, queries.to(dev)).cpu().numpy()[:, sel]
    S_ref = torch.exp(queries @ (hg_ref @ P["match.W.weight"][0]).t()).numpy()
    np.testing.assert_allclose(S, S_ref, rtol=1e-4, atol=1e-30)
