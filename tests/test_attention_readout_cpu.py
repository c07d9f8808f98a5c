"""CPU: the attention readout's numpy restatement (model_zoo.host_attention_readout) against the torch reference of
tests/attention_readout_ref.py, the reference's own gradients (gradcheck), two identities that tie both to the reference-pinned oracle
(a gate that sees positions only IS a weighted mean readout; a gate that sees nothing IS the mean readout), the model assembly with the
"AR" string beside the unchanged MR / WMR / CR assemblies, and the argument checks of the two C entry points (no GPU needed: they return
before any device work)."""
import ctypes

import numpy as np
import torch

import attention_readout_ref as ref
import txe_oracle as orc

# the batch of tests/test_gpu_readout_match_ops.py: node counts 1..5, 63..68, 127..129, 200; every position class empty somewhere; G = 71
EGONETS = [(0, 0), (0, 1), (2, 0), (1, 2), (2, 2), (20, 42), (3, 60), (0, 64), (30, 35), (66, 0), (7, 60), (40, 86), (64, 63), (1, 127),
           (99, 100)]
SHAPES = (EGONETS * 5)[:71]
D, A = 24, 10


def _inputs(seed=3, shapes=SHAPES, d=D, a=A):
    graph = orc.batch_egonets(shapes)
    rs = np.random.RandomState(seed)
    n = graph["num_nodes"]
    params = {"gate_hidden.weight": rs.standard_normal((a, d)) / np.sqrt(d), "gate_hidden.bias": rs.standard_normal(a) * 0.1,
              "gate_position.weight": rs.standard_normal((3, a)), "gate_out.weight": rs.standard_normal((1, a))}
    return graph, rs.standard_normal((n, d)), params


def _reference(graph, h, params, dtype=torch.float64):
    t = lambda k: torch.from_numpy(np.asarray(params[k])).to(dtype)
    hg, alpha = ref.attention_readout(graph["graph_off"], torch.from_numpy(h).to(dtype), graph["pos"], t("gate_hidden.weight"),
                                      t("gate_hidden.bias"), t("gate_position.weight"), t("gate_out.weight"))
    return hg.numpy(), alpha.numpy()


def test_host_restatement_equals_the_float64_reference():
    from taxoexpan_amd.model_zoo import host_attention_readout
    graph, h, params = _inputs()
    hg, alpha = host_attention_readout(params, graph["graph_off"].numpy(), h, graph["pos"].numpy())
    want_hg, want_alpha = _reference(graph, h, params)
    assert hg.dtype == alpha.dtype == np.float64 and hg.shape == (71, D) and alpha.shape == (graph["num_nodes"],)
    assert np.abs(hg - want_hg).max() <= 1e-12 and np.abs(alpha - want_alpha).max() <= 1e-12
    sums = np.add.reduceat(alpha, graph["graph_off"].numpy()[:-1])
    assert np.abs(sums - 1.0).max() <= 1e-12                                   # a softmax per egonet
    hg32, alpha32 = host_attention_readout(params, graph["graph_off"].numpy(), h, graph["pos"].numpy(), dtype=np.float32)
    assert hg32.dtype == alpha32.dtype == np.float32 and np.abs(hg32 - want_hg).max() <= 1e-4


def test_host_restatement_gives_an_empty_egonet_a_zero_row():
    from taxoexpan_amd.model_zoo import host_attention_readout
    graph, h, params = _inputs(shapes=[(1, 2), (0, 0)], seed=4)
    goff = np.array([0, 4, 4, 5])                                              # the middle segment holds no node
    hg, alpha = host_attention_readout(params, goff, h, graph["pos"].numpy())
    t = lambda k: torch.from_numpy(np.asarray(params[k]))
    want, want_alpha = ref.attention_readout(torch.from_numpy(goff), torch.from_numpy(h), graph["pos"], t("gate_hidden.weight"),
                                             t("gate_hidden.bias"), t("gate_position.weight"), t("gate_out.weight"))
    assert not hg[1].any() and not want[1].any()
    assert np.abs(hg - want.numpy()).max() <= 1e-12 and np.abs(alpha - want_alpha.numpy()).max() <= 1e-12 and alpha[4] == 1.0


def test_reference_gradients_pass_gradcheck():
    graph = orc.batch_egonets([(0, 0), (1, 2), (2, 3)])
    rs = np.random.RandomState(8)
    n, d, a = graph["num_nodes"], 5, 4
    ts = [torch.from_numpy(x).requires_grad_(True) for x in (rs.standard_normal((n, d)), rs.standard_normal((a, d)) * 0.5, rs.standard_normal(a) * 0.1,
                                                             rs.standard_normal((3, a)), rs.standard_normal((1, a)))]
    fn = lambda h, W, b, P, u: ref.attention_readout(graph["graph_off"], h, graph["pos"], W, b, P, u)[0]
    assert torch.autograd.gradcheck(fn, ts)
    Y = torch.from_numpy(rs.standard_normal((n, a))).requires_grad_(True)          # the operator's own inputs: h and Y independent
    op = lambda h, Y_, P, u: ref.attention_pool(graph["graph_off"], h, Y_, graph["pos"], P, u)[0]
    assert torch.autograd.gradcheck(op, (ts[0], Y, ts[3], ts[4]))


def test_position_only_gate_is_the_weighted_mean_readout():
    """gate_hidden zero: s_v = <u, tanh(P[pos_v])> = s_c depends on the class alone, alpha_v = exp(s_c) / sum exp(s_c'), which is
    WeightedMeanReadout with softplus(pw[c]) = exp(s_c), i.e. pw[c] = log(expm1(exp(s_c)))"""
    from taxoexpan_amd.model_zoo import host_attention_readout
    graph, h, params = _inputs(seed=5)
    params["gate_hidden.weight"] = np.zeros((A, D))
    params["gate_hidden.bias"] = np.zeros(A)
    s_c = np.tanh(params["gate_position.weight"]) @ params["gate_out.weight"].reshape(-1)
    pw = torch.from_numpy(np.log(np.expm1(np.exp(s_c)))).reshape(3, 1)
    want = orc.weighted_mean_readout(graph["graph_off"], torch.from_numpy(h), graph["pos"], pw).numpy()
    assert np.abs(_reference(graph, h, params)[0] - want).max() <= 1e-12
    assert np.abs(host_attention_readout(params, graph["graph_off"].numpy(), h, graph["pos"].numpy())[0] - want).max() <= 1e-12


def test_blind_gate_is_the_mean_readout():
    from taxoexpan_amd.model_zoo import host_attention_readout
    graph, h, params = _inputs(seed=6)
    params["gate_hidden.weight"] = np.zeros((A, D))
    params["gate_hidden.bias"] = np.zeros(A)
    params["gate_out.weight"] = np.zeros((1, A))
    want = orc.mean_readout(graph["graph_off"], torch.from_numpy(h)).numpy()
    assert np.abs(_reference(graph, h, params)[0] - want).max() <= 1e-12
    assert np.abs(host_attention_readout(params, graph["graph_off"].numpy(), h, graph["pos"].numpy())[0] - want).max() <= 1e-12


OPTS = dict(in_dim=12, hidden_dim=8, out_dim=7, pos_dim=5, num_layers=1, heads=[4, 1], feat_drop=0.1, attn_drop=0.1, hidden_drop=0.1,
            out_drop=0.1)
PGAT_KEYS = {"graph_propagate.gat_layers.0.attn_l": (1, 4, 8), "graph_propagate.gat_layers.0.attn_r": (1, 4, 8),
             "graph_propagate.gat_layers.0.fc.weight": (32, 17), "graph_propagate.gat_layers.1.attn_l": (1, 1, 7),
             "graph_propagate.gat_layers.1.attn_r": (1, 1, 7), "graph_propagate.gat_layers.1.fc.weight": (7, 37),
             "graph_propagate.prop_position_embeddings.0.weight": (3, 5), "graph_propagate.prop_position_embeddings.1.weight": (3, 5)}


def _shapes(model):
    return {k: tuple(v.shape) for k, v in model.state_dict().items()}


def test_attention_readout_model_builds_on_the_cpu():
    from taxoexpan_amd import TaxoExpan, model_zoo
    m = TaxoExpan("PGAT", "AR", "BIM", attention_dim=9, **OPTS)
    assert isinstance(m.readout, model_zoo.AttentionReadout)
    assert _shapes(m) == dict(PGAT_KEYS, **{"readout.gate_hidden.weight": (9, 7), "readout.gate_hidden.bias": (9,),
                                            "readout.gate_position.weight": (3, 9), "readout.gate_out.weight": (1, 9),
                                            "match.W.weight": (1, 7, 12)})
    assert m.match.W.in1_features == 7                                          # the matcher's graph side is out_dim wide
    d = TaxoExpan("PGCN", "AR", "MLP", **OPTS)                                  # no attention_dim: 100
    assert tuple(d.readout.gate_hidden.weight.shape) == (100, 7) and tuple(d.readout.gate_out.weight.shape) == (1, 100)
    assert tuple(d.match.ffn[0].weight.shape) == (8, 7 + 12)
    alone = model_zoo.AttentionReadout(6)
    assert sorted(alone.state_dict()) == ["gate_hidden.bias", "gate_hidden.weight", "gate_out.weight", "gate_position.weight"]
    assert tuple(alone.gate_hidden.weight.shape) == (100, 6) and tuple(alone.gate_position.weight.shape) == (3, 100)


def test_the_three_existing_readout_strings_build_what_they_built():
    from taxoexpan_amd import TaxoExpan, model_zoo
    mr, wmr, cr = (TaxoExpan("PGAT", r, "BIM", **OPTS) for r in ("MR", "WMR", "CR"))
    assert type(mr.readout) is model_zoo.MeanReadout and type(wmr.readout) is model_zoo.WeightedMeanReadout
    assert type(cr.readout) is model_zoo.ConcatReadout
    assert _shapes(mr) == dict(PGAT_KEYS, **{"match.W.weight": (1, 7, 12)})
    assert _shapes(wmr) == dict(PGAT_KEYS, **{"readout.position_weights.weight": (3, 1), "match.W.weight": (1, 7, 12)})
    assert _shapes(cr) == dict(PGAT_KEYS, **{"match.W.weight": (1, 21, 12)})
    assert list(wmr.state_dict())[-2:] == ["readout.position_weights.weight", "match.W.weight"]
    unknown = TaxoExpan("PGAT", "nope", "BIM", **OPTS)                          # a string in no table leaves the attributes unset
    assert not hasattr(unknown, "readout") and not hasattr(unknown, "match")


def test_entry_points_check_their_arguments_before_any_device_work():
    from taxoexpan_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)                                                   # host memory: never read by a call that is refused
    G, Dm, Am, V = 2, 8, 4, 3
    fwd = dict(graph_off=a, G=G, h=a, ld_h=Dm, D=Dm, Y=a, ld_y=Am, A=Am, pos=a, P=a, vocab=V, u=a, hg=a, alpha=a, stream=None)
    bwd = dict(graph_off=a, G=G, h=a, ld_h=Dm, D=Dm, Y=a, ld_y=Am, A=Am, pos=a, P=a, vocab=V, u=a, hg=a, alpha=a, d_hg=a, ld_dhg=Dm,
               d_h=a, ld_dh=Dm, d_Y=a, ld_dy=Am, d_P=a, d_u=a, ws=a, ws_bytes=0, stream=None)
    need = lib.txe_readout_attn_bwd_ws_bytes(G, Am, V)
    assert need == G * (V + 1) * Am * 4 and lib.txe_readout_attn_bwd_ws_bytes(0, Am, V) == 0
    bad = [("A", 0), ("D", 0), ("vocab", 0), ("vocab", 9), ("G", -1)]
    for name, args, fn in (("fwd", fwd, lib.txe_readout_attn_fwd), ("bwd", bwd, lib.txe_readout_attn_bwd)):
        pointers = [k for k, v in args.items() if v == a and k != "ws"]
        assert len(pointers) == (8 if name == "fwd" else 13)
        for k in pointers:                                                      # every required pointer, NULL in turn
            assert fn(*dict(args, **{k: None}).values()) == -1, (name, k)
        for k, v in bad:
            assert fn(*dict(args, **{k: v}).values()) == -1, (name, k, v)
        assert fn(*dict(args, G=0).values()) == 0, name                         # nothing to do: TXE_OK, nothing launched
    assert lib.txe_readout_attn_bwd(*bwd.values()) == -3                        # no workspace at all
    assert lib.txe_readout_attn_bwd(*dict(bwd, ws_bytes=need - 1).values()) == -3
    assert lib.txe_readout_attn_bwd(*dict(bwd, ws=None, ws_bytes=need).values()) == -1
