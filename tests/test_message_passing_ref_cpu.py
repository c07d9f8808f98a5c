"""The float64 references of tests/test_gpu_message_passing_ops.py (tests/message_passing_ref.py) against the oracle's own layers, which
the reference goldens pin: the GAT sweep against orc.gat_layer(..., return_parts=True), the GCN sweep against orc.gcn_layer, in float64
on the two graphs of that file, to 1e-12 of the tensor's largest entry.  Also: what the graphs promise."""
import numpy as np
import pytest
import torch

import message_passing_ref as mp
import txe_oracle as orc


def _graphs():
    s1, d1 = mp.generic_multigraph()
    s2, d2, n2 = mp.egonet_batch()
    return {"multigraph": (s1, d1, mp.G1_N), "egonets": (s2, d2, n2)}


def _close(got, want, what):
    got, want = got.detach().numpy(), want.detach().numpy()
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), what


@pytest.mark.parametrize("gname", ["multigraph", "egonets"])
@pytest.mark.parametrize("attn_p", [0.0, 0.3])
def test_gat_sweep_reference_is_the_oracle_layers_message_passing(gname, attn_p):
    src, dst, n = _graphs()[gname]
    H, D, K = 3, 5, 7
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.standard_normal((n, K)))
    W, al, ar = (torch.from_numpy(rs.standard_normal(s)) for s in ((H * D, K), (1, H, D), (1, H, D)))
    keep = torch.from_numpy((rs.random_sample((len(src), H, 1)) >= attn_p).astype(np.float64)) if attn_p else None
    s, d = torch.from_numpy(src), torch.from_numpy(dst)
    want, parts = orc.gat_layer(s, d, n, x, W, al, ar, 0.2, attn_keep=keep, attn_scale=1.0 / (1.0 - attn_p), return_parts=True)
    out, alpha = mp.gat_sweep(s, d, n, parts["ft"], parts["a1"].squeeze(-1), parts["a2"].squeeze(-1), 0.2,
                              keep.squeeze(-1) if attn_p else None, 1.0 / (1.0 - attn_p))
    assert out.dtype == torch.float64
    _close(out, want, "out")
    _close(alpha, parts["alpha"].squeeze(-1), "alpha")
    # the same edges in destination-CSR order (what the kernels see): the same rows, alpha permuted
    order = np.argsort(dst, kind="stable")
    sc, dc = mp.in_csr_order(src, dst)
    out_c, alpha_c = mp.gat_sweep(torch.from_numpy(sc), torch.from_numpy(dc), n, parts["ft"], parts["a1"].squeeze(-1), parts["a2"].squeeze(-1),
                                  0.2, keep.squeeze(-1)[order] if attn_p else None, 1.0 / (1.0 - attn_p))
    _close(out_c, want, "out, CSR order")
    _close(alpha_c, parts["alpha"].squeeze(-1)[order], "alpha, CSR order")
    act, _ = mp.gat_sweep(s, d, n, parts["ft"], parts["a1"].squeeze(-1), parts["a2"].squeeze(-1), 0.2, None, 1.0, act_slope=0.01)
    plain, _ = mp.gat_sweep(s, d, n, parts["ft"], parts["a1"].squeeze(-1), parts["a2"].squeeze(-1), 0.2)
    _close(act, torch.nn.functional.leaky_relu(plain, 0.01), "activation")


@pytest.mark.parametrize("gname", ["multigraph", "egonets"])
@pytest.mark.parametrize("bias,act", [(True, 0.01), (False, None), (True, None)])
def test_gcn_sweep_reference_is_the_oracle_layers_message_passing(gname, bias, act):
    src, dst, n = _graphs()[gname]
    K, Fo = 7, 6
    rs = np.random.RandomState(6)
    x, W = torch.from_numpy(rs.standard_normal((n, K))), torch.from_numpy(rs.standard_normal((K, Fo)))
    b = torch.from_numpy(rs.standard_normal(Fo)) if bias else None
    s, d = torch.from_numpy(src), torch.from_numpy(dst)
    want = orc.gcn_layer(s, d, n, x, W, b, orc.gcn_norm(d, n, torch.float64), act_slope=act)
    got = mp.gcn_sweep(s, d, n, x @ W, b, act)
    assert got.dtype == torch.float64
    _close(got, want, "out")


def test_next_logits_and_head_mean_references():
    rs = np.random.RandomState(8)
    x, wa = torch.from_numpy(rs.standard_normal((9, 64))), torch.from_numpy(rs.standard_normal((2, 64)))
    keep = torch.from_numpy((rs.random_sample((9, 64)) >= 0.5).astype(np.float64))
    want = torch.stack([(torch.nn.functional.dropout(x, 0.0) * keep * 2.0 * wa[r]).sum(1) for r in range(2)], 1)
    _close(mp.next_logits(x, keep, 2.0, wa), want, "a12")
    _close(mp.next_logits(x, None, 1.0, wa), x @ wa.t(), "a12, no mask")
    y = torch.from_numpy(rs.standard_normal((5, 3, 4)))
    _close(mp.head_mean(y), (y[:, 0] + y[:, 1] + y[:, 2]) / 3.0, "head mean")


def test_the_two_graphs_hold_what_the_gpu_cases_rely_on():
    src, dst = mp.generic_multigraph()
    n = mp.G1_N
    assert n % 4 and n % 8 and len(src) <= 3000
    indeg, outdeg = np.bincount(dst, minlength=n), np.bincount(src, minlength=n)
    assert {0, 1, 2, 63, 64, 65, 128, 129, 200} <= set(indeg.tolist())
    assert {0, 1, 16, 17, 64, 65, 200} <= set(outdeg.tolist())
    assert indeg[n - 1] == 200 and indeg[mp.G1_LONE] == 0 and outdeg[mp.G1_LONE] == 0
    assert (src == dst).any() and len(set(zip(src.tolist(), dst.tolist()))) < len(src)
    # the widened logits: every G1_WIDE destination has in-edges from sources of both signs, and its logits span more than 180
    a_src = mp.widen_logits(np.random.RandomState(0).standard_normal((n, 4)).astype(np.float32))
    a_dst = np.random.RandomState(1).standard_normal((n, 4)).astype(np.float32)
    e = orc._leaky(torch.from_numpy(a_src[src] + a_dst[dst]), 0.2).numpy()
    for v in mp.G1_WIDE:
        ev = e[dst == v]
        assert (ev.max(0) - ev.min(0)).min() > 180.0, v
        with np.errstate(over="ignore"):
            assert np.exp(ev.astype(np.float32)).max() == np.inf        # (what a softmax without the running maximum would do in fp32)
    s2, d2, n2 = mp.egonet_batch()
    assert n2 == sum(k + 1 + m for k, m in mp.EGONETS) == 992 and len(s2) == 2 * n2 - len(mp.EGONETS)
    assert np.bincount(d2, minlength=n2).max() == 100 and np.bincount(s2, minlength=n2).max() == 128      # (both past one 64-edge chunk)
