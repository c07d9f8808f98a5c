"""Reference of the attention readout (taxoexpan_amd.model_zoo.AttentionReadout) for the tests: the defining expression in torch on the
CPU, one torch.softmax per egonet in a Python loop, gradients from autograd, any dtype.  Written from the definition alone -- it shares
no code with model_zoo.host_attention_readout or the kernels.

    Y[v]     = W h[v] + b
    s[v]     = sum_j u[j] tanh(Y[v][j] + P[pos[v]][j])
    alpha    = softmax of s over each egonet
    hg[g]    = sum_{v in g} alpha[v] h[v]          (an egonet without nodes: a zero row)
"""
import torch


def attention_pool(graph_off, h, Y, pos, P, u):
    """(hg [G, D], alpha [N]) from the node states h [N, D] and the gate's pre-activations Y [N, A] (the operator's own inputs)"""
    s = torch.tanh(Y + P[pos.long()]) @ u.reshape(-1)
    rows, alphas = [], []
    for beg, end in zip(graph_off[:-1].tolist(), graph_off[1:].tolist()):
        if end == beg:
            rows.append(h.new_zeros(h.shape[1]))
            continue
        a = torch.softmax(s[beg:end], dim=0)
        alphas.append(a)
        rows.append(a @ h[beg:end])
    alpha = torch.cat(alphas) if alphas else s.new_zeros(0)
    return torch.stack(rows) if rows else h.new_zeros((0, h.shape[1])), alpha


def attention_readout(graph_off, h, pos, W, b, P, u):
    """the whole module: gate_hidden (W [A, D], b [A]), gate_position (P [vocab, A]), gate_out (u [1, A] or [A])"""
    return attention_pool(graph_off, h, h @ W.t() + b, pos, P, u)


def run(fn, dtype, arrays, weights):
    """fn(*tensors) -> tuple of outputs, in `dtype` on the CPU; backward of sum_k <out_k, weights_k> (None: that output is left out).
    Returns ([outputs as numpy], [gradient of every array as numpy])"""
    ts = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in arrays]
    outs = fn(*ts)
    total = sum((o * torch.from_numpy(w).to(dtype)).sum() for o, w in zip(outs, weights) if w is not None)
    total.backward()
    return [o.detach().numpy() for o in outs], [t.grad.numpy() for t in ts]
