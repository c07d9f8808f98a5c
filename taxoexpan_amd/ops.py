"""torch.autograd bindings of the libtxe kernels (include/txe.h).

torch is plumbing here: it owns device memory (caching allocator), the current HIP stream and autograd's tape;
every number is produced by the hand-written HIP kernels.  There is no CPU path -- host tensors raise.
"""
import collections
import ctypes
import functools
import math
import typing
import weakref

import torch

from . import _lib
from ._lib import call, ptr, pure

LEAKY_SLOPE = 0.01  # F.leaky_relu default, the only activation model.py:25-41 passes


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("taxoexpan_amd: tensors must live on the MI355X (no CPU fallback exists); "
                               "got a host tensor")


def _f32(t):
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _rows(t):
    """2-D fp32 tensor with unit column stride; returns (tensor, ld)."""
    if t.dtype != torch.float32:
        t = t.float()
    if t.dim() != 2 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t, t.stride(0)


_BACKWARD_TWICE = ("taxoexpan_amd: backward through this propagation stack a second time -- its saved activations (several hundred MB per "
                   "batch) are released by the first backward; run the forward again (retain_graph=True is not supported here)")
# Alternative routes to the same numbers, kept because a parity test compares each with the default one.  Plain module attributes: tests
# monkeypatch them, tests/conftest.py's TXE_TEST_ROUTE sets one for a whole run.  (The library itself reads no environment variable.)
_NO_FUSED_LOGITS = False    # the folded layer's attention logits by their own sweep instead of the aggregation's epilogue
_NO_TABLE_SWEEP = False     # table rows materialised (txe_gather_add_rows) instead of formed inside the sweep
_NO_SIDE_STREAM = False     # everything on the caller's stream
_NO_MATCH_FOLD = False      # the graph vector hg = Z W^T is always formed (never folded into the bilinear matcher's run products)
_NO_FOLD_EDOT = False       # the folded matcher's T does not ride in the Z sweep: backward runs its <dZ, X> sweep
_NO_FUSED_BWD = False       # the folded layer's backward as the unfused chain (d_X' materialised)
_NO_QUERY_RUNS = False      # stacked query rows always take the GEMM form of the bilinear match
_NO_SPLIT_GEMM = False      # the first layer's projection on the fp32 MFMA instead of the bf16 pipe's six plane products
_NO_TAIL_CHAIN = False      # every layer's last reduction launch in place instead of chained into the bottom layer's
_FWD_SWEEP = 0              # txe_gat_aggregate_fwd's npw argument (0 = chosen from the batch; tools/kt_quick.py sets others)
_NO_VIRTUAL_X = False       # a first layer's input X = dropout([h | Emb[pos]]) is written by the preparation launch and read back by the packs
_NO_WALK_PLAN = False       # the egonet-walking backward sweep works the graphs' shapes out of the CSR arrays in every workgroup (no per-batch plan)
_NO_EGO_WALK = False        # the forward sweep runs one wave per node and the fused backward sweep fetches X'[v] per out-edge, instead of walking egonets
_NO_REFORM_X = False        # the egonet-walking backward sweep loads the X' rows of parents and siblings instead of forming them again from Y
_I32_MEMO = {}       # id(source tensor) -> (weakref, version, device, int32 copy): `pos` is converted once per batch, not once per module


def _i32(t, device):
    if t is None:
        return None
    if t.dtype == torch.int32 and t.device == device:
        return t.contiguous()
    key = id(t)
    hit = _I32_MEMO.get(key)
    if hit is not None and hit[0]() is t and hit[1] == t._version and hit[2] == device:
        return hit[3]
    out = t.to(device=device, dtype=torch.int32).contiguous()
    if len(_I32_MEMO) > 64:
        for k in [k for k, v in _I32_MEMO.items() if v[0]() is None]:
            del _I32_MEMO[k]
        if len(_I32_MEMO) > 64:
            _I32_MEMO.clear()
    _I32_MEMO[key] = (weakref.ref(t), t._version, device, out)
    return out


def _empty(shape, ref, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=ref.device)


def _ws(nbytes, ref):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=ref.device)


def new_seed():
    """64-bit dropout seed drawn from torch's CPU generator (so torch.manual_seed makes runs repeatable)."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


ROUTES = {}           # kind -> the route the LAST call of that kind took ('match': _Bilinear.forward; 'stack' / 'stack_bwd': the propagation
                      # stack's cfg.final (+ '+edot') and its backward; 'fold': the folded matcher's forward) -- tests assert on it, bench.py
                      # reports it; debug_capture() additionally collects every note of its block in `routes`


def note_route(kind, name):
    ROUTES[kind] = name
    if _CAPTURE is not None:
        _CAPTURE.routes.append((kind, name))


_GRAD_READY = None    # scoring.overlapped_gradient_allreduce: called as (layer index, [parameter gradients]) the moment a layer's are done
_GRAD_FLUSH = None    # ... and once before the stack returns its gradients to autograd
_CAPTURE = None       # debug_capture(): list that receives (csr, cfg, per-layer states) of every stack forward


class _CaptureList(list):
    """debug_capture()'s list of stack forwards, plus `.routes`: every (kind, route) noted inside the block, in order"""

    def __init__(self):
        super().__init__()
        self.routes = []


class debug_capture:
    """`with ops.debug_capture() as runs:` -- every GAT / GCN stack forward inside the block appends (csr, cfg, states): the per-layer
    buffers of the fused stack (X = padded layer input, None where it is never stored: layer 0 on the table route or with st.vx;
    Y = projection output, alpha [E, H] in destination-CSR order, cl = the folded output layer's GatFolded / GcnFolded: cl.Z,
    cl.alpha, ...).  Parity tests read the intermediates the reference exposes per layer (model_zoo.py:90-95) from here;
    nothing is copied and nothing changes in the computation."""

    def __enter__(self):
        global _CAPTURE
        self._prev, _CAPTURE = _CAPTURE, _CaptureList()
        return _CAPTURE

    def __exit__(self, *exc):
        global _CAPTURE
        _CAPTURE = self._prev
        return False


def apply_stack(fn, csr, cfg, *args):
    """fn.apply with the caller's grad mode recorded in cfg: inside Function.forward grad mode is always off and needs_input_grad
    only mirrors requires_grad, so this is how a no_grad pass (evaluation) avoids keeping the backward state -- and may take the
    table-projection path of GatheredRows."""
    cfg.grad_enabled = torch.is_grad_enabled()
    return fn.apply(csr, cfg, *args)


# ---- the frame GATStackFunction and GCNStackFunction share around their layer loops -----------------------------------------------------
def _stack_begin(ctx, csr, cfg, h, pos, rpos, pw, params, feat_p):
    """A stack forward's inputs, normalised: (need, z_only, collapse, table, src, ld_h, ref, N, kh, pos).
    need: keep the backward state (see apply_stack); collapse: the output layer is folded behind the readout, z_only: and stops at Z;
    table: layer 0 projects src.table and gathers (GatheredRows), otherwise src [N, kh] with row pitch ld_h holds the
    features; ref: the allocation reference (src, or the table).  What backward needs of the inputs goes on ctx here: csr, cfg, h_req,
    link, and -- only for a folded layer with position weights -- rpos, pwf (pw flat, fp32), pw_shape."""
    need = cfg.grad_enabled and any(ctx.needs_input_grad)
    z_only = (cfg.final == "collapse_z")        # 'collapse' that stops at Z: the Function returns (Z [G, Kp], the output layer's packed weights)
    collapse = (cfg.final == "collapse") or z_only
    table = _use_table(h, need, feat_p) and not (collapse and cfg.n_layers == 1)
    if isinstance(h, GatheredRows) and not table:
        h = h.tensor()
    if table:
        _need_cuda(h.table, *[p for p in params if p is not None])
        src, ld_h, ref, N = h, 0, h.table, h.index.shape[0]
    else:
        _need_cuda(h, *[p for p in params if p is not None])
        src, ld_h = _rows(h)
        ref, N = src, src.shape[0]
    weighted = collapse and pw is not None
    ctx.csr, ctx.cfg, ctx.h_req, ctx.link = csr, cfg, ctx.needs_input_grad[2], (cfg.link if z_only else None)
    ctx.rpos, ctx.pwf, ctx.pw_shape = ((_i32(rpos, ref.device), _f32(pw.reshape(-1)), pw.shape) if weighted else (None, None, None))
    return need, z_only, collapse, table, src, ld_h, ref, N, ref.shape[1], _i32(pos, ref.device)


def _stack_folded_result(ctx, st, res, z_only, need):
    """what a stack returns for its folded output layer `st`: res (hg [G, D]), or with z_only (Z, the layer's packed weights)"""
    if z_only:
        res = (res, st.Wp)
        ctx.mark_non_differentiable(st.Wp)
        ctx.set_materialize_grads(False)        # (no zero "gradient" of the packed weights: a 4 MB fill per step)
    if not need:
        st.cl = st.desc = st.mask = st.Wp = st.X = None
    return res


def _stack_end(ctx, states, need, route):
    ctx.states = states if need else None
    note_route("stack", route)
    if _CAPTURE is not None:
        _CAPTURE.append((ctx.csr, ctx.cfg, states))


def _stack_bwd_begin(ctx, d_res, n_params, implicit=False):
    """(the saved states, d_res as fp32) -- or (None, the Function's all-None gradients) when no gradient arrived: collapse_z does not
    materialise absent gradients, Z took no part in the loss, and the saved state can go.  implicit: no tensor is expected (the
    matcher's 'dZ' travels through the FoldLink, not through autograd)."""
    states = ctx.states
    if states is None:
        raise RuntimeError(_BACKWARD_TWICE)
    if implicit:
        return states, None
    if d_res is None:
        ctx.states = None
        return None, (None,) * (6 + n_params)
    return states, _f32(d_res)


def _stack_bwd_end(ctx, states, d_X, d_pw, grads):
    """the Function's gradients (csr, cfg, h, pos, rpos, pw, *params) from the bottom layer's d_X; releases the saved state"""
    d_h = d_X[:, :states[0].Kh].contiguous() if ctx.h_req else None
    ctx.states = None
    if d_pw is not None:
        d_pw = d_pw.reshape(ctx.pw_shape)
    return (None, None, d_h, None, None, d_pw, *grads)


# ================================================================================================================
# Node features that are rows of a taxonomy feature table (SURVEY 8f-2 "dedup by _id")
# ================================================================================================================
class GatheredRows:
    """x[v] = table[index[v]], kept symbolic.  The batched egonets of an evaluation repeat every taxonomy node many times (MAG-Full:
    1.1 M batch nodes over 431 k taxonomy nodes); without dropout the first layer's projection depends only on (taxonomy node,
    position), so PGAT / PGCN in eval mode project the TABLE once (`projection_cache()` keeps it across the chunks of one evaluation)
    and gather.  Every other consumer sees the ordinary [N, d] tensor (materialised on first use)."""

    def __init__(self, table, index):
        self.table, self.index = table, index
        self._tensor = None

    shape = property(lambda self: torch.Size((self.index.shape[0], self.table.shape[1])))
    device = property(lambda self: self.table.device)
    dtype = property(lambda self: self.table.dtype)
    is_cuda = property(lambda self: self.table.is_cuda)
    requires_grad = False

    def dim(self):
        return 2

    def size(self, d=None):
        return self.shape if d is None else self.shape[d]

    def to(self, *args, **kwargs):
        t = self.table.to(*args, **kwargs)
        return self if t is self.table else GatheredRows(t, self.index.to(t.device))

    def tensor(self):
        if self._tensor is None:
            self._tensor = self.table.index_select(0, self.index.long())
        return self._tensor

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self.tensor(), name)

    def __getitem__(self, idx):
        return self.tensor()[idx]

    def __len__(self):
        return int(self.index.shape[0])

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        from torch.utils._pytree import tree_map
        owner = getattr(func, "__self__", None)
        if isinstance(owner, type) and issubclass(owner, torch.autograd.Function) and getattr(owner, "accepts_gathered_rows", False):
            with torch._C.DisableTorchFunctionSubclass():       # our own encoders take the symbolic form as it is
                return func(*args, **(kwargs or {}))
        un = lambda a: a.tensor() if isinstance(a, GatheredRows) else a
        return func(*tree_map(un, tuple(args)), **tree_map(un, dict(kwargs or {})))

    def __add__(self, other):
        return self.tensor() + other

    __radd__ = __add__

    def __mul__(self, other):
        return self.tensor() * other

    __rmul__ = __mul__

    def __repr__(self):
        return f"GatheredRows(table={tuple(self.table.shape)}, rows={int(self.index.shape[0])})"


_PROJ_CACHE = None


class projection_cache:
    """`with projection_cache(expected_rows):` -- table projections (first-layer W applied to a whole feature table) are reused by
    every forward inside the block.  Only for a scope in which the weights do not change (one evaluation pass).  expected_rows =
    how many batch nodes the pass will encode in total: the table is projected only if it has fewer rows than that (or than the
    batch at hand)."""

    def __init__(self, expected_rows=0):
        self.expected_rows = int(expected_rows)

    def __enter__(self):
        global _PROJ_CACHE
        self._prev, _PROJ_CACHE = _PROJ_CACHE, ({} if _PROJ_CACHE is None else _PROJ_CACHE)
        _PROJ_CACHE["expected_rows"] = max(_PROJ_CACHE.get("expected_rows", 0), self.expected_rows)
        return self

    def __exit__(self, *exc):
        global _PROJ_CACHE
        _PROJ_CACHE = self._prev
        return False


def _use_table(h, need, feat_p):
    """project the table instead of the batch?  only without gradients / dropout, and when it is less work (or already cached)"""
    return (isinstance(h, GatheredRows) and not need and feat_p == 0.0 and h.table.is_cuda and h.table.dim() == 2
            and h.table.dtype == torch.float32 and h.table.is_contiguous()
            and h.table.shape[0] <= max(h.index.shape[0], 0 if _PROJ_CACHE is None else _PROJ_CACHE.get("expected_rows", 0)))


def _gat_table_projection(st, src):
    """(T [n_table, Fp], T2 [vocab, Fp] or None): the packed first-layer weights applied to every row of the feature table and to the
    position-embedding rows -- features, a1 and a2 columns alike (they are all linear in the input)."""
    key = ("gat", src.table.data_ptr(), tuple(src.table.shape), st.W.data_ptr(), st.al.data_ptr(), None if st.P is None else st.P.data_ptr())
    if _PROJ_CACHE is not None and key in _PROJ_CACHE:
        return _PROJ_CACHE[key]
    tab = src.table
    n_tab, Kh, Kp, Fp = tab.shape[0], st.Kh, st.Kp, st.Fp
    s = _lib.stream_ptr()
    Kt = pure("txe_gat_padded_k", Kh, 0)
    Xt = _empty((n_tab, Kt), tab)
    call("txe_gat_build_x", ptr(tab), tab.stride(0), n_tab, Kh, None, None, 0, ptr(Xt), s)
    Wp = _empty((Fp, Kp), tab)
    call("txe_gat_pack_weights", ptr(st.W), ptr(st.al), ptr(st.ar), st.H, st.D, Kh + st.Pd, ptr(Wp), s)
    tws = _tail_ws(tab)
    T = _empty((n_tab, Fp), tab)
    # the padding columns [Kh, Kt) of Xt are zero, so whatever Wp holds there (position columns) does not contribute
    if _NO_SPLIT_GEMM:
        call("txe_gemm_plain", 0, ptr(Xt), Kt, ptr(Wp), Kp, ptr(T), Fp, n_tab, Fp, min(Kt, Kp), 1, 0, ptr(tws), tws.numel(), s)
    else:                                               # the table's projection on the bf16 pipe (route bit 8)
        wsb = pure("txe_gemm_plain_split_ws_bytes", n_tab, Fp, min(Kt, Kp))
        sws = _ws(wsb, tab)
        call("txe_gemm_plain", 0, ptr(Xt), Kt, ptr(Wp), Kp, ptr(T), Fp, n_tab, Fp, min(Kt, Kp), 1, 8, ptr(sws), wsb, s)
    T2 = None
    if st.Pd > 0:
        T2 = _empty((st.P.shape[0], Fp), tab)
        call("txe_gemm_plain", 0, ptr(st.P), st.Pd, ptr(Wp) + 4 * Kh, Kp, ptr(T2), Fp, st.P.shape[0], Fp, st.Pd, 1, 0, None, 0, s)
    if _PROJ_CACHE is not None:
        _PROJ_CACHE[key] = (T, T2, Wp, src.table, st.W)          # (operands kept alive: the key holds their addresses)
        return _PROJ_CACHE[key]
    return T, T2


def _gcn_table_projection(st, src):
    """(T [n_table, Fop], T2 [vocab, Fop] or None): the first GCNLayer's weight applied to every table row / position-embedding row"""
    key = ("gcn", src.table.data_ptr(), tuple(src.table.shape), st.W.data_ptr(), None if st.P is None else st.P.data_ptr())
    if _PROJ_CACHE is not None and key in _PROJ_CACHE:
        return _PROJ_CACHE[key]
    tab = src.table
    n_tab, Kh, Fop = tab.shape[0], st.Kh, st.Fop
    s = _lib.stream_ptr()
    Kt = pure("txe_gat_padded_k", Kh, 0)
    Xt = _empty((n_tab, Kt), tab)
    call("txe_gat_build_x", ptr(tab), tab.stride(0), n_tab, Kh, None, None, 0, ptr(Xt), s)
    kp128 = (st.Kp + 127) // 128 * 128
    Wp = _empty((kp128, Fop), tab)                 # [Kh + Pd (padded)][Fop]: feature rows first, then the position rows
    call("txe_gcn_pack_weights", ptr(st.W), Kh + st.Pd, st.Fo, ptr(Wp), s)
    tws = _tail_ws(tab)
    T = _empty((n_tab, Fop), tab)
    call("txe_gemm_plain", 1, ptr(Xt), Kt, ptr(Wp), Fop, ptr(T), Fop, n_tab, Fop, min(Kt, kp128), 1, 0, ptr(tws), tws.numel(), s)
    T2 = None
    if st.Pd > 0:
        T2 = _empty((st.P.shape[0], Fop), tab)
        call("txe_gemm_plain", 1, ptr(st.P), st.Pd, ptr(Wp) + 4 * Kh * Fop, Fop, ptr(T2), Fop, st.P.shape[0], Fop, st.Pd, 1, 0, None, 0, s)
    if _PROJ_CACHE is not None:
        _PROJ_CACHE[key] = (T, T2, Wp, src.table, st.W)
        return _PROJ_CACHE[key]
    return T, T2


# ================================================================================================================
# GAT stack (PGAT / GAT / a single GATLayer)
# ================================================================================================================
class GATConfig:
    """static description of a stack of GATLayers (model_zoo.py:52-114,169-220)"""

    def __init__(self, heads, out_dims, pos_dims, vocab, attn_slope, act_slope, feat_p, attn_p, final, seed):
        self.heads, self.out_dims, self.pos_dims, self.vocab = list(heads), list(out_dims), list(pos_dims), vocab
        self.attn_slope, self.act_slope = float(attn_slope), act_slope
        self.feat_p, self.attn_p = float(feat_p), float(attn_p)
        self.final = final          # 'mean' (PGAT/GAT: .mean(1) over heads of the last layer) | 'none' (GATLayer: N x H x D)
        self.seed = int(seed)
        self.n_layers = len(self.heads)
        # what the caller of one run adds on a copy: apply_stack its grad mode; DeferredNodeOutput._collapse `final` = 'collapse' /
        # 'collapse_z' and, for the latter, the FoldLink and the matcher's job (folded_match_job)
        self.grad_enabled, self.link, self.fold_job = True, None, None


def dropout_mask(n_rows, n_cols, p, seed, ref):
    """keep-bit mask (int32 words [n_rows, ceil(n_cols/32)]) of nn.Dropout(p) over an [n_rows, n_cols] operand, or None"""
    if p <= 0.0:
        return None
    mask = torch.empty((n_rows, (n_cols + 31) // 32), dtype=torch.int32, device=ref.device)
    call("txe_dropout_mask", n_rows, n_cols, p, seed, ptr(mask), _lib.stream_ptr())
    return mask


_tail_ws_cache = {}


def _tail_ws(ref):
    """persistent GEMM tail-splitting scratch per (device, stream): reuse is stream-ordered and the contents never outlive one
    GEMM + its fix-up kernel, so two streams (or threads on their own streams) must not share a buffer"""
    key = (ref.device.index, torch.cuda.current_stream(ref.device).cuda_stream)
    t = _tail_ws_cache.get(key)
    if t is None:
        t = torch.empty(pure("txe_gemm_tail_ws_bytes"), dtype=torch.uint8, device=ref.device)
        _tail_ws_cache[key] = t
    return t


class GatFolded(typing.NamedTuple):
    """what the folded GAT output layer's forward keeps for its backward (_GatLayerState.cl): a12 [N, 2] attention logits' halves, alpha [E]
    (destination-CSR order), coef [N] / wsum [G] of the readout, gid [N] node -> graph, Z [G, Kp], hg [G, D] (None when the stack stops at Z)"""
    a12: torch.Tensor
    alpha: torch.Tensor
    coef: torch.Tensor
    wsum: torch.Tensor
    gid: torch.Tensor
    Z: torch.Tensor
    hg: typing.Optional[torch.Tensor]


class _GatLayerState:
    __slots__ = ("N", "device", "X", "Wp", "mask", "Y", "alpha", "W", "al", "ar", "P", "pos", "Kh", "Pd", "Kp", "Fp", "H", "D", "seed", "cl",
                 "x_dropped", "Xt", "vx", "desc")

    def __init__(self, N=0, device=None):
        self.N, self.device = N, device     # the batch's node count; where the layer's buffers live (_empty / _ws take the state as `ref`)
        self.X = self.Wp = self.mask = self.Y = self.alpha = self.Xt = None
        self.W = self.al = self.ar = self.P = None
        self.pos = None             # the nodes' positions if the layer has a position table P, else None
        self.Kh = self.Pd = self.Kp = self.Fp = self.H = self.D = self.seed = 0
        self.cl = None              # GatFolded: the output layer folded behind the readout
        self.desc = None            # ... and its (_lib.GraphBatch, _lib.GatFoldLayer): raw addresses of the batch's and this state's tensors
        self.x_dropped = False
        self.vx = False             # X is NOT stored, it stays None (a first layer on the bf16 pipe: the packs form dropout([h | Emb[pos]]) themselves)


def _virtual_x_ok(st, h, ld_h, N, need, first_is_folded):
    """may a FIRST layer's input stay unwritten?  Its only readers must be the two packs of the bf16-pipe products: the projection
    (txe_gat_dense_fwd_split_src) and, with a backward pass to come, the weight gradient's contraction-major form (Xt)."""
    if _NO_SPLIT_GEMM or _NO_VIRTUAL_X or first_is_folded or N == 0 or not torch.is_tensor(h) or h.dtype != torch.float32:
        return False
    if pure("txe_gat_dense_split_ws_bytes", N, st.Kh, st.Pd, st.H, st.D) == 0:
        return False
    return (not need) or pure("txe_gat_dense_split_xt_bytes", N, st.Kh, st.Pd, st.H, st.D) > 0


def _x_dropped_ok(cfg, states, l, collapse):
    """may layer l's input be stored dropped?  Not the folded output layer (its sweeps apply the mask themselves); a layer above the
    first needs the aggregation below to drop what it writes: 16-byte rows, H <= 4 (the fast kernel family), an activation between."""
    L = len(states)
    if collapse and l == L - 1:
        return False
    if l == 0:
        return True
    sp = states[l - 1]
    return sp.D % 4 == 0 and states[l].Kp % 4 == 0 and sp.H <= 4


def _gat_layers_prepare(items, feat_p):
    """Several layers of a stack prepared in ONE launch (txe_gat_layers_prepare): layer input X = [h | Emb[pos] | 0] (h == None: the
    aggregation below writes the feature columns), packed weights, keep mask.  items = [(st, h, ld_h, dropped)], st.X allocated unless
    st.vx.  A layer's preparation never depends on the layer below's output, so the whole stack is prepared before its first GEMM.
    dropped: X is written with the feature dropout already applied (a first layer on raw features whose X only GEMMs read)."""
    descs = (_lib.GatPrepareDesc * len(items))()
    for d, (st, h, ld_h, dropped) in zip(descs, items):
        N = st.N
        st.Wp = _empty((st.Fp, st.Kp), st)
        st.mask = torch.empty((N, (st.Kh + st.Pd + 31) // 32), dtype=torch.int32, device=st.device) if feat_p > 0.0 else None
        d.h, d.ld_h, d.n_nodes, d.Kh, d.pos, d.P, d.Pd, d.X = ptr(h), ld_h, N, st.Kh, ptr(st.pos), ptr(st.P), st.Pd, ptr(st.X)
        d.W, d.attn_l, d.attn_r, d.H, d.D, d.Wp = ptr(st.W), ptr(st.al), ptr(st.ar), st.H, st.D, ptr(st.Wp)
        d.feat_drop_p, d.seed, d.mask = feat_p, st.seed, ptr(st.mask)
        st.x_dropped = bool(dropped and feat_p > 0.0)
        d.x_dropped = int(st.x_dropped)
    call("txe_gat_layers_prepare", ctypes.cast(descs, ctypes.c_void_p), len(items), _lib.stream_ptr())


def _graph_batch(csr, N):
    """the batch of graphs as the folded layers' entry points take it (raw addresses: csr owns the arrays)"""
    return _lib.GraphBatch(rowptr_in=ptr(csr.rowptr_in), col_src=ptr(csr.col_src), rowptr_out=ptr(csr.rowptr_out), col_dst=ptr(csr.col_dst),
                           pos_out=ptr(csr.pos_out), graph_off=ptr(csr.graph_off), n_nodes=N, n_edges=csr.n_edges, G=csr.n_graphs)


def _gat_collapse_fwd(csr, st, rpos, pw, feat_p, attn_p, attn_slope, a12=None, z_only=False, fold_job=None, link=None):
    """output layer (one head, prepared) folded behind the weighted-mean readout: hg [G, D] (txe_gat_collapse_fwd).
    a12 given: the previous layer's aggregation has formed its attention logits.
    z_only: stop at Z [G, Kp] (hg = Z W^T is left to the consumer: FoldedGraphLinearFunction / BilinearFoldedRunsFunction)."""
    N, G, E = st.N, csr.n_graphs, csr.n_edges
    ready = a12 is not None
    if not ready:
        a12 = _empty((max(N, 1), 2), st)
    alpha, coef = _empty((max(E, 1),), st), _empty((max(N, 1),), st)
    wsum, Z, hg = _empty((max(G, 1),), st), _empty((max(G, 1), st.Kp), st), (None if z_only else _empty((G, st.D), st))
    gid = torch.empty(max(N, 1), dtype=torch.int32, device=st.device)
    wsb = pure("txe_gat_collapse_ws_bytes", N, E, G, st.Kh, st.Pd, st.D, 8)
    split_hg = not z_only and G > 0 and not _NO_SPLIT_GEMM
    if split_hg:                                         # room for Z and the weight rows as packed planes: hg = Z W^T on the bf16 pipe
        wsb += pure("txe_gat_collapse_split_ws_bytes", G, st.Kh, st.Pd, st.D)
    ws = _ws(wsb, st)
    match = None
    if z_only and fold_job is not None and link is not None and N > 0 and G > 0 and not _NO_FOLD_EDOT:
        nt = pure("txe_gat_collapse_e_tiles", N, G, st.Kh, st.Pd)
        job = fold_job(st.Wp, st.D) if nt > 0 else None      # the matcher's runs, V and T, formed now: T rides in the Z sweep
        if job is not None:
            zrow = job.run_ids(G)
            link.fwd, link.e_part = job, _empty((N, nt), st)
            match = _lib.FoldMatch(Tf=ptr(job.T), zrow=ptr(zrow), e_part=ptr(link.e_part))
            job.score = FoldScore(csr.graph_off, N, G, st.Kh, st.Pd, coef, wsum, feat_p, int(st.mask is not None and feat_p > 0.0))
    # the descriptors hold raw addresses: st.cl (and st, csr) own the tensors, and both go when the state does
    st.cl = GatFolded(a12, alpha, coef, wsum, gid, Z, hg)
    batch = _graph_batch(csr, N)
    layer = _lib.GatFoldLayer(X=ptr(st.X), Kh=st.Kh, Pd=st.Pd, pos=ptr(rpos), Wp=ptr(st.Wp), W=ptr(st.W), attn_l=ptr(st.al), attn_r=ptr(st.ar),
                              D=st.D, feat_drop_p=feat_p, mask=ptr(st.mask), attn_slope=attn_slope, attn_drop_p=attn_p, seed=st.seed + 1,
                              pw=ptr(pw), a12=ptr(a12), alpha=ptr(alpha), coef=ptr(coef), wsum=ptr(wsum), gid=ptr(gid), Z=ptr(Z), hg=ptr(hg),
                              ld_hg=st.D)
    st.desc = (batch, layer)
    call("txe_gat_collapse_fwd", _lib.ref(batch), _lib.ref(layer), _lib.ref(match),
         (_lib.FOLD_A12_READY if ready else 0) | (_lib.FOLD_HG_SPLIT if split_hg else 0), ptr(ws), wsb, _lib.stream_ptr())
    return Z if z_only else hg


def _gat_fold_grads(st, layer, rpos, pw, vocab):
    """the folded layer's parameter-gradient tensors and their descriptor; sets what backward adds to the layer's: the vocabulary, and the
    positions as the position table's gradient reads them (forward had the readout's)"""
    dW, dal, dar = torch.empty_like(st.W), torch.empty_like(st.al), torch.empty_like(st.ar)
    dP = torch.empty_like(st.P) if st.P is not None else None
    d_pw = torch.empty_like(pw) if pw is not None else None
    layer.pos, layer.vocab = ptr(st.pos if st.pos is not None else rpos), max(vocab, pw.numel() if pw is not None else 0)
    return (dW, dal, dar, dP, d_pw), _lib.GatFoldGrads(dW=ptr(dW), d_attn_l=ptr(dal), d_attn_r=ptr(dar), dP=ptr(dP), d_pw=ptr(d_pw))


def _gat_collapse_bwd(csr, st, rpos, pw, vocab, d_hg, act_on, act_slope):
    N, G, E = st.N, csr.n_graphs, csr.n_edges
    batch, layer = st.desc
    d_hg, ld = _rows(d_hg)
    out, grads = _gat_fold_grads(st, layer, rpos, pw, vocab)
    d_X = _empty((N, st.Kp), st)
    wsb = pure("txe_gat_collapse_ws_bytes", N, E, G, st.Kh, st.Pd, st.D, max(layer.vocab, 8))
    ws = _ws(wsb, st)
    call("txe_gat_collapse_bwd", _lib.ref(batch), _lib.ref(layer), ptr(d_hg), ld, int(act_on), act_slope if act_slope else 1.0, ptr(d_X),
         _lib.ref(grads), ptr(ws), wsb, _lib.stream_ptr())
    return (d_X,) + out


def _gat_layer_fwd(csr, st, h, ld_h, out, ld_out, feat_p, attn_p, attn_slope, out_mode, act_slope, save, nxt=None, out_drop=None):
    """one prepared layer: projection (of X; of h, pos and the mask themselves when st.vx; of the table when h is a GatheredRows), then
    the attention / aggregation sweep into out.  nxt = (prepared state of the next, folded one-head layer, a12 buffer): its attention logits ride in the aggregation's epilogue."""
    H, D, Kh, Pd, Kp, Fp, pos = st.H, st.D, st.Kh, st.Pd, st.Kp, st.Fp, st.pos
    F = H * D
    s = _lib.stream_ptr()
    if isinstance(h, GatheredRows):            # eval-mode first layer on table rows: project the table, gather
        N = h.index.shape[0]
        T, T2 = _gat_table_projection(st, h)[:2]
        nx_kp = nxt[0].Kp if nxt is not None else 0
        if (T2 is not None and pos is not None and not save and not _NO_TABLE_SWEEP and attn_p == 0.0
                and pure("txe_gat_aggregate_table_supported", H, D, Fp, T2.shape[0], nx_kp) == 1):
            # the projected rows T[id] + T2[pos] are formed inside the sweep: no [N, Fp] round trip through HBM
            st.Y = st.alpha = None
            call("txe_gat_aggregate_table_fwd", ptr(csr.rowptr_in), ptr(csr.col_src), N, ptr(T), Fp, ptr(_i32(h.index, T.device)), ptr(T2),
                 ptr(pos), T2.shape[0], H, D, attn_slope, out_mode, act_slope, ptr(out), ld_out,
                 *((ptr(nxt[0].Wp) + 4 * nxt[0].D * nxt[0].Kp, nx_kp, ptr(nxt[1])) if nxt is not None else (None, 0, None)),
                 4 if _NO_EGO_WALK else (_FWD_SWEEP if H == 4 and D % 4 == 0 else 0), s)
            return
        st.Y = _empty((N, Fp), T)
        call("txe_gather_add_rows", ptr(T), Fp, ptr(_i32(h.index, T.device)), ptr(T2), Fp, ptr(pos) if T2 is not None else None, N, Fp,
             ptr(st.Y), Fp, s)
    else:
        N = st.N
        st.Y = _empty((N, Fp), st)
        tws = _tail_ws(st)
        dropped = st.x_dropped
        if (dropped or feat_p == 0.0) and not _NO_SPLIT_GEMM:      # X is a plain operand: fp32-accurate product on the bf16 pipe
            wsb = pure("txe_gat_dense_split_ws_bytes", N, Kh, Pd, H, D)
            sws = _ws(wsb, st)
            xtb = pure("txe_gat_dense_split_xt_bytes", N, Kh, Pd, H, D) if save else 0
            st.Xt = _ws(xtb, st) if xtb else None        # X packed contraction-major: the backward pass's weight gradient reads it
            if st.vx:                                      # X was never written: the packs read h, the position table and the mask
                call("txe_gat_dense_fwd_split_src", ptr(h), ld_h, ptr(pos), ptr(st.P), ptr(st.mask), feat_p if st.mask is not None else 0.0,
                     N, Kh, Pd, ptr(st.Wp), H, D, ptr(st.Xt), ptr(st.Y), ptr(sws), wsb, s)
            else:
                call("txe_gat_dense_fwd_split", ptr(st.X), N, Kh, Pd, ptr(st.Wp), H, D, None, None, ptr(st.Xt), ptr(st.Y), ptr(sws), wsb, s)
            note_route("proj", "bf16x6")
        else:
            call("txe_gat_dense_fwd", ptr(st.X), N, Kh, Pd, ptr(st.Wp), H, D, 0.0 if dropped else feat_p, None if dropped else ptr(st.mask), ptr(st.Y),
                 ptr(tws), tws.numel(), s)
            note_route("proj", "fp32")
        _launch_pending_prefetch()
    st.alpha = _empty((max(csr.n_edges, 1), H), st.Y) if save else None
    call("txe_gat_aggregate_fwd", ptr(csr.rowptr_in), ptr(csr.col_src), N, ptr(st.Y), Fp, ptr(st.Y) + 4 * F, ptr(st.Y) + 4 * (F + H), Fp,
         H, D, attn_slope, attn_p, st.seed + 1, out_mode, act_slope, ptr(out), ld_out, ptr(st.alpha),
         *((ptr(nxt[0].Wp) + 4 * nxt[0].D * nxt[0].Kp, nxt[0].Kp, ptr(nxt[0].mask), feat_p, ptr(nxt[1])) if nxt is not None
           else ((None, out_drop.Kp, ptr(out_drop.mask), feat_p, None) if out_drop is not None else (None, 0, None, 0.0, None))),
         4 if _NO_EGO_WALK else (_FWD_SWEEP if H == 4 and D % 4 == 0 else 0), s)


def _gat_aggregate_bwd(csr, st, attn_p, attn_slope, d_pre, ld_dpre):
    """message/reduce backward of one layer: d_Y [N, Fp] = [d_ft | d_a1 | d_a2 | 0] from the gradient of its aggregated output"""
    N = st.N
    H, D, Fp = st.H, st.D, st.Fp
    F, Fe = H * D, H * D + 2 * H
    d_Y = _empty((N, Fp), st)
    dz = _empty((max(csr.n_edges, 1) * H,), st)
    call("txe_gat_aggregate_bwd", ptr(csr.rowptr_in), ptr(csr.col_src), ptr(csr.rowptr_out), ptr(csr.col_dst), ptr(csr.pos_out),
         N, ptr(st.Y), Fp, ptr(st.Y) + 4 * F, ptr(st.Y) + 4 * (F + H), Fp, H, D, attn_slope, attn_p, st.seed + 1, ptr(st.alpha),
         ptr(d_pre), ld_dpre, ptr(d_Y), Fp, ptr(d_Y) + 4 * F, ptr(d_Y) + 4 * (F + H), Fp, ptr(dz), Fp - Fe, _lib.stream_ptr())   # clears d_Y's padding too
    return d_Y


class _TailChain:
    """the deferred phase-B reductions of a stack's backward pass (include/txe.h: txe_gat_dense_bwd `chain`): host memory the C entry
    points fill, plus the workspaces / operands the deferred jobs read -- kept alive until the launch that runs them has been enqueued
    (a buffer released earlier could be handed to a later allocation of the same stream and overwritten before that launch)"""

    def __init__(self):
        self.buf = ctypes.create_string_buffer(_lib.TAIL_CHAIN_BYTES)
        self.ptr = ctypes.cast(self.buf, ctypes.c_void_p)
        self.keep = []


def _gat_dense_bwd(st, vocab, feat_p, d_Y, need_dh, act_on, act_slope, chain=None, defer=False):
    """projection backward of one layer from d_Y: (d_X or None, dW, d_attn_l, d_attn_r, dP).
    chain / defer: see _TailChain (defer: this layer's last reduction launch is left to the bottom layer's)"""
    N = st.N
    dW, dal, dar = torch.empty_like(st.W), torch.empty_like(st.al), torch.empty_like(st.ar)
    dP = torch.empty_like(st.P) if st.P is not None else None
    d_X = _empty((N, st.Kp), st) if (need_dh or st.Pd > 0) else None
    wsb = pure("txe_gat_dense_ws_bytes", N, st.Kh, st.Pd, st.H, st.D, vocab)
    split_dx = bool(need_dh) and not _NO_SPLIT_GEMM
    if split_dx:                                       # room for d_Y and Wp as packed planes: d_X = d_Y Wp on the bf16 pipe
        wsb += pure("txe_gat_dense_bwd_split_ws_bytes", N, st.Kh, st.Pd, st.H, st.D)
    ws = _ws(wsb, st)
    def run(phases):
        call("txe_gat_dense_bwd", ptr(st.X), N, st.Kh, st.Pd, ptr(st.pos), vocab, ptr(st.Wp), ptr(st.W), ptr(st.al), ptr(st.ar), st.H, st.D, feat_p,
             ptr(st.mask), ptr(d_Y), int(need_dh), int(act_on), act_slope if act_slope else 1.0, ptr(d_X), ptr(dW), ptr(dal), ptr(dar),
             ptr(dP), int(st.x_dropped), ptr(st.Xt), phases, chain.ptr if chain is not None else None, ptr(ws), wsb, _lib.stream_ptr())
    # (a first PGAT layer's d_X -- position columns only -- is one HBM stream over d_Y, txe_dxpos.hip; every other d_X is a GEMM)
    run(_lib.DENSE_ALL | (_lib.DENSE_DX_SPLIT if split_dx else 0) | (_lib.PH_DEFER if (defer and chain is not None) else 0))
    if chain is not None:
        chain.keep += [ws, d_Y, st]
    return d_X, dW, dal, dar, dP


def _gat_layer_bwd(csr, st, vocab, feat_p, attn_p, attn_slope, d_pre, ld_dpre, need_dh, act_on, act_slope, chain=None, defer=False):
    d_Y = _gat_aggregate_bwd(csr, st, attn_p, attn_slope, d_pre, ld_dpre)
    return _gat_dense_bwd(st, vocab, feat_p, d_Y, need_dh, act_on, act_slope, chain, defer)


def _order(first, then):
    """work submitted to stream `then` from now on starts after everything already submitted to `first` (txe_stream_order: an event
    without the system-scope fence -- two streams of one device need no L2 write-back in front of the next kernel)"""
    call("txe_stream_order", first.cuda_stream, then.cuda_stream)


_side_streams = {}


def _side_stream(device):
    s = _side_streams.get(device.index)
    if s is None:
        s = _side_streams[device.index] = torch.cuda.Stream(device=device)
    return s


def _fused_bwd_ok(csr, st, sp):
    """can the folded layer `st`'s backward run fused with the message/reduce backward of the layer below `sp`?"""
    return (not _NO_FUSED_BWD and sp.alpha is not None and sp.H * sp.D == st.Kh and st.cl is not None and csr.n_edges > 0
            and pure("txe_gat_fused_bwd_supported", st.Kh, st.Pd, sp.H, sp.D) == 1)


class FoldLink:
    """What the producer of Z (GATStackFunction, cfg.final == 'collapse_z') shares with whoever consumes Z as the folded graph vector
    hg = Z W^T: the consumer's backward leaves the main part of the output layer's weight gradient here (S slices [D, Kp], summed in
    order) and hands dZ back through autograd; the producer's backward adds the attention rows' part and returns the whole dW."""
    __slots__ = ("part", "S", "fwd", "e_part", "ds", "s", "apply_exp", "by_k", "one_col")

    def __init__(self):
        self.part, self.S = None, 0
        # the producer's weight packing: a GAT layer's Wp [Fp][Kp] (rows < D the weight) or -- by_k -- a GCN layer's Wp [Kp128][Fop] (row k, D
        # columns; row one_col holds the bias and column one_col of Z counts as 1).  by_k: `part` comes back as [Kp][D], row one_col = d_bias
        self.by_k, self.one_col = False, -1
        # with a matcher job (fwd: the FoldJob of folded_match_job) the producer forms T before its Z sweep and the sweep leaves
        # <T[run(g)], keep X[u]> per node (e_part); backward's <dZ, X> sweep then becomes a scaling by the matcher's score gradient ds
        # (with the scores s and its apply_exp, left here by the matcher's backward)
        self.fwd, self.e_part = None, None
        self.ds, self.s, self.apply_exp = None, None, 0

    @property
    def carried_T(self):
        """the producer's Z sweep carried T: e_part is there and the job holds what sums the scores from it (FoldJob.score)"""
        return self.e_part is not None and self.fwd is not None and self.fwd.score is not None

    @property
    def dz_implicit(self):
        """the matcher's backward left its score gradient: the producer reads 'dZ[g]' as ds_g T[run(g)], no dZ tensor exists"""
        return self.e_part is not None and self.ds is not None

    def edot_args(self, zgid):
        """the matcher's share of txe_gat_collapse_bwd_fused, a _lib.FoldMatch (None unless dz_implicit); zgid: [N] int32 scratch"""
        if not self.dz_implicit:
            return None
        return _lib.FoldMatch(e_part=ptr(self.e_part), m_ds=ptr(self.ds), m_s=ptr(self.s), m_exp=int(self.apply_exp), Tf=ptr(self.fwd.T),
                              zrow=ptr(self.fwd.run_id), zgid=ptr(zgid))


_NO_LINK = FoldLink()  # (read only) what _gat_collapse_bwd_fused reads when nobody consumed Z: no weight-gradient part, no matcher's share


def walk_plan(csr):
    """the batch's plan for the egonet-walking sweeps (txe_egonet_walk_plan): a view of the graphs like the two CSR orders, built once per
    batch -- by the first backward pass that wants it, or by the loader that built the batch -- and kept on the CSR object"""
    key = id(csr.rowptr_in)                               # (the CSR views are cached on their graph: one tensor object per batch)
    ent = _WALK_PLANS.get(key)
    if ent is not None and ent[0]() is csr.rowptr_in:
        return ent[1]
    N = csr.n_nodes
    plan = torch.empty(pure("txe_egonet_walk_plan_bytes", N) // 4, dtype=torch.int32, device=csr.rowptr_in.device)
    call("txe_egonet_walk_plan", ptr(csr.rowptr_in), ptr(csr.col_src), ptr(csr.rowptr_out), ptr(csr.col_dst), ptr(csr.pos_out),
         ptr(csr.graph_off), N, csr.n_graphs, ptr(plan), _lib.stream_ptr())
    _WALK_PLANS[key] = (weakref.ref(csr.rowptr_in, lambda _ref, key=key: _WALK_PLANS.pop(key, None)), plan)   # (the plan dies with its graph)
    return plan


_WALK_PLANS = {}       # id of a CSR's rowptr_in tensor -> (weak reference to it, the plan)


def _gat_collapse_bwd_fused(csr, st, sp, rpos, pw, vocab, attn_p, attn_slope, d_hg, act_slope, chain=None, link=None):
    """txe_gat_collapse_bwd_fused: the folded layer's parameter gradients AND the layer below's d_Y in one sweep (no d_X).
    link given: d_hg IS dZ [G, Kp] (the consumer of Z folded hg = Z W^T into its own products, FoldLink)."""
    N, G, E = st.N, csr.n_graphs, csr.n_edges
    batch, layer = st.desc
    lk = link or _NO_LINK
    edot = lk.dz_implicit                           # the <dZ, X> sweep was done in forward (FoldLink)
    if d_hg is None:
        if not edot:
            raise RuntimeError("folded output layer: no gradient arrived for the graph vector")
        ld = st.Kp                                  # (edot: 'dZ[g]' is the matcher's ds_g T[run(g)], read from the link -- no tensor)
    else:
        d_hg, ld = _rows(d_hg)
    out, grads = _gat_fold_grads(st, layer, rpos, pw, vocab)
    d_Yp = _empty((N, sp.Fp), st)
    dz = _empty((max(E, 1) * sp.H,), st)
    below = _lib.GatFoldBelow(Yp=ptr(sp.Y), ld_yp=sp.Fp, Hp=sp.H, Dp=sp.D, attn_slope_p=attn_slope, attn_drop_p_p=attn_p, seed_p=sp.seed + 1,
                              alpha_p=ptr(sp.alpha), d_Yp=ptr(d_Yp), ld_dyp=sp.Fp, n_pad=sp.Fp - (sp.H * sp.D + 2 * sp.H), dz_p=ptr(dz))
    zgid = torch.empty(max(N, 1), dtype=torch.int32, device=st.device) if edot else None
    match = lk.edot_args(zgid)
    plan = walk_plan(csr) if (sp.H == 4 and not _NO_EGO_WALK and not _NO_WALK_PLAN) else None
    wsb = pure("txe_gat_collapse_bwd_fused_ws_bytes", N, E, G, st.Kh, st.Pd, st.D, max(layer.vocab, 8), sp.H)
    ws = _ws(wsb, st)
    # one set of descriptors for every call of this backward pass: the calls differ in `phases` alone
    args = (_lib.ref(batch), _lib.ref(layer), _lib.ref(below), _lib.ref(match), _lib.ref(grads), ptr(d_hg), ld, act_slope if act_slope else 1.0)
    rest = (ptr(lk.part) if lk.S > 0 else None, lk.S, ptr(plan), chain.ptr if chain is not None else None, ptr(ws), wsb)
    # the walk may form the parents' and siblings' X' rows again only where X' IS the activated aggregate of the layer below, stored
    # un-dropped (the folded layer's input always is un-dropped: _x_dropped_ok; out_mode 1 <=> an activation between the layers)
    reform = sp.H == 4 and not _NO_EGO_WALK and not _NO_REFORM_X and act_slope is not None and not st.x_dropped and st.X is not None
    note_route("bwd_walk", "reform" if reform else ("load" if sp.H == 4 and not _NO_EGO_WALK else "edges"))
    always = ((_lib.FUSED_EDOT if edot else 0) | (_lib.FUSED_NO_EGO_WALK if _NO_EGO_WALK else 0)
              | (0 if reform else _lib.WALK_NO_REFORM))

    def run(phases):
        call("txe_gat_collapse_bwd_fused", *args, phases | always, *rest, _lib.stream_ptr())
    last = _lib.FUSED_REDUCE | (_lib.PH_DEFER if chain is not None else 0)     # (with a chain the final reductions are left to the bottom layer's launch)
    if chain is not None:
        chain.keep += [ws, d_hg, st, sp, zgid] + ([link.part, link.fwd, link.ds, link.s] if link is not None else [])
    if link is not None:                            # dZ given: no product left in this layer's backward, nothing for a second stream
        if ld != st.Kp and not edot:
            raise RuntimeError("folded graph vector: dZ must have the padded row pitch")
        run(_lib.FUSED_SWEEP | _lib.FUSED_DZ_GIVEN)
        run(last | _lib.FUSED_DZ_GIVEN)
    elif _NO_SIDE_STREAM:
        run(_lib.FUSED_DZ | _lib.FUSED_DW | _lib.FUSED_SWEEP | last)
    else:
        # the folded layer's weight-gradient GEMM (MFMA-bound, needs only d_hg and Z) runs on a second stream under the HBM-bound
        # sweeps: complementary resources, and nothing downstream waits for it before the final reduction
        # (| FUSED_DW_BESIDE on every call: the product beside other kernels takes few fat k-slices, and the workspace is laid out for them)
        main, side = torch.cuda.current_stream(), _side_stream(st.device)
        _order(main, side)
        with torch.cuda.stream(side):
            run(_lib.FUSED_DW | _lib.FUSED_DW_BESIDE)
        run(_lib.FUSED_DZ | _lib.FUSED_DW_BESIDE)
        run(_lib.FUSED_SWEEP | _lib.FUSED_DW_BESIDE)
        _order(side, main)
        run(last | _lib.FUSED_DW_BESIDE)
    return (d_Yp,) + out


class GATStackFunction(torch.autograd.Function):
    """params per layer: (W [H*D, Kin], attn_l [1,H,D], attn_r [1,H,D], P [vocab, Pd] or None).
    cfg.final: 'mean' -> N x D (PGAT / GAT), 'none' -> N x H x D (GATLayer), 'collapse' -> G x D: the one-head output layer folded
    behind MeanReadout (pw None) / WeightedMeanReadout (pw = position_weights.weight, rpos = node positions)."""
    accepts_gathered_rows = True

    @staticmethod
    def forward(ctx, csr, cfg, h, pos, rpos, pw, *params):
        need, z_only, collapse, table, src, ld_h, ref, N, kh, pos = _stack_begin(ctx, csr, cfg, h, pos, rpos, pw, params, cfg.feat_p)
        L = cfg.n_layers
        states = []
        with _lib.on_device(ref.device):
            for l in range(L):
                st = _GatLayerState(N, ref.device)
                st.W, st.al, st.ar, st.P = (_f32(p) for p in params[4 * l:4 * l + 4])
                st.H, st.D, st.Kh = cfg.heads[l], cfg.out_dims[l], kh
                st.Pd, st.pos = (0, None) if st.P is None else (st.P.shape[1], pos)
                st.Kp = pure("txe_gat_padded_k", st.Kh, st.Pd)
                st.Fp = pure("txe_gat_padded_f", st.H, st.D)
                st.seed = cfg.seed + 16 * l
                states.append(st)
                kh = st.H * st.D
            # every layer's input buffer now (not the first's where the table or the packs stand in for it), and ONE preparation launch for
            # the whole stack.  (a layer that is not the folded one: only its GEMMs read X, so X is stored with the dropout applied -- by
            #  the preparation (raw features, position columns) and by the aggregation of the layer below (out_drop))
            states[0].vx = (not table) and _virtual_x_ok(states[0], src, ld_h, N, need, collapse and L == 1)
            todo = states[1:] if (table or states[0].vx) else states
            for st in todo:
                st.X = _empty((N, st.Kp), st)
            _gat_layers_prepare([(st, (src if l == 0 else None), (ld_h if l == 0 else 0), _x_dropped_ok(cfg, states, l, collapse))
                                 for l, st in enumerate(states) if not (table and l == 0)], cfg.feat_p)
            fused_a12 = None
            for l, st in enumerate(states):
                last = (l == L - 1)
                if last and collapse:
                    res = _gat_collapse_fwd(csr, st, ctx.rpos, ctx.pwf, cfg.feat_p, cfg.attn_p, cfg.attn_slope, a12=fused_a12, z_only=z_only,
                                            fold_job=cfg.fold_job if (z_only and need) else None, link=cfg.link)
                    res = _stack_folded_result(ctx, st, res, z_only, need)
                    break
                F = st.H * st.D
                # (not the last layer: the aggregation writes straight into the next layer's padded input)
                out, ld_out = (_empty((N, F), st), F) if last else (states[l + 1].X, states[l + 1].Kp)
                nxt = None
                if (collapse and l + 1 == L - 1 and N > 0 and st.D % 4 == 0 and states[l + 1].Kp - F <= 128 and states[l + 1].Kp <= 4096
                        and not _NO_FUSED_LOGITS):
                    # the folded output layer's keep mask and folded attention rows feed this layer's epilogue
                    fused_a12 = _empty((N, 2), st)
                    nxt = (states[l + 1], fused_a12)
                # (the layer above reads its input through plain GEMM operands: this layer's aggregation applies that layer's dropout)
                out_drop = states[l + 1] if (not last and nxt is None and states[l + 1].x_dropped) else None
                _gat_layer_fwd(csr, st, src if l == 0 else None, ld_h if l == 0 else 0, out, ld_out, cfg.feat_p, cfg.attn_p, cfg.attn_slope,
                               0 if (last or cfg.act_slope is None) else 1, cfg.act_slope or 1.0, need, nxt, out_drop)
                if not need:
                    st.Y = st.mask = st.Wp = None
                    if l > 0:
                        st.X = None
            H, D = cfg.heads[-1], cfg.out_dims[-1]
            if collapse:
                pass
            elif cfg.final == "mean" and H > 1:
                res = _empty((N, D), ref)
                call("txe_head_mean_fwd", ptr(out), H, D, N, ptr(res), _lib.stream_ptr())
            else:
                res = out.view(N, D) if cfg.final == "mean" else out.view(N, H, D)
        ctx.param_ids, ctx.pw_id = [id(p) for p in params], id(pw)
        _stack_end(ctx, states, need, cfg.final + ("+edot" if (ctx.link is not None and ctx.link.carried_T) else ""))
        return res

    @staticmethod
    def backward(ctx, d_res, *_unused):
        csr, cfg = ctx.csr, ctx.cfg
        L = cfg.n_layers
        H, D = cfg.heads[-1], cfg.out_dims[-1]
        z_only = (cfg.final == "collapse_z")
        collapse = (cfg.final == "collapse") or z_only
        edot = ctx.link is not None and ctx.link.dz_implicit
        states, d_res = _stack_bwd_begin(ctx, d_res, 4 * L, implicit=edot)
        if states is None:
            return d_res
        N = states[0].N
        grads = [None] * (4 * L)
        d_pw = None
        note_route("stack_bwd", "fused+edot" if edot else ("collapse" if collapse else "layers"))
        with _lib.on_device(states[0].device):
            if collapse:
                d_pre, ld_dpre = None, 0
            elif cfg.final == "mean" and H > 1:
                d_pre = _empty((N, H * D), d_res)
                call("txe_head_mean_bwd", ptr(d_res), H, D, N, ptr(d_pre), _lib.stream_ptr())
            else:
                d_pre = d_res.reshape(N, H * D)
            if d_pre is not None:
                ld_dpre = d_pre.stride(0)
            d_X = None
            d_Y_ready = None                       # d_Y of layer l already produced by the fused sweep of layer l+1
            # the layers' last reduction launches (parameter gradients only) are chained into the bottom layer's -- unless somebody
            # wants every layer's gradients the moment its backward ends (the overlapped gradient all-reduce)
            chain = _TailChain() if (_GRAD_READY is None and L > 1 and not _NO_TAIL_CHAIN) else None
            for l in range(L - 1, -1, -1):
                st = states[l]
                need_dh = (l > 0) or ctx.h_req
                # the input of layer l>0 is leaky_relu(out_{l-1}) (fused epilogue): fold its derivative into dX
                act_on = (l > 0 and cfg.act_slope is not None)
                if collapse and l == L - 1:
                    if l > 0 and _fused_bwd_ok(csr, st, states[l - 1]):
                        d_Y_ready, dW, dal, dar, dP, d_pw = _gat_collapse_bwd_fused(
                            csr, st, states[l - 1], ctx.rpos, ctx.pwf, cfg.vocab, cfg.attn_p, cfg.attn_slope, d_res,
                            cfg.act_slope if act_on else None, chain, link=(ctx.link or FoldLink()) if z_only else None)
                    elif z_only:
                        raise RuntimeError("collapse_z was requested for a stack whose fused backward does not apply (folded_graph_vector_ok)")
                    else:
                        d_X, dW, dal, dar, dP, d_pw = _gat_collapse_bwd(csr, st, ctx.rpos, ctx.pwf, cfg.vocab, d_res, act_on, cfg.act_slope)
                elif d_Y_ready is not None:
                    d_X, dW, dal, dar, dP = _gat_dense_bwd(st, cfg.vocab, cfg.feat_p, d_Y_ready, need_dh, act_on, cfg.act_slope, chain,
                                                           defer=l > 0)
                    d_Y_ready = None
                else:
                    d_X, dW, dal, dar, dP = _gat_layer_bwd(csr, st, cfg.vocab, cfg.feat_p, cfg.attn_p, cfg.attn_slope, d_pre, ld_dpre, need_dh,
                                                           act_on, cfg.act_slope, chain, defer=l > 0)
                grads[4 * l:4 * l + 4] = [dW, dal, dar, dP]
                if _GRAD_READY is not None:               # (tensors, ids of the parameters they are the gradients of)
                    last_c = collapse and l == L - 1
                    _GRAD_READY(l, [dW, dal, dar, dP] + ([d_pw] if last_c else []), ctx.param_ids[4 * l:4 * l + 4] + ([ctx.pw_id] if last_c else []))
                if l > 0 and d_Y_ready is None:
                    d_pre, ld_dpre = d_X, st.Kp            # its first H*D(l-1) columns are d(pre-activation out_{l-1})
            res = _stack_bwd_end(ctx, states, d_X, d_pw, grads)
            if chain is not None:                  # (nothing left unless the bottom layer took a route without a phase B of its own)
                call("txe_gat_tail_flush", chain.ptr, _lib.stream_ptr())
                chain.keep = []
            if _GRAD_FLUSH is not None:
                _GRAD_FLUSH()
        return res


# ================================================================================================================
# GCN stack (PGCN / GCN / a single GCNLayer)
# ================================================================================================================
class GCNConfig:
    def __init__(self, out_dims, vocab, act_slopes, drop_ps, seed):
        self.out_dims, self.vocab = list(out_dims), vocab
        self.act_slopes = list(act_slopes)      # per layer: slope of the fused leaky_relu or None
        self.drop_ps = [float(p) for p in drop_ps]
        self.seed = int(seed)
        self.n_layers = len(self.out_dims)
        # 'layers' (N x Fo), or what DeferredNodeOutput._collapse sets on a copy: 'collapse' / 'collapse_z' with its FoldLink (see GATConfig)
        self.final, self.grad_enabled, self.link, self.fold_job = "layers", True, None, None


class GcnFolded(typing.NamedTuple):
    """what the folded GCN output layer's forward keeps for its backward (_GcnLayerState.cl): as in GatFolded"""
    coef: torch.Tensor
    wsum: torch.Tensor
    gid: torch.Tensor
    Z: torch.Tensor


class _GcnLayerState:
    __slots__ = ("N", "device", "X", "Wp", "mask", "W", "b", "P", "pos", "Kh", "Pd", "Kp", "Fo", "Fop", "seed", "cl", "x_dropped", "desc")

    def __init__(self, N=0, device=None):
        self.N, self.device = N, device     # as in _GatLayerState
        self.X = self.Wp = self.mask = self.W = self.b = self.P = None
        self.pos = None             # the nodes' positions if the layer has a position table P, else None
        self.Kh = self.Pd = self.Kp = self.Fo = self.Fop = self.seed = 0
        self.cl = None              # GcnFolded: the output layer folded behind the readout
        self.desc = None            # ... and its (_lib.GraphBatch, _lib.GcnFoldLayer), as in _GatLayerState
        self.x_dropped = False


def _gcn_layers_prepare(csr, cfg, todo, h, ld_h, norm, collapse, z_only):
    """_gat_layers_prepare for GCN layers, todo = [(l, st)] with st.X allocated: ONE launch (txe_gcn_layers_prepare) writes the layer
    inputs' position / padding columns (layer 0: the features h too), the packed weights and the keep masks -- none of it depends on
    a layer below's output -- and forms the degree normalisation `norm`.  Nothing to prepare (one layer, on the table route): txe_gcn_norm."""
    if not todo:
        call("txe_gcn_norm", ptr(csr.rowptr_in), csr.n_nodes, ptr(norm), _lib.stream_ptr())
        return
    descs = (_lib.GcnPrepareDesc * len(todo))()
    for d, (l, st) in zip(descs, todo):
        N, drop_p, folded = st.N, cfg.drop_ps[l], (collapse and l == cfg.n_layers - 1)
        st.Wp = _empty(((st.Kp + 127) // 128 * 128, st.Fop), st)
        st.mask = torch.empty((N, (st.Kh + st.Pd + 31) // 32), dtype=torch.int32, device=st.device) if drop_p > 0.0 else None
        # (a first layer on raw features that is not the folded one: only its GEMMs read X -> stored with the dropout applied)
        st.x_dropped = bool(l == 0 and not folded and drop_p > 0.0)
        # (folded into the matcher: the bias rides as one more weight row, behind a column of Z that counts as 1)
        bias_row = st.b if (folded and z_only) else None
        d.h, d.ld_h, d.n_nodes, d.Kh = ptr(h if l == 0 else None), (ld_h if l == 0 else 0), N, st.Kh
        d.pos, d.P, d.Pd, d.X = ptr(st.pos), ptr(st.P), st.Pd, ptr(st.X)
        d.W, d.Fo, d.Wp, d.drop_p, d.seed, d.mask = ptr(st.W), st.Fo, ptr(st.Wp), drop_p, st.seed, ptr(st.mask)
        d.x_dropped, d.bias_row = int(st.x_dropped), ptr(bias_row)
    call("txe_gcn_layers_prepare", ctypes.cast(descs, ctypes.c_void_p), len(todo), ptr(csr.rowptr_in), csr.n_nodes, ptr(norm), _lib.stream_ptr())


def _gcn_layer_fwd(csr, st, h, norm, out, ld_out, drop_p, act_slope):
    """one prepared layer: the projection hw = dropout(X) W (h a GatheredRows: gathered from the projected table instead), then the
    normalised aggregation + bias (+ leaky_relu, act_slope not None) into out"""
    N, s = st.N, _lib.stream_ptr()
    hw = _empty((N, st.Fop), st)
    if isinstance(h, GatheredRows):            # eval-mode first layer on table rows: project the table, gather
        T, T2 = _gcn_table_projection(st, h)[:2]
        call("txe_gather_add_rows", ptr(T), st.Fop, ptr(_i32(h.index, st.device)), ptr(T2), st.Fop, ptr(st.pos) if T2 is not None else None,
             N, st.Fop, ptr(hw), st.Fop, s)
        st.mask = st.Wp = None
    else:
        tws = _tail_ws(st)
        call("txe_gcn_dense_fwd", ptr(st.X), N, st.Kh, st.Pd, ptr(st.Wp), st.Fo, 0.0 if st.x_dropped else drop_p,
             None if st.x_dropped else ptr(st.mask), ptr(hw), ptr(tws), tws.numel(), s)
        _launch_pending_prefetch()
    call("txe_gcn_aggregate_fwd", ptr(csr.rowptr_in), ptr(csr.col_src), N, ptr(hw), st.Fop, ptr(norm), ptr(st.b),
         0 if act_slope is None else 1, act_slope or 1.0, st.Fo, ptr(out), ld_out, s)


def _gcn_collapse_fwd(csr, st, rpos, pw, norm, drop_p, z_only=False, link=None):
    """the (activation-free, prepared) output layer folded behind the weighted-mean readout: hg [G, Fo] (txe_gcn_collapse_fwd).
    z_only: stop at Z [G, Kp]; the consumer of Z learns from `link` how this layer's weights are packed (FoldLink.by_k / one_col)."""
    N, G = st.N, csr.n_graphs
    coef, wsum = _empty((max(N, 1),), st), _empty((max(G, 1),), st)
    gid = torch.empty(max(N, 1), dtype=torch.int32, device=st.device)
    Z, hg = _empty((max(G, 1), st.Kp), st), (None if z_only else _empty((G, st.Fo), st))
    wsb = pure("txe_gcn_collapse_ws_bytes", N, G, st.Kh, st.Pd, st.Fo, 8)
    ws = _ws(wsb, st)
    # the descriptors hold raw addresses: st.cl (and st, csr, ctx.norm) own the tensors, and both go when the state does
    st.cl = GcnFolded(coef, wsum, gid, Z)
    batch = _graph_batch(csr, N)
    layer = _lib.GcnFoldLayer(X=ptr(st.X), Kh=st.Kh, Pd=st.Pd, pos=ptr(rpos), Wp=ptr(st.Wp), Fo=st.Fo, bias=ptr(st.b), drop_p=drop_p,
                              mask=ptr(st.mask), norm=ptr(norm), pw=ptr(pw), coef=ptr(coef), wsum=ptr(wsum), gid=ptr(gid), Z=ptr(Z),
                              hg=ptr(hg), ld_hg=st.Fo)
    st.desc = (batch, layer)
    call("txe_gcn_collapse_fwd", _lib.ref(batch), _lib.ref(layer), ptr(ws), wsb, _lib.stream_ptr())
    if z_only and link is not None:
        link.by_k, link.one_col = True, (st.Kh + st.Pd if st.b is not None else -1)
    return Z if z_only else hg


def _gcn_layer_bwd(csr, st, norm, vocab, drop_p, d_pre, ld_dpre, need_dh, act_slope):
    """one layer's backward from the gradient of its aggregated (pre-activation) output: (d_X or None, dW, d_b, dP).
    act_slope: of the leaky_relu that produced this layer's input (None: none), its derivative is folded into d_X"""
    N, s = st.N, _lib.stream_ptr()
    d_hw = _empty((N, st.Fop), st)
    d_b = torch.empty_like(st.b) if st.b is not None else None
    wsb = pure("txe_gcn_aggregate_bwd_ws_bytes", N, st.Fo)
    ws = _ws(wsb, st)
    call("txe_gcn_aggregate_bwd", ptr(csr.rowptr_out), ptr(csr.col_dst), N, ptr(d_pre), ld_dpre, ptr(norm), st.Fo, ptr(d_hw), st.Fop, ptr(d_b),
         ptr(ws), wsb, s)
    d_X = _empty((N, st.Kp), st) if (need_dh or st.Pd > 0) else None
    dW = torch.empty_like(st.W)
    dP = torch.empty_like(st.P) if st.P is not None else None
    wsb2 = pure("txe_gcn_dense_ws_bytes", N, st.Kh, st.Pd, st.Fo, vocab)
    ws2 = _ws(wsb2, st)
    call("txe_gcn_dense_bwd", ptr(st.X), N, st.Kh, st.Pd, ptr(st.pos), vocab, ptr(st.Wp), st.Fo, drop_p, ptr(st.mask), ptr(d_hw), int(need_dh),
         int(act_slope is not None), 1.0 if act_slope is None else act_slope, ptr(d_X), ptr(dW), ptr(dP), int(st.x_dropped), ptr(ws2), wsb2, s)
    return d_X, dW, d_b, dP


def _gcn_collapse_bwd(csr, st, rpos, pw, vocab, d_hg, act_slope, z_only=False, link=None):
    """the folded layer's backward (txe_gcn_collapse_bwd): (d_X, dW, d_b, dP, d_pw).  z_only: d_hg IS dZ [G, Kp], and the consumer of Z
    left dW (and d_b as row Kh + Pd) in link.part [Kp][Fo]"""
    N, G = st.N, csr.n_graphs
    batch, layer = st.desc
    d_hg, ld = _rows(d_hg)
    if z_only:
        part = link.part if link is not None else None
        if part is None or link.S != 1 or tuple(part.shape) != (st.Kp, st.Fo):
            raise RuntimeError("folded GCN output layer: the consumer of Z left no weight gradient in the FoldLink")
        Kt = st.Kh + st.Pd
        dW, d_b = part[:Kt], (part[Kt] if st.b is not None else None)
    else:
        dW = torch.empty_like(st.W)
        d_b = torch.empty_like(st.b) if st.b is not None else None
    d_X = _empty((N, st.Kp), st)
    dP = torch.empty_like(st.P) if st.P is not None else None
    d_pw = torch.empty_like(pw) if pw is not None else None
    # (what backward adds to the layer's descriptor: the vocabulary, and the positions as the position table's gradient reads them)
    layer.pos, layer.vocab = ptr(st.pos if st.pos is not None else rpos), max(vocab, pw.numel() if pw is not None else 0)
    wsb = pure("txe_gcn_collapse_ws_bytes", N, G, st.Kh, st.Pd, st.Fo, max(layer.vocab, 8))
    ws = _ws(wsb, st)
    grads = _lib.GcnFoldGrads(dW=None if z_only else ptr(dW), d_b=None if z_only else ptr(d_b), dP=ptr(dP), d_pw=ptr(d_pw))
    call("txe_gcn_collapse_bwd", _lib.ref(batch), _lib.ref(layer), ptr(d_hg), ld, int(act_slope is not None), 1.0 if act_slope is None else act_slope,
         ptr(d_X), _lib.ref(grads), int(z_only), ptr(ws), wsb, _lib.stream_ptr())
    return d_X, dW, d_b, dP, d_pw


class GCNStackFunction(torch.autograd.Function):
    """params per layer: (W [Kin, Fo], bias [Fo] or None, P [vocab, Pd] or None).
    cfg.final == 'collapse': G x Fo -- the (activation-free) output layer folded behind MeanReadout (pw None) /
    WeightedMeanReadout (txe_gcn_collapse_*)."""

    accepts_gathered_rows = True

    @staticmethod
    def forward(ctx, csr, cfg, h, pos, rpos, pw, *params):
        need, z_only, collapse, table, src, ld_h, ref, N, kh, pos = _stack_begin(ctx, csr, cfg, h, pos, rpos, pw, params, cfg.drop_ps[0])
        L = cfg.n_layers
        states = []
        with _lib.on_device(ref.device):
            for l in range(L):
                st = _GcnLayerState(N, ref.device)
                st.W, st.b, st.P = (_f32(p) for p in params[3 * l:3 * l + 3])
                st.Kh, st.Fo = kh, cfg.out_dims[l]
                st.Pd, st.pos = (0, None) if st.P is None else (st.P.shape[1], pos)
                st.Kp = pure("txe_gat_padded_k", st.Kh, st.Pd)
                st.Fop = pure("txe_gcn_padded_f", st.Fo)
                st.seed = cfg.seed + 16 * l
                states.append(st)
                kh = st.Fo
            # every layer's input buffer now (not the first's on the table route), and ONE preparation launch for the whole stack
            norm = _empty((max(N, 1),), ref)
            todo = [(l, st) for l, st in enumerate(states) if not (table and l == 0)]
            for l, st in todo:
                st.X = _empty((N, st.Kp), st)
            _gcn_layers_prepare(csr, cfg, todo, src, ld_h, norm, collapse, z_only)
            for l, st in enumerate(states):
                last = (l == L - 1)
                if last and collapse:
                    out = _gcn_collapse_fwd(csr, st, ctx.rpos, ctx.pwf, norm, cfg.drop_ps[l], z_only, cfg.link)
                    out = _stack_folded_result(ctx, st, out, z_only, need)
                    break
                # (not the last layer: the aggregation writes straight into the next layer's padded input)
                out, ld_out = (_empty((N, st.Fo), st), st.Fo) if last else (states[l + 1].X, states[l + 1].Kp)
                _gcn_layer_fwd(csr, st, src if l == 0 else None, norm, out, ld_out, cfg.drop_ps[l], cfg.act_slopes[l])
                if not need:
                    st.mask = st.Wp = None
                    if l > 0:
                        st.X = None
        ctx.norm = norm
        ctx.out = out if (need and not z_only) else None     # (a standalone activated layer's backward reads its output)
        _stack_end(ctx, states, need, cfg.final)
        return out

    @staticmethod
    def backward(ctx, d_out, *_unused):
        csr, cfg, norm = ctx.csr, ctx.cfg, ctx.norm
        L = cfg.n_layers
        collapse = cfg.final in ("collapse", "collapse_z")
        states, d_out = _stack_bwd_begin(ctx, d_out, 3 * L)
        if states is None:
            return d_out
        grads = [None] * (3 * L)
        d_pw = None
        with _lib.on_device(states[0].device):
            if collapse:
                d_pre = None
            elif cfg.act_slopes[-1] is not None:   # a standalone activated layer: undo the fused activation explicitly
                d_pre = torch.empty_like(d_out)
                call("txe_leaky_relu_bwd", ptr(d_out), ptr(ctx.out), cfg.act_slopes[-1], d_out.numel(), ptr(d_pre), _lib.stream_ptr())
            else:
                d_pre = d_out
            ld_dpre = d_pre.stride(0) if d_pre is not None else 0
            d_X = None
            for l in range(L - 1, -1, -1):
                st = states[l]
                # the input of layer l>0 is leaky_relu(out_{l-1}) (fused epilogue, where layer l-1 has an activation): fold its derivative into dX
                act_slope = cfg.act_slopes[l - 1] if l > 0 else None
                if collapse and l == L - 1:
                    d_X, dW, d_b, dP, d_pw = _gcn_collapse_bwd(csr, st, ctx.rpos, ctx.pwf, cfg.vocab, d_out, act_slope,
                                                               cfg.final == "collapse_z", ctx.link)
                else:
                    d_X, dW, d_b, dP = _gcn_layer_bwd(csr, st, norm, cfg.vocab, cfg.drop_ps[l], d_pre, ld_dpre, (l > 0) or ctx.h_req, act_slope)
                grads[3 * l:3 * l + 3] = [dW, d_b, dP]
                if l > 0:
                    d_pre, ld_dpre = d_X, st.Kp            # its first Fo(l-1) columns are d(pre-activation out_{l-1})
            return _stack_bwd_end(ctx, states, d_X, d_pw, grads)


# ================================================================================================================
# Readout (MeanReadout / WeightedMeanReadout)
# ================================================================================================================
class ReadoutFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, csr, h, pos, pw):
        _need_cuda(h, pw)
        h, ld_h = _rows(h)
        G, D = csr.n_graphs, h.shape[1]
        pos = _i32(pos, h.device) if pw is not None else None
        pwf = _f32(pw.reshape(-1)) if pw is not None else None
        hg, wsum = _empty((G, D), h), _empty((max(G, 1),), h)
        with _lib.on_device(h.device):
            call("txe_readout_fwd", ptr(csr.graph_off), G, ptr(h), ld_h, ptr(pos), ptr(pwf), D, ptr(hg), ptr(wsum),
                 _lib.stream_ptr())
        ctx.csr, ctx.pos, ctx.misc = csr, pos, (h, ld_h, pwf, hg, wsum)
        ctx.pw_shape = None if pw is None else pw.shape
        return hg

    @staticmethod
    def backward(ctx, d_hg):
        csr, pos = ctx.csr, ctx.pos
        h, ld_h, pwf, hg, wsum = ctx.misc
        G, D = csr.n_graphs, h.shape[1]
        d_hg = _f32(d_hg)
        d_h = _empty((h.shape[0], D), h)
        vocab = 0 if pwf is None else pwf.numel()
        d_pw = torch.empty_like(pwf) if pwf is not None else None
        ws = _empty((max(G, 1) * max(vocab, 1),), h) if pwf is not None else None
        with _lib.on_device(h.device):
            call("txe_readout_bwd", ptr(csr.graph_off), G, ptr(h), ld_h, ptr(pos), ptr(pwf), vocab, D, ptr(hg), ptr(wsum), ptr(d_hg),
                 ptr(d_h), D, ptr(d_pw), ptr(ws), _lib.stream_ptr())
        return None, d_h, None, (d_pw.reshape(ctx.pw_shape) if d_pw is not None else None)


class ReadoutMultiFunction(torch.autograd.Function):
    """mode 1 SumReadout, 2 MaxReadout, 3 ConcatReadout (model_zoo.py:244-276)"""

    @staticmethod
    def forward(ctx, csr, h, pos, mode):
        _need_cuda(h)
        h, ld_h = _rows(h)
        G, D = csr.n_graphs, h.shape[1]
        pos = _i32(pos, h.device) if mode == 3 else None
        hg = _empty((G, 3 * D if mode == 3 else D), h)
        argmax = torch.empty((max(G, 1), D), dtype=torch.int32, device=h.device) if mode == 2 else None
        with _lib.on_device(h.device):
            call("txe_readout_multi_fwd", ptr(csr.graph_off), G, ptr(h), ld_h, ptr(pos), D, mode, ptr(hg), ptr(argmax), _lib.stream_ptr())
        ctx.misc = (csr, pos, mode, argmax, h.shape[0], D)
        return hg

    @staticmethod
    def backward(ctx, d_hg):
        csr, pos, mode, argmax, N, D = ctx.misc
        d_hg = _f32(d_hg)
        d_h = _empty((N, D), d_hg)
        with _lib.on_device(d_hg.device):
            call("txe_readout_multi_bwd", ptr(csr.graph_off), csr.n_graphs, ptr(pos), D, mode, ptr(d_hg), ptr(argmax), ptr(d_h), D,
                 _lib.stream_ptr())
        return None, d_h, None, None


class ReadoutAttnFunction(torch.autograd.Function):
    """AttentionReadout (model_zoo.AttentionReadout): hg[g] = sum_v alpha_v h[v], alpha = softmax over the egonet of
    s_v = <u, tanh(Y[v] + P[pos_v])>, with Y = gate_hidden(h) handed in by the caller (a LinearFunction, whose own backward carries d_Y on
    to h and the gate's weights).  Returns (hg [G, D], alpha [N]); alpha is not differentiable."""

    @staticmethod
    def forward(ctx, csr, h, Y, pos, P, u):
        _need_cuda(h, Y, P, u)
        h, ld_h = _rows(h)
        Y, ld_y = _rows(Y)
        G, N, D, A = csr.n_graphs, h.shape[0], h.shape[1], Y.shape[1]
        Pf, uf = _f32(P), _f32(u.reshape(-1))
        if Y.shape[0] != N or tuple(Pf.shape[1:]) != (A,) or uf.numel() != A:
            raise ValueError("ReadoutAttnFunction: h [N, D], Y [N, A], P [vocab, A] and u [A] do not fit together")
        pos = _i32(pos, h.device)
        if G == 0 or N == 0:                                # nothing to launch (an empty tensor has no address to hand over)
            hg, alpha = h.new_zeros((G, D)), _empty((N,), h)
        else:
            hg, alpha = _empty((G, D), h), _empty((N,), h)
            with _lib.on_device(h.device):
                call("txe_readout_attn_fwd", ptr(csr.graph_off), G, ptr(h), ld_h, D, ptr(Y), ld_y, A, ptr(pos), ptr(Pf), Pf.shape[0],
                     ptr(uf), ptr(hg), ptr(alpha), _lib.stream_ptr())
        ctx.csr, ctx.pos, ctx.misc = csr, pos, (h, ld_h, Y, ld_y, Pf, uf, hg, alpha)
        ctx.u_shape = u.shape
        ctx.mark_non_differentiable(alpha)
        return hg, alpha

    @staticmethod
    def backward(ctx, d_hg, _d_alpha):
        csr, pos = ctx.csr, ctx.pos
        h, ld_h, Y, ld_y, Pf, uf, hg, alpha = ctx.misc
        G, (N, D), A, vocab = csr.n_graphs, h.shape, Y.shape[1], Pf.shape[0]
        d_hg, ld_dhg = _rows(d_hg)
        d_h, d_Y = _empty((N, D), h), _empty((N, A), h)
        if G == 0 or N == 0:                                # nothing is launched: the parameters' gradients are zero
            return None, d_h, d_Y, None, torch.zeros_like(Pf), torch.zeros_like(uf).reshape(ctx.u_shape)
        d_P, d_u = torch.empty_like(Pf), torch.empty_like(uf)
        with _lib.on_device(h.device):
            wsb = pure("txe_readout_attn_bwd_ws_bytes", G, A, vocab)
            ws = _ws(wsb, h)
            call("txe_readout_attn_bwd", ptr(csr.graph_off), G, ptr(h), ld_h, D, ptr(Y), ld_y, A, ptr(pos), ptr(Pf), vocab, ptr(uf),
                 ptr(hg), ptr(alpha), ptr(d_hg), ld_dhg, ptr(d_h), D, ptr(d_Y), A, ptr(d_P), ptr(d_u), ptr(ws), wsb, _lib.stream_ptr())
        return None, d_h, d_Y, None, d_P, d_u.reshape(ctx.u_shape)


class LinearFunction(torch.autograd.Function):
    """y = act([x1 | x2] W^T + b): nn.Linear over a virtual concat (the MLP matcher, model_zoo.py:285-298); act 0/1 relu/2 tanh"""

    @staticmethod
    def forward(ctx, x1, x2, W, b, act):
        _need_cuda(x1, x2, W, b)
        x1, ld1 = _rows(x1)
        l = x1.shape[1]
        if x2 is not None:
            x2, ld2 = _rows(x2)
            r = x2.shape[1]
        else:
            ld2, r = 0, 0
        Wf, bf = _f32(W), _f32(b)
        G, O = x1.shape[0], Wf.shape[0]
        y = _empty((G, O), x1)
        with _lib.on_device(x1.device):
            call("txe_linear_fwd", ptr(x1), ld1, l, ptr(x2), ld2, r, G, ptr(Wf), ptr(bf), O, int(act), ptr(y), _lib.stream_ptr())
        ctx.misc = (x1, ld1, l, x2, ld2, r, Wf, bf is not None, int(act), y)
        ctx.req = (ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return y

    @staticmethod
    def backward(ctx, dy):
        x1, ld1, l, x2, ld2, r, Wf, has_b, act, y = ctx.misc
        dy = _f32(dy)
        G, O = y.shape
        need1, need2 = ctx.req
        dx1 = _empty((G, l), y) if (need1 or need2) else None
        dx2 = _empty((G, r), y) if (need2 and x2 is not None) else None
        dW = torch.empty_like(Wf)
        db = _empty((O,), y) if has_b else None
        with _lib.on_device(y.device):
            wsb = pure("txe_linear_bwd_ws_bytes", G, l, r, O)
            ws = _ws(wsb, y)
            call("txe_linear_bwd", ptr(x1), ld1, l, ptr(x2), ld2, r, G, ptr(Wf), O, act, ptr(y), ptr(dy), ptr(dx1), l, ptr(dx2), r, ptr(dW),
                 ptr(db), ptr(ws), wsb, _lib.stream_ptr())
        return (dx1 if need1 else None), (dx2 if need2 else None), dW, db, None


# ================================================================================================================
# Bilinear match (BIM / LBM) -- pairwise form of training, model.py:86
# ================================================================================================================
class QueryPrefetch:
    """bilinear_query_prefetch's token: V [G, l] = e2 W^T, the tensors it was asked for with their versions at that moment, the second
    stream (`stream`: where V is written once launched there, else None) and the operands of the launch"""
    __slots__ = ("V", "e2", "e2_version", "W", "W_version", "stream", "launched", "e2c", "ld2", "Wf", "side")

    def __init__(self, e2, W, e2c, ld2, Wf, V, side):
        self.V, self.e2, self.e2_version, self.W, self.W_version = V, e2, e2._version, W, W._version
        self.e2c, self.ld2, self.Wf, self.side = e2c, ld2, Wf, side
        self.stream, self.launched = side, False

    def matches(self, e2, W, G, l):
        """is V still the projection of these very tensors, unwritten since, for G pairs of l columns?"""
        return (self.e2 is e2 and self.e2_version == e2._version and self.W is W and self.W_version == W._version
                and tuple(self.V.shape) == (G, l))

    def launch(self, on_side=True):
        if self.launched:
            return
        self.launched = True
        V, e2c, Wf, side, device = self.V, self.e2c, self.Wf, self.side, self.e2.device
        if on_side:
            _order(torch.cuda.current_stream(device), side)
        with _lib.on_device(device), torch.cuda.stream(side if on_side else torch.cuda.current_stream(device)):
            call("txe_bilinear_query_project", ptr(e2c), self.ld2, V.shape[0], V.shape[1], e2c.shape[1], ptr(Wf), ptr(V), _lib.stream_ptr())
        if on_side:
            # V was allocated on the caller's stream and is written on the second one: tell the caching allocator, so that a token
            # that is never consumed (rejected by forward, an exception in between) cannot hand V's block to a main-stream tensor
            # while the projection is still writing it; the same for the operands it reads
            for t in (V, e2c, Wf):
                t.record_stream(side)
        self.stream = side if on_side else None


def bilinear_query_prefetch(e2, W):
    """V = e2 W^T of the query-side match (BilinearPairFunction), launched on the second stream: it depends on the queries and the
    matcher's weight only, so it can run under the encoder (TaxoExpan.forward calls this before graph_propagate).  Returns a token for
    BilinearPairFunction.apply(..., pre=token); None when there is nothing to gain (gradient wanted for e2, CPU tensors, no side stream)."""
    if _NO_SIDE_STREAM or not (torch.is_tensor(e2) and e2.is_cuda and W.is_cuda) or e2.requires_grad or e2.dim() != 2 or e2.shape[0] == 0:
        return None
    e2c, ld2 = _rows(e2)
    Wf = _f32(W).reshape(W.shape[-2], W.shape[-1])
    tok = QueryPrefetch(e2, W, e2c, ld2, Wf, _empty((e2c.shape[0], Wf.shape[0]), e2c), _side_stream(e2.device))
    # launched by the encoder behind its first projection GEMM (_launch_pending_prefetch): started at the very beginning its workgroups
    # take slots before the persistent first-layer projection's, whose late starters then finish late
    del _pending_prefetch[:]                    # (a token nobody launched holds no device work: dropping it is safe)
    _pending_prefetch.append(tok)
    return tok


_pending_prefetch = []


def _launch_pending_prefetch():
    while _pending_prefetch:
        _pending_prefetch.pop().launch()


class BilinearPairFunction(torch.autograd.Function):
    """s_i = e1_i^T W e2_i (exp optionally).  When e2 needs no gradient (queries: always so in training) the query-side form runs:
    V = e2 W^T in forward makes backward's d_e1 = dsl * V elementwise (txe_bilinear_query_*); otherwise the candidate-side form
    U = e1 W with gradients to both inputs (txe_bilinear_pair_*).  pre: a bilinear_query_prefetch token whose V is used if it still
    matches e2 / W."""

    @staticmethod
    def forward(ctx, e1, e2, W, apply_exp, pre=None):
        _need_cuda(e1, e2, W)
        e1, ld1 = _rows(e1)
        e2_in = e2
        e2, ld2 = _rows(e2)
        Wf = _f32(W).reshape(W.shape[-2], W.shape[-1])
        G, l = e1.shape
        r = e2.shape[1]
        s = _empty((G,), e1)
        query_side = not ctx.needs_input_grad[1]
        with _lib.on_device(e1.device):
            if query_side:
                if pre is not None and pre.matches(e2_in, W, G, l):
                    U = pre.V
                    pre.launch(on_side=False)                    # (nobody started it: in line, on this stream)
                    if pre.stream is not None:
                        _order(pre.stream, torch.cuda.current_stream())
                    call("txe_bilinear_query_dot", ptr(e1), ld1, ptr(U), G, l, int(apply_exp), ptr(s), _lib.stream_ptr())
                else:
                    U = _empty((max(G, 1), l), e1)          # V = e2 W^T
                    call("txe_bilinear_query_fwd", ptr(e1), ld1, ptr(e2), ld2, G, l, r, ptr(Wf), int(apply_exp), ptr(U), ptr(s), _lib.stream_ptr())
            else:
                U = _empty((max(G, 1), r), e1)
                call("txe_bilinear_pair_fwd", ptr(e1), ld1, ptr(e2), ld2, G, l, r, ptr(Wf), int(apply_exp), ptr(U), ptr(s),
                     _lib.stream_ptr())
        ctx.misc = (e1, ld1, e2, ld2, Wf, U, s, int(apply_exp), W.shape, query_side)
        return s.unsqueeze(1)

    @staticmethod
    def backward(ctx, ds):
        e1, ld1, e2, ld2, Wf, U, s, apply_exp, wshape, query_side = ctx.misc
        G, l = e1.shape
        r = e2.shape[1]
        ds = _f32(ds.reshape(-1))
        d_e1 = _empty((G, l), e1)
        dW = torch.empty_like(Wf)
        with _lib.on_device(e1.device):
            if query_side:
                wsb = pure("txe_bilinear_query_bwd_ws_bytes", G, l, r)
                ws = _ws(wsb, e1)
                call("txe_bilinear_query_bwd", ptr(e1), ld1, ptr(e2), ld2, G, l, r, apply_exp, ptr(U), ptr(s), ptr(ds), ptr(d_e1), l, ptr(dW),
                     ptr(ws), wsb, _lib.stream_ptr())
                return d_e1, None, dW.reshape(wshape), None, None
            d_e2 = _empty((G, r), e1)
            wsb = pure("txe_bilinear_pair_bwd_ws_bytes", G, l, r)
            ws = _ws(wsb, e1)
            call("txe_bilinear_pair_bwd", ptr(e1), ld1, ptr(e2), ld2, G, l, r, ptr(Wf), apply_exp, ptr(U), ptr(s), ptr(ds), ptr(d_e1),
                 l, ptr(d_e2), r, ptr(dW), ptr(ws), wsb, _lib.stream_ptr())
        return d_e1, d_e2, dW.reshape(wshape), None, None


class RepeatedRows:
    """A [G, r] matrix whose rows repeat in RUNS, kept as its U distinct rows: the query features of a training batch -- one query is
    paired with 1 + negative_size consecutive anchors and the reference's collate stacks its row once per pair (data_loaders.py:9-28).
    rows [U, r] (device), run_off [U + 1] int32 (device; first pair of every run, run_off[U] = G).  BIM / LBM take it as their query
    argument and project U rows instead of G (BilinearRunsFunction); every other consumer calls dense().  data_loaders.DeviceBatchLoader
    yields it as the query features (repeated_queries=True)."""

    def __init__(self, rows, run_off, n_rows):
        self.rows, self.run_off, self.n_rows = rows, run_off, int(n_rows)
        assert run_off.dtype == torch.int32 and run_off.numel() == rows.shape[0] + 1

    @staticmethod
    def from_ids(table, ids, device=None):
        """table[ids] with the runs of equal consecutive ids found on the host (ids: host int array)"""
        import numpy as np
        ids = np.asarray(ids).reshape(-1)
        start = np.flatnonzero(np.concatenate([[True], ids[1:] != ids[:-1]])) if ids.size else np.zeros(0, dtype=np.int64)
        dev = table.device if device is None else device
        off = torch.from_numpy(np.concatenate([start, [ids.size]]).astype(np.int32)).to(dev)
        return RepeatedRows(table.index_select(0, torch.from_numpy(ids[start].astype(np.int64)).to(table.device)).to(dev), off, ids.size)

    shape = property(lambda self: (self.n_rows, self.rows.shape[1]))
    device = property(lambda self: self.rows.device)
    dtype = property(lambda self: self.rows.dtype)
    requires_grad = property(lambda self: self.rows.requires_grad)

    def dim(self):
        return 2

    def dense(self):
        # rows on the device that ask for a gradient (a trainable feature table's leaves): their gradient is a fixed-order run sum
        if self.rows.requires_grad and self.rows.is_cuda and torch.is_grad_enabled():
            return RepeatRowsFunction.apply(self.rows, self.run_off, self.n_rows)
        cnt = (self.run_off[1:] - self.run_off[:-1]).long()
        return self.rows.repeat_interleave(cnt, dim=0, output_size=self.n_rows)

    def to(self, device):
        rows = self.rows.to(device)
        return RepeatedRows(rows, self.run_off.to(rows.device), self.n_rows)


class RepeatRowsFunction(torch.autograd.Function):
    """RepeatedRows.dense() for rows that ask for a gradient (feature_table.FeatureTable: the distinct query rows are leaves).  Forward is
    the repeat_interleave that dense() always was, the same bits; backward sums each run's pair gradients left to right in one launch
    (txe_rows_run_sum) -- repeat_interleave's own backward is an index_add_ with floating-point atomics, whose order changes from run
    to run."""

    @staticmethod
    def forward(ctx, rows, run_off, n_rows):
        _need_cuda(rows)
        ctx.run_off, ctx.shape = run_off, rows.shape
        cnt = (run_off[1:] - run_off[:-1]).long()
        return rows.repeat_interleave(cnt, dim=0, output_size=n_rows)

    @staticmethod
    def backward(ctx, d_out):
        d_out, ld = _rows(_f32(d_out))
        U, r = ctx.shape
        d_rows = _empty((U, r), d_out)
        with _lib.on_device(d_out.device):
            call("txe_rows_run_sum", ptr(d_out), ld, ptr(ctx.run_off), U, d_out.shape[0], r, ptr(d_rows), r, _lib.stream_ptr())
        return d_rows, None, None


def dense_rows(x):
    """a plain tensor from a tensor or a RepeatedRows"""
    return x.dense() if isinstance(x, RepeatedRows) else x


class BilinearRunsFunction(torch.autograd.Function):
    """s_i = e1_i^T W q_i (exp optionally) for queries given as RepeatedRows: V = rows W^T has U rows, backward's weight gradient
    sums a run's pairs first (txe_bilinear_runs_*).  No gradient to the queries."""

    @staticmethod
    def forward(ctx, e1, W, apply_exp, rows, run_off):
        _need_cuda(e1, rows, W)
        e1, ld1 = _rows(e1)
        rows, ldq = _rows(rows)
        Wf = _f32(W).reshape(W.shape[-2], W.shape[-1])
        G, l = e1.shape
        U, r = rows.shape
        s = _empty((G,), e1)
        V = _empty((max(U, 1), l), e1)
        with _lib.on_device(e1.device):
            call("txe_bilinear_runs_fwd", ptr(e1), ld1, ptr(rows), ldq, ptr(run_off), G, U, l, r, ptr(Wf), int(apply_exp), ptr(V), ptr(s),
                 _lib.stream_ptr())
        ctx.misc = (e1, ld1, rows, ldq, run_off, V, s, int(apply_exp), W.shape)
        return s.unsqueeze(1)

    @staticmethod
    def backward(ctx, ds):
        e1, ld1, rows, ldq, run_off, V, s, apply_exp, wshape = ctx.misc
        G, l = e1.shape
        U, r = rows.shape
        ds = _f32(ds.reshape(-1))
        d_e1 = _empty((G, l), e1)
        dW = _empty((l, r), e1)
        with _lib.on_device(e1.device):
            wsb = pure("txe_bilinear_runs_bwd_ws_bytes", U, l, r)
            ws = _ws(wsb, e1)
            call("txe_bilinear_runs_bwd", ptr(e1), ld1, ptr(rows), ldq, ptr(run_off), G, U, l, r, apply_exp, ptr(V), ptr(s), ptr(ds), ptr(d_e1), l,
                 ptr(dW), ptr(ws), wsb, _lib.stream_ptr())
        return d_e1, dW.reshape(wshape), None, None, None


def find_row_runs(e2):
    """runs of equal consecutive rows of the stacked query matrix e2 [G, r], found on the device (txe_rows_find_runs): returns
    (run_id [G], run_off [G + 1], n_runs [1]) int32 device tensors -- no host synchronisation"""
    _need_cuda(e2)
    e2c, ld2 = _rows(e2)
    G, r = e2c.shape
    run_id = torch.empty(max(G, 1), dtype=torch.int32, device=e2.device)
    run_off = torch.empty(G + 1, dtype=torch.int32, device=e2.device)
    n_runs = torch.empty(1, dtype=torch.int32, device=e2.device)
    with _lib.on_device(e2.device):
        call("txe_rows_find_runs", ptr(e2c), ld2, G, r, ptr(run_id), ptr(run_off), ptr(n_runs), _lib.stream_ptr())
    return run_id, run_off, n_runs


class BilinearStackedRunsFunction(torch.autograd.Function):
    """BilinearRunsFunction on the reference collate's STACKED query matrix (one row per pair): the runs of equal consecutive rows are
    found on the device in every call (bit-wise row comparison + a scan, no host synchronisation) and the products run on one row per
    run (txe_bilinear_stacked_*).  Right for any e2; the caller (model_zoo._Bilinear) takes this form when its first training batch
    showed that rows repeat.  No gradient to the queries."""

    @staticmethod
    def forward(ctx, e1, e2, W, apply_exp):
        _need_cuda(e1, e2, W)
        e1, ld1 = _rows(e1)
        e2, ld2 = _rows(e2)
        Wf = _f32(W).reshape(W.shape[-2], W.shape[-1])
        G, l = e1.shape
        r = e2.shape[1]
        _run_id, run_off, n_runs = find_row_runs(e2)
        s = _empty((G,), e1)
        V = _empty((max(G, 1), l), e1)                        # (sized for G runs; the batch's runs fill the first rows)
        with _lib.on_device(e1.device):
            call("txe_bilinear_stacked_fwd", ptr(e1), ld1, ptr(e2), ld2, ptr(run_off), ptr(n_runs), G, l, r, ptr(Wf), int(apply_exp), ptr(V),
                 ptr(s), _lib.stream_ptr())
        ctx.misc = (e1, ld1, e2, ld2, run_off, n_runs, V, s, int(apply_exp), W.shape)
        return s.unsqueeze(1)

    @staticmethod
    def backward(ctx, ds):
        e1, ld1, e2, ld2, run_off, n_runs, V, s, apply_exp, wshape = ctx.misc
        G, l = e1.shape
        r = e2.shape[1]
        ds = _f32(ds.reshape(-1))
        d_e1 = _empty((G, l), e1)
        dW = _empty((l, r), e1)
        with _lib.on_device(e1.device):
            wsb = pure("txe_bilinear_stacked_bwd_ws_bytes", G, l, r)
            ws = _ws(wsb, e1)
            call("txe_bilinear_stacked_bwd", ptr(e1), ld1, ptr(e2), ld2, ptr(run_off), ptr(n_runs), G, l, r, apply_exp, ptr(V), ptr(s), ptr(ds),
                 ptr(d_e1), l, ptr(dW), ptr(ws), wsb, _lib.stream_ptr())
        return d_e1, None, dW.reshape(wshape), None


def _plain_gemm(layout, A, lda, B, ldb, C, ldc, M, N, K):
    """txe_gemm_plain on the route the model paths take (route 0, no k-splits), with the stream's tail-splitting scratch"""
    tws = _tail_ws(C)
    call("txe_gemm_plain", layout, ptr(A), lda, ptr(B), ldb, ptr(C), ldc, M, N, K, 1, 0, ptr(tws), tws.numel(), _lib.stream_ptr())


class InBatchNCEFunction(torch.autograd.Function):
    """The in-batch loss of a training batch: every one of the Q queries against every one of the batch's G graph vectors,
    masked by the taxonomy (txe_inbatch_nce).  hg [G, l] (materialised), W [1, l, r], queries [Q, r] (one row per query), groups: a
    sampler.InBatchGroups of the same Q and G.  Forward: V = q W^T, B = V hg^T (txe_gemm_plain, layout 0), exp in place for LBM
    (txe_inbatch_exp), then the loss launch, which leaves the gradient to B in place of the scores.  Backward: d_hg = dB^T V, dV = dB hg,
    dW = dV^T q (layouts 2, 1, 2).  No gradient to the queries, unless query_grad=True (a trainable feature table: d_q = dV W, layout 1;
    without it queries that ask for a gradient are refused).  valid_total: None, or an int64 [1] device counter that gains the
    batch's valid (query, column) pairs.  Returns the sum-reduced fp32 loss (a 0-dim tensor)."""

    @staticmethod
    def forward(ctx, hg, W, queries, apply_exp, groups, valid_total=None, query_grad=False):
        _need_cuda(hg, W, queries)
        if queries.requires_grad and not query_grad:
            raise ValueError("InBatchNCEFunction: the queries are taxonomy features and get no gradient (detach them, or pass "
                             "query_grad=True when the feature table trains)")
        hg, ldh = _rows(hg)
        q, ldq = _rows(queries)
        Wf = _f32(W).reshape(W.shape[-2], W.shape[-1])
        (G, l), (Q, r) = hg.shape, q.shape
        if Wf.shape != (l, r):
            raise ValueError(f"InBatchNCEFunction: W {tuple(W.shape)} does not match hg [{G}, {l}] and queries [{Q}, {r}]")
        if (groups.Q, groups.G) != (Q, G):
            raise ValueError(f"InBatchNCEFunction: the groups describe {groups.Q} queries x {groups.G} columns, the batch has {Q} x {G}")
        if groups.anchor.device != hg.device:
            raise ValueError("InBatchNCEFunction: the groups live on another device")
        if G < 1 or Q * G >= 2 ** 31:
            raise ValueError(f"InBatchNCEFunction: needs G >= 1 and Q * G < 2^31, got Q = {Q}, G = {G}")
        if valid_total is not None and not (valid_total.dtype == torch.int64 and valid_total.numel() == 1 and valid_total.device == hg.device):
            raise ValueError("InBatchNCEFunction: valid_total is one int64 element on the batch's device")
        loss = _empty((), hg)
        ctx.misc = None
        with _lib.on_device(hg.device):
            if Q == 0:                                        # an empty sum: nothing to launch, no gradient
                return loss.zero_()
            V, B = _empty((Q, l), hg), _empty((Q, G), hg)
            _plain_gemm(0, q, ldq, Wf, r, V, l, Q, l, r)
            _plain_gemm(0, V, l, hg, ldh, B, G, Q, G, l)
            if apply_exp:
                call("txe_inbatch_exp", ptr(B), G, Q, G, _lib.stream_ptr())
            wsb = pure("txe_inbatch_nce_ws_bytes", Q)
            ws = _ws(wsb, hg)
            call("txe_inbatch_nce", ptr(B), G, Q, G, ptr(groups.pos_col), ptr(groups.anchor), ptr(groups.qnode), ptr(groups.mask_ptr),
                 ptr(groups.mask_idx), int(bool(apply_exp)), ptr(loss), ptr(B), G, None, ptr(valid_total), ptr(ws), wsb, _lib.stream_ptr())
        ctx.misc = (hg, ldh, q, ldq, V, B, W.shape, Wf)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        if ctx.misc is None:
            return None, None, None, None, None, None, None
        from .loss import _scaled
        hg, ldh, q, ldq, V, dB, wshape, Wf = ctx.misc
        (G, l), (Q, r) = hg.shape, q.shape
        dB = _scaled(dB, grad_loss)
        d_hg = dW = d_q = None
        with _lib.on_device(hg.device):
            if ctx.needs_input_grad[0]:
                d_hg = _empty((G, l), hg)
                _plain_gemm(2, dB, G, V, l, d_hg, l, G, l, Q)
            if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
                dV = _empty((Q, l), hg)
                _plain_gemm(1, dB, G, hg, ldh, dV, l, Q, l, G)
            if ctx.needs_input_grad[1]:
                dW = _empty((l, r), hg)
                _plain_gemm(2, dV, l, q, ldq, dW, r, l, r, Q)
                dW = dW.reshape(wshape)
            if ctx.needs_input_grad[2]:                       # (query_grad=True: forward refuses otherwise) d_q = dV W
                d_q = _empty((Q, r), hg)
                _plain_gemm(1, dV, l, Wf, r, d_q, r, Q, r, l)
        return d_hg, dW, d_q, None, None, None, None


def gcn_folded_graph_vector_ok(csr, cfg, params):
    """may a GCN stack hand out Z instead of hg (cfg.final = 'collapse_z')?  The output layer's bias then rides as one more weight row
    behind a column of Z that counts as 1: its input width must leave a padding column ((Kin) % 32 != 0)."""
    if _NO_MATCH_FOLD or csr.n_edges <= 0 or csr.n_graphs <= 0 or csr.n_nodes <= 0:
        return False
    W, b = params[-3], params[-2]
    return b is None or (W.shape[0] % 32) != 0


def folded_graph_vector_ok(csr, cfg):
    """may a GAT stack hand out Z instead of hg (cfg.final = 'collapse_z')?  Needs the fused backward of the folded layer (the only one
    that takes dZ): at least two layers, the shapes txe_gat_fused_bwd_supported covers, edges, and the default routes."""
    if _NO_MATCH_FOLD or _NO_FUSED_BWD or cfg.n_layers < 2 or cfg.heads[-1] != 1 or csr.n_edges <= 0 or csr.n_graphs <= 0 or csr.n_nodes <= 0:
        return False
    kh = cfg.heads[-2] * cfg.out_dims[-2]
    return pure("txe_gat_fused_bwd_supported", kh, cfg.pos_dims[-1], cfg.heads[-2], cfg.out_dims[-2]) == 1


def folded_graph_linear(Z, Wp, D, link=None):
    """hg [G, D] = Z [G, Kp] Wp[:D]^T (link.by_k: Z Wp[:, :D] + bias), outside autograd (DeferredGraphVector.detach)"""
    _need_cuda(Z, Wp)
    G, Kp = Z.shape
    hg = _empty((G, D), Z)
    with _lib.on_device(Z.device):
        tws = _tail_ws(Z)
        if link is not None and link.by_k:          # a GCN layer's packing: hg = Z Wp[:Kp, :D] + bias (row one_col; Z's column there is 0)
            call("txe_gemm_plain", 1, ptr(Z), Kp, ptr(Wp), Wp.stride(0), ptr(hg), D, G, D, Kp, 1, 0, ptr(tws), tws.numel(), _lib.stream_ptr())
            if link.one_col >= 0:
                hg += Wp[link.one_col, :D]
        else:
            call("txe_gemm_plain", 0, ptr(Z), Kp, ptr(Wp), Kp, ptr(hg), D, G, D, Kp, 1, 0, ptr(tws), tws.numel(), _lib.stream_ptr())
    return hg


class FoldedGraphLinearFunction(torch.autograd.Function):
    """hg [G, D] = Z [G, Kp] Wp[:D]^T -- the graph vector of a 'collapse_z' stack materialised after all (some consumer other than the
    bilinear run matcher wants the tensor).  Backward: dZ = d_hg Wp[:D] through autograd, the weight gradient's main part d_hg^T Z as
    split-K slices through the FoldLink (the stack's backward finishes dW)."""

    @staticmethod
    def forward(ctx, Z, Wp, link, D):
        _need_cuda(Z, Wp)
        G, Kp = Z.shape
        hg = folded_graph_linear(Z, Wp, D, link)
        note_route("fold", "materialised")
        ctx.misc = (Z, Wp, link, D)
        return hg

    @staticmethod
    def backward(ctx, d_hg):
        Z, Wp, link, D = ctx.misc
        G, Kp = Z.shape
        d_hg, ld = _rows(_f32(d_hg))
        dZ = _empty((G, Kp), Z)
        if link.by_k:                               # dZ = d_hg Wp[:, :D]^T;  part [Kp][D] = Z^T d_hg, row one_col = d_bias = column sums of d_hg
            part = _empty((Kp, D), Z)
            with _lib.on_device(Z.device):
                tws = _tail_ws(Z)
                call("txe_gemm_plain", 0, ptr(d_hg), ld, ptr(Wp), Wp.stride(0), ptr(dZ), Kp, G, Kp, D, 1, 0, ptr(tws), tws.numel(), _lib.stream_ptr())
                call("txe_gemm_plain", 2, ptr(Z), Kp, ptr(d_hg), ld, ptr(part), D, Kp, D, G, 1, 0, None, 0, _lib.stream_ptr())
            if link.one_col >= 0:
                part[link.one_col] = d_hg.sum(0)
            link.part, link.S = part, 1
            return dZ, None, None, None
        S = max(1, min(8, G // 512))
        part = _empty((S * D, Kp), Z)
        with _lib.on_device(Z.device):
            tws = _tail_ws(Z)
            call("txe_gemm_plain", 1, ptr(d_hg), ld, ptr(Wp), Kp, ptr(dZ), Kp, G, Kp, D, 1, 0, ptr(tws), tws.numel(), _lib.stream_ptr())
            call("txe_gemm_plain", 2, ptr(d_hg), ld, ptr(Z), Kp, ptr(part), Kp, D, Kp, G, S, 0, None, 0, _lib.stream_ptr())
        link.part, link.S = part, S
        return dZ, None, None, None


def folded_match_job(e2, rows, run_off, Wm):
    """What a 'collapse_z' stack calls right before its Z sweep (cfg.fold_job): the query-side half of BilinearFoldedRunsFunction -- the
    runs (found on the device in the stacked e2, or given as rows + run_off), V = Wm q, T = Wp[:D]^T V and the graph -> run map -- on the
    caller's stream.  T then rides in the sweep (FoldLink.e_part) and the matcher's forward starts from the scores."""
    def job(Wp, D):
        Wmf = _f32(Wm).reshape(Wm.shape[-2], Wm.shape[-1])
        l, r = Wmf.shape
        if l != D or not Wm.is_cuda:
            return None
        Kp = Wp.shape[1]
        with _lib.on_device(Wp.device):
            if rows is None:
                Q, ldq = _rows(e2)
                G = U = Q.shape[0]
                run_id, roff, n_runs = find_row_runs(Q)
                first_row = 1
            else:
                Q, ldq = _rows(rows)
                U, first_row, roff, n_runs = Q.shape[0], 0, run_off, None
                G = None
            V, T = _empty((max(U, 1), l), Wp), _empty((max(U, 1), Kp), Wp)
            call("txe_bilinear_folded_fwd", None, Kp, G if G is not None else 1, Kp, ptr(Wp), Kp, l, ptr(Q), ldq, r, ptr(roff), ptr(n_runs), U, first_row,
                 ptr(Wmf), 0, ptr(V), ptr(T), None, 1, 0, -1, _lib.stream_ptr())
        return FoldJob(e2, rows, run_off, Wm, Wp, Q, ldq, roff, n_runs, U, first_row, V, T, run_id if rows is None else None)
    return job


class FoldScore(typing.NamedTuple):
    """what txe_gat_collapse_fold_scores needs to sum the matcher's scores from FoldLink.e_part, left by the stack whose Z sweep filled it:
    graph offsets, nodes, graphs, the folded layer's Kh / Pd, the readout's coef [N] / wsum [G], the feature dropout and whether it is on"""
    graph_off: torch.Tensor
    N: int
    G: int
    Kh: int
    Pd: int
    coef: torch.Tensor
    wsum: torch.Tensor
    feat_p: float
    masked: int


class FoldJob:
    """what folded_match_job's callable has formed: the tensors it was built for (queries e2 or rows + run_off, the matcher's Wm and its
    version, the output layer's Wp) and the query-side half of BilinearFoldedRunsFunction.forward -- Q / ldq, run offsets roff, n_runs, U
    runs, first_row, V [U, l], T [U, Kp], graph -> run map run_id; score: the FoldScore of the Z sweep that carried T, else None"""
    __slots__ = ("e2", "rows", "run_off", "Wm", "Wm_version", "Wp", "Q", "ldq", "roff", "n_runs", "U", "first_row", "V", "T", "run_id", "score")

    def __init__(self, e2, rows, run_off, Wm, Wp, Q, ldq, roff, n_runs, U, first_row, V, T, run_id):
        self.e2, self.rows, self.run_off, self.Wm, self.Wm_version, self.Wp = e2, rows, run_off, Wm, Wm._version, Wp
        self.Q, self.ldq, self.roff, self.n_runs, self.U, self.first_row, self.V, self.T = Q, ldq, roff, n_runs, U, first_row, V, T
        self.run_id, self.score = run_id, None

    def matches(self, Wp, Wm, e2, rows, run_off, G):
        """was the job run for these very tensors, Wm unwritten since (and, runs found in the stacked e2, for G rows)?"""
        return (self.Wp is Wp and self.Wm is Wm and self.Wm_version == Wm._version and self.e2 is e2
                and self.rows is rows and self.run_off is run_off and (rows is not None or self.U == G))

    def run_ids(self, G):
        """graph -> run for the given-runs form (the stacked form's run detection has produced it)"""
        if self.run_id is None:
            self.run_id = torch.empty(max(G, 1), dtype=torch.int32, device=self.T.device)
            call("txe_runs_expand", ptr(self.roff), self.U, G, ptr(self.run_id), _lib.stream_ptr())
        return self.run_id


class BilinearFoldedRunsFunction(torch.autograd.Function):
    """The bilinear match on the folded graph vector (txe_bilinear_folded_*): s_i = <Z_i, T[u(i)]>, T[u] = Wp[:D]^T (Wm q_u) -- the output
    layer's D x Kp product runs on the U run rows of the repeating queries instead of the G graph rows, forward and backward.  Queries:
    the stacked matrix e2 [G, r] (runs found on the device, rows = run_off = None) or the U distinct rows + run offsets.  Gradients: dZ
    (to the stack through autograd), the main part of the output layer's dW (through the FoldLink), dWm.  None to the queries."""

    @staticmethod
    def forward(ctx, Z, Wp, link, D, Wm, apply_exp, e2, rows, run_off):
        _need_cuda(Z, Wp, Wm)
        G, Kp = Z.shape
        Wmf = _f32(Wm).reshape(Wm.shape[-2], Wm.shape[-1])
        l, r = Wmf.shape
        if l != D:
            raise RuntimeError("bilinear matcher: l_dim does not match the graph vector")
        job = link.fwd
        ready = job is not None and job.matches(Wp, Wm, e2, rows, run_off, G)
        if ready:                                   # the stack asked for the runs, V and T before its Z sweep (folded_match_job)
            Q, ldq, run_off, n_runs, U, first_row, V, T = job.Q, job.ldq, job.roff, job.n_runs, job.U, job.first_row, job.V, job.T
        else:
            link.fwd = link.e_part = None           # (whatever rode in the sweep belongs to other queries / weights)
            if rows is None:
                Q, ldq = _rows(e2)
                _run_id, run_off, n_runs = find_row_runs(Q)
                U, first_row = G, 1
            else:
                Q, ldq = _rows(rows)
                n_runs, U, first_row = None, Q.shape[0], 0
            V, T = _empty((max(U, 1), l), Z), _empty((max(U, 1), Kp), Z)
        s = _empty((G,), Z)
        # 'edot': the stack ran the matcher's job and its Z sweep carried T; 'job': it ran the job only; 'inline': V / T formed here
        edot = ready and link.carried_T
        note_route("fold", "edot" if edot else ("job" if ready else "inline"))
        with _lib.on_device(Z.device):
            if edot:
                # T rode in the stack's Z sweep: the scores are sums of its per-node dot products over each graph's few nodes, no sweep over Z
                sc = job.score
                call("txe_gat_collapse_fold_scores", ptr(sc.graph_off), sc.N, sc.G, sc.Kh, sc.Pd, ptr(sc.coef), ptr(sc.wsum), ptr(link.e_part),
                     sc.feat_p, sc.masked, int(apply_exp), ptr(s), _lib.stream_ptr())
            else:
                call("txe_bilinear_folded_fwd", ptr(Z), Kp, G, Kp, ptr(Wp), Wp.stride(0), l, ptr(Q), ldq, r, ptr(run_off), ptr(n_runs), U, first_row,
                     ptr(Wmf), int(apply_exp), ptr(V), ptr(T), ptr(s), 2 if ready else 3, int(link.by_k), int(link.one_col), _lib.stream_ptr())
        ctx.misc = (Z, Wp, link, Wmf, Q, ldq, run_off, n_runs, U, first_row, V, T, s, int(apply_exp), Wm.shape)
        return s.unsqueeze(1)

    @staticmethod
    def backward(ctx, ds):
        Z, Wp, link, Wmf, Q, ldq, run_off, n_runs, U, first_row, V, T, s, apply_exp, wshape = ctx.misc
        G, Kp = Z.shape
        l, r = Wmf.shape
        ds = _f32(ds.reshape(-1))
        edot = link.carried_T                       # the stack reads "dZ[g]" as dsl_g T[run(g)] (FoldLink): no dZ tensor exists
        dZ = None if edot else _empty((G, Kp), Z)
        dT, dV = _empty((max(U, 1), Kp), Z), _empty((max(U, 1), l), Z)
        dWm, dWf = _empty((l, r), Z), (_empty((Kp, l), Z) if link.by_k else _empty((l, Kp), Z))
        with _lib.on_device(Z.device):
            call("txe_bilinear_folded_bwd", ptr(Z), Kp, G, Kp, ptr(Wp), Wp.stride(0), l, ptr(Q), ldq, r, ptr(run_off), ptr(n_runs), U, first_row, apply_exp,
                 ptr(V), ptr(T), ptr(s), ptr(ds), ptr(dZ), Kp, ptr(dT), ptr(dV), ptr(dWm), ptr(dWf), int(link.by_k), int(link.one_col),
                 _lib.stream_ptr())
        link.part, link.S = dWf, 1
        link.ds, link.s, link.apply_exp = (ds, s, apply_exp) if edot else (None, None, 0)
        return dZ, None, None, None, dWm.reshape(wshape), None, None, None, None


# ================================================================================================================
# inference-side helpers (no autograd)
# ================================================================================================================
class BilinearPrepared:
    """the candidate side of a BIM / LBM matcher, once per candidate set: full [max(G, 1), rp] = hg W with every row zero-padded to rp
    columns (U = full[:G, :r]); planes = its packed bf16 planes for the split route, or None (the C side then packs per call); version
    = full._version when they were packed -- a later in-place write to U leaves them stale, and _planes() stops handing them out"""
    __slots__ = ("full", "G", "r", "rp", "planes", "version", "__weakref__")

    def __init__(self, full, G, r, rp, planes, version):
        self.full, self.G, self.r, self.rp, self.planes, self.version = full, G, r, rp, planes, version

    @property
    def U(self):
        return self.full[:self.G, :self.r]

    def gather(self, idx):
        """the rows idx, gathered WITH their zero padding (a plain U[idx] of r = 250 is a packed copy: 8-byte rows, a ragged last k-tile)"""
        return BilinearPrepared(self.full.index_select(0, idx), int(idx.numel()), self.r, self.rp, None, 0)


def bilinear_prepare(hg, W):
    """U = hg @ W[0]  (G x r): the factored half of the bilinear form, computed once per candidate set.  Returns BilinearPrepared."""
    _need_cuda(hg, W)
    hg, ld = _rows(hg)
    Wf = _f32(W).reshape(W.shape[-2], W.shape[-1])
    G, l = hg.shape
    r = Wf.shape[1]
    # rows zero-padded to a whole number of 32-column k-tiles: the scoring GEMM then runs every k-tile on the plain 16-byte
    # loader (r = 250 would leave a ragged last tile on the generic one); zeros add exactly nothing to the products
    rp = (r + 31) // 32 * 32
    Ufull = _empty((max(G, 1), rp), hg)
    if rp != r:
        # the WEIGHT is padded instead of U: W [l][r] -> [l][rp] with zero columns (0.5 MB), so the product writes U's zero padding
        # itself and reads a 16-byte-aligned operand (rows of 250 floats are only 8-byte aligned: the two-float loader ran this GEMM
        # at 47 TF/s, 130 us of the 0.54-ms MAG-CS scoring pass)
        Wp = torch.zeros((l, rp), dtype=torch.float32, device=hg.device)
        Wp[:, :r].copy_(Wf)
        Wf = Wp
    planes = None
    with _lib.on_device(hg.device):
        swb = 0 if (_NO_SPLIT_GEMM or G < 1) else pure("txe_gemm_plain_split_ws_bytes", G, rp, l)
        sws = _ws(swb, hg) if swb else None
        call("txe_bilinear_project", ptr(hg), ld, G, l, ptr(Wf), rp, ptr(Ufull), rp, ptr(sws), swb, _lib.stream_ptr())
        if not _NO_SPLIT_GEMM and G >= 1:
            # the candidates' bf16 planes for the scoring loop, once per candidate set: the loop over query blocks packs only its queries
            planes = torch.empty(pure("txe_split_packed_bytes", G, rp), dtype=torch.uint8, device=hg.device)
            call("txe_split_pack", ptr(Ufull), rp, G, rp, 1, ptr(planes), _lib.stream_ptr())
    return BilinearPrepared(Ufull, G, r, rp, planes, Ufull._version)


def bilinear_project(hg, W):
    """bilinear_prepare() as the [G, r] tensor U.  The tensor carries its BilinearPrepared (attribute `prepared`): the score_* functions
    find the padded pitch and the planes on this very tensor -- not on a slice, a view or a copy of it.  (U -> prepared -> full and no
    way back: dropping U frees the buffer and the planes at once.)"""
    prep = bilinear_prepare(hg, W)
    U = prep.U
    U.prepared = prep
    return U


def _as_prepared(U):
    """the candidate side of a score_* call: a BilinearPrepared as it is; a tensor's `prepared` if the tensor still is that object's U;
    any other tensor as an unpadded, unpacked candidate set"""
    if isinstance(U, BilinearPrepared):
        return U
    prep = getattr(U, "prepared", None)
    if prep is not None and U.data_ptr() == prep.full.data_ptr() and U.shape == (prep.G, prep.r) and U.stride() == (prep.full.stride(0), 1):
        return prep
    U = _rows(U)[0]
    return BilinearPrepared(U, U.shape[0], U.shape[1], U.shape[1], None, 0)


def _planes(prep, K):
    """the packed planes of prep's rows for a reduction over K columns, or None: they cover the padded width, and they are the rows'
    only while nothing has written to the buffer since the pack"""
    ok = prep.planes is not None and K == prep.rp and prep.full._version == prep.version and not _NO_SPLIT_GEMM
    return prep.planes if ok else None


def gather_padded_rows(U, idx):
    """U[idx] for a bilinear_project output, gathered WITH its zero padding (BilinearPrepared.gather), for positive_scores_staircase"""
    return _as_prepared(U).gather(idx)


def _query_layout(nq, r, ldq, rp, q_padded):
    """what a score kernel's query operand needs: nq queries of r columns on a pitch of ldq floats against candidates whose rows are
    zero-padded to rp columns.  Returns (what to do, the contraction width K, the pitch afterwards).  Every fused route promises the
    bits of every other one: they all take K and the loader (the pitch) from here."""
    if nq > 0 and rp != r:                              # both operands zero-padded to whole k-tiles: K = rp, the plain 16-byte loader
        return ("padded", rp, ldq) if q_padded else ("pad", rp, rp)
    if nq > 0 and ldq % 4 != 0:                         # rows re-laid on a 16-byte pitch (a few hundred KB per block)
        return "relay", r, (r + 3) // 4 * 4
    return "as_is", r, ldq


def _lay_queries(Q, prep, q_padded=False):
    """Q as _query_layout asks: (Q, ldq, K).  q_padded: Q is a row block of pad_queries_like(all queries, U) -- fp32, its columns up
    to the candidates' padded width zeros already; the pointer is taken as it is."""
    if q_padded:
        assert Q.dtype == torch.float32 and Q.dim() == 2 and Q.stride(1) == 1, "q_padded: a row block of pad_queries_like()"
    else:
        Q = _rows(Q)[0]
    nq, r = Q.shape
    assert r == prep.r, "the queries' width != the candidates'"
    how, K, ldq = _query_layout(nq, r, Q.stride(0), prep.rp, q_padded)
    if how == "padded":
        assert ldq == prep.rp, "q_padded: a row block of pad_queries_like()"
    elif how == "pad":
        Qp = torch.zeros((nq, prep.rp), dtype=torch.float32, device=Q.device)
        Qp[:, :r].copy_(Q)
        Q = Qp
    elif how == "relay":
        Qp = _empty((nq, ldq), Q)[:, :r]
        Qp.copy_(Q)
        Q = Qp
    return Q, ldq, K


def _score_sws(nq, G, r, ref, u_packed=False):
    """scratch with which a scoring entry point runs on the bf16 matrix pipe: (tensor, bytes), or (None, 0) on the fp32-MFMA
    route.  The four entry points compare scores bit for bit among themselves: the switch is one module attribute for all of them.
    u_packed: the candidates' planes exist already (_planes) -- room for the queries' only."""
    if _NO_SPLIT_GEMM or nq < 1 or G < 1:
        return None, 0
    n = (pure("txe_split_packed_bytes", int(nq), int(r)) + 255) // 256 * 256 if u_packed else pure("txe_score_split_ws_bytes", int(nq), int(G), int(r))
    return _ws(n, ref), n


# ----------------------------------------------------------------------------------------------------------------
# the modes of the all-candidate loop -- store, count, best-k, log-partition -- once for every matcher family
# ----------------------------------------------------------------------------------------------------------------
class _Family:
    """what the mode functions below (and scoring.prepare_matcher's loop over blocks) take from a matcher family:
    prefix: of its C entry points -- prefix + "_block" / "_count_block" / "_topk_block" / "_topk_wide_block" / "_lse_block" /
    "_moments_block";
    queries(Q, prep, q_padded=False): one block's prepared query side, its row count in .n;
    head(qp, prep) / tail(qp, prep, store=False): the C arguments in front of / behind a mode's own (store: for prefix_block);
    ref(qp, prep): the tensor whose device the outputs and the scratch follow;
    project(hg, match): the candidate side; loop_queries(Q, prep): all queries prepared once, their row blocks go to queries();
    positives(qb, prep, off, rows, out): the thresholds of the ranking, whose route differs per family.
    BIM / LBM is the subclass below; MLP and NTN (_MLP, _NTN further down) are instances made of their sections' functions."""

    def __init__(self, prefix, **functions):
        self.prefix = prefix
        self.__dict__.update(functions)

    def tail(self, qp, prep, store=False):
        return ()


# one query block of a BIM / LBM call: Q laid as _query_layout asks (pitch ldq, contraction width K), its row count, the candidates' planes
# that go with K (up: _planes) and the scratch of the bf16 route beside them (sws, swb: _score_sws)
_BilinearQueries = collections.namedtuple("_BilinearQueries", "Q ldq K n up sws swb")


class _BilinearFamily(_Family):
    """BIM (apply_exp false) / LBM (true) over a BilinearPrepared"""
    prefix = "txe_score"

    def __init__(self, apply_exp):
        self.apply_exp = apply_exp

    def project(self, hg, match):
        return bilinear_prepare(hg, match.W.weight)

    def loop_queries(self, Q, prep):
        return pad_queries_like(Q, prep)

    def positives(self, qb, prep, off, rows, out):
        return positive_scores_staircase(qb, prep.gather(rows), self.apply_exp, off, out)

    def queries(self, Q, prep, q_padded=False):
        _need_cuda(Q, prep.full)
        Q, ldq, K = _lay_queries(Q, prep, q_padded)
        up = _planes(prep, K)
        return _BilinearQueries(Q, ldq, K, Q.shape[0], up, *_score_sws(Q.shape[0], prep.G, K, Q, up is not None))

    def head(self, qp, prep):
        return (ptr(qp.Q), qp.ldq, qp.n, ptr(prep.full), prep.full.stride(0), prep.G, qp.K, int(self.apply_exp))

    def tail(self, qp, prep, store=False):
        tws = _tail_ws(qp.Q) if store else None         # (the stored block's whole rounds run on persistent workgroups: their scratch)
        return ((ptr(tws), tws.numel()) if store else ()) + (ptr(qp.sws), qp.swb, ptr(qp.up))

    def ref(self, qp, prep):
        return qp.Q


def _store_block(fam, Q, prep, out=None):
    """S [nq, G] of one query block; default: rows on a 16-byte pitch (vector stores / rank sweeps)"""
    qp = fam.queries(Q, prep)
    nq, G, ref = qp.n, prep.G, fam.ref(qp, prep)
    S = out if out is not None else _empty((nq, (G + 3) // 4 * 4), ref)[:, :G]
    assert S.dtype == torch.float32 and (S.numel() == 0 or S.stride(1) == 1)
    if nq > 0 and G > 0:
        with _lib.on_device(ref.device):
            call(fam.prefix + "_block", *fam.head(qp, prep), ptr(S), S.stride(0) if nq > 1 else max(S.stride(0), G),
                 *fam.tail(qp, prep, store=True), _lib.stream_ptr())
    return S


def _count_block(fam, Q, prep, pos_off, thr, larger_is_better, counts, q_padded=False):
    """counts int32 [n_pos] += the candidates strictly better than each positive's threshold; counts None: zeros made here"""
    qp = fam.queries(Q, prep, q_padded)
    ref = fam.ref(qp, prep)
    pos_off = _i32(pos_off, ref.device)
    thr = _f32(thr)
    if counts is None:
        counts = torch.zeros(max(int(thr.numel()), 1), dtype=torch.int32, device=ref.device)
    if thr.numel() == 0 or qp.n == 0 or prep.G == 0:    # (a query block without a single positive: nothing to count)
        return counts
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() >= thr.numel()
    with _lib.on_device(ref.device):
        call(fam.prefix + "_count_block", *fam.head(qp, prep), ptr(pos_off), ptr(thr), int(larger_is_better), ptr(counts),
             *fam.tail(qp, prep), _lib.stream_ptr())
    return counts


def _topk_scratch(sc, nq, need, ref):
    """the best-k entry points' per-tile lists (key fp32 / idx int32 [need]) and floors (int32 [nq]) in the dict a loop over blocks
    passes along (None: for this call only), grown when a block needs more or the device changed"""
    sc = sc if sc is not None else {}
    if sc.get("n", 0) < need or sc.get("nq", 0) < nq or sc["key"].device != ref.device:
        sc["key"], sc["idx"], sc["n"] = _empty((need,), ref), torch.empty(need, dtype=torch.int32, device=ref.device), need
        sc["floor"], sc["nq"] = torch.empty(nq, dtype=torch.int32, device=ref.device), nq
    return sc


TOPK_WIDE_MAX = 64          # txe_topk_wide_max(): the widest fused best-k (rounds of 8 under a ceiling; csrc/txe_common.h)


def _topk_ceil(sc, nq, ref):
    """the wide best-k entry points' ceilings (8 * nq bytes: [nq] fp32 keys, then [nq] int32 columns) beside _topk_scratch's buffers"""
    if sc.get("ceil_nq", 0) < nq or sc["ceil"].device != ref.device:
        sc["ceil"], sc["ceil_nq"] = torch.empty(2 * nq, dtype=torch.int32, device=ref.device), nq
    return sc["ceil"]


def _topk_block(fam, Q, prep, k, larger_is_better, idx_base, scratch, q_padded=False):
    """(idx int32 [nq, k], key fp32 [nq, k]) of one query block: up to 8 the one pass of prefix_topk_block, above it prefix_topk_wide_block's
    rounds"""
    qp = fam.queries(Q, prep, q_padded)
    nq, G, ref = qp.n, prep.G, fam.ref(qp, prep)
    assert 1 <= k <= TOPK_WIDE_MAX and k <= G, fam.prefix[4:] + "_topk_block: 1 <= k <= min(64, candidates)"
    idx = torch.empty((nq, k), dtype=torch.int32, device=ref.device)
    key = _empty((nq, k), ref)
    if nq == 0:
        return idx, key
    with _lib.on_device(ref.device):
        sc = _topk_scratch(scratch, nq, nq * pure("txe_score_topk_tiles", G) * min(k, 8), ref)
        args = (*fam.head(qp, prep), int(larger_is_better), int(k), int(idx_base), ptr(sc["key"]), ptr(sc["idx"]), ptr(sc["floor"]), ptr(idx),
                ptr(key), *fam.tail(qp, prep))
        if k <= 8:
            call(fam.prefix + "_topk_block", *args, _lib.stream_ptr())
        else:
            call(fam.prefix + "_topk_wide_block", *args, ptr(_topk_ceil(sc, nq, ref)), _lib.stream_ptr())
    return idx, key


def _lse_scratch(sc, need, ref):
    """the log-partition entry points' per-tile (max, sum) pairs (two fp32 [need]) in the dict a loop over blocks passes along (None: for
    this call only), grown when a block needs more or the device changed"""
    sc = sc if sc is not None else {}
    if sc.get("lse_n", 0) < need or sc["lse_max"].device != ref.device:
        sc["lse_max"], sc["lse_sum"], sc["lse_n"] = _empty((need,), ref), _empty((need,), ref), need
    return sc


def _lse_block(fam, Q, prep, larger_is_better, scratch, q_padded=False):
    """lse fp32 [nq] of one query block: one pass of prefix_lse_block"""
    qp = fam.queries(Q, prep, q_padded)
    nq, G, ref = qp.n, prep.G, fam.ref(qp, prep)
    assert G >= 1, fam.prefix[4:] + "_lse_block: at least one candidate"
    lse = _empty((nq,), ref)
    if nq == 0:
        return lse
    with _lib.on_device(ref.device):
        sc = _lse_scratch(scratch, nq * pure("txe_score_topk_tiles", G), ref)
        call(fam.prefix + "_lse_block", *fam.head(qp, prep), int(larger_is_better), ptr(sc["lse_max"]), ptr(sc["lse_sum"]), ptr(lse),
             *fam.tail(qp, prep), _lib.stream_ptr())
    return lse


def _check_beta(beta, what="beta"):
    """the score scale of the moments mode as the fp32 the kernels take: finite and > 0 (ValueError before any launch)"""
    try:
        b = float(beta)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a finite number > 0, got {beta!r}") from None
    b32 = float(torch.tensor(b, dtype=torch.float32).item()) if math.isfinite(b) else b
    if isinstance(beta, bool) or not (math.isfinite(b32) and b32 > 0.0):
        raise ValueError(f"{what} must be finite and > 0 (in fp32), got {beta!r}")
    return b32


def _moments_scratch(sc, need, ref):
    """the moments entry points' per-tile quadruples (four fp32 [need]) in the dict a loop over blocks passes along (None: for this call
    only), grown when a block needs more or the device changed"""
    sc = sc if sc is not None else {}
    if sc.get("mom_n", 0) < need or sc["mom"][0].device != ref.device:
        sc["mom"], sc["mom_n"] = tuple(_empty((need,), ref) for _ in range(4)), need
    return sc


def _moments_block(fam, Q, prep, larger_is_better, beta, scratch, q_padded=False):
    """(lse, mean, var, entropy) float64 [nq, 4] of one query block at the score scale beta: one pass of prefix_moments_block"""
    beta = _check_beta(beta)
    qp = fam.queries(Q, prep, q_padded)
    nq, G, ref = qp.n, prep.G, fam.ref(qp, prep)
    assert G >= 1, fam.prefix[4:] + "_moments_block: at least one candidate"
    out = torch.empty((nq, 4), dtype=torch.float64, device=ref.device)
    if nq == 0:
        return out
    with _lib.on_device(ref.device):
        sc = _moments_scratch(scratch, nq * pure("txe_score_topk_tiles", G), ref)
        call(fam.prefix + "_moments_block", *fam.head(qp, prep), int(larger_is_better), beta, *(ptr(t) for t in sc["mom"]), ptr(out),
             *fam.tail(qp, prep), _lib.stream_ptr())
    return out


def score_block(Q, U, apply_exp, out=None):
    """S[q][g] = match(hg[g], Q[q]) for a block of queries against every candidate (test_fast.py:116-123).  U: a [G, r] tensor (that of
    bilinear_project brings its padding and planes along) or a BilinearPrepared, here and in the score_* functions below."""
    return _store_block(_BilinearFamily(apply_exp), Q, _as_prepared(U), out)


def positive_scores(Q, U, apply_exp, pos_off, pos_idx):
    """thr[j] = match(hg[pos_idx[j]], Q[q(j)]) for each query's true parents, through the SAME score kernel as the full block
    (bit-identical values: the fused ranking compares against them).  pos_idx rows of U that are out of range (< 0: a positive that
    lives in another candidate shard) give 0."""
    _need_cuda(Q, U)
    dev = Q.device
    pos_off = _i32(pos_off, dev)
    pos_idx = _i32(pos_idx, dev)
    n_pos = int(pos_idx.numel())
    if n_pos == 0:
        return torch.zeros(0, dtype=torch.float32, device=dev)
    counts = (pos_off[1:] - pos_off[:-1]).long()
    qid = torch.repeat_interleave(torch.arange(Q.shape[0], device=dev), counts)
    local = pos_idx >= 0
    Ug = U[pos_idx.clamp(min=0).long()]
    Sp = score_block(Q, Ug, apply_exp)
    thr = Sp[qid, torch.arange(n_pos, device=dev)]
    return torch.where(local, thr, torch.zeros_like(thr)).contiguous()


def pad_queries_like(Q, U):
    """the query matrix zero-padded to U's k-tile pitch, ONCE for a whole scoring loop: blocks `Qp[q0:q1, :r]` of the result go to
    score_count_block(..., q_padded=True) without being copied again.  Returns Q itself (fp32, unit column stride) when U carries no
    padding: the entry points re-lay a block on an odd pitch themselves, and the staircase reads it where it lies."""
    prep = _as_prepared(U)
    Qr = _rows(Q)[0]
    how = _query_layout(Qr.shape[0], Qr.shape[1], Qr.stride(0), prep.rp, False)[0]
    return _lay_queries(Qr, prep)[0][:, :prep.r] if how == "pad" else Qr


def positive_scores_staircase(Q, Up, apply_exp, pos_off, out):
    """out[j] = match(Q[q], Up[j]) for j in [pos_off[q], pos_off[q+1]): Up holds the candidate rows of the queries' true parents, query
    by query (a tensor, or BilinearPrepared.gather's result).  The score kernel's own tiles (bit-identical values), only those along
    the staircase (txe_score_positives).  The queries are read where they lie, on any pitch: of _query_layout's answers only 'both
    operands padded' (pad_queries_like + gather) applies -- the whole reduction on the plain loader, the very k-tiles
    txe_score_count_block runs."""
    prep = _as_prepared(Up)
    _need_cuda(Q, prep.full)
    assert Q.dtype == torch.float32 and Q.stride(1) == 1 and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= prep.G
    nq, r = Q.shape
    ldq = Q.stride(0)
    how, K, _ = _query_layout(nq, r, ldq, prep.rp, ldq == prep.rp)
    if how != "padded":
        K = r
    with _lib.on_device(Q.device):
        sws, swb = _score_sws(nq, prep.G, K, Q)
        call("txe_score_positives", ptr(Q), ldq, nq, ptr(prep.full), prep.full.stride(0), prep.G, K, int(apply_exp), ptr(pos_off), ptr(out),
             ptr(sws), swb, _lib.stream_ptr())
    return out


def score_count_block(Q, U, apply_exp, pos_off, thr, larger_is_better=True, counts=None, q_padded=False):
    """fused scoring + ranking of one query block against a candidate (shard) matrix U: int32 counts [n_pos] of candidates that beat
    each positive's score thr[j] (txe_score_count_block; no [nq x G] score block is materialised).
    q_padded: Q is a row block of pad_queries_like(all queries, U) -- its columns up to U's padded width are zeros already."""
    return _count_block(_BilinearFamily(apply_exp), Q, _as_prepared(U), pos_off, thr, larger_is_better, counts, q_padded)


def score_topk_block(Q, U, apply_exp, k, larger_is_better=True, idx_base=0, q_padded=False, scratch=None):
    """fused scoring + best-k selection of one query block against a candidate (shard) matrix U (txe_score_topk_block): returns
    (idx int32 [nq, k] = candidate rows + idx_base, best first, ties by ascending row like Python's stable sort, NaN last;
    key fp32 [nq, k] = the scores, negated when smaller is better).  No [nq x G] block is materialised.  1 <= k <= min(64, G): up to 8
    the one pass of txe_score_topk_block, above it txe_score_topk_wide_block's ceil(k / 8) rounds of 8 under a ceiling (same order, same
    scores, one pass of the score tiles per round).
    q_padded: as in score_count_block.  scratch: dict reused across the blocks of a loop (the per-tile lists)."""
    return _topk_block(_BilinearFamily(apply_exp), Q, _as_prepared(U), k, larger_is_better, idx_base, scratch, q_padded)


def topk_merge(keys, idx, k):
    """best k of the (key, idx) entries of every row (txe_topk_merge; keys fp32 / idx int32 [nq, cnt], idx == INT_MAX: empty slot):
    the merge of per-rank best-k lists of a candidate-sharded loop.  Returns (idx [nq, k], key [nq, k]).  1 <= k <= 64: above 8
    txe_topk_merge_wide's rounds of 8 under a ceiling over the same lists (the idx of a row must then be distinct)."""
    _need_cuda(keys, idx)
    assert 1 <= k <= TOPK_WIDE_MAX, "topk_merge: 1 <= k <= 64"
    keys, idx = _f32(keys), idx.to(torch.int32).contiguous()
    nq, cnt = keys.shape
    out_i = torch.empty((nq, k), dtype=torch.int32, device=keys.device)
    out_k = _empty((nq, k), keys)
    with _lib.on_device(keys.device):
        if k <= 8:
            call("txe_topk_merge", ptr(keys), ptr(idx), nq, cnt, int(k), 0, ptr(out_i), ptr(out_k), _lib.stream_ptr())
        else:
            ceil = torch.empty(2 * max(nq, 1), dtype=torch.int32, device=keys.device)
            call("txe_topk_merge_wide", ptr(keys), ptr(idx), nq, cnt, int(k), 0, ptr(out_i), ptr(out_k), ptr(ceil), _lib.stream_ptr())
    return out_i, out_k


def score_lse_block(Q, U, apply_exp, larger_is_better=True, q_padded=False, scratch=None):
    """fused scoring + log-partition of one query block against a candidate matrix U (txe_score_lse_block): fp32 [nq],
    lse[q] = log sum_g exp(z[q][g]) with z the score (larger is better) or its negative -- the exact denominator of loss.py:52-57 over
    every candidate.  No [nq x G] block is materialised.  G >= 1.  A NaN score gives NaN, a z = +Inf gives +Inf, all z = -Inf gives
    -Inf.  q_padded: as in score_count_block.  scratch: dict reused across the blocks of a loop (the per-tile pairs)."""
    return _lse_block(_BilinearFamily(apply_exp), Q, _as_prepared(U), larger_is_better, scratch, q_padded)


def lse_merge(part_max, part_sum):
    """lse [nq] of rows given as (max, sum exp(z - max)) pairs (txe_lse_merge; two fp32 [nq, cnt]; (-inf, 0) is an empty slot): the
    merge of the per-tile pairs of the score kernels, or of the per-rank pairs of a candidate-sharded loop"""
    _need_cuda(part_max, part_sum)
    part_max, part_sum = _f32(part_max), _f32(part_sum)
    assert part_max.dim() == 2 and part_max.shape == part_sum.shape
    nq, cnt = part_max.shape
    lse = _empty((nq,), part_max)
    if nq > 0:
        with _lib.on_device(part_max.device):
            call("txe_lse_merge", ptr(part_max), ptr(part_sum), nq, cnt, ptr(lse), _lib.stream_ptr())
    return lse


def score_moments_block(Q, U, apply_exp, larger_is_better=True, beta=1.0, q_padded=False, scratch=None):
    """fused scoring + moments of one query block against a candidate matrix U (txe_score_moments_block): float64 [nq, 4] =
    (lse, mean, var, entropy) of p = softmax(t), t = fl32(beta * z), z the score (larger is better) or its negative; include/txe.h states
    the definitions and the special values.  No [nq x G] block is materialised.  G >= 1; beta finite and > 0 (ValueError).
    q_padded / scratch: as in score_lse_block."""
    return _moments_block(_BilinearFamily(apply_exp), Q, _as_prepared(U), larger_is_better, beta, scratch, q_padded)


def moments_merge(part_max, part_s0, part_s1, part_s2):
    """(lse, mean, var, entropy) float64 [nq, 4] of rows given as quadruples (txe_moments_merge; four fp32 [nq, cnt]; (-inf, 0, 0, 0) is
    an empty slot): the merge of the per-tile quadruples of the score kernels, or of the per-rank ones of a candidate-sharded loop"""
    _need_cuda(part_max, part_s0, part_s1, part_s2)
    parts = [_f32(t) for t in (part_max, part_s0, part_s1, part_s2)]
    assert parts[0].dim() == 2 and all(t.shape == parts[0].shape for t in parts)
    nq, cnt = parts[0].shape
    out = torch.empty((nq, 4), dtype=torch.float64, device=parts[0].device)
    if nq > 0:
        with _lib.on_device(parts[0].device):
            call("txe_moments_merge", *(ptr(t) for t in parts), nq, cnt, ptr(out), _lib.stream_ptr())
    return out


SELECT_K_MAX = 4096     # txe_select_k keeps its survivors in LDS


def normalized_rows(x, pack=True):
    """x / ||x||_2 per row (txe_row_normalize) as a BilinearPrepared: rows zero-padded to whole 32-column k-tiles and, on the split
    route (pack), their bf16 planes packed once -- the candidate side of a cosine_block loop; `.full[:n]` is the padded query side.  A
    zero-norm or non-finite row becomes NaN."""
    _need_cuda(x)
    x, ld = _rows(x)
    n, d = x.shape
    rp = (d + 31) // 32 * 32
    full = torch.zeros((max(n, 1), rp), dtype=torch.float32, device=x.device)
    planes = None
    with _lib.on_device(x.device):
        call("txe_row_normalize", ptr(x), ld, n, d, ptr(full), rp, _lib.stream_ptr())
        if pack and not _NO_SPLIT_GEMM and n >= 1:
            planes = torch.empty(pure("txe_split_packed_bytes", n, rp), dtype=torch.uint8, device=x.device)
            call("txe_split_pack", ptr(full), rp, n, rp, 1, ptr(planes), _lib.stream_ptr())
    return BilinearPrepared(full, n, d, rp, planes, full._version)


def cosine_block(Qn, Cn, out):
    """out [nq, G] = Qn Cn^T on the score GEMM (txe_score_block, no exp): Qn = rows of normalized_rows(queries).full (padded like the
    candidates), Cn = normalized_rows(candidates)"""
    _need_cuda(Qn, Cn.full, out)
    assert Qn.dtype == torch.float32 and Qn.stride(1) == 1 and Qn.stride(0) == Cn.rp and out.dtype == torch.float32 and out.stride(1) == 1
    nq, G, K = Qn.shape[0], Cn.G, Cn.rp
    assert out.shape == (nq, G)
    with _lib.on_device(Qn.device):
        tws = _tail_ws(Qn)
        up = _planes(Cn, K)
        sws, swb = _score_sws(nq, G, K, Qn, up is not None)
        call("txe_score_block", ptr(Qn), Cn.rp, nq, ptr(Cn.full), Cn.rp, G, K, 0, ptr(out), out.stride(0), ptr(tws), tws.numel(), ptr(sws), swb,
             ptr(up), _lib.stream_ptr())
    return out


def select_k(S, k, mask_off=None, mask_idx=None, want_keys=False, out=None):
    """per row of S [nq, G] (fp32, unit column stride, any row pitch; not written) the k unmasked columns with the largest value, best
    first, equal values by ascending column, NaN last; -1 where fewer than k exist (txe_select_k).  Masks: CSR on the device, int32
    mask_off [nq + 1] indexing into mask_idx.  Returns idx int32 [nq, k], or (idx, keys fp32 [nq, k]) with want_keys."""
    _need_cuda(S, mask_off, mask_idx)
    k = int(k)
    if not 1 <= k <= SELECT_K_MAX:
        raise ValueError(f"select_k: 1 <= k <= {SELECT_K_MAX}, got {k}")
    if (mask_off is None) != (mask_idx is None):
        raise ValueError("select_k: mask_off and mask_idx go together")
    assert S.dim() == 2 and S.dtype == torch.float32 and S.stride(1) == 1 and S.shape[1] >= 1 and (S.shape[0] <= 1 or S.stride(0) >= S.shape[1])
    nq, G = S.shape
    idx = out if out is not None else torch.empty((nq, k), dtype=torch.int32, device=S.device)
    assert idx.dtype == torch.int32 and idx.is_contiguous() and idx.shape == (nq, k)
    keys = _empty((nq, k), S) if want_keys else None
    if mask_idx is not None and mask_idx.numel() == 0:
        mask_off = mask_idx = None                         # nothing is masked: no bitmap
    if nq > 0:
        if mask_off is not None:
            assert mask_off.dtype == torch.int32 and mask_idx.dtype == torch.int32 and mask_off.numel() == nq + 1
            assert mask_off.is_contiguous() and mask_idx.is_contiguous()
        with _lib.on_device(S.device):
            wsb = pure("txe_select_k_ws_bytes", nq, G) if mask_off is not None else 0
            ws = _ws(wsb, S) if wsb else None
            call("txe_select_k", ptr(S), S.stride(0) if nq > 1 else max(S.stride(0), G), nq, G, ptr(mask_off), ptr(mask_idx), k, ptr(idx),
                 ptr(keys), ptr(ws), wsb, _lib.stream_ptr())
    return (idx, keys) if want_keys else idx


def rank_finalize(pos_off, thr, counts, larger_is_better=True, out=None):
    """ranks (int32) from the fused counts: positives never count against each other (metric.py:7-31).  out: int32 [>= n_pos]"""
    _need_cuda(thr)
    pos_off = _i32(pos_off, thr.device)
    n_pos = int(thr.numel())
    ranks = out if out is not None else torch.empty(max(n_pos, 1), dtype=torch.int32, device=thr.device)
    if n_pos == 0:
        return ranks[:0]
    with _lib.on_device(thr.device):
        call("txe_rank_finalize", ptr(pos_off), int(pos_off.numel()) - 1, ptr(_f32(thr)), ptr(counts), int(larger_is_better), ptr(ranks),
             _lib.stream_ptr())
    return ranks[:n_pos]


def rank_block(S, pos_off, pos_idx, larger_is_better=True):
    """ranks of each query's true parents among the candidates (metric.py:7-31 semantics), int32 on device."""
    _need_cuda(S)
    nq, G = S.shape
    pos_off = _i32(pos_off, S.device)
    pos_idx = _i32(pos_idx, S.device)
    ranks = torch.empty(max(int(pos_idx.numel()), 1), dtype=torch.int32, device=S.device)
    with _lib.on_device(S.device):
        call("txe_rank_block", ptr(S), S.stride(0), nq, G, ptr(pos_off), ptr(pos_idx), ptr(ranks), int(larger_is_better), None,
             _lib.stream_ptr())
    return ranks[:pos_idx.numel()]


# ================================================================================================================
# MLP matcher (model_zoo.py:285-298) on the all-candidate loop: txe_mlp_* (VALU pair kernel, no [G, l+r] x [l+r, H] product per query)
# ================================================================================================================
class MLPPrepared:
    """the candidate side of the MLP matcher, once per candidate set: Ap [G, Hp] = hg W1a^T + b1 zero-padded to Hp, flags [G] (rows
    with NaN / +-Inf / huge values: their pairs take the literal formula), mw [Hp + 2] = (w2 padded, b2, the flag limit), W1bT [r, H]"""
    __slots__ = ("Ap", "flags", "mw", "W1bT", "G", "H", "r")

    def __init__(self, Ap, flags, mw, W1bT, G, H, r):
        self.Ap, self.flags, self.mw, self.W1bT, self.G, self.H, self.r = Ap, flags, mw, W1bT, G, H, r


class MLPQueries:
    """the query side of one block: nB [nq, Hp] = -(Q W1b^T) zero-padded, c [nq] = b2 + B w2, flags [nq]"""
    __slots__ = ("nB", "c", "flags", "n")

    def __init__(self, nB, c, flags, n):
        self.nB, self.c, self.flags, self.n = nB, c, flags, n

    @property
    def shape(self):
        return (self.n, self.nB.shape[1])

    def __getitem__(self, sl):
        """a row block (slice) of a prepared query set: rows are independent, so a block of the whole set's preparation is the block's own"""
        assert isinstance(sl, slice) and sl.step in (None, 1)
        lo, hi, _ = sl.indices(self.n)
        hi = max(hi, lo)
        return MLPQueries(self.nB[lo:hi], self.c[lo:hi], self.flags[lo:hi], hi - lo)


def mlp_project(hg, match):
    """prepare the candidate side of an MLP matcher for scoring: A = hg W1a^T + b1 on the fp32 GEMM (txe_linear_fwd), padded and
    flagged by txe_mlp_project.  Returns MLPPrepared."""
    W1, b1 = match.ffn[0].weight, match.ffn[0].bias
    w2, b2 = match.ffn[2].weight, match.ffn[2].bias
    _need_cuda(hg, W1, b1, w2, b2)
    hg, ld = _rows(hg)
    G, l = hg.shape
    H, K = W1.shape
    r = K - l
    assert r >= 1 and w2.numel() == H and b2.numel() == 1, "mlp_project: ffn = Linear(l + r, H), ReLU, Linear(H, 1)"
    with _lib.on_device(hg.device):
        Hp = pure("txe_mlp_padded_h", H)
        Ap = _empty((max(G, 1), Hp), hg)
        flags = torch.zeros(max(G, 1), dtype=torch.int32, device=hg.device)
        mw = _empty((Hp + 2,), hg)
        A = None
        if G > 0:
            W1a = _f32(W1[:, :l])
            A = _empty((G, H), hg)
            call("txe_linear_fwd", ptr(hg), ld, l, None, 0, 0, G, ptr(W1a), ptr(_f32(b1)), H, 0, ptr(A), _lib.stream_ptr())
        call("txe_mlp_project", ptr(A) if A is not None else None, H, G, H, ptr(_f32(w2.reshape(-1))), ptr(_f32(b2.reshape(-1))),
             ptr(Ap), ptr(mw), ptr(flags), _lib.stream_ptr())
    return MLPPrepared(Ap[:G], flags[:G], mw, _f32(W1[:, l:].t()), G, H, r)


def mlp_prepare_queries(Q, prep):
    """the query side of a block (or of a whole query set: MLPQueries slices into blocks)"""
    if isinstance(Q, MLPQueries):
        return Q
    _need_cuda(Q)
    Q, ldq = _rows(Q)
    nq, r = Q.shape
    assert r == prep.r, "mlp_prepare_queries: query width != the matcher's r"
    Hp = prep.mw.numel() - 2
    nB = _empty((max(nq, 1), Hp), Q)
    c = _empty((max(nq, 1),), Q)
    flags = torch.zeros(max(nq, 1), dtype=torch.int32, device=Q.device)
    if nq > 0:
        with _lib.on_device(Q.device):
            call("txe_mlp_query_project", ptr(Q), ldq, nq, r, ptr(prep.W1bT), prep.H, ptr(prep.mw), ptr(nB), ptr(c), ptr(flags),
                 _lib.stream_ptr())
    return MLPQueries(nB[:nq], c[:nq], flags[:nq], nq)


def _mlp_args(qp, prep):
    return (ptr(prep.Ap), ptr(prep.flags), prep.G, ptr(qp.nB), ptr(qp.c), ptr(qp.flags), qp.n, prep.H, ptr(prep.mw))


def mlp_score_block(Q, prep, out=None):
    """S[q][g] = match(hg[g], Q[q]) of an MLP matcher for a block of queries (raw [nq, r] or MLPQueries) against every candidate
    (txe_mlp_score_block).  out: [nq, G] view with unit column stride; default: rows on a 16-byte pitch like score_block."""
    return _store_block(_MLP, Q, prep, out)


def mlp_positive_scores(Q, prep, pos_off, pos_idx, out=None):
    """thr[j] = match(hg[pos_idx[j]], Q[q]) for each query's true parents (the pair kernel's own chain: bit-identical to the stored
    block); pos_idx outside [0, G) (a positive that lives in another candidate shard) gives 0"""
    qp = mlp_prepare_queries(Q, prep)
    dev = prep.Ap.device
    pos_off = _i32(pos_off, dev)
    pos_idx = _i32(pos_idx, dev)
    n_pos = int(pos_idx.numel())
    thr = out if out is not None else torch.zeros(n_pos, dtype=torch.float32, device=dev)
    assert thr.dtype == torch.float32 and thr.is_contiguous() and thr.numel() >= n_pos
    if n_pos > 0 and qp.n > 0:
        with _lib.on_device(dev):
            call("txe_mlp_score_positives", *_mlp_args(qp, prep), ptr(pos_off), ptr(pos_idx), n_pos, ptr(thr), _lib.stream_ptr())
    return thr[:n_pos]


def mlp_score_count_block(Q, prep, pos_off, thr, larger_is_better=True, counts=None):
    """fused scoring + ranking of one query block (txe_mlp_score_count_block): int32 counts [n_pos] of candidates strictly better than
    each positive's threshold; no [nq x G] block is materialised.  counts (zeroed by the caller) accumulate: shards add."""
    return _count_block(_MLP, Q, prep, pos_off, thr, larger_is_better, counts)


def mlp_score_topk_block(Q, prep, k, larger_is_better=True, idx_base=0, scratch=None):
    """fused scoring + best-k selection of one query block (txe_mlp_score_topk_block): (idx int32 [nq, k] = candidate rows + idx_base,
    key fp32 [nq, k]) in score_topk_block's order and conventions.  1 <= k <= min(64, G), above 8 by txe_mlp_score_topk_wide_block's
    rounds.  scratch: dict reused across blocks."""
    return _topk_block(_MLP, Q, prep, k, larger_is_better, idx_base, scratch)


def mlp_score_lse_block(Q, prep, larger_is_better=True, scratch=None):
    """fused scoring + log-partition of one query block (txe_mlp_score_lse_block): fp32 [nq] in score_lse_block's definition and
    conventions.  G >= 1.  scratch: dict reused across blocks."""
    return _lse_block(_MLP, Q, prep, larger_is_better, scratch)


def mlp_score_moments_block(Q, prep, larger_is_better=True, beta=1.0, scratch=None):
    """fused scoring + moments of one query block (txe_mlp_score_moments_block): float64 [nq, 4] in score_moments_block's definition"""
    return _moments_block(_MLP, Q, prep, larger_is_better, beta, scratch)


_MLP = _Family("txe_mlp_score", project=mlp_project, loop_queries=mlp_prepare_queries, positives=mlp_positive_scores, head=_mlp_args,
               queries=lambda Q, prep, q_padded=False: mlp_prepare_queries(Q, prep), ref=lambda qp, prep: prep.Ap)


# ================================================================================================================
# NTN matcher (model_zoo.py:331-346) on the all-candidate loop: txe_ntn_* (the score GEMM's tile once per bilinear slice, tanh and the
# sum over slices in its registers, the score GEMM's own store / pick / count / best-k epilogue)
# ================================================================================================================
NTN_MAX_K = 16          # slices the kernel's entry points accept


class NTNPrepared:
    """the candidate side of an NTN matcher, once per candidate set: full [max(G, 1), k * rp] -- slice j of candidate g, U_j[g] = hg[g] W_j,
    lies at full[g, j * rp : j * rp + r], zero-padded to rp columns (bilinear_prepare's rule: whole 32-column k-tiles) --
    a [k, max(G, 1)] = V1 hg^T + b, u [k] = u_R.weight, V2 [k, r] = the query half of V.weight"""
    __slots__ = ("full", "a", "u", "V2", "G", "r", "rp", "k")

    def __init__(self, full, a, u, V2, G, r, rp, k):
        self.full, self.a, self.u, self.V2, self.G, self.r, self.rp, self.k = full, a, u, V2, G, r, rp, k

    def slice(self, j):
        """U_j as a [G, r] view"""
        return self.full[:self.G, j * self.rp:j * self.rp + self.r]

    def gather(self, idx):
        """the rows idx of every slice (with their zero padding) and of a: the candidate side of ntn_positive_scores"""
        idx = idx.long()
        return NTNPrepared(self.full.index_select(0, idx), self.a.index_select(1, idx), self.u, self.V2, int(idx.numel()), self.r, self.rp, self.k)


class NTNQueries:
    """the query side of a block: Qp [nq, rp] = the queries zero-padded like the candidates' slices, c [k, nq] = V2 Q^T"""
    __slots__ = ("Qp", "c", "n")

    def __init__(self, Qp, c, n):
        self.Qp, self.c, self.n = Qp, c, n

    @property
    def shape(self):
        return (self.n, self.Qp.shape[1])

    def __getitem__(self, sl):
        """a row block (slice) of a prepared query set: rows are independent, so a block of the whole set's preparation is the block's own"""
        assert isinstance(sl, slice) and sl.step in (None, 1)
        lo, hi, _ = sl.indices(self.n)
        hi = max(hi, lo)
        return NTNQueries(self.Qp[lo:hi], self.c[:, lo:hi], hi - lo)


def ntn_project(hg, match):
    """prepare the candidate side of an NTN matcher for scoring: the k products U_j = hg W_j as ONE txe_bilinear_project on the stacked,
    zero-padded weight [l, k * rp] (the route bilinear_prepare takes: the bf16 pipe's fp32-accurate product unless _NO_SPLIT_GEMM; made
    once, so every scoring mode reads the same values) and a = V1 hg^T + b (txe_ntn_project).  Returns NTNPrepared."""
    W, b, V, u = match.W.weight, match.W.bias, match.V.weight, match.u_R.weight
    _need_cuda(hg, W, b, V, u)
    hg, ld = _rows(hg)
    G, l = hg.shape
    k, lw, r = W.shape
    assert lw == l and V.shape == (k, l + r) and u.numel() == k and b is not None and b.numel() == k, \
        "ntn_project: W = Bilinear(l, r, k), V = Linear(l + r, k), u_R = Linear(k, 1)"
    assert 1 <= k <= NTN_MAX_K, f"ntn_project: 1 <= k <= {NTN_MAX_K}"
    rp = (r + 31) // 32 * 32
    Wst = torch.zeros((l, k, rp), dtype=torch.float32, device=hg.device)
    Wst[:, :, :r].copy_(W.detach().permute(1, 0, 2))
    full = _empty((max(G, 1), k * rp), hg)
    a = _empty((k, max(G, 1)), hg)
    V1 = _f32(V.detach()[:, :l])
    with _lib.on_device(hg.device):
        if G > 0:
            swb = 0 if _NO_SPLIT_GEMM else pure("txe_gemm_plain_split_ws_bytes", G, k * rp, l)
            sws = _ws(swb, hg) if swb else None
            call("txe_bilinear_project", ptr(hg), ld, G, l, ptr(Wst), k * rp, ptr(full), k * rp, ptr(sws), swb, _lib.stream_ptr())
            call("txe_ntn_project", ptr(hg), ld, G, l, ptr(V1), l, ptr(_f32(b.detach())), k, ptr(a), a.stride(0), _lib.stream_ptr())
        else:
            full.zero_()
            a.zero_()
    return NTNPrepared(full, a, _f32(u.detach().reshape(-1)), _f32(V.detach()[:, l:]), G, r, rp, k)


def ntn_prepare_queries(Q, prep):
    """the query side of a block (or of a whole query set: NTNQueries slices into blocks): the padded queries and c (txe_ntn_query_project)"""
    if isinstance(Q, NTNQueries):
        return Q
    _need_cuda(Q)
    Q, ldq = _rows(Q)
    nq, r = Q.shape
    assert r == prep.r, "ntn_prepare_queries: query width != the matcher's r"
    Qp = torch.zeros((max(nq, 1), prep.rp), dtype=torch.float32, device=Q.device)
    c = _empty((prep.k, max(nq, 1)), Q)
    if nq > 0:
        Qp[:nq, :r].copy_(Q)
        with _lib.on_device(Q.device):
            call("txe_ntn_query_project", ptr(Q), ldq, nq, r, ptr(prep.V2), r, prep.k, ptr(c), c.stride(0), _lib.stream_ptr())
    return NTNQueries(Qp[:nq], c[:, :nq], nq)


def _ntn_args(qp, prep):
    """(Q, ld_q, nq, U, ld_u, slice_u, G, r, a, ld_a, c, ld_c, u, k) of the txe_ntn_score_* entry points: both operands padded to rp, the
    reduction runs over all of it (zeros add exactly nothing)"""
    return (ptr(qp.Qp), prep.rp, qp.n, ptr(prep.full), prep.full.stride(0), prep.rp, prep.G, prep.rp, ptr(prep.a), prep.a.stride(0),
            ptr(qp.c), qp.c.stride(0), ptr(prep.u), prep.k)


def ntn_score_block(Q, prep, out=None):
    """S[q][g] = match(hg[g], Q[q]) of an NTN matcher for a block of queries (raw [nq, r] or NTNQueries) against every candidate
    (txe_ntn_score_block).  out: [nq, G] view with unit column stride; default: rows on a 16-byte pitch like score_block."""
    return _store_block(_NTN, Q, prep, out)


def ntn_positive_scores(Q, prep, pos_off, pos_idx, out=None, rows_valid=False):
    """thr[j] = match(hg[pos_idx[j]], Q[q]) for each query's true parents: the score kernel's own tiles over the GATHERED candidate side
    (NTNPrepared.gather), only those along the staircase of (query, own positive) pairs -- bit-identical to the stored block.  pos_idx
    outside [0, G) (a positive that lives in another candidate shard) gives 0; rows_valid: the caller promises there is none (and masks
    such positives itself)."""
    qp = ntn_prepare_queries(Q, prep)
    dev = prep.full.device
    pos_off = _i32(pos_off, dev)
    pos_idx = pos_idx.to(dev)
    n_pos = int(pos_idx.numel())
    thr = out if out is not None else torch.zeros(n_pos, dtype=torch.float32, device=dev)
    assert thr.dtype == torch.float32 and thr.is_contiguous() and thr.numel() >= n_pos
    if n_pos > 0 and qp.n > 0 and prep.G > 0:
        rows = pos_idx.long()
        ok = None
        if not rows_valid:
            ok = (rows >= 0) & (rows < prep.G)
            rows = torch.where(ok, rows, torch.zeros_like(rows))
        gp = prep.gather(rows)
        with _lib.on_device(dev):
            call("txe_ntn_score_positives", *_ntn_args(qp, gp), ptr(pos_off), ptr(thr), _lib.stream_ptr())
        if ok is not None:
            thr[:n_pos].copy_(torch.where(ok, thr[:n_pos], torch.zeros((), device=dev)))
    return thr[:n_pos]


def ntn_score_count_block(Q, prep, pos_off, thr, larger_is_better=True, counts=None):
    """fused scoring + ranking of one query block (txe_ntn_score_count_block): int32 counts [n_pos] of candidates strictly better than
    each positive's threshold; no [nq x G] block is materialised.  counts (zeroed by the caller) accumulate: shards add."""
    return _count_block(_NTN, Q, prep, pos_off, thr, larger_is_better, counts)


def ntn_score_topk_block(Q, prep, k, larger_is_better=True, idx_base=0, scratch=None):
    """fused scoring + best-k selection of one query block (txe_ntn_score_topk_block): (idx int32 [nq, k] = candidate rows + idx_base,
    key fp32 [nq, k]) in score_topk_block's order and conventions.  1 <= k <= min(64, G), above 8 by txe_ntn_score_topk_wide_block's
    rounds.  scratch: dict reused across blocks."""
    return _topk_block(_NTN, Q, prep, k, larger_is_better, idx_base, scratch)


def ntn_score_lse_block(Q, prep, larger_is_better=True, scratch=None):
    """fused scoring + log-partition of one query block (txe_ntn_score_lse_block): fp32 [nq] in score_lse_block's definition and
    conventions.  G >= 1.  scratch: dict reused across blocks."""
    return _lse_block(_NTN, Q, prep, larger_is_better, scratch)


def ntn_score_moments_block(Q, prep, larger_is_better=True, beta=1.0, scratch=None):
    """fused scoring + moments of one query block (txe_ntn_score_moments_block): float64 [nq, 4] in score_moments_block's definition"""
    return _moments_block(_NTN, Q, prep, larger_is_better, beta, scratch)


# (positives: the loop hands over the positives' local rows, those of another shard clamped to 0, and masks their scores itself, as for BIM / LBM)
_NTN = _Family("txe_ntn_score", project=ntn_project, loop_queries=ntn_prepare_queries, head=_ntn_args,
               positives=functools.partial(ntn_positive_scores, rows_valid=True),
               queries=lambda Q, prep, q_padded=False: ntn_prepare_queries(Q, prep), ref=lambda qp, prep: prep.full)
