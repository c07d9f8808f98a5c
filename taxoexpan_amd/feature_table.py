"""The term-embedding table as a trainable input (an addition: the reference freezes its embeddings, and so does every path here unless a
FeatureTable is handed to the loader and the trainer -- DESIGN 4.15).

A batch reads the table through two gathers, x = features[_id] and the distinct query rows; backward leaves one gradient row per
OCCURRENCE of a table row.  Two launches per step turn that into an updated table (csrc/txe_rowgrad.hip): txe_rowgrad_group sorts the
occurrences by row, txe_sparse_adam_rows sums every touched row's gradients in a fixed order and applies txe_adam_step's update to that
row of the table and of its moments.  Rows that do not occur are neither read nor written (lazy Adam); no floating-point atomics, so a
run is bit-repeatable like the rest of the library.
    FeatureTable            the table, its moments and the step
    host_row_sums           the numpy restatement of the kernel's summation order
    host_sparse_adam_rows   the numpy restatement of the whole step, float32 (operation for operation) or float64 (the definition)
Out of scope, on purpose: clipping the table's gradient (the step log's norm is over occurrences, not over table rows), weight decay (a
decay applied to the rows of a batch only would be another regulariser than the dense one), averaged weights of the table
(optim.Adam(ema_decay=...) averages the model's parameters only).  Rows of held-out terms never occur in a training batch: they keep
their initial vectors while their neighbours move.  Extra device memory: 2 x the table (3 x with amsgrad)."""
import numpy as np
import torch

from . import _lib
from .optim import host_guarded_adam

SPLIT = 64          # RG_SPLIT of csrc/txe_rowgrad.hip: a longer segment is summed in slices
SLICES = 16         # RG_WAVES: the slices of a long segment


def _seq_sum(g):
    """s = g[0]; s = s + g[k], k = 1 .. len - 1, in g's dtype"""
    s = g[0].copy()
    for k in range(1, g.shape[0]):
        s = s + g[k]
    return s


def host_segment_sum(g):
    """the sum of the L rows of g [L, d] in the order of txe_sparse_adam_rows, in g's dtype -- a function of L alone:
    L <= 64: left to right; L > 64: c = ceil(L / 16), the slices [j c, min(L, (j + 1) c)) left to right each, then their partial sums
    left to right"""
    L = g.shape[0]
    if L <= SPLIT:
        return _seq_sum(g)
    c = -(-L // SLICES)
    return _seq_sum(np.stack([_seq_sum(g[j * c:min(L, (j + 1) * c)]) for j in range(-(-L // c))]))


def host_row_sums(ids_a, d_a, ids_b, d_b, n_rows, dtype=np.float32):
    """(rows, sums): the table rows that occur, ascending, and the sum of their occurrences' gradient rows [len(rows), d] in `dtype`.
    Occurrences are grouped as txe_rowgrad_group groups them: by row, within a row in ascending occurrence index, a's before b's; an id
    outside [0, n_rows) is dropped.  float32 adds in the kernel's order with every sum rounded to fp32; float64 is the same order with
    nothing rounded to fp32."""
    dtype = np.dtype(dtype).type
    ids_a, ids_b = (np.asarray(i).astype(np.int64).reshape(-1) for i in (ids_a, ids_b))
    d_a, d_b = (np.asarray(g, dtype=np.float32) for g in (d_a, d_b))
    d = d_a.shape[1] if d_a.ndim == 2 and d_a.shape[0] else (d_b.shape[1] if d_b.ndim == 2 else 0)
    g = np.concatenate([d_a.reshape(-1, d), d_b.reshape(-1, d)], 0).astype(dtype)
    ids = np.concatenate([ids_a, ids_b])
    if g.shape[0] != ids.shape[0]:
        raise ValueError("one gradient row per occurrence")
    occ = np.flatnonzero((ids >= 0) & (ids < n_rows))
    occ = occ[np.argsort(ids[occ], kind="stable")]
    rows, start = np.unique(ids[occ], return_index=True)
    bounds = list(start) + [len(occ)]
    sums = np.zeros((len(rows), d), dtype=dtype)
    for s in range(len(rows)):
        sums[s] = host_segment_sum(g[occ[bounds[s]:bounds[s + 1]]])
    return rows, sums


def host_sparse_adam_rows(weight, exp_avg, exp_avg_sq, max_exp_avg_sq, ids_a, d_a, ids_b, d_b, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                          step=1, trainable=None, first_bad=None, dtype=np.float32):
    """txe_rowgrad_group + txe_sparse_adam_rows on the host: the new (weight, exp_avg, exp_avg_sq, max_exp_avg_sq) as `dtype` arrays (None
    for max_exp_avg_sq = plain Adam); no argument is changed.  float32 is the kernel operation for operation: host_row_sums' order, then
    optim.host_guarded_adam's arithmetic (weight_decay 0, the GLOBAL `step`) on the touched rows.  float64 is the definition with nothing
    rounded to fp32.  Rows that do not occur, rows whose `trainable` entry is 0 and -- with first_bad >= 0 -- every row come back as
    they were."""
    dtype = np.dtype(dtype).type
    if step < 1:
        raise ValueError("step counts from 1")
    w, m, v = (np.array(a, dtype=dtype) for a in (weight, exp_avg, exp_avg_sq))
    x = None if max_exp_avg_sq is None else np.array(max_exp_avg_sq, dtype=dtype)
    if first_bad is not None and int(first_bad) >= 0:
        return w, m, v, x
    rows, sums = host_row_sums(ids_a, d_a, ids_b, d_b, w.shape[0], dtype)
    if trainable is not None:
        keep = np.asarray(trainable).reshape(-1)[rows] != 0
        rows, sums = rows[keep], sums[keep]
    if len(rows):
        p_, m_, v_, x_ = host_guarded_adam(w[rows], sums, m[rows], v[rows], None if x is None else x[rows], lr=lr, beta1=beta1, beta2=beta2,
                                           eps=eps, weight_decay=0.0, step=step, dtype=dtype)
        w[rows], m[rows], v[rows] = p_, m_, v_
        if x is not None:
            x[rows] = x_
    return w, m, v, x


class FeatureTable:
    """The feature table of `dataset` on `device`, trained by lazy Adam.
    weight IS the storage of this table's device taxonomy (`.dtax`, a dataset.device_taxonomy(device)): it is updated in place, so every
    device consumer that is given this taxonomy -- DeviceBatchLoader(feature_table=...), and through the loader's `.dtax`
    evaluate.candidate_graphs and sampler.mine_hard_negatives -- reads the current table with no copy.  Host consumers (evaluate / infer /
    retrieve, the host sampler's test_topk path) read dataset.node_features and dataset.kv: write_back() refreshes them.
    exp_avg / exp_avg_sq (/ max_exp_avg_sq with amsgrad) have the table's shape; step_count is the number of steps taken; `updated` is a
    torch.cuda.Event recorded after every step (and at construction / load_state_dict): a stream that gathers rows for the NEXT batch
    waits for it.
    trainable_rows: None (all rows), a boolean mask [n_rows] or an iterable of row ids; the other rows are never written.
    With normalize_embed=True the table holds the L2-normalised rows the dataset serves; they are NOT re-normalised while they train.
    Not covered: gradient clipping, weight decay, averaged weights (see the module docstring)."""

    def __init__(self, dataset, device, lr, betas=(0.9, 0.999), eps=1e-8, amsgrad=False, trainable_rows=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("taxoexpan_amd.feature_table.FeatureTable lives on the GPU (no CPU path; host_sparse_adam_rows is the restatement)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if lr < 0.0 or eps < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("invalid Adam hyper-parameter")
        self.dataset, self.device = dataset, device
        self.lr, self.betas, self.eps, self.amsgrad = float(lr), (float(betas[0]), float(betas[1])), float(eps), bool(amsgrad)
        self.dtax = dataset.device_taxonomy(device)
        w = self.dtax.features
        if w is None or w.dim() != 2 or w.dtype != torch.float32:
            raise ValueError("FeatureTable needs a dataset with a 2-D fp32 feature table")
        if not w.is_contiguous():
            w = self.dtax.features = w.contiguous()
        self.weight = w
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(w), torch.zeros_like(w)
        self.max_exp_avg_sq = torch.zeros_like(w) if self.amsgrad else None
        self.trainable = None
        if trainable_rows is not None:
            t = torch.as_tensor(np.asarray(trainable_rows if not torch.is_tensor(trainable_rows) else trainable_rows.cpu()))
            if t.dtype == torch.bool:
                if t.shape != (w.shape[0],):
                    raise ValueError(f"a trainable_rows mask has one entry per table row ({w.shape[0]}), got {tuple(t.shape)}")
                mask = t
            else:
                t = t.reshape(-1).long()
                if t.numel() and (int(t.min()) < 0 or int(t.max()) >= w.shape[0]):
                    raise ValueError("trainable_rows holds a row id outside the table")
                mask = torch.zeros(w.shape[0], dtype=torch.bool)
                mask[t] = True
            self.trainable = mask.to(torch.uint8).to(device)
        self.step_count = 0
        self._leaves = None
        self._ws = None
        self.updated = torch.cuda.Event()
        with torch.cuda.device(device):
            self.updated.record(torch.cuda.current_stream(device))

    # ---- one step ---------------------------------------------------------------------------------------------------------------
    def leaves(self, g, qf, x=None):
        """Mark the batch's node features `x` (default g.ndata["x"]; a loader that pops them hands them in) and the distinct query rows
        of `qf` (an ops.RepeatedRows, what DeviceBatchLoader(feature_table=...) yields) as requiring gradients; returns
        (x, qf, g.ndata["_id"], g.query_ids).  Both are leaves: backward leaves the per-occurrence gradients in x.grad and qf.rows.grad,
        where step() finds them."""
        from .ops import RepeatedRows
        if x is None:
            x = g.ndata["x"]
        if not isinstance(qf, RepeatedRows):
            raise ValueError("FeatureTable.leaves needs the query features as an ops.RepeatedRows (DeviceBatchLoader(repeated_queries=True))")
        ids_a, ids_b = g.ndata["_id"], getattr(g, "query_ids", None)
        if ids_b is None:
            raise ValueError("FeatureTable.leaves: the batch has no g.query_ids (DeviceBatchLoader(feature_table=...) attaches them)")
        if not (torch.is_tensor(x) and x.is_leaf and qf.rows.is_leaf):
            raise ValueError("FeatureTable.leaves needs the gathered rows themselves (plain leaf tensors)")
        if x.shape[0] != ids_a.numel() or qf.rows.shape[0] != ids_b.numel():
            raise ValueError("FeatureTable.leaves: one id per gathered row")
        x.requires_grad_(True)
        qf.rows.requires_grad_(True)
        self._leaves = (x, qf.rows, ids_a, ids_b)
        return x, qf, ids_a, ids_b

    def _side(self, t, ids, what):
        """(ids int32, gradient fp32 with unit column stride, its pitch, its row count) of one gather"""
        g = t.grad
        if g is None:
            if t.shape[0] == 0:
                return None, None, self.weight.shape[1], 0
            raise RuntimeError(f"FeatureTable.step: {what} got no gradient -- the route the model took does not deliver it (a missing "
                               "gradient is an error, not a frozen row)")
        if g.dtype != torch.float32 or g.device != self.device or g.shape != t.shape:
            raise RuntimeError(f"FeatureTable.step: {what} has a gradient of another dtype, device or shape")
        if g.stride(1) != 1 or g.stride(0) < g.shape[1]:
            g = g.contiguous()
        ids = ids.to(device=self.device, dtype=torch.int32)
        return (ids if ids.is_contiguous() else ids.contiguous()), g, g.stride(0), g.shape[0]

    @torch.no_grad()
    def step(self, guard=None):
        """The two launches (txe_rowgrad_group, txe_sparse_adam_rows) on the current stream, over the gradients that backward left in the
        leaves of the last leaves() call; step_count += 1; `updated` is recorded.  guard (an optim.StepGuard): its first_bad is honoured
        -- once it is >= 0 the launch loads and stores nothing; the host still counts the step, see discount_frozen_steps.  A guard
        that carries a clip (gnorm2 or max_grad_norm) is a ValueError: the log's norm is over occurrences and is not the table
        gradient's norm."""
        if guard is not None and (guard.gnorm2 is not None or guard.max_grad_norm is not None):
            raise ValueError("FeatureTable.step: a guard that clips is not supported (the step log's norm is taken over per-occurrence "
                             "gradients, not over the table's rows)")
        if self._leaves is None:
            raise RuntimeError("FeatureTable.step: no leaves (call leaves(g, qf) before the forward pass of every step)")
        x, rows, ids_a, ids_b = self._leaves
        ia, ga, lda, na = self._side(x, ids_a, "the batch's node features")
        ib, gb, ldb, nb = self._side(rows, ids_b, "the distinct query rows")
        w = self.weight
        n_rows, d = w.shape
        with _lib.on_device(self.device):
            need = _lib.pure("txe_rowgrad_ws_bytes", na, nb)
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
            ws, s = self._ws, _lib.stream_ptr()
            _lib.call("txe_rowgrad_group", _lib.ptr(ia), na, _lib.ptr(ib), nb, n_rows, ws.data_ptr(), ws.numel(), s)
            _lib.call("txe_sparse_adam_rows", w.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), _lib.ptr(self.max_exp_avg_sq),
                      w.stride(0), n_rows, d, _lib.ptr(ga), lda, na, _lib.ptr(gb), ldb, nb, ws.data_ptr(), ws.numel(), _lib.ptr(self.trainable),
                      self.lr, self.betas[0], self.betas[1], self.eps, self.step_count + 1, None if guard is None else guard.first_bad, s)
            self.updated.record(torch.cuda.current_stream(self.device))
        torch.autograd.graph.increment_version(w)               # whatever memoises on the table sees a written tensor
        self.step_count += 1
        self._leaves = None

    def discount_frozen_steps(self, n):
        """take back `n` steps that the host counted and the device skipped (optim.Adam.discount_frozen_steps' meaning): step_count -= n,
        never below 0"""
        n = int(n)
        if n < 0:
            raise ValueError(f"discount_frozen_steps needs n >= 0, got {n}")
        self.step_count = max(self.step_count - n, 0)

    # ---- state ------------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """weight, moments (the tensors themselves, as a module's state_dict() hands out its parameters), step and hyper-parameters"""
        return {"weight": self.weight, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "max_exp_avg_sq": self.max_exp_avg_sq,
                "step": self.step_count, "lr": self.lr, "betas": self.betas, "eps": self.eps, "amsgrad": self.amsgrad,
                "trainable": self.trainable}

    @torch.no_grad()
    def load_state_dict(self, state):
        """state_dict()'s counterpart: the tensors are COPIED into this table's storage (the device taxonomy keeps reading it); a table
        of another shape is refused (ValueError, nothing changed)"""
        shape = tuple(self.weight.shape)
        for k in ("weight", "exp_avg", "exp_avg_sq"):
            if tuple(state[k].shape) != shape:
                raise ValueError(f"FeatureTable.load_state_dict: {k} has shape {tuple(state[k].shape)}, this table {shape}")
        ams = bool(state["amsgrad"])
        if ams and (state.get("max_exp_avg_sq") is None or tuple(state["max_exp_avg_sq"].shape) != shape):
            raise ValueError("FeatureTable.load_state_dict: an amsgrad state needs max_exp_avg_sq of the table's shape")
        tr = state.get("trainable")
        if tr is not None and tuple(tr.shape) != (shape[0],):
            raise ValueError("FeatureTable.load_state_dict: trainable has one entry per table row")
        self.weight.copy_(state["weight"])
        self.exp_avg.copy_(state["exp_avg"])
        self.exp_avg_sq.copy_(state["exp_avg_sq"])
        if ams:
            if self.max_exp_avg_sq is None:
                self.max_exp_avg_sq = torch.zeros_like(self.weight)
            self.max_exp_avg_sq.copy_(state["max_exp_avg_sq"])
        else:
            self.max_exp_avg_sq = None
        self.trainable = None if tr is None else tr.to(device=self.device, dtype=torch.uint8).contiguous()
        self.amsgrad, self.step_count = ams, int(state["step"])
        self.lr, self.betas, self.eps = float(state["lr"]), (float(state["betas"][0]), float(state["betas"][1])), float(state["eps"])
        torch.autograd.graph.increment_version(self.weight)
        self._leaves = None
        with torch.cuda.device(self.device):
            self.updated.record(torch.cuda.current_stream(self.device))

    @torch.no_grad()
    def write_back(self, dataset=None):
        """ONE device-to-host copy of the table into dataset.node_features (default: the table's own dataset; in place, so whatever
        shares that tensor -- the graph dataset's g_full.ndata["x"] when the embeddings are not normalised -- sees it too), and the rows
        dataset.kv holds are refreshed from it: evaluate / infer / retrieve and the host sampler's test_topk path then serve the trained
        vectors.  A dataset whose table has another shape is refused."""
        dataset = self.dataset if dataset is None else dataset
        if tuple(dataset.node_features.shape) != tuple(self.weight.shape):
            raise ValueError(f"FeatureTable.write_back: the dataset's table is {tuple(dataset.node_features.shape)}, this one "
                             f"{tuple(self.weight.shape)}")
        host = self.weight.cpu()
        dataset.node_features.copy_(host)
        kv = getattr(dataset, "kv", None)
        if kv is not None:
            kv.add([str(i) for i in range(host.shape[0])], host.numpy(), replace=True)
        return dataset

    @torch.no_grad()
    def refresh(self, loader):
        """make a loader over ANOTHER dataset of the same taxonomy (the validation loader) serve this table: write_back into its dataset,
        and a device-to-device copy into its resident table (DeviceBatchLoader.features) when that is not this table's storage"""
        ds = getattr(loader, "dataset", None)
        if ds is not None and hasattr(ds, "node_features") and tuple(ds.node_features.shape) == tuple(self.weight.shape):
            self.write_back(ds)
        feats = getattr(loader, "features", None)
        if torch.is_tensor(feats) and feats.is_cuda and feats.data_ptr() != self.weight.data_ptr() and feats.shape == self.weight.shape:
            feats.copy_(self.weight)
            torch.cuda.current_stream(feats.device).synchronize()      # (that loader's side stream orders itself against nothing)
