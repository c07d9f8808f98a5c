"""The generated cases of the in-batch loss tests (tests/test_in_batch_cpu.py checks their properties, tests/test_gpu_in_batch.py runs
the kernel on them), their float64 restatement and the torch fp32 yardstick, each computed once per case."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
N_NODES = 2000
MASK_LENS = (0, 1, 63, 64, 65, 300)
BIT_COLS = 65536            # IB_BIT_COLS of csrc/txe_inbatch.hip: rows up to here keep their validity bits in LDS, longer rows search again
# (Q, G, first mask length (index into MASK_LENS) of the case's ordinary rows, has an all-masked last row)
SHAPES = {"1x1": (1, 1, 0, False), "1x2": (1, 2, 0, False), "3x12": (3, 12, 1, True), "5x65": (5, 65, 3, True), "7x257": (7, 257, 0, True),
          "4x1025": (4, 1025, 5, True), "2x65536": (2, BIT_COLS, 2, False), "1x65600": (1, BIT_COLS + 64, 5, False)}
ISSUE_SHAPES = ("1x1", "1x2", "3x12", "5x65", "7x257", "4x1025")


def _csr(rows):
    """{node: sorted ids} -> (mask_ptr [N_NODES + 1], mask_idx) int32"""
    cnt = np.zeros(N_NODES, dtype=np.int64)
    for v, r in rows.items():
        cnt[v] = len(r)
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    idx = np.zeros(int(ptr[-1]), dtype=np.int32)
    for v, r in rows.items():
        idx[ptr[v]:ptr[v + 1]] = r
    return ptr, idx


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(S fp32 [Q, G + 3] with NaN behind column G, S_plain (the same without the NaN / +Inf planted in masked columns), pos_col,
    anchor, qnode, mask_ptr, mask_idx, Q, G, and `rows`: per query row what was planted -- length of its mask row, the columns dup (the positive's anchor again: masked), last (the row's last entry: masked),
    below / above (misses just outside the row: valid), all_masked)"""
    Q, G, len0, with_all_masked = SHAPES[name]
    rng = np.random.default_rng(sum(ord(c) for c in name) * 7919)
    anchor = rng.integers(0, N_NODES, size=G).astype(np.int32)
    qnode = (7 * np.arange(Q) + 3).astype(np.int32)[::-1].copy()          # (descending: the CSR rows are not met in order)
    free = list(rng.permutation(G))
    pos_col = np.asarray([free.pop() for _ in range(Q)], dtype=np.int32)
    masks, rows = {}, []
    n_plain = Q - 1 if with_all_masked else Q
    S = np.full((Q, G + 3), np.nan, dtype=np.float32)
    S[:, :G] = rng.uniform(-6.0, 6.0, size=(Q, G)).astype(np.float32)
    for i in range(n_plain):
        L = MASK_LENS[(len0 + i) % len(MASK_LENS)]
        row = np.sort(rng.choice(np.arange(100, N_NODES - 100), size=L, replace=False)).astype(np.int32)
        masks[int(qnode[i])] = row
        info = dict(L=L, dup=None, last=None, below=None, above=None, all_masked=False)
        if L >= 1 and G >= 2:
            anchor[pos_col[i]] = row[0]                                   # the positive's own anchor, the row's FIRST entry: stays valid
            take = lambda: int(free.pop()) if free else None
            for key, a in (("dup", row[0]), ("last", row[-1]), ("below", row[0] - 1), ("above", row[-1] + 1)):
                c = take()
                if c is not None:
                    anchor[c], info[key] = a, c
        rows.append(info)
    if G >= 4:
        a, b = (int(free.pop()) for _ in range(2)) if len(free) >= 2 else (None, None)
        if a is not None:
            anchor[b] = anchor[a]                                         # a duplicate anchor whatever the draw
    if name == "1x2":
        S[0, :2] = (1e4, 1e4 - 1)                                         # finite only with the maximum taken off
    if with_all_masked:                                                   # the last row: every anchor of the batch is in its mask row
        masks[int(qnode[Q - 1])] = np.unique(anchor).astype(np.int32)
        rows.append(dict(L=len(masks[int(qnode[Q - 1])]), dup=None, last=None, below=None, above=None, all_masked=True))
    if G == 1:
        rows[0]["all_masked"] = True                                      # (nothing but the positive)
    mask_ptr, mask_idx = _csr(masks)
    from taxoexpan_amd.loss import host_in_batch_valid
    valid = host_in_batch_valid(pos_col, anchor, qnode, mask_ptr, mask_idx)
    S_plain = S.copy()                                                    # (for the runs without masks: nothing special planted)
    for i in range(Q):                                                    # NaN and +Inf where the row is masked
        gone = np.flatnonzero(~valid[i])
        if len(gone) >= 1:
            S[i, gone[0]] = np.nan
        if len(gone) >= 2:
            S[i, gone[1]] = np.inf
    for a in (S, S_plain, pos_col, anchor, qnode, mask_ptr, mask_idx):
        a.setflags(write=False)
    return dict(name=name, Q=Q, G=G, S=S, S_plain=S_plain, pos_col=pos_col, anchor=anchor, qnode=qnode, mask_ptr=mask_ptr, mask_idx=mask_idx, rows=rows)


@functools.lru_cache(maxsize=None)
def reference(name, masked=True):
    """the float64 restatement and the torch fp32 yardstick of a case, once: dict(valid, loss, d, n_valid, row_loss, lse, e_row (the
    yardstick's error per row), e_d (per gradient element), row_gate, d_gate (chain_exp 0; times max(1, |S|) under chain_exp))"""
    from taxoexpan_amd.loss import host_in_batch_nce, host_in_batch_valid
    c = case(name)
    G, S = c["G"], np.array((c["S"] if masked else c["S_plain"])[:, :c["G"]])
    mp, mi = (c["mask_ptr"], c["mask_idx"]) if masked else (None, None)
    valid = host_in_batch_valid(c["pos_col"], c["anchor"], c["qnode"], mp, mi)
    loss, d, n_valid = host_in_batch_nce(S, c["pos_col"], c["anchor"], c["qnode"], mp, mi)
    tgt = torch.from_numpy(c["pos_col"].astype(np.int64))
    fill = lambda dtype: torch.where(torch.from_numpy(np.array(valid)), torch.from_numpy(S).to(dtype), torch.tensor(-np.inf, dtype=dtype))
    x64 = fill(torch.float64).requires_grad_(True)
    row64 = F.cross_entropy(x64, tgt, reduction="none")
    row64.sum().backward()
    x32 = fill(torch.float32).requires_grad_(True)
    row32 = F.cross_entropy(x32, tgt, reduction="none")
    row32.sum().backward()
    row_loss = row64.detach().numpy()
    with np.errstate(invalid="ignore"):
        e_row = np.abs(row32.detach().numpy().astype(np.float64) - row_loss)
        e_d = np.where(valid, np.abs(x32.grad.numpy().astype(np.float64) - x64.grad.numpy()), 0.0)
    s_pos = S[np.arange(c["Q"]), c["pos_col"]].astype(np.float64)
    lse = row_loss + s_pos
    row_gate = np.maximum(2 * e_row, (n_valid + 16) * EPS * np.maximum(1.0, np.maximum(np.abs(lse), np.abs(s_pos))))
    d_gate = np.maximum(2 * e_d, 8 * EPS * np.maximum(1.0, np.abs(d)))
    return dict(valid=valid, loss=loss, d=d, n_valid=n_valid, row_loss=row_loss, torch_d=x64.grad.numpy(), lse=lse, e_row=e_row, e_d=e_d,
                row_gate=row_gate, d_gate=d_gate)


def foreign_masked(Q, k, seed=3):
    """a [Q, 1 + k] grouped batch laid out as the device sampler lays it out, with every foreign column masked: column i (1 + k) + j has
    the anchor 100 i + j and query i's mask row holds every other group's anchors.  dict like case(), plus k"""
    rng = np.random.default_rng(seed)
    G = Q * (1 + k)
    anchor = (100 * np.repeat(np.arange(Q), 1 + k) + np.tile(np.arange(1 + k), Q)).astype(np.int32)
    qnode = (5 * np.arange(Q) + 1).astype(np.int32)
    pos_col = (np.arange(Q) * (1 + k)).astype(np.int32)
    own = np.repeat(np.arange(Q), 1 + k)
    mask_ptr, mask_idx = _csr({int(qnode[i]): np.sort(anchor[own != i]) for i in range(Q)})
    S = rng.uniform(-6.0, 6.0, size=(Q, G)).astype(np.float32)
    return dict(Q=Q, G=G, k=k, S=S, pos_col=pos_col, anchor=anchor, qnode=qnode, mask_ptr=mask_ptr, mask_idx=mask_idx)
