"""CPU: the host restatement of the retrieval stage (scoring.host_retrieve / host_select_k) -- against the test-mode sampler that
tests/test_dataset.py pins call for call to the reference (data_loader/dataset.py:316-330), and its order, tie, mask and argument
rules on hand-made rows."""
import os
import shutil

import numpy as np
import pytest
import torch

from golden_util import GOLDEN_DIR

MIN_GAP = 1e-5        # the smallest float64 gap between neighbouring distances that makes the order independent of fp32 rounding


@pytest.fixture(scope="module")
def raw(tmp_path_factory):
    from taxoexpan_amd.dataset import MAGDataset
    d = tmp_path_factory.mktemp("toy_retrieval")
    for fn in os.listdir(os.path.join(GOLDEN_DIR, "toy_taxo")):
        shutil.copy(os.path.join(GOLDEN_DIR, "toy_taxo", fn), d)
    return MAGDataset(name="toy", path=str(d), raw=True)


def toy_masks(ds, cand):
    """node2masks of every query as candidate rows (CSR), unsorted on purpose: set order"""
    index = {a: i for i, a in enumerate(cand)}
    off, idx = [0], []
    for q in ds.node_list:
        idx += [index[a] for a in ds.node2masks[q] if a in index]
        off.append(len(idx))
    return np.asarray(off), np.asarray(idx, dtype=np.int64)


def sorted_pool_gaps(ds, cand, q, k):
    """float64 cosine distances of query q's unmasked pool, sorted: the gaps between the first k + 1 of them"""
    x = ds.node_features.numpy().astype(np.float64)
    pool = [a for a in cand if a not in ds.node2masks[q]]
    m, v = x[pool], x[q]
    d = np.sort(1.0 - (m @ v) / (np.linalg.norm(m, axis=1) * np.linalg.norm(v)))
    assert len(pool) > k                                          # the pool is never exhausted on this set
    return np.diff(d[:k + 1])


@pytest.mark.parametrize("normalize_embed", [False, True])
@pytest.mark.parametrize("k", [5, 16, 64])
def test_host_retrieve_equals_the_test_mode_sampler(raw, normalize_embed, k):
    from taxoexpan_amd.dataset import MaskedGraphDataset
    from taxoexpan_amd.scoring import host_retrieve
    ds = MaskedGraphDataset(raw, mode="test", sampling_mode=0, expand_factor=100, normalize_embed=normalize_embed, test_topk=k)
    cand = sorted(ds.all_positions)
    assert len(cand) == 134 and len(ds.node_list) == 8
    off, idx = toy_masks(ds, cand)
    # precondition for exact equality: no two neighbouring distances among the first k + 1 closer than fp32 rounding can move them
    gap = min(float(sorted_pool_gaps(ds, cand, q, k).min()) for q in ds.node_list)
    print(f"k={k} normalize_embed={normalize_embed}: smallest gap {gap:.3e}")
    assert gap > MIN_GAP
    cf = ds.node_features[torch.as_tensor(cand)]
    qf = ds.node_features[torch.as_tensor(ds.node_list)]
    got = host_retrieve(qf, cf, k, off, idx)
    assert got.shape == (8, k) and got.dtype == np.int32
    for i, q in enumerate(ds.node_list):
        _q, inst = ds.sample(i)
        negatives = [a for a, label, *_ in inst if label == 0]
        assert [a for a, label, *_ in inst if label == 1] == ds.node2parents[q]
        assert [cand[j] for j in got[i]] == negatives, (q, k)


def test_duplicated_rows_come_out_in_ascending_column_order():
    from taxoexpan_amd.scoring import host_retrieve, host_select_k
    # two non-zero entries per row: a dot product of two such rows is one rounded sum whatever order a BLAS adds the terms in, so
    # equal rows give bit-equal similarities
    base = np.array([[3.0, 4.0, 0.0], [0.0, 5.0, 12.0], [8.0, 0.0, 6.0], [0.0, 3.0, 4.0], [5.0, 12.0, 0.0]])
    cf = base[[3, 0, 3, 1, 3, 0, 2, 4, 3]]                            # rows 0, 2, 4, 8 are one vector; 1 and 5 another
    qf = base[[3, 0]]
    got = host_retrieve(qf, cf, 4)
    assert got[0].tolist() == [0, 2, 4, 8]
    assert got[1, :2].tolist() == [1, 5]
    S = np.array([[1.0, 2.0, 2.0, -0.0, 0.0, 2.0, 0.5]], dtype=np.float32)
    assert host_select_k(S, 2).tolist() == [[1, 2]]
    assert host_select_k(S, 7).tolist() == [[1, 2, 5, 0, 6, 3, 4]]     # -0.0 == +0.0: columns 3, 4 in order


def test_masks_padding_and_nan():
    from taxoexpan_amd.scoring import host_retrieve, host_select_k
    S = np.array([[0.1, 0.9, 0.5, 0.7],
                  [0.3, 0.2, 0.1, 0.0],
                  [np.nan, -np.inf, 0.0, np.nan]], dtype=np.float32)
    off = np.array([0, 5, 7, 7])
    idx = np.array([3, 0, 1, 2, 0, 1, 1])                             # row 0 fully masked (unsorted, a duplicate), row 1 masks 1, row 2 nothing
    got = host_select_k(S, 3, off, idx)
    assert got[0].tolist() == [-1, -1, -1]
    assert got[1].tolist() == [0, 2, 3]
    assert got[2].tolist() == [2, 0, 1]                               # NaN ranks with -inf: columns 0, 1, 3 in order behind the 0.0
    assert host_select_k(S, 6, off, idx)[1].tolist() == [0, 2, 3, -1, -1, -1]     # k above the unmasked count: the whole row, then -1
    assert host_select_k(S, 4)[2].tolist() == [2, 0, 1, 3]
    # a NaN (zero-norm) candidate row sorts last; a NaN query row returns the columns in order
    cf = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    qf = np.array([[1.0, 0.1], [0.0, 0.0]])
    got = host_retrieve(qf, cf, 4)
    assert got[0].tolist() == [1, 3, 2, 0]
    assert got[1].tolist() == [0, 1, 2, 3]
    assert host_retrieve(qf, cf, 2, np.array([0, 1, 2]), np.array([1, 0])).tolist() == [[3, 2], [1, 2]]
    assert host_retrieve(torch.as_tensor(qf), torch.as_tensor(cf), 2, block=1).tolist() == [[1, 3], [0, 1]]


def test_argument_errors():
    from taxoexpan_amd import scoring
    from taxoexpan_amd.evaluate import evaluate, infer
    cf = np.eye(3)
    qf = np.eye(3)[:2]
    for fn in (scoring.host_retrieve, scoring.retrieve_candidates):       # (the device entry point checks before it touches a tensor)
        for k in (0, -1, 4097):
            with pytest.raises(ValueError):
                fn(qf, cf, k)
        with pytest.raises(ValueError):
            fn(qf, cf, 2, mask_idx=np.array([0]))
        with pytest.raises(ValueError):
            fn(qf, cf, 2, mask_off=np.array([0, 0, 0]))
    with pytest.raises(ValueError):
        scoring.host_retrieve(qf, cf, 2, np.array([0, 1]), np.array([0]))         # Q + 1 offsets wanted
    with pytest.raises(ValueError):
        scoring.host_retrieve(qf, cf, 2, np.array([0, 1, 1]), np.array([3]))      # a column outside the candidates
    assert scoring.host_retrieve(qf, cf, 4096).shape == (2, 4096)
    for k in (0, 4097):
        with pytest.raises(ValueError):
            evaluate(None, None, "cpu", retrieve=k)
        with pytest.raises(ValueError):
            infer(None, None, None, "cpu", retrieve=k)


def test_select_k_entry_point_checks_k_before_any_device_work():
    """txe_select_k / txe_row_normalize return TXE_ERR_ARG for bad arguments without a device"""
    from taxoexpan_amd import _lib
    lib = _lib.load()
    for k in (0, -3, 4097):
        assert lib.txe_select_k(None, 8, 1, 8, None, None, k, None, None, None, 0, None) == -1
    assert lib.txe_select_k(None, 8, 1, 8, None, None, 4, None, None, None, 0, None) == -1       # NULL S
    assert lib.txe_select_k_ws_bytes(3, 65) == 3 * 3 * 4 and lib.txe_select_k_ws_bytes(0, 65) == 0
    assert lib.txe_row_normalize(None, 8, 1, 8, None, 8, None) == -1
