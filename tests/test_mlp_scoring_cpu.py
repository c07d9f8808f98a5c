"""CPU: the MLP matcher's all-candidate entry points (txe_mlp_*) reject bad arguments before touching a device, and the candidate-sharded
scoring / ranking logic runs an MLP matcher with injected local functions (the collectives over gloo, world 2)."""
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import txe_oracle as orc

P_ = 0x1000          # a non-NULL pointer value that is never dereferenced: every call below fails its argument checks first


def test_mlp_entry_points_reject_bad_arguments_without_a_device():
    from taxoexpan_amd import _lib
    lib = _lib.load()
    assert lib.txe_mlp_padded_h(500) == 512 and lib.txe_mlp_padded_h(1) == 16 and lib.txe_mlp_padded_h(33) == 48 and lib.txe_mlp_padded_h(0) == 0
    p = P_
    assert lib.txe_mlp_project(p, 4, 10, 0, p, p, p, p, p, None) == -1            # H < 1
    assert lib.txe_mlp_project(p, 3, 10, 4, p, p, p, p, p, None) == -1            # ld_a < H
    assert lib.txe_mlp_project(p, 4, -1, 4, p, p, p, p, p, None) == -1            # G < 0
    assert lib.txe_mlp_project(p, 4, 10, 4, None, p, p, p, p, None) == -1         # no w2
    assert lib.txe_mlp_query_project(p, 2, 5, 3, p, 4, p, p, p, p, None) == -1     # ld_q < r
    assert lib.txe_mlp_query_project(p, 3, -1, 3, p, 4, p, p, p, p, None) == -1
    assert lib.txe_mlp_query_project(p, 3, 5, 3, p, 0, p, p, p, p, None) == -1
    assert lib.txe_mlp_score_block(p, p, 10, p, p, p, 5, 0, p, p, 12, None) == -1            # H < 1
    assert lib.txe_mlp_score_block(p, p, 10, p, p, p, 5, 4, p, p, 8, None) == -1             # ld_s < G
    assert lib.txe_mlp_score_block(p, p, -2, p, p, p, 5, 4, p, p, 12, None) == -1
    assert lib.txe_mlp_score_block(p, None, 10, p, p, p, 5, 4, p, p, 12, None) == -1         # no candidate flags
    assert lib.txe_mlp_score_positives(p, p, 10, p, p, p, 5, 4, p, None, p, 3, p, None) == -1
    assert lib.txe_mlp_score_positives(p, p, 10, p, p, p, 5, 4, p, p, p, -1, p, None) == -1
    assert lib.txe_mlp_score_count_block(p, p, 10, p, p, p, 5, 4, p, p, None, 1, p, None) == -1
    assert lib.txe_mlp_score_count_block(p, p, 10, p, p, p, -5, 4, p, p, p, 1, p, None) == -1
    for k in (0, 9):
        assert lib.txe_mlp_score_topk_block(p, p, 10, p, p, p, 5, 4, p, 1, k, 0, p, p, p, p, p, None) == -1
    assert lib.txe_mlp_score_topk_block(p, p, 0, p, p, p, 5, 4, p, 1, 5, 0, p, p, p, p, p, None) == -1      # no candidates
    assert lib.txe_mlp_score_topk_block(p, p, 10, p, p, p, 5, 4, p, 1, 5, 0, None, p, p, p, p, None) == -1
    # nothing to do: success without a launch
    assert lib.txe_mlp_score_block(p, p, 10, p, p, p, 0, 4, p, p, 12, None) == 0
    assert lib.txe_mlp_score_count_block(p, p, 0, p, p, p, 5, 4, p, p, p, 1, p, None) == 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _mlp_host(match, hg, q):
    W1, b1, w2, b2 = (t.detach() for t in (match.ffn[0].weight, match.ffn[0].bias, match.ffn[2].weight, match.ffn[2].bias))
    return torch.stack([orc.mlp_match(hg, qq.expand(hg.shape[0], -1), W1, b1, w2, b2).squeeze(1) for qq in q]) if q.shape[0] else \
        torch.zeros((0, hg.shape[0]))


def _worker(rank, world, port, G, Q, ret):
    from taxoexpan_amd import scoring
    from taxoexpan_amd.model_zoo import MLP
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    torch.manual_seed(3)
    l, r = 7, 5
    m = MLP(l, r, 6)
    gen = torch.Generator().manual_seed(1)
    hg = torch.randn(G, l, generator=gen)
    q = torch.randn(Q, r, generator=gen)
    rs = np.random.RandomState(2)
    lists = [sorted(rs.choice(G, size=1 + i % 3, replace=False).tolist()) for i in range(Q)]
    pos_off = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int64)
    pos_idx = np.concatenate(lists).astype(np.int64)
    lo, hi = scoring.shard_bounds(G, world, rank)
    hl = hg[lo:hi]

    def local_score(qb, out):
        out[:, :hi - lo] = _mlp_host(m, hl, qb)

    S_sh = scoring.score_all_sharded(m, hl, G, q, block=4, local_score_fn=local_score)
    S = _mlp_host(m, hg, q)

    def fns(rows, base):
        def f_thr(qb, off, idx_local):
            Sb = _mlp_host(m, rows, qb)
            qid = torch.repeat_interleave(torch.arange(qb.shape[0]), (off[1:] - off[:-1]).long())
            ok = idx_local >= 0
            return torch.where(ok, Sb[qid, idx_local.long().clamp(min=0)], torch.zeros(()))

        def f_cnt(qb, off, thr):
            Sb = _mlp_host(m, rows, qb)
            qid = torch.repeat_interleave(torch.arange(qb.shape[0]), (off[1:] - off[:-1]).long())
            return (Sb[qid] > thr[:, None]).sum(1).to(torch.int32)
        return f_thr, f_cnt
    got = scoring.rank_all_fused(m, hl, q, pos_off, pos_idx, block=4, shard_lo=lo, local_fns=fns(hl, lo), sharded=True)
    solo = scoring.rank_all_fused(m, hg, q, pos_off, pos_idx, block=4, local_fns=fns(hg, 0))
    want = np.concatenate([orc.ranks_of_positives(S[i].numpy(), pos_idx[pos_off[i]:pos_off[i + 1]]) for i in range(Q)])
    ret[rank] = (torch.allclose(S_sh, S, rtol=1e-5, atol=1e-6),     # (host products of other row counts round differently)
                  bool(torch.equal(got, solo)), bool(np.array_equal(got.numpy(), want)))
    dist.destroy_process_group()


def test_sharded_scoring_and_ranking_of_an_mlp_matcher_world2():
    for G, Q in ((23, 9), (5, 3)):
        ret = mp.Manager().dict()
        mp.spawn(_worker, args=(2, _free_port(), G, Q, ret), nprocs=2, join=True)
        assert ret[0] == (True, True, True) and ret[1] == (True, True, True), dict(ret)
