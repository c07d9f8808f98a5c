"""TEST INFRASTRUCTURE: one rank of a world-size-N job on cuda:0 over gloo (launched by tests/test_gpu_mlp_scoring.py through
torch.distributed.run): the MLP matcher's candidate-sharded scoring loop (all-gathered score blocks, all-reduced counts, all-gathered
best-k lists) against the unsharded loop of the same process, BIT FOR BIT.  Prints "OK <rank>"."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from taxoexpan_amd.model_zoo import MLP
    from taxoexpan_amd.scoring import rank_all_fused, score_all, score_all_sharded, shard_bounds, topk_parents_fused
    G, Q, l, r, H = 3001, 77, 50, 25, 40
    torch.manual_seed(7)
    m = MLP(l, r, H).to(dev)
    gen = torch.Generator().manual_seed(123)
    hg = torch.randn(G, l, generator=gen).to(dev)
    hg[1700] = hg[5]                                        # a tie across the shards
    queries = torch.randn(Q, r, generator=gen).to(dev)
    rs = np.random.RandomState(0)
    lists = [sorted(rs.choice(G, size=1 + i % 3, replace=False).tolist()) for i in range(Q)]
    pos_off = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int64)
    pos_idx = np.concatenate(lists).astype(np.int64)
    lo, hi = shard_bounds(G, world, rank)
    with torch.no_grad():
        S = score_all(m, hg, queries)
        S_sh = score_all_sharded(m, hg[lo:hi], G, queries, block=32)
        assert torch.equal(S_sh, S), "scores"
        for larger in (True, False):
            want = rank_all_fused(m, hg, queries, pos_off, pos_idx, block=32, larger_is_better=larger)
            got = rank_all_fused(m, hg[lo:hi], queries, pos_off, pos_idx, block=32, larger_is_better=larger, shard_lo=lo, sharded=True)
            assert torch.equal(got, want), ("ranks", larger)
            for k in (1, 5, 8):
                want = topk_parents_fused(m, hg, queries, None, k, larger, block=32)
                got = topk_parents_fused(m, hg[lo:hi], queries, None, k, larger, block=32, shard_lo=lo, sharded=True)
                assert torch.equal(got, want), ("topk", k, larger)
    torch.cuda.synchronize()
    dist.barrier()
    print(f"OK {rank}", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
