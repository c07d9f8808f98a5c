"""TEST INFRASTRUCTURE: one rank of a world-size-N job on cuda:0 over gloo (launched by tests/test_gpu_topk_wide.py through
torch.distributed.run): the candidate-sharded best-k for k = 20 (every rank's [Q, 20] lists all-gathered and merged in rounds of 8
under a ceiling, txe_topk_merge_wide) against the unsharded selection of the same process, BIT FOR BIT, for LBM and MLP.  Prints
"OK <rank>"."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from taxoexpan_amd.model_zoo import LBM, MLP
    from taxoexpan_amd.scoring import shard_bounds, topk_parents_fused
    G, Q, l, r, H, k = 3001, 77, 50, 25, 40, 20
    gen = torch.Generator().manual_seed(123)
    hg = (torch.randn(G, l, generator=gen) * 0.3).to(dev)
    hg[1700:1712] = hg[5]                                   # a tie group of 13 across the shards and across a round's end
    queries = torch.nn.functional.normalize(torch.randn(Q, r, generator=gen), dim=1).to(dev)
    lo, hi = shard_bounds(G, world, rank)
    for make in (lambda: LBM(l, r), lambda: MLP(l, r, H)):
        torch.manual_seed(7)
        m = make().to(dev)
        with torch.no_grad():
            for larger in (True, False):
                want = topk_parents_fused(m, hg, queries, None, k, larger, block=32, return_scores=True)
                got = topk_parents_fused(m, hg[lo:hi], queries, None, k, larger, block=32, shard_lo=lo, sharded=True, return_scores=True)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), ("topk", type(m).__name__, larger)
    torch.cuda.synchronize()
    dist.barrier()
    print(f"OK {rank}", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
