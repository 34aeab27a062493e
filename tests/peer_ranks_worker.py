"""Several ranks of the sharded sweep on ONE GPU, one PROCESS per rank (run by tests/test_gpu_multi.py through
torch.distributed.run, gloo rendezvous): every rank is a context with its own stream and its own shard of the
market, the symmetric buffers are the library's IPC export (dist.open_peer_buffers).  One rank per process gives
every rank's stream a hardware queue of its own, which the ranks' waiting launches need.  Checks, over 30
evaluations with alternating launch order: every rank's {Psi, acc} is finite, bit-identical across ranks, and
equal to the rank-ordered sum of the ranks' local results."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import torch.distributed as dist

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth
from cfmmrouter_amd.dist import open_peer_buffers, shard_batches
from helpers import oracle_sweep, rel_to_max

torch.cuda.set_device(0)
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
n = 512
market = [synth.product_pools(240_000, n, seed=71), synth.geomean_pools(80_000, n, seed=72)]
count = n + 1
be = cr.DeviceBackend(n, shard_batches(market, rank, world))
be.ctx.set_option("alternate", 0)   # local and sharded sweeps are compared bit for bit: same tile direction every time
peer = open_peer_buffers(be.ctx, None, torch.device("cuda", 0))
assert peer is not None, "no rank-to-rank mapping of the peer buffers"
out = torch.zeros(count, dtype=torch.float64, device="cuda")
loc = torch.zeros(count, dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
seq = 0
for it in range(30):
    v = synth.sweep_prices(n, seed=700 + it)
    vt = torch.from_numpy(v).cuda()
    torch.cuda.synchronize()
    be.ctx.set_peers([], 0, 0, 0)                      # local result first (sharding off)
    be.ctx.sweep_dev(vt.data_ptr(), loc.data_ptr(), it % 2 == 0)
    torch.cuda.synchronize()
    locs = [torch.zeros(count, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(locs, loc.cpu())
    want = locs[0].clone()
    for r in range(1, world):
        want += locs[r]                                # rank order, as reduce_gather adds
    be.ctx.set_peers(list(peer.ptrs), world, rank, seq)
    dist.barrier()
    position = rank if it % 3 else world - 1 - rank    # launch order must not matter
    time.sleep(0.002 * position)
    be.ctx.sweep_dev(vt.data_ptr(), out.data_ptr(), it % 2 == 0)
    torch.cuda.synchronize()
    seq += 1
    got = out.cpu()
    assert bool(torch.isfinite(got).all()), ("timeout", it, rank)
    assert torch.equal(got, want), ("mismatch", it, rank)
    outs = [torch.zeros(count, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(outs, got)
    assert all(torch.equal(o, got) for o in outs), ("ranks differ", it, rank)
if rank == 0:
    psi_o = oracle_sweep(market, n, v, nthreads=8)[2]
    assert rel_to_max(out.cpu().numpy()[:n], psi_o) <= 1e-12
peer.close()
be.close()
dist.barrier()
dist.destroy_process_group()
print(f"PEER_RANKS_OK world={world} rank={rank}", flush=True)
