"""Worker of tests/test_dpmpp_mis_emulated.py: one gloo rank of a W-rank ``DPMSolverSamplerInst.sample()`` over the CPU op emulation
-- the tiny_box case at order 2 with a mask, exactly the call the test then makes in one process.  Started with multiprocessing's
``spawn``; puts (rank, result as numpy, number of draws this rank made) on the queue."""
import os

import torch


def run(rank, world, port, q, threads):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    torch.set_num_threads(threads)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from tests import test_dpmpp_mis_emulated as t
    from tests import dpmpp_cases as dc
    meta, inp, _, _, _ = t.env()
    noises = dc.make_noises(tuple(inp["x"].shape), dc.S, True)
    if rank != 0:
        # only rank 0's draws may count: every other rank feeds other values through its noise_fn
        noises = [n + float(rank) for n in noises]
    out, drawn = t.run(t.sampler_for(), 2, True, noises=noises)
    q.put((rank, out.numpy().copy(), drawn))          # by value: a tensor would travel as a handle that dies with this process
    dist.barrier()
    dist.destroy_process_group()
