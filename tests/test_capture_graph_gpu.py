"""``engine.capture_graph``: the hipGraph capture of both engines runs with the cyclic garbage collector held off (a dead cycle
finalised between two captured launches aborted a sampler test of the GPU suite), and gives it back afterwards."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_capture_graph_keeps_the_collector_out_and_restores_it():
    from instancediffusion_amd.engine import capture_graph
    x = torch.zeros(8, device="cuda")
    x.add_(0)                                                # warm-up outside the capture
    torch.cuda.synchronize()
    graph, seen = torch.cuda.CUDAGraph(), []
    assert gc.isenabled()
    with capture_graph(graph):
        seen.append(gc.isenabled())
        x.add_(1)
    assert seen == [False] and gc.isenabled()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert bool((x == 2).all())
    gc.disable()                                             # a caller that runs without the collector keeps it off
    try:
        with capture_graph(torch.cuda.CUDAGraph()):
            x.add_(1)
        assert not gc.isenabled()
    finally:
        gc.enable()
