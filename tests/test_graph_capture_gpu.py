"""`_lib.graph_capture`: every graph capture of the package goes through it.  torch.cuda.graph no longer collects garbage before a
capture begins, and a dead reference cycle that holds a torch.cuda.CUDAGraph, destroyed by the cyclic collector INSIDE a later
capture, ends the process (`~CUDAGraph` calls into HIP: 'operation not permitted when stream is capturing', thrown from a
destructor).  The GPU suite died that way once, inside PatchAttackStep._capture's capture of a whole iteration."""
import gc
import weakref

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _Holder:
    """A reference cycle around a captured graph: what a finished attack step is to the collector."""

    def __init__(self, graph):
        self.graph, self.me = graph, self


def test_capture_collects_dead_graphs_first_and_holds_the_collector_off():
    from understanding_flow_robustness_amd import _lib as L
    x = torch.zeros(64, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x.add_(1.0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    was_enabled = gc.isenabled()
    gc.disable()                                  # nothing collects the cycle below before graph_capture does
    try:
        old = torch.cuda.CUDAGraph()
        with L.graph_capture(old):
            x.add_(1.0)
        dead = weakref.ref(_Holder(old))
        del old
        assert dead() is not None                 # a dead cycle: only the collector can free it
        gc.enable()
        new = torch.cuda.CUDAGraph()
        with L.graph_capture(new):
            assert dead() is None, "the dead graph must be gone before the capture begins"
            assert not gc.isenabled(), "no cyclic collection inside a capture"
            x.add_(1.0)
        assert gc.isenabled()
        x.zero_()
        new.replay()
        torch.cuda.synchronize()
        assert float(x.sum()) == 64.0
    finally:
        (gc.enable if was_enabled else gc.disable)()
