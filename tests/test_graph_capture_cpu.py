"""`_lib.graph_capture` without a device: the collector is off inside the capture and back on after it, whatever happens inside;
and it is the package's only way into `torch.cuda.graph` (tests/test_graph_capture_gpu.py says why)."""
import ast
import gc
import os

import pytest
import torch


def test_collector_is_off_inside_and_back_on_afterwards(monkeypatch):
    from understanding_flow_robustness_amd import _lib as L
    seen = []

    class _Capture:                                # stands in for torch.cuda.graph: no device here
        def __init__(self, graph, **kwargs):
            seen.append(("made", graph, kwargs))

        def __enter__(self):
            seen.append(("enter", gc.isenabled()))

        def __exit__(self, *exc):
            seen.append(("exit", gc.isenabled()))
            return False

    monkeypatch.setattr(torch.cuda, "graph", _Capture)
    assert gc.isenabled()
    with L.graph_capture("g", pool=None):
        assert not gc.isenabled()
    assert gc.isenabled()
    assert seen == [("made", "g", {"pool": None}), ("enter", False), ("exit", False)]
    with pytest.raises(ValueError):
        with L.graph_capture("g"):
            raise ValueError("inside the capture")
    assert gc.isenabled()
    gc.disable()                                   # a caller that runs with the collector off keeps it off
    try:
        with L.graph_capture("g"):
            pass
        assert not gc.isenabled()
    finally:
        gc.enable()


def test_the_package_captures_through_graph_capture_only():
    """`ast` over the package: `torch.cuda.graph(` appears in _lib.graph_capture and nowhere else."""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "understanding_flow_robustness_amd")
    found = []
    for base, _, names in os.walk(root):
        for name in names:
            if not name.endswith(".py"):
                continue
            path = os.path.join(base, name)
            with open(path) as fh:
                tree = ast.parse(fh.read(), path)
            for node in ast.walk(tree):
                if isinstance(node, ast.Call) and ast.unparse(node.func) == "torch.cuda.graph":
                    found.append(os.path.relpath(path, root))
    assert found == ["_lib.py"], found
