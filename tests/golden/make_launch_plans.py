"""Records the igemm launch plan of every native engine on the CPU (descriptors only hold pointers: no device is needed) and
writes `launch_plans_small.json`, the fixture of tests/test_launch_planner_cpu.py.

Per `igemm.make_launch` call, in call order:
    [long-form launch signature, in_chunk0, variant, splitk, ws.numel() | None, balance, resident, products,
     [out, out_f32, add, mask, tail chunk offsets], tail_plan.on | None]

    python tests/golden/make_launch_plans.py                          # rewrite the fixture (shapes of 64 x 128)
    python tests/golden/make_launch_plans.py --large --out plans.json  # the benchmark's shapes, for a before / after comparison

The fixture was recorded before the engines moved onto `igemm.LaunchQueue`; a pull request that changes a plan on purpose
re-records it and says so.
"""
import argparse
import contextlib
import json
import os
import sys
from argparse import Namespace
from types import SimpleNamespace

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from understanding_flow_robustness_amd import igemm as ig                                   # noqa: E402
from understanding_flow_robustness_amd.flownets.utils_model import fetch_model              # noqa: E402

FIXTURE = os.path.join(HERE, "launch_plans_small.json")
_OFFSETS = ("out_chunk0", "out_f32_chunk0", "add_chunk0", "mask_chunk0", "tail_chunk0")


@contextlib.contextmanager
def recording(calls: list):
    """Every `igemm.make_launch` inside appends its record to `calls`."""
    real = ig.make_launch

    def make_launch(wi, x, in_chunk0, rows, out_hw, **kw):
        launch = real(wi, x, in_chunk0, rows, out_hw, **kw)
        ws = kw.get("ws")
        calls.append([ig.launch_signature(wi, x.B * rows[0] * rows[1], kw, rows), int(in_chunk0), int(kw.get("variant", 0)),
                      int(kw.get("splitk", 1)), None if ws is None else int(ws.numel()), bool(kw.get("balance", False)),
                      kw.get("resident"), int(launch.desc.products), [int(kw.get(k, 0)) for k in _OFFSETS],
                      None if launch.tail_plan is None else int(launch.tail_plan.on)])
        return launch

    ig.make_launch = make_launch
    try:
        yield calls
    finally:
        ig.make_launch = real


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _net(name, seed):
    return fetch_model(Namespace(flownet=name), synthetic_seed=seed)


def _flownetc(name, B, H, W):
    from understanding_flow_robustness_amd.flownetc_engine import FlowNetCHeadEngine
    eng = FlowNetCHeadEngine(_net(name, 0), B, H, W, "cpu")
    eng._build_prefix()
    for wh, ww in ((96, 96), (64, 96)):
        eng.window_prefix(wh, ww)
    win = torch.zeros(B, 8, dtype=torch.int32)
    width, corr_width = (576, 416) if W >= 576 else (96, 64)
    for resident in (None, 12):            # (a small chip, so that small grids have a tail round)
        band = SimpleNamespace(win=win, width=width, corr_width=corr_width)
        if resident is not None:
            band.tail_resident = resident
        eng.attach_band(band)


def _flownets_trunk(B, H, W):
    """FlowNet2's FlowNetS sub-network (12 input channels): the head engine without the siamese front, and its stem's PlaneGraph.
    (A plan depends on shapes only, so the sub-networks keep their initial weights.)"""
    from understanding_flow_robustness_amd.flownetc_engine import FlowNetCHeadEngine
    from understanding_flow_robustness_amd.flownets.flownet2 import FlowNetS
    from understanding_flow_robustness_amd.plane_graph import stem_graph
    net = FlowNetS().eval()
    FlowNetCHeadEngine(net, B, H, W, "cpu")
    stem_graph(net, B, H, W, 12, "cpu")


def _flownet2_graphs(B, H, W):
    """FlowNet2's small-displacement and fusion sub-networks as PlaneGraphs."""
    from understanding_flow_robustness_amd.flownets.flownet2 import FlowNetFusion, FlowNetSD, _fusion_graph, _sd_graph
    _sd_graph(FlowNetSD().eval(), B, H, W, "cpu")
    _fusion_graph(FlowNetFusion().eval(), B, H, W, "cpu")


def _pwc(B, H, W):
    from understanding_flow_robustness_amd.pwc_engine import PwcHeadEngine, _PyramidPrefix
    eng = PwcHeadEngine(_net("PWCNet", 1), B, H, W, "cpu")
    _PyramidPrefix(eng, 2 * B, H, W, backward=False, f2_out=eng.F[2])
    _PyramidPrefix(eng, 2 * B, 32, 64, backward=True)


def _raft(B, H, W, products):
    from understanding_flow_robustness_amd.plane_graph import stem_graph
    from understanding_flow_robustness_amd.raft_encoder_engine import RaftEncoderEngine
    from understanding_flow_robustness_amd.raft_engine import RaftUpdateEngine
    net = _net("RAFT", 2)
    with ig.products(products), _env(UFR_RAFT_STREAMS="0"):
        RaftUpdateEngine(net, B, H, W, "cpu")
        RaftEncoderEngine(net.fnet, 2 * B, H, W, "cpu")
        RaftEncoderEngine(net.cnet, B, H, W, "cpu")
        wo = _net("RAFT_FlowNetCEncoder_WoContext", 4)
        stem_graph(wo.fnet, 2 * B, H, W, 3, "cpu", head=wo.conv_redir)


def cases(large: bool = False):
    """{name: thunk}: every engine at 64 x 128, or (large) at the benchmark's shapes."""
    big, one, fn2 = ((8, 384, 1280), (1, 384, 1280), (1, 448, 1024)) if large else ((1, 64, 128),) * 3
    tag = lambda s: "x".join(str(v) for v in s)
    out = {f"FlowNetC_{tag(big)}": lambda: _flownetc("FlowNetC", *big),
           f"FlowNetCFlexLarger_k3_reps3_{tag(big)}": lambda: _flownetc("FlowNetCFlexLarger_k3_reps3", *big),
           f"FlowNetS_trunk_{tag(fn2)}": lambda: _flownets_trunk(*fn2),
           f"FlowNet2_graphs_{tag(fn2)}": lambda: _flownet2_graphs(*fn2),
           f"PWCNet_{tag(big)}": lambda: _pwc(*big)}
    for p in (6, 1):
        out[f"RAFT_{tag(one)}_products{p}"] = lambda p=p: _raft(*one, p)
    return out


def record(large: bool = False, only=None) -> dict:
    plans = {}
    with torch.no_grad():
        for name, build in cases(large).items():
            if only is None or name in only:
                with recording([]) as calls:
                    build()
                plans[name] = calls
    return plans


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--large", action="store_true")
    ap.add_argument("--out", default=FIXTURE)
    a = ap.parse_args()
    plans = record(a.large)
    with open(a.out, "w") as f:
        json.dump(plans, f, separators=(",", ":"))
        f.write("\n")
    print({k: len(v) for k, v in plans.items()})
