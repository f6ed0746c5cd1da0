"""Robust FlowNetC's patch-attack iteration (FlowNetCFlexLarger_k3_reps3, the CVPR'22 paper's model) on the engines: bench.py's C2
workload -- 384 x 1280, 8 pairs behind one 51 x 51 circular patch, attack() calls of max_count = 2 with new frames and placements
per call (load: paste, window placement, full-frame prefix; then the captured iterations) -- with the prefix on the 280 x 280
window around the patch and as the full-frame step (UFR_CONE=0's form), in one process, alternating.  One JSON line.

    python tools/bench_flownetc_flex.py [--steps K] [--warmup W] [--rounds R] [--only windowed|full]

--only runs one form (K iterations after the warm-up), e.g. under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import sys
import time
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402

NAME = "FlowNetCFlexLarger_k3_reps3"


def make_step(net, args, cone, device):
    from understanding_flow_robustness_amd.flownets.utils_model import predict_flow
    from understanding_flow_robustness_amd.patch_attack import PatchAttackStep
    B, P = bench.B_PER_GPU, bench.PATCH
    step = PatchAttackStep(net, args, B, bench.H, bench.W, device=device, shared_patch=True, use_graph=True, warmup=2,
                           patch_hw=(P, P), use_cone=cone)
    g = torch.Generator().manual_seed(7)
    patch0 = torch.rand(1, 3, P, P, generator=g).to(device)
    mask_p = bench.circle_mask(P).expand(1, 3, P, P).contiguous().to(device)
    batches = []
    for k in range(2):
        tgt, ref, origins = bench.synthetic_batch(B, 1000 + 17 * k, device)
        with torch.no_grad():
            target = -torch.cat([predict_flow(net, None, tgt[i:i + 1], ref[i:i + 1], args) for i in range(B)])   # main.py:395
        batches.append(((tgt, ref, patch0, mask_p, patch0, target), origins))
    load = lambda call: step.load(*batches[call % 2][0], origins=batches[call % 2][1])
    load(0)
    step.run(0)                                   # warm-up + graph capture, reloads operands
    return step, load


def timed(step, load, iterations, mc, first_call):
    """ms per iteration of `iterations` iterations as attack() calls of `mc` (nothing read back inside the timed region)."""
    executed = torch.zeros(1, device=step.dev)
    torch.cuda.synchronize(step.dev)
    t0 = time.perf_counter()
    call, left = first_call, iterations
    while left > 0:
        load(call)
        n = min(mc, left)
        step.enqueue(n)
        executed.add_(step.state[1])
        call, left = call + 1, left - n
    torch.cuda.synchronize(step.dev)
    ms = (time.perf_counter() - t0) * 1e3 / iterations
    if int(executed) != iterations:
        raise SystemExit(f"only {int(executed)} of {iterations} iterations took effect (loss gate tripped)")
    return ms, call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=("windowed", "full"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flownetc_flex.py needs an MI355X: the product path has no CPU fallback")
    from understanding_flow_robustness_amd import _lib as L
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    device = torch.device("cuda:0")
    args = Namespace(flownet=NAME, l2=False, alpha=0.0, lr=1000.0, max_count=2)
    net = fetch_model(args, synthetic_seed=0).to(device)
    forms = [f for f in ("windowed", "full") if opt.only in (None, f)]
    steps = {f: make_step(net, args, f == "windowed", device) for f in forms}
    calls = {f: 0 for f in forms}
    for f in forms:                                # warm-up calls of each form
        _, calls[f] = timed(*steps[f], opt.warmup, args.max_count, calls[f])
    times = {f: [] for f in forms}
    for _ in range(opt.rounds):                    # the forms alternate: drift of the box's clock hits both alike
        for f in forms:
            ms, calls[f] = timed(*steps[f], opt.steps, args.max_count, calls[f])
            times[f].append(ms)
    win = steps.get("windowed", (None,))[0]
    line = dict(model=NAME, pairs=bench.B_PER_GPU, hw=[bench.H, bench.W], patch=bench.PATCH, max_count=args.max_count,
                steps_per_round=opt.steps, rounds=opt.rounds,
                **{f"{f}_ms_per_iteration": round(sorted(v)[len(v) // 2], 3) for f, v in times.items()},
                **{f"{f}_ms_rounds": [round(x, 3) for x in v] for f, v in times.items()},
                window_hw=list(win.win_hw) if win is not None else None,
                band_width=(win.band.width if win is not None and win.band is not None else None),
                vendor_fallbacks={f"{k[0]}: {k[1]}": v for k, v in L.VENDOR_FALLBACKS.items()},
                device=torch.cuda.get_device_name(device))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
