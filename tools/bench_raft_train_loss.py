#!/usr/bin/env python3
"""RAFT's training loss from the low-resolution predictions: the fused pass (csrc/raft_train_loss.hip) against the unfused path, on one box.

    timeout 1100 python tools/bench_raft_train_loss.py [--height 384 --width 1280 --pairs 1 4 --preds 12 --out profiles/raft_train_loss.json]

For every pair count, two comparisons:
  1. the loss stage alone, from the 12 (flow, mask) pairs with gradients to the loss and all 24 gradients: `RaftPredictions.upsampled()`
     + `training._sequence_loss_torch` + `backward()` (the code before the fused pass existed, untouched by it) against
     `training.sequence_loss(RaftPredictions)` + `backward()`.  Also recorded: the device launches of one call of either leg (torch's
     profiler), and for the fused leg the bytes it has to move (masks read, mask gradients written, flows read, flow gradients written,
     ground truth and valid read once: `algorithm_bytes`; plus its workspace and the backward's scaling pass: `moved_bytes`) over the
     measured time, as a share of the 6.3 TB/s a streaming copy achieves on this chip;
  2. the whole `finetune_step` on RAFT (`synthetic_seed=0`), `fused_raft_loss` True against False.
Timing as in tools/bench_train_step.py: device events around a window of calls sized to a target time after warm-up calls, five
windows per candidate, the candidates ALTERNATING window by window; median and spread (min, max) are written.  No speed gate.  Needs a
GPU: no fallback."""
from __future__ import annotations

import argparse
import json
import os
import sys
import warnings
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_wgrad import compare  # noqa: E402

DEV = "cuda"
ACHIEVABLE_TBS = 6.3
HYPER = dict(lr=1e-4, wdecay=1e-4, epsilon=1e-8, num_steps=1_000_000, clip=1.0, gamma=0.8, adv_train=True, iters=12)


def _row(t, a, b):
    return dict(**{k: t[k] for k in t}, ratio=t[a]["median_ms"] / t[b]["median_ms"])


def _launches(fn):
    """Device activities (kernels and copies) of one call, or the reason they could not be counted."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    except Exception as e:
        return f"not counted: {type(e).__name__}: {e}"


def bench_loss(pairs, H, W, npred) -> dict:
    from understanding_flow_robustness_amd import training as T
    from understanding_flow_robustness_amd.flownets.raft import RaftPredictions
    g = torch.Generator(device=DEV).manual_seed(1)
    h, w = H // 8, W // 8
    flows = [(torch.randn(pairs, 2, h, w, device=DEV, generator=g) * 4).requires_grad_(True) for _ in range(npred)]
    masks = [(torch.randn(pairs, 576, h, w, device=DEV, generator=g) * 2).requires_grad_(True) for _ in range(npred)]
    gt = torch.randn(pairs, 2, H, W, device=DEV, generator=g) * 20.0
    valid = (torch.rand(pairs, H, W, device=DEV, generator=g) > 0.2).float()
    preds = RaftPredictions(flows, masks)

    def clear():
        for t in flows + masks:
            t.grad = None

    def fused():
        clear()
        T.sequence_loss(preds, gt, valid)[0].backward()

    def unfused():
        clear()
        T._sequence_loss_torch(preds.upsampled(), gt, valid, 0.8, T.MAX_FLOW, False, False, False, 1, False)[0].backward()
    t = compare({"fused": fused, "unfused": unfused}, warmup=3, windows=5, target_ms=50.0, max_iters=200)
    grads = 4 * npred * pairs * (576 + 2) * h * w
    algorithm = 2 * grads + 4 * pairs * 3 * H * W
    moved = algorithm + 2 * 8 * 18 * npred * pairs * h * w + 2 * grads
    sec = t["fused"]["median_ms"] * 1e-3
    return dict(pairs=pairs, predictions=npred, coarse=[h, w], launches=dict(fused=_launches(fused), unfused=_launches(unfused)),
                algorithm_bytes=algorithm, moved_bytes=moved, fused_algorithm_tb_per_s=algorithm / sec / 1e12,
                fused_moved_tb_per_s=moved / sec / 1e12, fused_moved_share_of_achievable_bandwidth=moved / sec / 1e12 / ACHIEVABLE_TBS,
                achievable_tb_per_s=ACHIEVABLE_TBS, **_row(t, "fused", "unfused"))


def bench_step(x1, x2, flow, valid) -> dict:
    from understanding_flow_robustness_amd import training as T
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    args = Namespace(flownet="RAFT", **HYPER)

    def make(fused):
        net = fetch_model(Namespace(flownet="RAFT"), synthetic_seed=0).to(DEV)
        net.train()
        net.freeze_bn()
        for q in net.parameters():
            q.requires_grad_(True)
        opt, sched = T.fetch_optimizer(args, net)
        return lambda: T.finetune_step(net, opt, sched, x1, x2, flow, valid, args, fused_raft_loss=fused)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = compare({"fused": make(True), "unfused": make(False)}, warmup=2, windows=5, target_ms=200.0, max_iters=10)
    return _row(t, "fused", "unfused")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--preds", type=int, default=12)
    ap.add_argument("--no-step", action="store_true", help="the loss stage only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raft_train_loss.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_raft_train_loss: needs a HIP device (there is no CPU fallback)")
    result = dict(device=torch.cuda.get_device_name(0), height=a.height, width=a.width, torch=torch.__version__, rows=[],
                  method="device events, warm-up calls, 5 alternating windows of ~50 ms (whole steps: ~200 ms), median / min / max in ms; "
                         "ratio = fused / unfused")
    for pairs in a.pairs:
        row = dict(loss=bench_loss(pairs, a.height, a.width, a.preds))
        ls = row["loss"]
        print(f"pairs {pairs} loss stage: fused {ls['fused']['median_ms']:.3f} ms ({ls['launches']['fused']} launches, "
              f"{ls['fused_moved_tb_per_s']:.2f} TB/s moved = {100 * ls['fused_moved_share_of_achievable_bandwidth']:.0f} % of {ACHIEVABLE_TBS} TB/s), "
              f"unfused {ls['unfused']['median_ms']:.3f} ms ({ls['launches']['unfused']} launches) (x{ls['ratio']:.3f})", flush=True)
        if not a.no_step:
            g = torch.Generator(device=DEV).manual_seed(0)
            x1 = torch.rand(pairs, 3, a.height, a.width, device=DEV, generator=g)
            x2 = torch.rand(pairs, 3, a.height, a.width, device=DEV, generator=g)
            flow = torch.randn(pairs, 2, a.height, a.width, device=DEV, generator=g) * 2.0
            valid = (torch.rand(pairs, a.height, a.width, device=DEV, generator=g) > 0.1).float()
            row["step"] = bench_step(x1, x2, flow, valid)
            print(f"pairs {pairs} finetune_step: fused {row['step']['fused']['median_ms']:.2f} ms, unfused "
                  f"{row['step']['unfused']['median_ms']:.2f} ms (x{row['step']['ratio']:.3f})", flush=True)
        result["rows"].append(row)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:                           # after every row: a run cut short keeps what it measured
            json.dump(result, f, indent=1)
            f.write("\n")
        torch.cuda.empty_cache()
    print(json.dumps(dict(out=a.out, rows=len(result["rows"]))))


if __name__ == "__main__":
    main()
