#!/usr/bin/env python3
"""The training loss, the clipped AdamW step and the whole fine-tuning step of FlowNetC and PWC-Net: native against torch, on one box.

    timeout 1100 python tools/bench_train_step.py [--height 384 --width 1280 --pairs 1 8 --nets FlowNetC PWCNet --out profiles/train_step.json]

For every network and pair count, three comparisons:
  1. the loss alone, forward + backward: `training.sequence_loss` on the kernel path against its plain-torch restatement, on the
     shapes the network's training forward returns;
  2. the optimiser alone: `ClippedAdamW.step(clip)` against `clip_grad_norm_` + `torch.optim.AdamW` in its default form, and against
     `fused=True` where this torch builds it.  Also reported: the bytes the algorithm needs (8 passes x 4 bytes x parameters: read
     g for the norm; read p, g, m, v; write p, m, v) over the measured time, and that rate as a share of the 6.3 TB/s a streaming
     copy achieves on this chip -- the kernel's share of ACHIEVABLE bandwidth, not of the data-sheet peak;
  3. the whole `finetune_step` inside `band_conv.native_training()`: the new loss and optimiser against the torch ones (the
     restatement + clip_grad_norm_ + torch.optim.AdamW) around the same native convolutions.
Timing as in tools/bench_wgrad.py: device events around a window of calls sized to a target time after warm-up calls, five windows per
candidate, the candidates ALTERNATING window by window; median and spread (min, max) are written.  Needs a GPU: no fallback."""
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
NET_FLAGS = {"FlowNetC": dict(flowNetC=True), "PWCNet": dict(pwc=True)}
HYPER = dict(lr=1e-4, wdecay=1e-4, epsilon=1e-8, num_steps=1_000_000, clip=1.0, gamma=0.8, adv_train=True)


def _net(flownet):
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    net = fetch_model(Namespace(flownet=flownet), synthetic_seed=0).to(DEV)
    net.train()
    for q in net.parameters():
        q.requires_grad_(True)
    return net


def _row(t, a, b):
    return dict(**{k: t[k] for k in t}, ratio=t[a]["median_ms"] / t[b]["median_ms"])


def bench_loss(net, flownet, x1, x2, flow, valid) -> dict:
    from understanding_flow_robustness_amd import training as T
    kw = NET_FLAGS[flownet]
    with torch.no_grad():
        shapes = [tuple(f.shape) for f in net(x1, x2)]
    g = torch.Generator(device=DEV).manual_seed(1)
    preds = [torch.randn(s, device=DEV, generator=g).requires_grad_(True) for s in shapes]

    def native():
        for p in preds:
            p.grad = None
        T.sequence_loss(preds, flow, valid, **kw)[0].backward()

    def restatement():
        for p in preds:
            p.grad = None
        T._sequence_loss_torch(preds, flow, valid, 0.8, T.MAX_FLOW, kw.get("flowNetC", False), kw.get("pwc", False), False, 1, False)[0].backward()
    t = compare({"native": native, "torch": restatement}, warmup=3, windows=5, target_ms=50.0, max_iters=200)
    return dict(scales=[list(s) for s in shapes], **_row(t, "native", "torch"))


def bench_optimizer(net) -> dict:
    from understanding_flow_robustness_amd.training import ClippedAdamW
    params = [p for p in net.parameters()]
    g = torch.Generator(device=DEV).manual_seed(2)
    for p in params:
        p.grad = torch.randn(p.shape, device=DEV, generator=g) * 1e-3
    n = sum(p.numel() for p in params)
    kw = dict(lr=HYPER["lr"], weight_decay=HYPER["wdecay"], eps=HYPER["epsilon"])
    saved = [p.detach().clone() for p in params]                 # every candidate steps the same parameters: restored afterwards
    mine, plain = ClippedAdamW(params, **kw), torch.optim.AdamW(params, **kw)
    cands = {"native": lambda: mine.step(clip=HYPER["clip"]),
             "torch": lambda: (torch.nn.utils.clip_grad_norm_(params, HYPER["clip"]), plain.step())}
    fused_note = None
    try:
        fused = torch.optim.AdamW(params, fused=True, **kw)
        fused.step()
        cands["torch_fused"] = lambda: (torch.nn.utils.clip_grad_norm_(params, HYPER["clip"]), fused.step())
    except Exception as e:                                       # this torch does not build the fused form for this device
        fused_note = f"fused=True is not available: {type(e).__name__}: {e}"
    t = compare(cands, warmup=3, windows=5, target_ms=50.0, max_iters=200)
    with torch.no_grad():
        for p, s in zip(params, saved):
            p.copy_(s)
            p.grad = None
    need = 8 * 4 * n
    tbs = need / (t["native"]["median_ms"] * 1e-3) / 1e12
    best = min((k for k in t if k != "native"), key=lambda k: t[k]["median_ms"])
    return dict(parameters=n, tensors=len(params), algorithm_bytes=need, native_tb_per_s=tbs,
                native_share_of_achievable_bandwidth=tbs / ACHIEVABLE_TBS, achievable_tb_per_s=ACHIEVABLE_TBS,
                best_torch_form=best, native_over_best_torch=t["native"]["median_ms"] / t[best]["median_ms"], fused_note=fused_note,
                **_row(t, "native", "torch"))


def bench_step(flownet, x1, x2, flow, valid) -> dict:
    from understanding_flow_robustness_amd import training as T
    from understanding_flow_robustness_amd.band_conv import native_training
    args = Namespace(flownet=flownet, **HYPER, **NET_FLAGS[flownet])
    kw = NET_FLAGS[flownet]

    def make(new):
        net = _net(flownet)
        if new:
            opt, sched = T.fetch_optimizer(args, net)

            def step():
                with native_training():
                    T.finetune_step(net, opt, sched, x1, x2, flow, valid, args)
        else:
            opt = torch.optim.AdamW(net.parameters(), lr=args.lr, weight_decay=args.wdecay, eps=args.epsilon)
            sched = torch.optim.lr_scheduler.OneCycleLR(opt, args.lr, args.num_steps + 100, pct_start=0.05, cycle_momentum=False,
                                                        anneal_strategy="linear")

            def step():                                          # the same iteration with the torch loss and optimiser
                with native_training():
                    opt.zero_grad()
                    loss, _ = T._sequence_loss_torch(net(x1, x2), flow, valid, args.gamma, T.MAX_FLOW, kw.get("flowNetC", False),
                                                     kw.get("pwc", False), False, 1, False)
                    if not torch.isnan(loss).item():
                        loss.backward()
                        torch.nn.utils.clip_grad_norm_(net.parameters(), args.clip)
                        opt.step()
                        sched.step()
        return step
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = compare({"native": make(True), "torch": make(False)}, warmup=2, windows=5, target_ms=200.0, max_iters=10)
    return _row(t, "native", "torch")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--nets", nargs="+", default=list(NET_FLAGS), choices=list(NET_FLAGS))
    ap.add_argument("--no-step", action="store_true", help="the loss and the optimiser only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_step.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_step: needs a HIP device (there is no CPU fallback)")
    result = dict(device=torch.cuda.get_device_name(0), height=a.height, width=a.width, torch=torch.__version__, rows=[],
                  method="device events, warm-up calls, 5 alternating windows of ~50 ms (whole steps: ~200 ms), median / min / max in ms; "
                         "ratio = native / torch")
    for flownet in a.nets:
        net = _net(flownet)
        opt_row = bench_optimizer(net)                            # independent of the pair count
        print(f"{flownet} optimiser ({opt_row['parameters']} parameters in {opt_row['tensors']} tensors): native "
              f"{opt_row['native']['median_ms']:.3f} ms = {opt_row['native_tb_per_s']:.2f} TB/s of algorithm bytes "
              f"({100 * opt_row['native_share_of_achievable_bandwidth']:.0f} % of {ACHIEVABLE_TBS} TB/s achievable), torch "
              f"{opt_row['torch']['median_ms']:.3f} ms" + (f", torch fused {opt_row['torch_fused']['median_ms']:.3f} ms" if "torch_fused" in opt_row else ""),
              flush=True)
        for pairs in a.pairs:
            g = torch.Generator(device=DEV).manual_seed(0)
            x1 = torch.rand(pairs, 3, a.height, a.width, device=DEV, generator=g)
            x2 = torch.rand(pairs, 3, a.height, a.width, device=DEV, generator=g)
            flow = torch.randn(pairs, 2, a.height, a.width, device=DEV, generator=g) * 2.0
            flow[:, :, 100:140, 300:420] = float("nan")          # invalid pixels, as KITTI's ground truth has them
            valid = torch.ones(pairs, a.height, a.width, device=DEV)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                row = dict(net=flownet, pairs=pairs, loss=bench_loss(net, flownet, x1, x2, flow, valid), optimizer=opt_row)
            print(f"{flownet} pairs {pairs} loss fwd+bwd: native {row['loss']['native']['median_ms']:.3f} ms, torch "
                  f"{row['loss']['torch']['median_ms']:.3f} ms (x{row['loss']['ratio']:.2f})", flush=True)
            if not a.no_step:
                row["step"] = bench_step(flownet, x1, x2, flow, valid)
                print(f"{flownet} pairs {pairs} finetune_step in native_training(): new loss + optimiser {row['step']['native']['median_ms']:.2f} ms, "
                      f"torch loss + optimiser {row['step']['torch']['median_ms']:.2f} ms (x{row['step']['ratio']:.3f})", flush=True)
            result["rows"].append(row)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:                           # after every row: a run cut short keeps what it measured
                json.dump(result, f, indent=1)
                f.write("\n")
        del net
    print(json.dumps(dict(out=a.out, rows=len(result["rows"]))))


if __name__ == "__main__":
    main()
