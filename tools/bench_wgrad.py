#!/usr/bin/env python3
"""Weight-gradient kernel and native fine-tuning step of FlowNetC (or PWC-Net) against the vendor library, on one box.

    timeout 900 python tools/bench_wgrad.py [--height 384 --width 1280 --pairs 1 8 --out profiles/wgrad_layers.json]
    timeout 900 python tools/bench_wgrad.py --net pwc          (writes profiles/wgrad_layers_pwc.json)

For every layer of the network at the given frame size and every pair count:
  * `ufr_igemm_wgrad` (igemm.make_wgrad_launch, default split) against `torch.nn.grad.conv2d_weight` (transposed layers: the
    weight output of `aten.convolution_backward`) on the same seeded operands, with the two results' largest difference;
  * one fine-tuning step (training mode, every parameter trainable, forward + backward of a multi-scale loss) inside and outside
    `band_conv.native_training()`.
Timing: device events around a window of launches sized to ~50 ms after three warm-up launches (the vendor library picks its
algorithm on the first), five windows per candidate, the candidates ALTERNATING window by window; the median and the spread
(min, max) of the windows are written.  Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda"


def layers(H: int, W: int, pairs: int):
    """(name, images, Cin, Cout, Hin, Win, k, stride, padding, transposed) of every convolution of FlowNetC (the siamese stem runs
    on 2 x pairs images)."""
    from understanding_flow_robustness_amd.flownets.flownetc import FlowNetC
    scale = {"conv1": 1, "conv2": 2, "conv3": 4, "conv_redir": 8, "conv3_1": 8, "conv4": 8, "conv4_1": 16, "conv5": 16, "conv5_1": 32,
             "conv6": 32, "conv6_1": 64}
    out = []
    for name, cin, cout, k, s in FlowNetC._ENCODER:
        n = 2 * pairs if name in ("conv1", "conv2", "conv3") else pairs
        out.append((name, n, cin, cout, H // scale[name], W // scale[name], k, s, (k - 1) // 2, False))
    for (name, cin, cout), sc in zip(FlowNetC._DECODER, (64, 32, 16, 8)):
        out.append((name, pairs, cin, cout, H // sc, W // sc, 4, 2, 1, True))
    for (name, cin), sc in zip(FlowNetC._HEADS, (64, 32, 16, 8, 4)):
        out.append((name, pairs, cin, 2, H // sc, W // sc, 3, 1, 1, False))
    for name, sc in zip(FlowNetC._UPS, (64, 32, 16, 8)):
        out.append((name, pairs, 2, 2, H // sc, W // sc, 4, 2, 1, True))
    return out


def pwc_layers(H: int, W: int, pairs: int):
    """The same rows plus a dilation for every convolution a PWC-Net training step runs (the siamese pyramid on 2 x pairs images;
    `deconv2` is built by the reference and never called: left out)."""
    from understanding_flow_robustness_amd.flownets.pwcnet import PWCDCNet
    net = PWCDCNet()
    scale = {}
    for lvl, (_, _, first, second, third) in enumerate(PWCDCNet._PYRAMID, start=1):
        scale["conv" + first] = (1 << (lvl - 1), 2 * pairs)
        scale["conv" + second] = scale["conv" + third] = (1 << lvl, 2 * pairs)
    for lvl in (6, 5, 4, 3, 2):
        for name in [f"conv{lvl}_{i}" for i in range(5)] + [f"predict_flow{lvl}"] + ([f"deconv{lvl}", f"upfeat{lvl}"] if lvl > 2 else []):
            scale[name] = (1 << lvl, pairs)
    for i in range(1, 8):
        scale[f"dc_conv{i}"] = (4, pairs)
    out = []
    for name, (sc, n) in scale.items():
        mod = getattr(net, name)
        conv = mod[0] if isinstance(mod, torch.nn.Sequential) else mod
        transposed = isinstance(conv, torch.nn.ConvTranspose2d)
        out.append((name, n, conv.in_channels, conv.out_channels, H // sc, W // sc, conv.kernel_size[0], conv.stride[0], conv.padding[0],
                    transposed, conv.dilation[0]))
    return out


def window_ms(fn, iters: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def compare(cands: dict, warmup: int = 3, windows: int = 5, target_ms: float = 50.0, max_iters: int = 200) -> dict:
    """{name: fn} -> {name: {median_ms, min_ms, max_ms, iters}}: the candidates alternate window by window."""
    iters = {}
    for name, fn in cands.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        iters[name] = max(1, min(max_iters, int(target_ms / max(window_ms(fn, 2), 1e-3))))
    times = {name: [] for name in cands}
    for _ in range(windows):
        for name, fn in cands.items():
            times[name].append(window_ms(fn, iters[name]))
    return {name: dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), iters=iters[name]) for name, t in times.items()}


def bench_layer(spec) -> dict:
    from understanding_flow_robustness_amd import igemm as ig
    name, n, cin, cout, H, W, k, s, p, transposed = spec[:10]
    d = spec[10] if len(spec) > 10 else 1
    g = torch.Generator(device=DEV).manual_seed(0)
    Ho, Wo = (2 * H, 2 * W) if transposed else ((H + 2 * p - (k - 1) * d - 1) // s + 1, (W + 2 * p - (k - 1) * d - 1) // s + 1)
    x = torch.randn(n, cin, H, W, device=DEV, generator=g)
    gy = torch.randn(n, cout, Ho, Wo, device=DEV, generator=g)
    wshape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
    xp = ig.Planes(n, H, W, ig.pad32(cin) // 32, DEV).load_nchw(x)
    gp = ig.Planes(n, Ho, Wo, ig.pad32(cout) // 32, DEV).load_nchw(gy)
    dw = torch.empty(wshape, device=DEV)
    launch = ig.make_wgrad_launch(xp, 0, cin, gp, 0, cout, k, s, p, transposed=transposed, dw=dw, dilation=d)
    if transposed:
        w0 = torch.empty(wshape, device=DEV)

        def vendor():
            return torch.ops.aten.convolution_backward(gy, x, w0, None, (s, s), (p, p), (1, 1), True, (0, 0), 1, (False, True, False))[1]
    else:
        def vendor():
            return torch.nn.grad.conv2d_weight(x, wshape, gy, s, p, d)
    launch()
    ref = vendor()
    diff = float((dw - ref).abs().max()) / float(ref.abs().max())
    t = compare({"native": launch, "vendor": vendor})
    flops = 2.0 * n * (H * W if transposed else Ho * Wo) * k * k * cin * cout
    return dict(layer=name, images=n, cin=cin, cout=cout, h=H, w=W, kernel=k, stride=s, dilation=d, transposed=transposed, splitm=int(launch.desc.splitm),
                gflop=flops / 1e9, native=t["native"], vendor=t["vendor"], native_over_vendor=t["native"]["median_ms"] / t["vendor"]["median_ms"],
                native_tflops=flops / t["native"]["median_ms"] / 1e9, max_rel_diff_to_vendor=diff)


def bench_step(H: int, W: int, pairs: int, flownet: str = "FlowNetC") -> dict:
    import warnings
    from argparse import Namespace

    from understanding_flow_robustness_amd.band_conv import native_training
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    net = fetch_model(Namespace(flownet=flownet), synthetic_seed=0).to(DEV)
    net.train()
    for q in net.parameters():
        q.requires_grad_(True)
    g = torch.Generator(device=DEV).manual_seed(0)
    x1, x2 = torch.rand(pairs, 3, H, W, device=DEV, generator=g), torch.rand(pairs, 3, H, W, device=DEV, generator=g)
    weights = (0.005, 0.01, 0.02, 0.08, 0.32)                  # finest scale first, as the forward returns them

    def step():
        net.zero_grad(set_to_none=True)
        sum(wt * (f ** 2).mean() for wt, f in zip(weights, net(x1, x2))).backward()

    def native():
        with native_training():
            step()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = compare({"native": native, "vendor": step}, warmup=2, windows=5, target_ms=200.0, max_iters=10)
    return dict(pairs=pairs, h=H, w=W, native=t["native"], vendor=t["vendor"],
                native_over_vendor=t["native"]["median_ms"] / t["vendor"]["median_ms"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--net", choices=("flownetc", "pwc"), default="flownetc", help="pwc: PWC-Net's layers and step, profiles/wgrad_layers_pwc.json")
    ap.add_argument("--out", default=None, help="default: profiles/wgrad_layers.json (--net pwc: profiles/wgrad_layers_pwc.json)")
    ap.add_argument("--no-step", action="store_true", help="kernel timings only")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "wgrad_layers_pwc.json" if a.net == "pwc" else "wgrad_layers.json")
    layer_list, flownet = (pwc_layers, "PWCNet") if a.net == "pwc" else (layers, "FlowNetC")
    if not torch.cuda.is_available():
        raise SystemExit("bench_wgrad: needs a HIP device (there is no CPU fallback)")
    result = dict(device=torch.cuda.get_device_name(0), net=flownet, height=a.height, width=a.width, layers=[], steps=[],
                  method="device events, 3 warm-up launches, 5 alternating windows of ~50 ms (steps: ~200 ms), median / min / max in ms")
    for pairs in a.pairs:
        for spec in layer_list(a.height, a.width, pairs):
            row = dict(pairs=pairs, **bench_layer(spec))
            result["layers"].append(row)
            print(f"pairs {pairs} {row['layer']:22s} native {row['native']['median_ms']:8.3f} ms  vendor {row['vendor']['median_ms']:8.3f} ms  "
                  f"x{row['native_over_vendor']:.2f}  ({row['native_tflops']:.1f} TFLOP/s, splitm {row['splitm']}, diff {row['max_rel_diff_to_vendor']:.1e})",
                  flush=True)
        tot_n = sum(r["native"]["median_ms"] for r in result["layers"] if r["pairs"] == pairs)
        tot_v = sum(r["vendor"]["median_ms"] for r in result["layers"] if r["pairs"] == pairs)
        print(f"pairs {pairs} all layers: native {tot_n:.3f} ms, vendor {tot_v:.3f} ms", flush=True)
        result.setdefault("layer_totals", []).append(dict(pairs=pairs, native_ms=tot_n, vendor_ms=tot_v))
        if not a.no_step:
            row = bench_step(a.height, a.width, pairs, flownet)
            result["steps"].append(row)
            print(f"pairs {pairs} fine-tuning step: native {row['native']['median_ms']:.2f} ms, vendor {row['vendor']['median_ms']:.2f} ms "
                  f"(x{row['native_over_vendor']:.2f})", flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:                       # after every pair count: a run cut short keeps what it measured
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(dict(out=a.out, layers=len(result["layers"]), steps=len(result["steps"]))))


if __name__ == "__main__":
    main()
