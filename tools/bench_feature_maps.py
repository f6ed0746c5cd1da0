"""The layer statistics of test_patch_embeddings.py (the spatial mean of every feature map of a forward) at the paper's size:
FlowNetC, 384 x 1280, seeded synthetic weights and frames, one pair and eight.  Three things in one process, alternating:

  literal   the reference's method from functions that predate `feature_means`: the torch spelling's capture (UFR_ENGINE=0),
            `.cpu().numpy()` of every map, `np.mean` over its pixels -- per pair of the batch, as the script runs batch 1;
  means     `feature_maps.feature_means`: one native forward, the statistics kernel over the planes, one host read;
  kernel    the statistics launches alone (device events around `iters` back-to-back runs), with the bytes they read
            (6 per plane element, 4 per flow element) against `--hbm-tbs` (the achievable HBM rate of the box, 6.3 TB/s).

The two forms' means are compared first.  Every shape is warmed, every timed window ends in a synchronise, the figures are
medians of `--windows` alternating windows.  There is no speed gate: the numbers are recorded.

    python tools/bench_feature_maps.py [--windows 5] [--out profiles/feature_maps.json]"""
import argparse
import json
import os
import statistics
import sys
import time
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def literal_means(net, args, tgt, ref):
    """What the script does, one pair at a time: all maps to the host, np.mean there."""
    from understanding_flow_robustness_amd.flownets.utils_model import compute_feature_map, predict_flow
    rows = []
    os.environ["UFR_ENGINE"] = "0"
    try:
        for i in range(tgt.shape[0]):
            _, maps = predict_flow(net, None, tgt[i:i + 1], ref[i:i + 1], args, return_feat_maps=True)
            rows.append({k: compute_feature_map(v, "mean") for k, v in maps.items()})
    finally:
        os.environ["UFR_ENGINE"] = "1"
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--hbm-tbs", type=float, default=6.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_maps.json"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_feature_maps: no HIP device; nothing is measured without one")
    from understanding_flow_robustness_amd import _lib as L
    from understanding_flow_robustness_amd import feature_maps as fm
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    H, W = opt.height, opt.width
    args = Namespace(flownet="FlowNetC")
    net = fetch_model(args, synthetic_seed=0).to(DEV)
    for p in net.parameters():
        p.requires_grad_(False)
    result = {"what": "spatial mean of the 28 feature maps of one forward", "network": "FlowNetC (synthetic weights, seed 0)",
              "frame": [H, W], "windows": opt.windows, "device": torch.cuda.get_device_name(0), "hbm_tbs_assumed": opt.hbm_tbs,
              "batches": {}}
    for B in opt.batches:
        g = torch.Generator().manual_seed(B)
        tgt, ref = torch.rand(B, 3, H, W, generator=g).to(DEV), torch.rand(B, 3, H, W, generator=g).to(DEV)
        forms = {"literal": lambda: literal_means(net, args, tgt, ref), "means": lambda: fm.feature_means(net, tgt, ref, args)}
        lit, nat = forms["literal"](), forms["means"]()                 # warm every shape; compare before anything is timed
        torch.cuda.synchronize()
        worst = max(float(np.abs(nat[k] - lit[k]).max() / max(np.abs(lit[k]).max(), 1e-30)) for k in lit)
        print(f"B={B}: worst |means - literal| / max|literal| over the keys = {worst:.3e}", flush=True)
        if worst > 1e-3:
            raise SystemExit("bench_feature_maps: the two forms disagree; nothing is timed")
        times = {k: [] for k in forms}
        for w in range(opt.windows):
            for name, fn in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
            print(f"B={B} window {w}: " + ", ".join(f"{k} {v[-1] * 1e3:.2f} ms" for k, v in times.items()), flush=True)
        # the statistics launches alone, on the planes the last forward left
        plan = next(p for p in L.engine_cache(net, "_ufr_feature_stats_plans").values() if p.B == B)
        nbytes = 0
        for key, (_, cn, px) in plan.cols.items():
            nbytes += B * int(px) * (4 * cn if key in ("flow6", "flow5", "flow4", "flow3", "predict") else 6 * ((cn + 31) // 32 * 32))
        kernel = []
        for _ in range(opt.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(opt.iters):
                plan.run()
            e1.record()
            torch.cuda.synchronize()
            kernel.append(e0.elapsed_time(e1) / opt.iters)
        k_ms = statistics.median(kernel)
        result["batches"][str(B)] = {
            "worst_relative_difference": worst,
            "ms": {k: statistics.median(v) * 1e3 for k, v in times.items()},
            "ms_all_windows": {k: [x * 1e3 for x in v] for k, v in times.items()},
            "statistics_kernel": {"ms": k_ms, "ms_all_windows": kernel, "bytes_read": nbytes, "tb_per_s": nbytes / k_ms / 1e9,
                                  "share_of_achievable_hbm": nbytes / k_ms / 1e9 / opt.hbm_tbs},
        }
        print(json.dumps({str(B): result["batches"][str(B)]["ms"], "kernel": result["batches"][str(B)]["statistics_kernel"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
