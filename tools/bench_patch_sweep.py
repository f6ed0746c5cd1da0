"""The patch location sweep (patch_sweep.py) at the paper's size: FlowNetC, 384 x 1280, a 51 x 51 circular patch, stride 25
(14 x 50 = 700 positions), chunk 8, seeded synthetic weights and frames.  Three forms in one process, alternating:

  literal   the reference's loop (test_moving_patch.py:299-445) from functions that predate the sweep: host
            `circle_transform(moving=True, norotate=True, fixed_loc=...)`, upload, torch paste, `predict_flow` at batch 1,
            `losses.compute_epe` / `compute_cossim`;
  generic   sweep_patch_locations(cone=False);
  windowed  sweep_patch_locations(cone=True).

The three forms' maps are compared first.  Every shape is warmed, every timed window ends in a synchronise, the figures are medians
of `--windows` alternating windows.  The windowed path's split into restore / paste / prefix / head / metrics comes from device
events in a run of its own.  `--net pwc` adds one generic-path figure for PWC-Net (384 x 1280 as well).

    python tools/bench_patch_sweep.py [--windows 5] [--net pwc] [--out profiles/patch_sweep.json]"""
import argparse
import json
import os
import statistics
import sys
import time
from argparse import Namespace

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def literal_sweep(net, args, tgt, ref, gt, patch, mask, stride):
    from understanding_flow_robustness_amd.flownets.utils_model import predict_flow
    from understanding_flow_robustness_amd.losses import compute_cossim, compute_epe
    from understanding_flow_robustness_amd.utils_patch import circle_transform
    with torch.no_grad():
        flow = predict_flow(net, None, tgt, ref, args)
    epe, cos_sim = compute_epe(gt=gt, pred=flow), compute_cossim(gt, flow)
    shape, pshape = tuple(tgt.shape), patch.shape
    ys, xs = range(0, shape[-2] - pshape[-2], stride), range(0, shape[-1] - pshape[-1], stride)
    adv_epe, adv_cos = np.zeros((len(ys), len(xs))), np.zeros((len(ys), len(xs)))
    bt, _, hg, wg = gt.shape
    for x in xs:
        for y in ys:
            pf, mf, _, _, _, _ = circle_transform(patch, mask, patch.copy(), shape, pshape, 0, norotate=True, fixed_loc=(x, y), moving=True)
            p, m = torch.FloatTensor(pf).to(DEV), torch.FloatTensor(mf).to(DEV)
            patch_flow = torch.cat((torch.zeros((bt, 2, hg, wg)), torch.ones((bt, 1, hg, wg))), 1).to(DEV)
            adv_tgt = torch.clamp(torch.mul((1 - m), tgt) + torch.mul(m, p), 0, 1)
            adv_ref = torch.clamp(torch.mul((1 - m), ref) + torch.mul(m, p), 0, 1)
            with torch.no_grad():
                adv_flow = predict_flow(net, None, adv_tgt, adv_ref, args)
            m_res = F.interpolate(m, size=(hg, wg), mode="bilinear", align_corners=False)
            gt_adv = torch.mul((1 - m_res), gt) + torch.mul(m_res, patch_flow)
            adv_epe[y // stride, x // stride] = compute_epe(gt=gt_adv, pred=adv_flow)
            adv_cos[y // stride, x // stride] = compute_cossim(gt_adv, adv_flow)
    return adv_epe, adv_cos, epe, cos_sim


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--net", default=None, choices=[None, "pwc"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_sweep.json"))
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--patch", type=int, default=51)
    ap.add_argument("--stride", type=int, default=25)
    ap.add_argument("--chunk", type=int, default=8)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_patch_sweep: no HIP device; nothing is measured without one")
    from understanding_flow_robustness_amd import patch_sweep as ps
    from understanding_flow_robustness_amd.chunked_eval import recorded_events, stage_ms
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    from understanding_flow_robustness_amd.utils_patch import createCircularMask
    H, W, S, stride, chunk = opt.height, opt.width, opt.patch, opt.stride, opt.chunk
    args = Namespace(flownet="FlowNetC", norotate=True)
    net = fetch_model(args, synthetic_seed=0).to(DEV)
    g = torch.Generator().manual_seed(0)
    tgt, ref = torch.rand(1, 3, H, W, generator=g).to(DEV), torch.rand(1, 3, H, W, generator=g).to(DEV)
    hg, wg = H - 9, W - 38                                      # KITTI's 375 x 1242 behind a 384 x 1280 network input
    gt = torch.cat((torch.randn(1, 2, hg, wg, generator=g) * 5.0, (torch.rand(1, 1, hg, wg, generator=g) > 0.3).float()), 1).to(DEV)
    patch = np.random.RandomState(0).rand(1, 3, S, S)
    disc = createCircularMask(S, S).astype("float32")
    mask = np.array([[disc, disc, disc]])
    n = len(ps.sweep_grid(H, W, S, S, stride)[2])

    forms = {
        "literal": lambda: literal_sweep(net, args, tgt, ref, gt, patch, mask, stride),
        "generic": lambda: ps.sweep_patch_locations(net, tgt, ref, gt, patch, mask, args, stride=stride, chunk=chunk, cone=False),
        "windowed": lambda: ps.sweep_patch_locations(net, tgt, ref, gt, patch, mask, args, stride=stride, chunk=chunk, cone=True),
    }
    # warm every shape, and compare the maps before anything is timed
    gen, winr = forms["generic"](), forms["windowed"]()
    lit = forms["literal"]()
    torch.cuda.synchronize()
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(b)))
    agreement = {
        "generic_vs_literal_epe_rel": rel(gen.adv_epe, lit[0]), "generic_vs_literal_cos_abs": float(np.abs(gen.adv_cos_sim - lit[1]).max()),
        "windowed_vs_generic_epe_rel": rel(winr.adv_epe, gen.adv_epe),
        "windowed_vs_generic_cos_abs": float(np.abs(winr.adv_cos_sim - gen.adv_cos_sim).max()),
        "clean_epe": [lit[2], gen.epe, winr.epe], "worst": [list(gen.worst), list(winr.worst)],
    }
    print("agreement:", json.dumps(agreement), flush=True)
    if max(agreement["generic_vs_literal_epe_rel"], agreement["windowed_vs_generic_epe_rel"], agreement["generic_vs_literal_cos_abs"],
           agreement["windowed_vs_generic_cos_abs"]) > 1e-4:
        raise SystemExit("bench_patch_sweep: the three forms disagree; nothing is timed")
    times = {k: [] for k in forms}
    for w in range(opt.windows):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
        print(f"window {w}: " + ", ".join(f"{k} {v[-1]:.3f} s" for k, v in times.items()), flush=True)
    # the windowed path's stages, from device events, in a run of its own
    split = stage_ms(recorded_events(ps.sweep_patch_locations, forms["windowed"]), ps.WINDOWED_STAGES)
    result = {
        "what": "patch location sweep, one frame pair", "network": "FlowNetC (synthetic weights, seed 0)", "frame": [H, W],
        "ground_truth": [hg, wg], "patch": S, "stride": stride, "positions": n, "chunk": chunk, "windows": opt.windows,
        "device": torch.cuda.get_device_name(0), "agreement": agreement,
        "seconds_per_sweep": {k: statistics.median(v) for k, v in times.items()},
        "ms_per_position": {k: statistics.median(v) / n * 1e3 for k, v in times.items()},
        "seconds_all_windows": times,
        "windowed_split_ms_per_sweep": split,
        "windowed_split_ms_per_position": {k: v / n for k, v in split.items()},
    }
    if opt.net == "pwc":
        pargs = Namespace(flownet="PWCNet", norotate=True)
        pwc = fetch_model(pargs, synthetic_seed=0).to(DEV)
        run = lambda: ps.sweep_patch_locations(pwc, tgt, ref, gt, patch, mask, pargs, stride=stride, chunk=chunk)
        run()
        torch.cuda.synchronize()
        t = []
        for _ in range(opt.windows):
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        result["pwcnet_generic"] = {"seconds_per_sweep": statistics.median(t), "ms_per_position": statistics.median(t) / n * 1e3,
                                    "seconds_all_windows": t}
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    if os.path.exists(opt.out):                # the metrics kernel's recorded errors (tests/test_patch_sweep_gpu.py) stay
        with open(opt.out) as f:
            kept = json.load(f).get("metrics_kernel_errors")
        if kept is not None:
            result["metrics_kernel_errors"] = kept
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("seconds_per_sweep", "ms_per_position", "windowed_split_ms_per_position")}), flush=True)


if __name__ == "__main__":
    main()
