"""The patch evaluation (patch_eval.py) at the paper's size: FlowNetC, 384 x 1280 frames, a 375 x 1242 ground truth with holes in its
valid channel, a 51 x 51 circular patch, `--different_pos`, 200 synthetic items (kitti2015's count), seeded synthetic weights.  Two
forms in one process, alternating:

  literal   the script's loop (test_patch.py:242-466) from this project's host mirrors: `circle_transform_different` on the host,
            five uploads, `predict_flow` at batch 1 twice, torch pastes, `scipy.ndimage.zoom` of the canvas flow on the host,
            `losses.compute_epe` / `compute_cossim` (four `.item()` per item);
  native    evaluate_patch at chunk 1, 4 and 8.

The forms' per-item metrics are compared first (on the first `--check` items).  Every shape is warmed, every timed window ends in a
synchronise, the figures are medians of `--windows` alternating windows.  The device time of `ufr_eval_paste` and `ufr_eval_metrics`
comes from device events in a run of its own.

    python tools/bench_patch_eval.py [--windows 5] [--items 200] [--out profiles/patch_eval.json]"""
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
from scipy.ndimage import zoom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def literal_loop(net, args, loader, patch, mask):
    from understanding_flow_robustness_amd.flownets.utils_model import predict_flow
    from understanding_flow_robustness_amd.losses import compute_cossim, compute_epe
    from understanding_flow_robustness_amd.utils_patch import circle_transform_different
    rows = []
    with torch.no_grad():
        for past, tgt, ref, gt in loader:
            flow_fwd = predict_flow(net, past, tgt, ref, args)
            pf, mf, flow_full, _, _, _, _ = circle_transform_different(patch, mask, patch.copy(), tuple(tgt.shape), patch.shape, 0,
                                                                       norotate=args.norotate, fixed_loc=(-1, -1))
            p_tgt, p_ref, m_tgt, m_ref = (torch.FloatTensor(a).to(DEV) for a in (pf[0], pf[1], mf[0], mf[1]))
            flow_full = torch.FloatTensor(flow_full)
            adv_tgt = torch.clamp(torch.mul((1 - m_tgt), tgt) + torch.mul(m_tgt, p_tgt), 0, 1)
            adv_past = torch.clamp(torch.mul((1 - m_tgt), past) + torch.mul(m_tgt, p_tgt), 0, 1)
            adv_ref = torch.clamp(torch.mul((1 - m_ref), ref) + torch.mul(m_ref, p_ref), 0, 1)
            adv_flow = predict_flow(net, adv_past, adv_tgt, adv_ref, args)
            bt, _, hg, wg = gt.shape
            m_res = F.interpolate(m_tgt, size=(hg, wg), mode="bilinear", align_corners=False)
            m_ref = F.interpolate(m_ref, size=(hg, wg), mode="bilinear", align_corners=False)
            gt_occ = torch.mul((1 - m_ref), gt) + torch.mul(m_ref, torch.zeros((bt, 3, hg, wg)).to(DEV))
            patch_flow = torch.from_numpy(zoom(flow_full, zoom=(1, 1, hg / flow_full.shape[2], wg / flow_full.shape[3]), order=1)).to(DEV)
            gt_adv = torch.mul((1 - m_res), gt_occ) + torch.mul(m_res, patch_flow)
            rows.append((compute_epe(gt=gt_occ, pred=flow_fwd), compute_epe(gt=gt_adv, pred=adv_flow), compute_cossim(gt_occ, flow_fwd),
                         compute_cossim(gt_adv, adv_flow)))
    return np.asarray(rows, dtype=np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--items", type=int, default=200)
    ap.add_argument("--check", type=int, default=16, help="items whose metrics are compared between the forms before timing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_eval.json"))
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--patch", type=int, default=51)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_patch_eval: no HIP device; nothing is measured without one")
    from understanding_flow_robustness_amd import patch_eval as pe
    from understanding_flow_robustness_amd.chunked_eval import recorded_events, stage_ms
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    from understanding_flow_robustness_amd.utils_patch import createCircularMask
    H, W, S, n = opt.height, opt.width, opt.patch, opt.items
    hg, wg = H - 9, W - 38                                      # KITTI's 375 x 1242 behind a 384 x 1280 network input
    args = Namespace(flownet="FlowNetC", patch_type="circle", different_pos=True, norotate=False)
    net = fetch_model(args, synthetic_seed=0).to(DEV)
    g = torch.Generator().manual_seed(0)
    loader = []
    for _ in range(n):
        past, tgt, ref = (torch.rand(1, 3, H, W, generator=g).to(DEV) for _ in range(3))
        gt = torch.cat((torch.randn(1, 2, hg, wg, generator=g) * 5.0, (torch.rand(1, 1, hg, wg, generator=g) > 0.3).float()), 1).to(DEV)
        loader.append((past, tgt, ref, gt))
    patch = np.random.RandomState(0).rand(1, 3, S, S)
    disc = createCircularMask(S, S).astype("float32")
    mask = np.array([[disc, disc, disc]])
    chunks = (1, 4, 8)

    def native(chunk, items=loader):
        np.random.seed(1337)
        return pe.evaluate_patch(net, items, patch, mask, patch.shape, args, chunk=chunk)

    def literal(items=loader):
        np.random.seed(1337)
        return literal_loop(net, args, items, patch, mask)

    forms = {"literal": literal}
    forms.update({f"native_chunk{c}": (lambda c=c: native(c)) for c in chunks})
    # warm every shape (a ragged last chunk included), and compare the metrics before anything is timed
    head = loader[:opt.check]
    want = literal(head)
    agreement = {}
    for c in chunks:
        got = native(c, head).per_item
        native(c, loader[:2 * c + 1])
        agreement[f"chunk{c}_epe_rel"] = float(np.max(np.abs(got[:, :2] - want[:, :2]) / np.abs(want[:, :2])))
        agreement[f"chunk{c}_cos_abs"] = float(np.max(np.abs(got[:, 2:] - want[:, 2:])))
    torch.cuda.synchronize()
    print("agreement:", json.dumps(agreement), flush=True)
    if max(agreement.values()) > 1e-4:
        raise SystemExit("bench_patch_eval: the forms disagree; nothing is timed")
    times = {k: [] for k in forms}
    for w in range(opt.windows):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
        print(f"window {w}: " + ", ".join(f"{k} {v[-1]:.3f} s" for k, v in times.items()), flush=True)
    # the two entries' device time, from device events, in a run of its own per chunk size
    split = {}
    for c in chunks:
        acc = stage_ms(recorded_events(pe.evaluate_patch, lambda: native(c)), ("paste", "forward", "metrics"))
        split[f"chunk{c}"] = {k: v / n for k, v in acc.items()}
    result = {
        "what": "patch evaluation over a validation set, --different_pos", "network": "FlowNetC (synthetic weights, seed 0)",
        "frame": [H, W], "ground_truth": [hg, wg], "patch": S, "items": n, "windows": opt.windows,
        "device": torch.cuda.get_device_name(0), "agreement_first_items": dict(agreement, items=len(head)),
        "seconds_per_evaluation": {k: statistics.median(v) for k, v in times.items()},
        "ms_per_item": {k: statistics.median(v) / n * 1e3 for k, v in times.items()},
        "seconds_all_windows": times,
        "device_ms_per_item": split,
        "conditions": "measured once, one box; synthetic frames resident on the device (no data loading in either form); "
                      "wall clock around whole evaluations, each window ends in a synchronise",
    }
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("seconds_per_evaluation", "ms_per_item", "device_ms_per_item")}), flush=True)


if __name__ == "__main__":
    main()
