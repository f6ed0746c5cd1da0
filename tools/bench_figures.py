"""The figures of the patch evaluation (patch_eval.evaluate_patch(save_path=...), flowlib.py, csrc/flow_viz.hip) at the paper's size:
FlowNetC, 384 x 1280 frames, a 375 x 1242 ground truth with holes in its valid channel, a 51 x 51 circular patch, `--different_pos`,
40 synthetic items resident on the device, chunk 4, files on tmpfs, seeded synthetic weights.  Forms, alternating in one process:

  no_files  evaluate_patch without save_path: the baseline;
  png, jpg  evaluate_patch with save_path, strips as `viz%03d.png` (zlib, lossless) / `viz%03d.jpg` (PIL's defaults, the script's);
  host      the literal host path from this project's mirrors, for `--host-items` items of one evaluation: two frames, two flows and
            the scored ground truth copied to the host, `flowlib.viz_strip_host` (flow_to_image four times, resize, erode,
            concatenate).  No file is written and no forward runs in this form: it is the figure alone.

Every shape is warmed, every timed window ends in a synchronise, the figures are medians of `--windows` alternating windows.  The
device time of `ufr_eval_blend_gt`, `ufr_viz_ranges` and `ufr_viz_strip` comes from device events in a run of its own; the strip's
rate is the bytes the algorithm needs (every input once, the strip once) over that time, as a share of the 6.3 TB/s streaming copy.
The host time of the file encoders alone (zlib / PIL on one strip) is measured too: it shows whether the encode or the device sets
the per-item time.

    python tools/bench_figures.py [--windows 5] [--items 40] [--out profiles/figures.json]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
STREAM_COPY_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--items", type=int, default=40)
    ap.add_argument("--host-items", type=int, default=4, help="items of the literal host path per window")
    ap.add_argument("--chunk", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "figures.json"))
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--patch", type=int, default=51)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_figures: no HIP device; nothing is measured without one")
    from understanding_flow_robustness_amd import flowlib
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
        valid = (torch.rand(1, 1, hg, wg, generator=g) > 0.3).float()
        gt = torch.cat((torch.randn(1, 2, hg, wg, generator=g) * 5.0 * valid, valid), 1).to(DEV)
        loader.append((past, tgt, ref, gt))
    patch = np.random.RandomState(0).rand(1, 3, S, S)
    disc = createCircularMask(S, S).astype("float32")
    mask = np.array([[disc, disc, disc]])
    tmp_root = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    out_dir = tempfile.mkdtemp(prefix="ufr_figures_", dir=tmp_root)

    def evaluate(image_format=None, items=loader):
        np.random.seed(1337)
        save = None if image_format is None else os.path.join(out_dir, image_format)
        return pe.evaluate_patch(net, items, patch, mask, patch.shape, args, chunk=opt.chunk, save_path=save,
                                 image_format=image_format or "jpg")

    # what the strips are built from, for the host form: device tensors of the first chunks
    kept = []
    pe.evaluate_patch._debug_figures = lambda first, *t: kept.append([x.clone() for x in t]) if len(kept) * opt.chunk < opt.host_items else None
    try:
        with_files = evaluate("png", loader[:max(opt.host_items, 2 * opt.chunk + 1)])      # warms the ragged chunk too
    finally:
        pe.evaluate_patch._debug_figures = None
    operands = [torch.cat([c[i] for c in kept])[:opt.host_items] for i in range(5)]

    def host():
        strips = []
        for k in range(opt.host_items):
            cpu = [t[k].cpu().numpy() for t in operands]                                     # five D2H copies per item, like the script
            strips.append(flowlib.viz_strip_host(*cpu))
        return strips

    # the device strips and the host strips agree before anything is timed
    device_strips = flowlib.viz_strip(*operands).cpu().numpy()
    host_strips = host()
    differing = int(sum((a != b).sum() for a, b in zip(device_strips, host_strips)))
    print(f"device strips against the host mirror on {opt.host_items} items: {differing} differing bytes", flush=True)
    if differing > 10:
        raise SystemExit("bench_figures: the device strips differ from the host mirror; nothing is timed")
    evaluate("jpg", loader[:2 * opt.chunk + 1])
    plain = evaluate(None)
    same = 2 * opt.chunk                                        # the items both runs served in chunks of the same size
    if not np.array_equal(plain.per_item[:same], with_files.per_item[:same]):
        raise SystemExit("bench_figures: per_item differs with and without files; nothing is timed")
    torch.cuda.synchronize()

    forms = {"no_files": lambda: evaluate(None), "png": lambda: evaluate("png"), "jpg": lambda: evaluate("jpg"), "host": host}
    per = {"no_files": n, "png": n, "jpg": n, "host": opt.host_items}
    times = {k: [] for k in forms}
    for w in range(opt.windows):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
        print(f"window {w}: " + ", ".join(f"{k} {v[-1] / per[k] * 1e3:.2f} ms/item" for k, v in times.items()), flush=True)
    # the entries' device time, from device events, in a run of its own
    stages = ("paste", "forward", "metrics", "blend", "ranges", "strip")
    runs = [stage_ms(recorded_events(pe.evaluate_patch, lambda: evaluate("png")), stages) for _ in range(3)]
    split = {s: statistics.median(r[s] for r in runs) / n for s in stages}
    strip_bytes = 18 * H * W + 40 * H * W + 8 * hg * wg          # the strip once; two frames and two flows once; u and v of g once
    strip_tbs = strip_bytes / (split["strip"] * 1e-3) / 1e12
    # the encoders alone, on the host: one strip
    strip = device_strips[0]
    encode = {}
    for fmt in ("png", "jpg"):
        path = os.path.join(out_dir, "encode_probe." + fmt)
        if pe.checked_image_format(fmt) != fmt:
            continue
        reps = []
        for _ in range(5):
            t0 = time.perf_counter()
            pe.save_strip(path, strip, fmt)
            reps.append(time.perf_counter() - t0)
        encode[fmt] = {"ms": statistics.median(reps) * 1e3, "bytes": os.path.getsize(path)}
    shutil.rmtree(out_dir, ignore_errors=True)
    ms = {k: statistics.median(v) / per[k] * 1e3 for k, v in times.items()}
    result = {
        "what": "patch evaluation with its figures and result files, --different_pos", "network": "FlowNetC (synthetic weights, seed 0)",
        "frame": [H, W], "ground_truth": [hg, wg], "patch": S, "items": n, "chunk": opt.chunk, "host_items": opt.host_items,
        "windows": opt.windows, "device": torch.cuda.get_device_name(0), "files_on": tmp_root or tempfile.gettempdir(),
        "differing_bytes_device_vs_host": differing,
        "ms_per_item": ms,
        "ms_per_item_all_windows": {k: [t / per[k] * 1e3 for t in v] for k, v in times.items()},
        "figure_ms_per_item": {"png": ms["png"] - ms["no_files"], "jpg": ms["jpg"] - ms["no_files"], "host": ms["host"]},
        "device_ms_per_item": split,
        "strip": {"bytes_per_item": strip_bytes, "TB_per_s": strip_tbs, "share_of_streaming_copy": strip_tbs / STREAM_COPY_TBS},
        "host_encode_one_strip": encode,
        "conditions": "measured once, one box; synthetic frames resident on the device (no data loading); wall clock around whole "
                      "evaluations, each window ends in a synchronise; the host form builds the strips only (no forward, no files)",
    }
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("ms_per_item", "figure_ms_per_item", "device_ms_per_item", "strip", "host_encode_one_strip")}),
          flush=True)


if __name__ == "__main__":
    main()
