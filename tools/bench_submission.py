"""`create_sintel_submission` (validation.py) on Sintel-sized frames: RAFT with seeded synthetic weights at 436 x 1024 (padded to
440 x 1024), two sequences of 25 synthetic frames resident on the device, the `.flo` files written to a tmpfs directory.  Four forms
in one process, alternating:

  literal / literal_warm   `fused=False`: the reference's loop (training/evaluate.py:201-240): F.pad, one batch-1 forward, the
                           prediction copied to the host and written; with `warm_start` the next forward starts from
                           `forward_interpolate` of this one's low-resolution flow;
  fused / fused_warm       `fused=True`: chunks of 4 through one pad, forward and encode launch; with `warm_start` a batch-1 chain
                           whose host read overlaps the next frame.

Every form is warmed, every timed window ends in a synchronise, the figures are medians of `--windows` alternating windows.  The
device time of the stages (interpolate, pad, forward, encode) comes from device events in a run of its own.  `ufr_forward_interpolate`
alone is timed at 55 x 128 (Sintel's 1/8 grid) and 47 x 156 (KITTI's) for 1, 4 and 16 slices (UFR_FORWARD_INTERPOLATE_SLICES is the
fastest), next to the host restatement's scipy call on this machine's CPU.

    python tools/bench_submission.py [--windows 5] [--frames 25] [--out profiles/submission.json]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def time_interpolate(L, reps=200):
    out = {}
    for h, w in ((55, 128), (47, 156)):
        g = torch.Generator().manual_seed(h)
        flow = (10.0 * torch.randn(1, 2, h, w, generator=g)).to(DEV)
        res, want = torch.empty_like(flow), None
        row = {}
        for slices in (1, 4, 16):
            call = lambda: L.check(L.lib().ufr_forward_interpolate_sliced(L.ptr(flow), L.ptr(res), 1, h, w, slices, L.stream()), "interpolate")
            for _ in range(5):
                call()
            torch.cuda.synchronize()
            want = res.clone() if want is None else want
            if not torch.equal(res, want):
                raise SystemExit(f"bench_submission: {slices} slices give another result at {h} x {w}; nothing is timed")
            medians = []
            for _ in range(5):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(reps):
                    call()
                end.record()
                torch.cuda.synchronize()
                medians.append(start.elapsed_time(end) / reps * 1e3)
            row[f"slices_{slices}_us"] = statistics.median(medians)
        from understanding_flow_robustness_amd import validation as V
        host = flow[0].cpu().numpy()
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            V._interpolate_host(host)
            t.append((time.perf_counter() - t0) * 1e3)
        row["host_restatement_ms"] = statistics.median(t)
        out[f"{h}x{w}"] = row
        print(f"forward_interpolate {h} x {w}:", json.dumps(row), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--frames", type=int, default=25, help="frames per sequence (two sequences per pass, two passes)")
    ap.add_argument("--size", default="436x1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "submission.json"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_submission: no HIP device; nothing is measured without one")
    from understanding_flow_robustness_amd import _lib as L
    from understanding_flow_robustness_amd import kitti_io
    from understanding_flow_robustness_amd import validation as V
    from understanding_flow_robustness_amd.chunked_eval import recorded_events, stage_ms
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    kernel = time_interpolate(L)
    H, W = (int(v) for v in opt.size.split("x"))
    args = Namespace(flownet="RAFT")
    net = fetch_model(args, synthetic_seed=2).to(DEV).eval().requires_grad_(False)
    args.mixed_precision = False                         # float32, as the tests run it; RAFT takes its 12 iterations from its own args
    g = torch.Generator().manual_seed(0)
    frames = [(seq, fr) for seq in ("alley_3", "cave_3") for fr in range(opt.frames)]
    make = lambda: [tuple(torch.randint(0, 256, (1, 3, H, W), generator=g).float().to(DEV) for _ in range(2)) + (tail,) for tail in frames]
    loaders = {"clean": make(), "final": []}             # one pass: the second repeats the first
    n = len(frames)
    tmpfs = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    root = tempfile.mkdtemp(prefix="ufr_submission_", dir=tmpfs)
    try:
        def run(fused, warm, tag=None):
            out = os.path.join(root, tag or f"{'fused' if fused else 'literal'}{'_warm' if warm else ''}")
            V.create_sintel_submission(net, 32, warm, out, loaders=loaders, chunk=4, fused=fused)
            return out

        forms = {"literal": (False, False), "fused": (True, False), "literal_warm": (False, True), "fused_warm": (True, True)}
        outs = {k: run(*v) for k, v in forms.items()}    # warms every shape; the files are compared before anything is timed
        torch.cuda.synchronize()
        agreement = {}
        for warm in ("", "_warm"):
            worst, top, same = 0.0, 0.0, True
            for seq, fr in frames:
                name = os.path.join("clean", seq, "frame%04d.flo" % (fr + 1))
                a, b = kitti_io.read_flo(os.path.join(outs["literal" + warm], name)), kitti_io.read_flo(os.path.join(outs["fused" + warm], name))
                worst, top, same = max(worst, float(abs(a - b).max())), max(top, float(abs(a).max())), same and bool((a == b).all())
            agreement["fused" + warm] = {"max_abs_difference": worst, "largest_flow": top, "identical": same}
        print("agreement:", json.dumps(agreement), flush=True)
        if not all(v["max_abs_difference"] <= 1e-4 * v["largest_flow"] for v in agreement.values()):
            raise SystemExit("bench_submission: the forms disagree; nothing is timed")
        times = {k: [] for k in forms}
        for w in range(opt.windows):
            for form, (fused, warm) in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(fused, warm)
                torch.cuda.synchronize()
                times[form].append(time.perf_counter() - t0)
            print(f"window {w}: " + ", ".join(f"{k} {v[-1]:.3f} s" for k, v in times.items()), flush=True)
        stages = {}
        for form in ("fused", "fused_warm"):
            acc = stage_ms(recorded_events(V.create_sintel_submission, lambda: run(*forms[form])), ("interpolate", "pad", "forward", "encode"))
            stages[form] = {"ms_per_frame": {k: v / n for k, v in acc.items()}}
    finally:
        shutil.rmtree(root, ignore_errors=True)
    result = {
        "what": "create_sintel_submission: pad, forward, (warm start: forward_interpolate), unpad, .flo files",
        "network": "RAFT (synthetic weights, seed 2), 12 iterations, float32", "frame": [H, W],
        "pad_left_right_top_bottom": V.InputPadder((1, 3, H, W))._pad, "frames": n, "sequences": 2, "windows": opt.windows,
        "output_directory_on_tmpfs": tmpfs is not None, "device": torch.cuda.get_device_name(0),
        "agreement": agreement,
        "seconds_per_submission": {k: statistics.median(v) for k, v in times.items()},
        "ms_per_frame": {k: statistics.median(v) / n * 1e3 for k, v in times.items()},
        "seconds_all_windows": times,
        "device_stages": stages,
        "forward_interpolate": dict(kernel, default_slices=int(_default_slices())),
        "conditions": "measured once, one box; synthetic frames resident on the device (no data loading in either form); wall clock "
                      "around whole submissions including the file writes, each window ends in a synchronise; no speed gate",
    }
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("ms_per_frame", "device_stages", "forward_interpolate")}), flush=True)


def _default_slices():
    import re
    with open(os.path.join(ROOT, "include", "ufr_hip.h")) as f:
        return re.search(r"#define\s+UFR_FORWARD_INTERPOLATE_SLICES\s+(\d+)", f.read()).group(1)


if __name__ == "__main__":
    main()
