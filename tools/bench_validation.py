"""The validation of the fine-tuning loop (validation.py) on KITTI-sized items: 200 synthetic items resident on the device, seeded
synthetic weights.  Two configurations --

  flownetc_384x1280   `validate_kitti(model, flowNetC=True)`: FlowNetC, items that need no padding (the flowNetC rule keeps a padded
                      height of 384 only);
  raft_376x1242       `validate_kitti(model, iters)`: RAFT, padded KITTI-style to 376 x 1248 (3 + 3 columns);

-- and in each two forms in one process, alternating:

  literal   `fused=False`: the reference's loop (training/evaluate.py:346-392): F.pad, one batch-1 forward per item, a host copy,
            per-pixel numpy arrays in a list, np.concatenate and np.mean at the end;
  native    `fused=True` at chunk 1, 4 and 8.

The forms' results are compared first (on the first `--check` items).  Every shape is warmed, every timed window ends in a
synchronise, the figures are medians of `--windows` alternating windows.  The device time of `ufr_validation_pad`, the forward and
`ufr_validation_metrics` comes from device events in a run of its own.

    python tools/bench_validation.py [--windows 5] [--items 200] [--out profiles/validation.json]"""
import argparse
import json
import os
import statistics
import sys
import time
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
CONFIGS = {
    "flownetc_384x1280": dict(flownet="FlowNetC", seed=0, flowNetC=True, size=(384, 1280), iters=None),
    "raft_376x1242": dict(flownet="RAFT", seed=2, flowNetC=False, size=(376, 1242), iters=12),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--items", type=int, default=200)
    ap.add_argument("--check", type=int, default=8, help="items whose results are compared between the forms before timing")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validation.json"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_validation: no HIP device; nothing is measured without one")
    from understanding_flow_robustness_amd import validation as V
    from understanding_flow_robustness_amd.chunked_eval import recorded_events, stage_ms
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    n, chunks = opt.items, (1, 4, 8)
    configs = {}
    for name in opt.configs.split(","):
        cfg = CONFIGS[name]
        H, W = cfg["size"]
        args = Namespace(flownet=cfg["flownet"])
        net = fetch_model(args, synthetic_seed=cfg["seed"]).to(DEV).eval().requires_grad_(False)
        if not cfg["flowNetC"]:
            args.mixed_precision = False                 # float32, as the tests run it; RAFT takes its 12 iterations from its own args
        g = torch.Generator().manual_seed(0)
        loader = []
        for _ in range(n):
            image1, image2 = (torch.randint(0, 256, (1, 3, H, W), generator=g).float().to(DEV) for _ in range(2))
            flow_gt = (torch.randn(1, 2, H, W, generator=g) * 5.0).to(DEV)
            loader.append((image1, image2, flow_gt, (torch.rand(1, H, W, generator=g) < 0.5).float().to(DEV)))
        head = (net,) if cfg["flowNetC"] else (net, cfg["iters"])

        def evaluate(fused, chunk=1, items=loader):
            return V.validate_kitti(*head, flowNetC=cfg["flowNetC"], loader=items, chunk=chunk, fused=fused, verbose=False)

        forms = {"literal": lambda: evaluate(False)}
        forms.update({f"native_chunk{c}": (lambda c=c: evaluate(True, c)) for c in chunks})
        # warm every shape (a ragged last chunk included), and compare the results before anything is timed
        first = loader[:opt.check]
        want = evaluate(False, items=first)
        agreement = {}
        for c in chunks:
            got = evaluate(True, c, first)
            evaluate(True, c, loader[:2 * c + 1])
            for key in want:
                agreement[f"chunk{c}_{key}_rel"] = abs(float(got[key]) - float(want[key])) / abs(float(want[key]))
        torch.cuda.synchronize()
        print(f"{name}: agreement:", json.dumps(agreement), flush=True)
        if not max(agreement.values()) <= 1e-4:
            raise SystemExit("bench_validation: the forms disagree; nothing is timed")
        times = {k: [] for k in forms}
        for w in range(opt.windows):
            for form, fn in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[form].append(time.perf_counter() - t0)
            print(f"{name}: window {w}: " + ", ".join(f"{k} {v[-1]:.3f} s" for k, v in times.items()), flush=True)
        split = {}
        for c in chunks:
            acc = stage_ms(recorded_events(V._fused_table, lambda: evaluate(True, c)), ("pad", "forward", "metrics"))
            total = sum(acc.values())
            split[f"chunk{c}"] = {"ms_per_item": {k: v / n for k, v in acc.items()},
                                  "share": {k: (v / total if total > 0 else 0.0) for k, v in acc.items()}}
        configs[name] = {
            "network": f"{cfg['flownet']} (synthetic weights, seed {cfg['seed']})", "frame": [H, W], "flowNetC": cfg["flowNetC"],
            "iters": cfg["iters"], "pad_left_right_top_bottom": V.InputPadder((1, 3, H, W), mode="kitti")._pad,
            "agreement_first_items": dict(agreement, items=len(first)),
            "seconds_per_validation": {k: statistics.median(v) for k, v in times.items()},
            "ms_per_item": {k: statistics.median(v) / n * 1e3 for k, v in times.items()},
            "seconds_all_windows": times,
            "device_stages": split,
        }
        del net, loader
        torch.cuda.empty_cache()
    result = {
        "what": "validate_kitti over a validation set: pad, forward, per-item end-point error and outlier share",
        "items": n, "windows": opt.windows, "device": torch.cuda.get_device_name(0), "configurations": configs,
        "conditions": "measured once, one box; synthetic frames resident on the device (no data loading in either form); wall "
                      "clock around whole validations, each window ends in a synchronise; no speed gate",
    }
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({m: {k: r[k] for k in ("ms_per_item", "device_stages")} for m, r in configs.items()}), flush=True)


if __name__ == "__main__":
    main()
