"""The global-attack evaluation (global_eval.py) at the universal perturbation's size: FlowNetC, 256 x 640 frames, the ground truth at
its own size, 200 synthetic items resident on the device, seeded synthetic weights.  Two modes -- a fixed perturbation
(`--universal_evaluation`) and I-FGSM at 3 steps per item -- and in each two forms in one process, alternating:

  literal   perturb_main.run's loop (:466-812) from this project's mirrors: `predict_flow` at batch 1 twice, the attack, five D2H
            copies per item, and at the end `validate`'s float32 metrics on re-uploaded host arrays (six `.item()` per item) and
            numpy norms (global_eval.validate_rows);
  native    evaluate_perturbation at chunk 1, 4 and 8.

The forms' per-item tables are compared first (on the first `--check` items).  Every shape is warmed, every timed window ends in a
synchronise, the figures are medians of `--windows` alternating windows.  The device time of `ufr_global_apply`, the forward and
`ufr_global_metrics` comes from device events in a run of its own (fixed-perturbation mode).

    python tools/bench_global_eval.py [--windows 5] [--items 200] [--out profiles/global_eval.json]"""
import argparse
import json
import os
import random
import statistics
import sys
import time
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def literal_loop(net, args, loader, perturb_model=None, noise=None):
    from understanding_flow_robustness_amd import global_eval as ge
    from understanding_flow_robustness_amd.flownets.utils_model import predict_flow
    noises0, noises1, origins, outputs, gts = [], [], [], [], []
    for image0, image1, ground_truth, ground_truth_downsampled in loader:
        gts.append(np.squeeze(ground_truth.cpu().numpy()))
        with torch.no_grad():
            flow_origin = predict_flow(net, None, image0, image1, args)
        if noise is not None:
            image0_output, image1_output = torch.clamp(image0 + noise[0], 0.0, 1.0), torch.clamp(image1 + noise[1], 0.0, 1.0)
            noise0_output, noise1_output = torch.clone(noise[0]), torch.clone(noise[1])
        else:
            noise0_output, noise1_output, image0_output, image1_output = perturb_model.forward(net, image0, image1,
                                                                                                ground_truth_downsampled)
        with torch.no_grad():
            flow_output = predict_flow(net, None, image0_output, image1_output, args)
        noises0.append(np.transpose(np.squeeze(noise0_output.detach().cpu().numpy()), (1, 2, 0)))
        noises1.append(np.transpose(np.squeeze(noise1_output.detach().cpu().numpy()), (1, 2, 0)))
        origins.append(np.squeeze(flow_origin.detach().cpu().numpy()))
        outputs.append(np.squeeze(flow_output.detach().cpu().numpy()))
    with torch.no_grad():
        return ge.validate_rows(noises0, noises1, origins, outputs, gts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--items", type=int, default=200)
    ap.add_argument("--check", type=int, default=16, help="items whose tables are compared between the forms before timing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_eval.json"))
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=640)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_global_eval: no HIP device; nothing is measured without one")
    from understanding_flow_robustness_amd import global_eval as ge
    from understanding_flow_robustness_amd.chunked_eval import recorded_events, stage_ms
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    from understanding_flow_robustness_amd.perturb_model import PerturbationsModel
    H, W, n = opt.height, opt.width, opt.items
    args = Namespace(flownet="FlowNetC", flow_loss="l2")
    net = fetch_model(args, synthetic_seed=0).to(DEV)
    g = torch.Generator().manual_seed(0)
    loader = []
    for _ in range(n):
        image0, image1 = (torch.rand(1, 3, H, W, generator=g).to(DEV) for _ in range(2))
        gt = torch.cat((torch.randn(1, 2, H, W, generator=g) * 5.0, (torch.rand(1, 1, H, W, generator=g) > 0.3).float()), 1).to(DEV)
        loader.append((image0, image1, gt, gt))
    eps = 0.02
    noise = tuple((torch.rand(1, 3, H, W, generator=g) * 2 * eps - eps).to(DEV) for _ in range(2))
    make_pm = lambda: PerturbationsModel(perturb_method="ifgsm", perturb_mode="both", output_norm=eps, n_step=3, learning_rate=0.005,
                                         args=args)
    chunks = (1, 4, 8)

    def seed():
        torch.manual_seed(0)
        random.seed(0)
        np.random.seed(0)

    result_modes = {}
    for mode in ("fixed_noise", "ifgsm_3_steps"):
        kw = (lambda: dict(noise=noise)) if mode == "fixed_noise" else (lambda: dict(perturb_model=make_pm()))

        def native(chunk, items=loader):
            seed()
            return ge.evaluate_perturbation(net, items, args, chunk=chunk, **kw())

        def literal(items=loader):
            seed()
            return literal_loop(net, args, items, **kw())

        forms = {"literal": literal}
        forms.update({f"native_chunk{c}": (lambda c=c: native(c)) for c in chunks})
        # warm every shape (a ragged last chunk included), and compare the tables before anything is timed
        head = loader[:opt.check]
        want = literal(head)
        agreement = {}
        for c in chunks:
            got = native(c, head).per_item
            native(c, loader[:2 * c + 1])
            rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(b)))
            agreement[f"chunk{c}_noise_rel"] = rel(got[:, :4], want[:, :4])
            agreement[f"chunk{c}_epe_l1_rel"] = rel(got[:, 4:8], want[:, 4:8])
            agreement[f"chunk{c}_cos_abs"] = float(np.max(np.abs(got[:, 8:] - want[:, 8:])))
        torch.cuda.synchronize()
        print(f"{mode}: agreement:", json.dumps(agreement), flush=True)
        if not max(agreement.values()) <= 1e-4:
            raise SystemExit("bench_global_eval: the forms disagree; nothing is timed")
        times = {k: [] for k in forms}
        for w in range(opt.windows):
            for name, fn in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
            print(f"{mode}: window {w}: " + ", ".join(f"{k} {v[-1]:.3f} s" for k, v in times.items()), flush=True)
        # device time of the stages, from device events, in a run of its own per chunk size (in the attack mode "apply" is the
        # stacking of what the attacks returned; the attacks themselves run between the chunks and are not inside these events)
        split = {}
        for c in chunks:
            acc = stage_ms(recorded_events(ge.evaluate_perturbation, lambda: native(c)), ("apply", "forward", "metrics"))
            total = sum(acc.values())
            split[f"chunk{c}"] = {"ms_per_item": {k: v / n for k, v in acc.items()},
                                  "share": {k: (v / total if total > 0 else 0.0) for k, v in acc.items()}}
        result_modes[mode] = {
            "agreement_first_items": dict(agreement, items=len(head)),
            "seconds_per_evaluation": {k: statistics.median(v) for k, v in times.items()},
            "ms_per_item": {k: statistics.median(v) / n * 1e3 for k, v in times.items()},
            "seconds_all_windows": times,
            "device_stages": split,
        }
    result = {
        "what": "global-attack evaluation over a validation set: clean forward, perturbation, attacked forward, validate's table",
        "network": "FlowNetC (synthetic weights, seed 0)", "frame": [H, W], "ground_truth": [H, W], "items": n,
        "windows": opt.windows, "device": torch.cuda.get_device_name(0), "modes": result_modes,
        "conditions": "measured once, one box; synthetic frames resident on the device (no data loading in either form); wall "
                      "clock around whole evaluations, each window ends in a synchronise; no speed gate",
    }
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({m: {k: r[k] for k in ("ms_per_item", "device_stages")} for m, r in result_modes.items()}), flush=True)


if __name__ == "__main__":
    main()
