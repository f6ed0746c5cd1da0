"""`PerturbationsModel.forward` of the iterative attacks that used to run step by step, at the README's global-attack size:
FlowNetC, 256 x 640, seeded synthetic weights and frames, B = 1 and 8, 40 steps.  Three configurations -- I-FGSM with input
diversity, MI-FGSM, MI-FGSM with input diversity (probability 0.5) -- each in two forms in one process, alternating:

  fused   the cached, graph-captured step with the launches of csrc/perturb_step.hip, the transforms of all steps drawn up front;
  eager   `fused=False`: eager autograd per step, torch operators for the momentum and the resize, host RNG draws in between.

Both forms see the same seeds; their outputs are compared first (the share of pixels that differ by more than 1e-6 is recorded).
Every shape is warmed (the graph is captured before anything is timed), every timed window ends in a synchronise, the figures
are medians of `--windows` alternating windows.  There is no speed gate: the numbers are recorded, whichever form wins.

    python tools/bench_perturb_model.py [--windows 5] [--steps 40] [--out profiles/perturb_model.json]"""
import argparse
import json
import os
import random
import statistics
import sys
import time
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
CONFIGS = (("ifgsm_diverse", "ifgsm", 0.5), ("mifgsm", "mifgsm", 0.0), ("mifgsm_diverse", "mifgsm", 0.5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perturb_model.json"))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_perturb_model: no HIP device; nothing is measured without one")
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    from understanding_flow_robustness_amd.perturb_model import PerturbationsModel
    H, W = opt.height, opt.width
    args = Namespace(flownet="FlowNetC", flow_loss="l2")
    net = fetch_model(args, synthetic_seed=0).to(DEV)
    result = {"what": "PerturbationsModel.forward, seconds per call", "network": "FlowNetC (synthetic weights, seed 0)", "frame": [H, W],
              "n_step": opt.steps, "windows": opt.windows, "device": torch.cuda.get_device_name(0), "batches": {}}
    for B in opt.batches:
        g = torch.Generator().manual_seed(B)
        i0, i1 = torch.rand(B, 3, H, W, generator=g).to(DEV), torch.rand(B, 3, H, W, generator=g).to(DEV)
        gt = torch.cat((3 * torch.randn(B, 2, H, W, generator=g), (torch.rand(B, 1, H, W, generator=g) > 0.2).float()), 1).to(DEV)
        result["batches"][str(B)] = {}
        for tag, method, p in CONFIGS:
            def call(fused):
                pm = PerturbationsModel(perturb_method=method, perturb_mode="both", output_norm=0.02, n_step=opt.steps,
                                        learning_rate=0.002, momentum=0.47, probability_diverse_input=p, args=args, fused=fused)
                torch.manual_seed(7)
                random.seed(7)
                return pm.forward(net, i0, i1, gt)
            forms = {"fused": lambda: call(True), "eager": lambda: call(False)}
            a, b = forms["fused"](), forms["eager"]()                 # warm both; the fused call captures its graph here
            torch.cuda.synchronize()
            differing = max(float(((x - y).abs() > 1e-6).float().mean()) for x, y in zip(a[:2], b[:2]))
            times = {k: [] for k in forms}
            for w in range(opt.windows):
                for name, fn in forms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[name].append(time.perf_counter() - t0)
            ms = {k: statistics.median(v) * 1e3 for k, v in times.items()}
            result["batches"][str(B)][tag] = {"ms": ms, "ms_all_windows": {k: [x * 1e3 for x in v] for k, v in times.items()},
                                              "eager_over_fused": ms["eager"] / ms["fused"], "share_of_pixels_differing": differing,
                                              "probability_diverse_input": p}
            print(json.dumps({"B": B, "config": tag, **result["batches"][str(B)][tag]["ms"], "differing": differing}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
