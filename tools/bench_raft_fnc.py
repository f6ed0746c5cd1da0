"""RAFT_FlowNetCEncoder_WoContext's patch-attack iteration on the engines at 384 x 1280: one pair (a canvas-sized patch, the
reference's call) and 8 pairs behind one 51 x 51 patch, all-pairs and on-the-fly correlation, with RAFT's (config C3) iteration of
the same process beside each -- the two models differ in the encoders only (FlowNetC's stem + conv_redir against two
BasicEncoders), so the gap is what the BasicEncoder pair costs.  Plus the context head's two launches on their own.  One JSON line.

    python tools/bench_raft_fnc.py [--steps K] [--rounds R] [--pairs 1,8] [--corr allpairs,alt] [--only fnc|raft]

--only / --pairs / --corr narrow the run to one step, e.g. under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import sys
import time
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

DEV = "cuda:0"
H, W, PATCH = 384, 1280, 51
MODELS = {"fnc": ("RAFT_FlowNetCEncoder_WoContext", 4), "raft": ("RAFT", 2)}


def make_step(flownet, seed, B, alternate):
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model, predict_flow
    from understanding_flow_robustness_amd.patch_attack import PatchAttackStep
    args = Namespace(flownet=flownet, l2=False, alpha=0.0, lr=1000.0, max_count=2, alternate_corr=alternate)
    net = fetch_model(args, synthetic_seed=seed).to(DEV)
    g = torch.Generator().manual_seed(0)
    tgt, ref = torch.rand(B, 3, H, W, generator=g).to(DEV), torch.rand(B, 3, H, W, generator=g).to(DEV)
    if B > 1:          # one patch in patch coordinates behind the B pairs
        mask = torch.ones(1, 3, PATCH, PATCH, device=DEV)
        patch = torch.rand(1, 3, PATCH, PATCH, generator=g).to(DEV)
        placed = dict(origins=[(100, 600)] * B)
    else:
        mask = torch.zeros(B, 3, H, W, device=DEV)
        mask[:, :, 100:100 + PATCH, 600:600 + PATCH] = 1
        patch = torch.rand(1, 3, H, W, generator=g).to(DEV)
        placed = {}
    with torch.no_grad():
        target = -torch.cat([predict_flow(net, None, tgt[i:i + 1], ref[i:i + 1], args) for i in range(B)])
    step = PatchAttackStep(net, args, B, H, W, device=DEV, patch_hw=(PATCH, PATCH) if B > 1 else None)
    step.load(tgt, ref, patch, mask, patch, target, **placed)
    step.run(0)                                   # warm-up + graph capture
    step.enqueue(2)
    torch.cuda.synchronize()
    return step


def timed(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step.enqueue(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def context_head(B, iters=50):
    """The two launches of csrc/raft_context_head.hip on [B, 256, 48, 160] with HIP events: us and GB/s of the bytes they must move
    (forward: ctx in, net | inp out; backward: net | inp and both gradients in, g_ctx out)."""
    from understanding_flow_robustness_amd.raft_glue import context_split
    x = torch.randn(B, 256, H // 8, W // 8, device=DEV).requires_grad_(True)
    gn, gi = torch.randn(B, 128, H // 8, W // 8, device=DEV), torch.randn(B, 128, H // 8, W // 8, device=DEV)
    out = {}

    def events(fn):
        for _ in range(5):
            fn()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) * 1e3 / iters

    with torch.no_grad():
        us = events(lambda: context_split(x, 128))
    out["forward"] = dict(us=round(us, 2), mbytes=round(2 * x.numel() * 4 / 1e6, 2), gbytes_per_s=round(2 * x.numel() * 4 / us / 1e3, 1))
    net, inp = context_split(x, 128)
    us = events(lambda: torch.autograd.grad((net, inp), x, (gn, gi), retain_graph=True))
    out["backward"] = dict(us=round(us, 2), mbytes=round(3 * x.numel() * 4 / 1e6, 2), gbytes_per_s=round(3 * x.numel() * 4 / us / 1e3, 1),
                           note="event time of autograd.grad: the launch plus one empty() and the autograd node")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pairs", default="1,8")
    ap.add_argument("--corr", default="allpairs,alt")
    ap.add_argument("--only", choices=tuple(MODELS))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_raft_fnc.py needs an MI355X: the product path has no CPU fallback")
    from understanding_flow_robustness_amd import _lib as L
    models = [m for m in MODELS if opt.only in (None, m)]
    cases = []
    for B in (int(p) for p in opt.pairs.split(",")):
        for corr in opt.corr.split(","):
            steps = {m: make_step(*MODELS[m], B, corr == "alt") for m in models}
            times = {m: [] for m in models}
            for _ in range(opt.rounds):            # the models alternate: drift of the clock hits both alike
                for m in models:
                    times[m].append(timed(steps[m], opt.steps))
            med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
            case = dict(pairs=B, correlation="alt_cuda_corr" if corr == "alt" else "all-pairs",
                        **{f"{m}_ms_per_iteration": round(med[m], 3) for m in models},
                        **{f"{m}_ms_rounds": [round(x, 3) for x in times[m]] for m in models})
            if len(models) == 2:
                case["raft_minus_fnc_ms"] = round(med["raft"] - med["fnc"], 3)
            cases.append(case)
            del steps
            torch.cuda.empty_cache()
    line = dict(tool="bench_raft_fnc", hw=[H, W], patch=PATCH, steps_per_round=opt.steps, rounds=opt.rounds, cases=cases,
                context_head={f"{B}_pairs": context_head(B) for B in (1, 8)} if opt.only is None else None,
                vendor_fallbacks={f"{k[0]}: {k[1]}": v for k, v in L.VENDOR_FALLBACKS.items()},
                device=torch.cuda.get_device_name(0))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
