"""Golden fixtures of input diversity and MI-FGSM, produced by running the REFERENCE's own code on the CPU:
global_attacks/perturb_model.py `PerturbationsModel` (:148-272), its `__diverse_input` (:759-821), `__ifgsm` (:475-619) and
`__mifgsm` (:621-757) on models/FlowNetC.py; see make_golden.py for the contract.

    python tests/golden/make_golden_perturb_di.py [golden] [check]

`golden` writes perturb_model_di_flownetc.npz.  Frames, weights seed and 2-channel ground truth are those of
make_golden_models.gen_perturb_model (the same generator draws in the same order; the arrays themselves stay in
perturb_model_flownetc.npz and only their float64 sums are repeated here), plus a validity channel for the 3-channel ground truth.
Under `torch.manual_seed(seed)` / `random.seed(seed)` it stores
  * four consecutive `__diverse_input` calls at p = 0.5 on the top-left 20 x 30 corner of the frames and of the 3-channel ground
    truth: the outputs, the values `random.randint` returned inside them (`di_rows`: apply, nh, nw, top, left), and the next
    `torch.rand(1)` / `random.random()` afterwards, which pin how much of either stream was consumed;
  * noise0 / noise1 of `ifgsm` and `mifgsm` at p = 1.0 with the 2-channel ground truth and of `mifgsm` at p = 0.5 with the
    3-channel one (n_step 3, lr 0.008, eps 0.02, mu 0.47, flow_loss l2), with the generator states' next draws alike.

`check` measures how far the reference stays inside the tests' acceptance condition (share of pixels differing by more than
1e-6 below 5e-3) when only rounding changes: the reference against itself with every weight multiplied by 1 +- r (sign drawn per
element).  With the seeds below, worst of the three configurations and both frames:
  r = 3e-7: no pixel differs; r = 3e-6: 4.07e-5 of the pixels differ   (the condition is 5e-3)
"""
from __future__ import annotations

import os
import random
import sys
import warnings
from argparse import Namespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_harness as rh  # noqa: E402
from make_golden import save  # noqa: E402
from make_golden_models import _ref_flownetc  # noqa: E402
from understanding_flow_robustness_amd.flownets.weights import state_dict_digest  # noqa: E402

DI_SEED = 18                                  # the four __diverse_input calls
CONFIGS = (("ifgsm_di", "ifgsm", 1.0, 2, 11), ("mifgsm_di", "mifgsm", 1.0, 2, 12), ("mifgsm_di_valid", "mifgsm", 0.5, 3, 13))
HYPER = dict(perturb_mode="both", output_norm=0.02, n_step=3, learning_rate=0.008, momentum=0.47)
CORNER = (20, 30)


def inputs(net):
    """gen_perturb_model's draws, then the validity channel."""
    H, W = 64, 128
    g = torch.Generator().manual_seed(121)
    i0, i1 = torch.rand(1, 3, H, W, generator=g), torch.rand(1, 3, H, W, generator=g)
    with torch.no_grad():
        gt = net(i0, i1) + 3.0 * torch.randn(1, 2, H, W, generator=g)
    valid = (torch.rand(1, 1, H, W, generator=g) > 0.2).float()
    return i0, i1, gt, torch.cat((gt, valid), 1)


def _model(pm, method, p):
    return pm.PerturbationsModel(perturb_method=method, probability_diverse_input=p, device=torch.device("cpu"), disparity=False,
                                 targeted=False, print_out=False, args=Namespace(flownet="FlowNetC", flow_loss="l2"), **HYPER)


def _attack(pm, net, method, p, seed, i0, i1, gt):
    torch.manual_seed(seed)
    random.seed(seed)
    n0, n1, _, _ = _model(pm, method, p).forward(net, i0.clone(), i1.clone(), gt.clone())
    return n0.detach(), n1.detach(), torch.rand(1), random.random()


def gen_golden():
    pm = rh.ref_module("global_attacks.perturb_model")
    net, sd = _ref_flownetc(seed=0)
    i0, i1, gt2, gt3 = inputs(net)
    out = dict(weight_digest=state_dict_digest(sd), img0_sum=i0.double().sum(), img1_sum=i1.double().sum(), gt_sum=gt2.double().sum(),
               valid=gt3[:, 2:].to(torch.uint8), di_seed=DI_SEED)
    # four consecutive transforms at p = 0.5; the values random.randint hands the reference are recorded as it draws them
    h, w = CORNER
    c0, c1, cg = i0[..., :h, :w].contiguous(), i1[..., :h, :w].contiguous(), gt3[..., :h, :w].contiguous()
    model = _model(pm, "ifgsm", 0.5)
    drawn, real = [], random.randint
    torch.manual_seed(DI_SEED)
    random.seed(DI_SEED)
    rows = []
    for k in range(4):
        del drawn[:]
        random.randint = lambda a, b: (drawn.append(real(a, b)), drawn[-1])[1]
        try:
            o0, o1, og = model._PerturbationsModel__diverse_input(c0.clone(), c1.clone(), cg.clone())
        finally:
            random.randint = real
        rows.append([1] + list(drawn) if drawn else [0, h, w, 0, 0])
        out[f"di{k}_img0"], out[f"di{k}_img1"], out[f"di{k}_gt"] = o0, o1, og
    out["di_rows"] = np.asarray(rows, dtype=np.int32)
    out["di_next_rand"], out["di_next_random"] = torch.rand(1), np.float64(random.random())
    print("rows", rows)
    for tag, method, p, cg_n, seed in CONFIGS:
        n0, n1, nr, nrand = _attack(pm, net, method, p, seed, i0, i1, gt2 if cg_n == 2 else gt3)
        out[f"{tag}_noise0"], out[f"{tag}_noise1"], out[f"{tag}_seed"] = n0, n1, seed
        out[f"{tag}_next_rand"], out[f"{tag}_next_random"] = nr, np.float64(nrand)
    save("perturb_model_di_flownetc", **out)


def gen_check():
    """The reference against itself under relative weight jitter: the share of pixels that differ by more than 1e-6."""
    pm = rh.ref_module("global_attacks.perturb_model")
    net, sd = _ref_flownetc(seed=0)
    i0, i1, gt2, gt3 = inputs(net)
    base = {tag: _attack(pm, net, method, p, seed, i0, i1, gt2 if cg == 2 else gt3)[:2] for tag, method, p, cg, seed in CONFIGS}
    for r in (3e-7, 3e-6):
        g = torch.Generator().manual_seed(77)
        jit = {k: (v * (1.0 + r * (2.0 * torch.randint(0, 2, v.shape, generator=g) - 1.0)).to(v.dtype) if v.is_floating_point() else v)
               for k, v in sd.items()}
        net.load_state_dict(jit)
        worst = 0.0
        for tag, method, p, cg, seed in CONFIGS:
            got = _attack(pm, net, method, p, seed, i0, i1, gt2 if cg == 2 else gt3)[:2]
            for a, b in zip(got, base[tag]):
                worst = max(worst, float(((a - b).abs() > 1e-6).float().mean()))
        print(f"jitter {r:g}: worst share of differing pixels {worst:.2e}")
    net.load_state_dict(sd)


GENERATORS = {"golden": gen_golden, "check": gen_check}

if __name__ == "__main__":
    torch.set_num_threads(8)
    rh.install()
    for which in sys.argv[1:] or list(GENERATORS):
        print(f"== {which}")
        GENERATORS[which]()
