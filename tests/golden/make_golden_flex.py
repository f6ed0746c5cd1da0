"""Golden fixtures of the Robust FlowNetC family, produced by running the REFERENCE's own classes on the CPU
(models/FlowNetC_flexible_larger_field.py with kernel_size 3 / number_of_reps 3, models/FlowNetC_predict_bias.py,
patch_attacks/main.py::attack); see make_golden.py for the contract.

    python tests/golden/make_golden_flex.py [keys] [fwd] [attack]

Weights come from synthetic_state_dict (per-key seeded): only inputs, outputs and a weight checksum are stored.  The
384 x 640 attack trace stores the seed of its frames and target (plus checksums), and the patch's bounding box only.
"""
from __future__ import annotations

import json
import os
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
from understanding_flow_robustness_amd.flownets.weights import state_dict_digest, synthetic_state_dict  # noqa: E402

ATTACK_HW, ATTACK_SEED, ATTACK_S = (384, 640), 61, 25
ATTACK_PLACES = (("mid", (171, 301)), ("edge", (0, 615)))


def _ref(kind, seed=0):
    if kind == "flex":
        net = rh.ref_module("models.FlowNetC_flexible_larger_field").FlowNetC_flexible_larger_field(
            kernel_size=3, number_of_reps=3, dilation=1)
    else:
        net = rh.ref_module("models.FlowNetC_predict_bias").FlowNetC_predict_bias()
    net = net.eval()
    sd = synthetic_state_dict(net.state_dict(), seed=seed)
    net.load_state_dict(sd)
    return net, sd


def attack_inputs():
    """Frames and target of the 384 x 640 trace (the test regenerates them from the same seed)."""
    H, W = ATTACK_HW
    g = torch.Generator().manual_seed(ATTACK_SEED)
    tgt, ref = torch.rand(1, 3, H, W, generator=g), torch.rand(1, 3, H, W, generator=g)
    target = torch.randn(1, 2, H, W, generator=g)
    return tgt, ref, target, g


def circle_patch(S, g):
    """The patch box [1,3,S,S] and its circular mask (utils_patch.py:236-247: radius S/2 - 2), values U[0,1)."""
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    c = S // 2
    mask = ((yy - c) ** 2 + (xx - c) ** 2 <= (c - 2) ** 2).float().expand(1, 3, S, S).contiguous()
    return torch.rand(1, 3, S, S, generator=g) * mask, mask


def gen_keys():
    out = {}
    for tag, kind in (("FlowNetC_flexible_larger_field_k3_reps3", "flex"), ("FlowNetC_predict_bias", "bias")):
        net, _ = _ref(kind)
        out[tag] = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    path = os.path.join(HERE, "flex_state_dict_keys.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print(f"wrote {path}")


FWD_CASES = (("flex", "flownetc_flex_k3r3_fwd_64x128", (2, 64, 128), 71), ("flex", "flownetc_flex_k3r3_fwd_128x192", (1, 128, 192), 72),
             ("bias", "flownetc_predict_bias_fwd_64x128", (2, 64, 128), 73))


def fwd_inputs(B, H, W, seed):
    """Frames and cosine target of a forward fixture (the test regenerates them from the stored seed)."""
    g = torch.Generator().manual_seed(seed)
    x1, x2 = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
    return x1, x2, torch.randn(B, 2, H, W, generator=g)


# Every stem pre-activation of a forward fixture's frames lies at least this far from zero, relative to its layer's largest
# |pre-activation| (float64).  A LeakyReLU whose pre-activation is within float32 rounding of zero takes slope 1 in one float32
# evaluation and 0.1 in another, and every image gradient behind it moves: the first 64 x 128 draw (seed 71) has a stage-2
# unit at -5.9e-9 (2.3e-8 of its layer's largest) that the CPU evaluations put below zero and the device's float32 paths --
# MIOpen's and the engine's alike -- above, 1.5e-2 of max |d loss / d frame 2| on its 23-pixel receptive field.  Drawing
# frames whose stem keeps this margin makes the comparison at FlowNetC's tolerances one of arithmetic, not of rounding luck.
STEM_MARGIN = 2e-7


def stem_margin(net, x1, x2):
    """Smallest |pre-activation| / largest |pre-activation| of any stem layer of the reference module, in float64."""
    layers = ([b[0] for st in (net.convs1, net.convs2, net.convs3) for b in st] if hasattr(net, "convs1")
              else [net.conv1[0], net.conv2[0], net.conv3[0]])
    mean = torch.tensor([0.40066648, 0.39482617, 0.3784785], dtype=torch.float64).view(1, 3, 1, 1)
    x, worst = torch.cat((x1, x2)).double() - mean, 1.0
    with torch.no_grad():
        for c in layers:
            z = torch.nn.functional.conv2d(x, c.weight.double(), c.bias.double(), c.stride, c.padding)
            worst = min(worst, float(z.abs().min() / z.abs().max()))
            x = torch.nn.functional.leaky_relu(z, 0.1)
    return worst


def gen_fwd():
    """Forward flow and d(loss)/d(images), shaped like make_golden_models.gen_flownetc (frames and target as seed + checksums);
    the seed is the first of base, base + 100, ... whose frames keep STEM_MARGIN."""
    for kind, tag, (B, H, W), seed in FWD_CASES:
        net, sd = _ref(kind)
        while stem_margin(net, *fwd_inputs(B, H, W, seed)[:2]) < STEM_MARGIN:
            seed += 100
        margin = stem_margin(net, *fwd_inputs(B, H, W, seed)[:2])
        print(f"{tag}: seed {seed}, stem margin {margin:.2e}")
        x1, x2, tgt = fwd_inputs(B, H, W, seed)
        x1.requires_grad_(True)
        x2.requires_grad_(True)
        flow = net(x1, x2)
        loss = (1 - torch.nn.functional.cosine_similarity(flow, tgt)).mean()
        loss.backward()
        save(tag, seed=seed, x1_sum=x1.double().sum(), x2_sum=x2.double().sum(), target_sum=tgt.double().sum(), flow=flow,
             loss=loss, g1=x1.grad, g2=x2.grad, weight_digest=state_dict_digest(sd), weight_seed=0, stem_margin=margin)


def gen_attack():
    """patch_attacks/main.py:523-613 run verbatim on Robust FlowNetC at 384 x 640 for 2 iterations: cosine and L2 loss at an
    lr whose first update peaks near 0.5 (the +-2 clamp stays inactive), and cosine at the default lr = 1000; a 25-px patch
    in the interior and one at the top edge next to the right edge."""
    main = rh.ref_module("patch_attacks.main")
    net, sd = _ref("flex")
    for p in net.parameters():
        p.requires_grad_(True)
    H, W = ATTACK_HW
    S = ATTACK_S
    tgt, ref, target, g = attack_inputs()
    out = dict(seed=ATTACK_SEED, tgt_sum=tgt.double().sum(), ref_sum=ref.double().sum(), target_sum=target.double().sum(),
               weight_digest=state_dict_digest(sd), weight_seed=0)

    def run(l2, lr, iters, patch0, mask):
        main.args = Namespace(flownet="FlowNetCFlexLarger_k3_reps3", l2=l2, alpha=0.0, lr=lr, max_count=iters, log_terminal=False)
        return main.attack(net, tgt.clone(), None, ref.clone(), patch0.clone(), mask.clone(), patch0.clone(), target.clone(), None)
    for place, (cy, cx) in ATTACK_PLACES:
        pb, mb = circle_patch(S, g)
        patch0, mask = torch.zeros(1, 3, H, W), torch.zeros(1, 3, H, W)
        patch0[:, :, cy:cy + S, cx:cx + S], mask[:, :, cy:cy + S, cx:cx + S] = pb, mb
        out[f"{place}_patch0"], out[f"{place}_mask"], out[f"{place}_yx"] = pb, mb, np.array([cy, cx])
        for name, l2, lr in (("cos", False, None), ("l2", True, None), ("cos_lr1000", False, 1000.0)):
            if lr is None:                   # random-init gradients are tiny: the lr whose first update peaks at 0.5
                _, _, _, p1 = run(l2, 1.0, 1, patch0, mask)
                lr = float(np.float32(0.5 / float(((p1 - patch0) * mask).abs().max())))
            a_t, _, a_r, p = run(l2, lr, 2, patch0, mask)
            box = (slice(None), slice(None), slice(cy, cy + S), slice(cx, cx + S))
            out[f"{place}_{name}_lr"] = np.array(lr)
            out[f"{place}_{name}_patch"] = p[box]
            out[f"{place}_{name}_adv_tgt"] = a_t[box]
            out[f"{place}_{name}_adv_ref"] = a_r[box]
            print(place, name, lr, float(((p - patch0) * mask).abs().max()))
    save("attack_flownetc_flex_k3r3_384x640", **out)


GENERATORS = {"keys": gen_keys, "fwd": gen_fwd, "attack": gen_attack}

if __name__ == "__main__":
    torch.set_num_threads(8)
    rh.install()
    for which in sys.argv[1:] or list(GENERATORS):
        print(f"== {which}")
        GENERATORS[which]()
