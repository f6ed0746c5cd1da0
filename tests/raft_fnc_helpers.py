"""Shared by test_raft_fnc_cpu.py and test_raft_fnc_gpu.py: the fixtures of tests/golden/make_golden_raft_fnc.py."""
from argparse import Namespace

import torch

from conftest import load_golden, t

NAME = "RAFT_FlowNetCEncoder_WoContext"
WEIGHT_SEED = 4


def fetch(device="cpu", **extra):
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    args = Namespace(flownet=NAME, **extra)
    return fetch_model(args, synthetic_seed=WEIGHT_SEED).to(device), args


def encoder_case(device="cpu"):
    """raft_fnc_encoder_64x96: the golden, the frames in [0, 1) and the four weights of the functional, regenerated from its seed."""
    z = load_golden("raft_fnc_encoder_64x96")
    B, _, h, w = z["fmap1"].shape
    g = torch.Generator().manual_seed(int(z["seed"]))
    x1, x2 = torch.rand(B, 3, 8 * h, 8 * w, generator=g), torch.rand(B, 3, 8 * h, 8 * w, generator=g)
    ws = [torch.randn(B, c, h, w, generator=g) for c in (256, 256, 128, 128)]
    for got, key in ((x1.double().sum(), "x1_sum"), (x2.double().sum(), "x2_sum"), (sum(v.double().sum() for v in ws), "w_sum")):
        assert abs(float(got) - float(z[key])) <= 1e-6 * abs(float(z[key])) + 1e-6, "input generator drift"
    return z, x1.to(device), x2.to(device), [v.to(device) for v in ws]


def model_golden():
    """raft_fnc_128x192 and its two gradient files as one dict with raft_128x192.npz's keys."""
    z = load_golden("raft_fnc_128x192")
    z.update(load_golden("raft_fnc_128x192_g1"))
    z.update(load_golden("raft_fnc_128x192_g2"))
    return z


def check_weights(net, z):
    from understanding_flow_robustness_amd.flownets.weights import state_dict_digest
    digest = state_dict_digest({k: v.detach().cpu() for k, v in net.state_dict().items()})
    assert abs(digest - float(z["weight_digest"])) <= 1e-6 * float(z["weight_digest"]), "synthetic weights drifted from the fixture's"


def encoder_heads(net, x1, x2, model_path=False):
    """(fmap1, fmap2, net0, inp) as RAFT.forward makes them on [0, 1] frames through predict_flow's x 255; by default spelled out in torch operators."""
    im1, im2 = 2 * ((x1 * 255.0) / 255.0) - 1.0, 2 * ((x2 * 255.0) / 255.0) - 1.0
    if model_path:                        # the model's own route: the engines when they serve the tensors, else the torch spelling
        return net.context_features(im1.contiguous(), im2.contiguous())
    fmap1, fmap2 = net.fnet([im1.contiguous(), im2.contiguous()])
    n, i = torch.split(net.conv_redir(fmap1), [128, 128], dim=1)
    return fmap1, fmap2, torch.tanh(n), torch.relu(i)


def check_encoder(z, outs, grads):
    """FlowNetC's gates (tests/test_flownetc_flex_gpu.py:100-104)."""
    from closeness import assert_close
    for name, o in zip(("fmap1", "fmap2", "net0", "inp"), outs):
        assert_close(o, t(z[name]), rtol=1e-4, atol_scale=1e-5, what=name)
    for name, g in zip(("g1", "g2"), grads):
        assert_close(g, t(z[name]), rtol=1e-3, atol_scale=2e-4, what=f"gradient {name}")
