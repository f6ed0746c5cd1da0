"""GPU suite of feature-map capture, replacement and layer statistics on the native engines (feature_maps.py,
flownetc_engine.py `segment_map` / `capture` / `forward_replaced`, csrc/feature_stats.hip).

Capture gate, per key: the native map's error against a float64 torch forward, relative to the map's largest magnitude, is at
most twice the float32 torch spelling's (UFR_ENGINE=0) against the same arbiter -- the factor covers the igemm's "MIOpen fp32
level" accuracy -- floored by the gate tests/test_engine_gpu.py applies to the flow (rtol 1e-4, atol 1e-4 x scale).  With
UFR_FEATURE_MAPS_GATE_OUT set, the measured figures are appended to that file (profiles/feature_maps_gate.txt is one such run)."""
import copy
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from closeness import assert_close
from conftest import t
from test_feature_maps_cpu import KEY_SETS, frames, golden_flex, golden_flownetc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -53
NAMES = ("FlowNetC", "FlowNetCFlexLarger_k3_reps3")
EFFECTIVE = ("conv3ab", "corr", "conv_redir", "conv3_1")


def fetch(name, seed=0):
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    net = fetch_model(Namespace(flownet=name), synthetic_seed=seed).to(DEV)
    for p in net.parameters():
        p.requires_grad_(False)
    return net


@pytest.fixture(scope="module")
def nets():
    return {name: fetch(name) for name in NAMES}


def pair(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 3, H, W, generator=g).to(DEV), torch.rand(B, 3, H, W, generator=g).to(DEV)


def arbiter(net, x1, x2):
    """The 28 maps of a float64 torch forward."""
    net64 = copy.deepcopy(net).double()
    net64.normalize_correctly = lambda im: im.double() - net64._mean64
    with torch.no_grad():
        return net64.forward_torch_maps(x1.double(), x2.double())


def fm():
    from understanding_flow_robustness_amd import feature_maps
    return feature_maps


@pytest.mark.parametrize("B,H,W", [(2, 64, 128), (1, 128, 192)])
@pytest.mark.parametrize("name", NAMES)
def test_native_capture_vs_float64(nets, monkeypatch, name, B, H, W):
    net = nets[name]
    x1, x2 = pair(B, H, W, 11 * B + H)
    flow64, want = arbiter(net, x1, x2)
    monkeypatch.setenv("UFR_ENGINE", "0")
    assert not fm().native_ok(net, x1)
    flow_t, torch32 = fm().forward_with_maps(net, x1, x2)
    monkeypatch.setenv("UFR_ENGINE", "1")
    assert fm().native_ok(net, x1)
    flow_n, native = fm().forward_with_maps(net, x1, x2)
    assert list(native) == fm().FLOWNETC_KEYS == list(torch32)
    lines = [f"{name} B={B} {H}x{W}: key, max|native - f64| / max|f64|, max|torch32 - f64| / max|f64|"]
    failures = []
    for k in fm().FLOWNETC_KEYS:
        ref = want[k]
        scale = float(ref.abs().max())
        assert native[k].shape == ref.shape and native[k].dtype == torch.float32, k
        e_n, e_t = (native[k].double() - ref).abs(), (torch32[k].double() - ref).abs()
        lines.append(f"  {k:22s} {float(e_n.max()) / scale:.3e} {float(e_t.max()) / scale:.3e}")
        bound = torch.maximum(torch.full_like(ref, 2.0 * float(e_t.max())), 1e-4 * ref.abs() + 1e-4 * scale)
        if bool((e_n > bound).any()):
            failures.append(k)
    print("\n".join(lines))
    out = os.environ.get("UFR_FEATURE_MAPS_GATE_OUT")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")
    assert not failures, failures
    assert_close(flow_n, flow64, rtol=1e-4, atol_scale=1e-4, what="flow")
    # the layer statistics: one forward, the kernel over the planes, one host read -- against the captured maps in float64
    means = fm().feature_means(net, x1, x2, Namespace(flownet=name))
    for k in fm().FLOWNETC_KEYS:
        x = native[k].double()
        n = x.shape[2] * x.shape[3]
        mean = (x.sum((2, 3)) / n).cpu().numpy()
        # the kernel bound over n (2 n 2^-53 sum|x| / n), plus the division by n, which rounds once on each side
        bound = (2.0 * U * x.abs().sum((2, 3))).cpu().numpy() + 2.0 * U * np.abs(mean)
        assert means[k].dtype == np.float64 and means[k].shape == mean.shape, k
        assert bool((np.abs(means[k] - mean) <= bound).all()), (k, float(np.abs(means[k] - mean).max()))


@pytest.fixture(scope="module")
def replacement(nets):
    """Batch 2 at 64 x 128 with a different donor per image: the donor pair's maps, captured natively."""
    net = nets["FlowNetC"]
    donor, recipient = pair(2, 64, 128, 21), pair(2, 64, 128, 22)
    _, maps = fm().forward_with_maps(net, *donor)
    plain, plain_maps = fm().forward_with_maps(net, *recipient, None, ["conv3_1", "conv4"])
    assert torch.equal(plain, net(*recipient))
    plain.maps = plain_maps
    return net, donor, recipient, {k: v.clone() for k, v in maps.items()}, plain


@pytest.mark.parametrize("tag", EFFECTIVE)
def test_replaced_forward_vs_torch_spelling_and_zero_copy(replacement, monkeypatch, tag):
    net, donor, recipient, maps, plain = replacement
    keys = KEY_SETS[tag]
    ow = {k: maps[k] for k in keys}
    args = Namespace(flownet="FlowNetC")
    from understanding_flow_robustness_amd.flownets.utils_model import predict_flow
    got, got_maps = predict_flow(net, None, *recipient, args, return_feat_maps=True, overwrite_feat_maps=ow, feat_maps_to_numpy=False)
    monkeypatch.setenv("UFR_ENGINE", "0")
    want, want_maps = predict_flow(net, None, *recipient, args, return_feat_maps=True, overwrite_feat_maps=ow, feat_maps_to_numpy=False)
    monkeypatch.setenv("UFR_ENGINE", "1")
    assert_close(got, want, rtol=1e-4, atol_scale=1e-4, what=f"{tag}: replaced flow")
    # the replacement must show where the gate can see it: with these weights the cost volume moves the flow by 1e-4 of its
    # magnitude only (measured on the torch spelling), but the first map behind it, conv3_1, by 1.3e-3; the other sets move
    # the first map behind them by 8e-2 or more
    down = "conv4" if tag == "conv3_1" else "conv3_1"
    assert_close(got_maps[down], want_maps[down], rtol=1e-4, atol_scale=1e-4, what=f"{tag}: {down} behind the replaced map")
    moved = float((got_maps[down] - plain.maps[down]).abs().max()) / float(plain.maps[down].abs().max())
    assert moved > 5e-4 and not torch.equal(got, plain), f"{tag}: the replacement moved {down} by {moved:.1e} of its magnitude"
    for k in keys:                                       # handed back: the recipient's computed maps, not the donor's
        assert_close(got_maps[k], want_maps[k], rtol=1e-4, atol_scale=1e-4, what=f"{tag}: computed {k}")
        assert not torch.equal(got_maps[k], maps[k])
    inject = net(*recipient, overwrite_feat_maps=ow).clone()         # launches of the replaced segments skipped
    assert torch.equal(inject, got), "computing the replaced maps first changed the flow"
    gt = torch.zeros(2, 3, 64, 128, device=DEV)
    gt[:, 2] = 1.0
    r = fm().replace_features(net, donor, recipient, gt, None, list(keys), args)       # zero-copy: nothing captured or injected
    assert torch.equal(r["adv_flow"], inject), f"{tag}: zero-copy differs from capture-and-inject"
    assert r["epe"] != r["adv_epe"]


@pytest.mark.parametrize("tag", ["conv3a_alone", "conv4"])
def test_ignored_keys_change_nothing(replacement, tag):
    net, _, recipient, maps, plain = replacement
    got = net(*recipient, overwrite_feat_maps={k: maps[k] for k in KEY_SETS[tag]})
    assert torch.equal(got, plain)


def test_ordinary_forward_is_untouched_by_the_analysis_calls(replacement):
    net, donor, recipient, maps, plain = replacement
    fm().forward_with_maps(net, *donor)
    net(*donor, overwrite_feat_maps={"conv3_1": maps["conv3_1"], "corr": maps["corr"]})
    fm().replace_features(net, donor, recipient, torch.ones(2, 3, 64, 128, device=DEV), None, ["conv3a", "conv3b"])
    fm().feature_means(net, *donor)
    assert torch.equal(net(*recipient), plain)


def test_attack_step_after_a_replaced_forward_equals_a_fresh_network():
    """The engine is cached per network and the attack step relies on what its planes hold: 2 iterations of the smallest step of
    tests/test_attack_glue_gpu.py (2 pairs, 128 x 768, a 20 x 20 patch) after analysis calls on the same engine, against the
    same run on a freshly built network."""
    from understanding_flow_robustness_amd.patch_attack import PatchAttackStep
    B, H, W, S = 2, 128, 768, 20
    g = torch.Generator().manual_seed(29)
    tgt, ref = torch.rand(B, 3, H, W, generator=g).to(DEV), torch.rand(B, 3, H, W, generator=g).to(DEV)
    target = torch.randn(B, 2, H, W, generator=g).to(DEV)
    disc = torch.ones(1, 3, S, S, device=DEV)
    patch0 = torch.rand(1, 3, S, S, generator=g).to(DEV)
    args = Namespace(flownet="FlowNetC", l2=False, alpha=0.0, lr=1.0, max_count=2)

    def run(net):
        step = PatchAttackStep(net, args, B, H, W, device=DEV, patch_hw=(S, S), use_graph=False)
        step.load(tgt, ref, patch0, disc, patch0, target, origins=[(3, 5), (60, 400)])
        assert step.eng is not None
        step.run(2)
        torch.cuda.synchronize()
        return step.patch.clone(), step.adv_tgt.detach().clone()

    used = fetch("FlowNetC")
    _, maps = fm().forward_with_maps(used, tgt, ref, None, ["conv3a", "conv3b", "corr"])
    used(ref, tgt, overwrite_feat_maps={"corr": maps["corr"]})
    fm().replace_features(used, (tgt, ref), (ref, tgt), torch.ones(B, 3, H, W, device=DEV), None, ["conv3a", "conv3b"])
    fm().feature_means(used, tgt, ref)
    got, want = run(used), run(fetch("FlowNetC"))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], patch0.expand_as(got[0]))


def test_native_path_vs_the_references_maps_and_overwrite_flows(nets):
    z, donor = golden_flownetc()
    net = nets["FlowNetC"]
    _, (p1, p2) = frames(z["seed"])
    p1, p2 = p1.to(DEV), p2.to(DEV)
    assert fm().native_ok(net, p1)
    flow, maps = fm().forward_with_maps(net, p1, p2)
    assert_close(flow, t(z["flow"]), rtol=1e-4, atol_scale=1e-4, what="flow")
    for k in fm().FLOWNETC_KEYS:
        assert_close(maps[k][0], t(z[k]), rtol=1e-4, atol_scale=1e-4, what=k)
    for tag, keys in KEY_SETS.items():
        got = net(p1, p2, overwrite_feat_maps={k: donor[k] for k in keys})           # numpy [C,H,W]: the reference's form
        assert_close(got, t(z["flow_" + tag]), rtol=1e-4, atol_scale=1e-4, what=tag)
    zf = golden_flex()
    _, (q1, q2) = frames(zf["seed"])
    flow, maps = fm().forward_with_maps(nets["FlowNetCFlexLarger_k3_reps3"], q1.to(DEV), q2.to(DEV))
    assert_close(flow, t(zf["flow"]), rtol=1e-4, atol_scale=1e-4, what="Robust FlowNetC flow")
    for k in ("conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "corr", "conv3_1", "conv6_1", "predict"):
        assert_close(maps[k][0], t(zf[k]), rtol=1e-4, atol_scale=1e-4, what=f"Robust FlowNetC {k}")
