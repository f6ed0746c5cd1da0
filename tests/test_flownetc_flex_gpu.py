"""GPU suite: the Robust FlowNetC family (flownets/flownetc_flex.py) on the engines -- the prefix chain of conv1_direct +
igemm launches (flownetc_engine.py, plane_graph.stem_graph) in front of FlowNetC's native head -- against the reference's
goldens (tests/golden/make_golden_flex.py), the torch / MIOpen spelling and float64 evaluations of the same module."""
import copy
from argparse import Namespace

import pytest
import torch
import torch.nn.functional as F

from closeness import assert_close
from conftest import load_golden, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROBUST = "FlowNetCFlexLarger_k3_reps3"


def _net(name=ROBUST):
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    n = fetch_model(Namespace(flownet=name), synthetic_seed=0).to(DEV)
    for p in n.parameters():
        p.requires_grad_(False)
    return n


@pytest.fixture(scope="module")
def net():
    return _net()


@pytest.fixture(scope="module")
def scaled():
    """Robust FlowNetC whose 12 stem layers keep the activations' scale (weights N(0, 2 / fan_in), biases N(0, 0.05^2)): with the
    seeded Xavier weights every layer halves it, the biases dominate the deep layers and pre-activations within rounding of zero
    -- where two float32 evaluations take different LeakyReLU slopes -- decide the comparison with float64 rather than the
    arithmetic under test (as in test_plane_graph_gpu.py's `_realistic`)."""
    n = _net()
    g = torch.Generator().manual_seed(29)
    with torch.no_grad():
        for stage in n.stem_stages():
            for _, block in stage:
                c = block[0]
                c.weight.copy_(torch.randn(c.weight.shape, generator=g).mul_((2.0 / c.weight[0].numel()) ** 0.5))
                c.bias.copy_(torch.randn(c.bias.shape, generator=g).mul_(0.05))
    return n


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) / float(b.abs().max())


def _fallbacks():
    from understanding_flow_robustness_amd import _lib as L
    return dict(L.VENDOR_FALLBACKS)


def _seeded(seed, *shapes):
    """make_golden_flex.py's inputs: U[0,1) frames, then N(0,1) tensors, from one CPU generator."""
    g = torch.Generator().manual_seed(seed)
    out = [torch.rand(*s, generator=g) for s in shapes[:2]]
    return out + [torch.randn(*s, generator=g) for s in shapes[2:]], g


def _stem64(net, x):
    """The prefix in float64: (stage-2, stage-3) outputs of the mean-subtracted frames."""
    y = x.double() - net._mean64.double()
    outs = []
    for stage in net.stem_stages():
        for _, block in stage:
            c = block[0]
            y = F.leaky_relu(F.conv2d(y, c.weight.double(), c.bias.double(), c.stride, c.padding), 0.1)
        outs.append(y)
    return outs[1], outs[2]


def _double_copy(net):
    cached = {k: net.__dict__.pop(k) for k in [k for k in net.__dict__ if k.startswith("_ufr_")]}   # ctypes: not copyable
    n64 = copy.deepcopy(net).double()
    net.__dict__.update(cached)
    return n64


@pytest.mark.parametrize("name,golden", [(ROBUST, "flownetc_flex_k3r3_fwd_64x128"), (ROBUST, "flownetc_flex_k3r3_fwd_128x192"),
                                         ("FlowNetCFlexLarger_k5_reps0", "flownetc_predict_bias_fwd_64x128")])
def test_whole_network_vs_reference_golden(name, golden, monkeypatch):
    """Forward + image gradients with the engines on (native stem, native head) against the reference's classes run on the CPU, at
    test_engine_gpu.py's tolerances; no convolution of the forward or the backward falls back to the vendor library.  (The fixtures'
    frames keep every stem pre-activation >= 2e-7 of its layer's largest away from zero: make_golden_flex.STEM_MARGIN.)"""
    monkeypatch.setenv("UFR_ENGINE", "1")
    z = load_golden(golden)
    B, _, H, W = z["flow"].shape
    (x1, x2, tgt), _ = _seeded(int(z["seed"]), (B, 3, H, W), (B, 3, H, W), (B, 2, H, W))
    for a, key in ((x1, "x1_sum"), (x2, "x2_sum"), (tgt, "target_sum")):
        assert abs(float(a.double().sum()) - float(z[key])) <= 1e-6 * abs(float(z[key])), "input generator drift"
    net = _net(name)
    before = _fallbacks()
    x1, x2 = x1.to(DEV).requires_grad_(True), x2.to(DEV).requires_grad_(True)
    flow = net(x1, x2)
    assert_close(flow, t(z["flow"]), rtol=1e-4, atol_scale=1e-4, what="flow")
    loss = (1 - F.cosine_similarity(flow, tgt.to(DEV))).mean()
    g1, g2 = torch.autograd.grad(loss, (x1, x2))
    assert_close(g1, t(z["g1"]), rtol=1e-3, atol_scale=2e-4, what="d loss / d frame 1")
    assert_close(g2, t(z["g2"]), rtol=1e-3, atol_scale=2e-4, what="d loss / d frame 2")
    assert _fallbacks() == before
    assert "_ufr_plane_graphs" in net.__dict__ and "_ufr_head_engines" in net.__dict__


def test_native_network_vs_torch_spelling_at_the_benchmark_size(scaled, monkeypatch):
    """Native stem + engine head against the torch / MIOpen spelling (UFR_ENGINE=0) at 384 x 1280, 2 pairs: flow and both image
    gradients, each judged against a float64 evaluation of the same module (the engines may be no further from it than the
    vendor's float32 path, x3)."""
    net = scaled
    B, H, W = 2, 384, 1280
    (x1, x2, gflow), _ = _seeded(5, (B, 3, H, W), (B, 3, H, W), (B, 2, H, W))
    x1, x2, gflow = x1.to(DEV), x2.to(DEV), gflow.to(DEV)
    outs = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("UFR_ENGINE", knob)
        a, b = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
        flow = net(a, b)
        outs[knob] = (flow.detach(), torch.autograd.grad(flow, (a, b), gflow))
    monkeypatch.setenv("UFR_ENGINE", "0")
    n64 = _double_copy(net)
    a, b = x1.double().requires_grad_(True), x2.double().requires_grad_(True)
    c2, c3 = _stem64(n64, torch.cat((a, b)))
    flow64 = n64.head(c2[:B], c3[:B], c3[B:])
    grads64 = torch.autograd.grad(flow64, (a, b), gflow.double())
    (f0, g0), (f1, g1) = outs["0"], outs["1"]
    print(f"flow: engine {_rel(f1, flow64):.2e}, torch fp32 {_rel(f0, flow64):.2e} of max |flow| (vs float64)")
    assert _rel(f1, flow64) <= max(3 * _rel(f0, flow64), 1e-5)
    for what, e, v, truth in zip(("d/d frame 1", "d/d frame 2"), g1, g0, grads64):
        e_eng, e_t32 = _rel(e, truth), _rel(v, truth)
        print(f"{what}: engine {e_eng:.2e}, torch fp32 {e_t32:.2e} of max |gradient| (vs float64)")
        assert e_eng <= max(3 * e_t32, 5e-4), f"{what}: engine {e_eng:.2e} vs torch fp32 {e_t32:.2e}"
        beyond = lambda x: float(((x.double() - truth).abs() > 1e-4 * float(truth.abs().max())).float().mean())
        frac, frac_t = beyond(e), beyond(v)
        assert frac <= max(3 * frac_t, 1e-2), f"{what}: {frac:.2e} of the entries beyond 1e-4 (torch fp32: {frac_t:.2e})"


def test_window_prefix_chain_on_the_engine_equals_the_torch_prefix(scaled, monkeypatch):
    """flownetc_engine.py `window_prefix_forward` / `window_prefix_backward` with Robust FlowNetC's 12-layer chain (conv1_direct,
    eleven igemm launches and their data gradients, the skip tap's gradient added where stage 3's first data gradient lands)
    against torch autograd through `net.encode` (UFR_ENGINE=0) on the same 248 x 248 window stack, judged against float64."""
    from understanding_flow_robustness_amd.flownetc_engine import get_engine
    net = scaled
    B, H, W, wh, ww = 2, 384, 640, 248, 248
    g = torch.Generator().manual_seed(23)
    eng = get_engine(net, B, H, W, DEV)
    xw = torch.rand(2 * B, 3, wh, ww, generator=g).to(DEV)
    win = torch.zeros(B, 8, dtype=torch.int32, device=DEV)
    win[:, 1] = 64
    eng.window_prefix_forward(xw, win, 0, 0)
    P = eng._wprefix
    assert len(P["fwd"]) == 11 and len(P["bwd"]) == 12
    monkeypatch.setenv("UFR_ENGINE", "0")
    x32 = xw.clone().requires_grad_(True)
    c2, c3 = net.encode(x32)
    x64 = xw.double().requires_grad_(True)
    c2_64, c3_64 = _stem64(net, x64)
    for name, got, t32, t64 in (("stage 2", P["c2_nchw"], c2, c2_64), ("stage 3", P["c3_nchw"], c3, c3_64)):
        e_eng, e_t = _rel(got, t64), _rel(t32.detach(), t64)
        print(f"{name}: engine {e_eng:.2e}, torch fp32 {e_t:.2e} (vs float64)")
        assert e_eng <= max(3 * e_t, 2e-6), name
    gw2 = torch.randn(B, 128, wh // 4, ww // 4, generator=g).to(DEV)
    gw3 = torch.randn(2 * B, 256, wh // 8, ww // 8, generator=g).to(DEV)
    gw2_all = torch.cat((gw2, torch.zeros_like(gw2)), 0)
    gx = eng.window_prefix_backward(gw3, gw2)
    (gx32,) = torch.autograd.grad((c2, c3), x32, (gw2_all, gw3))
    (gx64,) = torch.autograd.grad((c2_64, c3_64), x64, (gw2_all.double(), gw3.double()))
    e_eng, e_t = _rel(gx, gx64), _rel(gx32, gx64)
    print(f"d/d window: engine {e_eng:.2e}, torch fp32 {e_t:.2e} (vs float64)")
    assert e_eng <= max(3 * e_t, 5e-4)
    beyond = lambda x: float(((x.double() - gx64).abs() > 1e-4 * float(gx64.abs().max())).float().mean())
    assert beyond(gx) <= max(3 * beyond(gx32), 1e-2), (beyond(gx), beyond(gx32))


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_attack_matches_reference_trace(net, monkeypatch, use_graph):
    """patch_attacks/main.py::attack on the reference's Robust FlowNetC, 2 iterations at 384 x 640 (make_golden_flex.py): the
    windowed step on the engines (248 x 248 window for the 25-px patch), cosine / L2 loss, unclamped lr and lr = 1000, a patch in
    the interior and one at the top edge."""
    from understanding_flow_robustness_amd._lib import engine_cache
    from understanding_flow_robustness_amd.patch_attack import attack
    monkeypatch.setenv("UFR_ENGINE", "1")
    z = load_golden("attack_flownetc_flex_k3r3_384x640")
    H, W, S = 384, 640, 25
    (tgt, ref, target), _ = _seeded(int(z["seed"]), (1, 3, H, W), (1, 3, H, W), (1, 2, H, W))
    for a, key in ((tgt, "tgt_sum"), (ref, "ref_sum"), (target, "target_sum")):
        assert abs(float(a.double().sum()) - float(z[key])) <= 1e-6 * abs(float(z[key])), "input generator drift"
    tgt, ref, target = tgt.to(DEV), ref.to(DEV), target.to(DEV)
    before = _fallbacks()
    for place in ("mid", "edge"):
        cy, cx = (int(v) for v in z[f"{place}_yx"])
        box = (slice(None), slice(None), slice(cy, cy + S), slice(cx, cx + S))
        patch0, mask = torch.zeros(1, 3, H, W, device=DEV), torch.zeros(1, 3, H, W, device=DEV)
        patch0[box], mask[box] = t(z[f"{place}_patch0"], DEV), t(z[f"{place}_mask"], DEV)
        mb = t(z[f"{place}_mask"])
        for name, l2 in (("cos", False), ("l2", True), ("cos_lr1000", False)):
            args = Namespace(flownet=ROBUST, l2=l2, alpha=0.0, lr=float(z[f"{place}_{name}_lr"]), max_count=2)
            patch = patch0.clone()
            a_t, _, a_r, _ = attack(net, tgt, None, ref, patch, mask, patch0, target, None, args=args, use_graph=use_graph)
            ref_patch = t(z[f"{place}_{name}_patch"])
            upd = float(((ref_patch - t(z[f"{place}_patch0"])) * mb).abs().max())
            err = float(((patch.cpu()[box] - ref_patch) * mb).abs().max())
            adv = max(float((a_t.cpu()[box] - t(z[f"{place}_{name}_adv_tgt"])).abs().max()),
                      float((a_r.cpu()[box] - t(z[f"{place}_{name}_adv_ref"])).abs().max()))
            print(f"{place} {name}: patch err {err:.3e} (update {upd:.3e}), adv image err {adv:.3e}")
            # (at the default lr = 1000 random-init gradients move the patch by ~5e-4 only: held relative to that update too)
            assert upd > (1e-4 if name == "cos_lr1000" else 1e-1), f"{place} {name}: degenerate update {upd:.3e}"
            assert err <= 1e-4 * max(upd, 1.0) and err <= 1e-2 * upd and adv <= 2e-4, \
                f"{place} {name}: patch err {err:.3e}, update {upd:.3e}, adv image err {adv:.3e}"
    steps = list(engine_cache(net, "_ufr_patch_steps").values())
    assert steps and all(s.cone is not None and s.win_hw == (248, 248) and s.eng is not None for s in steps)
    assert _fallbacks() == before


def _same_update(pf, pc, p0, sel, what):
    """test_cone_gpu.py's criterion for two implementations of the same 2-iteration attack: >= 95 % of the patch pixels agree to
    1e-4 of the update and every pixel to 5e-2 (a misplaced window or band is off by O(1))."""
    upd = float(((pf - p0) * sel).abs().max())
    err = ((pf - pc) * sel).abs()
    assert 1e-3 < upd < 1.9, f"{what}: test lr leaves the update degenerate ({upd})"
    off = float((err > 1e-4 * upd + 1e-6).sum()) / max(float((sel != 0).sum()), 1.0)
    assert off <= 0.05 and float(err.max()) <= 5e-2 * upd, \
        f"{what}: {off:.2%} of the patch pixels differ by more than 1e-4, worst {float(err.max()) / upd:.2e} of the update"
    return upd


@pytest.mark.parametrize("shared", [True, False], ids=["shared_patch", "per_sample"])
def test_windowed_step_equals_full_frame_step(net, monkeypatch, shared):
    """The windowed step (280 x 280 prefix window for a 51-px patch, column band, incremental head) against the full-frame step
    (UFR_CONE=0's form: native stem on the whole frame) at 384 x 1280, 4 pairs, corner / edge / interior placements."""
    from understanding_flow_robustness_amd.patch_attack import PatchAttackStep
    monkeypatch.setenv("UFR_ENGINE", "1")
    B, H, W, S = 4, 384, 1280, 51
    (tgt, ref, target), g = _seeded(13, (B, 3, H, W), (B, 3, H, W), (B, 2, H, W))
    tgt, ref, target = tgt.to(DEV), ref.to(DEV), target.to(DEV)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    circ = (((yy - 25) ** 2 + (xx - 25) ** 2) <= 25 ** 2).float()          # bounding box: the full 51 pixels
    origins = [(0, 0), (333, 1229), (0, 600), (170, 640)]
    if shared:
        mask = circ.expand(1, 3, S, S).contiguous().to(DEV)
        patch0 = torch.rand(1, 3, S, S, generator=g).to(DEV)
        sel = mask
    else:
        mask = torch.zeros(B, 3, H, W)
        for n, (y, x) in enumerate(origins):
            mask[n, :, y:y + S, x:x + S] = circ
        mask = mask.to(DEV)
        patch0 = torch.rand(B, 3, H, W, generator=g).to(DEV) * mask
        sel = mask

    def run(cone, lr, iters, graph):
        args = Namespace(flownet=ROBUST, l2=False, alpha=0.0, lr=lr, max_count=iters)
        kw = dict(patch_hw=(S, S)) if shared else dict(shared_patch=False)
        step = PatchAttackStep(net, args, B, H, W, device=DEV, use_cone=cone, use_graph=graph, **kw)
        step.load(tgt, ref, patch0, mask, patch0, target, **(dict(origins=origins) if shared else {}))
        step.run(iters)
        return step, step.patch.clone()
    _, p1 = run(False, 1.0, 1, False)
    lr = 0.5 / float(((p1 - patch0) * sel).abs().max())
    full, pf = run(False, lr, 2, False)
    win, pc = run(True, lr, 2, True)
    assert full.cone is None and win.cone is not None and win.win_hw == (280, 280)
    assert win.eng is not None and win.band is not None and win.band.width > 0
    _same_update(pf, pc, patch0, sel, "shared patch" if shared else "per-sample patches")
