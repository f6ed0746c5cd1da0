"""GPU suite: FlowNetC + the fused patch-attack step against the reference's golden vectors and the
CPU oracle (EPE / patch pixels within 1e-4 relative, BASELINE.json north_star)."""
from argparse import Namespace

import pytest
import torch

from closeness import assert_close
from conftest import load_golden, t
from test_flow_oracle_cpu import ATTACK_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 1e-4   # north_star tolerance for floating-point outputs


@pytest.fixture(scope="module")
def net():
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    return fetch_model(Namespace(flownet="FlowNetC"), synthetic_seed=0).to(DEV)


@pytest.fixture(scope="module")
def sd(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


@pytest.mark.parametrize("case", ["flownetc_fwd_64x128", "flownetc_fwd_128x192"])
def test_flownetc_forward_and_image_gradients_vs_reference(net, case):
    from understanding_flow_robustness_amd import losses
    z = load_golden(case)
    x1, x2 = t(z["x1"], DEV).requires_grad_(True), t(z["x2"], DEV).requires_grad_(True)
    flow = net(x1, x2)
    assert_close(flow, t(z["flow"]), rtol=REL, atol_scale=REL, what="flow")
    # EPE parity: end-point error between build and reference flow, relative to the flow magnitude
    epe = (flow.detach().cpu() - t(z["flow"])).pow(2).sum(1).sqrt().mean()
    mag = t(z["flow"]).pow(2).sum(1).sqrt().mean()
    assert float(epe) <= REL * float(mag), f"EPE {float(epe):.3e} vs |flow| {float(mag):.3e}"
    gt = t(z["target"], DEV)
    assert abs(losses.compute_epe(gt, flow.detach()) - losses.compute_epe(gt.cpu(), t(z["flow"]))) \
        <= REL * losses.compute_epe(gt.cpu(), t(z["flow"]))
    loss = (1 - torch.nn.functional.cosine_similarity(flow, gt)).mean()
    g1, g2 = torch.autograd.grad(loss, (x1, x2))
    assert abs(float(loss) - float(z["loss"])) < 1e-5
    assert_close(g1, t(z["g1"]), rtol=1e-3, atol_scale=2e-4, what="d loss / d frame 1")
    assert_close(g2, t(z["g2"]), rtol=1e-3, atol_scale=2e-4, what="d loss / d frame 2")


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("name,l2,lr", ATTACK_CASES)
def test_attack_matches_reference_trace(net, name, l2, lr, use_graph):
    """attack() of patch_attacks/main.py:523-613, 1 and 2 iterations, HIP-graph and eager forms."""
    from understanding_flow_robustness_amd.patch_attack import attack
    z = load_golden("attack_flownetc_64x128")
    for iters in (1, 2):
        args = Namespace(flownet="FlowNetC", l2=l2, alpha=0.0, lr=lr, max_count=iters)
        patch = t(z["patch0"], DEV).clone()
        a_t, none, a_r, out_patch = attack(net, t(z["tgt"], DEV), None, t(z["ref"], DEV), patch, t(z["mask"], DEV),
                                           t(z["patch0"], DEV), t(z["target"], DEV), None, args=args,
                                           use_graph=use_graph)
        assert none is None and out_patch is patch            # in-place contract (main.py:581)
        ref_patch = t(z[f"{name}_it{iters}_patch"])
        upd = (ref_patch - t(z["patch0"])).abs().max()
        err = (patch.cpu() - ref_patch).abs().max()
        assert float(err) <= REL * max(float(upd), 1.0), \
            f"{name} it{iters}: patch err {float(err):.3e}, update magnitude {float(upd):.3e}"
        assert_close(a_t[:, :, 20:45, 50:75], t(z[f"{name}_it{iters}_adv_tgt"]), rtol=REL, atol_scale=REL)
        assert_close(a_r[:, :, 20:45, 50:75], t(z[f"{name}_it{iters}_adv_ref"]), rtol=REL, atol_scale=REL)


def test_attack_fused_kernels_bit_exact_vs_torch(net):
    """paste / update / loss kernels against the reference's own torch expressions on identical
    inputs: elementwise stages are bit-exact, the loss scalar to fp32 summation order."""
    from understanding_flow_robustness_amd import _lib as L
    g = torch.Generator().manual_seed(3)
    B, H, W = 3, 24, 40
    tgt, ref = torch.rand(B, 3, H, W, generator=g).to(DEV), torch.rand(B, 3, H, W, generator=g).to(DEV)
    mask = (torch.rand(B, 3, H, W, generator=g) > 0.5).float().to(DEV)
    patch = (torch.rand(1, 3, H, W, generator=g) * 3 - 1).to(DEV)
    a_t, a_r = torch.empty_like(tgt), torch.empty_like(tgt)
    CHW = 3 * H * W
    L.check(L.lib().ufr_patch_paste(L.ptr(tgt), L.ptr(ref), L.ptr(patch), L.ptr(mask), L.ptr(a_t), L.ptr(a_r), B,
                                    CHW, 0, CHW, 0, 0.0, 1.0, L.stream()))
    assert torch.equal(a_t, torch.mul(1 - mask, tgt) + torch.mul(mask, patch))
    assert torch.equal(a_r, torch.mul(1 - mask, ref) + torch.mul(mask, patch))
    g_t, g_r = torch.randn(B, 3, H, W, generator=g).to(DEV) * 1e-3, torch.randn(B, 3, H, W, generator=g).to(DEV) * 1e-3
    # canvas form, per-sample patches: the reference's B=1 arithmetic sample by sample (main.py:575-600)
    pp = (torch.rand(B, 3, H, W, generator=g) * 3 - 1).to(DEV)
    p2 = pp.clone()
    L.check(L.lib().ufr_patch_update(L.ptr(tgt), L.ptr(ref), L.ptr(g_t), L.ptr(g_r), L.ptr(p2), L.ptr(mask), L.ptr(a_t),
                                     L.ptr(a_r), B, CHW, CHW, CHW, 500.0, 2.0, 0.0, 1.0, None, L.stream()))
    want = pp - torch.clamp(500.0 * (g_t + g_r), -2, 2)
    assert torch.equal(p2, want)
    assert torch.equal(a_t, torch.clamp(torch.mul(1 - mask, tgt) + torch.mul(mask, want), 0, 1))
    # one canvas patch behind several pairs is refused: that case lives in patch coordinates
    rc = L.lib().ufr_patch_update(L.ptr(tgt), L.ptr(ref), L.ptr(g_t), L.ptr(g_r), L.ptr(p2), L.ptr(mask), L.ptr(a_t),
                                  L.ptr(a_r), B, CHW, 0, CHW, 500.0, 2.0, 0.0, 1.0, None, L.stream())
    assert rc != 0
    # patch-coordinate family: crop + group sums, fixed-order apply, placed paste -- against torch expressions
    ph, pw = 7, 9
    B4 = 4
    tgt4, ref4 = torch.rand(B4, 3, H, W, generator=g).to(DEV), torch.rand(B4, 3, H, W, generator=g).to(DEV)
    g4t, g4r = torch.randn(B4, 3, H, W, generator=g).to(DEV) * 1e-3, torch.randn(B4, 3, H, W, generator=g).to(DEV) * 1e-3
    P = (torch.rand(1, 3, ph, pw, generator=g) * 3 - 1).to(DEV)
    Mp = (torch.rand(1, 3, ph, pw, generator=g) > 0.3).float().to(DEV)
    org = [(0, 0), (17, 31), (5, 12), (10, 3)]
    origins = torch.tensor(org, dtype=torch.int32, device=DEV)
    loss_local = torch.tensor([0.625], device=DEV)
    n = 3 * ph * pw
    for groups in (1, 2, 4):
        rows = torch.full((groups, n + 1), float("nan"), device=DEV)
        L.check(L.lib().ufr_patch_grad_crop(L.ptr(g4t), L.ptr(g4r), L.ptr(Mp), L.ptr(origins), None, L.ptr(loss_local),
                                            L.ptr(rows), B4, H, W, ph, pw, groups, L.stream()))
        per = B4 // groups
        for gi in range(groups):
            acc = torch.zeros(3, ph, pw, device=DEV)
            for b in range(gi * per, (gi + 1) * per):
                oy, ox = org[b]
                acc = acc + (g4t[b, :, oy:oy + ph, ox:ox + pw] + g4r[b, :, oy:oy + ph, ox:ox + pw])
            assert torch.equal(rows[gi, :n].view(3, ph, pw), acc * (Mp[0] != 0))
            assert float(rows[gi, n]) == (0.625 if gi == 0 else 0.0)
        P2, loss = P.clone(), torch.zeros(1, device=DEV)
        L.check(L.lib().ufr_patch_apply(L.ptr(rows), groups, L.ptr(P2), L.ptr(loss), ph, pw, 500.0, 2.0, None, L.stream()))
        G = torch.zeros(n, device=DEV)
        for gi in range(groups):
            G = G + rows[gi, :n]
        assert torch.equal(P2.view(-1), P.view(-1) - torch.clamp(500.0 * G, -2, 2)) and float(loss) == 0.625
    a4t, a4r, m4 = torch.empty_like(tgt4), torch.empty_like(tgt4), torch.empty_like(tgt4)
    L.check(L.lib().ufr_patch_paste_placed(L.ptr(tgt4), L.ptr(ref4), L.ptr(P), L.ptr(Mp), L.ptr(origins), None, L.ptr(a4t),
                                           L.ptr(a4r), L.ptr(m4), B4, H, W, ph, pw, 1, 0.0, 1.0, None, L.stream()))
    canvas_m, canvas_p = torch.zeros_like(tgt4), torch.zeros_like(tgt4)
    for b, (oy, ox) in enumerate(org):
        canvas_m[b, :, oy:oy + ph, ox:ox + pw] = Mp[0]
        canvas_p[b, :, oy:oy + ph, ox:ox + pw] = P[0]
    assert torch.equal(m4, canvas_m)
    assert torch.equal(a4t, torch.clamp(torch.mul(1 - canvas_m, tgt4) + torch.mul(canvas_m, canvas_p), 0, 1))
    assert torch.equal(a4r, torch.clamp(torch.mul(1 - canvas_m, ref4) + torch.mul(canvas_m, canvas_p), 0, 1))
    # the re-paste of a call's later iterations touches the patch rectangles only: after a full paste, a changed patch and the
    # rectangle paste must leave the very canvas a second full paste would write (clipped placements included)
    P3 = (torch.rand(1, 3, ph, pw, generator=g) * 3 - 1).to(DEV)
    for org_t in (origins, torch.tensor([(-3, -2), (H - 4, W - 5), (5, 12), (10, 3)], dtype=torch.int32, device=DEV)):
        full_t, full_r, rect_t, rect_r = (torch.empty_like(tgt4) for _ in range(4))
        for dst_t, dst_r, patch in ((rect_t, rect_r, P), (full_t, full_r, P3)):
            L.check(L.lib().ufr_patch_paste_placed(L.ptr(tgt4), L.ptr(ref4), L.ptr(patch), L.ptr(Mp), L.ptr(org_t), None, L.ptr(dst_t),
                                                   L.ptr(dst_r), None, B4, H, W, ph, pw, 1, 0.0, 1.0, None, L.stream()))
        L.check(L.lib().ufr_patch_paste_placed_rect(L.ptr(tgt4), L.ptr(ref4), L.ptr(P3), L.ptr(Mp), L.ptr(org_t), L.ptr(rect_t),
                                                    L.ptr(rect_r), B4, H, W, ph, pw, 1, 0.0, 1.0, None, L.stream()))
        assert torch.equal(rect_t, full_t) and torch.equal(rect_r, full_r)
    stopped = torch.tensor([1.0, 0, 0, 0], device=DEV)                          # a tripped gate makes it a no-op
    keep = rect_t.clone()
    L.check(L.lib().ufr_patch_paste_placed_rect(L.ptr(tgt4), L.ptr(ref4), L.ptr(P), L.ptr(Mp), L.ptr(origins), L.ptr(rect_t),
                                                L.ptr(rect_r), B4, H, W, ph, pw, 1, 0.0, 1.0, L.ptr(stopped), L.stream()))
    assert torch.equal(rect_t, keep)
    import numpy as np
    bad = np.array([[0, 0], [20, 31], [5, 12], [10, 3]], dtype=np.int32)       # 20 + 7 > 24: leaves the frame
    rc = L.lib().ufr_patch_paste_placed(L.ptr(tgt4), L.ptr(ref4), L.ptr(P), L.ptr(Mp), L.ptr(origins), bad.ctypes.data,
                                        L.ptr(a4t), L.ptr(a4r), None, B4, H, W, ph, pw, 1, 0.0, 1.0, None, L.stream())
    assert rc != 0
    # device-resident origins are not validated on the host: a placement that leaves the frame (or starts left of / above
    # it) is clipped by the paste, and the crop sums only the pixels inside the frame -- no out-of-bounds read
    off = [(-3, -2), (H - 4, W - 5), (5, 12), (10, 3)]
    origins_off = torch.tensor(off, dtype=torch.int32, device=DEV)
    rows = torch.full((1, n + 1), float("nan"), device=DEV)
    L.check(L.lib().ufr_patch_grad_crop(L.ptr(g4t), L.ptr(g4r), L.ptr(Mp), L.ptr(origins_off), None, L.ptr(loss_local),
                                        L.ptr(rows), B4, H, W, ph, pw, 1, L.stream()))
    acc = torch.zeros(3, ph, pw, device=DEV)
    for b, (oy, ox) in enumerate(off):
        for i in range(ph):
            for j in range(pw):
                if 0 <= oy + i < H and 0 <= ox + j < W:
                    acc[:, i, j] = acc[:, i, j] + (g4t[b, :, oy + i, ox + j] + g4r[b, :, oy + i, ox + j])
    assert torch.equal(rows[0, :n].view(3, ph, pw), acc * (Mp[0] != 0))
    flow, target = torch.randn(B, 2, H, W, generator=g).to(DEV), torch.randn(B, 2, H, W, generator=g).to(DEV)
    for kind in (0, 1):
        f = flow.clone().requires_grad_(True)
        if kind == 0:
            ref_loss = (1 - torch.nn.functional.cosine_similarity(f, target)).mean()
        else:
            ref_loss = (torch.sum((f - target) ** 2, dim=1) + 1e-8).sqrt().mean()
        (ref_g,) = torch.autograd.grad(ref_loss, f)
        gf, loss, ws = torch.empty_like(flow), torch.zeros(1, device=DEV), torch.empty(L.LOSS_PARTIALS, device=DEV)
        L.check(L.lib().ufr_flow_loss(L.ptr(flow), L.ptr(target), L.ptr(gf), L.ptr(loss), B, H * W, kind, 1.0,
                                      L.ptr(ws), L.stream()))
        assert abs(float(loss) - float(ref_loss)) < 1e-5
        again = torch.zeros(1, device=DEV)                    # fixed-order reduction: the scalar is bit-reproducible
        L.check(L.lib().ufr_flow_loss(L.ptr(flow), L.ptr(target), L.ptr(gf), L.ptr(again), B, H * W, kind, 1.0,
                                      L.ptr(ws), L.stream()))
        assert torch.equal(loss, again)
        assert_close(gf, ref_g, rtol=1e-4, atol_scale=1e-5, what=f"loss kind {kind} gradient")


@pytest.mark.parametrize("B,h,w", [(8, 96, 320), (2, 24, 40), (1, 7, 9), (3, 16, 33)])
def test_upsampled_flow_loss_equals_interpolate_then_loss(B, h, w):
    """csrc/attack.hip `ufr_flow2_upsampled_loss`: loss on interpolate(flow2 * 20, x4, bilinear, align_corners=False)
    (models/FlowNetC.py:193-197 + main.py:557-566) and its gradient with respect to flow2, against torch's interpolate +
    ufr_flow_loss + autograd -- the three passes over the full-size flow it replaces; ragged grids included."""
    from understanding_flow_robustness_amd import _lib as L
    g = torch.Generator().manual_seed(h * w)
    flow2 = torch.randn(B, 2, h, w, generator=g).to(DEV)
    target = torch.randn(B, 2, 4 * h, 4 * w, generator=g).to(DEV)
    for kind in (0, 1):
        f2 = flow2.clone().requires_grad_(True)
        up = torch.nn.functional.interpolate(f2 * 20.0, scale_factor=4, mode="bilinear", align_corners=False)
        gf, ref_loss, ws = torch.empty_like(up), torch.zeros(1, device=DEV), torch.empty(L.LOSS_PARTIALS, device=DEV)
        L.check(L.lib().ufr_flow_loss(L.ptr(up.detach().contiguous()), L.ptr(target), L.ptr(gf), L.ptr(ref_loss), B, 16 * h * w, kind,
                                      0.75, L.ptr(ws), L.stream()))
        (ref_g,) = torch.autograd.grad(up, f2, gf)
        got_g, loss = torch.full_like(flow2, float("nan")), torch.zeros(1, device=DEV)
        L.check(L.lib().ufr_flow2_upsampled_loss(L.ptr(flow2), 20.0, L.ptr(target), L.ptr(got_g), L.ptr(loss), B, h, w, kind, 0.75,
                                                 L.ptr(ws), L.stream()))
        assert abs(float(loss) - float(ref_loss)) <= 2e-6 * max(1.0, abs(float(ref_loss))), (kind, float(loss), float(ref_loss))
        assert_close(got_g, ref_g, rtol=1e-4, atol_scale=1e-4, what=f"upsampled loss kind {kind}: gradient of flow2")  # (sums of ~64 terms in another order: 3e-5 of the max seen)
        again = torch.zeros(1, device=DEV)
        L.check(L.lib().ufr_flow2_upsampled_loss(L.ptr(flow2), 20.0, L.ptr(target), L.ptr(got_g), L.ptr(again), B, h, w, kind, 0.75,
                                                 L.ptr(ws), L.stream()))
        assert torch.equal(loss, again)                       # fixed-order reduction
    if B * -(-h // 16) * -(-w // 16) <= L.LOSS_PARTIALS:
        return
    pytest.fail("unreachable: every parametrisation fits the partial sums")


@pytest.mark.parametrize("B,Cin,H,W", [(8, 1024, 6, 20), (2, 194, 24, 40), (3, 37, 7, 9), (1, 16, 1, 5), (1, 770, 24, 80)])
def test_two_channel_layers_vs_torch(B, Cin, H, W):
    """csrc/small_cout.hip: predict_flow (Conv2d(Cin,2,3,1,1)) and upsampled_flow (ConvTranspose2d(2,2,4,2,1))
    forward and data gradient against torch, channel-split and direct paths, ragged sizes, with / without bias."""
    from understanding_flow_robustness_amd.band_conv import flow_head, flow_upsample
    g = torch.Generator().manual_seed(Cin + H)
    conv = torch.nn.Conv2d(Cin, 2, 3, 1, 1).to(DEV)
    x = torch.randn(B, Cin, H, W, generator=g).to(DEV)
    xr = x.clone().requires_grad_(True)
    ref = conv(xr)
    gy = torch.randn(B, 2, H, W, generator=g).to(DEV)
    (g_ref,) = torch.autograd.grad(ref, xr, gy)
    for p in conv.parameters():
        p.requires_grad_(False)
    xo = x.clone().requires_grad_(True)
    out = flow_head(xo, conv)
    assert out.grad_fn is not None and type(out.grad_fn).__name__.startswith("_Conv3x3C2"), "fast path not taken"
    # both are fp32 sums over up to 9 x 1026 terms in different orders: judge them against a float64 evaluation (the
    # kernel may be no further from it than 3x MIOpen's own error, or 2e-6 of the largest value)
    x64 = x.double().requires_grad_(True)
    ref64 = torch.nn.functional.conv2d(x64, conv.weight.double(), conv.bias.double(), 1, 1)
    (g64,) = torch.autograd.grad(ref64, x64, gy.double())
    rel = lambda a, b: float((a.double() - b).abs().max()) / float(b.abs().max())
    assert rel(out, ref64.detach()) <= max(3 * rel(ref, ref64.detach()), 2e-6), (rel(out, ref64.detach()), rel(ref, ref64.detach()))
    (g_out,) = torch.autograd.grad(out, xo, gy)
    assert rel(g_out, g64) <= max(3 * rel(g_ref, g64), 2e-6), (rel(g_out, g64), rel(g_ref, g64))
    again = flow_head(x, conv)
    assert torch.equal(again, out.detach()), "channel-split reduction must be deterministic"
    for bias in (True, False):
        up = torch.nn.ConvTranspose2d(2, 2, 4, 2, 1, bias=bias).to(DEV)
        f = torch.randn(B, 2, H, W, generator=g).to(DEV)
        fr = f.clone().requires_grad_(True)
        r = up(fr)
        gu = torch.randn_like(r)
        (gr,) = torch.autograd.grad(r, fr, gu)
        for p in up.parameters():
            p.requires_grad_(False)
        fo = f.clone().requires_grad_(True)
        o = flow_upsample(fo, up)
        assert type(o.grad_fn).__name__.startswith("_Deconv4x4C2")
        assert_close(o, r, rtol=1e-5, atol_scale=1e-6, what="upsampled_flow forward")
        (go,) = torch.autograd.grad(o, fo, gu)
        assert_close(go, gr, rtol=1e-5, atol_scale=1e-6, what="upsampled_flow data gradient")


@pytest.mark.parametrize("shape", [(2, 5, 7, 12), (1, 3, 5, 7), (3, 64, 24, 40)])
def test_fused_conv_epilogue_bit_exact_vs_torch(shape):
    """csrc/bias_act.hip: LeakyReLU(x + bias) in place and its adjoint equal the torch pair bit for bit
    (vectorised and scalar paths), and `conv_leaky` equals the module pair on a block of FlowNetC."""
    from understanding_flow_robustness_amd import _lib as L
    from understanding_flow_robustness_amd.band_conv import conv_leaky
    g = torch.Generator().manual_seed(shape[1])
    x = torch.randn(*shape, generator=g).to(DEV)
    bias = torch.randn(shape[1], generator=g).to(DEV)
    want = torch.nn.functional.leaky_relu(x + bias.view(1, -1, 1, 1), 0.1)
    y = x.clone()
    L.check(L.lib().ufr_bias_leaky_forward(L.ptr(y), L.ptr(bias), shape[0], shape[1], shape[2] * shape[3], 0.1, L.stream()))
    assert torch.equal(y, want)
    gy = torch.randn(*shape, generator=g).to(DEV)
    gx = torch.empty_like(gy)
    L.check(L.lib().ufr_leaky_backward(L.ptr(y), L.ptr(gy), L.ptr(gx), gy.numel(), 0.1, L.stream()))
    assert torch.equal(gx, torch.ops.aten.leaky_relu_backward(gy, want, 0.1, True))
    for block in (torch.nn.Sequential(torch.nn.Conv2d(shape[1], 6, 3, 2, 1), torch.nn.LeakyReLU(0.1, inplace=True)),
                  torch.nn.Sequential(torch.nn.ConvTranspose2d(shape[1], 6, 4, 2, 1), torch.nn.LeakyReLU(0.1, inplace=True))):
        block = block.to(DEV)
        xin = x.clone().requires_grad_(True)
        ref = block(xin)                                        # parameters trainable: the plain modules run
        (g_ref,) = torch.autograd.grad(ref.sum() + (ref ** 2).sum(), xin)
        for p in block.parameters():
            p.requires_grad_(False)
        xin2 = x.clone().requires_grad_(True)
        out = conv_leaky(xin2, block)
        assert torch.equal(out, ref)
        (g_out,) = torch.autograd.grad(out.sum() + (out ** 2).sum(), xin2)
        assert torch.equal(g_out, g_ref)


def test_attack_gate_semantics(net):
    """`while loss_scalar > 0.1` + `count > max_count-1` on the device: once the loss of iteration k is
    <= 0.1 the later replays leave patch and frames untouched."""
    from understanding_flow_robustness_amd.patch_attack import PatchAttackStep
    args = Namespace(flownet="FlowNetC", l2=False, alpha=0.0, lr=1e3, max_count=4)
    step = PatchAttackStep(net, args, 1, 64, 128, device=DEV)
    g = torch.Generator().manual_seed(5)
    tgt, ref = torch.rand(1, 3, 64, 128, generator=g).to(DEV), torch.rand(1, 3, 64, 128, generator=g).to(DEV)
    mask = torch.zeros(1, 3, 64, 128, device=DEV)
    mask[:, :, 10:30, 10:30] = 1
    patch = torch.rand(1, 3, 64, 128, generator=g).to(DEV)
    with torch.no_grad():
        flow = net(tgt * (1 - mask) + mask * patch, ref * (1 - mask) + mask * patch)
    step.load(tgt, ref, patch, mask, patch, flow)          # target == current flow -> loss ~ 0 at once
    n, loss = step.run(4)
    assert n == 1 and loss <= 0.1
    after_one = step.patch.clone()
    step.enqueue(3)
    torch.cuda.synchronize()
    assert torch.equal(step.patch, after_one)
    step.load(tgt, ref, patch, mask, patch, -flow)         # opposite target: never converges in 3
    n, loss = step.run(3)
    assert n == 3 and loss > 0.1


def test_batched_shared_patch_vs_oracle(net, sd, oracle):
    """ONE patch in patch coordinates behind two pairs at different placements against the oracle's
    `patch_attack_placed`, through the drop-in attack() with `origins=`; with sum_groups the single-process step
    reproduces the sharded summation tree."""
    from oracle import flow_oracle as fo
    from understanding_flow_robustness_amd.patch_attack import PatchAttackStep, attack
    g = torch.Generator().manual_seed(17)
    tgt, ref = torch.rand(2, 3, 64, 128, generator=g), torch.rand(2, 3, 64, 128, generator=g)
    origins = [(10, 20), (30, 80)]
    mask_p = torch.ones(1, 3, 20, 20)
    mask_p[:, :, :3, :3] = 0                                  # part of the square is not shown
    patch0 = torch.rand(1, 3, 20, 20, generator=g)
    target = torch.randn(2, 2, 64, 128, generator=g)
    cpu_patch = patch0.clone()
    trace = []
    c_t, c_r, cpu_patch, n, _ = fo.patch_attack_placed(lambda a, b: fo.flownetc_forward(sd, a, b), tgt, ref, cpu_patch,
                                                       mask_p, origins, target, lr=1e5, max_count=2, trace=trace)
    args = Namespace(flownet="FlowNetC", l2=False, alpha=0.0, lr=1e5, max_count=2)
    gpu_patch = patch0.clone().to(DEV)
    a_t, _, a_r, _ = attack(net, tgt.to(DEV), None, ref.to(DEV), gpu_patch, mask_p.to(DEV), patch0.to(DEV),
                            target.to(DEV), None, args=args, origins=origins)
    upd = float((cpu_patch - patch0).abs().max())
    assert 1e-2 < upd
    assert float((gpu_patch.cpu() - cpu_patch).abs().max()) <= REL * max(upd, 1.0)
    assert_close(a_t, c_t, rtol=REL, atol_scale=REL)
    assert torch.equal(gpu_patch.cpu()[:, :, :3, :3], patch0[:, :, :3, :3])          # unseen pixels get no gradient
    # both pairs' gradients reach the same patch pixel
    G = trace[0]["G"]
    one = (trace[0]["g_tgt"][0:1, :, 10:30, 20:40] + trace[0]["g_ref"][0:1, :, 10:30, 20:40]) * (mask_p != 0)
    assert float((G - one).abs().max()) > 0.1 * float(G.abs().max())
    # the same with two summation groups (what two ranks with one pair each compute): bit-identical here, where a
    # group holds one pair
    step = PatchAttackStep(net, args, 2, 64, 128, device=DEV, patch_hw=(20, 20), sum_groups=2)
    step.load(tgt.to(DEV), ref.to(DEV), patch0.to(DEV), mask_p.to(DEV), patch0.to(DEV), target.to(DEV), origins=origins)
    step.run(2)
    assert float((step.patch.cpu() - cpu_patch).abs().max()) <= REL * max(upd, 1.0)
    with pytest.raises(ValueError, match="patch coordinates"):
        PatchAttackStep(net, args, 2, 64, 128, device=DEV)                            # canvas patch behind two pairs
    with pytest.raises(ValueError, match="leaves the frame"):
        step.load(tgt.to(DEV), ref.to(DEV), patch0.to(DEV), mask_p.to(DEV), patch0.to(DEV), target.to(DEV),
                  origins=[(10, 20), (50, 80)])


def _bench_placements(B, H, W, size=51):
    return [(100 + 5 * b, 600 - 30 * b) for b in range(B)]


def _disc(size=51, radius=23):
    yy, xx = torch.meshgrid(torch.arange(size), torch.arange(size), indexing="ij")
    c = size // 2
    return (((yy - c) ** 2 + (xx - c) ** 2) <= radius ** 2).float().expand(1, 3, size, size).contiguous()


def test_attack_full_size_properties(net):
    """BASELINE config C2 (384x1280, 8 pairs behind one 51x51 patch): size-independent properties -- pixels outside
    the placed masks are exactly clamp(frame), two identical runs agree (MIOpen's data-gradient kernels are not
    bit-reproducible, so to 1e-4 of the update), and the iteration count is the requested one."""
    from understanding_flow_robustness_amd.patch_attack import PatchAttackStep
    B, H, W = 8, 384, 1280
    args = Namespace(flownet="FlowNetC", l2=False, alpha=0.0, lr=1e3, max_count=2)
    step = PatchAttackStep(net, args, B, H, W, device=DEV, patch_hw=(51, 51))
    g = torch.Generator().manual_seed(0)
    tgt, ref = torch.rand(B, 3, H, W, generator=g).to(DEV), torch.rand(B, 3, H, W, generator=g).to(DEV)
    origins, mask_p = _bench_placements(B, H, W), _disc().to(DEV)
    patch = torch.rand(1, 3, 51, 51, generator=g).to(DEV)
    with torch.no_grad():
        target = -torch.cat([net(tgt[i:i + 1], ref[i:i + 1]) for i in range(B)])
    outs = []
    for _ in range(2):
        step.load(tgt, ref, patch, mask_p, patch, target, origins=origins)
        n, loss = step.run(2)
        assert n == 2 and loss == loss
        outs.append((step.patch.clone(), step.adv_tgt.detach().clone()))
    upd = float((outs[0][0] - patch).abs().max())
    assert float((outs[0][0] - outs[1][0]).abs().max()) <= 1e-4 * max(upd, 1.0)
    assert float((outs[0][1] - outs[1][1]).abs().max()) <= 1e-4
    outside = step.mask == 0
    assert torch.equal(outs[0][1][outside], tgt.clamp(0, 1)[outside])
    assert float((outs[0][0] - patch).abs().max()) > 0


# placements that exercise every clipping case of the windowed step: the four corners, two edges, and two pairs whose
# windows overlap each other's columns (the band's origin table is per pair)
EDGE_PLACEMENTS = [(0, 0), (333, 1229), (0, 1229), (333, 0), (170, 0), (0, 600), (150, 600), (160, 615)]


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("seed,case", [(2, "interior"), (5, "edges")])
def test_headline_configuration_vs_cpu_oracle(net, sd, oracle, seed, case):
    """The benchmark's own configuration -- 8 pairs at 384x1280 behind one 51x51 circular patch, windowed prefix,
    column band, incremental head forward, captured graphs, 2 iterations -- against the CPU oracle's
    `patch_attack_placed` (minutes of CPU work, once per case): patch pixels to 1e-4 relative.  Two seeds: the bench's interior
    placements, and placements at the frame's corners / edges with overlapping windows."""
    from oracle import flow_oracle as fo
    from understanding_flow_robustness_amd.patch_attack import PatchAttackStep
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B, H, W = 8, 384, 1280
    g = torch.Generator().manual_seed(seed)
    tgt, ref = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
    origins, mask_p = (_bench_placements(B, H, W) if case == "interior" else EDGE_PLACEMENTS), _disc()
    patch0 = torch.rand(1, 3, 51, 51, generator=g)
    predict = lambda a, b: fo.flownetc_forward(sd, a, b)
    with torch.no_grad():
        target = -torch.cat([predict(tgt[i:i + 1], ref[i:i + 1]) for i in range(B)])
    # lr: random-init gradients are tiny; pick the step whose first update peaks near 0.5 so the +-2 clamp (which
    # would hide gradient errors) stays inactive
    probe, trace = patch0.clone(), []
    fo.patch_attack_placed(predict, tgt, ref, probe, mask_p, origins, target, lr=1.0, max_count=1, trace=trace)
    lr = 0.5 / (0.5 * float(trace[0]["G"].abs().max()))
    cpu_patch = patch0.clone()
    fo.patch_attack_placed(predict, tgt, ref, cpu_patch, mask_p, origins, target, lr=lr, max_count=2)
    args = Namespace(flownet="FlowNetC", l2=False, alpha=0.0, lr=lr, max_count=2)
    step = PatchAttackStep(net, args, B, H, W, device=DEV, patch_hw=(51, 51))
    step.load(tgt.to(DEV), ref.to(DEV), patch0.to(DEV), mask_p.to(DEV), patch0.to(DEV), target.to(DEV), origins=origins)
    n, _ = step.run(2)
    assert n == 2 and step.cone is not None and step.band is not None and step.band.width > 0 and step.graph_next is not None
    upd = float((cpu_patch - patch0).abs().max())
    err = float((step.patch.cpu() - cpu_patch).abs().max())
    assert 0.3 < upd < 1.9
    assert err <= REL * max(upd, 1.0), f"headline configuration: patch err {err:.3e}, update {upd:.3e}"


@pytest.mark.parametrize("B,H,W,P,origins", [(1, 256, 256, 51, [(100, 90)]),                       # the reference's training crop size
                                              (3, 128, 448, 25, [(0, 0), (103, 423), (50, 200)]),  # three pairs, corners + interior
                                              (2, 320, 192, 33, [(280, 10), (7, 150)])])           # taller than wide
def test_attack_at_other_frame_sizes_vs_cpu_oracle(net, sd, oracle, B, H, W, P, origins):
    """The fused step at frame sizes other than the benchmark's (windowed prefix, band or no band as the width allows, conv1 from
    the raw frames, rectangle re-paste, window crop): two iterations behind one PxP patch against the CPU oracle's
    `patch_attack_placed`, 1e-4 of the update."""
    from oracle import flow_oracle as fo
    from understanding_flow_robustness_amd.patch_attack import PatchAttackStep
    torch.set_num_threads(min(16, torch.get_num_threads()))
    g = torch.Generator().manual_seed(H + W)
    tgt, ref = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
    yy, xx = torch.meshgrid(torch.arange(P), torch.arange(P), indexing="ij")
    mask_p = (((yy - P // 2) ** 2 + (xx - P // 2) ** 2) <= (P // 2 - 2) ** 2).float().expand(1, 3, P, P).contiguous()
    patch0 = torch.rand(1, 3, P, P, generator=g)
    predict = lambda a, b: fo.flownetc_forward(sd, a, b)
    with torch.no_grad():
        target = -torch.cat([predict(tgt[i:i + 1], ref[i:i + 1]) for i in range(B)])
    probe, trace = patch0.clone(), []
    fo.patch_attack_placed(predict, tgt, ref, probe, mask_p, origins, target, lr=1.0, max_count=1, trace=trace)
    lr = 0.5 / (0.5 * float(trace[0]["G"].abs().max()))
    cpu_patch = patch0.clone()
    fo.patch_attack_placed(predict, tgt, ref, cpu_patch, mask_p, origins, target, lr=lr, max_count=2)
    args = Namespace(flownet="FlowNetC", l2=False, alpha=0.0, lr=lr, max_count=2)
    step = PatchAttackStep(net, args, B, H, W, device=DEV, patch_hw=(P, P))
    step.load(tgt.to(DEV), ref.to(DEV), patch0.to(DEV), mask_p.to(DEV), patch0.to(DEV), target.to(DEV), origins=origins)
    n, _ = step.run(2)
    upd = float((cpu_patch - patch0).abs().max())
    err = float((step.patch.cpu() - cpu_patch).abs().max())
    print(f"{B} x {H}x{W}, patch {P}: cone {step.cone is not None}, window {step.win_hw}, update {upd:.3e}, step vs oracle {err / upd:.2e}")
    assert n == 2 and step.graph is not None and 0.2 < upd < 1.9
    assert err <= REL * max(upd, 1.0), f"{B} x {H}x{W}: patch err {err:.3e}, update {upd:.3e}"
