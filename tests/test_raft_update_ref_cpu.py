"""CPU suite: the plain references of tests/raft_kernel_refs.py (what the GPU tests of csrc/raft_update.hip and
csrc/raft_norm.hip compare the kernels with) are themselves right: against F.conv2d, the SepConvGRU half-step
(models/raft/update.py:49-71, restated as tests/test_gru_gpu.py restates it), F.instance_norm and torch.autograd, in float64;
the float32 slab pre-activation against the same additions spelled out one number at a time."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import raft_kernel_refs as R


def _close(a, b, tol=1e-12):
    scale = max(float(b.abs().max()), 1e-30)
    assert a.shape == b.shape and float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max()) / scale


@pytest.mark.parametrize("H,W", [(3, 5), (1, 9), (9, 11)])
def test_flow_patches_times_the_weight_matrix_is_convf1(H, W):
    g = torch.Generator().manual_seed(H * 16 + W)
    B = 2
    flow = torch.randn(B, 2, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(128, 2, 7, 7, generator=g, dtype=torch.float64)
    patches = R.flow_patches(flow)                                       # [4][M][32]
    assert patches.shape == (4, B * H * W, 32)
    rows = patches.permute(1, 0, 2).reshape(B * H * W, 128)
    assert bool((rows[:, 98:] == 0).all())
    want = F.conv2d(flow, w, padding=3).permute(0, 2, 3, 1).reshape(B * H * W, 128)
    _close(rows @ R.convf1_weight_as_matrix(w), want)
    # the stated channel order, one element at a time: k = tap * 2 + ch, tap = ky * 7 + kx
    for b, y, x, ky, kx, ch in ((0, 0, 0, 3, 3, 0), (1, H - 1, W - 1, 0, 6, 1), (0, H // 2, W // 2, 6, 0, 1), (1, 0, W - 1, 2, 4, 0)):
        yy, xx = y + ky - 3, x + kx - 3
        v = float(flow[b, ch, yy, xx]) if 0 <= yy < H and 0 <= xx < W else 0.0
        assert float(rows[(b * H + y) * W + x, (ky * 7 + kx) * 2 + ch]) == v


def test_layout_helpers_and_the_three_way_split_are_exact():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 64, 3, 5, generator=g)
    cm = R.to_cm(x)
    assert cm.shape == (2, 30, 32) and torch.equal(R.from_cm(cm, 2, 3, 5), x)
    assert float(cm[1, (1 * 3 + 2) * 5 + 4, 7]) == float(x[1, 32 + 7, 2, 4])
    v = torch.cat((torch.randn(4096, generator=g) * 100, torch.tensor([0.0, -0.0, 1e-30, 3.0e38, -7.0])))
    p = R.split3(v)
    assert p.dtype == torch.bfloat16 and torch.equal(R.merge3(p), v)
    from understanding_flow_robustness_amd import igemm as ig
    assert torch.equal(p.view(3, -1), ig._split3(v))


def _gru_setup(seed, B=2, H=4, W=6, Ch=32, Cx=32):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(B=B, H=H, W=W, Ch=Ch, h0=torch.tanh(r(B, Ch, H, W)), x=r(B, Cx, H, W), wzr=r(2 * Ch, Ch + Cx, 1, 5) * 0.2,
                bzr=r(2 * Ch), wq=r(Ch, Ch + Cx, 1, 5) * 0.2, bq=r(Ch), czr=r(B, 2 * Ch, H, W), cq=r(B, Ch, H, W), w=r(B, Ch, H, W))


def _half_step(h, s, czr, cq):
    """SepConvGRU's horizontal half-step with the stacked z | r convolution; czr / cq: the share of the pre-activations that is
    the same in every iteration (the context features')."""
    Ch, x = s["Ch"], s["x"]
    zr = torch.sigmoid(F.conv2d(torch.cat([h, x], 1), s["wzr"], s["bzr"], padding=(0, 2)) + czr)
    z, r = zr[:, :Ch], zr[:, Ch:]
    q = torch.tanh(F.conv2d(torch.cat([r * h, x], 1), s["wq"], s["bq"], padding=(0, 2)) + cq)
    return (1 - z) * h + z * q


def test_gru_forward_references_are_the_sepconvgru_half_step():
    s = _gru_setup(3)
    B, H, W, Ch = s["B"], s["H"], s["W"], s["Ch"]
    h = s["h0"]
    zr_pre = F.conv2d(torch.cat([h, s["x"]], 1), s["wzr"], s["bzr"], padding=(0, 2)) + s["czr"]
    zr, rh = R.gates_forward(R.to_cm(zr_pre), R.to_cm(h))
    assert zr.shape == (2 * Ch // 32, B * H * W, 32)
    _close(R.from_cm(zr, B, H, W), torch.sigmoid(zr_pre))
    _close(R.from_cm(rh, B, H, W), torch.sigmoid(zr_pre[:, Ch:]) * h)
    q_pre = F.conv2d(torch.cat([R.from_cm(rh, B, H, W), s["x"]], 1), s["wq"], s["bq"], padding=(0, 2)) + s["cq"]
    q, out = R.blend_forward(R.to_cm(q_pre), zr[:Ch // 32], R.to_cm(h))
    _close(R.from_cm(q, B, H, W), torch.tanh(q_pre))
    _close(R.from_cm(out, B, H, W), _half_step(h, s, s["czr"], s["cq"]))


def test_gru_adjoint_references_are_autograd_of_two_chained_half_steps():
    """Two chained half-steps with shared addends.  The hand-written chain -- blend adjoint, the candidate convolution's adjoint,
    gates adjoint (g_h picked up where the blend left it), the gate convolution's adjoint, with the running sums of g_q_pre and
    g_zr_pre carried from the second step into the first -- must give autograd's d/d h0 and, in the running sums, autograd's
    gradients of the shared addends."""
    s = _gru_setup(4)
    B, H, W, Ch = s["B"], s["H"], s["W"], s["Ch"]
    c = Ch // 32
    h0, czr, cq = (s[k].clone().requires_grad_(True) for k in ("h0", "czr", "cq"))
    h1 = _half_step(h0, s, czr, cq)
    h2 = _half_step(h1, s, czr, cq)
    want_h0, want_czr, want_cq = torch.autograd.grad((h2 * s["w"]).sum(), (h0, czr, cq))

    cm, nchw = R.to_cm, lambda t: R.from_cm(t, B, H, W)

    def conv_adjoint(inp, weight, g_out):
        inp = inp.detach().requires_grad_(True)
        (gi,) = torch.autograd.grad(F.conv2d(inp, weight, padding=(0, 2)), inp, g_out)
        return gi[:, :Ch]

    # forward of both steps through the references, keeping what the adjoint reads
    saved, h = [], s["h0"]
    for _ in range(2):
        zr_pre = F.conv2d(torch.cat([h, s["x"]], 1), s["wzr"], s["bzr"], padding=(0, 2)) + s["czr"]
        zr, rh = R.gates_forward(cm(zr_pre), cm(h))
        q_pre = F.conv2d(torch.cat([nchw(rh), s["x"]], 1), s["wq"], s["bq"], padding=(0, 2)) + s["cq"]
        q, out = R.blend_forward(cm(q_pre), zr[:c], cm(h))
        saved.append((h, zr, rh, q))
        h = nchw(out)
    _close(h, h2.detach())
    g = cm(s["w"])
    acc_gq, acc_gzr = torch.zeros(c, B * H * W, 32, dtype=torch.float64), torch.zeros(2 * c, B * H * W, 32, dtype=torch.float64)
    for hin, zr, rh, q in reversed(saved):
        gq, g_z, g_h, acc_gq = R.blend_backward(q, zr[:c], cm(hin), g, acc_gq)
        g_rh = cm(conv_adjoint(torch.cat([nchw(rh), s["x"]], 1), s["wq"], nchw(gq)))
        gzr, g_h, acc_gzr, left = R.gates_backward(zr, cm(hin), g_z, g_rh, g_h, acc_gzr, consume=True)
        assert not bool(left.any())
        g = g_h + cm(conv_adjoint(torch.cat([hin, s["x"]], 1), s["wzr"], nchw(gzr)))
    _close(nchw(g), want_h0, 1e-11)
    _close(nchw(acc_gq), want_cq, 1e-11)
    _close(nchw(acc_gzr), want_czr, 1e-11)
    # without the running sums and without consuming: nothing else changes, g_rh comes back as it went in
    hin, zr, rh, q = saved[1]
    a = R.blend_backward(q, zr[:c], cm(hin), cm(s["w"]), torch.ones_like(q))
    b = R.blend_backward(q, zr[:c], cm(hin), cm(s["w"]), None)
    assert b[3] is None and all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and torch.equal(a[3], 1 + a[0])
    g_rh = torch.randn(q.shape, dtype=torch.float64)
    out = R.gates_backward(zr, cm(hin), a[1], g_rh, a[2], None, consume=False)
    assert out[2] is None and out[3] is g_rh


@pytest.mark.parametrize("relu1", [0, 1])
@pytest.mark.parametrize("relu2", [0, 1])
@pytest.mark.parametrize("with_res", [False, True])
def test_norm_references_are_instance_norm_and_its_autograd(relu1, relu2, with_res):
    g = torch.Generator().manual_seed(relu1 * 4 + relu2 * 2 + with_res)
    n, C, H, W = 2, 64, 5, 7
    x = (torch.randn(n, C, H, W, generator=g, dtype=torch.float64) * 3 + 0.5).requires_grad_(True)
    res = torch.randn(n, C, H, W, generator=g, dtype=torch.float64) if with_res else None
    G = torch.randn(n, C, H, W, generator=g, dtype=torch.float64)
    v = F.instance_norm(x, eps=1e-5)
    v = torch.relu(v) if relu1 else v
    v = v + res if with_res else v
    want = torch.relu(v) if relu2 else v
    (want_gx,) = torch.autograd.grad(want, x, G)
    xc = R.to_cm(x.detach())
    mean, rstd = R.norm_stats(xc, n, 1e-5)
    assert mean.shape == rstd.shape == (n, C)
    _close(mean, x.detach().mean((2, 3)))
    _close(rstd, 1.0 / torch.sqrt(x.detach().var((2, 3), unbiased=False) + 1e-5))
    out = R.norm_forward(xc, n, mean, rstd, R.to_cm(res) if with_res else None, relu1, relu2)
    _close(R.from_cm(out, n, H, W), want.detach())
    gz, s0, s1 = R.norm_backward(xc, R.to_cm(G), n, mean, rstd, out if relu2 else None, relu1)
    _close(R.from_cm(gz, n, H, W), want_gx, 1e-11)
    assert s0.shape == s1.shape == (n, C)
    # the folded-BatchNorm form: no statistics, the ReLU masks alone
    xf = x.detach().clone().requires_grad_(True)
    v = torch.relu(xf) if relu1 else xf
    v = v + res if with_res else v
    wantf = torch.relu(v) if relu2 else v
    (want_gf,) = torch.autograd.grad(wantf, xf, G)
    outf = R.norm_forward(xc, n, None, None, R.to_cm(res) if with_res else None, relu1, relu2)
    assert torch.equal(R.from_cm(outf, n, H, W), wantf.detach())
    gf, none0, none1 = R.norm_backward(xc, R.to_cm(G), n, None, None, outf if relu2 else None, relu1)
    assert none0 is None and none1 is None and torch.equal(R.from_cm(gf, n, H, W), want_gf)


@pytest.mark.parametrize("S,with_addend", [(1, False), (3, True), (8, True), (13, False)])
def test_slab_preactivation_is_float32_additions_in_the_stated_order(S, with_addend):
    """zeros, + slab 0 .. + slab S-1, + addend, + bias: every step rounded to float32 (numpy scalars, one number at a time).  The
    values are spread over many binades so that another order, or a float64 sum rounded once, gives other bits."""
    g = torch.Generator().manual_seed(S)
    M, Npad, col0, nch = 5, 128, 32, 2
    slabs = torch.randn(S, M, Npad, generator=g) * torch.exp(torch.randn(S, M, Npad, generator=g) * 3)
    bias = torch.randn(Npad, generator=g)
    addend = torch.randn(nch, M, 32, generator=g) * 10 if with_addend else None
    got = R.slab_preact(slabs, bias, addend, col0, nch)
    assert got.dtype == torch.float32 and got.shape == (nch, M, 32)
    sl, bi = slabs.numpy(), bias.numpy()
    other = 0
    for ch in range(nch):
        for m in range(M):
            for j in range(32):
                col = col0 + ch * 32 + j
                v = np.float32(0.0)
                for s in range(S):
                    v = np.float32(v + sl[s, m, col])
                if with_addend:
                    v = np.float32(v + addend.numpy()[ch, m, j])
                v = np.float32(v + bi[col])
                assert got.numpy()[ch, m, j] == v
                once = np.float32(sl[:, m, col].astype(np.float64).sum() + (float(addend[ch, m, j]) if with_addend else 0.0) + float(bi[col]))
                other += int(once != v)
    assert S == 1 and not with_addend or other > 0, "the inputs do not tell the stated order from a sum rounded once"


def test_motion_finish_and_finalize_references():
    g = torch.Generator().manual_seed(6)
    B, H, W, S, N = 2, 3, 4, 3, 100
    M = B * H * W
    slabs, bias, flow = torch.randn(S, M, 128, generator=g), torch.randn(126, generator=g), torch.randn(B, 2, H, W, generator=g)
    for slope in (0.0, 0.1):
        v = R.motion_finish_slabs(slabs, bias, N, slope, flow).permute(1, 0, 2).reshape(M, 128)
        pre = (slabs[0] + slabs[1] + slabs[2])[:, :N] + bias[:N]
        assert torch.equal(v[:, :N], F.leaky_relu(pre, slope) if slope else torch.relu(pre))
        assert not bool(v[:, N:126].any()) and torch.equal(v[:, 126:], flow.permute(0, 2, 3, 1).reshape(M, 2))
        gsum, mask = torch.randn(M, 32, generator=g), torch.randn(M, 32, generator=g).round()
        want = gsum * torch.where(mask > 0, 1.0, slope)
        assert torch.equal(R.grad_finalize(gsum, mask, slope), want)
    c1, c0, d = torch.randn(7, generator=g), torch.randn(7, generator=g), torch.randn(7, generator=g)
    new, saved, fl = R.coords_step(c1, d, c0)
    assert torch.equal(new, c1 + d) and torch.equal(saved, new) and torch.equal(fl, (c1 + d) - c0)
    new, saved, fl = R.coords_step(c1, None, c0)
    assert torch.equal(new, c1) and torch.equal(saved, c1) and torch.equal(fl, c1 - c0)
