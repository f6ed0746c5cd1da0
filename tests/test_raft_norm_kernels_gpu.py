"""GPU suite: every entry point of csrc/raft_norm.hip called on its own through `_lib`, against the plain references of
tests/raft_kernel_refs.py (proved on the CPU by tests/test_raft_update_ref_cpu.py): the statistics against a float64 two-pass
mean and 1 / sqrt(var + eps) (one float32 ulp: they are rounded once from float64), the forward and the adjoint against float64 at
three times the error of F.instance_norm (and its autograd) in float32 on this device, the folded-BatchNorm forms (stats = NULL)
and the masked copy bit for bit.  Buffers are wider than the call needs and full of a sentinel; the last shape has more 8-channel
groups than one launch has threads, so the grid-stride loops of the unfused kernels run a second time."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import raft_kernel_refs as R
from raft_kernel_refs import DEV, F32, Gate, LAUNCH_THREADS, PlaneBuf, device_lib as _lib, device_rand as _rand

pytestmark = pytest.mark.gpu
SHAPES = [(2, 17, 23, 3), (1, 33, 37, 1), (2, 32, 64, 2), (2, 128, 160, 4)]
EPS = float(torch.tensor(1e-5, dtype=torch.float32))                    # the float the entry receives


def _input(g, n, H, W, chunks, hard_channels=False):
    """[chunks][n*HW][32]; hard_channels (the statistics test): a channel of mean 50 and deviation 0.01 (image 0, channel 0) and a
    constant one (last image, channel 1)."""
    HW = H * W
    x = torch.randn(chunks, n * HW, 32, generator=g) * 3 + 0.5
    if hard_channels:
        x[0, :HW, 0] = 50.0 + 0.01 * torch.randn(HW, generator=g)
        x[0, (n - 1) * HW:, 1] = 2.3
    return x.to(DEV)


def _workspace(lib, HW, n, chunks):
    return torch.empty(lib.ufr_cm_norm_workspace_doubles(HW, n, chunks), dtype=torch.float64, device=DEV)


def _ulps(got, want64):
    """Distance in float32 units in the last place between `got` and the float64 value rounded once."""
    w = want64.float()
    assert bool((torch.sign(got) == torch.sign(w)).all())
    return int((got.view(torch.int32).long() - w.view(torch.int32).long()).abs().max())


@pytest.mark.parametrize("n,H,W,chunks", SHAPES)
def test_norm_statistics_are_the_float64_two_pass_values_rounded_once(n, H, W, chunks):
    L, lib = _lib()
    HW, C = H * W, chunks * 32
    g = torch.Generator().manual_seed(HW + n)
    x = F32(_input(g, n, H, W, chunks, hard_channels=True))
    ws = _workspace(lib, HW, n, chunks)
    mean64, rstd64 = R.norm_stats(x.t.double(), n, EPS)
    sa, sb = F32(shape=(n, C, 2)), F32(shape=(n, C, 2))
    out = PlaneBuf(chunks + 1, n * HW, 0)
    L.check(lib.ufr_cm_norm_stats(x.ptr, sa.ptr, L.ptr(ws), HW, n, chunks, EPS, L.stream()), "stats")
    L.check(lib.ufr_cm_norm_stats_apply(x.ptr, sb.ptr, L.ptr(ws), EPS, None, 0, 0, out.ptr, out.stride, 0, HW, n, chunks, 0, 0, L.stream()), "stats + apply")
    for name, s in (("ufr_cm_norm_stats", sa), ("ufr_cm_norm_stats_apply", sb)):
        um, ur = _ulps(s.t[..., 0], mean64), _ulps(s.t[..., 1], rstd64)
        print(f"raft_update_kernel_errors norm statistics {n}x{H}x{W} chunks={chunks} {name}: mean {um} ulp, rstd {ur} ulp of the rounded float64 value")
        assert um <= 1 and ur <= 1 and s.guards_hold()
    assert abs(float(sa.t[0, 0, 0]) - 50.0) < 0.01 and 50.0 < float(sa.t[0, 0, 1]) < 200.0          # deviation 0.01: rstd ~ 1 / sqrt(1e-4 + 1e-5)
    assert _ulps(sa.t[n - 1, 1, 1:2], torch.tensor([1.0 / EPS ** 0.5], dtype=torch.float64, device=DEV)) <= 1, "variance 0 must give 1 / sqrt(eps)"
    assert float(sa.t[n - 1, 1, 0]) == float(torch.tensor(2.3, dtype=torch.float32))
    assert x.guards_hold() and out.rest_holds(chunks)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("relu1,relu2", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("n,H,W,chunks", SHAPES)
def test_norm_forward_against_float64_in_all_three_forms(n, H, W, chunks, relu1, relu2, with_res):
    L, lib = _lib()
    HW, M, C, rc0, oc0 = H * W, n * H * W, chunks * 32, 1, 2
    g = torch.Generator().manual_seed(HW + n + relu1 * 2 + relu2)
    xv = _input(g, n, H, W, chunks)
    x = F32(xv)
    resv = _rand(g, chunks, M, 32) if with_res else None
    res = PlaneBuf(rc0 + chunks + 1, M, rc0, resv) if with_res else None
    ws = _workspace(lib, HW, n, chunks)
    res_args = (res.ptr, res.stride, rc0) if with_res else (None, 0, 0)
    mean64, rstd64 = R.norm_stats(xv.double(), n, EPS)
    want64 = R.norm_forward(xv.double(), n, mean64, rstd64, resv.double() if with_res else None, relu1, relu2)
    v = F.instance_norm(R.from_cm(xv, n, H, W), eps=EPS)                # the float32 torch spelling on this device
    v = torch.relu(v) if relu1 else v
    v = v + R.from_cm(resv, n, H, W) if with_res else v
    want32 = R.to_cm(torch.relu(v) if relu2 else v)
    gate = Gate(f"norm forward {n}x{H}x{W} chunks={chunks} relu=({relu1},{relu2}) res={int(with_res)}")
    # fused: statistics finished inside the apply kernel
    stats_a, out_a = F32(shape=(n, C, 2)), PlaneBuf(oc0 + chunks + 1, M, oc0)
    L.check(lib.ufr_cm_norm_stats_apply(x.ptr, stats_a.ptr, L.ptr(ws), EPS, *res_args, out_a.ptr, out_a.stride, oc0, HW, n, chunks, relu1, relu2,
                                        L.stream()), "stats + apply")
    gate.add("ufr_cm_norm_stats_apply", out_a.values(chunks), want32, want64)
    # unfused: statistics, then the streaming apply kernel
    stats_b, out_b = F32(shape=(n, C, 2)), PlaneBuf(oc0 + chunks + 2, M, oc0)
    L.check(lib.ufr_cm_norm_stats(x.ptr, stats_b.ptr, L.ptr(ws), HW, n, chunks, EPS, L.stream()), "stats")
    L.check(lib.ufr_cm_norm_apply(x.ptr, stats_b.ptr, *res_args, out_b.ptr, out_b.stride, oc0, HW, n, chunks, relu1, relu2, L.stream()), "apply")
    gate.add("ufr_cm_norm_stats + ufr_cm_norm_apply", out_b.values(chunks), want32, want64)
    assert torch.equal(out_a.own(chunks), out_b.own(chunks)) and torch.equal(stats_a.t, stats_b.t)
    # stats = NULL (BatchNorm folded into the convolution): relu2(res + relu1(x)) is one float32 addition -- bit for bit
    out_c = PlaneBuf(oc0 + chunks + 1, M, oc0)
    L.check(lib.ufr_cm_norm_apply(x.ptr, None, *res_args, out_c.ptr, out_c.stride, oc0, HW, n, chunks, relu1, relu2, L.stream()), "apply (folded)")
    assert torch.equal(out_c.own(chunks), R.split3(R.norm_forward(xv, n, None, None, resv, relu1, relu2)))
    assert not relu2 or not bool((want64 < 0).any())
    for o in (out_a, out_b, out_c):
        assert o.rest_holds(chunks)
    assert x.guards_hold() and torch.equal(x.t, xv) and (res is None or (res.rest_holds(chunks) and torch.equal(res.own(chunks), R.split3(resv))))
    assert stats_a.guards_hold() and stats_b.guards_hold()
    gate.check()


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("relu1", [0, 1])
@pytest.mark.parametrize("n,H,W,chunks", SHAPES)
def test_norm_adjoint_against_float64_with_and_without_statistics(n, H, W, chunks, relu1, with_mask):
    """The ReLU masks come from the kernel's own float32 statistics and output plane (checked by the two tests above), so the sign of
    x - mean is the same on every side and no element is left out."""
    L, lib = _lib()
    HW, M, C, oc0, gc0 = H * W, n * H * W, chunks * 32, 2, 1
    g = torch.Generator().manual_seed(HW + n + relu1 * 2 + with_mask)
    xv = _input(g, n, H, W, chunks)
    x, resv, Gv = F32(xv), _rand(g, chunks, M, 32), _rand(g, chunks, M, 32)
    res, G = PlaneBuf(chunks, M, 0, resv), F32(Gv)
    ws = _workspace(lib, HW, n, chunks)
    stats, out = F32(shape=(n, C, 2)), PlaneBuf(oc0 + chunks + 1, M, oc0)
    L.check(lib.ufr_cm_norm_stats_apply(x.ptr, stats.ptr, L.ptr(ws), EPS, res.ptr, res.stride, 0, out.ptr, out.stride, oc0, HW, n, chunks, relu1,
                                        int(with_mask), L.stream()), "stats + apply")
    mean32, rstd32 = stats.t[..., 0].clone(), stats.t[..., 1].clone()
    plane0 = out.own(chunks)[0].float() if with_mask else None          # the adjoint reads plane 0 of the forward's output as its mask
    pos = (R.norm_xhat(xv, n, mean32, rstd32) > 0) if relu1 else None   # float32, the kernel's own two roundings
    mask_args = (out.ptr, oc0) if with_mask else (None, 0)
    # ---- the statistics form (fused second stage)
    sums, gz = F32(shape=(n, C, 2)), PlaneBuf(gc0 + chunks + 1, M, gc0)
    L.check(lib.ufr_cm_norm_backward(x.ptr, G.ptr, *mask_args, stats.ptr, sums.ptr, L.ptr(ws), gz.ptr, gz.stride, gc0, HW, n, chunks, relu1,
                                     L.stream()), "backward")
    gz64, s0_64, s1_64 = R.norm_backward(xv.double(), Gv.double(), n, mean32.double(), rstd32.double(), plane0, relu1, pos)
    # float32 torch spelling: F.instance_norm and its autograd on this device, the ReLUs as the same fixed masks
    xi = R.from_cm(xv, n, H, W).requires_grad_(True)
    y = F.instance_norm(xi, eps=EPS)
    y = y * R.from_cm(pos.float(), n, H, W) if relu1 else y
    y = y + R.from_cm(resv, n, H, W)
    y = y * R.from_cm((plane0 > 0).float(), n, H, W) if with_mask else y
    (gx32,) = torch.autograd.grad(y, xi, R.from_cm(Gv, n, H, W))
    _, s0_32, s1_32 = R.norm_backward(xv, Gv, n, mean32, rstd32, plane0, relu1, pos)
    gate = Gate(f"norm adjoint {n}x{H}x{W} chunks={chunks} relu1={relu1} mask={int(with_mask)}")
    gate.add("gz planes", gz.values(chunks), R.to_cm(gx32), gz64)
    gate.add("sums[0] = mean g", sums.t[..., 0], s0_32, s0_64)
    gate.add("sums[1] = mean g xhat", sums.t[..., 1], s1_32, s1_64)
    assert gz.rest_holds(chunks) and sums.guards_hold()
    # ---- stats = NULL (the unfused streaming kernel): G [mask > 0] [x > 0] -- bit for bit
    gz_f = PlaneBuf(gc0 + chunks + 2, M, gc0)
    L.check(lib.ufr_cm_norm_backward(x.ptr, G.ptr, *mask_args, None, None, None, gz_f.ptr, gz_f.stride, gc0, HW, n, chunks, relu1, L.stream()),
            "backward (folded)")
    want_f, _, _ = R.norm_backward(xv, Gv, n, None, None, plane0, relu1)
    assert torch.equal(gz_f.own(chunks), R.split3(want_f)) and gz_f.rest_holds(chunks)
    assert chunks * M * 4 > LAUNCH_THREADS or (n, H, W, chunks) != SHAPES[-1]
    assert torch.equal(x.t, xv) and torch.equal(G.t, Gv) and x.guards_hold() and G.guards_hold() and out.rest_holds(chunks) and stats.guards_hold()
    gate.check()


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("elems", [8 * 35, 8 * LAUNCH_THREADS + 8 * 1001])
def test_masked_copy_is_where_mask_plane0_positive(elems, in_place):
    L, lib = _lib()
    offset = 4096 + 8
    g = torch.Generator().manual_seed(elems % 9973)
    Gv = _rand(g, elems)
    maskv = torch.round(_rand(g, elems, scale=1.5))
    assert bool((maskv == 0).any()) and bool((maskv < 0).any()) and bool((maskv > 0).any())
    mask = torch.full((offset + elems + 64,), 7.0, dtype=torch.bfloat16, device=DEV)
    mask[offset:offset + elems] = maskv.to(torch.bfloat16)
    G = F32(Gv)
    out = G if in_place else F32(shape=(elems,))
    L.check(lib.ufr_cm_masked_copy(G.ptr, ctypes.c_void_p(mask.data_ptr()), offset, out.ptr, elems, L.stream()), "masked copy")
    assert torch.equal(out.t, torch.where(maskv > 0, Gv, torch.zeros_like(Gv)))
    assert out.guards_hold() and G.guards_hold() and (in_place or torch.equal(G.t, Gv))
