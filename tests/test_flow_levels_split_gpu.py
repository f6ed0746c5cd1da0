"""GPU suite: predict_flow on the starved grids with its chunk slices spread over the grid (csrc/engine_small.hip
`flow_head_split_gemm` + `flow_head_split_finish`) against the two launches it replaces, ufr_flow_head_planes_forward_mfma and
ufr_flow_up_planes_forward.  The split form adds the same partial sums in the same order, so flow_k and the written chunk of the
concatenation are compared with torch.equal; the float32 entry ufr_flow_head_planes_forward (another rounding sequence) bounds
the error of both at the 1e-5 of tests/test_engine_gpu.py."""
from argparse import Namespace

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 2
# 6 x 20: level 6 of the headline's frame; 5 x 7 and 13 x 33: neither side a multiple of a tile (edge tiles, halo clamps, a partial
# m-tile of the flat pixel list); 12 x 40: level 5
GRIDS = [(6, 20), (5, 7), (13, 33), (12, 40)]
# 1024: 32 chunks; 1026: the 2-channel tail chunk, 33 chunks = 8 slices of 5 with a short and an empty one; 544: 17 chunks = slices of
# 3 with a short and two empty ones; 200: 7 chunks in two slices of 4 and 3; 70: 3 chunks, one slice
CHANNELS = [1024, 1026, 544, 200, 70]


def _L():
    from understanding_flow_robustness_amd import _lib as L
    return L


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("H,W", GRIDS)
@pytest.mark.parametrize("C", CHANNELS)
def test_split_forward_and_finish_equal_the_two_launches(C, H, W):
    from understanding_flow_robustness_amd import igemm as ig
    from understanding_flow_robustness_amd.flownetc_engine import _pack_flow_head, _pack_flow_head_mfma, pf_split_plan
    L = _L()
    lib, st = L.lib(), L.stream()
    g = torch.Generator().manual_seed(1000 * H + C)
    x = torch.randn(B, C, H, W, generator=g).to(DEV)
    w = (torch.randn(2, C, 3, 3, generator=g) * 0.1).to(DEV)
    b = torch.randn(2, generator=g).to(DEV)
    up_w = torch.randn(2, 2, 4, 4, generator=g).to(DEV)
    up_b = torch.randn(2, generator=g).to(DEV)
    chunks = ig.pad32(C) // 32
    pl = ig.Planes(B, H, W, chunks + 1, DEV).load_nchw(x, chunk0=1)
    wm = _pack_flow_head_mfma(w)
    slices, starved, floats = pf_split_plan(B, H, W, chunks)
    assert starved and floats == slices * B * H * W * 18
    assert slices == (8 if chunks >= 16 else 2 if chunks >= 4 else 1)

    def fine():
        t = ig.Planes(B, 2 * H, 2 * W, 3, DEV)
        t.t.fill_(0.25)                                     # the neighbouring chunks must stay as they are
        return t

    # today's two launches
    flow_old = torch.full((B, 2, H, W), float("nan"), device=DEV)
    L.check(lib.ufr_flow_head_planes_forward_mfma(L.ptr(pl.t), pl.plane_stride, 1, chunks, L.ptr(wm), chunks, L.ptr(b), L.ptr(flow_old),
                                                  B, H, W, st))
    up_old = fine()
    L.check(lib.ufr_flow_up_planes_forward(L.ptr(flow_old), L.ptr(up_w), L.ptr(up_b), L.ptr(up_old.t), up_old.plane_stride, 1, B, H, W, st))
    # the split form
    partials = torch.full((floats,), float("nan"), device=DEV)
    flow_new = torch.full((B, 2, H, W), float("nan"), device=DEV)
    up_new = fine()
    L.check(lib.ufr_flow_head_planes_forward_split(L.ptr(pl.t), pl.plane_stride, 1, chunks, L.ptr(wm), chunks, L.ptr(partials), floats,
                                                   slices, B, H, W, st))
    assert bool(torch.isfinite(partials).all())            # every (slice, pixel, n) is written, an empty slice as zeros
    L.check(lib.ufr_flow_head_split_finish(L.ptr(partials), floats, slices, L.ptr(b), L.ptr(flow_new), L.ptr(up_w), L.ptr(up_b),
                                           L.ptr(up_new.t), up_new.plane_stride, 1, B, H, W, st))
    assert torch.equal(flow_new, flow_old)
    assert torch.equal(up_new.t, up_old.t)
    # the sum alone (what `_pf_forward(k)` leaves when it is called on its own), and an upsampling without bias
    flow_only = torch.full((B, 2, H, W), float("nan"), device=DEV)
    L.check(lib.ufr_flow_head_split_finish(L.ptr(partials), floats, slices, L.ptr(b), L.ptr(flow_only), None, None, None, 0, 0, B, H, W, st))
    assert torch.equal(flow_only, flow_old)
    up_old2, up_new2 = fine(), fine()
    L.check(lib.ufr_flow_up_planes_forward(L.ptr(flow_old), L.ptr(up_w), None, L.ptr(up_old2.t), up_old2.plane_stride, 2, B, H, W, st))
    L.check(lib.ufr_flow_head_split_finish(L.ptr(partials), floats, slices, L.ptr(b), L.ptr(flow_only), L.ptr(up_w), None, L.ptr(up_new2.t),
                                           up_new2.plane_stride, 2, B, H, W, st))
    assert torch.equal(up_new2.t, up_old2.t)
    # the float32 entry: another rounding sequence, the bound of tests/test_engine_gpu.py
    flow_f32 = torch.empty(B, 2, H, W, device=DEV)
    L.check(lib.ufr_flow_head_planes_forward(L.ptr(pl.t), pl.plane_stride, 1, chunks, L.ptr(_pack_flow_head(w)), chunks, L.ptr(b),
                                             L.ptr(flow_f32), B, H, W, st))
    assert _rel(flow_new, flow_f32) <= 1e-5


def test_split_entries_refuse_what_would_move_the_bits_or_leave_a_buffer():
    from understanding_flow_robustness_amd import igemm as ig
    from understanding_flow_robustness_amd.flownetc_engine import pf_split_plan
    L = _L()
    lib, st = L.lib(), L.stream()
    H, W, chunks = 6, 20, 32
    pl = ig.Planes(B, H, W, chunks, DEV)
    slices, _, floats = pf_split_plan(B, H, W, chunks)
    buf = torch.zeros(floats, device=DEV)
    p = L.ptr(buf)
    assert lib.ufr_flow_head_planes_forward_split(L.ptr(pl.t), pl.plane_stride, 0, chunks, p, chunks, p, floats, slices // 2, B, H, W, st) == -1
    assert b"chunk slices asked" in lib.ufr_last_error()
    assert lib.ufr_flow_head_planes_forward_split(L.ptr(pl.t), pl.plane_stride, 0, chunks, p, chunks, p, floats - 1, slices, B, H, W, st) == -1
    assert b"partials buffer" in lib.ufr_last_error()
    assert lib.ufr_flow_head_planes_forward_split(L.ptr(pl.t), pl.plane_stride, 1, chunks, p, chunks, p, floats, slices, B, H, W, st) == -1
    assert b"leave the planes operand" in lib.ufr_last_error()
    assert lib.ufr_flow_head_split_finish(p, floats - 1, slices, p, p, None, None, None, 0, 0, B, H, W, st) == -1
    fine = ig.Planes(B, 2 * H, 2 * W, 2, DEV)
    assert lib.ufr_flow_head_split_finish(p, floats, slices, p, p, p, None, L.ptr(fine.t), fine.plane_stride, 2, B, H, W, st) == -1
    assert b"leaves the planes" in lib.ufr_last_error()


def test_engine_splits_the_starved_levels_and_keeps_the_others():
    """8 pairs at 384 x 768: level 4 (24 x 48) brings 8 * 6 * 2 = 96 four-row tiles and runs the split form, level 3 (48 x 96) brings
    288 and keeps the launch it had; either way `_pf_forward(k)` on its own leaves the flow of the unsplit launch."""
    from understanding_flow_robustness_amd.flownetc_engine import get_engine
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    L = _L()
    net = fetch_model(Namespace(flownet="FlowNetC"), synthetic_seed=0).to(DEV)
    eng = get_engine(net, 8, 384, 768, DEV)
    assert sorted(eng.pf_split) == [4, 5, 6]
    g = torch.Generator().manual_seed(3)
    for k in (4, 3):
        src, chunks = eng.pf_src[k]
        src.load_nchw(torch.randn(8, 32 * chunks, src.H, src.W, generator=g).to(DEV), 0)
        eng.flow[k].fill_(float("nan"))
        eng._pf_forward(k)
        want = torch.empty_like(eng.flow[k])
        L.check(L.lib().ufr_flow_head_planes_forward_mfma(L.ptr(src.t), src.plane_stride, 0, chunks, L.ptr(eng.pf_wm[k]), chunks,
                                                          L.ptr(eng.pf_b[k]), L.ptr(want), 8, src.H, src.W, L.stream()))
        assert torch.equal(eng.flow[k], want)
    assert eng.pf_ran[4] == "split" and eng.pf_ran[3] == "mfma" and eng._pf_pending is None
