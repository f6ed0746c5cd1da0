"""GPU suite: the fused glue launches of the patch-coordinate attack step -- loading a call (ufr_attack_place +
ufr_attack_load_frames), the window features into the head's buffers (ufr_window_features_planes), the front and the tail of the
captured iteration (ufr_window_gather_pair, ufr_patch_grad_crop_packed, ufr_patch_apply_paste_rect) -- each against the
multi-launch sequence of older entry points it replaces, with torch.equal: nothing here is compared by tolerance."""
import ctypes as C
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W, S = 2, 128, 768, 20          # W: the narrowest multiple of 64 at which a 96-pixel window leaves room for a column band
F32 = dict(dtype=torch.float32, device=DEV)
UFR_EINVAL = -1                       # include/ufr_hip.h


@pytest.fixture(scope="module")
def net():
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    n = fetch_model(Namespace(flownet="FlowNetC"), synthetic_seed=0).to(DEV)
    for p in n.parameters():
        p.requires_grad_(False)
    return n


@pytest.fixture(scope="module")
def operands():
    g = torch.Generator().manual_seed(29)
    tgt, ref = torch.rand(B, 3, H, W, generator=g).to(DEV), torch.rand(B, 3, H, W, generator=g).to(DEV)
    target = torch.randn(B, 2, H, W, generator=g).to(DEV)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    disc = (((yy - 9.5) ** 2 + (xx - 9.5) ** 2) <= 10.0 ** 2).float().expand(1, 3, S, S).contiguous().to(DEV)
    patch0 = torch.rand(1, 3, S, S, generator=g).to(DEV)
    return tgt, ref, target, disc, patch0


def _L():
    from understanding_flow_robustness_amd import _lib as L
    return L


def _i32(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------------------------------------------------------- the old sequences
def old_load(step, tgt, ref, patch, mask_p, patch_init, origins):
    """What load() of a patch-coordinate step issued before: the copies, the un-clamped full-canvas paste that also writes the canvas
    masks, ufr_cone_window on those masks and the torch arithmetic of the band origins.  Returns the tensors by name."""
    L = _L()
    lib, st = L.lib(), L.stream()
    o = dict(tgt=tgt.clone(), ref=ref.clone(), patch=patch.clone(), mask_p=mask_p.clone(), patch_init=patch_init.clone(),
             patch_loaded=patch.clone(), origins=_i32(origins), state=torch.zeros(4, **F32),
             adv_tgt=torch.zeros_like(tgt), adv_ref=torch.zeros_like(tgt), mask=torch.zeros_like(tgt),
             win=torch.zeros(B, 8, dtype=torch.int32, device=DEV), band_win=torch.zeros(B, 8, dtype=torch.int32, device=DEV))
    L.check(lib.ufr_patch_paste_placed(L.ptr(o["tgt"]), L.ptr(o["ref"]), L.ptr(o["patch"]), L.ptr(o["mask_p"]), L.ptr(o["origins"]),
                                       None, L.ptr(o["adv_tgt"]), L.ptr(o["adv_ref"]), L.ptr(o["mask"]), B, H, W, S, S, 0, step.lo,
                                       step.hi, None, st), "placed paste")
    wh, ww = step.win_hw
    L.check(lib.ufr_cone_window(L.ptr(o["mask"]), B, 3 * H * W, 3, H, W, C.byref(step._chain), wh, ww, L.ptr(o["win"]),
                                L.ptr(o["state"][3:]), st), "cone window")
    from understanding_flow_robustness_amd.band_conv import corr_band_origin
    start = torch.div(o["win"][:, 1] - step._band_reach, 32, rounding_mode="floor") * 32
    o["band_win"][:, 1] = start.clamp(0, W - step.band.width)
    o["band_win"][:, 2] = corr_band_origin(o["win"][:, 1], step.band.corr_width, W)
    return o


def step_tensors(step):
    return dict(tgt=step.tgt, ref=step.ref, patch=step.patch, mask_p=step.mask_p, patch_init=step.patch_init,
                patch_loaded=step.patch_loaded, origins=step.origins, state=step.state, adv_tgt=step.adv_tgt.detach(),
                adv_ref=step.adv_ref.detach(), win=step.win, band_win=step.band.win)


@pytest.fixture(scope="module")
def loaded_step(net, operands):
    """One step of 2 pairs at 128 x 768 behind a 20 x 20 disc: a 96 x 96 window and a column band narrower than the frame."""
    from understanding_flow_robustness_amd.patch_attack import PatchAttackStep
    tgt, ref, target, disc, patch0 = operands
    args = Namespace(flownet="FlowNetC", l2=False, alpha=0.0, lr=1.0, max_count=2)
    step = PatchAttackStep(net, args, B, H, W, device=DEV, patch_hw=(S, S), use_graph=False)
    step.load(tgt, ref, patch0, disc, patch0, target, origins=[(3, 5), (60, 400)])
    assert step.cone is not None and step.win_hw == (96, 96) and step.eng is not None
    assert 0 < step.band.width < W and 0 < step.band.corr_width <= step.band.width
    return step


PLACEMENTS = {
    "corners": [(0, 0), (H - S, W - S)],
    "other corners": [(0, W - S), (H - S, 0)],
    "edge and interior": [(0, 300), (50, 400)],
    "windows overlap in columns": [(10, 300), (90, 320)],
}


# ---------------------------------------------------------------------------------------------------------------- 1. load
@pytest.mark.parametrize("name", list(PLACEMENTS))
@pytest.mark.parametrize("device_origins", [False, True])
def test_load_equals_the_old_sequence(loaded_step, operands, name, device_origins):
    step = loaded_step
    tgt, ref, target, disc, patch0 = operands
    origins = PLACEMENTS[name]
    patch_init = patch0 * 0.5
    step.load(tgt, ref, patch0, disc, patch_init, target, origins=_i32(origins) if device_origins else origins)
    old = old_load(step, tgt, ref, patch0, disc, patch_init, origins)
    new = step_tensors(step)
    for k in new:
        assert torch.equal(new[k], old[k]), f"{name}: {k} differs from the old load sequence"
    assert torch.equal(step.target, target) and step._first
    assert float(step.state[3]) == 0.0
    assert torch.equal(step.mask, old["mask"]), "the canvas masks read after the load"
    assert torch.equal(step.adv_tgt.detach(), old["adv_tgt"]), "reading the masks left the pasted frames alone"


def test_load_refuses_a_placement_outside_the_frame_before_any_launch(loaded_step, operands):
    L = _L()
    step = loaded_step
    tgt, ref, target, disc, patch0 = operands
    step.load(tgt, ref, patch0, disc, patch0, target, origins=[(3, 5), (60, 400)])
    before = {k: v.clone() for k, v in step_tensors(step).items()}
    for bad in ([(0, 0), (H - S + 1, 0)], [(-1, 0), (0, 0)], [(0, W - S + 1), (0, 0)]):
        with pytest.raises(ValueError):
            step.load(tgt * 0.5, ref, patch0 * 0.5, disc, patch0, target, origins=bad)
        host = np.ascontiguousarray(np.asarray(bad, dtype=np.int32))
        rc = L.lib().ufr_attack_place(L.ptr(patch0), L.ptr(disc), L.ptr(patch0), None, host.ctypes.data, L.ptr(step.patch),
                                      L.ptr(step.mask_p), L.ptr(step.patch_init), L.ptr(step.patch_loaded), L.ptr(step.origins),
                                      L.ptr(step.state), B, H, W, S, S, None, 0, 0, None, None, 0, 0, 0, 0, L.stream())
        assert rc == UFR_EINVAL and b"leaves the frame" in L.lib().ufr_last_error()
    torch.cuda.synchronize()
    for k, v in step_tensors(step).items():
        assert torch.equal(v, before[k]), f"{k} changed by a refused load"


def _place_both(step, mask_p, origins, wh, ww):
    """ufr_attack_place against paste (canvas masks) + ufr_cone_window + the band arithmetic, for a window of wh x ww."""
    L = _L()
    lib, st = L.lib(), L.stream()
    from understanding_flow_robustness_amd.band_conv import CORR_REACH, corr_band_origin
    bw, cw, reach = step.band.width, step.band.corr_width, step._band_reach
    od = _i32(origins)
    patch = torch.rand(1, 3, S, S, device=DEV)
    canvas, scratch = torch.zeros(B, 3, H, W, **F32), torch.zeros(2, B, 3, H, W, **F32)
    L.check(lib.ufr_patch_paste_placed(L.ptr(scratch[0]), L.ptr(scratch[0]), L.ptr(patch), L.ptr(mask_p), L.ptr(od), None,
                                       L.ptr(scratch[1]), L.ptr(scratch[1]), L.ptr(canvas), B, H, W, S, S, 0, 0.0, 1.0, None, st),
            "placed paste")
    win_o, band_o, state_o = (torch.zeros(B, 8, dtype=torch.int32, device=DEV), torch.zeros(B, 8, dtype=torch.int32, device=DEV),
                              torch.zeros(4, **F32))
    L.check(lib.ufr_cone_window(L.ptr(canvas), B, 3 * H * W, 3, H, W, C.byref(step._chain), wh, ww, L.ptr(win_o),
                                L.ptr(state_o[3:]), st), "cone window")
    band_o[:, 1] = (torch.div(win_o[:, 1] - reach, 32, rounding_mode="floor") * 32).clamp(0, W - bw)
    band_o[:, 2] = corr_band_origin(win_o[:, 1], cw, W)
    win_n, band_n, state_n = torch.zeros_like(win_o), torch.zeros_like(band_o), torch.full((4,), 7.0, **F32)
    dst = [torch.zeros(1, 3, S, S, **F32) for _ in range(4)]
    od_n = torch.zeros_like(od)
    L.check(lib.ufr_attack_place(L.ptr(patch), L.ptr(mask_p), L.ptr(patch), L.ptr(od), None, *[L.ptr(d) for d in dst], L.ptr(od_n),
                                 L.ptr(state_n), B, H, W, S, S, C.byref(step._chain), wh, ww, L.ptr(win_n), L.ptr(band_n), bw, reach,
                                 cw, CORR_REACH, st), "attack place")
    assert torch.equal(dst[0], patch) and torch.equal(dst[1], mask_p) and torch.equal(dst[3], patch) and torch.equal(od_n, od)
    assert torch.equal(win_n, win_o), (win_n.tolist(), win_o.tolist())
    assert torch.equal(band_n, band_o) and torch.equal(state_n, state_o)
    return win_n, state_n


def test_place_flags_a_mask_larger_than_the_window(loaded_step, operands):
    """A 20-pixel disc needs more than a 64 x 64 window: both pairs overflow, in the old sequence and in the placement launch."""
    _, state = _place_both(loaded_step, operands[3], [(10, 300), (90, 320)], 64, 64)
    assert float(state[3]) == 2.0
    _, state = _place_both(loaded_step, operands[3], [(10, 300), (90, 320)], 96, 96)
    assert float(state[3]) == 0.0


def test_place_with_an_empty_and_with_a_one_pixel_mask(loaded_step):
    win, state = _place_both(loaded_step, torch.zeros(1, 3, S, S, **F32), [(0, 0), (50, 400)], 96, 96)
    assert win[:, :4].abs().sum() == 0 and win[0, 5] == -1 and float(state[3]) == 0.0       # empty box
    one = torch.zeros(1, 3, S, S, **F32)
    one[0, 2, S - 1, 0] = 1.0                            # a single element, last channel only
    win, _ = _place_both(loaded_step, one, [(0, 0), (H - S, W - S)], 96, 96)
    assert win[1, 4:].tolist() == [H - 1, H - 1, W - S, W - S]


def test_place_clips_device_origins_that_leave_the_frame(loaded_step, operands):
    """Device-resident origins are not validated: the canvas shows the part of the mask inside the frame, and the box is that part's."""
    _place_both(loaded_step, operands[3], [(-7, -12), (H - 6, W - 9)], 96, 96)
    _place_both(loaded_step, operands[3], [(H + 5, 0), (40, W - 1)], 96, 96)


# ---------------------------------------------------------------------------------------------------------------- 2. window features
@pytest.mark.parametrize("wins", [[(0, 0), (8, 336)], [(32, 672), (16, 200)]])
def test_window_features_equal_the_six_launch_sequence(wins):
    """Origins at image edges (the rim is kept there) and interior ones (rim skipped), margins m2 = 3 != m3 = 2."""
    L = _L()
    from understanding_flow_robustness_amd import igemm as ig
    lib, st = L.lib(), L.stream()
    wh = ww = 96
    m2, m3 = 3, 2
    g = torch.Generator().manual_seed(5)
    win = torch.zeros(B, 8, dtype=torch.int32, device=DEV)
    win[:, :2] = _i32(wins)
    c2w, c3w = ig.Planes(2 * B, wh // 4, ww // 4, 4, DEV), ig.Planes(2 * B, wh // 8, ww // 8, 8, DEV)
    for p in (c2w, c3w):
        v = torch.randn(p.chunks * p.M * 32, generator=g)
        v[::7] = 0.0
        v[3::11] = -0.0
        p.t.copy_(ig._split3(v.to(DEV)).view(p.t.shape))

    def buffers():
        return (ig.Planes(B, H // 4, W // 4, 6, DEV), ig.Planes(B, H // 8, W // 8, 8, DEV), ig.Planes(B, H // 8, W // 8, 8, DEV),
                torch.zeros(2 * B, 256, H // 8, W // 8, **F32), torch.zeros(2 * B, 256, wh // 8, ww // 8, **F32))
    cat2, c3a, c3b, c3n, c3wn = buffers()
    c2wn = torch.zeros(2 * B, 128, wh // 4, ww // 4, **F32)
    c2w.to_nchw(128, 0, out=c2wn)
    c3w.to_nchw(256, 0, out=c3wn)
    L.check(lib.ufr_window_scatter_planes(L.ptr(c2wn), L.ptr(cat2.t), cat2.plane_stride, 0, L.ptr(win), B, B, 128, H // 4, W // 4,
                                          wh // 4, ww // 4, 4, m2, st), "old conv2")
    for k, dst in ((0, c3a), (1, c3b)):
        L.check(lib.ufr_window_scatter_planes(L.ptr(c3wn[k * B:]), L.ptr(dst.t), dst.plane_stride, 0, L.ptr(win), B, B, 256, H // 8,
                                              W // 8, wh // 8, ww // 8, 8, m3, st), "old conv3")
    L.check(lib.ufr_window_scatter(L.ptr(c3wn), L.ptr(c3n), L.ptr(win), B, 2 * B, 256, H // 8, W // 8, wh // 8, ww // 8, 8, m3, st),
            "old conv3 nchw")
    cat2_n, c3a_n, c3b_n, c3n_n, c3wn_n = buffers()
    L.check(lib.ufr_window_features_planes(L.ptr(c2w.t), c2w.plane_stride, L.ptr(c3w.t), c3w.plane_stride, L.ptr(cat2_n.t),
                                           cat2_n.plane_stride, L.ptr(c3a_n.t), c3a_n.plane_stride, L.ptr(c3b_n.t),
                                           c3b_n.plane_stride, L.ptr(c3n_n), L.ptr(c3wn_n), L.ptr(win), B, H, W, wh, ww, m2, m3, st),
            "window features")
    # bit patterns, not values: a plane entry of -0 must not pass for +0
    bits = lambda t: t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)
    for name, a, b in (("cat2", cat2_n.t, cat2.t), ("c3a_p", c3a_n.t, c3a.t), ("c3b_p", c3b_n.t, c3b.t), ("c3_nchw", c3n_n, c3n),
                       ("window c3_nchw", c3wn_n, c3wn)):
        assert torch.equal(bits(a), bits(b)), f"{name} differs from the six-launch sequence"
    assert float(c3n.abs().sum()) > 0 and float(cat2.t.float().abs().sum()) > 0
    # refused before the launch: a window that does not fit, planes too small for the images
    bad = lib.ufr_window_features_planes(L.ptr(c2w.t), c2w.plane_stride, L.ptr(c3w.t), c3w.plane_stride, L.ptr(cat2_n.t),
                                         cat2_n.plane_stride, L.ptr(c3a_n.t), c3a_n.plane_stride // 2, L.ptr(c3b_n.t),
                                         c3b_n.plane_stride, L.ptr(c3n_n), L.ptr(c3wn_n), L.ptr(win), B, H, W, wh, ww, m2, m3, st)
    assert bad == UFR_EINVAL


# ---------------------------------------------------------------------------------------------------------------- 3. front and tail
def test_window_gather_pair_equals_two_gathers_and_a_fill(operands):
    L = _L()
    lib, st = L.lib(), L.stream()
    tgt, ref = operands[0], operands[1]
    wh = ww = 96
    win = torch.zeros(B, 8, dtype=torch.int32, device=DEV)
    win[:, :2] = _i32([(32, 672), (8, 336)])
    old = torch.zeros(2 * B, 3, wh, ww, **F32)
    for src, dst in ((tgt, old), (ref, old[B:])):
        L.check(lib.ufr_window_gather(L.ptr(src), L.ptr(dst), L.ptr(win), B, B, 3, H, W, wh, ww, 1, 0, st), "gather")
    new, loss = torch.zeros_like(old), torch.full((1,), 3.0, **F32)
    L.check(lib.ufr_window_gather_pair(L.ptr(tgt), L.ptr(ref), L.ptr(new), L.ptr(win), L.ptr(loss), B, 3, H, W, wh, ww, st), "pair")
    assert torch.equal(new, old) and float(loss) == 0.0


@pytest.mark.parametrize("stopped,do_clamp", [(0, 1), (1, 1), (0, 0)])
def test_fused_tail_equals_unpack_crop_apply_rect_paste(operands, stopped, do_clamp):
    L = _L()
    lib, st = L.lib(), L.stream()
    tgt, ref, _, disc, patch0 = operands
    wh = ww = 96
    n = 3 * S * S
    g = torch.Generator().manual_seed(41)
    G = torch.randn(1, 2 * B * (wh // 2 + 3) * (ww // 2 + 2), 32, generator=g).to(DEV)
    win = torch.zeros(B, 8, dtype=torch.int32, device=DEV)
    win[:, :2] = _i32([(32, 672), (8, 336)])
    origins = _i32([(H - S, W - S - 3), (40, 420)])          # the second pair's patch is cut by its window's right edge: x0 + ww = 432
    loss_local = torch.full((1,), 0.625, **F32)
    state = torch.tensor([float(stopped), 1.0, 0.5, 0.0], **F32)
    step, bound = 0.75, 2.0                                  # gradients of order 1: some steps reach the +-2 clamp, most do not

    def fresh():
        return dict(patch=patch0.clone() * 1.5 - 0.2, rows=torch.full((2, n + 1), 9.0, **F32), loss=torch.full((1,), 9.0, **F32),
                    adv_tgt=tgt.clone(), adv_ref=ref.clone())
    o, f = fresh(), fresh()
    gxw = torch.zeros(2 * B, 3, wh, ww, **F32)
    L.check(lib.ufr_conv1_unpack_grad(L.ptr(G), L.ptr(gxw), 2 * B, wh, ww, st), "unpack")
    L.check(lib.ufr_patch_grad_crop_window(L.ptr(gxw), L.ptr(win), L.ptr(disc), L.ptr(origins), L.ptr(loss_local), L.ptr(o["rows"]), B,
                                           H, W, wh, ww, S, S, 2, st), "crop")
    L.check(lib.ufr_patch_apply(L.ptr(o["rows"]), 2, L.ptr(o["patch"]), L.ptr(o["loss"]), S, S, step, bound, L.ptr(state), st), "apply")
    L.check(lib.ufr_patch_paste_placed_rect(L.ptr(tgt), L.ptr(ref), L.ptr(o["patch"]), L.ptr(disc), L.ptr(origins), L.ptr(o["adv_tgt"]),
                                            L.ptr(o["adv_ref"]), B, H, W, S, S, do_clamp, 0.0, 1.0, L.ptr(state), st), "rect paste")
    L.check(lib.ufr_patch_grad_crop_packed(L.ptr(G), L.ptr(win), L.ptr(disc), L.ptr(origins), L.ptr(loss_local), L.ptr(f["rows"]), B,
                                           H, W, wh, ww, S, S, 2, st), "crop (packed)")
    L.check(lib.ufr_patch_apply_paste_rect(L.ptr(f["rows"]), 2, L.ptr(f["patch"]), L.ptr(f["loss"]), L.ptr(tgt), L.ptr(ref), L.ptr(disc),
                                           L.ptr(origins), L.ptr(f["adv_tgt"]), L.ptr(f["adv_ref"]), B, H, W, S, S, step, bound,
                                           do_clamp, 0.0, 1.0, L.ptr(state), st), "apply + rect paste")
    for k in o:
        assert torch.equal(f[k], o[k]), f"{k} differs from the unfused tail"
    assert float(loss_local) == 0.625 and float(o["loss"]) == 0.625
    moved = not torch.equal(o["patch"], patch0 * 1.5 - 0.2)
    assert moved == (not stopped) and (stopped or not torch.equal(o["adv_tgt"], tgt))
    assert float(o["rows"][1, :n].abs().sum()) > 0 and float(o["rows"][0, :n].abs().sum()) > 0


# ---------------------------------------------------------------------------------------------------------------- 4. whole step
def _old_path_step_class():
    from understanding_flow_robustness_amd.patch_attack import CLAMP_BOUND, PatchAttackStep
    L = _L()

    class OldPathStep(PatchAttackStep):
        """The same step driven through the older entry points, launch by launch: load() and the iteration as they were issued
        before the fused glue launches (FlowNetC engine, fused loss, one rank)."""

        def _load_placed(self, tgt, ref, patch, mask, patch_init, target, prefix_features, origins):
            with torch.no_grad():
                self.tgt.copy_(tgt); self.ref.copy_(ref)
                oh = np.ascontiguousarray(np.asarray(origins.cpu() if torch.is_tensor(origins) else origins, dtype=np.int32))
                self.origins_host = oh.reshape(self.B, 2)
                self.origins.copy_(torch.from_numpy(self.origins_host))
                self.mask_p.copy_(mask.reshape(self.mask_p.shape))
                self.patch.copy_(patch.reshape(self.patch.shape))
                self.patch_init.copy_(patch_init.reshape(self.patch.shape))
                self.target.copy_(target)
                self.state.zero_()
                L.check(L.lib().ufr_patch_paste_placed(
                    L.ptr(self.tgt), L.ptr(self.ref), L.ptr(self.patch), L.ptr(self.mask_p), L.ptr(self.origins), None,
                    L.ptr(self.adv_tgt), L.ptr(self.adv_ref), L.ptr(self._canvas()), self.B, self.H, self.W, self.ph, self.pw, 0,
                    self.lo, self.hi, None, L.stream()), "placed paste")
                self._mask_stale = False
                self._first = True
                self.patch_loaded.copy_(self.patch)
                if self.win_hw is None:
                    self._setup_cone()
                self._cone_refresh(prefix_features)        # ufr_cone_window on the canvas masks + the torch band arithmetic

        def _canvas(self):
            if self._mask_canvas is None:
                self._mask_canvas = torch.zeros_like(self.tgt)
            return self._mask_canvas

        def _part_a(self):
            lib, Bn, Hn, Wn, eng = L.lib(), self.B, self.H, self.W, self.eng
            assert self.eng_kind == "flownetc" and self._fused_loss and self.world == 1 and self.alpha == 0.0
            self.loss_local.zero_()
            self._win_copy(lib.ufr_window_gather, self.adv_tgt, self.xw, Bn, 3, Hn, Wn, 1, 0)
            self._win_copy(lib.ufr_window_gather, self.adv_ref, self.xw[Bn:], Bn, 3, Hn, Wn, 1, 0)
            (ls2, m2, _, _, gw2), (ls3, m3, _, _, gw3) = self.taps
            wh, ww = self.win_hw
            P = eng.window_prefix(wh, ww)
            eng._conv1(P, self.xw.detach(), None)
            for _, launch, _ in P["fwd"]:
                launch()
            P["c2"].to_nchw(128, 0, out=P["c2_nchw"])
            P["c3"].to_nchw(256, 0, out=P["c3_nchw"])
            eng.scatter_window_features(P["c2_nchw"], P["c3_nchw"], self.win, wh, ww, m2, m3)
            eng.forward_cached(self.band)
            L.check(lib.ufr_flow2_upsampled_loss(L.ptr(eng.flow_out), float(eng.flow_scale), L.ptr(self.target), L.ptr(self.g_flow2),
                                                 L.ptr(self.loss_local), Bn, Hn // 4, Wn // 4, self.kind, 1.0 - self.alpha,
                                                 L.ptr(self.loss_ws), L.stream()), "upsampled flow loss")
            self.band.g3_window, self.band.g3_margin = gw3, m3
            self.band.eng_window, self.band.g2_margin = True, m2
            g2a, g3a, g3b = eng.backward(self.g_flow2.contiguous(), self.band, skip_unread=self.skip_unread)
            if g2a is not None:
                self._win_copy(lib.ufr_window_gather, g2a, gw2, Bn, 128, Hn // ls2, Wn // ls2, ls2, m2)
            if g3a is not None:
                self._win_copy(lib.ufr_window_gather, g3a, gw3, Bn, 256, Hn // ls3, Wn // ls3, ls3, m3)
                self._win_copy(lib.ufr_window_gather, g3b, gw3[Bn:], Bn, 256, Hn // ls3, Wn // ls3, ls3, m3)
            gxw = eng.window_prefix_backward(gw3, None if g2a is None else gw2)            # ends in ufr_conv1_unpack_grad
            L.check(lib.ufr_patch_grad_crop_window(L.ptr(gxw), L.ptr(self.win), L.ptr(self.mask_p), L.ptr(self.origins),
                                                   L.ptr(self.loss_local), L.ptr(self.rows_local), Bn, Hn, Wn, wh, ww, self.ph, self.pw,
                                                   self.groups, L.stream()), "crop")
            L.check(lib.ufr_patch_apply(L.ptr(self.rows_all), self.rows_all.shape[0], L.ptr(self.patch), L.ptr(self.loss_cur), self.ph,
                                        self.pw, self.step, CLAMP_BOUND, L.ptr(self.state), L.stream()), "apply")
            self._paste(do_clamp=True, gate=True)          # ufr_patch_paste_placed, or _rect in the later-iteration form
            self._gate()

    return OldPathStep


def test_whole_step_equals_the_step_driven_through_the_old_entry_points(net, operands):
    """2 pairs, 2 iterations, graphs on: this tree's step against the same step issued launch by launch through the entry points it
    had before.  Patch, pasted frames and loss must be equal, call after call."""
    from understanding_flow_robustness_amd.patch_attack import PatchAttackStep
    tgt, ref, target, disc, patch0 = operands
    probe_args = Namespace(flownet="FlowNetC", l2=False, alpha=0.0, lr=1.0, max_count=2)
    probe = _old_path_step_class()(net, probe_args, B, H, W, device=DEV, patch_hw=(S, S), use_graph=False)
    probe.load(tgt, ref, patch0, disc, patch0, target, origins=PLACEMENTS["edge and interior"])
    probe.run(1)
    lr = 0.25 / float(((probe.patch - patch0) * disc).abs().max())       # updates of a quarter: visible, unclamped
    args = Namespace(flownet="FlowNetC", l2=False, alpha=0.0, lr=lr, max_count=2)
    new = PatchAttackStep(net, args, B, H, W, device=DEV, patch_hw=(S, S), use_graph=True, sum_groups=2)
    old = _old_path_step_class()(net, args, B, H, W, device=DEV, patch_hw=(S, S), use_graph=True, sum_groups=2)
    for name in ("edge and interior", "corners", "windows overlap in columns"):
        outs = []
        for step in (new, old):
            step.load(tgt, ref, patch0, disc, patch0, target, origins=PLACEMENTS[name])
            n, loss = step.run(2)
            outs.append((step.patch.clone(), step.adv_tgt.detach().clone(), step.adv_ref.detach().clone(), n, loss,
                         step.rows_local.clone()))
        assert new.graph_next is not None and new.graph_next is not new.graph and new.eng is not None
        (pn, an, rn, nn, ln, wn), (po, ao, ro, no, lo, wo) = outs
        assert nn == no == 2 and ln == lo, (name, nn, no, ln, lo)
        assert torch.equal(wn, wo), f"{name}: gradient rows"
        assert torch.equal(pn, po) and torch.equal(an, ao) and torch.equal(rn, ro), name
        assert float(((pn - patch0) * disc).abs().max()) > 0.1
