"""GPU suite for the windowed encoder of the patch attack (csrc/window.hip, cone.py, patch_attack.py):
device-side window placement against the host arithmetic, gather/scatter against tensor slicing, the
windowed attack step against the reference's trace (golden) and against the full-frame step at the
benchmark size."""
import ctypes as C
from argparse import Namespace

import pytest
import torch

from closeness import assert_close
from conftest import load_golden, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 1e-4


@pytest.fixture(scope="module")
def net():
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    return fetch_model(Namespace(flownet="FlowNetC"), synthetic_seed=0).to(DEV)


def _spec():
    from understanding_flow_robustness_amd.flownets.flownetc import FlowNetC
    return FlowNetC.CONE


def test_cone_window_kernel_matches_host_arithmetic():
    from understanding_flow_robustness_amd import _lib as L
    spec, H, W = _spec(), 192, 320
    boxes = [(0, 24, 0, 24), (0, 9, 290, 319), (170, 191, 0, 30), (167, 191, 300, 319), (77, 101, 131, 155),
             (5, 5, 9, 9), (90, 140, 100, 150), None]
    N = len(boxes)
    mask = torch.zeros(N, 3, H, W, device=DEV)
    for n, b in enumerate(boxes):
        if b is not None:
            mask[n, n % 3, b[0]:b[1] + 1, b[2]:b[3] + 1] = 1.0     # one channel is enough: any-channel box
    wh, ww = spec.window_size(51, H), spec.window_size(51, W)
    win = torch.full((N, 8), -7, dtype=torch.int32, device=DEV)
    over = torch.zeros(1, device=DEV)
    chain = spec.to_c()
    L.check(L.lib().ufr_cone_window(L.ptr(mask), N, 3 * H * W, 3, H, W, C.byref(chain), wh, ww, L.ptr(win),
                                    L.ptr(over), L.stream()))
    got = win.cpu().tolist()
    assert float(over) == 0.0
    for n, b in enumerate(boxes):
        if b is None:
            assert got[n][:4] == [0, 0, 0, 0]
            continue
        assert got[n][4:] == list(b)
        assert got[n][0] == spec.origin(b[0], b[1], H, wh) and got[n][1] == spec.origin(b[2], b[3], W, ww)
        assert got[n][2] == spec.need(b[0], b[1], H)[1] * 8 and got[n][3] == spec.need(b[2], b[3], W)[1] * 8
    # a window sized for a 9-pixel patch overflows on the 51-pixel box, and says so
    small = spec.window_size(9, H)
    L.check(L.lib().ufr_cone_window(L.ptr(mask), N, 3 * H * W, 3, H, W, C.byref(chain), small, small, L.ptr(win),
                                    L.ptr(over), L.stream()))
    want_over = sum(1 for b in boxes if b is not None and
                    (spec.need(b[0], b[1], H)[1] * 8 > small or spec.need(b[2], b[3], W)[1] * 8 > small))
    assert want_over >= 1 and float(over) == float(want_over)
    w = win.cpu()
    assert int(w[:, 0].min()) >= 0 and int(w[:, 0].max()) <= H - small and int(w[:, 1].max()) <= W - small


def test_window_gather_scatter_match_slicing():
    from understanding_flow_robustness_amd import _lib as L
    g = torch.Generator().manual_seed(2)
    N, Cc, Hf, Wf, wh, ww, ls, m = 4, 5, 24, 40, 8, 12, 4, 2
    src = torch.randn(N, Cc, Hf, Wf, generator=g).to(DEV)
    win = torch.zeros(2, 8, dtype=torch.int32, device=DEV)
    win[0, :2] = torch.tensor([0, 28 * ls // 1], dtype=torch.int32)        # top edge + right edge of the tensor
    win[1, :2] = torch.tensor([8 * ls, 12 * ls], dtype=torch.int32)        # interior
    out = torch.full((N, Cc, wh, ww), 9.0, device=DEV)
    L.check(L.lib().ufr_window_gather(L.ptr(src), L.ptr(out), L.ptr(win), 2, N, Cc, Hf, Wf, wh, ww, ls, m, L.stream()))
    back = torch.full_like(src, -5.0)
    L.check(L.lib().ufr_window_scatter(L.ptr(out), L.ptr(back), L.ptr(win), 2, N, Cc, Hf, Wf, wh, ww, ls, 0, L.stream()))
    for n in range(N):
        y0, x0 = (0, 28) if n % 2 == 0 else (8, 12)
        want = src[n, :, y0:y0 + wh, x0:x0 + ww].clone()
        if n % 2 == 0:                       # rim only on the interior edges: bottom and left
            want[:, wh - m:, :] = 0; want[:, :, :m] = 0
        else:
            want[:, :m] = 0; want[:, wh - m:] = 0; want[:, :, :m] = 0; want[:, :, ww - m:] = 0
        assert torch.equal(out[n], want)
        assert torch.equal(back[n, :, y0:y0 + wh, x0:x0 + ww], want)
        outside = back[n].clone()
        outside[:, y0:y0 + wh, x0:x0 + ww] = -5.0
        assert bool((outside == -5.0).all())
    # scatter with a margin leaves the rim of the destination untouched
    back2 = torch.full_like(src, -5.0)
    L.check(L.lib().ufr_window_scatter(L.ptr(out), L.ptr(back2), L.ptr(win), 2, N, Cc, Hf, Wf, wh, ww, ls, m, L.stream()))
    assert bool((back2[1, :, 8:8 + m, 12:12 + ww] == -5.0).all())
    assert torch.equal(back2[1, :, 8 + m:8 + wh - m, 12 + m:12 + ww - m], src[1, :, 8 + m:8 + wh - m, 12 + m:12 + ww - m])
    # bad arguments are refused on the host
    assert L.lib().ufr_window_gather(L.ptr(src), L.ptr(out), L.ptr(win), 2, N, Cc, Hf, Wf, Hf + 1, ww, ls, m, L.stream()) != 0


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("place", ["edge", "mid"])
def test_windowed_attack_matches_reference_trace(net, place, use_graph):
    """patch_attacks/main.py::attack, two iterations at 192x320 -- the prefix runs on a 96x96 window."""
    from understanding_flow_robustness_amd.patch_attack import _STEP_CACHE_ATTR, attack
    z = load_golden("attack_flownetc_cone_192x320")
    cy, cx = (int(v) for v in z[f"{place}_yx"])
    S = 25
    for name, lr in (("lr5", 5.0), ("lr1e6", 1.0e6)):
        args = Namespace(flownet="FlowNetC", l2=False, alpha=0.0, lr=lr, max_count=2)
        patch = t(z[f"{place}_patch0"], DEV).clone()
        a_t, _, a_r, _ = attack(net, t(z["tgt"], DEV), None, t(z["ref"], DEV), patch, t(z[f"{place}_mask"], DEV),
                                t(z[f"{place}_patch0"], DEV), t(z["target"], DEV), None, args=args, use_graph=use_graph)
        steps = [s for s in net.__dict__[_STEP_CACHE_ATTR].values() if (s.H, s.W) == (192, 320)]
        assert steps and all(s.cone is not None and s.win_hw == (96, 96) for s in steps), "windowed path not taken"
        ref_patch = t(z[f"{place}_{name}_patch"])
        p0 = t(z[f"{place}_patch0"])[:, :, cy:cy + S, cx:cx + S]
        upd = float((ref_patch - p0).abs().max())
        err = float((patch[:, :, cy:cy + S, cx:cx + S].cpu() - ref_patch).abs().max())
        assert err <= REL * max(upd, 1.0), f"{place} {name}: patch err {err:.3e}, update {upd:.3e}"
        assert_close(a_t[:, :, cy:cy + S, cx:cx + S], t(z[f"{place}_{name}_adv_tgt"]), rtol=REL, atol_scale=REL)
        assert_close(a_r[:, :, cy:cy + S, cx:cx + S], t(z[f"{place}_{name}_adv_ref"]), rtol=REL, atol_scale=REL)


@pytest.mark.parametrize("place", ["edge", "mid"])
def test_full_frame_attack_matches_reference_on_the_whole_canvas(place, monkeypatch):
    """`UFR_CONE=0` restores the reference's returned `patch_var` EVERYWHERE (main.py:581-583 adds image gradient to every
    canvas pixel, also outside the mask; the windowed step leaves those as loaded): the whole canvas against
    the reference's own run -- float64 sum and abs-sum over the canvas and every (3rd row, 5th column) sample."""
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    from understanding_flow_robustness_amd.patch_attack import _STEP_CACHE_ATTR, attack
    monkeypatch.setenv("UFR_CONE", "0")
    z, zc = load_golden("attack_flownetc_cone_192x320"), load_golden("attack_flownetc_cone_192x320_canvas")
    fresh = fetch_model(Namespace(flownet="FlowNetC"), synthetic_seed=0).to(DEV)     # its own step cache: no windowed step to reuse
    for name, lr in (("lr5", 5.0), ("lr1e6", 1.0e6)):
        args = Namespace(flownet="FlowNetC", l2=False, alpha=0.0, lr=lr, max_count=2)
        patch = t(z[f"{place}_patch0"], DEV).clone()
        attack(fresh, t(z["tgt"], DEV), None, t(z["ref"], DEV), patch, t(z[f"{place}_mask"], DEV), t(z[f"{place}_patch0"], DEV),
               t(z["target"], DEV), None, args=args)
        assert all(s.cone is None for s in fresh.__dict__[_STEP_CACHE_ATTR].values()), "the full-frame iteration was asked for"
        got = patch.cpu()
        want = t(zc[f"{place}_{name}_canvas_samples"])
        upd = float((want - t(z[f"{place}_patch0"])[:, :, ::3, ::5]).abs().max())
        err = float((got[:, :, ::3, ::5] - want).abs().max())
        assert upd > 1e-6 and err <= REL * upd, f"{place} {name}: canvas err {err:.3e}, update {upd:.3e}"
        moved_outside = float(((want - t(z[f"{place}_patch0"])[:, :, ::3, ::5]) * (1 - t(z[f"{place}_mask"])[:, :, ::3, ::5])).abs().max())
        assert moved_outside > 1e-4 * upd                       # the reference does move pixels outside the mask
        s_sum, s_abs = (float(v) for v in zc[f"{place}_{name}_canvas_sums"])
        assert abs(float(got.double().sum()) - s_sum) <= REL * s_abs and abs(float(got.double().abs().sum()) - s_abs) <= REL * s_abs


def _run_step(net, use_cone, masks, B, H, W, lr, shared, iters=3, seed=0, use_graph=True):
    """`masks`: canvas masks [B,3,H,W] (one pair, or per-sample patches), or -- one patch behind B > 1 pairs, which
    lives in patch coordinates -- tuples (mask_p [1,3,ph,pw], origins [(row, column)] * B)."""
    from understanding_flow_robustness_amd.patch_attack import PatchAttackStep
    args = Namespace(flownet="FlowNetC", l2=False, alpha=0.0, lr=lr, max_count=iters)
    placed = isinstance(masks[0], tuple)
    assert placed == (shared and B > 1)
    patch_hw = tuple(masks[0][0].shape[-2:]) if placed else None
    step = PatchAttackStep(net, args, B, H, W, device=DEV, shared_patch=shared, use_cone=use_cone, use_graph=use_graph,
                           patch_hw=patch_hw)
    g = torch.Generator().manual_seed(seed)
    tgt, ref = torch.rand(B, 3, H, W, generator=g).to(DEV), torch.rand(B, 3, H, W, generator=g).to(DEV)
    patch = (torch.rand(1, 3, *patch_hw, generator=g) if placed else torch.rand(1 if shared else B, 3, H, W, generator=g)).to(DEV)
    target = torch.randn(B, 2, H, W, generator=g).to(DEV)
    outs = []
    for mask in masks:
        if placed:
            step.load(tgt, ref, patch, mask[0], patch, target, origins=mask[1])
        else:
            step.load(tgt, ref, patch, mask, patch, target)
        n, loss = step.run(iters)
        outs.append((step.patch.clone(), step.adv_tgt.detach().clone(), n, loss))
    return step, patch, outs


def _engine_on():
    import os
    return os.environ.get("UFR_ENGINE", "1") == "1"


def _sel(mask, shared):
    """Where two implementations of a step must agree: the patch pixels a mask shows."""
    if isinstance(mask, tuple):
        return mask[0]
    return mask.amax(0, keepdim=True) if shared else mask


def _unclamped_lr(net, mask, B, H, W, shared):
    """Random-init gradients are tiny and scale with 1/(H*W): pick the lr whose first update peaks at 0.5,
    so the +-2 clamp (which would hide any gradient error) stays inactive for a few iterations."""
    _, p0, out = _run_step(net, False, [mask], B, H, W, 1.0, shared, iters=1, use_graph=False)
    return 0.5 / float(((out[0][0] - p0) * _sel(mask, shared)).abs().max())


def _same_update(pf, pc, p0, sel, what):
    """Two implementations of the same multi-iteration attack.  From the second iteration on a one-ulp
    difference can flip a LeakyReLU somewhere and move the gradient entries behind it, so: at least 95% of the patch
    pixels agree to 1e-4 of the update and every pixel to 5e-2 (a misplaced window or band is off by O(1)).
    The control (tools/diag_step_chaos.py, profiles/r2_step_chaos_control.txt): two FULL-FRAME steps that differ only in
    the igemm kernel's summation order agree to 2.4e-7 after one iteration and drift to 7.8e-3 / 1.5e-2 of the update on
    ~1% of one placement's pixels after two / three, while the windowed step stays within 5e-7 of the full-frame step
    that sums in its order."""
    upd = float(((pf - p0) * sel).abs().max())
    err = ((pf - pc) * sel).abs()
    assert 1e-3 < upd < 1.9, f"{what}: test lr leaves the update degenerate ({upd})"
    off = float((err > 1e-4 * upd + 1e-6).sum()) / max(float((sel != 0).sum()), 1.0)
    worst = 5e-2
    assert off <= 0.05 and float(err.max()) <= worst * upd, \
        f"{what}: {off:.2%} of the patch pixels differ by more than 1e-4, worst {float(err.max()) / upd:.2e} of the update"
    return upd


def test_later_iteration_form_equals_the_full_frame_step_from_a_shared_state(net):
    """The LATER-iteration form of the step (`graph_next`: windowed prefix, band-only forward of the head's first blocks from the
    cached activations, banded adjoints, rectangle-only re-paste) held STRICTLY: both steps run iteration 1, then the full-frame
    step's patch is injected into the windowed step, so iteration 2 starts from ONE shared state and `_same_update`'s slack for
    compounded LeakyReLU flips is not needed -- 1e-5 of the second update, 4 pairs at 384x1280 behind one patch (corner, edges,
    interior)."""
    from understanding_flow_robustness_amd.patch_attack import PatchAttackStep
    B, H, W, S = 4, 384, 1280, 51
    g = torch.Generator().manual_seed(17)
    tgt, ref = torch.rand(B, 3, H, W, generator=g).to(DEV), torch.rand(B, 3, H, W, generator=g).to(DEV)
    target = torch.randn(B, 2, H, W, generator=g).to(DEV)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    mask_p = (((yy - 25) ** 2 + (xx - 25) ** 2) <= 23 ** 2).float().expand(1, 3, S, S).contiguous().to(DEV)
    patch0 = torch.rand(1, 3, S, S, generator=g).to(DEV)
    origins = [(0, 0), (333, 1229), (0, 600), (170, 640)]

    def make(cone, graph, lr):
        args = Namespace(flownet="FlowNetC", l2=False, alpha=0.0, lr=lr, max_count=2)
        st = PatchAttackStep(net, args, B, H, W, device=DEV, patch_hw=(S, S), use_cone=cone, use_graph=graph)
        st.load(tgt, ref, patch0, mask_p, patch0, target, origins=origins)
        st.run(0)                                      # capture (graphs) + reload
        return st
    probe = make(False, False, 1.0)
    probe._iteration()
    lr = 0.25 / float(((probe.patch - patch0) * mask_p).abs().max())     # two unclamped updates
    full, win = make(False, False, lr), make(True, True, lr)
    assert win.cone is not None and win.band is not None and win.band.inc_layers and win.graph_next is not win.graph
    full._iteration()
    win._iteration()
    p1 = full.patch.detach().clone()
    first = float(((win.patch - p1) * mask_p).abs().max()) / float(((p1 - patch0) * mask_p).abs().max())
    assert first <= 1e-4, first                          # (the strict one-iteration test holds this to 1e-5)
    with torch.no_grad():                                # ONE shared state for iteration 2
        win.patch.copy_(p1)
        win._paste(do_clamp=True)
    assert torch.equal(win.adv_tgt.detach(), full.adv_tgt.detach()) and not win._first
    full._iteration()
    win._iteration()                                     # graph_next
    upd2 = float(((full.patch - p1) * mask_p).abs().max())
    err2 = float(((win.patch - full.patch) * mask_p).abs().max())
    print(f"second update {upd2:.3e}; later-iteration form vs full-frame step {err2 / upd2:.2e} of it")
    assert upd2 > 1e-3 and err2 <= 1e-5 * upd2, f"{err2 / upd2:.2e} of the second update"


def test_incremental_head_forward_equals_full_forward(net):
    """The deterministic half of the windowed step, checked strictly: after an update of the patch, the flow
    from the band-only recomputation of conv3_1 / conv4 / conv4_1 (cached activations of the previous
    iteration elsewhere) equals the flow of the full head forward."""
    from understanding_flow_robustness_amd.patch_attack import PatchAttackStep
    B, H, W = 4, 384, 1280
    args = Namespace(flownet="FlowNetC", l2=False, alpha=0.0, lr=1.0e7, max_count=3)     # saturating step: a large change
    step = PatchAttackStep(net, args, B, H, W, device=DEV, shared_patch=False, use_graph=False)
    g = torch.Generator().manual_seed(3)
    tgt, ref = torch.rand(B, 3, H, W, generator=g).to(DEV), torch.rand(B, 3, H, W, generator=g).to(DEV)
    patch = torch.rand(B, 3, H, W, generator=g).to(DEV)
    target = torch.randn(B, 2, H, W, generator=g).to(DEV)
    mask = torch.zeros(B, 3, H, W, device=DEV)
    for b, (y, x) in enumerate([(0, 0), (333, 1229), (170, 615), (100, 1100)]):
        mask[b, :, y:y + 51, x:x + 51] = 1
    step.load(tgt, ref, patch, mask, patch, target)
    assert step.band is not None and step.band.inc_layers
    before = step.adv_tgt.detach().clone()
    step._iteration()                                        # first iteration: full forward, caches filled, patch updated
    assert float((step.adv_tgt.detach() - before).abs().max()) > 1e-3, "the update must change the frames"
    with torch.enable_grad():
        def head_output():            # the full-size flow, or (the loss kernel upsamples it itself) the engine's flow2
            f = step._forward_cone()
            return (step.eng.flow[2] if f is None else f).detach().clone()
        step.band.incremental = True
        f_inc = head_output()
        step.band.incremental = False
        f_full = head_output()
    scale = float(f_full.abs().max())
    assert float((f_inc - f_full).abs().max()) <= 1e-5 * scale, float((f_inc - f_full).abs().max()) / scale


def test_windowed_step_equals_full_frame_step_at_bench_size(net):
    """384x1280 (BASELINE configs[1] frame size), per-sample placements in the corners, on the edges and in
    the interior, re-placed between attack() calls of ONE captured step: same patch as the full-frame
    iteration (`_same_update`); the second call grows nothing and re-captures nothing."""
    B, H, W = 4, 384, 1280
    def masks_for(places):
        m = torch.zeros(B, 3, H, W, device=DEV)
        yy, xx = torch.meshgrid(torch.arange(51, device=DEV), torch.arange(51, device=DEV), indexing="ij")
        disc = (((yy - 25) ** 2 + (xx - 25) ** 2) <= 25 ** 2).float()
        for b, (y, x) in enumerate(places):
            m[b, :, y:y + 51, x:x + 51] = disc
        return m
    places1 = [(0, 0), (333, 1229), (0, 600), (170, 1229)]
    places2 = [(333, 0), (160, 640), (7, 1221), (160, 660)]              # two placements overlap
    yy, xx = torch.meshgrid(torch.arange(51, device=DEV), torch.arange(51, device=DEV), indexing="ij")
    disc = (((yy - 25) ** 2 + (xx - 25) ** 2) <= 25 ** 2).float().expand(1, 3, 51, 51).contiguous()
    for shared in (False, True):
        # per-sample canvas patches, then ONE patch in patch coordinates behind the four pairs
        first, second = ((disc, places1), (disc, places2)) if shared else (masks_for(places1), masks_for(places2))
        lr = _unclamped_lr(net, first, B, H, W, shared)
        s_full, p0, full = _run_step(net, False, [first, second], B, H, W, lr, shared)
        s_cone, _, cone = _run_step(net, True, [first, second], B, H, W, lr, shared)
        assert s_full.cone is None and s_cone.cone is not None
        assert s_cone.win_hw == (128, 128), s_cone.win_hw
        assert s_cone.band is not None and s_cone.band.width == 608       # conv3_1..conv5 adjoints on a column band
        graph_before = s_cone.graph
        for (pf, af, nf, lf), (pc, ac, nc, lc), mask in zip(full, cone, (first, second)):
            upd = _same_update(pf, pc, p0, _sel(mask, shared), f"shared={shared}")
            assert nf == nc and abs(lf - lc) <= 1e-4 * max(abs(lf), 1.0)
            assert float((af - ac).abs().max()) <= 5e-3 * upd + 1e-6
        assert s_cone.graph is graph_before


def test_windowed_step_random_placements(net):
    """24 seeded random placements (8 pairs x 3 attack() calls of one captured step, private patches) at the
    benchmark size: window, column band and windowed correlation adjoint against the full-frame step."""
    B, H, W = 8, 384, 1280
    g = torch.Generator().manual_seed(1234)
    yy, xx = torch.meshgrid(torch.arange(51, device=DEV), torch.arange(51, device=DEV), indexing="ij")
    disc = (((yy - 25) ** 2 + (xx - 25) ** 2) <= 23 ** 2).float()
    masks = []
    for _ in range(3):
        m = torch.zeros(B, 3, H, W, device=DEV)
        for b in range(B):
            y = int(torch.randint(0, H - 51 + 1, (1,), generator=g))
            x = int(torch.randint(0, W - 51 + 1, (1,), generator=g))
            m[b, :, y:y + 51, x:x + 51] = disc
        masks.append(m)
    lr = _unclamped_lr(net, masks[0], B, H, W, False)
    s_full, p0, full = _run_step(net, False, masks, B, H, W, lr, False, iters=2)
    for use_graph in (True, False):          # two captured graphs (first / later iterations) and the eager form
        s_cone, _, cone = _run_step(net, True, masks, B, H, W, lr, False, iters=3 if use_graph else 2, use_graph=use_graph)
        assert s_cone.cone is not None and s_cone.band is not None and s_cone.band.width > 0
        assert s_cone.band.inc_layers == ("conv3_1", "conv4", "conv4_1")
        if not _engine_on():                     # the torch spelling keeps its activation caches on the band object
            assert set(s_cone.band.caches) == set(s_cone.band.inc_layers)
        if use_graph:
            assert s_cone.graph_next is not None and s_cone.graph_next is not s_cone.graph
            s_ref, _, ref3 = _run_step(net, False, masks, B, H, W, lr, False, iters=3)
            want = ref3
        else:
            want = full
        for (pf, _, nf, _), (pc, _, nc, _), mask in zip(want, cone, masks):
            _same_update(pf, pc, p0, mask, f"graph={use_graph}")
            assert nf == nc


def test_window_grows_when_a_larger_mask_arrives(net):
    """A step sized for a 21-pixel patch receives a 51-pixel one: the device flags the overflow, the host
    re-sizes, re-captures and redoes the call; the result equals the full-frame step."""
    B, H, W = 1, 192, 320
    small = torch.zeros(B, 3, H, W, device=DEV); small[:, :, 40:61, 100:121] = 1
    large = torch.zeros(B, 3, H, W, device=DEV); large[:, :, 90:141, 200:251] = 1
    lr = _unclamped_lr(net, large, B, H, W, True)
    s_full, p0, full = _run_step(net, False, [small, large], B, H, W, lr, True, iters=2)
    s_cone, _, cone = _run_step(net, True, [small, large], B, H, W, lr, True, iters=2)
    assert s_cone.win_hw is not None and s_cone.win_hw[0] >= 128
    for (pf, _, nf, _), (pc, _, nc, _), mask in zip(full, cone, (small, large)):
        _same_update(pf, pc, p0, mask, "grown window")
        assert nf == nc


@pytest.mark.parametrize("P,DP,C", [(21, 2, 256), (9, 1, 30)])
def test_corr_backward_window_equals_full_adjoint_on_the_window(P, DP, C):
    """csrc/correlation_window.hip against the full adjoint (pinned to the reference by tests/test_ops_gpu.py):
    equal on each sample's window cells (corners, edges, interior), exactly zero elsewhere."""
    from understanding_flow_robustness_amd import _lib as L
    from understanding_flow_robustness_amd import spatial_correlation_sampler_backend as be
    g = torch.Generator().manual_seed(P)
    B, H, W, wh, ww, ls = 4, 24, 40, 6, 8, 8
    a, b = torch.randn(B, C, H, W, generator=g).to(DEV), torch.randn(B, C, H, W, generator=g).to(DEV)
    go = torch.randn(B, P, P, H, W, generator=g).to(DEV)
    want1, want2 = be.backward(a, b, go, 1, 1, P, P, 0, 0, 1, 1, DP, DP, 1, 1)
    origins = [(0, 0), (H - wh, W - ww), (0, 17), (9, 11)]
    win = torch.zeros(B, 8, dtype=torch.int32, device=DEV)
    for n, (y, x) in enumerate(origins):
        win[n, 0], win[n, 1] = y * ls, x * ls
    g1, g2 = torch.full_like(a, 7.0), torch.full_like(b, 7.0)
    L.check(L.lib().ufr_corr_backward_window(L.ptr(a), L.ptr(b), L.ptr(go), L.ptr(g1), L.ptr(g2), B, C, H, W, P, DP,
                                             L.ptr(win), ls, wh, ww, L.stream()))
    inside = torch.zeros(B, 1, H, W, dtype=torch.bool, device=DEV)
    for n, (y, x) in enumerate(origins):
        inside[n, :, y:y + wh, x:x + ww] = True
    for got, want, name in ((g1, want1, "grad_input1"), (g2, want2, "grad_input2")):
        assert float(got.masked_select(~inside.expand_as(got)).abs().max()) == 0.0, name
        scale = float(want.abs().max())
        err = float(((got - want) * inside).abs().max())
        assert err <= 1e-5 * scale, f"{name}: {err:.3e} of {scale:.3e}"


def test_pwc_windowed_pyramid_prefix_equals_full_frame_step():
    """PWC-Net: pyramid levels 1-2 on a 120x120 window per pair (cone.py) against the full-frame iteration at
    384x1280: strictly after one iteration (same state, gradients differ by rounding only), robustly after two."""
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    from understanding_flow_robustness_amd.patch_attack import PatchAttackStep
    B, H, W = 2, 384, 1280
    net = fetch_model(Namespace(flownet="PWCNet"), synthetic_seed=1).to(DEV)
    g = torch.Generator().manual_seed(21)
    tgt, ref = torch.rand(B, 3, H, W, generator=g).to(DEV), torch.rand(B, 3, H, W, generator=g).to(DEV)
    patch = torch.rand(B, 3, H, W, generator=g).to(DEV)
    target = torch.randn(B, 2, H, W, generator=g).to(DEV)
    mask = torch.zeros(B, 3, H, W, device=DEV)
    for b, (y, x) in enumerate([(0, 1229), (170, 600)]):
        mask[b, :, y:y + 51, x:x + 51] = 1

    def run(use_cone, lr, iters):
        args = Namespace(flownet="PWCNet", l2=False, alpha=0.0, lr=lr, max_count=iters)
        step = PatchAttackStep(net, args, B, H, W, device=DEV, shared_patch=False, use_cone=use_cone, use_graph=False)
        step.load(tgt, ref, patch, mask, patch, target)
        n, _ = step.run(iters)
        return step, step.patch.clone(), n
    _, probe, _ = run(False, 1.0, 1)
    lr = 0.5 / float(((probe - patch) * mask).abs().max())
    for iters in (1, 2):
        s_full, pf, nf = run(False, lr, iters)
        s_cone, pc, nc = run(True, lr, iters)
        assert s_full.cone is None and s_cone.cone is not None and s_cone.win_hw == (120, 120)
        assert nf == nc == iters
        if iters == 1:
            upd = float(((pf - patch) * mask).abs().max())
            err = float(((pf - pc) * mask).abs().max())
            assert err <= 1e-4 * upd + 1e-6, f"one iteration: {err:.3e} of {upd:.3e}"
        else:
            _same_update(pf, pc, patch, mask, "PWC-Net, two iterations")


def test_attack_notices_new_weights(net):
    """A cached step (captured graphs, pre-packed engine weights) must not survive a change of the network's weights:
    after scaling one head convolution in place, attack() gives the result of a freshly built step, not the old one."""
    import copy
    from understanding_flow_robustness_amd.patch_attack import _STEP_CACHE_ATTR, attack
    z = load_golden("attack_flownetc_cone_192x320")
    args = Namespace(flownet="FlowNetC", l2=False, alpha=0.0, lr=1.0e6, max_count=2)      # saturating step: clamped signs
    run = lambda n: attack(n, t(z["tgt"], DEV), None, t(z["ref"], DEV), t(z["mid_patch0"], DEV).clone(), t(z["mid_mask"], DEV),
                           t(z["mid_patch0"], DEV), t(z["target"], DEV), None, args=args)[3]
    engines = net.__dict__.pop("_ufr_head_engines", None)
    steps = net.__dict__.pop(_STEP_CACHE_ATTR, None)
    net2 = copy.deepcopy(net)
    if engines is not None:
        net.__dict__["_ufr_head_engines"] = engines
    if steps is not None:
        net.__dict__[_STEP_CACHE_ATTR] = steps
    p_before = run(net2).clone()
    with torch.no_grad():
        net2.conv4_1[0].weight.mul_(-1.0)
    p_after = run(net2).clone()
    held = {k: net2.__dict__.pop(k) for k in ("_ufr_head_engines", _STEP_CACHE_ATTR) if k in net2.__dict__}
    fresh = copy.deepcopy(net2)                  # (captured graphs and ctypes descriptors cannot be copied)
    net2.__dict__.update(held)
    p_fresh = run(fresh)
    assert float((p_after - p_before).abs().max()) > 1e-3, "the weight change did not reach the attack"
    # (identical kernels and data: bit-equal with the engine's fixed-order reductions; MIOpen's prefix under
    # UFR_ENGINE_PREFIX=0 is not bit-reproducible from one handle to the next)
    assert float((p_after - p_fresh).abs().max()) <= 1e-5 * max(1.0, float(p_fresh.abs().max()))
