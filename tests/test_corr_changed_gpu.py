"""GPU suite: ufr_corr_forward_planes_changed (csrc/correlation_planes.hip) -- the cost volume's entries that can change when the
features change inside each sample's rectangle only -- against ufr_corr_forward_planes on the same features, bit for bit
(torch.equal on the raw planes; nothing here is compared by tolerance), and the attack step with and without it."""
from argparse import Namespace

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, LS = 3, 8                           # three placements per launch; cells of 8 pixels (conv3)
SENTINEL = 3.0


def _mods():
    from understanding_flow_robustness_amd import _lib as L
    from understanding_flow_robustness_amd import igemm as ig
    return L, ig


def new_out(ig, H, W):
    """conv3_1's input as the engine lays it out: chunk 0 (conv_redir's) in front, the volume in chunks 1..14."""
    out = ig.Planes(B, H, W, 15, DEV)
    out.t[:, 0] = SENTINEL
    out.t[:, 14, :, 25:] = SENTINEL     # channels 441..447
    return out


def full(L, a, b, out, H, W):
    L.check(L.lib().ufr_corr_forward_planes(L.ptr(a.t), L.ptr(b.t), a.plane_stride, L.ptr(out.t), out.plane_stride, 1, B, 256, H, W,
                                            21, 2, 1.0 / 256.0, 0.1, L.stream()))
    return out


_BASE = {}


def base(H, W):
    """Random features and their full volume, computed once per frame size and never written again."""
    if (H, W) not in _BASE:
        L, ig = _mods()
        g = torch.Generator().manual_seed(100 * H + W)
        f1, f2 = torch.randn(B, 256, H, W, generator=g).to(DEV), torch.randn(B, 256, H, W, generator=g).to(DEV)
        a, b = ig.Planes(B, H, W, 8, DEV).load_nchw(f1), ig.Planes(B, H, W, 8, DEV).load_nchw(f2)
        _BASE[(H, W)] = (f1, f2, full(L, a, b, new_out(ig, H, W), H, W))
    return _BASE[(H, W)]


def rectangle(win_yx, H, W, wh, ww, margin):
    """plane_layout.hip `window_features_kernel`: origin in cells (C division: towards zero), clamped; the rim of `margin` cells
    is trimmed on every edge that is not a frame edge."""
    y0 = min(max(int(win_yx[0] / LS), 0), H - wh)
    x0 = min(max(int(win_yx[1] / LS), 0), W - ww)
    return (y0 + (margin if y0 > 0 else 0), y0 + wh - (margin if y0 + wh < H else 0),
            x0 + (margin if x0 > 0 else 0), x0 + ww - (margin if x0 + ww < W else 0)), (y0, x0)


def windows(H, W, wh, ww, k):
    """Three pixel origins per launch: cell origins times 8 plus a remainder the division drops."""
    sets = [
        [(0, 0), ((H - wh) * LS, (W - ww) * LS), (3 * LS + 5, 5 * LS + 7)],                    # both corners; odd y0, odd x0
        [(-3 * LS, (W + 9) * LS), (1 * LS + 1, 2 * LS), ((H + 4) * LS, -1)],                    # clamped on every side; odd y0, even x0
        [(2 * LS, 7 * LS + 3), (0, (W - ww) * LS), ((H - wh) * LS + 7, 1 * LS)],               # even y0, odd x0; the other corners
    ]
    return sets[k]


CASES = [(wh, ww, margin, k) for (wh, ww) in ((16, 16), (8, 8), (16, 23)) for margin in (0, 2) for k in range(3)]


@pytest.mark.parametrize("wh,ww,margin,k", CASES)
@pytest.mark.parametrize("H,W", [(24, 40), (64, 80)])
def test_changed_entries_equal_the_full_volume_bit_for_bit(H, W, wh, ww, margin, k):
    """24 x 40 cells: the reach of 20 cells is clipped on all four sides; 64 x 80: rows and columns lie outside every reach."""
    L, ig = _mods()
    f1, f2, out0 = base(H, W)
    origins = windows(H, W, wh, ww, k)
    win = torch.zeros(B, 8, dtype=torch.int32, device=DEV)
    win[:, :2] = torch.tensor(origins, dtype=torch.int32)
    g = torch.Generator().manual_seed(17 + k)
    g1, g2 = f1.clone(), f2.clone()
    cells = set()
    for b, o in enumerate(origins):
        (y0, y1, x0, x1), (wy0, wx0) = rectangle(o, H, W, wh, ww, margin)
        assert 0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W
        cells.add((wy0 % 2, wx0 % 2, wy0 == 0, wx0 == 0, wy0 + wh == H, wx0 + ww == W))
        g1[b, :, y0:y1, x0:x1] = torch.randn(256, y1 - y0, x1 - x0, generator=g).to(DEV)
        g2[b, :, y0:y1, x0:x1] = torch.randn(256, y1 - y0, x1 - x0, generator=g).to(DEV)
    assert len(cells) == B                                          # three different kinds of placement in one launch
    a, bb = ig.Planes(B, H, W, 8, DEV).load_nchw(g1), ig.Planes(B, H, W, 8, DEV).load_nchw(g2)
    expected = full(L, a, bb, new_out(ig, H, W), H, W)
    got = new_out(ig, H, W)
    got.t.copy_(out0.t)
    L.check(L.lib().ufr_corr_forward_planes_changed(L.ptr(a.t), L.ptr(bb.t), a.plane_stride, L.ptr(got.t), got.plane_stride, 1, B, 256,
                                                    H, W, 21, 2, 1.0 / 256.0, 0.1, L.ptr(win), LS, wh, ww, margin, L.stream()))
    torch.cuda.synchronize()
    e16, g16, o16 = (t.t.view(torch.int16) for t in (expected, got, out0))
    differing = int((e16 != o16).sum())
    wrong = int((e16 != g16).sum())
    print(f"{H}x{W} window {wh}x{ww} margin {margin} set {k}: {differing} plane values change, {wrong} wrong after the changed form")
    assert differing > 10000                                        # the new features do move the volume: the test has power
    assert bool((got.t[:, 0] == SENTINEL).all()), "the chunk in front of the volume was written"
    assert bool((got.t[:, 14, :, 25:] == SENTINEL).all()), "channels 441..447 were written"
    assert torch.equal(g16, e16)


def test_attack_step_with_the_changed_form_equals_the_step_with_the_window_form():
    """2 pairs at 128 x 768 behind a 20-pixel disc (the shapes of tests/test_attack_glue_gpu.py), eager, three iterations of one
    call -- the second and third are later iterations -- with `corr_changed` on and off: every result is equal."""
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    from understanding_flow_robustness_amd.patch_attack import PatchAttackStep
    Bn, H, W, S = 2, 128, 768, 20
    net = fetch_model(Namespace(flownet="FlowNetC"), synthetic_seed=0).to(DEV)
    for p in net.parameters():
        p.requires_grad_(False)
    g = torch.Generator().manual_seed(29)
    tgt, ref = torch.rand(Bn, 3, H, W, generator=g).to(DEV), torch.rand(Bn, 3, H, W, generator=g).to(DEV)
    target = torch.randn(Bn, 2, H, W, generator=g).to(DEV)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    disc = (((yy - 9.5) ** 2 + (xx - 9.5) ** 2) <= 10.0 ** 2).float().expand(1, 3, S, S).contiguous().to(DEV)
    patch0 = torch.rand(1, 3, S, S, generator=g).to(DEV)
    origins = [(0, 300), (50, 400)]

    def run(lr, corr_changed, iterations):
        args = Namespace(flownet="FlowNetC", l2=False, alpha=0.0, lr=lr, max_count=iterations)
        step = PatchAttackStep(net, args, Bn, H, W, device=DEV, patch_hw=(S, S), use_graph=False, corr_changed=corr_changed)
        step.load(tgt, ref, patch0, disc, patch0, target, origins=origins)
        n, loss = step.run(iterations)
        assert step.eng is not None and step.band.width and step.band.cone_hw[1] // 8 <= 23
        return step.patch.clone(), loss, step.adv_tgt.detach().clone(), step.adv_ref.detach().clone(), n

    probe = run(1.0, False, 1)
    lr = 0.25 / float(((probe[0] - patch0) * disc).abs().max())     # updates of a quarter: visible, unclamped
    (pa, la, ta, ra, na), (pb, lb, tb, rb, nb) = run(lr, True, 3), run(lr, False, 3)
    assert na == nb == 3
    assert torch.equal(pa, pb) and la == lb and torch.equal(ta, tb) and torch.equal(ra, rb)
    assert float(((pa - patch0) * disc).abs().max()) > 0.1
