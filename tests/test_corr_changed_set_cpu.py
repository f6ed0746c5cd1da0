"""CPU suite: the geometry behind ufr_corr_forward_planes_changed (csrc/correlation_planes.hip) and the entry's refusals.

The cost volume out[d = (dy, dx), y, x] = <f1[:, y, x], f2[:, y + 2 (dy - 10), x + 2 (dx - 10)]> is built twice with torch on
the CPU; between the two builds both feature maps change inside one rectangle of cells only.  Every entry that differs must
have its cell (A) or its source cell (B) in the rectangle: that set is all the incremental kernel recomputes.  The refusals
run through the library before any HIP call, so nothing here needs a device."""
import ctypes

import pytest
import torch

C, P, R = 8, 21, 10


def volume(f1, f2):
    """[441, H, W]; a source cell outside the frame contributes 0."""
    _, H, W = f1.shape
    pad = torch.zeros(C, H + 4 * R, W + 4 * R, dtype=f1.dtype)
    pad[:, 2 * R:2 * R + H, 2 * R:2 * R + W] = f2
    out = torch.empty(P * P, H, W, dtype=f1.dtype)
    for dy in range(P):
        for dx in range(P):
            out[dy * P + dx] = (f1 * pad[:, 2 * dy:2 * dy + H, 2 * dx:2 * dx + W]).sum(0)
    return out


def allowed(H, W, rect):
    """[441, H, W] bool: (A) the cell or (B) its source cell lies in rect = (y0, y1, x0, x1)."""
    y0, y1, x0, x1 = rect
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    inside = lambda y, x: (y >= y0) & (y < y1) & (x >= x0) & (x < x1)
    ok = torch.empty(P * P, H, W, dtype=torch.bool)
    for dy in range(P):
        for dx in range(P):
            ok[dy * P + dx] = inside(yy, xx) | inside(yy + 2 * (dy - R), xx + 2 * (dx - R))
    return ok


FRAMES = {(24, 40): None, (64, 80): None}


def base(H, W):
    if FRAMES[(H, W)] is None:
        g = torch.Generator().manual_seed(H * 1000 + W)
        f1, f2 = torch.randn(C, H, W, generator=g, dtype=torch.float64), torch.randn(C, H, W, generator=g, dtype=torch.float64)
        FRAMES[(H, W)] = (f1, f2, volume(f1, f2))
    return FRAMES[(H, W)]


def rectangles(H, W):
    h, w = 12, 12
    return {
        "interior": (6, 6 + h, 10, 10 + w),
        "top left corner": (0, h, 0, w),
        "top right corner": (0, h, W - w, W),
        "bottom left corner": (H - h, H, 0, w),
        "bottom right corner": (H - h, H, W - w, W),
        "odd origin": (5, 5 + h, 13, 13 + w),
        "odd origin, odd size": (3, 3 + 7, 7, 7 + 11),
    }


@pytest.mark.parametrize("name", list(rectangles(24, 40)))
@pytest.mark.parametrize("H,W", list(FRAMES))
def test_entries_change_only_where_the_cell_or_its_source_cell_is_in_the_rectangle(H, W, name):
    f1, f2, before = base(H, W)
    y0, y1, x0, x1 = rect = rectangles(H, W)[name]
    assert 0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W
    g = torch.Generator().manual_seed(7)
    g1, g2 = f1.clone(), f2.clone()
    g1[:, y0:y1, x0:x1] = torch.randn(C, y1 - y0, x1 - x0, generator=g, dtype=torch.float64)
    g2[:, y0:y1, x0:x1] = torch.randn(C, y1 - y0, x1 - x0, generator=g, dtype=torch.float64)
    changed = volume(g1, g2) != before
    ok = allowed(H, W, rect)
    assert not bool((changed & ~ok).any()), f"{name}: an entry outside (A) and (B) changed"
    # the bound is tight (random features: every reachable entry with a source cell in the frame does change), and small
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    in_frame = torch.stack([((yy + 2 * (d // P - R)) >= 0) & ((yy + 2 * (d // P - R)) < H) & ((xx + 2 * (d % P - R)) >= 0)
                            & ((xx + 2 * (d % P - R)) < W) for d in range(P * P)])
    assert torch.equal(changed, ok & in_frame)
    assert int(changed.sum()) <= 2 * (y1 - y0) * (x1 - x0) * P * P


def test_the_entry_refuses_what_it_was_not_built_for():
    """Validation precedes every HIP call; the pointers are never dereferenced."""
    from understanding_flow_robustness_amd import _lib as L
    lib = L.lib()
    p = ctypes.c_void_p(4096)
    EINVAL, EUNSUPPORTED = -1, -2

    def call(f1=p, f2=p, out=p, win=p, B=2, Cn=256, H=48, W=160, patch=21, dil=2, ls=8, wh=16, ww=16, margin=2, chunk0=1):
        return lib.ufr_corr_forward_planes_changed(f1, f2, 1 << 20, out, 1 << 20, chunk0, B, Cn, H, W, patch, dil, 1.0 / 256.0, 0.1, win,
                                                   ls, wh, ww, margin, None)

    for kw in (dict(f1=None), dict(f2=None), dict(out=None), dict(win=None)):
        assert call(**kw) == EINVAL and b"null pointer" in lib.ufr_last_error(), kw
    for kw in (dict(Cn=128), dict(patch=9), dict(dil=1), dict(ww=24)):
        assert call(**kw) == EUNSUPPORTED, kw
    assert b"cells=24" in lib.ufr_last_error()
    for kw in (dict(B=0), dict(H=0), dict(W=-1), dict(ls=0), dict(wh=0), dict(ww=0), dict(margin=-1), dict(chunk0=-1),
               dict(H=8), dict(W=8), dict(wh=16, ww=16, margin=9), dict(wh=16, ww=8, margin=5), dict(wh=8, ww=16, margin=5)):
        assert call(**kw) == EINVAL, kw
    # the window form's limits are where they were, and the widest window the changed form takes is the window form's too
    assert lib.ufr_corr_forward_planes_window(p, p, 1 << 20, p, 1 << 20, 1, 2, 256, 48, 160, 21, 2, 1.0 / 256.0, 0.1, p, 8, 24,
                                              None) == EUNSUPPORTED
