"""GPU suite: csrc/attack.hip `ufr_flow2_upsampled_loss_fast` against `ufr_flow2_upsampled_loss`.  The fast launch keeps the tiles,
the pixel-to-thread assignment, the per-pixel arithmetic and the order of every sum, so the gradient AND the loss are compared with
torch.equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 2


# 16 x 16: one tile; 17 x 33 and 5 x 7: partial tiles, 5 x 7 with all four borders inside one tile; 24 x 80: level 2 of a 96 x 320
# frame, several full tiles and a partial row of them; 1 x 1 and 1 x 3: the index clamp on both sides of the same cell
@pytest.mark.parametrize("h,w", [(16, 16), (17, 33), (5, 7), (24, 80), (1, 1), (1, 3)])
@pytest.mark.parametrize("kind", [0, 1])
def test_fast_loss_equals_the_reference_launch(kind, h, w):
    from understanding_flow_robustness_amd import _lib as L
    lib, st = L.lib(), L.stream()
    g = torch.Generator().manual_seed(100 * h + w)
    flow2 = torch.randn(B, 2, h, w, generator=g).to(DEV)
    target = torch.randn(B, 2, 4 * h, 4 * w, generator=g).to(DEV)
    if kind == 0:
        flow2[0, :, 0, 0] = 0.0                            # a zero flow vector: the branch without the division by |flow|^2
    ws_old, ws_new = torch.zeros(L.LOSS_PARTIALS, device=DEV), torch.zeros(L.LOSS_PARTIALS, device=DEV)
    g_old, g_new = torch.full_like(flow2, float("nan")), torch.full_like(flow2, float("nan"))
    loss_old, loss_new = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    L.check(lib.ufr_flow2_upsampled_loss(L.ptr(flow2), 20.0, L.ptr(target), L.ptr(g_old), L.ptr(loss_old), B, h, w, kind, 0.75,
                                         L.ptr(ws_old), st))
    L.check(lib.ufr_flow2_upsampled_loss_fast(L.ptr(flow2), 20.0, L.ptr(target), L.ptr(g_new), L.ptr(loss_new), B, h, w, kind, 0.75,
                                              L.ptr(ws_new), st))
    assert bool(torch.isfinite(g_old).all()) and float(g_old.abs().max()) > 0.0
    assert torch.equal(g_new, g_old)
    assert torch.equal(ws_new, ws_old)                     # every workgroup's partial sum
    assert torch.equal(loss_new, loss_old) and float(loss_old) != 0.0


def test_fast_loss_refuses_what_the_reference_launch_refuses():
    from understanding_flow_robustness_amd import _lib as L
    lib = L.lib()
    p = torch.zeros(8, device=DEV)
    assert lib.ufr_flow2_upsampled_loss_fast(None, 20.0, L.ptr(p), L.ptr(p), L.ptr(p), 1, 1, 1, 0, 1.0, L.ptr(p), L.stream()) == -1
    assert lib.ufr_flow2_upsampled_loss_fast(L.ptr(p), 20.0, L.ptr(p), L.ptr(p), L.ptr(p), 1, 1, 1, 2, 1.0, L.ptr(p), L.stream()) == -1
    # more tiles than partial sums of the fixed-order reduction: the caller keeps the three-pass form
    rc = lib.ufr_flow2_upsampled_loss_fast(L.ptr(p), 20.0, L.ptr(p), L.ptr(p), L.ptr(p), 8, 16 * 12, 16 * 12, 0, 1.0, L.ptr(p), L.stream())
    assert rc not in (0, -1) and b"partial sums" in lib.ufr_last_error()
