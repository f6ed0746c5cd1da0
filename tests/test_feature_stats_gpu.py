"""GPU suite of the statistics kernel (csrc/feature_stats.hip): per-image, per-channel float64 sums of plane chunk ranges and of
NCHW float32 tensors against `planes.to_nchw().double().sum((2, 3))`.

Bound, per entry: |got - want| <= 2 n 2^-53 sum|x| with n the pixels per image.  Both sides add the same n exactly
representable values in float64, in different orders; a float64 sum of n terms is off by at most (n - 1) 2^-53 sum|x| (to
first order), so two of them differ by at most twice that."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -53
SLOPE = 0.1


def _L():
    from understanding_flow_robustness_amd import _lib as L
    return L


def make_planes(B, H, W, chunks, seed):
    """A planes buffer whose every lane holds mixed-sign data (the padded lanes of a narrower segment included)."""
    from understanding_flow_robustness_amd import igemm as ig
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, chunks * 32, H, W, generator=g) * torch.rand(B, chunks * 32, 1, 1, generator=g) * 3).to(DEV)
    return ig.Planes(B, H, W, chunks, DEV).load_nchw(x, 0)


def seg(src, chunk0, channels, image0=0, B=None, unleaky=0.0, out_col=0):
    L = _L()
    s = L.FeatureStatsSeg()
    planes = not torch.is_tensor(src)
    tens = src.t if planes else src
    s.src, s.kind = tens.data_ptr(), 0 if planes else 1
    s.plane_stride = src.plane_stride if planes else tens.numel()
    s.pixels, s.images = (src.H * src.W, src.B) if planes else (tens.shape[2] * tens.shape[3], tens.shape[0])
    s.image0, s.B, s.chunk0, s.channels = image0, (s.images - image0 if B is None else B), chunk0, channels
    s.unleaky, s.out_col = unleaky, out_col
    return s


def run(segs, rows, cols, stride=None, fill=0.0):
    L = _L()
    lib = L.lib()
    arr = (L.FeatureStatsSeg * len(segs))(*segs)
    need = lib.ufr_feature_stats_workspace_doubles(arr, len(segs))
    assert need > 0
    ws = torch.full((need,), float("nan"), dtype=torch.float64, device=DEV)
    stride = cols if stride is None else stride
    out = torch.full((rows, stride), fill, dtype=torch.float64, device=DEV)
    L.check(lib.ufr_feature_stats(arr, len(segs), L.ptr(ws), need, L.ptr(out), rows, cols, stride, L.stream()), "feature stats")
    torch.cuda.synchronize()
    return out


def want_of(x, unleaky=0.0):
    """(sums, sums of magnitudes) of an NCHW float32 tensor in float64, the un-leaky rule applied first."""
    if unleaky:
        from understanding_flow_robustness_amd.flownetc_engine import _unleaky
        x = _unleaky(x, unleaky)
    return x.double().sum((2, 3)), x.double().abs().sum((2, 3))


def check(got, want, mag, n, what):
    bound = 2.0 * n * U * mag
    err = (got - want).abs()
    assert bool((err <= bound).all()), f"{what}: max err {float(err.max()):.3e}, bound there {float(bound.flatten()[err.argmax()]):.3e}"


# one slab; 3 slabs with a ragged last one (4620 = 2 x 1600 + 1420); the slab cap (266,240 pixels > 128 x 2048: 2112-pixel slabs)
GRIDS = [(2, 1, 2), (2, 8, 16), (2, 16, 24), (1, 3, 5), (2, 70, 66), (1, 520, 512)]


@pytest.mark.parametrize("B,H,W", GRIDS)
def test_plane_sums_vs_float64(B, H, W):
    chunks = 2 if H * W > 4096 else 5
    P = make_planes(B, H, W, chunks, seed=H * W)
    n = H * W
    # whole buffer; a range with chunk0 > 0; 2 channels of a 32-lane chunk (the other 30 lanes hold data that must not count)
    cases = [(0, chunks * 32), (1, 32 * (chunks - 1)), (chunks - 1, 2), (0, 33)]
    for c0, cn in cases:
        got = run([seg(P, c0, cn)], B, cn)
        want, mag = want_of(P.to_nchw(cn, c0))
        check(got, want, mag, n, f"chunk0={c0} channels={cn}")
        assert torch.equal(got, run([seg(P, c0, cn)], B, cn)), "two runs differ"


@pytest.mark.parametrize("B,H,W", [(2, 8, 16), (1, 3, 5), (2, 40, 52)])
def test_unleaky_sums_the_values_in_front_of_the_activation(B, H, W):
    from understanding_flow_robustness_amd import igemm as ig
    g = torch.Generator().manual_seed(H)
    y = torch.randn(B, 70, H, W, generator=g).to(DEV)                       # in front of the LeakyReLU: mixed signs
    P = ig.Planes(B, H, W, 4, DEV).load_nchw(y, 1, slope=SLOPE)             # the planes hold LeakyReLU(y)
    got = run([seg(P, 1, 70, unleaky=SLOPE)], B, 70)
    held = P.to_nchw(70, 1)
    want, mag = want_of(held, SLOPE)
    check(got, want, mag, H * W, "unleaky")
    assert bool((held < 0).any()) and not torch.equal(want, held.double().sum((2, 3)))
    # the rule inverts the activation exactly: what it sums is what was loaded
    from understanding_flow_robustness_amd.flownetc_engine import _unleaky
    assert torch.equal(ig.Planes(B, H, W, 4, DEV).load_nchw(_unleaky(held, SLOPE), 1, slope=SLOPE).t[:, 1:4], P.t[:, 1:4])


def test_second_half_of_a_stacked_batch():
    P = make_planes(4, 8, 16, 2, seed=3)                                    # 2B images: first frames, then second frames
    full = P.to_nchw(64, 0)
    for image0 in (0, 2):
        got = run([seg(P, 0, 64, image0=image0, B=2)], 2, 64)
        want, mag = want_of(full[image0:image0 + 2])
        check(got, want, mag, 128, f"image0={image0}")


@pytest.mark.parametrize("B,H,W", [(2, 1, 2), (2, 16, 24), (1, 40, 52)])
def test_nchw_form(B, H, W):
    g = torch.Generator().manual_seed(W)
    flow = torch.randn(B, 2, H, W, generator=g).to(DEV)
    wide = torch.randn(B, 5, H, W, generator=g).to(DEV)
    got = run([seg(flow, 0, 2), seg(wide, 3, 2, out_col=2)], B, 4)
    want, mag = want_of(torch.cat((flow, wide[:, 3:5]), 1))
    check(got, want, mag, H * W, "nchw")
    assert torch.equal(got, run([seg(flow, 0, 2), seg(wide, 3, 2, out_col=2)], B, 4))


def test_segments_of_one_forward_land_in_one_matrix_and_leave_their_neighbours_alone():
    """Several segments of different buffers in one call, at column offsets of a result matrix whose row stride is wider than
    its columns: every column no segment owns keeps its sentinel."""
    P1, P2 = make_planes(2, 8, 16, 3, seed=5), make_planes(4, 40, 52, 2, seed=6)
    flow = torch.randn(2, 2, 4, 8, generator=torch.Generator().manual_seed(7)).to(DEV)
    segs = [seg(P1, 1, 40, out_col=3), seg(P2, 0, 2, image0=2, B=2, out_col=50), seg(flow, 0, 2, out_col=60),
            seg(P2, 1, 32, image0=0, B=2, unleaky=SLOPE, out_col=64)]
    cols, stride, sentinel = 100, 104, -7.25
    out = run(segs, 2, cols, stride, fill=sentinel)
    owned = torch.zeros(stride, dtype=torch.bool)
    parts = [(3, P1.to_nchw(40, 1), 0.0, 128), (50, P2.to_nchw(2, 0)[2:4], 0.0, 2080), (60, flow, 0.0, 32),
             (64, P2.to_nchw(32, 1)[0:2], SLOPE, 2080)]
    for col, x, unleaky, n in parts:
        want, mag = want_of(x, unleaky)
        check(out[:, col:col + x.shape[1]], want, mag, n, f"columns from {col}")
        owned[col:col + x.shape[1]] = True
    assert bool((out[:, ~owned.to(DEV)] == sentinel).all()), "a column outside every segment was written"
    assert torch.equal(out, run(segs, 2, cols, stride, fill=sentinel)), "two runs differ"
