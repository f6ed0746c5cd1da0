"""csrc/igemm_wgrad.hip with a dilation, through `igemm.make_wgrad_launch(..., dilation=d)`: the weight (and bias) gradient of the
dilated convolutions of PWC-Net's context network, against `torch.nn.grad.conv2d_weight(..., stride, padding, dilation)` in float64.

The harness and the gate are those of tests/test_wgrad_gpu.py: the error relative to max |result| is at most max(3 x the same
error of torch's own float32 operator, 1e-5); operands at a chunk offset inside wider buffers filled with 7.0, guard bands around
dw and db, the split over pixels with None, 1, 3 and a count that does not divide the pixel count, two runs bit-identical,
accumulate exact."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 1e-5
GUARD = 64
SENTINEL = -1234.5

# (B, Cin, Cout, H, W, k, s, p, d)
SHAPES = [
    (2, 70, 130, 13, 21, 3, 1, 2, 2),      # ragged channels, odd sides
    (1, 128, 96, 16, 32, 3, 1, 8, 8),      # dc_conv4 on the level-2 grid of a 64 x 128 frame
    (1, 96, 64, 16, 32, 3, 1, 16, 16),     # dc_conv5: the dilation is the height, the outer tap rows lie in the padding
    (2, 40, 34, 9, 11, 5, 1, 4, 2),        # 25 taps
    (1, 81, 128, 1, 2, 3, 1, 1, 1),        # PWC-Net's level-6 grid: two pixels, most taps outside
]


def _planes_inside_wider_buffer(t, chunk0):
    """`t` [B,C,H,W] at chunk `chunk0` of a buffer with one more chunk behind it, every other element 7.0."""
    from understanding_flow_robustness_amd import igemm as ig
    B, Cn, H, W = t.shape
    p = ig.Planes(B, H, W, chunk0 + ig.pad32(Cn) // 32 + 1, DEV)
    p.t.fill_(7.0)
    return p.load_nchw(t.contiguous(), chunk0)


def _guarded(shape):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _rel(got, ref):
    return float((got.double() - ref).abs().max()) / float(ref.abs().max())


def _gate(got, ref64, torch32, what):
    e, e_t = _rel(got, ref64), _rel(torch32, ref64)
    print(f"{what}: kernel {e:.3e}, torch float32 {e_t:.3e} of the float64 result")
    assert e <= max(3 * e_t, FLOOR), f"{what}: kernel {e:.3e} vs torch float32 {e_t:.3e} of the float64 result"


def _check(xp, cin, gp, cout, k, s, p, extra, wshape, bias_n, M, ref_w, t32_w, ref_b, t32_b, tag, each=None):
    """tests/test_wgrad_gpu.py's `_check`; `extra` = the keyword arguments under test (dilation / transposed), `each(dw)` a further
    assertion on every result."""
    from understanding_flow_robustness_amd import igemm as ig
    nondiv = next(q for q in (7, 5, 11, 13) if M % q)
    first = None
    for splitm in (None, 1, 3, nondiv):
        wbuf, dw = _guarded(wshape)
        bbuf, db = _guarded((bias_n,))
        launch = ig.make_wgrad_launch(xp, 1, cin, gp, 2, cout, k, s, p, dw=dw, db=db, splitm=splitm, **extra)
        launch()
        got_w, got_b = dw.clone(), db.clone()
        _gate(got_w, ref_w, t32_w, f"{tag} dw splitm={splitm}")
        _gate(got_b, ref_b, t32_b, f"{tag} db splitm={splitm}")
        assert _guards_intact(wbuf) and _guards_intact(bbuf), f"{tag} splitm={splitm}: a guard band was written"
        if each is not None:
            each(got_w, f"{tag} splitm={splitm}")
        dw.fill_(SENTINEL)
        db.fill_(SENTINEL)
        launch()                                                       # the same launch again: bit-identical
        assert torch.equal(dw, got_w) and torch.equal(db, got_b), f"{tag} splitm={splitm}: two runs differ"
        if splitm == 3:
            first = (got_w, got_b)
    # accumulate adds the complete sum once onto what is there
    g = torch.Generator(device=DEV).manual_seed(5)
    wbuf, dw = _guarded(wshape)
    bbuf, db = _guarded((bias_n,))
    pre_w = torch.randn(wshape, device=DEV, generator=g)
    pre_b = torch.randn(bias_n, device=DEV, generator=g)
    dw.copy_(pre_w)
    db.copy_(pre_b)
    ig.make_wgrad_launch(xp, 1, cin, gp, 2, cout, k, s, p, dw=dw, db=db, accumulate=True, splitm=3, **extra)()
    assert torch.equal(dw, pre_w + first[0]) and torch.equal(db, pre_b + first[1]), f"{tag}: accumulate is not prefill + result"
    assert _guards_intact(wbuf) and _guards_intact(bbuf)
    wbuf, dw = _guarded(wshape)                                         # and without a split (the main kernel adds)
    dw.copy_(pre_w)
    one = torch.empty(wshape, device=DEV)
    ig.make_wgrad_launch(xp, 1, cin, gp, 2, cout, k, s, p, dw=one, splitm=1, **extra)()
    ig.make_wgrad_launch(xp, 1, cin, gp, 2, cout, k, s, p, dw=dw, accumulate=True, splitm=1, **extra)()
    assert torch.equal(dw, pre_w + one) and _guards_intact(wbuf), f"{tag}: accumulate without a split"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dilated_weight_gradient_against_float64(shape):
    B, cin, cout, H, W, k, s, p, d = shape
    g = torch.Generator(device=DEV).manual_seed(1234)
    span = (k - 1) * d + 1
    Ho, Wo = (H + 2 * p - span) // s + 1, (W + 2 * p - span) // s + 1
    x = torch.randn(B, cin, H, W, device=DEV, generator=g)
    gy = torch.randn(B, cout, Ho, Wo, device=DEV, generator=g)
    wshape = (cout, cin, k, k)
    ref_w = torch.nn.grad.conv2d_weight(x.double(), wshape, gy.double(), s, p, d)
    t32_w = torch.nn.grad.conv2d_weight(x, wshape, gy, s, p, d)
    ref_b, t32_b = gy.double().sum((0, 2, 3)), gy.sum((0, 2, 3))
    xp, gp = _planes_inside_wider_buffer(x, 1), _planes_inside_wider_buffer(gy, 2)
    each = None
    if d >= H and p == d and k == 3:
        # every off-centre tap ROW reads rows y - d or y + d of a frame of H <= d rows: all padding.  Zeros are staged, never 7.0
        # and never a neighbouring image's rows: the result is exactly zero, not merely small
        assert bool((ref_w[:, :, 0, :] == 0).all()) and bool((ref_w[:, :, 2, :] == 0).all())

        def each(dw, what):
            assert bool((dw[:, :, 0, :] == 0).all()) and bool((dw[:, :, 2, :] == 0).all()), f"{what}: a tap row outside the frame is not 0"
            assert float(dw[:, :, 1, :].abs().max()) > 0
    _check(xp, cin, gp, cout, k, s, p, dict(dilation=d), wshape, cout, B * Ho * Wo, ref_w, t32_w, ref_b, t32_b, str(shape), each)


def test_dilation_one_through_the_new_argument_is_the_call_without_it():
    from understanding_flow_robustness_amd import igemm as ig
    B, cin, cout, H, W, k, s, p = 2, 70, 130, 13, 21, 3, 2, 1
    g = torch.Generator(device=DEV).manual_seed(99)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = torch.randn(B, cin, H, W, device=DEV, generator=g)
    gy = torch.randn(B, cout, Ho, Wo, device=DEV, generator=g)
    xp, gp = _planes_inside_wider_buffer(x, 1), _planes_inside_wider_buffer(gy, 2)
    for splitm in (None, 1, 3):
        res = []
        for extra in ({}, dict(dilation=1), dict(dilation=(1, 1))):
            dw, db = torch.empty(cout, cin, k, k, device=DEV), torch.empty(cout, device=DEV)
            ig.make_wgrad_launch(xp, 1, cin, gp, 2, cout, k, s, p, dw=dw, db=db, splitm=splitm, **extra)()
            res.append((dw, db))
        for dw, db in res[1:]:
            assert torch.equal(dw, res[0][0]) and torch.equal(db, res[0][1]), f"splitm={splitm}"


def test_a_transposed_layer_refuses_a_dilation_and_a_dilation_below_one_is_refused():
    from understanding_flow_robustness_amd import igemm as ig
    x, gy = torch.zeros(1, 32, 4, 8, device=DEV), torch.zeros(1, 2, 8, 16, device=DEV)
    xp, gp = ig.Planes(1, 4, 8, 1, DEV).load_nchw(x), ig.Planes(1, 8, 16, 1, DEV).load_nchw(gy)
    dw = torch.empty(32, 2, 4, 4, device=DEV)
    with pytest.raises(RuntimeError, match="transposed"):
        ig.make_wgrad_launch(xp, 0, 32, gp, 0, 2, 4, 2, 1, transposed=True, dw=dw, dilation=2)
    ig.make_wgrad_launch(xp, 0, 32, gp, 0, 2, 4, 2, 1, transposed=True, dw=dw, dilation=1)()
    with pytest.raises(RuntimeError, match="dilation"):
        ig.make_wgrad_launch(xp, 0, 32, xp, 0, 32, 3, 1, 1, dw=torch.empty(32, 32, 3, 3, device=DEV), dilation=0)


def test_upfeat_weight_and_bias_gradient():
    """`upfeat3` = ConvTranspose2d(529, 2, 4, 2, 1) on a 1 x 4 x 8 grid: the transposed check of tests/test_wgrad_gpu.py at the
    extreme channel ratio (17 chunks against two channels)."""
    B, cin, cout, H, W = 1, 529, 2, 4, 8
    g = torch.Generator(device=DEV).manual_seed(4321)
    x = torch.randn(B, cin, H, W, device=DEV, generator=g)
    gy = torch.randn(B, cout, 2 * H, 2 * W, device=DEV, generator=g)
    wshape = (cin, cout, 4, 4)

    def autograd_weight_gradient(dtype):
        w0 = torch.zeros(wshape, device=DEV, dtype=dtype, requires_grad=True)
        (gw,) = torch.autograd.grad(F.conv_transpose2d(x.to(dtype), w0, None, 2, 1), w0, gy.to(dtype))
        return gw

    ref_w, t32_w = autograd_weight_gradient(torch.float64), autograd_weight_gradient(torch.float32)
    ref_b, t32_b = gy.double().sum((0, 2, 3)), gy.sum((0, 2, 3))
    xp, gp = _planes_inside_wider_buffer(x, 1), _planes_inside_wider_buffer(gy, 2)
    _check(xp, cin, gp, cout, 4, 2, 1, dict(transposed=True), wshape, cout, B * H * W, ref_w, t32_w, ref_b, t32_b, "upfeat3")
