"""csrc/igemm_wgrad.hip through `igemm.make_wgrad_launch`: the weight (and bias) gradient of a convolution from plane operands,
against `torch.nn.grad.conv2d_weight` evaluated in float64.

Gate: the error relative to max |result| is at most max(3 x the same error of torch's own float32 operator, 1e-5) -- the 3 x rule
of tests/test_models_gpu.py (engine against torch float32, both measured on the float64 result) with the floor of
tests/test_igemm_gpu.py's TOL.  The operands sit at a chunk offset inside wider buffers filled with 7.0 (which must not reach the
result), dw lies between guard bands (which must stay as they were), the split over pixels runs with 1, 3 and a slice count that
does not divide the pixel count (each inside the gate, two runs bit-identical), and accumulate adds exactly."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 1e-5
GUARD = 64
SENTINEL = -1234.5

# (B, Cin, Cout, H, W, k, s, p): the smallest shapes at which the kernel can still go wrong
SHAPES = [
    (2, 96, 160, 24, 40, 3, 1, 1),     # several chunks on both sides
    (3, 70, 130, 13, 21, 3, 2, 1),     # ragged channels, odd sizes, M not a tile multiple
    (1, 64, 128, 20, 36, 5, 2, 2),     # 25 taps
    (2, 3, 64, 32, 48, 7, 2, 3),       # conv1: 49 taps, C = 3
    (2, 256, 32, 12, 20, 1, 1, 0),     # conv_redir
    (1, 194, 2, 16, 24, 3, 1, 1),      # predict_flow: N = 2
]
TRANSPOSED = [(2, 96, 160, 12, 20), (1, 2, 2, 12, 20)]


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


def _check(xp, cin, gp, cout, k, s, p, transposed, wshape, bias_n, M, ref_w, t32_w, ref_b, t32_b, tag):
    from understanding_flow_robustness_amd import igemm as ig
    nondiv = next(q for q in (7, 5, 11, 13) if M % q)
    first = None
    for splitm in (None, 1, 3, nondiv):
        wbuf, dw = _guarded(wshape)
        bbuf, db = _guarded((bias_n,))
        launch = ig.make_wgrad_launch(xp, 1, cin, gp, 2, cout, k, s, p, transposed=transposed, dw=dw, db=db, splitm=splitm)
        launch()
        got_w, got_b = dw.clone(), db.clone()
        _gate(got_w, ref_w, t32_w, f"{tag} dw splitm={splitm}")
        _gate(got_b, ref_b, t32_b, f"{tag} db splitm={splitm}")
        assert _guards_intact(wbuf) and _guards_intact(bbuf), f"{tag} splitm={splitm}: a guard band was written"
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
    ig.make_wgrad_launch(xp, 1, cin, gp, 2, cout, k, s, p, transposed=transposed, dw=dw, db=db, accumulate=True, splitm=3)()
    assert torch.equal(dw, pre_w + first[0]) and torch.equal(db, pre_b + first[1]), f"{tag}: accumulate is not prefill + result"
    assert _guards_intact(wbuf) and _guards_intact(bbuf)
    wbuf, dw = _guarded(wshape)                                         # and without a split (the main kernel adds)
    dw.copy_(pre_w)
    one = torch.empty(wshape, device=DEV)
    ig.make_wgrad_launch(xp, 1, cin, gp, 2, cout, k, s, p, transposed=transposed, dw=one, splitm=1)()
    ig.make_wgrad_launch(xp, 1, cin, gp, 2, cout, k, s, p, transposed=transposed, dw=dw, accumulate=True, splitm=1)()
    assert torch.equal(dw, pre_w + one) and _guards_intact(wbuf), f"{tag}: accumulate without a split"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_weight_gradient_against_float64(shape):
    B, cin, cout, H, W, k, s, p = shape
    g = torch.Generator(device=DEV).manual_seed(1234)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = torch.randn(B, cin, H, W, device=DEV, generator=g)
    gy = torch.randn(B, cout, Ho, Wo, device=DEV, generator=g)
    wshape = (cout, cin, k, k)
    ref_w = torch.nn.grad.conv2d_weight(x.double(), wshape, gy.double(), s, p)
    t32_w = torch.nn.grad.conv2d_weight(x, wshape, gy, s, p)
    ref_b, t32_b = gy.double().sum((0, 2, 3)), gy.sum((0, 2, 3))
    xp, gp = _planes_inside_wider_buffer(x, 1), _planes_inside_wider_buffer(gy, 2)
    _check(xp, cin, gp, cout, k, s, p, False, wshape, cout, B * Ho * Wo, ref_w, t32_w, ref_b, t32_b, str(shape))


@pytest.mark.parametrize("shape", TRANSPOSED, ids=lambda s: "x".join(map(str, s)))
def test_transposed_weight_gradient_is_the_same_call_with_the_operands_swapped(shape):
    """ConvTranspose2d(Cin, Cout, 4, 2, 1) against the float64 autograd weight gradient of `F.conv_transpose2d`; the result is
    torch's [Cin][Cout][4][4] layout, the bias gradient the sum of the fine gradient."""
    B, cin, cout, H, W = shape
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
    # the reduction runs over the coarse grid (the swapped call's gy operand is the layer's input)
    _check(xp, cin, gp, cout, 4, 2, 1, True, wshape, cout, B * H * W, ref_w, t32_w, ref_b, t32_b, "transposed " + str(shape))


def test_the_products_stack_does_not_reach_the_weight_gradient():
    """`with igemm.products(1):` (RAFT's reduced precision) changes the launches built inside; a weight gradient built inside is
    still the six-product form."""
    from understanding_flow_robustness_amd import igemm as ig
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(1, 32, 8, 12, device=DEV, generator=g)
    gy = torch.randn(1, 32, 8, 12, device=DEV, generator=g)
    xp, gp = ig.Planes(1, 8, 12, 1, DEV).load_nchw(x), ig.Planes(1, 8, 12, 1, DEV).load_nchw(gy)
    a, b = torch.empty(32, 32, 3, 3, device=DEV), torch.empty(32, 32, 3, 3, device=DEV)
    ig.make_wgrad_launch(xp, 0, 32, gp, 0, 32, 3, 1, 1, dw=a, splitm=1)()
    with ig.products(1):
        launch = ig.make_wgrad_launch(xp, 0, 32, gp, 0, 32, 3, 1, 1, dw=b, splitm=1)
    assert launch.desc.products == 6
    launch()
    assert torch.equal(a, b)
