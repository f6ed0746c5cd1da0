"""`band_conv.native_training()` on PWC-Net: a fine-tuning step (training mode, every parameter trainable) whose convolutions --
the pyramid, the DenseNet decoder, `predict_flow*`, `deconv*`, `upfeat*` and the dilated context network; forward, data gradient,
weight and bias gradient -- run on the hand-written kernels instead of the vendor library.

`synthetic_seed=0`; loss = sum over the five returned scales of the mean squared flow; two sizes: 2 pairs of 64 x 128 (the doubled
batch of adversarial training) and 1 pair of 128 x 192 (dilation 16 reaches inside the 32 x 48 grid).  Gate (the one of
tests/test_native_training_gpu.py): per parameter, the gradient's error against the float64 deep copy, relative to that
parameter's max |grad|, is at most max(3 x the same error of torch's float32 step, 2e-6).  The synthetic flows are about a
quarter of a pixel, so no warp sample sits near a cell border: the piecewise-warp allowance of tests/test_pwc_engine_gpu.py is
deliberately not used.  `deconv2` is built by the reference and never used: its two parameters are the only ones without a
gradient, in every leg."""
import copy
import warnings
from argparse import Namespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 2e-6
UNUSED = {"deconv2.weight", "deconv2.bias"}
SIZES = [(2, 64, 128), (1, 128, 192)]


def _net():
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    net = fetch_model(Namespace(flownet="PWCNet"), synthetic_seed=0).to(DEV)
    net.train()
    for p in net.parameters():
        p.requires_grad_(True)
    return net


def _loss(flows):
    assert isinstance(flows, tuple) and len(flows) == 5
    return sum((f ** 2).mean() for f in flows)


def _step(net, x1, x2):
    """One forward + backward through the public forward; {name: grad or None}."""
    net.zero_grad(set_to_none=True)
    _loss(net(x1, x2)).backward()
    return {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in net.named_parameters()}


def _step_float64(net, x1, x2):
    """The same step on a float64 deep copy (torch operators throughout: nothing native takes float64)."""
    return _step(copy.deepcopy(net).double(), x1.double(), x2.double())


def _errors(grads, truth):
    return {n: float((grads[n].double() - truth[n]).abs().max()) / float(truth[n].abs().max()) for n in truth if truth[n] is not None}


def _assert_gate(mine, yardstick, truth, what):
    for leg, grads in (("step under test", mine), ("torch float32", yardstick), ("float64", truth)):
        none = {n for n, g in grads.items() if g is None}
        assert none == UNUSED, f"{what}, {leg}: parameters without a gradient {sorted(none)} (only deconv2 is unused)"
    e, e_t = _errors(mine, truth), _errors(yardstick, truth)
    worst = max(e, key=lambda n: e[n] / max(3 * e_t[n], FLOOR))
    print(f"{what}: worst parameter {worst}: {e[worst]:.3e} vs torch float32 {e_t[worst]:.3e} of the float64 gradient")
    bad = {n: (e[n], e_t[n]) for n in e if not e[n] <= max(3 * e_t[n], FLOOR)}
    assert not bad, f"{what}: (error, torch float32's error) of the float64 gradient: {bad}"


class _VendorConvolutionsRaise:
    """F.conv2d / F.conv_transpose2d raise: any route to the vendor library fails the step."""

    def __init__(self, monkeypatch):
        self.mp = monkeypatch

    def __enter__(self):
        self.ctx = self.mp.context()
        m = self.ctx.__enter__()

        def refuse(*a, **k):
            raise AssertionError("a vendor convolution ran inside native_training()")
        m.setattr(torch.nn.functional, "conv2d", refuse)
        m.setattr(torch.nn.functional, "conv_transpose2d", refuse)

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc)


@pytest.fixture(scope="module")
def net():
    return _net()


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: "x".join(map(str, s)))
def setup(request, net):
    """The pairs of one size and the two references every test shares: the float64 step and torch's float32 step (the default
    path outside the context)."""
    B, H, W = request.param
    g = torch.Generator(device=DEV).manual_seed(0)
    x1 = torch.rand(B, 3, H, W, device=DEV, generator=g)
    x2 = torch.rand(B, 3, H, W, device=DEV, generator=g)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch32 = _step(net, x1, x2)
    truth = _step_float64(net, x1, x2)
    return net, x1, x2, torch32, truth


def test_a_native_step_matches_the_float64_gradients_without_any_vendor_convolution(setup, monkeypatch):
    from understanding_flow_robustness_amd import _lib as L
    from understanding_flow_robustness_amd.band_conv import native_training
    net, x1, x2, torch32, truth = setup
    counts = dict(L.VENDOR_FALLBACKS)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with native_training(), _VendorConvolutionsRaise(monkeypatch):
            mine = _step(net, x1, x2)                                   # completes: dc_conv2 .. dc_conv5 and upfeat* are served
    assert L.VENDOR_FALLBACKS == counts, "native_training() counted a vendor fallback"
    assert not [m for m in w if "hand-written engines" in str(m.message)]
    assert not L.native_training_on()
    _assert_gate(mine, torch32, truth, f"native step {tuple(x1.shape)}")


def test_outside_the_context_nothing_changes(setup, monkeypatch):
    """The default: the same step still leaves the engines for torch operators, counts it, and computes what plain torch modules
    compute (the yardstick is a replica of the forward on `act(conv(x))` / `F.conv_transpose2d` calls only) -- `upfeat*` as a
    `FlowUpsample` included."""
    from understanding_flow_robustness_amd import _lib as L
    from understanding_flow_robustness_amd import band_conv
    from understanding_flow_robustness_amd.flownets import pwcnet
    net, x1, x2, _, truth = setup
    key = ("PWCDCNet", "module in training mode")
    before = L.VENDOR_FALLBACKS.get(key, 0)

    def refuse(*a, **k):
        raise AssertionError("the native training path ran outside native_training()")
    with monkeypatch.context() as m:
        m.setattr(band_conv._NativeTrainConv, "apply", refuse)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            default = _step(net, x1, x2)
    assert L.VENDOR_FALLBACKS.get(key, 0) > before
    with monkeypatch.context() as m:                                    # plain torch modules in place of the three helpers
        m.setattr(pwcnet, "conv_leaky", lambda x, seq, *a: seq[1](seq[0](x)))
        m.setattr(band_conv, "flow_head", lambda x, conv: F.conv2d(x, conv.weight, conv.bias, 1, 1))
        m.setattr(band_conv, "flow_upsample", lambda x, d: F.conv_transpose2d(x, d.weight, d.bias, 2, 1))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            plain = _step(net, x1, x2)
    _assert_gate(default, plain, truth, f"default step {tuple(x1.shape)}")
    # upfeat outside the context is the module's own call, bit for bit
    up = net.upfeat3
    x = torch.randn(1, up.in_channels, 4, 8, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    with torch.no_grad():
        assert torch.equal(up(x), torch.nn.ConvTranspose2d.forward(up, x))


def _rel(got, ref):
    return float((got.double() - ref).abs().max()) / float(ref.abs().max())


def test_the_dilated_block_on_its_own(net, monkeypatch):
    """`conv_leaky` on dc_conv5 = Conv2d(96, 64, 3, 1, 16, 16) + LeakyReLU(0.1): forward, input, weight and bias gradient inside the
    gate on a (1, 96, 16, 32) input -- the dilation is the height of the grid."""
    from understanding_flow_robustness_amd.band_conv import conv_leaky, native_training
    seq = net.dc_conv5
    assert seq[0].dilation == (16, 16) and seq[0].padding == (16, 16)
    g = torch.Generator(device=DEV).manual_seed(16)
    x = torch.randn(1, 96, 16, 32, device=DEV, generator=g)
    gy = torch.randn(1, 64, 16, 32, device=DEV, generator=g)

    def run(block, dtype, native):
        block.zero_grad(set_to_none=True)
        xi = x.detach().clone().to(dtype).requires_grad_(True)           # a leaf of its own: `.grad` must not add up across the runs
        if native:
            with native_training(), _VendorConvolutionsRaise(monkeypatch):
                y = conv_leaky(xi, block)
                y.backward(gy.to(dtype))
        else:
            y = block(xi)
            y.backward(gy.to(dtype))
        return [t.detach().clone() for t in (y, xi.grad, block[0].weight.grad, block[0].bias.grad)]

    truth = run(copy.deepcopy(seq).double(), torch.float64, False)
    torch32 = run(seq, torch.float32, False)
    mine = run(seq, torch.float32, True)
    seq.zero_grad(set_to_none=True)
    for name, a, b, t in zip(("forward", "gx", "gw", "gb"), mine, torch32, truth):
        e, e_t = _rel(a, t), _rel(b, t)
        print(f"dc_conv5 {name}: native {e:.3e}, torch float32 {e_t:.3e} of the float64 result")
        assert e <= max(3 * e_t, FLOOR), f"dc_conv5 {name}: native {e:.3e} vs torch float32 {e_t:.3e}"
    # the outer tap rows only ever meet the padding
    assert bool((mine[2][:, :, 0, :] == 0).all()) and bool((mine[2][:, :, 2, :] == 0).all())


def test_stride_two_with_a_dilation_is_still_refused():
    from understanding_flow_robustness_amd.band_conv import conv_leaky, native_training
    block = torch.nn.Sequential(torch.nn.Conv2d(32, 32, 3, 2, 2, 2), torch.nn.LeakyReLU(0.1)).to(DEV)
    x = torch.randn(1, 32, 16, 32, device=DEV)
    with native_training():
        with pytest.raises(NotImplementedError, match="dilation"):
            conv_leaky(x, block)
        rect = torch.nn.Sequential(torch.nn.Conv2d(32, 32, 3, 1, (2, 4), (2, 4)), torch.nn.LeakyReLU(0.1)).to(DEV)
        with pytest.raises(NotImplementedError):
            conv_leaky(x, rect)                                           # a dilation that is not square


def test_the_attack_sees_the_updated_weights(net, monkeypatch):
    """One native step, one SGD update, then the frozen eval-mode forward the attack runs: the engines (their weight stamps are
    the parameters' (data_ptr, _version) tuples) must serve the NEW weights -- the forward differs from the one before the update
    and agrees with the UFR_ENGINE=0 forward of the updated network, both against its float64 forward (the rule of
    tests/test_pwc_engine_gpu.py: engine <= max(3 x torch float32, 1e-5))."""
    from understanding_flow_robustness_amd.band_conv import native_training
    from understanding_flow_robustness_amd.flownets.utils_model import predict_flow
    args = Namespace(flownet="PWCNet")
    net = copy.deepcopy(net)
    g = torch.Generator(device=DEV).manual_seed(0)
    x1 = torch.rand(1, 3, 64, 128, device=DEV, generator=g)
    x2 = torch.rand(1, 3, 64, 128, device=DEV, generator=g)

    def frozen_forward():
        net.eval()
        for p in net.parameters():
            p.requires_grad_(False)
        with torch.no_grad():
            return predict_flow(net, None, x1, x2, args).clone()

    monkeypatch.setenv("UFR_ENGINE", "1")
    before = frozen_forward()
    assert net.__dict__.get("_ufr_head_engines"), "the frozen forward did not run on the engine"
    net.train()
    for p in net.parameters():
        p.requires_grad_(True)
    with native_training(), _VendorConvolutionsRaise(monkeypatch):
        first = _step(net, x1, x2)
    lr = 0.02 * min(float(p.detach().abs().max()) / float(first[n].abs().max()) for n, p in net.named_parameters()
                    if first[n] is not None)
    torch.optim.SGD(net.parameters(), lr=lr).step()
    after = frozen_forward()
    assert not torch.equal(after, before), "the engines served the weights from before the update"
    monkeypatch.setenv("UFR_ENGINE", "0")
    plain = frozen_forward()
    with torch.no_grad():
        truth = copy.deepcopy(net).double()(x1.double(), x2.double())
    e, e_t = _rel(after, truth), _rel(plain, truth)
    print(f"updated network: engine forward {e:.3e}, UFR_ENGINE=0 forward {e_t:.3e} of the float64 flow; "
          f"moved {_rel(after, before.double()):.3e} of the flow by the update")
    assert e <= max(3 * e_t, 1e-5), f"engine forward {e:.3e} vs torch float32 {e_t:.3e} of the float64 flow"
