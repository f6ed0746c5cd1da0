"""`band_conv.native_training()`: a fine-tuning step of FlowNetC (training mode, every parameter trainable) whose convolutions --
forward, data gradient, weight and bias gradient -- run on the hand-written kernels instead of the vendor library.

One 64 x 128 pair, `synthetic_seed=0`; loss = sum over the five returned scales of the mean squared flow.  Gate (the one of
tests/test_models_gpu.py::test_flownets_trunk_on_the_engine_vs_float64): per parameter, the gradient's error against the float64
deep copy, relative to that parameter's max |grad|, is at most max(3 x the same error of torch's float32 step, 2e-6)."""
import copy
import warnings
from argparse import Namespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 2e-6


def _net():
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    net = fetch_model(Namespace(flownet="FlowNetC"), synthetic_seed=0).to(DEV)
    net.train()
    for p in net.parameters():
        p.requires_grad_(True)
    return net


def _loss(flows):
    assert isinstance(flows, tuple) and len(flows) == 5
    return sum((f ** 2).mean() for f in flows)


def _step(net, x1, x2):
    """One forward + backward through the public forward; {name: grad}."""
    net.zero_grad(set_to_none=True)
    _loss(net(x1, x2)).backward()
    return {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in net.named_parameters()}


def _step_float64(net, x1, x2):
    """The same step on a float64 deep copy (torch operators; `normalize_correctly` hands float32 on, so the copy's stem and head
    are called on the normalised frames cast to float64 -- the same values)."""
    n64 = copy.deepcopy(net).double()
    B = x1.shape[0]
    x = n64.normalize_correctly(torch.cat((x1, x2), 0)).double()
    _, c2, c3 = n64._stem_torch(x)
    _loss(n64._rest(c2[:B], c3[:B], c3[B:], None)).backward()
    return {n: p.grad.detach() for n, p in n64.named_parameters()}


def _errors(grads, truth):
    return {n: float((grads[n].double() - truth[n]).abs().max()) / float(truth[n].abs().max()) for n in truth}


def _assert_gate(mine, yardstick, truth, what):
    assert all(g is not None for g in mine.values()), [n for n, g in mine.items() if g is None]
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
def setup():
    """The network, the pair, and the two references every test shares: the float64 step and torch's float32 step (the default
    path outside the context)."""
    g = torch.Generator(device=DEV).manual_seed(0)
    x1 = torch.rand(1, 3, 64, 128, device=DEV, generator=g)
    x2 = torch.rand(1, 3, 64, 128, device=DEV, generator=g)
    net = _net()
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
            mine = _step(net, x1, x2)                                   # (a) completes
    assert L.VENDOR_FALLBACKS == counts, "native_training() counted a vendor fallback"          # (b)
    assert not [m for m in w if "hand-written engines" in str(m.message)]
    assert not L.native_training_on()
    _assert_gate(mine, torch32, truth, "native step")


def test_outside_the_context_nothing_changes(setup, monkeypatch):
    """The default: the same step still leaves the engines for torch operators, counts it, and computes what plain torch modules
    compute (the yardstick here is a replica of the forward on `act(conv(x))` module calls only)."""
    from understanding_flow_robustness_amd import _lib as L
    from understanding_flow_robustness_amd import band_conv
    from understanding_flow_robustness_amd.flownets import flownetc
    net, x1, x2, _, truth = setup
    key = ("FlowNetC", "module in training mode")
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
        m.setattr(flownetc, "conv_leaky", lambda x, seq, *a: seq[1](seq[0](x)))
        m.setattr(flownetc, "flow_head", lambda x, conv: F.conv2d(x, conv.weight, conv.bias, 1, 1))
        m.setattr(flownetc, "flow_upsample", lambda x, d: F.conv_transpose2d(x, d.weight, d.bias, 2, 1))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            plain = _step(net, x1, x2)
    _assert_gate(default, plain, truth, "default step")


def test_two_steps_with_an_update_in_between_see_the_new_weights(setup, monkeypatch):
    """The weight image is re-split on every call: after an SGD update the second step's gradients are those of the NEW weights."""
    from understanding_flow_robustness_amd.band_conv import native_training
    net0, x1, x2, _, _ = setup
    net = copy.deepcopy(net0)
    with native_training(), _VendorConvolutionsRaise(monkeypatch):
        first = _step(net, x1, x2)
    lr = 0.02 * min(float(p.detach().abs().max()) / float(first[n].abs().max()) for n, p in net.named_parameters())
    opt = torch.optim.SGD(net.parameters(), lr=lr)
    opt.step()
    with native_training(), _VendorConvolutionsRaise(monkeypatch):
        second = _step(net, x1, x2)
    assert all(not torch.equal(first[n], second[n]) for n in first), [n for n in first if torch.equal(first[n], second[n])]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch32 = _step(net, x1, x2)
    _assert_gate(second, torch32, _step_float64(net, x1, x2), "second native step")
