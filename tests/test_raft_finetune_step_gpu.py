"""`training.finetune_step` on RAFT with the fused loss (`fused_raft_loss=True`, the default): `synthetic_seed=0`, training mode with
`freeze_bn`, one 64 x 96 pair, `fetch_optimizer`'s ClippedAdamW.

  - the step completes with `RAFT.upsample_flow` made to raise: no full-resolution prediction is built;
  - the parameter gradients of forward + loss + backward agree between the fused and the unfused loss.  The forward is the same code
    in both legs and the backward is linear in the gradients the loss injects, so the difference is the rounding of the loss
    gradients plus the run-to-run noise of the vendor library's weight gradients.  Per parameter tensor: the largest absolute
    difference relative to the tensor's largest gradient magnitude; GATE = 8 x the larger of the measured unfused run-to-run
    difference and the measured fused-to-unfused difference, rounded up to a power of two and never above 1e-3.  All legs run with
    the vendor library's deterministic algorithms (`torch.backends.cudnn.deterministic`): with its default choice the feature
    encoder's weight gradients come out in one of several states, 3e-6, 8.4e-4 or 2.4e-3 apart from one unfused run to the next,
    which drowns what is compared.  Measured on the MI355X (profiles/raft_train_loss_gate.txt): two unfused runs differ by 0,
    fused and unfused by 1.231e-6 (fnet.conv1.weight, the same figure in every pair of runs); 8 x 1.231e-6 = 9.85e-6 rounds up to
    GATE = 2**-16.  The same comparison between gamma 0.8 and 0.85 (0.32) must exceed it.  The 15 encoder biases whose gradient
    is zero by construction (`_without_signal`) have no magnitude to be relative to -- what the backward leaves there is rounding,
    1e-8 of the largest gradient, and two legs differ by 1 .. 2 times its size -- and are held to that rounding level instead;
  - `fused_raft_loss=False` is the former path: `upsample_flow` runs 12 times;
  - the model's forward with `lowres_predictions=True`: 12 pairs whose `upsampled()` is the default forward's list.  The training
    forward is not bit-reproducible on the device (two default forwards differ by ~2e-5 on flows of ~50), so the comparison is
    held to 8 x the difference of two default forwards, not to bit equality (that is tests/test_raft_train_loss_cpu.py)."""
import warnings
from argparse import Namespace

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
HYPER = dict(lr=1e-4, wdecay=1e-4, epsilon=1e-8, num_steps=100, clip=1.0, gamma=0.8, adv_train=True, iters=12)
GATE = 2.0 ** -16        # 8 x the measured 1.231e-6, rounded up to a power of two (profiles/raft_train_loss_gate.txt)


def _net():
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    net = fetch_model(Namespace(flownet="RAFT"), synthetic_seed=0).to(DEV)
    net.train()
    net.freeze_bn()
    for p in net.parameters():
        p.requires_grad_(True)
    return net


def _batch():
    g = torch.Generator(device=DEV).manual_seed(0)
    x1, x2 = torch.rand(1, 3, 64, 96, device=DEV, generator=g), torch.rand(1, 3, 64, 96, device=DEV, generator=g)
    flow = torch.randn(1, 2, 64, 96, device=DEV, generator=g) * 2.0
    valid = (torch.rand(1, 64, 96, device=DEV, generator=g) > 0.1).float()
    return x1, x2, flow, valid


@pytest.fixture(scope="module")
def net():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return _net()


def test_the_forward_returns_the_low_resolution_predictions(net):
    from understanding_flow_robustness_amd.flownets.raft import RaftPredictions
    x1, x2, _, _ = _batch()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net(x1 * 255.0, x2 * 255.0)                              # the vendor library has chosen its algorithms
        want, again = net(x1 * 255.0, x2 * 255.0), net(x1 * 255.0, x2 * 255.0)
        preds = net(x1 * 255.0, x2 * 255.0, lowres_predictions=True)
    assert isinstance(want, list) and isinstance(preds, RaftPredictions) and len(preds) == 12 == len(want)
    assert all(f.shape == (1, 2, 8, 12) and f.requires_grad and f.is_contiguous() for f in preds.flows)
    assert all(m.shape == (1, 576, 8, 12) and m.requires_grad and m.is_contiguous() for m in preds.masks)
    for i, (a, b, c) in enumerate(zip(preds.upsampled(), want, again)):
        assert a.shape == (1, 2, 64, 96) and a.requires_grad and torch.isfinite(a).all() and torch.isfinite(b).all()
        noise, diff, scale = float((c - b).abs().max()), float((a - b).abs().max()), float(b.abs().max())
        print(f"prediction {i}: default to default {noise:.3e}, low-resolution to default {diff:.3e}, largest flow {scale:.3e}")
        assert diff <= 8 * max(noise, 2.0 ** -22 * scale), f"prediction {i}: {diff:.3e} against a run-to-run difference of {noise:.3e}"


def test_the_step_builds_no_full_resolution_prediction(net, monkeypatch):
    import copy

    from understanding_flow_robustness_amd import training as T
    from understanding_flow_robustness_amd.flownets.raft import RAFT
    net = copy.deepcopy(net)
    args = Namespace(flownet="RAFT", **HYPER)
    opt, sched = T.fetch_optimizer(args, net)
    x1, x2, flow, valid = _batch()
    before = [p.detach().clone() for p in net.parameters()]

    def refuse(*a, **kw):
        raise AssertionError("upsample_flow ran inside the fused step")
    monkeypatch.setattr(RAFT, "upsample_flow", staticmethod(refuse))
    monkeypatch.setattr(T, "_sequence_loss_torch", refuse)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss, metrics = T.finetune_step(net, opt, sched, x1, x2, flow, valid, args)
    assert torch.isfinite(loss) and set(metrics) == {"epe", "1px", "3px", "5px"} and all(v == v for v in metrics.values())
    assert loss._ufr_host_value == pytest.approx(float(loss), rel=1e-6)
    assert any(not torch.equal(p, b) for p, b in zip(net.parameters(), before)), "the optimiser did not step"
    assert all(torch.isfinite(p).all() for p in net.parameters())


def test_the_unfused_step_is_the_former_path(net, monkeypatch):
    import copy

    from understanding_flow_robustness_amd import training as T
    from understanding_flow_robustness_amd.flownets.raft import RAFT
    net = copy.deepcopy(net)
    args = Namespace(flownet="RAFT", **HYPER)
    opt, sched = T.fetch_optimizer(args, net)
    x1, x2, flow, valid = _batch()
    calls, inner = [0], RAFT.upsample_flow

    def counted(flow_lr, mask):
        calls[0] += 1
        return inner(flow_lr, mask)

    def refuse(*a, **kw):
        raise AssertionError("the fused kernel ran with fused_raft_loss=False")
    monkeypatch.setattr(RAFT, "upsample_flow", staticmethod(counted))
    monkeypatch.setattr(T, "_raft_loss_kernel", refuse)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss, metrics = T.finetune_step(net, opt, sched, x1, x2, flow, valid, args, fused_raft_loss=False)
    assert calls[0] == 12 and torch.isfinite(loss) and set(metrics) == {"epe", "1px", "3px", "5px"}


def _gradients(net, fused, gamma):
    from understanding_flow_robustness_amd import training as T
    x1, x2, flow, valid = _batch()
    net.zero_grad(set_to_none=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        preds = net(x1 * 255.0, x2 * 255.0, iters=12, lowres_predictions=fused)
    loss, _ = T.sequence_loss(preds, flow, valid, gamma)
    loss.backward()
    return {n: None if p.grad is None else p.grad.detach().clone() for n, p in net.named_parameters()}


def _without_signal(name):
    """The feature encoder's convolutions in front of its InstanceNorm (no affine part, batch statistics): the norm removes a
    constant, so the gradient of their biases is exactly zero and what the backward leaves is the rounding of a sum that cancels."""
    return name.startswith("fnet.") and name.endswith(".bias") and name != "fnet.conv2.bias"


def _worst(a, b):
    """(the largest per-tensor difference relative to the tensor's largest gradient magnitude in `b`, its tensor), over every
    parameter whose gradient is not zero by construction."""
    worst = (0.0, None)
    for n in b:
        assert (a[n] is None) == (b[n] is None), n
        if b[n] is None or _without_signal(n):
            continue
        assert torch.isfinite(a[n]).all() and torch.isfinite(b[n]).all(), n
        scale = float(b[n].abs().max())
        assert scale > 0.0, n
        e = float((a[n] - b[n]).abs().max()) / scale
        if e > worst[0]:
            worst = (e, n)
    return worst


def test_parameter_gradients_of_the_fused_and_the_unfused_loss_agree(net, monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    fused = _gradients(net, True, 0.8)
    plain, again = _gradients(net, False, 0.8), _gradients(net, False, 0.8)
    other = _gradients(net, False, 0.85)
    noise, diff, gamma = _worst(again, plain), _worst(fused, plain), _worst(other, plain)
    print(f"unfused run to run {noise[0]:.3e} ({noise[1]}); fused to unfused {diff[0]:.3e} ({diff[1]}); "
          f"gamma 0.85 to 0.8 {gamma[0]:.3e} ({gamma[1]}); gate {GATE:.3e}")
    assert sum(g is not None and not _without_signal(n) for n, g in plain.items()) > 100
    assert noise[0] <= GATE, f"two unfused runs differ by {noise[0]:.3e} ({noise[1]}): the comparison below means nothing"
    assert diff[0] <= GATE, f"fused and unfused parameter gradients differ by {diff[0]:.3e} ({diff[1]})"
    assert gamma[0] > GATE, f"the gate does not discriminate: gamma 0.85 against 0.8 differs by {gamma[0]:.3e} only"
    # the biases whose gradient is zero by construction have no magnitude to be relative to (two unfused runs differ by more than
    # their own size there): in every leg they stay at the rounding level of the largest gradient, 16 units in its last place
    top = max(float(g.abs().max()) for g in plain.values() if g is not None)
    silent = [n for n in plain if _without_signal(n)]
    assert len(silent) == 15
    for leg in (fused, plain, again):
        for n in silent:
            assert float(leg[n].abs().max()) <= 2.0 ** -20 * top, n
