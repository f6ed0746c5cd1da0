"""GPU suite: RAFT_FlowNetCEncoder_WoContext -- the context-head kernels (csrc/raft_context_head.hip) against torch, the encoder
graph (plane_graph.stem_graph with conv_redir as its head) and the whole model against the reference's goldens (tests/golden/make_golden_raft_fnc.py),
frame sides that are multiples of 8 only, the precision switch's cache key and the static-buffer contract of the engines."""
import pytest
import torch

from closeness import assert_close
from conftest import t
from raft_fnc_helpers import check_encoder, check_weights, encoder_case, encoder_heads, fetch, model_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 1e-4
ULP = 2.0 ** -23


class _on_the_engines:
    """The frozen leg of a golden test (tests/test_models_gpu.py): the caller's parameters are frozen, so every convolution must run
    on the hand-written engines -- any route to the vendor library inside the block fails the test."""
    def __init__(self, net, frozen):
        self.net, self.frozen = net, frozen

    def __enter__(self):
        from understanding_flow_robustness_amd import _lib as L
        if self.frozen:
            self.net.requires_grad_(False)
        self.before = dict(L.VENDOR_FALLBACKS)
        return self

    def __exit__(self, *exc):
        from understanding_flow_robustness_amd import _lib as L
        if self.frozen and exc[0] is None:
            grown = {k: v - self.before.get(k, 0) for k, v in L.VENDOR_FALLBACKS.items() if v != self.before.get(k, 0)}
            assert not grown, f"the frozen leg left the engines: {grown}"


FROZEN = pytest.mark.parametrize("frozen", [False, True], ids=["torch_spelling", "engines"])


@pytest.fixture(scope="module")
def golden():
    return model_golden()


# ------------------------------------------------------------------------------------------------------ 1. the context head
@pytest.mark.parametrize("B,Ct,Cr,H,W", [(1, 128, 128, 16, 24), (2, 128, 128, 5, 7), (2, 96, 64, 3, 1)])
def test_context_head_against_torch(B, Ct, Cr, H, W):
    """16-byte lanes (HW = 384), the one-float form (HW = 35, HW = 3), two images, unequal halves.  The ReLU half and the copy
    structure are exact; the tanh half may be one float32 ulp (2^-23 at |tanh| < 1) further from the float64 tanh of the same
    float32 input than torch.tanh is, its adjoint 2^-23 max |g| further than torch's float32 `g * (1 - net * net)` (a differently
    contracted 1 - t * t)."""
    from understanding_flow_robustness_amd.raft_glue import context_split
    g = torch.Generator().manual_seed(100 + H * W)
    ctx = 3 * torch.randn(B, Ct + Cr, H, W, generator=g)
    ctx[0, 1, 0, 0] = 0.0
    ctx[B - 1, Ct + 1, H - 1, 0] = 0.0
    gn, gi = torch.randn(B, Ct, H, W, generator=g).to(DEV), torch.randn(B, Cr, H, W, generator=g).to(DEV)
    x = ctx.to(DEV).requires_grad_(True)
    net, inp = context_split(x, Ct)
    assert net.shape == (B, Ct, H, W) and inp.shape == (B, Cr, H, W) and net.is_contiguous() and inp.is_contiguous()
    assert torch.equal(inp, torch.relu(x.detach()[:, Ct:]))
    truth = torch.tanh(x.detach()[:, :Ct].double())
    e_kernel = float((net.double() - truth).abs().max())
    e_torch = float((torch.tanh(x.detach()[:, :Ct]).double() - truth).abs().max())
    print(f"tanh half: kernel {e_kernel:.3e}, torch {e_torch:.3e} from the float64 tanh")
    assert e_kernel <= e_torch + ULP

    (g_ctx,) = torch.autograd.grad((net, inp), x, (gn, gi), retain_graph=True)
    assert g_ctx.shape == x.shape
    assert torch.equal(g_ctx[:, Ct:], torch.where(inp > 0, gi, torch.zeros_like(gi)))
    nd = net.detach()
    truth_g = gn.double() * (1 - nd.double() * nd.double())
    e_kernel = float((g_ctx[:, :Ct].double() - truth_g).abs().max())
    e_torch = float(((gn * (1 - nd * nd)).double() - truth_g).abs().max())
    print(f"tanh adjoint: kernel {e_kernel:.3e}, torch {e_torch:.3e} from the float64 expression")
    assert e_kernel <= e_torch + ULP * float(gn.abs().max())

    (only_net,) = torch.autograd.grad(net, x, gn, retain_graph=True)          # g_inp absent: the ReLU half of g_ctx is zero
    assert torch.equal(only_net[:, :Ct], g_ctx[:, :Ct]) and not bool(only_net[:, Ct:].any())
    (only_inp,) = torch.autograd.grad(inp, x, gi)                             # g_net absent
    assert torch.equal(only_inp[:, Ct:], g_ctx[:, Ct:]) and not bool(only_inp[:, :Ct].any())


def test_context_head_on_a_tensor_that_is_not_16_byte_aligned():
    """HW a multiple of 4 but ctx starting 4 bytes past a 16-byte boundary: the one-float form serves it, same results."""
    from understanding_flow_robustness_amd.raft_glue import context_split
    g = torch.Generator().manual_seed(5)
    B, Ct, Cr, H, W = 2, 8, 8, 2, 4
    store = torch.zeros(B * (Ct + Cr) * H * W + 1, device=DEV)
    x = store[1:].view(B, Ct + Cr, H, W)
    x.copy_(3 * torch.randn(B, Ct + Cr, H, W, generator=g))
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    want_net, want_inp = context_split(x.clone(), Ct)                           # the aligned copy: 16-byte lanes
    x.requires_grad_(True)
    net, inp = context_split(x, Ct)
    assert torch.equal(net, want_net) and torch.equal(inp, want_inp) and torch.equal(inp, torch.relu(x.detach()[:, Ct:]))
    gn = torch.randn(B, Ct, H, W, generator=g).to(DEV)
    (g_ctx,) = torch.autograd.grad(net, x, gn)
    assert torch.equal(g_ctx[:, :Ct], gn * (1 - net.detach() * net.detach())) and not bool(g_ctx[:, Ct:].any())


def test_context_split_declines_what_the_kernel_does_not_serve():
    from understanding_flow_robustness_amd.raft_glue import context_split
    assert context_split(torch.zeros(1, 4, 2, 2), 2) is None                                   # a CPU tensor
    assert context_split(torch.zeros(1, 4, 2, 2, device=DEV, dtype=torch.float64), 2) is None
    assert context_split(torch.zeros(1, 4, 2, 2, device=DEV), 4) is None                       # no ReLU half


# ------------------------------------------------------------------------------------------------------ 2. encoder + head
@FROZEN
def test_encoder_and_context_head_vs_reference(frozen):
    z, x1, x2, ws = encoder_case(DEV)
    net, _ = fetch(DEV)
    check_weights(net, z)
    x1.requires_grad_(True), x2.requires_grad_(True)
    with _on_the_engines(net, frozen):
        outs = encoder_heads(net, x1, x2, model_path=True)
        grads = torch.autograd.grad(sum((w * o).sum() for w, o in zip(ws, outs)), (x1, x2))
    assert ("_ufr_plane_graphs" in net.__dict__) == frozen
    # the frozen leg's halves come out of the context-head kernel, the other leg's out of torch.tanh / torch.relu
    assert (type(outs[2].grad_fn).__name__ == "_ContextSplitBackward") == frozen and outs[2].grad_fn is not None
    check_encoder(z, outs, grads)


# ------------------------------------------------------------------------------------------------------ 3. the whole model
def _check(z, net, args):
    from understanding_flow_robustness_amd.flownets.utils_model import predict_flow
    x1, x2 = t(z["x1"], DEV).requires_grad_(True), t(z["x2"], DEV).requires_grad_(True)
    flow = predict_flow(net, None, x1, x2, args)
    ref = t(z["flow"])
    assert_close(flow, ref, rtol=REL, atol_scale=REL, what="flow")
    epe = (flow.detach().cpu() - ref).pow(2).sum(1).sqrt().mean()
    print(f"EPE {float(epe):.3e} at a mean |flow| of {float(ref.pow(2).sum(1).sqrt().mean()):.3e}")
    assert float(epe) <= REL * float(ref.pow(2).sum(1).sqrt().mean()), f"EPE {float(epe):.3e}"
    loss = (1 - torch.nn.functional.cosine_similarity(flow, t(z["target"], DEV))).mean()
    print(f"loss {float(loss.detach()):.7f} vs {float(z['loss']):.7f}")
    assert abs(float(loss.detach()) - float(z["loss"])) < 2e-5
    g1, g2 = torch.autograd.grad(loss, (x1, x2))
    # The reference's own float32 disagreement with itself (a batch of two on 8 threads vs pair by pair on 1 thread) is the
    # conditioning yardstick; x10 for a device's summation order.  Floors: FlowNetC's entrywise gate, PWC-Net's bulk gates; caps:
    # what test_raft_vs_reference allows the instance-normalised RAFT.
    worst, q50_gate, q90_gate = 10 * float(z["g_spread_worst"]), max(10 * float(z["g_spread_q50"]), 2e-5), max(10 * float(z["g_spread_q90"]), 2e-4)
    assert q50_gate <= 1e-3 and q90_gate <= 5e-3
    for name, g, ref_g in (("grad frame 1", g1, t(z["g1"])), ("grad frame 2", g2, t(z["g2"]))):
        scale = float(ref_g.abs().max())
        err = (g.detach().double().cpu() - ref_g.double()).abs()
        rel = err.flatten() / scale
        q50, q90 = float(torch.quantile(rel, 0.5)), float(torch.quantile(rel, 0.9))
        print(f"{name}: median {q50:.2e}, 90 % within {q90:.2e}, max {float(rel.max()):.2e} of the gradient's scale "
              f"(reference's own spread: {float(z['g_spread_q50']):.2e}, {float(z['g_spread_q90']):.2e}, {float(z['g_spread_worst']):.2e})")
        bound = torch.clamp(torch.maximum(torch.full_like(err, worst * scale), 1e-3 * ref_g.double().abs() + 2e-4 * scale), max=5e-2 * scale)
        bad = err > bound
        assert not bool(bad.any()), f"{name}: {int(bad.sum())}/{bad.numel()} entries off; max err {float(rel.max()):.3e} of the scale"
        assert q50 <= q50_gate and q90 <= q90_gate, f"{name}: median {q50:.2e}, 90 % within {q90:.2e} of the scale"


def _attack_check(z, net, args, key, lr, iters, tol=1e-4):
    from understanding_flow_robustness_amd import _lib as L
    from understanding_flow_robustness_amd.patch_attack import attack
    args.l2, args.alpha, args.lr, args.max_count = False, 0.0, lr, iters
    patch = t(z["patch0"], DEV).clone()
    before = dict(L.VENDOR_FALLBACKS)
    attack(net, t(z["x1"], DEV)[:1], None, t(z["x2"], DEV)[:1], patch, t(z["mask"], DEV), t(z["patch0"], DEV),
           t(z["attack_target"], DEV), None, args=args)
    assert dict(L.VENDOR_FALLBACKS) == before, "attack() freezes the parameters: its forwards stay on the engines"
    ref, shown = t(z[key]), (t(z["mask"]) != 0).float()
    upd = float(((ref - t(z["patch0"])) * shown).abs().max())
    err = float(((patch.cpu() - ref) * shown).abs().max())
    print(f"{args.flownet} attack golden ({key}): patch error {err:.3e} at an update of {upd:.3e} = {err / max(upd, 1.0):.2e} (gate {tol:.0e})")
    assert err <= tol * max(upd, 1.0), f"patch err {err:.3e} vs update {upd:.3e}"


@FROZEN
@pytest.mark.parametrize("alternate", [False, True])
def test_raft_fnc_vs_reference(alternate, frozen, golden, monkeypatch):
    """Flow, EPE, loss, image gradients and a 2-iteration attack() against the reference run on the CPU (all-pairs correlation; the
    on-the-fly form agrees at the same gates); every figure is printed before its gate.  Measured on an MI355X over the four
    legs: EPE 2.5 - 2.6e-6 at a mean |flow| of 14.3 (1.8e-7 relative), loss equal to 7 digits; image gradients: median 5.2 - 8.7e-8,
    90 % within 1.6 - 2.7e-7, worst entry 0.9 - 1.7e-6 of the gradient's scale (gates 2e-5 / 2e-4 / FlowNetC's entrywise gate; the
    reference's own spread is 6.3e-8 / 1.9e-7 / 9.5e-7); attack patch 6.0e-8 from the reference's at an update of 2.1e-3 (gate 1e-4)."""
    net, args = fetch(DEV, alternate_corr=alternate)
    check_weights(net, golden)
    assert args.mixed_precision is True          # float32 all the same: the flag alone changes nothing here
    from understanding_flow_robustness_amd import raft_glue
    calls, kernel = [], raft_glue.context_split
    monkeypatch.setattr(raft_glue, "context_split", lambda *a: calls.append(1) or kernel(*a))
    with _on_the_engines(net, frozen):
        _check(golden, net, args)
    assert len(calls) == (1 if frozen else 0), "the frozen forward takes the context-head kernel, the torch spelling does not"
    _attack_check(golden, net, args, "attack_it2_patch", 1e4, 2)
    assert len(calls) > (1 if frozen else 0), "attack() freezes the parameters: its forwards take the kernel"


# ------------------------------------------------------------------------------------------------------ 4. sides that are multiples of 8 only
def test_sides_that_are_multiples_of_8_but_not_of_64(monkeypatch):
    from understanding_flow_robustness_amd import _lib as L
    from understanding_flow_robustness_amd.flownets.utils_model import predict_flow
    net, args = fetch(DEV)
    net.requires_grad_(False)
    g = torch.Generator().manual_seed(17)
    x1, x2 = torch.rand(1, 3, 72, 104, generator=g).to(DEV), torch.rand(1, 3, 72, 104, generator=g).to(DEV)
    monkeypatch.setenv("UFR_ENGINE", "0")
    with torch.no_grad():
        want = predict_flow(net, None, x1, x2, args)
    monkeypatch.setenv("UFR_ENGINE", "1")
    before = dict(L.VENDOR_FALLBACKS)
    with torch.no_grad():
        flow = predict_flow(net, None, x1, x2, args)
    grown = {k: v - before.get(k, 0) for k, v in L.VENDOR_FALLBACKS.items() if v != before.get(k, 0)}
    assert not grown or (len(grown) == 1 and sum(grown.values()) == 1 and all(k[1] for k in grown)), grown
    err = float((flow - want).abs().max()) / float(want.abs().max())
    print(f"72 x 104: {err:.2e} of max |flow| from the UFR_ENGINE=0 leg; refusals: {grown or 'none'}")
    assert tuple(flow.shape) == (1, 2, 72, 104) and err <= 1e-4


# ------------------------------------------------------------------------------------------------------ 5. cache and precision
def test_reduced_precision_graph_is_not_handed_to_a_float32_forward(monkeypatch):
    """The encoder graph's cache key carries the product count: a bf16 forward builds its own graph and the float32 forward behind
    it is bit for bit the forward of a model that never saw the switch."""
    from understanding_flow_robustness_amd.flownets.utils_model import predict_flow
    g = torch.Generator().manual_seed(19)
    x1, x2 = torch.rand(1, 3, 64, 128, generator=g).to(DEV), torch.rand(1, 3, 64, 128, generator=g).to(DEV)
    net, args = fetch(DEV)
    net.requires_grad_(False)
    assert args.mixed_precision is True
    monkeypatch.setenv("UFR_RAFT_PRECISION", "bf16")
    assert net.products() == 1
    with torch.no_grad():
        reduced = predict_flow(net, None, x1, x2, args).clone()
    monkeypatch.delenv("UFR_RAFT_PRECISION")
    assert net.products() == 6
    with torch.no_grad():
        full = predict_flow(net, None, x1, x2, args).clone()
    fresh, fresh_args = fetch(DEV)
    fresh.requires_grad_(False)
    with torch.no_grad():
        want = predict_flow(fresh, None, x1, x2, fresh_args)
    assert torch.equal(full, want)
    assert not torch.equal(reduced, full)
    keys = [k for k in net.__dict__["_ufr_plane_graphs"] if k[0] == "context_stem"]
    assert sorted(k[-1] for k in keys) == [1, 6]


# ------------------------------------------------------------------------------------------------------ 6. static buffers
def test_backward_after_a_second_forward_raises():
    from understanding_flow_robustness_amd.flownets.utils_model import predict_flow
    net, args = fetch(DEV)
    net.requires_grad_(False)
    g = torch.Generator().manual_seed(23)
    x1, x2 = torch.rand(1, 3, 64, 128, generator=g).to(DEV).requires_grad_(True), torch.rand(1, 3, 64, 128, generator=g).to(DEV)
    first = predict_flow(net, None, x1, x2, args)
    second = predict_flow(net, None, x1, x2, args)
    with pytest.raises(RuntimeError, match="another forward"):
        first.square().mean().backward()
    (g1,) = torch.autograd.grad(second.square().mean(), x1)                   # the latest forward is still differentiable
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0
