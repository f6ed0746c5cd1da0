"""`training.ClippedAdamW.step(clip=...)` (csrc/optim.hip: `ufr_grad_norm` + `ufr_adamw_step`) against torch.

Tensors of 1, 2, 7, 4095, 4096, 4097, 130*70*5 and 65,540 elements: below, at and above the 4096 elements a workgroup takes, several
workgroups, sizes that are no multiple of a 16-byte vector.  The 4097-element parameter is a view that starts one element into its
storage while its gradient and state do not (the pointers disagree modulo 16 bytes: the one-by-one form); the 65,540-element
parameter, its gradient and its state ALL start one element in (the vector form with a head of three and a tail of one).
Three steps, lr=1e-4, weight_decay=1e-4, eps=1e-8: step 1 on gradients of total norm about 2e3, steps 2 and 3 of about 2 (the
gradients scaled down; with clip=10 the coefficient is then exactly 1), clip=1.0 and clip=10.

Truth: torch.optim.AdamW + clip_grad_norm_ in float64 on the same (float32-representable) values.  Yardstick: the same in float32
on the device.  Gate, per tensor and step, for p, exp_avg, exp_avg_sq and for the total norm: the error relative to the largest
magnitude is at most max(3 x the yardstick's, 2**-22) -- 2**-22 is two float32 spacings at the largest magnitude.  Parameter errors
are NOT normalised by the size of the update (float32 torch itself is 5e-3 off by that measure)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 2.0 ** -22
SHAPES = [(1,), (2,), (7,), (4095,), (4096,), (4097,), (130, 70, 5), (65540,)]
P_VIEW, ALL_VIEW = 5, 7                   # indices into SHAPES
HYPER = dict(lr=1e-4, weight_decay=1e-4, eps=1e-8)
STEPS = 3


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def _values():
    """Initial parameters and the gradients of the three steps: float32-representable, as float64 CPU tensors."""
    g = torch.Generator().manual_seed(7)
    params = [torch.randn(s, generator=g).double() for s in SHAPES]
    total = sum(_numel(s) for s in SHAPES)
    grads = []
    for step in range(STEPS):
        scale = 2.0e3 / total ** 0.5 * (1.0 if step == 0 else 1.0e-3)
        grads.append([(torch.randn(s, generator=g) * scale).float().double() for s in SHAPES])
    return params, grads


def _offset_one(t):
    """A copy of `t` that starts one element into its storage."""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = base[1:].view(t.shape)
    view.copy_(t)
    assert view.storage_offset() == 1 and view.data_ptr() % 16 == 4
    return view


def _params(values, dtype, device, views):
    out = []
    for i, v in enumerate(values):
        t = v.to(dtype).to(device).clone()                       # a copy: the float64 leg would otherwise step `values` itself
        if views and i in (P_VIEW, ALL_VIEW):
            t = _offset_one(t)
        out.append(torch.nn.Parameter(t))
    return out


def _set_grads(params, grads, views):
    for i, (p, g) in enumerate(zip(params, grads)):
        t = g.to(p.dtype).to(p.device).clone()                   # a copy: clip_grad_norm_ scales the torch legs' gradients in place
        p.grad = _offset_one(t) if views and i == ALL_VIEW else t


def _snapshot(opt, params, norm):
    return dict(p=[p.detach().double().cpu() for p in params], m=[opt.state[p]["exp_avg"].double().cpu() for p in params],
                v=[opt.state[p]["exp_avg_sq"].double().cpu() for p in params], norm=float(norm))


def _torch_run(values, grads, clip, dtype, device):
    params = _params(values, dtype, device, False)
    opt = torch.optim.AdamW(params, **HYPER)
    out = []
    for step in range(STEPS):
        _set_grads(params, grads[step], False)
        norm = torch.nn.utils.clip_grad_norm_(params, clip)
        opt.step()
        out.append(_snapshot(opt, params, norm))
    return out


def _native_optimizer(params):
    from understanding_flow_robustness_amd.training import ClippedAdamW
    opt = ClippedAdamW(params, **HYPER)
    p = params[ALL_VIEW]                  # state that starts one element in, like the parameter and its gradient
    opt.state[p] = dict(step=torch.tensor(0.0), exp_avg=_offset_one(torch.zeros_like(p)), exp_avg_sq=_offset_one(torch.zeros_like(p)))
    return opt


def _native_run(values, grads, clip, steps=STEPS):
    params = _params(values, torch.float32, DEV, True)
    opt = _native_optimizer(params)
    out = []
    for step in range(steps):
        _set_grads(params, grads[step], True)
        opt.step(clip=clip)
        out.append(_snapshot(opt, params, opt.grad_norm))
    return out, params, opt


@pytest.fixture(scope="module")
def values():
    return _values()


@pytest.fixture(scope="module", params=[1.0, 10.0], ids=["clip1", "clip10"])
def legs(request, values):
    clip = request.param
    params, grads = values
    truth = _torch_run(params, grads, clip, torch.float64, "cpu")
    yard = _torch_run(params, grads, clip, torch.float32, DEV)
    return clip, truth, yard


def _gate(mine, yard, truth, what):
    for key in ("p", "m", "v"):
        for i, (a, y, t) in enumerate(zip(mine[key], yard[key], truth[key])):
            scale = float(t.abs().max())
            e, e_t = float((a - t).abs().max()) / scale, float((y - t).abs().max()) / scale
            assert e <= max(3 * e_t, FLOOR), f"{what}, {key} of tensor {i} {SHAPES[i]}: {e:.3e} vs torch float32 {e_t:.3e}"
    e, e_t = abs(mine["norm"] - truth["norm"]) / truth["norm"], abs(yard["norm"] - truth["norm"]) / truth["norm"]
    print(f"{what}: total norm {mine['norm']:.6g}, error {e:.3e} (torch float32 {e_t:.3e})")
    assert e <= max(3 * e_t, FLOOR), f"{what}, total norm: {e:.3e} vs torch float32 {e_t:.3e}"


def test_three_steps_are_inside_the_gate(values, legs):
    clip, truth, yard = legs
    assert truth[0]["norm"] == pytest.approx(2e3, rel=0.05) and truth[1]["norm"] == pytest.approx(2.0, rel=0.05)
    mine, params, _ = _native_run(*values, clip)
    assert params[P_VIEW].data_ptr() % 16 == 4 and params[P_VIEW].grad.data_ptr() % 16 == 0
    assert params[ALL_VIEW].data_ptr() % 16 == 4 and params[ALL_VIEW].grad.data_ptr() % 16 == 4
    for step in range(STEPS):
        _gate(mine[step], yard[step], truth[step], f"clip {clip}, step {step + 1}")


def test_the_coefficient_is_one_below_the_clip(values):
    """clip=10, steps 2 and 3 (norm about 2): min(1, 10 / (norm + 1e-6)) is exactly 1, and the step equals the one without a clip."""
    params, grads = values
    with_clip, _, opt = _native_run(params, grads, 10.0)
    assert float(opt._norm[1]) == 1.0 and 1.0 < float(opt.grad_norm) < 10.0
    ps = _params(params, torch.float32, DEV, True)
    plain = _native_optimizer(ps)
    _set_grads(ps, grads[0], True)
    plain.step(clip=10.0)
    for step in (1, 2):
        _set_grads(ps, grads[step], True)
        plain.step()                                           # no clip at all: the coefficient is 1 by definition
    assert all(torch.equal(p.detach().double().cpu(), q) for p, q in zip(ps, with_clip[-1]["p"]))


def test_two_runs_are_bit_identical(values):
    a, _, _ = _native_run(*values, 1.0)
    b, _, _ = _native_run(*values, 1.0)
    for sa, sb in zip(a, b):
        assert sa["norm"] == sb["norm"]
        assert all(torch.equal(x, y) for key in ("p", "m", "v") for x, y in zip(sa[key], sb[key]))


def test_a_parameter_without_a_gradient_is_untouched_and_the_gradients_stay(values):
    from understanding_flow_robustness_amd.training import ClippedAdamW
    params, grads = values
    ps = _params(params, torch.float32, DEV, True)
    idle = torch.nn.Parameter(torch.randn(33, device=DEV))
    before = idle.detach().clone()
    opt = ClippedAdamW(ps + [idle], **HYPER)
    _set_grads(ps, grads[0], True)
    kept = [p.grad.clone() for p in ps]
    moved = [p.detach().clone() for p in ps]
    opt.step(clip=1.0)
    assert torch.equal(idle, before) and idle.grad is None and len(opt.state[idle]) == 0
    assert all(torch.equal(p.grad, g) for p, g in zip(ps, kept)), "step(clip=...) rewrote the gradients"
    assert all(not torch.equal(p.detach(), q) for p, q in zip(ps, moved))
    assert opt.grad_norm.is_cuda and opt.grad_norm.dim() == 0


def test_the_state_continues_in_torch_adamw(values, legs):
    """Two native steps, state_dict() into torch.optim.AdamW, one torch step: inside the gate of three steps."""
    clip, truth, yard = legs
    params, grads = values
    _, ps, opt = _native_run(params, grads, clip, steps=2)
    successor = torch.optim.AdamW(ps, lr=1.0)
    successor.load_state_dict(opt.state_dict())
    assert successor.param_groups[0]["lr"] == HYPER["lr"]
    _set_grads(ps, grads[2], True)
    norm = torch.nn.utils.clip_grad_norm_(ps, clip)
    successor.step()
    _gate(_snapshot(successor, ps, norm), yard[2], truth[2], f"clip {clip}: two native steps + one torch step")


def test_several_param_groups_share_one_norm(values):
    from understanding_flow_robustness_amd.training import ClippedAdamW
    params, grads = values
    ps = _params(params, torch.float32, DEV, False)
    opt = ClippedAdamW([dict(params=ps[:4]), dict(params=ps[4:], lr=3e-4)], **HYPER)
    _set_grads(ps, grads[0], False)
    opt.step(clip=1.0)
    ref = _params(params, torch.float32, DEV, False)
    ropt = torch.optim.AdamW([dict(params=ref[:4]), dict(params=ref[4:], lr=3e-4)], **HYPER)
    _set_grads(ref, grads[0], False)
    norm = torch.nn.utils.clip_grad_norm_(ref, 1.0)
    ropt.step()
    assert float(opt.grad_norm) == pytest.approx(float(norm), rel=1e-6)
    for a, b in zip(ps, ref):
        assert float((a - b).abs().max()) <= 4 * FLOOR * float(b.abs().max())
