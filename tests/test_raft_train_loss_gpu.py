"""The fused RAFT loss (csrc/raft_train_loss.hip behind `training.sequence_loss` / `training.multiscale_epe` on a `RaftPredictions`):
convex upsampling, sequence loss and the gradient of every low-resolution flow and mask in three launches.

Yardstick: computed here, on the CPU, in float64, from the same float32 inputs: the torch spelling of `RAFT.upsample_flow`, then
`training._sequence_loss_torch` / `_multiscale_epe_torch` and autograd (both pinned to the reference by
tests/golden/training_loss_d_raft.npz and tests/test_raft_upsample_gpu.py).

Gate (the form of tests/test_train_loss_gpu.py): for the loss, the `epe` metric and every gradient tensor, the error relative to the
largest magnitude is at most max(3 x the error of the float32 unfused path on the device, 2**-22).  No element is exempted.

Shapes (B, coarse H x W, predictions): a = 2, 5 x 7, 3 (one partial column group, a border on every side); b = 1, 3 x 33, 12 (a full
group plus one column, the workload's count); c = 3, 2 x 40, 1 (a single prediction).

Inputs: flows ~ 4 N(0,1), masks ~ 2 N(0,1), `valid` with ~20 % zeros and one whole 8 x 8 cell of zeros, a handful of ground-truth
vectors of magnitude above 400.  The ground truth is built from the float64 upsamplings so that sign(up - gt) cannot flip under
float32 rounding: per element it lies above the maximum or below the minimum of the float64 up_i by 0.05 + U(0, 6), the side chosen
at random; and no valid pixel's float64 end-point error of the last prediction lies within 1e-4 of 1, 3 or 5, so the 1px / 3px / 5px
shares must equal the float64 ones exactly.  Both preconditions are asserted where the inputs are built."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 2.0 ** -22
SHAPES = {"a": (2, 5, 7, 3), "b": (1, 3, 33, 12), "c": (3, 2, 40, 1)}
SEEDS = {"a": 0, "b": 1, "c": 2}
# the defaults, and gamma 0.85 + div_flow 20 + not_excluding (the ground truth is then built 20 times as large: the margin holds after
# the division)
VARIANTS = {"plain": dict(), "g85div20": dict(gamma=0.85, div_flow=20, not_excluding=True)}
CASES = [("a", "plain", "seq"), ("b", "plain", "seq"), ("c", "plain", "seq"), ("a", "g85div20", "seq"), ("a", "g85div20", "epe"),
         ("a", "plain", "epe")]


def _T():
    from understanding_flow_robustness_amd import training as T
    return T


def _up_torch(flow, mask):
    """RAFT.upsample_flow's torch spelling (models/raft/raft.py:111-122) in the dtype of its inputs."""
    N, _, H, W = flow.shape
    mask = torch.softmax(mask.view(N, 1, 9, 8, 8, H, W), dim=2)
    up = torch.nn.functional.unfold(8 * flow, [3, 3], padding=1).view(N, 2, 9, 1, 1, H, W)
    return torch.sum(mask * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(N, 2, 8 * H, 8 * W)


def _loss_torch(lname, ups, gt, valid, gamma=0.8, max_flow=400, not_excluding=False, div_flow=1):
    T = _T()
    if lname == "seq":
        return T._sequence_loss_torch(ups, gt, valid, gamma, max_flow, False, False, not_excluding, div_flow, False)
    return T._multiscale_epe_torch(ups, gt, valid, gamma, max_flow, False, not_excluding, div_flow, False, False)


@functools.lru_cache(maxsize=None)
def _inputs(name, variant):
    """CPU tensors: float32 flows, masks, gt, valid (preconditions asserted)."""
    B, H, W, n = SHAPES[name]
    kw = VARIANTS[variant]
    g = torch.Generator().manual_seed(SEEDS[name])
    flows = [torch.randn(B, 2, H, W, generator=g) * 4 for _ in range(n)]
    masks = [torch.randn(B, 576, H, W, generator=g) * 2 for _ in range(n)]
    ups = torch.stack([_up_torch(f.double(), m.double()) for f, m in zip(flows, masks)])
    hi, lo = ups.max(dim=0).values, ups.min(dim=0).values
    above = torch.rand(hi.shape, generator=g) < 0.5
    off = 0.05 + 6 * torch.rand(hi.shape, generator=g, dtype=torch.float64)
    gt64 = torch.where(above, hi + off, lo - off)
    for _ in range(6):                                       # a handful of vectors longer than 400 (they stay outside [lo, hi])
        b, y, x = (int(torch.randint(0, s, (1,), generator=g)) for s in (B, 8 * H, 8 * W))
        gt64[b, :, y, x] = torch.where(above[b, :, y, x], 450.0 + off[b, :, y, x], -450.0 - off[b, :, y, x])
    scale = float(kw.get("div_flow", 1))
    gt = (gt64 * scale).float()
    valid = (torch.rand(B, 8 * H, 8 * W, generator=g) > 0.2).float()
    valid[0, 8:16, 16:24] = 0                                # one whole cell of a coarse pixel
    # precondition 1: the margin, as the kernel sees the ground truth (float32, divided in float32)
    seen = (gt / scale if scale > 1 else gt).double()
    margin = torch.maximum(seen - hi, lo - seen)
    assert float(margin.min()) > 0.0499, f"case {name}-{variant}: margin {float(margin.min())}"
    # precondition 2: no valid pixel of the last prediction within 1e-4 of a threshold
    v = _T()._valid_mask(seen, valid.double(), 400, kw.get("not_excluding", False))
    epe = (ups[-1] - seen).pow(2).sum(dim=1).sqrt()[v]
    assert 0 < epe.numel() < v.numel() and (valid[0, 8:16, 16:24] == 0).all()
    if not kw.get("not_excluding", False):
        assert int(((valid >= 0.5) & ~v).sum()) >= 1, "no long vector on a valid pixel"
    for t in (1.0, 3.0, 5.0):
        assert float((epe - t).abs().min()) > 1e-4, f"case {name}-{variant}: an end-point error within 1e-4 of {t}"
    return flows, masks, gt, valid


@functools.lru_cache(maxsize=None)
def _truth(name, variant, lname):
    """float64 on the CPU: (loss, metrics, [flow gradients..., mask gradients...])."""
    flows, masks, gt, valid = _inputs(name, variant)
    leaves = [t.double().requires_grad_(True) for t in flows + masks]
    n = len(flows)
    ups = [_up_torch(f, m) for f, m in zip(leaves[:n], leaves[n:])]
    kw = VARIANTS[variant]
    loss, metrics = _loss_torch(lname, ups, gt.double(), valid.double(), **kw)
    grads = torch.autograd.grad(loss, leaves)
    # the shares as exact ratios (the restatement rounds them to float32)
    seen = gt.double() / kw["div_flow"] if kw.get("div_flow", 1) > 1 else gt.double()
    v = _T()._valid_mask(seen, valid.double(), 400, kw.get("not_excluding", False))
    epe = (ups[-1].detach() - seen).pow(2).sum(dim=1).sqrt()[v]
    assert metrics["epe"] == float(epe.mean())
    for t in (1, 3, 5):
        share = int((epe < t).sum()) / epe.numel()
        assert abs(share - metrics[f"{t}px"]) < 1e-6
        metrics[f"{t}px"] = share
    return float(loss.detach()), metrics, [x.numpy() for x in grads]


def _run(lname, flows, masks, gt, valid, kw, fused, scale=None):
    """On the device: (loss, metrics, [flow gradients..., mask gradients...]) of the fused call or of the unfused float32 path."""
    from understanding_flow_robustness_amd.flownets.raft import RaftPredictions
    T = _T()
    n = len(flows)
    leaves = [t.detach().clone().to(DEV).requires_grad_(True) for t in list(flows) + list(masks)]
    preds = RaftPredictions(leaves[:n], leaves[n:])
    if fused:
        loss, metrics = (T.sequence_loss if lname == "seq" else T.multiscale_epe)(preds, gt, valid, **kw)
    else:
        loss, metrics = _loss_torch(lname, preds.upsampled(), gt, valid, **kw)
    if loss.requires_grad:
        (loss if scale is None else loss * scale).backward()
    return loss.detach().clone(), metrics, [x.grad for x in leaves]


@pytest.fixture(scope="module", params=CASES, ids=["-".join(c) for c in CASES])
def case(request):
    name, variant, lname = request.param
    flows, masks, gt, valid = _inputs(name, variant)
    gt, valid = gt.to(DEV), valid.to(DEV)
    yard = _run(lname, flows, masks, gt, valid, VARIANTS[variant], fused=False)
    return name, variant, lname, flows, masks, gt, valid, yard


def _refuse_restatement(m):
    def refuse(*a, **kw):
        raise AssertionError("the torch restatement ran on kernel-path inputs")
    m.setattr(_T(), "_sequence_loss_torch", refuse)
    m.setattr(_T(), "_multiscale_epe_torch", refuse)


def _gate(got, yard, want, what):
    scale = float(np.max(np.abs(want)))
    assert np.isfinite(got).all() and scale > 0, what
    e, e_t = float(np.max(np.abs(got - want))) / scale, float(np.max(np.abs(yard - want))) / scale
    print(f"{what}: fused {e:.3e}, unfused float32 {e_t:.3e} of the float64 value")
    assert e <= max(3 * e_t, FLOOR), f"{what}: fused {e:.3e} vs unfused float32 {e_t:.3e}"


def test_the_fused_path_is_inside_the_gate(case, monkeypatch):
    name, variant, lname, flows, masks, gt, valid, yard = case
    want_loss, want_metrics, want_grads = _truth(name, variant, lname)
    with monkeypatch.context() as m:
        _refuse_restatement(m)
        loss, metrics, grads = _run(lname, flows, masks, gt, valid, VARIANTS[variant], fused=True)
    y_loss, y_metrics, y_grads = yard
    assert loss.dtype == torch.float32 and loss.dim() == 0 and all(isinstance(v, float) for v in metrics.values())
    assert set(metrics) == set(want_metrics) == ({"epe", "1px", "3px", "5px"} | ({"loss"} if lname == "epe" else set()))
    tag = f"{name}-{variant}-{lname}"
    _gate(np.float64(float(loss)), np.float64(float(y_loss)), np.float64(want_loss), f"{tag} loss")
    _gate(np.float64(metrics["epe"]), np.float64(y_metrics["epe"]), np.float64(want_metrics["epe"]), f"{tag} epe")
    for px in ("1px", "3px", "5px"):
        assert metrics[px] == want_metrics[px], f"{tag} {px}: {metrics[px]} vs {want_metrics[px]}"
    if lname == "epe":
        assert float(np.float32(metrics["loss"])) == float(loss)        # the float64 value the float32 loss tensor was rounded from
    n = len(flows)
    for i, (g, y, w) in enumerate(zip(grads, y_grads, want_grads)):
        what = f"{tag} grad_{'flow' if i < n else 'mask'}{i % n}"
        assert g is not None and g.shape == w.shape, what
        _gate(g.double().cpu().numpy(), y.double().cpu().numpy(), w, what)


def test_pixels_outside_the_valid_set_get_exact_zeros(case):
    """g_up is exactly 0 where v == 0: a coarse pixel whose whole 8 x 8 cell is invalid gets zeros in all 576 mask gradients."""
    name, variant, lname, flows, masks, gt, valid, _ = case
    _, _, grads = _run(lname, flows, masks, gt, valid, VARIANTS[variant], fused=True)
    for g in grads[len(flows):]:
        assert not g[0, :, 1, 2].any()


def test_two_runs_are_bit_identical(case):
    name, variant, lname, flows, masks, gt, valid, _ = case
    a = _run(lname, flows, masks, gt, valid, VARIANTS[variant], fused=True)
    b = _run(lname, flows, masks, gt, valid, VARIANTS[variant], fused=True)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and a[1] == b[1]
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[2], b[2]))


def test_multiscale_epe_gives_the_same_loss_plus_its_metric():
    flows, masks, gt, valid = _inputs("a", "g85div20")
    gt, valid = gt.to(DEV), valid.to(DEV)
    s = _run("seq", flows, masks, gt, valid, VARIANTS["g85div20"], fused=True)
    e = _run("epe", flows, masks, gt, valid, VARIANTS["g85div20"], fused=True)
    assert torch.equal(s[0], e[0]) and e[1] == dict(s[1], loss=e[1]["loss"]) and float(np.float32(e[1]["loss"])) == float(e[0])
    assert all(torch.equal(x, y) for x, y in zip(s[2], e[2]))


def test_one_nan_in_the_ground_truth_makes_the_loss_nan(monkeypatch):
    flows, masks, gt, valid = _inputs("a", "plain")
    gt, valid = gt.to(DEV).clone(), valid.to(DEV).clone()
    gt[1, 0, 17, 30] = float("nan")
    valid[1, 17, 30] = 1.0
    want, _, _ = _run("seq", flows, masks, gt, valid, {}, fused=False)
    with monkeypatch.context() as m:
        _refuse_restatement(m)
        loss, metrics, _ = _run("seq", flows, masks, gt, valid, {}, fused=True)
    assert torch.isnan(want) and torch.isnan(loss)


def test_an_empty_valid_set(monkeypatch):
    flows, masks, gt, valid = _inputs("a", "plain")
    gt, valid = gt.to(DEV), torch.zeros_like(valid).to(DEV)
    with monkeypatch.context() as m:
        _refuse_restatement(m)
        loss, metrics, grads = _run("epe", flows, masks, gt, valid, {}, fused=True)
    assert float(loss) == 0.0 and metrics["loss"] == 0.0 and all(np.isnan(metrics[k]) for k in ("epe", "1px", "3px", "5px"))
    assert all(g is not None and not g.any() and not torch.isnan(g).any() for g in grads)


def test_other_inputs_take_the_restatement(monkeypatch):
    """float64 tensors, a ground truth of another size, the `flowNetC` / `pwc` keywords and the LIST form never reach the new kernel."""
    from understanding_flow_robustness_amd.flownets.raft import RaftPredictions
    T = _T()

    def refuse(*a, **kw):
        raise AssertionError("the fused kernel path ran")
    monkeypatch.setattr(T, "_raft_loss_kernel", refuse)
    flows, masks, gt, valid = _inputs("a", "plain")
    gt, valid = gt.to(DEV), valid.to(DEV)
    f64 = RaftPredictions([f.double().to(DEV) for f in flows], [m.double().to(DEV) for m in masks])
    loss, _ = T.sequence_loss(f64, gt.double(), valid.double())
    assert loss.dtype == torch.float64 and torch.isfinite(loss)
    f32 = RaftPredictions([f.to(DEV) for f in flows], [m.to(DEV) for m in masks])
    one = RaftPredictions([f[:1].to(DEV) for f in flows], [m[:1].to(DEV) for m in masks])
    loss, _ = T.sequence_loss(one, gt, valid)                             # predictions of batch 1 against a gt of batch 2: torch broadcasts
    assert loss.dtype == torch.float32 and torch.isfinite(loss)
    loss, metrics = T.multiscale_epe(f32, gt.double(), valid)             # one float64 operand
    assert torch.isfinite(loss) and "loss" in metrics
    loss, _ = T.sequence_loss(f32.upsampled(), gt, valid)                 # the list form
    assert torch.isfinite(loss)
    loss, _ = T.sequence_loss(f32, gt, valid, pwc=True)                   # the pyramid keywords: the list form's other branch
    assert torch.isfinite(loss)


def test_one_copy_of_the_metrics_and_no_other_synchronisation(monkeypatch):
    from understanding_flow_robustness_amd.flownets.raft import RaftPredictions
    T = _T()
    flows, masks, gt, valid = _inputs("b", "plain")
    gt, valid = gt.to(DEV), valid.to(DEV)
    leaves = [t.to(DEV).requires_grad_(True) for t in flows + masks]
    preds = RaftPredictions(leaves[:12], leaves[12:])
    T.sequence_loss(preds, gt, valid)[0].backward()            # library loaded, allocator warm
    calls = {"item": 0, "nonzero": 0, "cpu": 0, "sync": 0}
    item, nonzero, cpu, sync = torch.Tensor.item, torch.nonzero, torch.Tensor.cpu, torch.cuda.synchronize

    def counted(name, inner):
        def f(*a, **kw):
            calls[name] += 1
            return inner(*a, **kw)
        return f
    with monkeypatch.context() as m:
        _refuse_restatement(m)
        m.setattr(torch.Tensor, "item", counted("item", item))
        m.setattr(torch, "nonzero", counted("nonzero", nonzero))
        m.setattr(torch.Tensor, "nonzero", counted("nonzero", torch.Tensor.nonzero))
        m.setattr(torch.Tensor, "cpu", counted("cpu", cpu))
        m.setattr(torch.cuda, "synchronize", counted("sync", sync))
        loss, metrics = T.sequence_loss(preds, gt, valid)
        loss.backward()
    assert calls == {"item": 0, "nonzero": 0, "cpu": 1, "sync": 0}, calls
    assert all(x.grad is not None for x in leaves) and float(np.float32(loss._ufr_host_value)) == float(loss)


def test_backward_scales_by_the_incoming_gradient():
    flows, masks, gt, valid = _inputs("a", "plain")
    gt, valid = gt.to(DEV), valid.to(DEV)
    one = _run("seq", flows, masks, gt, valid, {}, fused=True)[2]
    quarter = _run("seq", flows, masks, gt, valid, {}, fused=True, scale=0.25)[2]
    assert all(q.abs().max() > 0 and torch.equal(q, g * 0.25) for q, g in zip(quarter, one))


# ---- at the C level -------------------------------------------------------------------------------------------------------------------
GUARD = 64
SENTINEL = -1234.5


def _poisoned(shape):
    """(buffer, the output view inside it): GUARD sentinels, the output filled with NaN, GUARD sentinels (the method of
    tests/test_ops_written_gpu.py)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    out = buf[GUARD:GUARD + n].view(shape)
    out.fill_(float("nan"))
    return buf, out


def _call(flows, masks, gt, valid, grad_flows, grad_masks, weights, div_flow=1.0, max_flow=400.0, exclude_large=1):
    from understanding_flow_robustness_amd import _lib as L
    lib = L.lib()
    B, _, H, W = flows[0].shape
    n = len(flows)
    d = L.RaftSequenceLossDesc()
    d.gt, d.valid, d.B, d.H, d.W, d.npred = gt.data_ptr(), valid.data_ptr(), B, H, W, n
    for i in range(n):
        d.flow[i], d.mask[i], d.grad_flow[i], d.grad_mask[i], d.weight[i] = (flows[i].data_ptr(), masks[i].data_ptr(),
                                                                             grad_flows[i].data_ptr(), grad_masks[i].data_ptr(), weights[i])
    d.div_flow, d.max_flow, d.exclude_large = div_flow, max_flow, exclude_large
    need = lib.ufr_raft_sequence_loss_workspace_doubles(B, H, W, n)
    ws = torch.empty(need, dtype=torch.float64, device=DEV)
    out = torch.full((8,), float("nan"), dtype=torch.float64, device=DEV)
    d.ws, d.ws_elems, d.out = ws.data_ptr(), need, out.data_ptr()
    rc = lib.ufr_raft_sequence_loss(ctypes.byref(d), L.stream())
    assert rc == 0, lib.ufr_last_error().decode()
    torch.cuda.synchronize()
    return out.cpu()


def test_every_gradient_element_is_written_and_nothing_beside_it():
    flows, masks, gt, valid = _inputs("a", "plain")
    flows, masks = [f.to(DEV) for f in flows], [m.to(DEV) for m in masks]
    gt, valid = gt.to(DEV), valid.to(DEV)
    gf, gm = [_poisoned(f.shape) for f in flows], [_poisoned(m.shape) for m in masks]
    weights = [0.8 ** (len(flows) - i - 1) for i in range(len(flows))]
    out = _call(flows, masks, gt, valid, [o for _, o in gf], [o for _, o in gm], weights)
    sentinel = torch.tensor(SENTINEL, device=DEV)
    for kind, pairs in (("grad_flow", gf), ("grad_mask", gm)):
        for i, (buf, o) in enumerate(pairs):
            assert bool((buf[:GUARD] == sentinel).all()) and bool((buf[-GUARD:] == sentinel).all()), f"{kind}[{i}]: a guard band was written"
            assert not torch.isnan(o).any(), f"{kind}[{i}]: elements left unwritten"
    # what was written is what the autograd path hands out
    loss, _, grads = _run("seq", flows, masks, gt, valid, {}, fused=True)
    assert float(out[0]) == pytest.approx(float(loss), rel=1e-6) and out[6] == 0 and out[7] == 0
    assert all(torch.equal(o, g) for (_, o), g in zip(gf + gm, grads))


def test_the_metric_reads_the_upsampling_of_the_forward_kernel(monkeypatch):
    """`up` inside the fused kernel is bit-equal to ufr_convex_upsample_forward's: with every pixel valid, the sum of the float32
    end-point errors is the float64 sum of the device's own errors, EXACTLY: every error is a float32 of at least 2**-6 (each
    component is 0.05 off), so a multiple of 2**-29, and the sum of the 15360 of them stays below 2**24: every float64 partial sum, in
    any order, is exact, and one float32 error that differed by one unit in the last place would change the sum."""
    from understanding_flow_robustness_amd.flownets.raft import RAFT
    flows, masks, gt, valid = _inputs("c", "plain")
    flows, masks = [f.to(DEV) for f in flows], [m.to(DEV) for m in masks]
    gt = gt.to(DEV).clamp(-250, 250)                           # every vector shorter than 400: every pixel counts
    valid = torch.ones_like(valid).to(DEV)
    with monkeypatch.context() as m:
        _refuse_restatement(m)
        _, metrics, _ = _run("seq", flows, masks, gt, valid, {}, fused=True)
    up = RAFT.upsample_flow(flows[-1], masks[-1])              # the device kernel
    epe = (up - gt).pow(2).sum(dim=1).sqrt()
    assert epe.dtype == torch.float32 and float(epe.min()) >= 2.0 ** -6 and float(epe.double().sum()) < 2.0 ** 24
    want = float(epe.double().sum()) / epe.numel()
    assert metrics["epe"] == want, (metrics["epe"], want)
