"""The kernel path of `training.sequence_loss` / `training.multiscale_epe` (csrc/train_loss.hip) on the fixtures the reference
produced in float64 (tests/golden/make_golden_training.py): case a (five scales, NaN block + a single NaN), case b (ratio 16, rows of
3) and case c (all-NaN ground truth), for the keyword sets `flowNetC`, `pwc`, `flowNetC + flownetc_weighing + div_flow=20`.

Gate: against the float64 fixture, the error relative to the largest magnitude is at most max(3 x the error of the float32 torch
restatement on the same device, 2**-22), for the loss, the `epe` metric and every gradient tensor; NaN positions equal the
fixture's; the 1px / 3px / 5px shares differ by at most one pixel's share; two runs are bit-identical; nothing in the call
synchronises besides the one copy of the metrics."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 2.0 ** -22
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYWORDS = {"fnc": dict(flowNetC=True), "pwc": dict(pwc=True), "fncw": dict(flowNetC=True, flownetc_weighing=True, div_flow=20)}
CASES = [(c, k) for c in "abc" for k in KEYWORDS]


def _run(fn, preds, gt, valid, kw):
    preds = [p.detach().clone().requires_grad_(True) for p in preds]
    loss, metrics = fn(preds, gt.clone(), valid, **kw)
    if loss.requires_grad:
        loss.backward()
    grads = [p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p) for p in preds]
    return loss.detach().clone(), metrics, grads


@pytest.fixture(scope="module", params=CASES, ids=[f"{c}-{k}" for c, k in CASES])
def case(request):
    """Inputs on the device, the fixture, and the float32 restatement's results (the yardstick), computed once."""
    c, k = request.param
    z = np.load(os.path.join(GOLDEN, f"training_loss_{c}.npz"))
    r = np.load(os.path.join(GOLDEN, f"training_loss_{c}_{k}.npz"))
    n = sum(name.startswith("pred") for name in z.files)
    gt = torch.from_numpy(z["gt"]).float().to(DEV)
    valid = torch.from_numpy(z["valid"]).float().to(DEV)
    preds = [torch.from_numpy(z[f"pred{i}"]).float().to(DEV) for i in range(n)]
    # the float32 inputs ARE the fixture's float64 inputs rounded: the rounding is part of both legs' error alike
    yard = {"seq": _run(_seq_torch, preds, gt, valid, KEYWORDS[k]), "epe": _run(_epe_torch, preds, gt, valid, KEYWORDS[k])}
    return c, k, gt, valid, preds, r, yard


def _seq_torch(preds, gt, valid, gamma=0.8, max_flow=400, flowNetC=False, pwc=False, not_excluding=False, div_flow=1,
               flownetc_weighing=False):
    from understanding_flow_robustness_amd import training as T
    return T._sequence_loss_torch(preds, gt, valid, gamma, max_flow, flowNetC, pwc, not_excluding, div_flow, flownetc_weighing)


def _epe_torch(preds, gt, valid, gamma=0.8, max_flow=400, flowNetC=False, not_excluding=False, div_flow=1, flownetc_weighing=False,
               pwc=False):
    from understanding_flow_robustness_amd import training as T
    return T._multiscale_epe_torch(preds, gt, valid, gamma, max_flow, flowNetC, not_excluding, div_flow, flownetc_weighing, pwc)


def _kernel(lname):
    from understanding_flow_robustness_amd import training as T
    return T.sequence_loss if lname == "seq" else T.multiscale_epe


def _scalar_gate(got, yard, want, what):
    if np.isnan(want):
        assert np.isnan(got), f"{what}: {got}, the fixture is NaN"
        return
    e, e_t = abs(got - want) / abs(want), abs(yard - want) / abs(want)
    print(f"{what}: kernel {e:.3e}, torch float32 {e_t:.3e} of the float64 value")
    assert e <= max(3 * e_t, FLOOR), f"{what}: kernel {e:.3e} vs torch float32 {e_t:.3e}"


@pytest.mark.parametrize("lname", ["seq", "epe"])
def test_the_kernel_path_is_inside_the_gate(case, lname, monkeypatch):
    from understanding_flow_robustness_amd import training as T
    c, k, gt, valid, preds, r, yard = case
    with monkeypatch.context() as m:                          # the restatement must not be what answers
        def refuse(*a, **kw):
            raise AssertionError("the torch restatement ran on kernel-path inputs")
        m.setattr(T, "_sequence_loss_torch", refuse)
        m.setattr(T, "_multiscale_epe_torch", refuse)
        loss, metrics, grads = _run(_kernel(lname), preds, gt, valid, KEYWORDS[k])
    y_loss, y_metrics, y_grads = yard[lname]
    assert loss.dtype == torch.float32 and loss.dim() == 0 and all(isinstance(v, float) for v in metrics.values())
    if int(r[f"{lname}_raised"]):
        # multiscale_epe, all-NaN ground truth: every scale is skipped (the reference then raises on its Python float): a zero loss,
        # zero gradients, an empty epe -- what the restatement reports
        assert float(loss) == 0.0 and float(y_loss) == 0.0 and metrics["loss"] == 0.0 and np.isnan(metrics["epe"])
        assert all(not g.any() for g in grads)
        return
    assert set(metrics) == set(y_metrics)
    _scalar_gate(float(loss), float(y_loss), float(r[f"{lname}_loss"]), f"{c}-{k} {lname} loss")
    _scalar_gate(metrics["epe"], y_metrics["epe"], float(r[f"{lname}_metric_epe"]), f"{c}-{k} {lname} epe")
    pixels = preds[0].shape[0] * preds[0].shape[2] * preds[0].shape[3]
    if lname == "epe":
        pixels -= int(np.isnan(r["epe_grad0"]).any(axis=1).sum())      # NaN entries are dropped from this metric
    for px in ("1px", "3px", "5px"):
        want = float(r[f"{lname}_metric_{px}"])
        assert abs(metrics[px] - want) <= 1.0 / pixels + 1e-12, f"{px}: {metrics[px]} vs {want}"
    for i, (g, y) in enumerate(zip(grads, y_grads)):
        want = r[f"{lname}_grad{i}"]
        got = g.double().cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"grad{i}: NaN positions differ from the fixture"
        if lname == "seq":
            assert np.array_equal(got == 0, want == 0), f"grad{i}: the exact zeros at NaN ground truth differ"
        if not np.isfinite(want).any() or np.nanmax(np.abs(want)) == 0:
            assert not np.nan_to_num(got).any()
            continue
        scale = np.nanmax(np.abs(want))
        e = np.nanmax(np.abs(got - want)) / scale
        e_t = np.nanmax(np.abs(y.double().cpu().numpy() - want)) / scale
        print(f"{c}-{k} {lname} grad{i}: kernel {e:.3e}, torch float32 {e_t:.3e} of the float64 gradient")
        assert e <= max(3 * e_t, FLOOR), f"grad{i}: kernel {e:.3e} vs torch float32 {e_t:.3e}"


@pytest.mark.parametrize("lname", ["seq", "epe"])
def test_two_runs_are_bit_identical(case, lname):
    c, k, gt, valid, preds, r, _ = case
    a = _run(_kernel(lname), preds, gt, valid, KEYWORDS[k])
    b = _run(_kernel(lname), preds, gt, valid, KEYWORDS[k])
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[2], b[2]))
    assert all((a[1][m] == b[1][m]) or (np.isnan(a[1][m]) and np.isnan(b[1][m])) for m in a[1])


@pytest.mark.parametrize("lname", ["seq", "epe"])
def test_one_copy_of_the_metrics_and_no_other_synchronisation(lname, monkeypatch):
    z = np.load(os.path.join(GOLDEN, "training_loss_a.npz"))
    gt = torch.from_numpy(z["gt"]).float().to(DEV)
    preds = [torch.from_numpy(z[f"pred{i}"]).float().to(DEV).requires_grad_(True) for i in range(5)]
    valid = torch.ones(2, 64, 128, device=DEV)
    fn = _kernel(lname)
    fn(preds, gt, valid, flowNetC=True)                       # library loaded, allocator warm
    calls = {"item": 0, "nonzero": 0, "cpu": 0, "sync": 0}
    item, nonzero, cpu, sync = torch.Tensor.item, torch.nonzero, torch.Tensor.cpu, torch.cuda.synchronize

    def counted(name, inner):
        def f(*a, **kw):
            calls[name] += 1
            return inner(*a, **kw)
        return f
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "item", counted("item", item))
        m.setattr(torch, "nonzero", counted("nonzero", nonzero))
        m.setattr(torch.Tensor, "nonzero", counted("nonzero", torch.Tensor.nonzero))
        m.setattr(torch.Tensor, "cpu", counted("cpu", cpu))
        m.setattr(torch.cuda, "synchronize", counted("sync", sync))
        loss, metrics = fn(preds, gt, valid, flowNetC=True)
        loss.backward()
    assert calls == {"item": 0, "nonzero": 0, "cpu": 1, "sync": 0}, calls
    assert all(p.grad is not None for p in preds)


def test_backward_scales_by_the_incoming_gradient():
    from understanding_flow_robustness_amd import training as T
    z = np.load(os.path.join(GOLDEN, "training_loss_b.npz"))
    gt = torch.from_numpy(z["gt"]).float().to(DEV)
    preds = [torch.from_numpy(z[f"pred{i}"]).float().to(DEV) for i in range(5)]
    valid = torch.ones(1, 16, 48, device=DEV)
    one = _run(T.sequence_loss, preds, gt, valid, dict(flowNetC=True))[2]
    leaves = [p.clone().requires_grad_(True) for p in preds]
    (T.sequence_loss(leaves, gt, valid, flowNetC=True)[0] * 0.25).backward()
    assert all(torch.equal(l.grad, g * 0.25) for l, g in zip(leaves, one))


def test_other_inputs_take_the_restatement(monkeypatch):
    """Ratios that are no integers, float64 and the RAFT branch never reach the kernel."""
    from understanding_flow_robustness_amd import training as T

    def refuse(*a, **kw):
        raise AssertionError("the kernel path ran")
    monkeypatch.setattr(T, "_loss_kernel", refuse)
    g = torch.Generator(device=DEV).manual_seed(0)
    gt = torch.randn(1, 2, 60, 100, device=DEV, generator=g)
    valid = torch.ones(1, 60, 100, device=DEV)
    loss, _ = T.sequence_loss([torch.randn(1, 2, 8, 13, device=DEV, generator=g)], gt, valid, flowNetC=True)
    assert torch.isfinite(loss)
    loss, _ = T.multiscale_epe([torch.randn(1, 2, 60, 100, device=DEV, generator=g)], gt, valid)          # RAFT
    assert torch.isfinite(loss)
    loss, _ = T.sequence_loss([torch.randn(1, 2, 30, 50, device=DEV, dtype=torch.float64)], gt.double(), valid, pwc=True)
    assert loss.dtype == torch.float64
