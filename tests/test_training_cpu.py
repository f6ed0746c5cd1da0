"""`understanding_flow_robustness_amd.training` without a GPU: the plain-torch restatement of the reference's two training losses
reproduces the float64 fixtures the reference itself produced (tests/golden/make_golden_training.py: losses, metrics, the gradient
of every prediction, NaN quirks included), `fetch_optimizer` gives the reference's learning-rate sequence, `ClippedAdamW` exchanges
state dicts with `torch.optim.AdamW`, and what it does not implement raises."""
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

from understanding_flow_robustness_amd import training as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYWORDS = {"fnc": dict(flowNetC=True), "pwc": dict(pwc=True), "fncw": dict(flowNetC=True, flownetc_weighing=True, div_flow=20),
            "raft": dict()}
CASES = [(c, k) for c in "abce" for k in ("fnc", "pwc", "fncw")] + [("d", "raft")]
LOSSES = {"seq": T.sequence_loss, "epe": T.multiscale_epe}
TOL = 1e-12


def load(case, kname):
    z = np.load(os.path.join(GOLDEN, f"training_loss_{case}.npz"))
    r = np.load(os.path.join(GOLDEN, f"training_loss_{case}_{kname}.npz"))
    preds = [torch.from_numpy(z[f"pred{i}"]) for i in range(sum(k.startswith("pred") for k in z.files))]
    return torch.from_numpy(z["gt"]), torch.from_numpy(z["valid"]), preds, r


def close(got, want, what):
    if np.isnan(want):
        assert np.isnan(got), f"{what}: {got}, the reference gives NaN"
    else:
        assert abs(got - want) <= TOL * max(abs(want), 1e-300), f"{what}: {got} vs {want}"


@pytest.mark.parametrize("lname", ["seq", "epe"])
@pytest.mark.parametrize("case,kname", CASES, ids=[f"{c}-{k}" for c, k in CASES])
def test_the_restatement_reproduces_the_reference(case, kname, lname):
    gt, valid, preds, r = load(case, kname)
    preds = [p.clone().requires_grad_(True) for p in preds]
    loss, metrics = LOSSES[lname](preds, gt.clone(), valid, **KEYWORDS[kname])
    if int(r[f"{lname}_raised"]):
        # multiscale_epe on an all-NaN ground truth: every scale is skipped, after which the reference calls .float() on a Python
        # float and raises.  Here the step reports a zero loss that depends on nothing.
        assert lname == "epe" and case == "c"
        assert float(loss) == 0.0 and not loss.requires_grad and metrics["loss"] == 0.0 and np.isnan(metrics["epe"])
        return
    close(float(loss), float(r[f"{lname}_loss"]), "loss")
    assert set(metrics) == {k[len(lname) + 8:] for k in r.files if k.startswith(f"{lname}_metric_")}
    for k, v in metrics.items():
        assert isinstance(v, float)
        close(v, float(r[f"{lname}_metric_{k}"]), f"metric {k}")
    loss.backward()
    for i, p in enumerate(preds):
        want = r[f"{lname}_grad{i}"]
        got = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"grad{i}: NaN positions differ"
        scale = np.nanmax(np.abs(want)) if np.isfinite(want).any() else 0.0
        assert np.nanmax(np.abs(got - want), initial=0.0) <= TOL * scale, f"grad{i}"
        assert np.array_equal(got == 0, want == 0), f"grad{i}: the exact zeros differ"


def test_the_nan_quirks_of_the_fixture_are_the_ones_written_down():
    """sequence_loss: gradient exactly 0 where the interpolated ground truth is NaN, finite elsewhere; multiscale_epe: NaN in both
    channels of every pixel whose interpolated ground truth has a NaN in either."""
    gt, _, preds, r = load("a", "fnc")
    for i, p in enumerate(preds):
        nan = torch.isnan(torch.nn.functional.interpolate(gt, p.shape[-2:], mode="area")).numpy()
        assert 0 < nan.mean() <= 0.10
        seq, epe = r[f"seq_grad{i}"], r[f"epe_grad{i}"]
        assert np.isfinite(seq).all() and (seq[nan] == 0).all() and (seq[~nan] != 0).all()
        either = nan.any(axis=1, keepdims=True).repeat(2, axis=1)
        assert np.array_equal(np.isnan(epe), either)


def test_pwc_alone_weighs_the_scales_like_raft_in_sequence_loss_only():
    gt, valid, preds, _ = load("b", "fnc")
    n = len(preds)
    terms = [float(T.sequence_loss([p], gt, valid, flowNetC=True)[0]) for p in preds]
    assert float(T.sequence_loss(preds, gt, valid, pwc=True)[0]) == pytest.approx(sum(0.8 ** (n - i - 1) * t for i, t in enumerate(terms)), rel=1e-12)
    assert float(T.sequence_loss(preds, gt, valid, flowNetC=True)[0]) == pytest.approx(sum(0.8 ** i * t for i, t in enumerate(terms)), rel=1e-12)
    assert float(T.multiscale_epe(preds, gt, valid, pwc=True)[0]) == float(T.multiscale_epe(preds, gt, valid, flowNetC=True)[0])


def test_fetch_optimizer_gives_the_reference_learning_rates():
    z = np.load(os.path.join(GOLDEN, "training_lr.npz"))
    model = torch.nn.Linear(3, 2)
    opt, sched = T.fetch_optimizer(Namespace(lr=1e-4, wdecay=1e-4, epsilon=1e-8, num_steps=100), model, 1)
    assert isinstance(opt, T.ClippedAdamW) and isinstance(sched, torch.optim.lr_scheduler.OneCycleLR)
    g = opt.param_groups[0]
    assert g["weight_decay"] == 1e-4 and g["eps"] == 1e-8 and g["betas"] == (0.9, 0.999) and sched.total_steps == 200
    lrs = []
    for i in range(int(z["total"])):                       # no gradient anywhere: step() has nothing to do and needs no GPU
        lrs.append(sched.get_last_lr()[0])
        opt.step()
        if i < int(z["total"]) - 1:
            sched.step()
    assert np.array_equal(np.array(lrs[:12]), z["first"]) and np.array_equal(np.array(lrs[-3:]), z["last"])
    opt2, sched2 = T.fetch_optimizer(Namespace(lr=1e-4, wdecay=1e-4, epsilon=1e-8, num_steps=100), model, 3)
    assert sched2.total_steps == 400


def _stepped_adamw(cls=torch.optim.AdamW):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(5, 4), torch.nn.Linear(4, 2))
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, eps=1e-8)
    for _ in range(2):
        opt.zero_grad()
        model(torch.randn(3, 5)).square().sum().backward()
        opt.step()
    return model, opt


def test_state_dicts_interchange_with_torch_adamw():
    model, ref = _stepped_adamw()
    sd = ref.state_dict()
    mine = T.ClippedAdamW(model.parameters(), lr=5e-2)
    mine.load_state_dict(sd)                                 # a reference checkpoint's optimizer_state_dict (train.py:122)
    assert mine.param_groups[0]["lr"] == 1e-3 and mine.param_groups[0]["weight_decay"] == 1e-4
    for p in model.parameters():
        assert set(mine.state[p]) == {"step", "exp_avg", "exp_avg_sq"} and float(mine.state[p]["step"]) == 2.0
        assert torch.equal(mine.state[p]["exp_avg"], ref.state[p]["exp_avg"])
    back = torch.optim.AdamW(model.parameters())
    back.load_state_dict(mine.state_dict())                  # and the other way round
    assert back.state_dict()["param_groups"] == sd["param_groups"]
    for a, b in zip(back.state_dict()["state"].values(), sd["state"].values()):
        assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    model(torch.randn(3, 5)).square().sum().backward()
    back.step()                                              # torch steps on from the state that went through ClippedAdamW
    assert float(back.state[next(model.parameters())]["step"]) == 3.0


@pytest.mark.parametrize("option", ["amsgrad", "maximize", "capturable", "differentiable", "fused"])
def test_unsupported_options_raise_at_construction(option):
    with pytest.raises(NotImplementedError, match=option):
        T.ClippedAdamW(torch.nn.Linear(2, 2).parameters(), **{option: True})


def test_unsupported_parameters_raise_at_the_step():
    lin = torch.nn.Linear(2, 2)                              # a CPU parameter
    lin(torch.ones(1, 2)).sum().backward()
    opt = T.ClippedAdamW(lin.parameters())
    with pytest.raises(NotImplementedError, match="HIP float32"):
        opt.step(clip=1.0)
    emb = torch.nn.Embedding(4, 3, sparse=True)
    emb(torch.tensor([1, 2])).sum().backward()
    with pytest.raises(NotImplementedError, match="sparse"):
        T.ClippedAdamW(emb.parameters()).step()
    half = torch.nn.Linear(2, 2).to(torch.float64)
    half(torch.ones(1, 2, dtype=torch.float64)).sum().backward()
    with pytest.raises(NotImplementedError, match="float64"):
        T.ClippedAdamW(half.parameters()).step()
    lin2 = torch.nn.Linear(2, 2)
    lin2(torch.ones(1, 2)).sum().backward()
    late = T.ClippedAdamW(lin2.parameters())
    late.param_groups[0]["amsgrad"] = True                   # what a loaded state dict can switch on
    with pytest.raises(NotImplementedError, match="amsgrad"):
        late.step()


def test_the_package_imports_without_a_gpu():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    code = ("import torch, understanding_flow_robustness_amd.training as T; "
            "assert not torch.cuda.is_available(); "
            "print(sorted(n for n in ('sequence_loss', 'multiscale_epe', 'ClippedAdamW', 'fetch_optimizer', 'finetune_step') if hasattr(T, n)))")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "['ClippedAdamW', 'fetch_optimizer', 'finetune_step', 'multiscale_epe', 'sequence_loss']"


def test_finetune_step_runs_on_torch_operators_with_any_optimizer():
    """The step's plumbing on the CPU: a toy two-scale model, torch's AdamW, the restatement of the loss; a NaN loss returns before
    the backward and leaves the parameters alone."""
    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.c = torch.nn.Conv2d(6, 2, 3, 1, 1)

        def forward(self, a, b):
            y = self.c(torch.cat((a, b), 1))
            return y, torch.nn.functional.avg_pool2d(y, 2)
    torch.manual_seed(0)
    net = Toy()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, 1e-3, 10)
    args = Namespace(flowNetC=True, adv_train=True, clip=1.0, gamma=0.8)
    x1, x2, flow = torch.rand(1, 3, 8, 16), torch.rand(1, 3, 8, 16), torch.randn(1, 2, 8, 16)
    before = net.c.weight.detach().clone()
    loss, metrics = T.finetune_step(net, opt, sched, x1, x2, flow, torch.ones(1, 8, 16), args)
    assert torch.isfinite(loss) and set(metrics) == {"epe", "1px", "3px", "5px"} and not torch.equal(net.c.weight, before)
    after = net.c.weight.detach().clone()
    loss, _ = T.finetune_step(net, opt, sched, x1, x2, torch.full_like(flow, float("nan")), torch.ones(1, 8, 16), args)
    assert torch.isnan(loss) and torch.equal(net.c.weight, after)
    args.multiscaleEPE = True
    loss, metrics = T.finetune_step(net, opt, sched, x1, x2, flow, torch.ones(1, 8, 16), args)
    assert "loss" in metrics and metrics["loss"] == pytest.approx(float(loss))
