"""Golden fixtures of the training losses and the learning-rate schedule, produced by running the REFERENCE's own
`training/utils.py` (sequence_loss, multiscale_epe, fetch_optimizer) on the CPU in float64; see make_golden.py for the contract.

    python tests/golden/make_golden_training.py

Run only where the reference is mounted (ref_harness.REF).  The modules `training.utils` imports and this box lacks
(`tensorboard`, `torch.utils.tensorboard`, `dataset_utils.*`) are stubbed here; the loss functions never touch them.
Only arrays are stored: inputs, losses, metrics and the gradient of every prediction (tests/golden/training_loss_<case>.npz: the inputs; training_loss_<case>_<keyword set>.npz: the results).

Loss cases, each for both losses and for the keyword sets `flowNetC`, `pwc`, `flowNetC + flownetc_weighing + div_flow=20`:
  a  ground truth 2x2x64x128, predictions 64x128 .. 4x8, a NaN block in pair 0 and one NaN in one channel of pair 1
  b  ground truth 1x2x16x48, predictions down to 1x3 (ratio 16, rows of 3)
  c  an all-NaN ground truth 1x2x16x32 (the empty mean of sequence_loss; multiscale_epe skips every scale, after which the
     reference itself raises: it calls `.float()` on the Python float it started from -- recorded as `raised`)
  d  the RAFT branch: three full-size predictions, no NaN
  e  ground truth 60x100: ratios that are no integers
"""
from __future__ import annotations

import importlib
import os
import sys
import types
import warnings
from argparse import Namespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ref_harness import REF  # noqa: E402  (where the reference is mounted)

KEYWORDS = {"fnc": dict(flowNetC=True), "pwc": dict(pwc=True), "fncw": dict(flowNetC=True, flownetc_weighing=True, div_flow=20)}


def reference_utils():
    """The reference's training.utils, imported from where it lies, with the modules missing offline stubbed."""
    def stub(name, **attrs):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
        return sys.modules[name]
    try:
        importlib.import_module("torch.utils.tensorboard")
    except Exception:
        stub("tensorboard")
        tb = stub("torch.utils.tensorboard", SummaryWriter=object)
        torch.utils.tensorboard = tb
    du = stub("dataset_utils")
    du.__path__ = []
    for sub in ("custom_transforms", "datasets", "kitti_datasets"):
        setattr(du, sub, stub("dataset_utils." + sub))
    sys.path.insert(0, REF)
    return importlib.import_module("training.utils")


def pyramid_case(B, H, W, sizes, seed, nan=None):
    g = torch.Generator().manual_seed(seed)
    gt = torch.randn(B, 2, H, W, generator=g, dtype=torch.float64) * 3.0
    if nan == "some":
        gt[0, :, 5:9, 17:30] = float("nan")
        gt[1, 1, 40, 77] = float("nan")
    elif nan == "all":
        gt[:] = float("nan")
    preds = [torch.randn(B, 2, h, w, generator=g, dtype=torch.float64) * 2.0 for h, w in sizes]
    return gt, preds, torch.ones(B, H, W, dtype=torch.float64)


CASES = {
    "a": lambda: pyramid_case(2, 64, 128, [(64, 128), (32, 64), (16, 32), (8, 16), (4, 8)], 11, "some"),
    "b": lambda: pyramid_case(1, 16, 48, [(16, 48), (8, 24), (4, 12), (2, 6), (1, 3)], 12),
    "c": lambda: pyramid_case(1, 16, 32, [(16, 32), (8, 16), (4, 8)], 13, "all"),
    "e": lambda: pyramid_case(1, 60, 100, [(15, 25), (8, 13), (4, 7)], 15),
}


def run(fn, gt, preds, valid, kw):
    preds = [p.clone().requires_grad_(True) for p in preds]
    out = dict(raised=np.array(0))
    try:
        loss, metrics = fn(preds, gt.clone(), valid, **kw)
    except AttributeError:                    # multiscale_epe without a single term: 0.0.float()
        out["raised"] = np.array(1)
        return out
    out["loss"] = np.array(float(loss), dtype=np.float64)
    for k, v in metrics.items():
        out["metric_" + k] = np.array(v, dtype=np.float64)
    if torch.is_tensor(loss) and loss.requires_grad:
        loss.backward()
    for i, p in enumerate(preds):
        out[f"grad{i}"] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
    return out


def main():
    U = reference_utils()
    for case, make in CASES.items():
        gt, preds, valid = make()
        if case == "a":
            for h, w in [p.shape[-2:] for p in preds]:
                share = float(torch.isnan(torch.nn.functional.interpolate(gt, (h, w), mode="area")).double().mean())
                assert 0 < share <= 0.10, (h, w, share)
                print(f"case a: {100 * share:.2f} % of the {h} x {w} ground truth is NaN")
        np.savez_compressed(os.path.join(HERE, f"training_loss_{case}.npz"), gt=gt.numpy(), valid=valid.numpy(),
                            **{f"pred{i}": p.numpy() for i, p in enumerate(preds)})
        for kname, kw in KEYWORDS.items():                  # one file per keyword set: every committed file stays under 1 MiB
            blob = {}
            for lname, fn in (("seq", U.sequence_loss), ("epe", U.multiscale_epe)):
                for k, v in run(fn, gt, preds, valid, kw).items():
                    blob[f"{lname}_{k}"] = v
            np.savez_compressed(os.path.join(HERE, f"training_loss_{case}_{kname}.npz"), **blob)
    # d: the RAFT branch
    g = torch.Generator().manual_seed(14)
    gt = torch.randn(2, 2, 24, 40, generator=g, dtype=torch.float64) * 3.0
    gt[0, :, 3, 4] = 500.0                                       # beyond max_flow: excluded by the mask
    valid = (torch.rand(2, 24, 40, generator=g) > 0.2).double()
    preds = [torch.randn(2, 2, 24, 40, generator=g, dtype=torch.float64) * 2.0 for _ in range(3)]
    np.savez_compressed(os.path.join(HERE, "training_loss_d.npz"), gt=gt.numpy(), valid=valid.numpy(),
                        **{f"pred{i}": p.numpy() for i, p in enumerate(preds)})
    blob = {}
    for lname, fn in (("seq", U.sequence_loss), ("epe", U.multiscale_epe)):
        for k, v in run(fn, gt, preds, valid, {}).items():
            blob[f"{lname}_{k}"] = v
    np.savez_compressed(os.path.join(HERE, "training_loss_d_raft.npz"), **blob)
    # the learning-rate schedule of fetch_optimizer(lr=1e-4, num_steps=100, inner_iteration=1)
    model = torch.nn.Linear(3, 2)
    opt, sched = U.fetch_optimizer(Namespace(lr=1e-4, wdecay=1e-4, epsilon=1e-8, num_steps=100), model, 1)
    lrs = []
    for i in range(200):
        lrs.append(sched.get_last_lr()[0])
        opt.step()
        if i < 199:                           # the schedule has exactly 200 values
            sched.step()
    np.savez_compressed(os.path.join(HERE, "training_lr.npz"), first=np.array(lrs[:12]), last=np.array(lrs[-3:]), total=np.array(200))


if __name__ == "__main__":
    main()
