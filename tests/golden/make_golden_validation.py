"""Fixtures of the validation (understanding_flow_robustness_amd/validation.py), produced by running the REFERENCE's
training/evaluate.py:270-392 on the CPU (see make_golden.py for the contract): `datasets.FlyingChairs`, `MpiSintel` and `KITTI` are
replaced with list datasets of seeded items (tests/validation_standin.py), the three functions run as they are, and what they return
and print is recorded.  Frames are not stored.  For the small stand-in cases the per-item error arrays the functions concatenate are
stored too; for the real networks the ground truth is built from the reference's prediction averaged over 8 x 8 blocks (stored)
plus seeded noise.  validation_input_padder.json holds `InputPadder._pad` for every (H, W) in 1..40 x 1..40, both modes.

Every set is checked here before it is written: each rate (1px, 3px, 5px, KITTI's outlier share) lies in [0.1, 0.9], KITTI's valid
masks hold 30 % to 70 % ones (but for the item without a valid pixel), and at most 0.1 % of a set's entries lie within a relative
1e-4 of a threshold."""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys
from argparse import Namespace

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import save  # noqa: E402
import ref_harness as rh  # noqa: E402
import validation_standin as S  # noqa: E402
from understanding_flow_robustness_amd.flownets.weights import state_dict_digest, synthetic_state_dict  # noqa: E402


class ListDataset(torch.utils.data.Dataset):
    """Unbatched items; the reference's DataLoader(batch_size=1) puts the batch axis back."""

    def __init__(self, items):
        self.items = [tuple(x[0] for x in item) for item in items]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


class RecordingNumpy:
    """numpy for training/evaluate.py, with the lists it concatenates kept."""

    def __init__(self):
        self.concatenated = []

    def __getattr__(self, name):
        return getattr(np, name)

    def concatenate(self, arrays, *a, **k):
        self.concatenated.append([np.array(x) for x in arrays])
        return np.concatenate(arrays, *a, **k)


class RecordingModel(torch.nn.Module):
    """The network with its inputs' shapes and its outputs kept (the flow in either calling convention)."""

    def __init__(self, net):
        super().__init__()
        self.net, self.flows, self.shapes = net, [], []

    def forward(self, *args, **kwargs):
        out = self.net(*args, **kwargs)
        self.shapes.append(tuple(args[0].shape))
        self.flows.append((out[1] if isinstance(out, tuple) else out).detach().clone())
        return out


def run_reference(ev, validator, model, flowNetC, items, iters):
    """-> (the returned dict or the exception, the printed text, the concatenated lists, the model's flows)."""
    sets = items if isinstance(items, dict) else {None: items}
    ev.datasets.FlyingChairs = lambda **k: ListDataset(sets[None])
    ev.datasets.KITTI = lambda **k: ListDataset(sets[None])
    ev.datasets.MpiSintel = lambda split, dstype: ListDataset(sets[dstype])
    ev.np = rec = RecordingNumpy()
    wrapped = RecordingModel(model)
    fn = getattr(ev, "validate_" + validator)
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            results = fn(wrapped, flowNetC=True) if flowNetC else fn(wrapped, iters)
    except ValueError as e:
        results = e
    finally:
        ev.np = np
    return results, out.getvalue(), rec.concatenated, wrapped


def check_rates(name, entries, outliers=None):
    entries = np.asarray(entries)
    rates = {"1px": float(np.mean(entries < 1)), "3px": float(np.mean(entries < 3)), "5px": float(np.mean(entries < 5))}
    if outliers is not None:
        rates["outliers"] = float(np.mean(outliers))
    bad = {k: v for k, v in rates.items() if not 0.1 <= v <= 0.9}
    assert not bad, f"{name}: rates outside [0.1, 0.9]: {bad} (all: {rates})"
    near = S.near_threshold(entries, (1.0, 3.0, 5.0), 1e-4)
    assert near <= 1e-3 * entries.size, f"{name}: {near} of {entries.size} entries within 1e-4 of a threshold"
    return rates


def kitti_entries(ev, wrapped, items, flowNetC):
    """The per-pixel arrays validate_kitti does not keep: restated from the recorded flows with the reference's padder."""
    padder_cls = rh.ref_module("models.raft.utils.utils").InputPadder
    kept = [it for it in items if not flowNetC or sum(padder_cls(it[0].shape, mode="kitti")._pad[2:]) + it[0].shape[-2] == 384]
    epes, ratios, vals = [], [], []
    for (image1, _, flow_gt, valid), flow_pr in zip(kept, wrapped.flows):
        flow = padder_cls(image1.shape, mode="kitti").unpad(flow_pr[0])
        epe = torch.sum((flow - flow_gt[0]) ** 2, dim=0).sqrt().view(-1)
        mag = torch.sum(flow_gt[0] ** 2, dim=0).sqrt().view(-1)
        val = valid[0].view(-1) >= 0.5
        epes.append(epe.numpy())
        ratios.append((epe / mag)[val & (epe > 3.0)].numpy())
        vals.append(val.numpy())
    return epes, ratios, vals


def record(name, ev, validator, model, flowNetC, items, iters, arrays, extra=None):
    results, printed, lists, wrapped = run_reference(ev, validator, model, flowNetC, items, iters)
    meta = {"validator": validator, "flowNetC": flowNetC, "printed": printed, "calls": wrapped.shapes}
    out = dict(extra or {})
    if isinstance(results, Exception):
        meta["raises"] = [type(results).__name__, str(results)]
    else:
        meta["results"] = {k: float(v) for k, v in results.items()}
        meta["result_dtypes"] = {k: type(v).__name__ for k, v in results.items()}
        meta["keys"] = list(results)
        if validator == "kitti":
            epes, ratios, vals = kitti_entries(ev, wrapped, items, flowNetC)
            outliers = lists[0]                                        # out[val] per item
            flat = np.concatenate(outliers)
            finite = np.concatenate([e for e, v in zip(epes, vals)])
            meta["rates"] = {"kitti": check_rates(name, finite, flat if flat.size else None)}
            meta["near"] = {"kitti": {str(rel): S.near_threshold(finite, (1.0, 3.0, 5.0), rel)
                                      + S.near_threshold(np.concatenate(ratios), (0.05,), rel) for rel in (1e-4, 1e-3, 1e-2)}}
            meta["entries"] = {"kitti": int(finite.size)}
            meta["valid_counts"] = [int(v.sum()) for v in vals]
            meta["outlier_counts"] = [int(o.sum()) for o in outliers]
            for v in vals:
                assert v.sum() == 0 or 0.3 <= v.mean() <= 0.7, f"{name}: valid share {v.mean()}"
            # per item: the float32 mean over the valid pixels as validate_kitti takes it (NaN for an item without one)
            out["kitti_epe_list"] = np.array([torch.as_tensor(e)[torch.as_tensor(v)].mean().item() for e, v in zip(epes, vals)])
            if arrays:
                out["kitti_entries"] = np.concatenate(epes).astype(np.float32)
        else:
            sets = ["chairs"] if validator == "chairs" else ["clean", "final"]
            meta["rates"], meta["near"], meta["entries"] = {}, {}, {}
            for key, per_item in zip(sets, lists):
                flat = np.concatenate(per_item)
                meta["rates"][key] = check_rates(f"{name}/{key}", flat)
                meta["near"][key] = {str(rel): S.near_threshold(flat, (1.0, 3.0, 5.0), rel) for rel in (1e-4, 1e-3, 1e-2)}
                meta["entries"][key] = int(flat.size)
                meta["rates"][key]["epe"] = float(np.mean(flat))
                if arrays:
                    out[f"entries_{key}"] = flat.astype(np.float32)
    out["meta"] = np.array(json.dumps(meta))
    save("validation_" + name, **out)
    print(name, meta.get("results", meta.get("raises")), meta.get("rates"))


def gen_padder():
    padder_cls = rh.ref_module("models.raft.utils.utils").InputPadder
    table = {mode: [[list(map(int, padder_cls((1, 3, h, w), mode=mode)._pad)) for w in range(1, 41)] for h in range(1, 41)]
             for mode in ("sintel", "kitti")}
    path = os.path.join(HERE, "validation_input_padder.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"doc": "InputPadder((1,3,H,W), mode)._pad = table[mode][H-1][W-1], H and W in 1..40", "table": table}, f,
                  separators=(",", ":"))
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


def gen_standin(ev):
    for name, (validator, flowNetC, gain, specs) in S.STANDIN_CASES.items():
        make = lambda sp: S.standin_items(sp, gain=gain, flowNetC=flowNetC)
        items = {k: make(v) for k, v in specs.items()} if isinstance(specs, dict) else make(specs)
        arrays = name in ("chairs", "sintel", "kitti_finite")
        record("standin_" + name, ev, validator, S.StandIn(gain).eval(), flowNetC, items, S.RAFT_ITERS, arrays)


def _coarse(ev, validator, model, flowNetC, specs, iters):
    """The reference's clean prediction of every item (pad, forward, unpad as the validator does), averaged over 8 x 8 blocks."""
    padder_cls = rh.ref_module("models.raft.utils.utils").InputPadder
    out = []
    for seed, H, W, _ in specs:
        image1, image2 = S.blocky_frames(seed, H, W)
        padder = padder_cls(image1.shape, **({"mode": "kitti"} if validator == "kitti" else {}))
        a, b = padder.pad(image1, image2) if validator != "chairs" else (image1, image2)
        with torch.no_grad():
            flow = model(a / 255.0, b / 255.0) if flowNetC else model(a, b, iters=iters, test_mode=True)[1]
        flow = padder.unpad(flow) if validator != "chairs" else flow
        out.append(F.avg_pool2d(flow, 8, ceil_mode=True)[0].numpy().astype(np.float16))
    return np.stack(out)


def gen_models(ev, scales):
    raft = rh.ref_module("models.raft.raft")
    args = Namespace(flownet="RAFT", small=False, mixed_precision=False, alternate_corr=False, fnorm="instance", cnorm="batch",
                     no_separate_context=False, corr_levels=4, iters=S.RAFT_ITERS, flowNetCEnc=False,
                     update_no_motion_downsampling=False)
    nets = {}
    net = raft.RAFT(args).eval()
    sd = synthetic_state_dict(net.state_dict(), seed=2)
    net.load_state_dict(sd)
    nets[False] = (net, state_dict_digest(sd), 2)
    net = rh.ref_module("models.FlowNetC").FlowNetC().eval()
    sd = synthetic_state_dict(net.state_dict(), seed=0)
    net.load_state_dict(sd)
    nets[True] = (net, state_dict_digest(sd), 0)
    for name, (validator, flowNetC, specs) in S.MODEL_CASES.items():
        model, digest, seed = nets[flowNetC]
        sets = specs if isinstance(specs, dict) else {None: specs}
        coarse = {k: _coarse(ev, validator, model, flowNetC, v, S.RAFT_ITERS) for k, v in sets.items()}
        items = {k: S.coarse_items(v, coarse[k], scales[name]) for k, v in sets.items()}
        extra = {("coarse_" + k if k else "coarse"): c for k, c in coarse.items()}
        extra.update(weight_digest=digest, weight_seed=seed, noise_scale=scales[name])
        record(name, ev, validator, model, flowNetC, items if isinstance(specs, dict) else items[None], S.RAFT_ITERS, False, extra)


if __name__ == "__main__":
    rh.install()
    torch.manual_seed(0)
    ev = rh.ref_module("training.evaluate")
    gen_padder()
    gen_standin(ev)
    gen_models(ev, {"raft_sintel": 2.0, "raft_kitti": 2.0, "flownetc_chairs": 3.0})
