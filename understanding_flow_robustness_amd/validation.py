"""The validation of the fine-tuning loop: `validate_chairs`, `validate_sintel` and `validate_kitti` of training/evaluate.py:270-392,
`InputPadder` of models/raft/utils/utils.py:7-30 and the dispatcher of training/train.py:302-324.

Reference, per item: a replicate pad through `F.pad`, one batch-1 forward, the prediction copied to the host, a per-pixel error
array kept in a Python list; `np.concatenate` and `np.mean` over the whole set at the end.  Here (`fused=True`) up to `chunk`
consecutive items of equal sizes are stacked, and per chunk

    ONE ufr_validation_pad (csrc/validation.hip)  ->  ONE forward of the K pairs  ->  ONE ufr_validation_metrics

run; the host reads the [N,8] float64 table once per call.  No prediction, error array or mask reaches the host.  `fused=False` is
the reference's loop as written, in torch and numpy, on whatever device the items are on.

The datasets are the caller's: every validator takes its loader(s) as a keyword.  Items are what the reference's
`DataLoader(batch_size=1)` yields: `(image1, image2, flow_gt, valid)`, frames [1,3,H,W] in 0..255, flow_gt [1,2,H,W], valid [1,H,W].
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib as L
from .chunked_eval import ChunkedEval, check_pair

COLS = 8             # UFR_VALIDATION_COLS (include/ufr_hip.h)
MODE_EPE, MODE_COMPONENTS, MODE_CHANNEL0 = 0, 1, 2


class InputPadder:
    """Pads images such that dimensions are divisible by 8 (models/raft/utils/utils.py:7-30, member for member)."""

    def __init__(self, dims, mode="sintel"):
        self.ht, self.wd = dims[-2:]
        pad_ht = (((self.ht // 8) + 1) * 8 - self.ht) % 8
        pad_wd = (((self.wd // 8) + 1) * 8 - self.wd) % 8
        if mode == "sintel":
            self._pad = [pad_wd // 2, pad_wd - pad_wd // 2, pad_ht // 2, pad_ht - pad_ht // 2]
        else:
            self._pad = [pad_wd // 2, pad_wd - pad_wd // 2, 0, pad_ht]

    def pad(self, *inputs):
        return [F.pad(x, self._pad, mode="replicate") for x in inputs]

    def unpad(self, x):
        ht, wd = x.shape[-2:]
        c = [self._pad[2], ht - self._pad[3], self._pad[0], wd - self._pad[1]]
        return x[..., c[0]:c[1], c[2]:c[3]]


class ValidationResults(dict):
    """The reference's result dict, key for key; `details` holds what the reference only prints (per set: the error mean over all
    entries, the 1px / 3px / 5px rates and the number of entries) and, for KITTI, the per-item end-point errors and the numbers of
    valid pixels and of outliers among them."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.details = {}

    def update(self, other=(), **kwargs):
        super().update(other, **kwargs)
        self.details.update(getattr(other, "details", {}))


def _need(loader, what):
    if loader is None:
        raise ValueError(f"{what}: the datasets are the caller's -- pass the loader whose items are the reference's batch-1 "
                         "(image1, image2, flow_gt, valid)")
    return loader


def _forward(model, image1, image2, iters, flowNetC):
    """The reference's two calls (evaluate.py:286-289); the division by 255 of the FlowNetC call is the caller's.  (RAFT itself
    reads its iteration count from its own `args.iters` and ignores the argument, models/raft/raft.py:126, here as there.)"""
    if flowNetC:
        return model(image1, image2)
    return model(image1, image2, iters=iters, test_mode=True)[1]


def _rates(epe_all):
    return {"epe": np.mean(epe_all), "1px": np.mean(epe_all < 1), "3px": np.mean(epe_all < 3), "5px": np.mean(epe_all < 5),
            "entries": int(epe_all.size)}


# ---- fused: chunks of stacked items, one table on the device -------------------------------------------------------------------
class _Chunks(ChunkedEval):
    """The chunk's pad, forward and metrics launch (chunked_eval.py: the waiting items, the result rows on the device)."""

    def __init__(self, model, iters, flowNetC, pad_mode, metric_mode, chunk):
        super().__init__(chunk)
        self.model, self.iters, self.flowNetC = model, iters, bool(flowNetC)
        self.pad_mode, self.metric_mode = pad_mode, metric_mode

    def add(self, image1, image2, flow_gt, valid):
        check_pair(image1, image2, "the loader yields batch-1 items: image1 and image2 [1,3,H,W]")
        if flow_gt.dim() != 4 or flow_gt.shape[0] != 1 or flow_gt.shape[1] != 2:
            raise ValueError("flow_gt must be [1,2,H,W]")
        if tuple(flow_gt.shape[2:]) != tuple(image1.shape[2:]):
            raise ValueError(f"flow_gt is {tuple(flow_gt.shape[2:])}, the frames are {tuple(image1.shape[2:])}")
        if valid is not None and tuple(valid.shape) != (1,) + tuple(flow_gt.shape[2:]):
            raise ValueError("valid must be [1,H,W]")
        super().add((tuple(image1.shape), tuple(flow_gt.shape), image1.device, valid is None), image1, image2, flow_gt, valid)

    def run_chunk(self, items):
        K = len(items)
        dev = items[0][1].device
        image1, image2, gt = (self.stack_f32([it[i] for it in items], dev) for i in (1, 2, 3))
        valid = self.stack_f32([it[4] for it in items], dev) if items[0][4] is not None else None
        H, W = int(image1.shape[2]), int(image1.shape[3])
        left, right, top, bottom = InputPadder(image1.shape, mode=self.pad_mode)._pad if self.pad_mode else (0, 0, 0, 0)
        lib = L.lib()
        self._mark("start")
        if self.flowNetC or top or bottom or left or right:
            pad1, pad2 = (torch.empty(K, 3, H + top + bottom, W + left + right, dtype=torch.float32, device=dev) for _ in range(2))
            L.check(lib.ufr_validation_pad(L.ptr(image1), L.ptr(image2), L.ptr(pad1), L.ptr(pad2), K, H, W, top, bottom, left, right,
                                           1 if self.flowNetC else 0, L.stream()), "validation pad")
        else:
            pad1, pad2 = image1, image2          # chairs through RAFT: the pad is the identity and nothing is divided
        self._mark("pad")
        flow = self.checked_flow(_forward(self.model, pad1, pad2, self.iters, self.flowNetC), K, H, W).to(torch.float32).contiguous()
        Hp, Wp = int(flow.shape[2]), int(flow.shape[3])
        self._mark("forward")
        ws = self.workspace(lib.ufr_validation_metrics_workspace_doubles(self.chunk, H, W), dev)
        out = torch.zeros(K, COLS, dtype=torch.float64, device=dev)
        L.check(lib.ufr_validation_metrics(L.ptr(flow), L.ptr(gt), L.ptr(valid) if valid is not None else None, K, Hp, Wp, top, left,
                                           H, W, self.metric_mode, L.ptr(ws), ws.numel(), L.ptr(out), 0, K, L.stream()),
                "validation metrics")
        self._mark("metrics")
        return out

    def read(self):
        """The one host synchronisation: the [N,8] table in loader order."""
        table = super().read()
        return table[0] if table else np.zeros((0, COLS))


def _fused_table(model, loader, iters, flowNetC, pad_mode, metric_mode, chunk, skip=None):
    model.eval()
    ev = _Chunks(model, iters, flowNetC, pad_mode, metric_mode, chunk)
    ev.events = getattr(_fused_table, "_debug_events", None)      # tools/bench_validation.py: device events around the stages
    for item in loader:
        image1, image2, flow_gt, valid = item
        for t, name in ((image1, "image1"), (image2, "image2"), (flow_gt, "flow_gt")):
            L.require_hip(t, name, contiguous=False)
            if t.dtype != torch.float32:
                raise RuntimeError(f"{name} must be float32 (fused=True); fused=False runs the reference's loop on any tensor")
        if skip is not None and skip(image1):
            continue
        ev.add(image1, image2, flow_gt, valid if pad_mode == "kitti" else None)
    return ev.read()


def _set_rates(table):
    """Sums over the items of a set, in float64: (mean, 1px, 3px, 5px) over all entries."""
    if len(table) == 0:
        np.concatenate([])               # the reference's ValueError for a set without items
    n = table[:, 1].sum()
    return {"epe": table[:, 0].sum() / n, "1px": table[:, 2].sum() / n, "3px": table[:, 3].sum() / n, "5px": table[:, 4].sum() / n,
            "entries": int(n)}


# ---- the three validators --------------------------------------------------------------------------------------------------------
@torch.no_grad()
def validate_chairs(model, iters: int = 24, flowNetC: bool = False, *, loader=None, chunk: int = 4, fused: bool = True,
                    verbose: bool = True):
    """Perform evaluation on the FlyingChairs (test) split (evaluate.py:270-295): no padding, a true end-point error per pixel, the
    float32 mean over all pixels of all items."""
    _need(loader, "validate_chairs")
    model.eval()
    if fused:
        rates = _set_rates(_fused_table(model, loader, iters, flowNetC, None, MODE_EPE, chunk))
        epe = np.float32(rates["epe"])
    else:
        epe_list = []
        for test_data in loader:
            image1, image2, flow_gt, _ = test_data
            if flowNetC:
                flow_pr = model(image1 / 255.0, image2 / 255.0)
            else:
                _, flow_pr = model(image1, image2, iters=iters, test_mode=True)
            epe = torch.sum((flow_pr[0].cpu() - flow_gt[0].cpu()) ** 2, dim=0).sqrt()
            epe_list.append(epe.view(-1).numpy())
        epe_all = np.concatenate(epe_list)
        rates = _rates(epe_all)
        epe = np.mean(epe_all)
    if verbose:
        print(f"Validation Chairs EPE: {epe:.3f}")
    results = ValidationResults({"chairs": epe})
    results.details["chairs"] = rates
    return results


@torch.no_grad()
def validate_sintel(model, iters: int = 32, flowNetC: bool = False, *, loaders=None, chunk: int = 4, fused: bool = True,
                    verbose: bool = True):
    """Peform validation using the Sintel (train) split (evaluate.py:298-343), quirks included: `flow - flow_gt` keeps the batch
    axis, so `torch.sum(..., dim=0)` sums over ONE sample and the error array holds the absolute error of each component, 2*H*W
    entries per item; with `flowNetC` the extra `[0]` leaves the u channel of sample 0, compared against both ground-truth channels.
    `results[dstype] = np.mean(epe_list)`: items of different sizes raise numpy's ValueError, as in the reference."""
    _need(loaders, "validate_sintel")
    for dstype in ["clean", "final"]:
        _need(loaders.get(dstype), f"validate_sintel ({dstype})")
    model.eval()
    results = ValidationResults()
    for dstype in ["clean", "final"]:
        loader = loaders[dstype]
        if fused:
            table = _fused_table(model, loader, iters, flowNetC, "sintel", MODE_CHANNEL0 if flowNetC else MODE_COMPONENTS, chunk)
            rates = _set_rates(table)
            if len(set(table[:, 1].tolist())) > 1:
                np.mean([np.zeros(int(n)) for n in table[:, 1]])          # numpy's refusal of a ragged list (evaluate.py:341)
            mean = np.float32(rates["epe"])
        else:
            epe_list = []
            for data_blob in loader:
                image1, image2, flow_gt, _ = data_blob
                padder = InputPadder(image1.shape)
                image1, image2 = padder.pad(image1, image2)
                if flowNetC:
                    flow_pr = model(image1 / 255.0, image2 / 255.0)[0]
                else:
                    _, flow_pr = model(image1, image2, iters=iters, test_mode=True)
                flow = padder.unpad(flow_pr[0])
                epe = torch.sum((flow - flow_gt) ** 2, dim=0).sqrt()
                epe_list.append(epe.view(-1).cpu().numpy())
            epe_all = np.concatenate(epe_list)
            rates = _rates(epe_all)
            mean = np.mean(epe_list)
        if verbose:
            print("Validation (%s) EPE: %f, 1px: %f, 3px: %f, 5px: %f" % (dstype, rates["epe"], rates["1px"], rates["3px"], rates["5px"]))
        results[dstype] = mean
        results.details[dstype] = rates
    return results


@torch.no_grad()
def validate_kitti(model, iters: int = 24, flowNetC: bool = False, *, loader=None, chunk: int = 4, fused: bool = True,
                   verbose: bool = True):
    """Peform validation using the KITTI-2015 (train) split (evaluate.py:346-392): `mode="kitti"` pads at the bottom; with
    `flowNetC` items whose padded height is not 384 are skipped; per item the float32 mean of the end-point error over
    `valid >= 0.5` (NaN for an item without a valid pixel, and NaN propagates); `kitti-epe` is the float64 mean of those,
    `kitti-f1` 100 times the share of valid pixels with an error above 3 and above 5 % of the ground truth's magnitude."""
    _need(loader, "validate_kitti")
    model.eval()
    if fused:
        padded_height = lambda image1: image1.shape[-2] + sum(InputPadder(image1.shape, mode="kitti")._pad[2:])
        skip = (lambda image1: padded_height(image1) != 384) if flowNetC else None
        table = _fused_table(model, loader, iters, flowNetC, "kitti", MODE_EPE, chunk, skip=skip)
        rates = _set_rates(table)
        with np.errstate(invalid="ignore", divide="ignore"):
            epe_list = (table[:, 5] / table[:, 6]).astype(np.float32).astype(np.float64)
            f1 = np.float32(100 * (table[:, 7].sum() / table[:, 6].sum()))
        rates.update(valid=int(table[:, 6].sum()), outliers=int(table[:, 7].sum()))
    else:
        out_list, epe_list, all_list = [], [], []
        for val_data in loader:
            image1, image2, flow_gt, valid_gt = val_data
            padder = InputPadder(image1.shape, mode="kitti")
            image1, image2 = padder.pad(image1, image2)
            if flowNetC:
                if image1.shape[-2] != 384:
                    continue
                flow_pr = model(image1 / 255.0, image2 / 255.0)
            else:
                _, flow_pr = model(image1, image2, iters=iters, test_mode=True)
            flow = padder.unpad(flow_pr[0]).cpu()
            flow_gt, valid_gt = flow_gt.cpu(), valid_gt.cpu()
            epe = torch.sum((flow - flow_gt[0]) ** 2, dim=0).sqrt()
            mag = torch.sum(flow_gt[0] ** 2, dim=0).sqrt()
            epe = epe.view(-1)
            mag = mag.view(-1)
            val = valid_gt[0].view(-1) >= 0.5
            out = ((epe > 3.0) & ((epe / mag) > 0.05)).float()
            epe_list.append(epe[val].mean().item())
            out_list.append(out[val].cpu().numpy())
            all_list.append(epe.numpy())
        epe_list = np.array(epe_list)
        out_list = np.concatenate(out_list)
        rates = _rates(np.concatenate(all_list))
        rates.update(valid=int(out_list.size), outliers=int(out_list.sum()))
        f1 = 100 * np.mean(out_list)
    epe = np.mean(epe_list)
    if verbose:
        print(f"Validation KITTI: {epe:f}, {f1:f}")
    results = ValidationResults({"kitti-epe": epe, "kitti-f1": f1})
    results.details["kitti"] = dict(rates, epe_list=[float(e) for e in epe_list])
    return results


def validate(model, names, loaders, iters: int = 12, flowNetC: bool = False, **kwargs):
    """The dispatcher of training/train.py:302-324: `results.update` in the order of `names`; a name other than "chairs", "sintel"
    and "kitti" is ignored, as there.  `loaders` is {"chairs": loader, "sintel": {"clean": loader, "final": loader}, "kitti": loader}.
    With `flowNetC` the validators run with their own default `iters`, as the reference calls them."""
    results = ValidationResults()
    if names is None:
        return results
    for val_dataset in names:
        head = (model,) if flowNetC else (model, iters)
        if val_dataset == "chairs":
            results.update(validate_chairs(*head, flowNetC=flowNetC, loader=loaders.get("chairs"), **kwargs))
        elif val_dataset == "sintel":
            results.update(validate_sintel(*head, flowNetC=flowNetC, loaders=loaders.get("sintel"), **kwargs))
        elif val_dataset == "kitti":
            results.update(validate_kitti(*head, flowNetC=flowNetC, loader=loaders.get("kitti"), **kwargs))
    return results
