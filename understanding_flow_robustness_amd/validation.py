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

At the end of the file: the test-server submissions of evaluate.py:201-267 (`create_sintel_submission`, `create_kitti_submission`) and
`forward_interpolate` of models/raft/utils/utils.py:33-59, on the same chunk loop with csrc/submission.hip's two entries.
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


# ---- the test-server submissions ---------------------------------------------------------------------------------------------------
# `create_sintel_submission` and `create_kitti_submission` of training/evaluate.py:201-267 with `forward_interpolate` of
# models/raft/utils/utils.py:33-59, the warm start of the Sintel loop.  The datasets are the caller's here too: the loaders yield the
# reference's batch-1 items `(image1, image2, (sequence, frame))` / `(image1, image2, (frame_id,))`, plain (`str`, `int`) or as a
# `DataLoader` collates them (a 1-element list, a 1-element tensor).
def _interpolate_host(flow, use_scipy=None):
    """One item [2,h,w] (numpy) on the host, the rule of `ufr_forward_interpolate` (include/ufr_hip.h): with scipy the reference's
    own arithmetic (`griddata(method="nearest")` over the points that stay inside the grid), otherwise -- `use_scipy=False`, or
    scipy does not import -- a float64 brute force over chunks of grid pixels in which the lowest index wins a tie."""
    dx, dy = flow[0], flow[1]
    ht, wd = dx.shape
    x0, y0 = np.meshgrid(np.arange(wd), np.arange(ht))
    x1, y1 = (x0 + dx).reshape(-1), (y0 + dy).reshape(-1)
    with np.errstate(invalid="ignore"):
        valid = (x1 > 0) & (x1 < wd) & (y1 > 0) & (y1 < ht)
    x1, y1, dx, dy = x1[valid], y1[valid], dx.reshape(-1)[valid], dy.reshape(-1)[valid]
    if x1.size == 0:
        return np.full((2, ht, wd), np.nan, dtype=np.float32)          # scipy 1.15's answer for an empty point set
    if use_scipy is None or use_scipy:
        try:
            from scipy import interpolate
        except ImportError:
            if use_scipy:
                raise
            interpolate = None
        if interpolate is not None:
            flow_x = interpolate.griddata((x1, y1), dx, (x0, y0), method="nearest", fill_value=0)
            flow_y = interpolate.griddata((x1, y1), dy, (x0, y0), method="nearest", fill_value=0)
            return np.stack([flow_x, flow_y], axis=0).astype(np.float32)
    x1, y1 = x1.astype(np.float64), y1.astype(np.float64)
    gx, gy = x0.reshape(-1).astype(np.float64), y0.reshape(-1).astype(np.float64)
    nearest = np.empty(gx.size, dtype=np.int64)
    step = max(1, (1 << 22) // x1.size)                                 # 32 MiB of distances at a time
    for s in range(0, gx.size, step):
        ex, ey = x1[None, :] - gx[s:s + step, None], y1[None, :] - gy[s:s + step, None]
        nearest[s:s + step] = np.argmin(ex * ex + ey * ey, axis=1)      # (argmin: the first, i.e. lowest, index of a minimum)
    return np.stack([dx[nearest].reshape(ht, wd), dy[nearest].reshape(ht, wd)], axis=0).astype(np.float32)


def forward_interpolate(flow):
    """models/raft/utils/utils.py:33-59: the flow [2,h,w] (or a batch [B,2,h,w], every item on its own) splatted forward and filled
    in by nearest neighbour.  A HIP float32 tensor runs `ufr_forward_interpolate` (csrc/submission.hip: exact, one launch, no host
    synchronisation) and THE RESULT STAYS ON THE INPUT'S DEVICE -- the reference returns a CPU tensor; a caller's `[None].cuda()`
    works on either.  Any other tensor takes the host restatement (`_interpolate_host`) and comes back as a CPU float32 tensor."""
    batched = flow.dim() == 4
    f = flow if batched else flow[None]
    if f.dim() != 4 or f.shape[1] != 2 or f.shape[0] < 1 or f.shape[2] < 1 or f.shape[3] < 1:
        raise ValueError(f"forward_interpolate takes a flow of shape [2,h,w] or [B,2,h,w], not {tuple(flow.shape)}")
    if f.is_cuda and f.dtype == torch.float32:
        f = f.detach().contiguous()
        out = torch.empty_like(f)
        with torch.cuda.device(f.device):
            L.check(L.lib().ufr_forward_interpolate(L.ptr(f), L.ptr(out), int(f.shape[0]), int(f.shape[2]), int(f.shape[3]), L.stream()),
                    "forward interpolate")
    else:
        out = torch.from_numpy(np.stack([_interpolate_host(item) for item in f.detach().cpu().numpy()])).float()
    return out if batched else out[0]


def _one(value):
    """An entry of an item's tail, plain or as `DataLoader(batch_size=1)` collates it."""
    if torch.is_tensor(value):
        return value.reshape(-1)[0].item()
    if isinstance(value, (list, tuple)):
        if len(value) != 1:
            raise ValueError(f"the loader yields batch-1 items; got {value!r}")
        return _one(value[0])
    return value


def _sintel_item(item):
    image1, image2, (sequence, frame) = item
    return image1, image2, str(_one(sequence)), int(_one(frame))


def _kitti_item(item):
    image1, image2, (frame_id,) = item
    return image1, image2, str(_one(frame_id))


def _require_fused(image1, image2):
    for t, name in ((image1, "image1"), (image2, "image2")):
        L.require_hip(t, name, contiguous=False)
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name} must be float32 (fused=True); fused=False runs the reference's loop on any tensor")
    check_pair(image1, image2, "the loader yields batch-1 items: image1 and image2 [1,3,H,W]")


class _EncodedWriter:
    """Predictions on their way to disk: `submit` encodes the K padded-frame predictions of a chunk on the device
    (`ufr_flow_encode`), starts their copy into one of two pinned buffers and THEN writes the files of the previous submit -- the
    device computes the next chunk meanwhile; `finish` writes the last one.  mode 0: `.flo` files, mode 1: KITTI flow maps."""

    def __init__(self, mode):
        self.mode, self.item_bytes = mode, (8 if mode == 0 else 6)
        self.pinned, self.turn, self.pending = [None, None], 0, None

    def submit(self, flow, top, left, H, W, paths):
        K, Hp, Wp = int(flow.shape[0]), int(flow.shape[2]), int(flow.shape[3])
        nbytes = K * H * W * self.item_bytes
        encoded = torch.empty(nbytes, dtype=torch.uint8, device=flow.device)
        L.check(L.lib().ufr_flow_encode(L.ptr(flow), L.ptr(encoded), K, Hp, Wp, top, left, H, W, self.mode, L.stream()), "flow encode")
        host = self.pinned[self.turn]
        if host is None or host.numel() < nbytes:
            host = self.pinned[self.turn] = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self.turn ^= 1
        host[:nbytes].copy_(encoded, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        previous, self.pending = self.pending, (host, nbytes, done, (K, H, W), list(paths))
        self._write(previous)

    def finish(self):
        previous, self.pending = self.pending, None
        self._write(previous)

    def _write(self, job):
        if job is None:
            return
        from . import kitti_io
        host, nbytes, done, (K, H, W), paths = job
        done.synchronize()                                             # the one host read of the chunk
        raw = host.numpy()[:nbytes]
        if self.mode == 0:
            for path, flow in zip(paths, raw.view(np.float32).reshape(K, H, W, 2)):
                kitti_io.write_flo(path, flow)
        else:
            for path, codes in zip(paths, raw.view(np.uint16).reshape(K, H, W, 3)):
                kitti_io.write_flow_kitti(path, codes)


class _SubmissionChunks(ChunkedEval):
    """The chunk's pad, forward, encode and copy; the files are the writer's."""

    def __init__(self, model, iters, pad_mode, writer, chunk, with_flow_init):
        super().__init__(chunk)
        self.model, self.iters, self.pad_mode, self.writer, self.with_flow_init = model, iters, pad_mode, writer, with_flow_init

    def add(self, image1, image2, path):
        _require_fused(image1, image2)
        super().add((tuple(image1.shape), image1.device), image1, image2, path)

    def padded(self, image1, image2):
        """Both frames of the stacked pairs on the padded frame (one `ufr_validation_pad`; the frames themselves when nothing is
        added) and the crop's origin."""
        K, _, H, W = image1.shape
        left, right, top, bottom = InputPadder(image1.shape, mode=self.pad_mode)._pad
        if not (top or bottom or left or right):
            return image1, image2, 0, 0
        pad1, pad2 = (torch.empty(K, 3, H + top + bottom, W + left + right, dtype=torch.float32, device=image1.device) for _ in range(2))
        L.check(L.lib().ufr_validation_pad(L.ptr(image1), L.ptr(image2), L.ptr(pad1), L.ptr(pad2), K, H, W, top, bottom, left, right, 0,
                                           L.stream()), "validation pad")
        return pad1, pad2, top, left

    def forward(self, image1, image2, paths, flow_init=None):
        """pad -> ONE forward -> encode and copy; -> the low-resolution flow."""
        K, H, W = int(image1.shape[0]), int(image1.shape[2]), int(image1.shape[3])
        pad1, pad2, top, left = self.padded(image1, image2)
        self._mark("pad")
        if self.with_flow_init:
            flow_low, flow = self.model(pad1, pad2, iters=self.iters, flow_init=flow_init, test_mode=True)
        else:
            flow_low, flow = self.model(pad1, pad2, iters=self.iters, test_mode=True)
        flow = self.checked_flow(flow, K, H, W).to(torch.float32).contiguous()
        if flow.shape[2] < top + H or flow.shape[3] < left + W:
            raise RuntimeError(f"the network returned a flow of shape {tuple(flow.shape)} for padded frames of {tuple(pad1.shape)}")
        self._mark("forward")
        self.writer.submit(flow, top, left, H, W, paths)
        self._mark("encode")
        return flow_low

    def run_chunk(self, items):
        dev = items[0][1].device
        image1, image2 = (self.stack_f32([it[i] for it in items], dev) for i in (1, 2))
        self._mark("start")
        self.forward(image1, image2, [it[3] for it in items])
        return ()

    def warm_frame(self, image1, image2, path, flow_low_prev):
        """One frame of a warm-started chain: interpolate (device) -> pad -> forward -> encode and copy."""
        _require_fused(image1, image2)
        with torch.cuda.device(image1.device):
            self._mark("start")
            flow_init = None
            if flow_low_prev is not None:
                left, right, top, bottom = InputPadder(image1.shape, mode=self.pad_mode)._pad
                grid = ((int(image1.shape[2]) + top + bottom) // 8, (int(image1.shape[3]) + left + right) // 8)
                if tuple(flow_low_prev.shape) != (1, 2) + grid:
                    raise ValueError(f"warm start: the previous frame's low-resolution flow is {tuple(flow_low_prev.shape[2:])}, this "
                                     f"frame's grid is {grid}: the frames of a sequence must have one size")
                flow_init = forward_interpolate(flow_low_prev)
            self._mark("interpolate")
            return self.forward(image1.detach().contiguous(), image2.detach().contiguous(), [path], flow_init)


@torch.no_grad()
def create_sintel_submission(model, iters: int = 32, warm_start: bool = False, output_path: str = "sintel_submission", *, loaders=None,
                             chunk: int = 4, fused: bool = True):
    """Create submission for the Sintel leaderboard (evaluate.py:201-240): per item of `loaders["clean"]` and `loaders["final"]` the
    pair is padded, `model(image1, image2, iters=iters, flow_init=flow_prev, test_mode=True)` runs, and the unpadded prediction is
    written to `<output_path>/<dstype>/<sequence>/frame%04d.flo` with `frame + 1`.  With `warm_start` every forward starts from
    `forward_interpolate` of the previous frame's low-resolution flow; a new sequence starts cold.

    `fused=True` (HIP float32 frames): without `warm_start` up to `chunk` consecutive items of equal size are stacked and per chunk
    ONE ufr_validation_pad, ONE forward, ONE ufr_flow_encode and one copy to the host run; with `warm_start` the frames of a sequence
    are a batch-1 chain in which only device launches run between two forwards (interpolate, pad, forward, encode) -- the encoded
    prediction is copied into a pinned buffer and written to disk while the next frame computes.  `fused=False` is the reference's
    loop as written, on whatever device the items are on."""
    _need(loaders, "create_sintel_submission")
    for dstype in ["clean", "final"]:
        _need(loaders.get(dstype), f"create_sintel_submission ({dstype})")
    import os

    from . import kitti_io
    model.eval()
    for dstype in ["clean", "final"]:
        flow_prev, sequence_prev = None, None
        writer = _EncodedWriter(0)
        ev = _SubmissionChunks(model, iters, "sintel", writer, 1 if warm_start else chunk, True)
        ev.events = getattr(create_sintel_submission, "_debug_events", None)   # tools/bench_submission.py: device events per stage
        for test_data in loaders[dstype]:
            image1, image2, sequence, frame = _sintel_item(test_data)
            if sequence != sequence_prev:
                flow_prev = None
            output_dir = os.path.join(output_path, dstype, sequence)
            output_file = os.path.join(output_dir, "frame%04d.flo" % (frame + 1))
            os.makedirs(output_dir, exist_ok=True)
            if fused and warm_start:
                flow_prev = ev.warm_frame(image1, image2, output_file, flow_prev)      # (kept as flow_low: interpolated when it is used)
            elif fused:
                ev.add(image1, image2, output_file)
            else:
                padder = InputPadder(image1.shape)
                image1, image2 = padder.pad(image1, image2)
                flow_low, flow_pr = model(image1, image2, iters=iters, flow_init=flow_prev, test_mode=True)
                flow = padder.unpad(flow_pr[0]).permute(1, 2, 0).cpu().numpy()
                if warm_start:
                    flow_prev = forward_interpolate(flow_low[0])[None].to(image1.device)
                kitti_io.write_flo(output_file, flow)
            sequence_prev = sequence
        ev.read()
        writer.finish()


@torch.no_grad()
def create_kitti_submission(model, iters: int = 24, output_path: str = "kitti_submission", *, loader=None, chunk: int = 4,
                            fused: bool = True):
    """Create submission for the KITTI leaderboard (evaluate.py:243-267): per item `(image1, image2, (frame_id,))` the pair is padded
    with `mode="kitti"`, `model(image1, image2, iters=iters, test_mode=True)` runs and the unpadded prediction is written as a 16-bit
    RGB PNG (`kitti_io.write_flow_kitti`) to `os.path.join(output_path, frame_id)`.  `fused` and `chunk` as in
    `create_sintel_submission`; the codes are then computed on the device (ufr_flow_encode, mode 1)."""
    _need(loader, "create_kitti_submission")
    import os

    from . import kitti_io
    model.eval()
    os.makedirs(output_path, exist_ok=True)
    writer = _EncodedWriter(1)
    ev = _SubmissionChunks(model, iters, "kitti", writer, chunk, False)
    ev.events = getattr(create_kitti_submission, "_debug_events", None)
    for test_data in loader:
        image1, image2, frame_id = _kitti_item(test_data)
        output_filename = os.path.join(output_path, frame_id)
        if fused:
            ev.add(image1, image2, output_filename)
        else:
            padder = InputPadder(image1.shape, mode="kitti")
            image1, image2 = padder.pad(image1, image2)
            _, flow_pr = model(image1, image2, iters=iters, test_mode=True)
            flow = padder.unpad(flow_pr[0]).permute(1, 2, 0).cpu().numpy()
            kitti_io.write_flow_kitti(output_filename, flow)
    ev.read()
    writer.finish()
