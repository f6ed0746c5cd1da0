"""The patch location sweep of the paper's Section 4.1 (patch_attacks/test_moving_patch.py:280-445, `--stride 25 --norotate`):
the finished patch is moved over one frame pair and the end-point error / cosine similarity against the blended ground truth is
recorded at every position.

Reference, per position: a canvas-sized host placement (`circle_transform(moving=True, fixed_loc=...)`), one H2D copy, five torch
operators for the paste, a batch-1 forward, a bilinear resize of the canvas mask, five operators for the blend and two metric calls
that each end in `.item()`.  Here the positions run in chunks of `chunk`; per chunk

    ufr_sweep_paste (csrc/patch_sweep.hip)  ->  the network on the batch  ->  ufr_sweep_metrics

and the host reads the [positions, 2] result buffer once per call.  Two paths:

generic   every network `fetch_model` builds: the chunk's adversarial canvases from the one clean pair, `predict_flow` on the batch.
windowed  networks with a convolutional prefix on the native FlowNetC engine (cone.py, flownetc_engine.py): in a sweep the clean
          frames never change and only the window moves, so conv1-3 of the clean pair are computed once, every chunk restores them
          (`load_prefix_features`), runs the prefix on a window around each position's patch (`window_prefix_forward`) and the head
          at full size (`forward_cached`).  The canvases are never materialised.

`sweep_scenes` is the scene loop of test_moving_patch.py:246-678 around it: per scene the statistics of both maps, the map resized
to the frame (`adv_epe_image_%03d.npy`), one more paste and forward at the first worst position and its six-panel strip
(flowlib.viz_strip on the ground truth `ufr_sweep_blend_gt` writes), and the script's two CSV files.
"""
from __future__ import annotations

import ctypes as C
import os
from argparse import Namespace
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L
from .chunked_eval import StageEvents, freeze

WINDOWED_STAGES = ("restore", "paste", "prefix", "head", "metrics")     # per chunk, in order (tools/bench_patch_sweep.py times them)
# `cone=None`: the windowed path where it can serve -- 0.366 against 0.755 ms per position for FlowNetC at 384 x 1280
# (tools/bench_patch_sweep.py, profiles/patch_sweep.json)
CONE_BY_DEFAULT = True


@dataclass
class SweepResult:
    adv_epe: np.ndarray          # float64 [ny, nx], indexed [y // stride, x // stride]
    adv_cos_sim: np.ndarray      # float64 [ny, nx]
    epe: float                   # the clean pair's metrics
    cos_sim: float
    worst: tuple                 # (y, x): first arg-max of adv_epe in the reference's visiting order
    locations: list              # [(y, x), ...] in visiting order (x outer, y inner)
    windowed: bool = False       # which path served the call


def sweep_grid(H, W, ph, pw, stride):
    """test_moving_patch.py:299-306: (ys, xs, locations); `locations` = [(y, x), ...] in visiting order, x outer and y inner; the
    maps are [len(ys), len(xs)] and position (y, x) lands at [y // stride, x // stride]."""
    if stride < 1:
        raise ValueError("stride must be positive")
    ys, xs = list(range(0, H - ph, stride)), list(range(0, W - pw, stride))
    return ys, xs, [(y, x) for x in xs for y in ys]


def _check_arguments(tgt_img, ref_future_img, flow_gt, patch, mask, args, chunk):
    for name, t in (("tgt_img", tgt_img), ("ref_future_img", ref_future_img)):
        if t.dim() != 4 or t.shape[1] != 3:
            raise ValueError(f"{name} must be [1,3,H,W]")
        if t.shape[0] != 1:
            raise ValueError(f"{name}: the sweep moves the patch over ONE frame pair (batch {t.shape[0]})")
    if ref_future_img.shape != tgt_img.shape:
        raise ValueError("tgt_img and ref_future_img differ in shape")
    if flow_gt.dim() != 4 or flow_gt.shape[0] != 1:
        raise ValueError("flow_gt must be [1,3,Hg,Wg] (one frame pair)")
    if flow_gt.shape[1] != 3:
        # test_moving_patch.py:430-432 blends three channels with a three-channel patch flow
        raise ValueError(f"flow_gt needs three channels (u, v, valid); it has {flow_gt.shape[1]}")
    if tuple(patch.shape[:2]) != (1, 3) or tuple(mask.shape) != tuple(patch.shape) or len(patch.shape) != 4:
        raise ValueError("patch and mask must be [1,3,ph,pw], in patch coordinates")
    if not getattr(args, "norotate", False):
        raise NotImplementedError("norotate=False draws one random rotation per position (test_moving_patch.py:323); the sweep "
                                  "implements the documented `--norotate` configuration only: set args.norotate = True")
    if int(chunk) < 1:
        raise ValueError("chunk must be positive")


def _placed_patch(patch, mask, dev):
    """`circle_transform(moving=True)` (utils_patch.py:272-273): clip(patch, 0, 1) * mask in float64, then the reference's
    `torch.FloatTensor(...)`.  Returns float32 (patch_p, mask_p) [1,3,ph,pw] on `dev`."""
    f64 = lambda a: (a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev, torch.float64)
    p, m = f64(patch), f64(mask)
    return (p.clamp(0.0, 1.0) * m).float().contiguous(), m.float().contiguous()


def _window_size(flow_net, H, W, ph, pw, dev):
    """(wh, ww) when the windowed path can serve this network and size, else the reason it cannot."""
    spec = getattr(flow_net, "CONE", None)
    if spec is None:
        return "the network exposes no convolutional prefix (CONE)"
    if getattr(flow_net, "ENGINE", "flownetc") != "flownetc":
        return "the network's windowed prefix is not the FlowNetC engine's"
    if H % spec.total_stride or W % spec.total_stride:
        return f"frame sides are not multiples of {spec.total_stride}"
    avail = getattr(flow_net, "engine_available", None)
    if avail is None or not avail(H, W, dev):
        return "the native engine does not serve this network at this size"
    wh, ww = spec.window_size(ph, H), spec.window_size(pw, W)
    if wh * ww * 2 > H * W:                    # PatchAttackStep._setup_cone's own test
        return f"the {wh}x{ww} window is not much smaller than the {H}x{W} frame"
    return wh, ww


class _Sweep(StageEvents):
    """The buffers and launches of one call."""

    def __init__(self, flow_net, tgt, ref, flow_gt, patch_p, mask_p, args, locations, chunk, ignore_mask_flow):
        from .patch_attack import _pixel_range
        self.net, self.args, self.dev = flow_net, args, tgt.device
        self.tgt, self.ref, self.gt = tgt, ref, flow_gt
        self.patch_p, self.mask_p = patch_p, mask_p
        self.H, self.W = int(tgt.shape[2]), int(tgt.shape[3])
        self.Hg, self.Wg = int(flow_gt.shape[2]), int(flow_gt.shape[3])
        self.ph, self.pw = int(patch_p.shape[2]), int(patch_p.shape[3])
        self.lo, self.hi = _pixel_range(args.flownet)
        self.K = int(chunk)
        self.valid_in_patch = 0 if ignore_mask_flow else 1
        self.n = len(locations)
        self.chunks = -(-self.n // self.K)
        rows = self.chunks * self.K
        # a ragged last chunk repeats its last position; the padded rows are dropped at the end
        padded = list(locations) + [locations[-1]] * (rows - self.n)
        self.origins_host = np.ascontiguousarray(np.asarray(padded, dtype=np.int32).reshape(rows, 2))
        self.origins = torch.from_numpy(self.origins_host).to(self.dev)
        self.rows = rows + 1                      # the last row receives the clean pair's metrics
        self.out = torch.zeros(self.rows, 2, dtype=torch.float32, device=self.dev)
        need = L.lib().ufr_sweep_metrics_workspace_doubles(self.K)
        self.ws = torch.zeros(need, dtype=torch.float64, device=self.dev)

    def _origin_args(self, c):
        off = c * self.K * 2
        return C.c_void_p(self.origins.data_ptr() + 4 * off), C.c_void_p(self.origins_host.ctypes.data + 4 * off)

    def metrics(self, flow, c):
        """Rows c*K .. c*K + K - 1 of the result buffer from the chunk's flows [K,2,H,W]."""
        if not flow.is_contiguous():
            flow = flow.contiguous()
        od, oh = self._origin_args(c)
        L.check(L.lib().ufr_sweep_metrics(L.ptr(flow), L.ptr(self.gt), L.ptr(self.mask_p), od, oh, self.K, self.H, self.W, self.Hg,
                                          self.Wg, self.ph, self.pw, self.valid_in_patch, L.ptr(self.ws), self.ws.numel(),
                                          L.ptr(self.out), c * self.K, self.rows, L.stream()), "sweep metrics")

    def clean_metrics(self, flow):
        flow = flow.contiguous()
        L.check(L.lib().ufr_sweep_metrics(L.ptr(flow), L.ptr(self.gt), None, None, None, 1, self.H, self.W, self.Hg, self.Wg, 0, 0,
                                          self.valid_in_patch, L.ptr(self.ws), self.ws.numel(), L.ptr(self.out), self.rows - 1,
                                          self.rows, L.stream()), "sweep metrics (clean)")

    # ------------------------------------------------------------------------------------------------ generic path
    def run_generic(self, hook):
        from .flownets.utils_model import predict_flow
        f32 = dict(dtype=torch.float32, device=self.dev)
        adv_tgt = torch.empty(self.K, 3, self.H, self.W, **f32)
        adv_ref = torch.empty_like(adv_tgt)
        self.clean_metrics(predict_flow(self.net, None, self.tgt, self.ref, self.args))
        for c in range(self.chunks):
            od, oh = self._origin_args(c)
            L.check(L.lib().ufr_sweep_paste(L.ptr(self.tgt), L.ptr(self.ref), L.ptr(self.patch_p), L.ptr(self.mask_p), od, oh,
                                            L.ptr(adv_tgt), L.ptr(adv_ref), self.K, self.H, self.W, self.ph, self.pw, self.lo, self.hi,
                                            None, 0, 0, None, None, L.stream()), "sweep paste")
            flow = predict_flow(self.net, None, adv_tgt, adv_ref, self.args)
            self.metrics(flow, c)
            if hook is not None:
                hook(c * self.K, flow)

    # ------------------------------------------------------------------------------------------------ windowed path
    def run_windowed(self, wh, ww, hook):
        from .flownetc_engine import get_engine
        net, K, H, W = self.net, self.K, self.H, self.W
        f32 = dict(dtype=torch.float32, device=self.dev)
        c2, c3 = net.encode(torch.cat((self.tgt, self.ref), 0))
        # the clean features of the one pair behind every position of a chunk: conv2 of the first frame, conv3 of the first frames
        # and then of the second frames, as load_prefix_features expects (copies: `encode` may hand out static buffers)
        c2_K = c2[:1].expand(K, -1, -1, -1).contiguous()
        c3_K = torch.cat((c3[:1].expand(K, -1, -1, -1), c3[1:2].expand(K, -1, -1, -1)), 0).contiguous()
        self.clean_metrics(net.head(c2_K[:1], c3_K[:1], c3_K[K:K + 1]))
        eng = get_engine(net, K, H, W, self.dev)
        m2, m3 = net.CONE.tap_margins()
        chain = net.CONE.to_c()
        xw = torch.empty(2 * K, 3, wh, ww, **f32)
        win = torch.zeros(K, 8, dtype=torch.int32, device=self.dev)
        for c in range(self.chunks):
            od, oh = self._origin_args(c)
            self._mark("start")
            eng.load_prefix_features(c2_K, c3_K)   # the clean features everywhere: undoes the previous chunk's windows
            self._mark("restore")
            L.check(L.lib().ufr_sweep_paste(L.ptr(self.tgt), L.ptr(self.ref), L.ptr(self.patch_p), L.ptr(self.mask_p), od, oh, None,
                                            None, K, H, W, self.ph, self.pw, self.lo, self.hi, C.byref(chain), wh, ww, L.ptr(win),
                                            L.ptr(xw), L.stream()), "sweep paste (window)")
            self._mark("paste")
            eng.window_prefix_forward(xw, win, m2, m3, c2_nchw=False)
            self._mark("prefix")
            # no band, no incremental head: both assume that the window stays where it was
            flow2 = eng.forward_cached(None)
            flow = torch.nn.functional.interpolate(flow2 * eng.flow_scale, scale_factor=4, mode="bilinear", align_corners=False)
            self._mark("head")
            self.metrics(flow, c)
            self._mark("metrics")
            if hook is not None:
                hook(c * K, flow)
        # leave the clean features behind, not the last chunk's windows (the engine is shared with the attack steps)
        eng.load_prefix_features(c2_K, c3_K)


def sweep_patch_locations(flow_net, tgt_img, ref_future_img, flow_gt, patch, mask, args: Namespace, stride=25, chunk=8,
                          ignore_mask_flow=False, cone=None) -> SweepResult:
    """test_moving_patch.py:280-445 for `whole_img == 0`, `--norotate`, no calibration (the same patch on both frames).

    tgt_img / ref_future_img: [1,3,H,W] HIP float32; flow_gt: [1,3,Hg,Wg] HIP float32 (u, v, valid), Hg x Wg need not be H x W;
    patch / mask: [1,3,ph,pw] numpy arrays or tensors in patch coordinates -- the placed patch is clip(patch, 0, 1) * mask.
    Positions: x in range(0, W - pw, stride) (outer), y in range(0, H - ph, stride) (inner).  Per position the frames are
    clamp((1 - M) * img + M * P), the ground truth is (1 - m) * flow_gt + m * (0, 0, 1) -- (0, 0, 0) with `ignore_mask_flow` --
    with m the canvas mask resized bilinearly to Hg x Wg, and the metrics are `losses.compute_epe` / `compute_cossim` of it.
    cone: None = the path the measurements favour for this network; True = the windowed path or an error; False = generic.
    The parameters are frozen like the attack steps freeze them (`patch_attack.release(flow_net)` gives the flags back); the
    host synchronises once."""
    _check_arguments(tgt_img, ref_future_img, flow_gt, patch, mask, args, chunk)
    L.require_hip(tgt_img, "tgt_img", contiguous=False)
    L.require_hip(ref_future_img, "ref_future_img", contiguous=False)
    L.require_hip(flow_gt, "flow_gt", contiguous=False)
    L.lib()
    dev = tgt_img.device
    H, W = int(tgt_img.shape[2]), int(tgt_img.shape[3])
    ph, pw = int(patch.shape[2]), int(patch.shape[3])
    if ph > H or pw > W:
        raise ValueError("the patch is larger than the frame")
    ys, xs, locations = sweep_grid(H, W, ph, pw, int(stride))
    if not locations:
        raise ValueError("no position: the patch fills the frame")
    freeze(flow_net)
    hook = getattr(sweep_patch_locations, "_debug_flows", None)
    events = getattr(sweep_patch_locations, "_debug_events", None)
    with torch.no_grad(), torch.cuda.device(dev):
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        patch_p, mask_p = _placed_patch(patch, mask, dev)
        sized = _window_size(flow_net, H, W, ph, pw, dev)
        if cone and isinstance(sized, str):
            raise RuntimeError(f"sweep_patch_locations(cone=True): the windowed path cannot serve this call: {sized}")
        windowed = not isinstance(sized, str) and (cone if cone is not None else CONE_BY_DEFAULT)
        sweep = _Sweep(flow_net, f32(tgt_img), f32(ref_future_img), f32(flow_gt), patch_p, mask_p, args, locations, chunk,
                       ignore_mask_flow)
        sweep.events = events                                     # tools/bench_patch_sweep.py: the windowed path's stages
        if windowed:
            sweep.run_windowed(*sized, hook)
        else:
            sweep.run_generic(hook)
        out = sweep.out.cpu().numpy().astype(np.float64)          # the one host synchronisation of the call
    adv_epe, adv_cos = np.zeros((len(ys), len(xs))), np.zeros((len(ys), len(xs)))
    worst, worst_epe = None, -1.0
    for i, (y, x) in enumerate(locations):
        adv_epe[y // stride, x // stride] = out[i, 0]
        adv_cos[y // stride, x // stride] = out[i, 1]
        if out[i, 0] > worst_epe:                                  # strict: the first maximum (test_moving_patch.py:447)
            worst_epe, worst = out[i, 0], (y, x)
    return SweepResult(adv_epe, adv_cos, float(out[-1, 0]), float(out[-1, 1]), worst, locations, bool(windowed))


# ---- the scene loop --------------------------------------------------------------------------------------------------------------------
RESULT_NAMES = ["epe", "adv_epe_avg", "adv_epe_min", "adv_epe_median", "adv_epe_max", "cos_sim", "adv_cos_sim_avg", "adv_cos_min",
                "adv_cos_median", "adv_cos_max"]                       # test_moving_patch.py:226-237


def moving_headers():
    """(header of moving_results.csv, header of moving_result_scenes.csv), test_moving_patch.py:238-245."""
    names = ", ".join(RESULT_NAMES) + "\n"
    return names, "scene, " + names


def _rounded_row(values):
    """The script's f-string of ten `round(., 4)` (test_moving_patch.py:503, :674): no blank after the first comma."""
    r = [round(v, 4) for v in values]
    return f"{r[0]},{r[1]}, " + ", ".join(str(v) for v in r[2:]) + "\n"


def moving_scene_line(index, values):
    return f"{index}, " + _rounded_row(values)


def moving_total_line(values):
    return _rounded_row(values)


class _Meter:
    """The script's AverageMeter (patch_attacks/logger.py:83-109) for one quantity: a running sum over the count, the minimum
    starting at 10e6 and the maximum starting at 0 -- so a map without a positive value reports a maximum of 0, like the script."""

    def __init__(self):
        self.sum, self.count, self.min, self.max = 0, 0, 10e6, 0

    def update(self, v):
        self.count += 1
        self.sum += v
        self.min = v if v < self.min else self.min
        self.max = v if v > self.max else self.max

    @property
    def avg(self):
        return self.sum / self.count


def scene_statistics(adv_epe, adv_cos_sim):
    """avg, min, median and max of both maps [ny, nx] as test_moving_patch.py:490-500 forms them: the meter over the positions in
    visiting order (x outer, y inner), the median by numpy."""
    stats = {}
    for name, m in (("adv_epe", np.asarray(adv_epe)), ("adv_cos_sim", np.asarray(adv_cos_sim))):
        meter, values = _Meter(), [float(v) for v in m.T.reshape(-1)]
        for v in values:
            meter.update(v)
        stats[name + "_avg"], stats[name + "_min"], stats[name + "_max"] = meter.avg, meter.min, meter.max
        stats[name + "_median"] = float(np.median(values))
    return stats


def zoomed_map(adv_epe, H, W):
    """test_moving_patch.py:474-481: the map resized to the frame by scipy.ndimage.zoom, order 1."""
    from scipy.ndimage import zoom
    adv_epe = np.asarray(adv_epe)
    return zoom(adv_epe, zoom=(H / adv_epe.shape[-2], W / adv_epe.shape[-1]), order=1)


def worst_strip(flow_net, tgt, ref, flow_gt, patch, mask, args, worst, ignore_mask_flow=False):
    """test_moving_patch.py:447-471, :529-654: one paste and one forward of the clean and the pasted pair at position `worst` =
    (y, x), the ground truth that position was scored with, and the six-panel strip: uint8 HIP tensor [1,H,6W,3]."""
    from . import flowlib
    from .flownets.utils_model import predict_flow
    from .patch_attack import _pixel_range
    dev = tgt.device
    with torch.no_grad(), torch.cuda.device(dev):
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        tgt, ref, gt = f32(tgt), f32(ref), f32(flow_gt)
        patch_p, mask_p = _placed_patch(patch, mask, dev)
        H, W, Hg, Wg = int(tgt.shape[2]), int(tgt.shape[3]), int(gt.shape[2]), int(gt.shape[3])
        ph, pw = int(patch_p.shape[2]), int(patch_p.shape[3])
        lo, hi = _pixel_range(args.flownet)
        origin_host = np.ascontiguousarray(np.asarray([worst], dtype=np.int32).reshape(1, 2))
        origin = torch.from_numpy(origin_host).to(dev)
        adv_tgt, adv_ref = torch.empty_like(tgt), torch.empty_like(ref)
        lib = L.lib()
        L.check(lib.ufr_sweep_paste(L.ptr(tgt), L.ptr(ref), L.ptr(patch_p), L.ptr(mask_p), L.ptr(origin), origin_host.ctypes.data,
                                    L.ptr(adv_tgt), L.ptr(adv_ref), 1, H, W, ph, pw, lo, hi, None, 0, 0, None, None, L.stream()),
                "sweep paste")
        flows = predict_flow(flow_net, None, torch.cat((tgt, adv_tgt)), torch.cat((ref, adv_ref)), args).contiguous()
        g = torch.empty(1, 3, Hg, Wg, dtype=torch.float32, device=dev)
        L.check(lib.ufr_sweep_blend_gt(L.ptr(gt), L.ptr(mask_p), L.ptr(origin), origin_host.ctypes.data, L.ptr(g), 1, H, W, Hg, Wg, ph,
                                       pw, 0 if ignore_mask_flow else 1, L.stream()), "sweep blend gt")
        hook = getattr(worst_strip, "_debug_figures", None)            # the tests: what the strip was built from
        if hook is not None:
            hook(tuple(worst), adv_tgt, adv_ref, flows[:1], flows[1:], g)
        return flowlib.viz_strip(adv_tgt, adv_ref, flows[:1], flows[1:], g)


def sweep_scenes(flow_net, loader, patch, mask, args: Namespace, stride=25, chunk=8, save_path=None, image_format="jpg",
                 ignore_mask_flow=False, cone=None):
    """The scene loop of test_moving_patch.py:246-678 around `sweep_patch_locations`, under its preconditions (`--norotate`, no
    calibration: an item with calibration needs the 3-D projection and raises NotImplementedError).

    loader yields the reference's batch-1 items `(ref_past, tgt, ref, flow_gt[, disp_gt, calib, poses])` as HIP tensors.  Per scene:
    the sweep and the clean metrics, the statistics of `scene_statistics`, and -- with `save_path` -- `viz%03d.jpg` in
    `save_path/moving_patch_worst_images` (the strip at the first worst position; `image_format="png"` lossless),
    `adv_epe_image_%03d.npy` in `save_path/moving_patch` (the map resized to the frame; the matplotlib overlay the script draws from
    it stays with the caller) and a row of `moving_result_scenes.csv`; at the end the one row of `moving_results.csv`.

    Returns (the per-scene SweepResults, table): table["scenes"] = per scene the ten numbers of `RESULT_NAMES`, table["total"] the
    ten of `moving_results.csv`: the running averages over ALL positions of all scenes and the means of the scenes' minima, medians
    and maxima (:660-675)."""
    from .patch_eval import StripWriter
    results, scenes = [], []
    totals = [_Meter() for _ in range(4)]                               # epe, adv_epe, cos_sim, adv_cos over every position
    writer = map_dir = None
    if save_path is not None:
        save_path = os.fspath(save_path)
        map_dir = os.path.join(save_path, "moving_patch")
        os.makedirs(map_dir, exist_ok=True)
        writer = StripWriter(os.path.join(save_path, "moving_patch_worst_images"), image_format)
        header, scene_header = moving_headers()
        with open(os.path.join(save_path, "moving_results.csv"), "w", encoding="utf-8") as f:
            f.write(header)
        with open(os.path.join(save_path, "moving_result_scenes.csv"), "w", encoding="utf-8") as f:
            f.write(scene_header)
    for i, item in enumerate(loader):
        tgt, ref, gt = item[1], item[2], item[3]
        if len(item) > 5 and len(item[5]) > 0:
            raise NotImplementedError("an item with calibration: the reference projects the patch into the 3-D scene "
                                      "(project_patch_3d_scene); that projection is not part of this project")
        r = sweep_patch_locations(flow_net, tgt, ref, gt, patch, mask, args, stride=stride, chunk=chunk,
                                  ignore_mask_flow=ignore_mask_flow, cone=cone)
        results.append(r)
        for y, x in r.locations:                                        # errors.update per position, in visiting order (:438)
            for meter, v in zip(totals, (r.epe, r.adv_epe[y // stride, x // stride], r.cos_sim, r.adv_cos_sim[y // stride, x // stride])):
                meter.update(float(v))
        st = scene_statistics(r.adv_epe, r.adv_cos_sim)
        scenes.append([r.epe, st["adv_epe_avg"], st["adv_epe_min"], st["adv_epe_median"], st["adv_epe_max"], r.cos_sim,
                       st["adv_cos_sim_avg"], st["adv_cos_sim_min"], st["adv_cos_sim_median"], st["adv_cos_sim_max"]])
        if save_path is not None:
            strip = worst_strip(flow_net, tgt, ref, gt, patch, mask, args, r.worst, ignore_mask_flow)
            writer.submit(strip, i)                                     # written while the next scene's sweep runs
            np.save(os.path.join(map_dir, "adv_epe_image_" + str(i).zfill(3) + ".npy"),
                    zoomed_map(r.adv_epe, int(tgt.shape[-2]), int(tgt.shape[-1])))
            with open(os.path.join(save_path, "moving_result_scenes.csv"), "a", encoding="utf-8") as f:
                f.write(moving_scene_line(i, scenes[-1]))
    if writer is not None:
        writer.finish()
    table = {"names": list(RESULT_NAMES), "scenes": np.asarray(scenes, dtype=np.float64).reshape(-1, 10), "total": None}
    if scenes:
        col = lambda j: float(np.mean([s[j] for s in scenes]))
        table["total"] = [totals[0].avg, totals[1].avg, col(2), col(3), col(4), totals[2].avg, totals[3].avg, col(7), col(8), col(9)]
        if save_path is not None:
            with open(os.path.join(save_path, "moving_results.csv"), "a", encoding="utf-8") as f:
                f.write(moving_total_line(table["total"]))
    return results, table
