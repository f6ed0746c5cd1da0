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
"""
from __future__ import annotations

import ctypes as C
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
