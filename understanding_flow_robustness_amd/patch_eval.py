"""The patch evaluation of the paper's tables (patch_attacks/test_patch.py:242-466): a finished patch, a random patch or a
hand-crafted self-similar pattern (`utils_patch.get_patch_and_mask`) is placed on every item of a validation set and the end-point
error / cosine similarity of the clean and the attacked prediction are recorded per item.  With `--different_pos` the patch moves,
turns and scales between the two frames, the ground truth it covers in the second frame is dropped and the ground truth inside
the patch becomes the patch's own motion.

Reference, per item: a canvas-sized host placement (six canvases and a flow field), five H2D copies, two batch-1 forwards, ten
torch operators for the pastes, two mask resizes, a `scipy.ndimage.zoom` of the canvas-sized flow on the host, ten operators for the
blends and four metric calls that each end in `.item()`.  Here the placement of every item is drawn in loader order (so the
`np.random` stream does not depend on `chunk`) as a record in patch coordinates (patch_transform.PlacementRecord), up to `chunk`
consecutive items of equal size are stacked, and per chunk

    ufr_eval_paste (csrc/patch_eval.hip)  ->  ONE forward of the 2K clean and pasted pairs  ->  ufr_eval_metrics

run; the host reads the results once, at the end.

With `save_path` the script's outputs are produced too (test_patch.py:163-236, :467-643): per chunk `ufr_eval_blend_gt` writes the
ground truth that was scored, `flowlib.viz_strip` (csrc/flow_viz.hip) builds the six-panel strips on the device, ONE copy takes them
into one of two pinned buffers and the files of the previous chunk are written while the device computes (the pattern of
validation._EncodedWriter); the CSV files follow at the end.  TensorBoard stays with the caller.
"""
from __future__ import annotations

from argparse import Namespace
import os
import warnings
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L
from .chunked_eval import ChunkedEval, check_pair


@dataclass
class EvalResult:
    per_item: np.ndarray         # float64 [N,4] in the order of `error_names`
    mean: np.ndarray             # float64 [4]: the plain mean over items (what the script's AverageMeter reports)
    locations: list              # per item [(x_tgt, y_tgt), (x_ref, y_ref)]
    error_names: list

    def csv_text(self):
        """(test_results.csv, test_result_scenes.csv) as the script writes them (test_patch.py:229-236, :623-643): the header, in
        the scene file one line per item, and the average as its AverageMeter forms it (a running sum in item order over the
        count)."""
        names = list(self.error_names)
        results = "{:>10}, {:>10}, {:>10}, {:>10}\n".format(*names)
        scenes = "{:>10}, {:>10}, {:>10}, {:>10}, {:>10}\n".format(*(["scene"] + names))
        total = [0.0] * 4
        for i, row in enumerate(self.per_item):
            row = [float(v) for v in row]
            total = [t + v for t, v in zip(total, row)]
            scenes += "{:10d}, {:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}\n".format(i, *row)
        avg = [t / len(self.per_item) for t in total] if len(self.per_item) else [0] * 4
        results += "{:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}\n".format(*avg)
        scenes += "{:>10}, {:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}\n".format(*(["avg"] + avg))
        return results, scenes

    def write_csv(self, save_path, different_pos=False):
        """`test_results[_diff_pos].csv` and `test_result_scenes[_diff_pos].csv` under `save_path` (test_patch.py:203-215); -> the
        two paths."""
        os.makedirs(save_path, exist_ok=True)
        tail = "_diff_pos.csv" if different_pos else ".csv"
        paths = os.path.join(save_path, "test_results" + tail), os.path.join(save_path, "test_result_scenes" + tail)
        for path, text in zip(paths, self.csv_text()):
            with open(path, "w", encoding="utf-8") as f:
                f.write(text)
        return paths


IMAGE_FORMATS = ("jpg", "png")


def save_strip(path, strip, image_format):
    """One strip, uint8 [H,6W,3] -> `path`: "jpg" as the script saves it (PIL's defaults), "png" lossless through
    `kitti_io.png_write`."""
    if image_format == "jpg":
        from PIL import Image
        Image.fromarray(strip).save(path)
    else:
        from . import kitti_io
        kitti_io.png_write(path, strip)


def checked_image_format(image_format):
    """"jpg" needs PIL; without it the strips are written as png, with a warning."""
    if image_format not in IMAGE_FORMATS:
        raise ValueError(f"image_format must be one of {IMAGE_FORMATS}, not {image_format!r}")
    if image_format == "jpg":
        try:
            import PIL.Image  # noqa: F401
        except ImportError:
            warnings.warn("PIL is not installed: the strips are written as viz###.png (lossless) instead of viz###.jpg")
            return "png"
    return image_format


class StripWriter:
    """Strips on their way to disk: `submit` starts the ONE copy of a chunk's strips into one of two pinned buffers and THEN writes
    the files of the previous submit -- the device computes meanwhile; `finish` writes the last one."""

    def __init__(self, directory, image_format):
        self.directory, self.format = directory, checked_image_format(image_format)
        os.makedirs(directory, exist_ok=True)
        self.pinned, self.turn, self.pending, self.paths = [None, None], 0, None, []

    def path(self, index):
        return os.path.join(self.directory, "viz" + str(index).zfill(3) + "." + self.format)

    def submit(self, strips, first_index):
        host = self.pinned[self.turn]
        if host is None or host.numel() < strips.numel():
            host = self.pinned[self.turn] = torch.empty(strips.numel(), dtype=torch.uint8).pin_memory()
        self.turn ^= 1
        host[:strips.numel()].copy_(strips.reshape(-1), non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        previous, self.pending = self.pending, (host, tuple(strips.shape), done, first_index)
        self._write(previous)

    def finish(self):
        previous, self.pending = self.pending, None
        self._write(previous)

    def _write(self, job):
        if job is None:
            return
        host, shape, done, first_index = job
        done.synchronize()                                             # the one host read of the chunk
        strips = host.numpy()[:int(np.prod(shape))].reshape(shape)
        for k, strip in enumerate(strips):
            self.paths.append(self.path(first_index + k))
            save_strip(self.paths[-1], strip, self.format)


def _refuse_3d(what):
    raise NotImplementedError(f"{what}: the reference projects the patch into the 3-D scene (project_patch_3d_scene, from depth, "
                              "calibration and poses); that projection is not part of this project")


class _Evaluation(ChunkedEval):
    """The state of one call: the float64 patch state and the locations; the chunk's paste, forward and metrics launch
    (chunked_eval.py: the waiting items, the results on the device)."""

    def __init__(self, flow_net, patch, mask, patch_shape, args, chunk):
        from .patch_attack import _pixel_range
        super().__init__(chunk)
        self.net, self.args = flow_net, args
        self.patch, self.mask, self.patch_shape = patch, mask, tuple(patch_shape)
        self.patch_d = self.mask_d = None
        self.lo, self.hi = _pixel_range(args.flownet)
        self.different = bool(getattr(args, "different_pos", False))
        self.homogeneous = bool(getattr(args, "HOMOGENUOUS", False))
        self.norotate = bool(getattr(args, "norotate", False))
        self.ignore = 1 if getattr(args, "ignore_mask_flow", False) else 0
        self.square = getattr(args, "patch_type", "circle") == "square"
        self.fixed_loc = (int(getattr(args, "fixed_loc_x", -1)), int(getattr(args, "fixed_loc_y", -1)))
        self.locations = []
        self.writer, self.done = None, 0                         # StripWriter of a call with save_path; items run so far
        self.figure_hook = None                                  # the tests: what the strips of a chunk were built from

    def _state(self, dev):
        if self.patch_d is None:
            f64 = lambda a: (a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev, torch.float64)
            self.patch_d, self.mask_d = f64(self.patch).contiguous(), f64(self.mask).contiguous()
        return self.patch_d, self.mask_d

    def place(self, data_shape, margin, dev):
        """test_patch.py:279-361: one item's placement record; `np.random` is consumed exactly as the script's transform does."""
        from . import patch_transform as pt
        patch_d, mask_d = self._state(dev)
        if self.different:                                       # whatever the patch type, like the script
            rec = pt.circle_transform_different_device(patch_d, mask_d, patch_d, data_shape, self.patch_shape, margin,
                                                       norotate=self.norotate, fixed_loc=self.fixed_loc)
            self.locations.append([(rec.origin_tgt[1], rec.origin_tgt[0]), (rec.origin_ref[1], rec.origin_ref[0])])
            return rec
        if self.square:
            cp, cm, _, x, y, (self.patch_d, self.mask_d, _) = pt.square_transform_device(patch_d, mask_d, patch_d, data_shape,
                                                                                         self.patch_shape, norotate=self.norotate)
            shape, slot = self.patch_d.shape, int(max(self.patch_d.shape[-2:]))
        else:
            cp, cm, _, x, y, shape = pt.circle_transform_device(patch_d, mask_d, patch_d, data_shape, self.patch_shape, margin,
                                                                norotate=self.norotate, fixed_loc=self.fixed_loc)
            slot = pt.slot_side(max(patch_d.shape[-2:]))
        self.locations.append([(x, y), (x, y)])
        return pt.record_from_canvas(cp, cm, x, y, shape, slot)

    def add(self, tgt, ref, gt, rec):
        super().add((tuple(tgt.shape), tuple(gt.shape), rec.slot), tgt, ref, gt, rec)

    def run_chunk(self, items):
        """One chunk: paste, ONE forward of the clean and the pasted pairs, metrics."""
        from .flownets.utils_model import predict_flow
        K = len(items)
        dev = items[0][1].device
        tgt, ref, gt = (self.stack_f32([it[i] for it in items], dev) for i in (1, 2, 3))
        recs = [it[4] for it in items]
        H, W, Hg, Wg, slot = int(tgt.shape[2]), int(tgt.shape[3]), int(gt.shape[2]), int(gt.shape[3]), recs[0].slot
        stack = lambda name: torch.stack([getattr(r, name) for r in recs]).contiguous()
        p_tgt, m_tgt = stack("patch_tgt"), stack("mask_tgt")
        second = recs[0].patch_ref is not None
        p_ref, m_ref = (stack("patch_ref"), stack("mask_ref")) if second else (None, None)
        flow = stack("flow").to(torch.float32) if recs[0].flow is not None else None     # the script's torch.FloatTensor(flow_full)
        places_host = np.ascontiguousarray(np.asarray([r.place() for r in recs], dtype=np.int32).reshape(K, 8))
        places = torch.from_numpy(places_host).to(dev)
        opt = lambda t: L.ptr(t) if t is not None else None
        adv_tgt, adv_ref = torch.empty_like(tgt), torch.empty_like(ref)
        lib = L.lib()
        self._mark("start")
        L.check(lib.ufr_eval_paste(L.ptr(tgt), L.ptr(ref), L.ptr(p_tgt), L.ptr(m_tgt), opt(p_ref), opt(m_ref), L.ptr(places),
                                   places_host.ctypes.data, L.ptr(adv_tgt), L.ptr(adv_ref), K, H, W, slot, slot, self.lo, self.hi,
                                   L.stream()), "eval paste")
        self._mark("paste")
        flows = predict_flow(self.net, None, torch.cat((tgt, adv_tgt)), torch.cat((ref, adv_ref)), self.args)
        flows = self.checked_flow(flows, 2 * K, H, W, same_size=True).contiguous()
        ws = self.workspace(lib.ufr_eval_metrics_workspace_doubles(self.chunk), dev)
        out = torch.zeros(K, 4, dtype=torch.float32, device=dev)
        self._mark("forward")
        L.check(lib.ufr_eval_metrics(L.ptr(flows[:K]), L.ptr(flows[K:]), L.ptr(gt), L.ptr(m_tgt), opt(m_ref), opt(flow), L.ptr(places),
                                     places_host.ctypes.data, K, H, W, Hg, Wg, slot, slot, self.ignore, L.ptr(ws), ws.numel(),
                                     L.ptr(out), 0, K, L.stream()), "eval metrics")
        self._mark("metrics")
        if self.writer is not None:
            from . import flowlib
            g = torch.empty(K, 3, Hg, Wg, dtype=torch.float32, device=dev)
            L.check(lib.ufr_eval_blend_gt(L.ptr(gt), L.ptr(m_tgt), opt(m_ref), opt(flow), L.ptr(places), places_host.ctypes.data,
                                          L.ptr(g), K, H, W, Hg, Wg, slot, slot, self.ignore, L.stream()), "eval blend gt")
            self._mark("blend")
            if self.figure_hook is not None:
                self.figure_hook(self.done, adv_tgt, adv_ref, flows[:K], flows[K:], g)
            strips = flowlib.viz_strip(adv_tgt, adv_ref, flows[:K], flows[K:], g, events=self._mark if self.events is not None else None)
            self.writer.submit(strips, self.done)
        self.done += K
        return out

    def write_back(self):
        """utils_patch.square_transform turns the CALLER's patch and mask in place; the accumulated turns are handed back."""
        if not (self.square and not self.different and self.patch_d is not None):
            return
        for dst, src in ((self.patch, self.patch_d), (self.mask, self.mask_d)):
            if torch.is_tensor(dst):
                dst.copy_(src.to(dst.dtype))
            else:
                np.copyto(dst, src.cpu().numpy().astype(dst.dtype, copy=False))


def output_dirs(save_path, args):
    """test_patch.py:163-177, :203-215: (where the CSV files go, where the images go)."""
    save_path = os.fspath(save_path)
    if getattr(args, "HOMOGENUOUS", False):
        save_path = os.path.join(save_path, "homogenuous_img")
        return save_path, save_path
    return save_path, os.path.join(save_path, "images_test_diff_pos" if getattr(args, "different_pos", False) else "images_test")


def evaluate_patch(flow_net, val_loader, patch, mask, patch_shape, args: Namespace, chunk=4, save_path=None,
                   image_format="jpg") -> EvalResult:
    """test_patch.py:242-643 without TensorBoard; with `save_path=None` without its images and CSV files too, and then the call
    launches nothing else.

    save_path: the script's `args.save_path`.  Per item the six-panel strip `images_test/viz%03d.jpg` (`images_test_diff_pos/`
    with different_pos; with HOMOGENUOUS everything goes into `save_path/homogenuous_img`), saved with PIL's defaults like the
    script's; `image_format="png"` writes `viz%03d.png` losslessly (also what is written, with a warning, when PIL is missing).
    `test_results[_diff_pos].csv` and `test_result_scenes[_diff_pos].csv` get the script's lines (`EvalResult.write_csv` writes them
    alone).  A network that answers below frame size (the script's `zoom` for FlowNetS) is refused.

    val_loader yields the reference's batch-1 items `(ref_past, tgt, ref, flow_gt[, disp_gt, calib, poses])` as HIP tensors
    (frames [1,3,H,W], flow_gt [1,3,Hg,Wg] = (u, v, valid)); patch / mask: [1,3,S,S] numpy arrays or tensors, as
    `utils_patch.get_patch_and_mask` returns them.  `args` fields (the script's defaults when absent): flownet, patch_type
    ("circle"), norotate (False), different_pos (False), fixed_loc_x / fixed_loc_y (-1), HOMOGENUOUS (False), ignore_mask_flow
    (False), true_motion (False).  The caller seeds `np.random` (the script: 1337); the draws are the script's, item by item,
    whatever `chunk` is.  `true_motion`, and an item with calibration while neither different_pos nor HOMOGENUOUS is set, need the
    3-D projection of the patch: NotImplementedError.  With `patch_type == "square"` the quarter turns accumulate in the caller's
    patch and mask, like the reference's in-place `square_transform`.  The parameters are frozen like the attack steps freeze
    them (`patch_attack.release(flow_net)` gives the flags back); the host synchronises once."""
    from .patch_attack import ERROR_NAMES
    if getattr(args, "true_motion", False):
        _refuse_3d("true_motion")
    ev = _Evaluation(flow_net, patch, mask, patch_shape, args, chunk)         # refuses chunk < 1
    if len(patch.shape) != 4 or tuple(patch.shape[:2]) != (1, 3) or tuple(mask.shape) != tuple(patch.shape):
        raise ValueError("patch and mask must be [1,3,S,S], in patch coordinates")
    ev.events = getattr(evaluate_patch, "_debug_events", None)            # tools/bench_patch_eval.py: device events around the entries
    if save_path is not None:
        csv_dir, image_dir = output_dirs(save_path, args)
        ev.writer = StripWriter(image_dir, image_format)
        ev.figure_hook = getattr(evaluate_patch, "_debug_figures", None)
    with torch.no_grad():
        for item in val_loader:
            tgt, ref, gt = item[1], item[2], item[3]
            calibrated = len(item) > 5 and len(item[5]) > 0
            if calibrated and not (ev.different or ev.homogeneous):
                _refuse_3d("an item with calibration (neither different_pos nor HOMOGENUOUS is set)")
            check_pair(tgt, ref, "the loader yields batch-1 items: tgt and ref [1,3,H,W]")
            if gt.dim() != 4 or gt.shape[0] != 1 or gt.shape[1] != 3:
                raise ValueError("flow_gt must be [1,3,Hg,Wg] (u, v, valid)")
            margin = int(item[4].max()) if calibrated else 0                          # test_patch.py:272-274
            L.require_hip(tgt, "tgt_img", contiguous=False)
            L.require_hip(ref, "ref_img", contiguous=False)
            L.require_hip(gt, "flow_gt", contiguous=False)
            rec = ev.place(tuple(tgt.shape), margin, tgt.device)
            ev.freeze_once(flow_net)
            if ev.homogeneous:                                                        # test_patch.py:255-259
                tgt, ref, gt = torch.full_like(tgt, 0.5), torch.full_like(ref, 0.5), torch.zeros_like(gt)
            ev.add(tgt, ref, gt, rec)
        ev.flush()
        ev.write_back()
        if ev.writer is not None:
            ev.writer.finish()
        rows = ev.read()                                                              # the one host synchronisation of the call
        per_item = rows[0].astype(np.float64) if rows else np.zeros((0, 4))
    mean = per_item.mean(axis=0) if len(per_item) else np.zeros(4)
    result = EvalResult(per_item, mean, ev.locations, list(ERROR_NAMES))
    if save_path is not None:
        result.write_csv(csv_dir, ev.different)
    return result
