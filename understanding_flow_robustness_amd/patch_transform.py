"""The patch's trip between its own SxS frame and the image canvas, on the device.

Device counterparts of `utils_patch.circle_transform` (patch_attacks/utils_patch.py:257-358) and of the
crop / zoom-back after the attack (patch_attacks/main.py:408-461).  The patch state is a float64 HIP tensor
[1,3,S,S] -- the reference's numpy arrays are float64 too -- and never visits the host: the reference spends
~80 ms per sample on three canvas-sized `np.zeros`, `scipy.ndimage` calls, float64->float32 conversion and
three H2D copies (plus the D2H on the way back), several times the attack iteration itself.

RNG mapping (bit-documented): `np.random` is consumed on the host in exactly the reference's order --
`random()` brightness offset, `random()` zoom factor, then per sample `random()` rotation angle,
`choice(W - 2S - 2 margin - 2)` column, `choice(H - 2S - 2)` row -- and the drawn numbers are passed to the
kernels; the resampling itself (csrc/placement.hip) reproduces scipy.ndimage's order-0/1, mode='constant'
arithmetic in float64.

`circle_transform_different_device` is the two-frame placement of `test_patch.py --different_pos`
(utils_patch.py:499-757): it returns a `PlacementRecord` in patch coordinates instead of canvases, which is what
patch_eval.py stacks into the tables of csrc/patch_eval.hip.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch
from scipy import special

from . import _lib as L


def _resample(src, out_hw, m, off, order):
    """src [N,C,h,w] float64 HIP tensor -> [N,C,oh,ow]; planes share the 2x2 matrix `m` and `off`."""
    L.require_hip(src, "patch state", contiguous=True)
    if src.dtype != torch.float64:
        raise TypeError("the patch state is float64 (like the reference's numpy arrays)")
    n, c, h, w = src.shape
    dst = torch.empty(n, c, out_hw[0], out_hw[1], dtype=torch.float64, device=src.device)
    L.check(L.lib().ufr_affine_resample_f64(L.ptr(src), L.ptr(dst), n * c, h, w, out_hw[0], out_hw[1], float(m[0]),
                                            float(m[1]), float(m[2]), float(m[3]), float(off[0]), float(off[1]),
                                            int(order), L.stream()), "affine resample")
    return dst


def zoom_device(x, factors, order):
    """scipy.ndimage.zoom(x, (1, 1, fy, fx), order=order) (mode='constant', grid_mode=False)."""
    h, w = x.shape[-2:]
    oh, ow = int(round(h * factors[0])), int(round(w * factors[1]))
    zy = (h - 1) / (oh - 1) if oh > 1 else 1.0
    zx = (w - 1) / (ow - 1) if ow > 1 else 1.0
    return _resample(x, (oh, ow), (zy, 0.0, 0.0, zx), (0.0, 0.0), order)


def rotate_device(x, angle, order=1):
    """scipy.ndimage.rotate(plane, angle, reshape=False, order=order) on every [h,w] plane of x."""
    h, w = x.shape[-2:]
    c, s = special.cosdg(angle), special.sindg(angle)
    rot = np.array([[c, s], [-s, c]])
    shape = np.asarray((h, w))
    out_center = rot @ ((shape - 1) / 2)
    offset = (shape - 1) / 2 - out_center
    return _resample(x, (h, w), (rot[0, 0], rot[0, 1], rot[1, 0], rot[1, 1]), offset, order)


def circle_transform_device(patch, mask, patch_init, data_shape, patch_shape, margin=0, center=False, norotate=False,
                            fixed_loc=(-1, -1), moving=False):
    """utils_patch.circle_transform with HIP tensors: float64 state in, float32 canvases [1,3,H,W] out.
    Returns (canvas_patch, canvas_mask, canvas_init, x, y, zoomed patch shape)."""
    if data_shape[0] != 1 or patch.shape[0] != 1:
        raise NotImplementedError("batch 1, like the reference (`patch[i]` for i < data_shape[0])")
    if not moving:
        patch = patch + np.random.random() * 0.1 - 0.05      # two array operations, like the reference
    patch = torch.clamp(patch, 0.0, 1.0) * mask
    image_w, image_h = data_shape[-1], data_shape[-2]
    if not moving:
        f = 1 + 0.05 * (np.random.random() - 0.5)
        patch = zoom_device(patch.contiguous(), (f, f), 1)
        mask = zoom_device(mask.contiguous(), (f, f), 0)
        patch_init = zoom_device(patch_init.contiguous(), (f, f), 1)
    new_shape = tuple(patch.shape)
    side = patch.shape[-1]
    if not norotate:
        angle = 10 * (np.random.random() - 0.5)
        patch, patch_init = rotate_device(patch.contiguous(), angle), rotate_device(patch_init.contiguous(), angle)
    if fixed_loc[0] < 0 or fixed_loc[1] < 0:
        if center:
            x, y = (image_w - side) // 2, (image_h - side) // 2
        else:
            x = side + margin + np.random.choice(image_w - 2 * side - 2 * margin - 2)
            y = side + np.random.choice(image_h - 2 * side - 2)
        assert x + side < image_w and y + side < image_h
    else:
        x, y = fixed_loc
    C = patch.shape[1]
    canvases = [torch.empty(1, C, image_h, image_w, dtype=torch.float32, device=patch.device) for _ in range(3)]
    L.check(L.lib().ufr_patch_place(L.ptr(patch.contiguous()), L.ptr(mask.contiguous()), L.ptr(patch_init.contiguous()), C,
                                    new_shape[-2], new_shape[-1], L.ptr(canvases[0]), L.ptr(canvases[1]),
                                    L.ptr(canvases[2]), image_h, image_w, int(y), int(x), L.stream()), "patch place")
    return canvases[0], canvases[1], canvases[2], int(x), int(y), new_shape


def slot_side(side):
    """The side of a placement slot for a patch of `side` pixels: no zoom factor 1 + 0.05 * (r - 0.5), r < 1, gives more samples."""
    return int(np.ceil(side * 1.025))


@dataclass
class PlacementRecord:
    """One item's placement in PATCH coordinates, padded to `slot` x `slot` with patch 0 / mask 0 / flow 0 so that K records stack
    into the tables of csrc/patch_eval.hip.  `origin_*` = (row, column) in the frame, `size_*` = (h, w) of the zoomed patch."""
    patch_tgt: torch.Tensor          # float32 [3,slot,slot]
    mask_tgt: torch.Tensor
    patch_ref: torch.Tensor          # None when both frames show the first record
    mask_ref: torch.Tensor
    flow: torch.Tensor               # float64 [3,slot,slot] = (u, v, 1) * mask_tgt of the patch's own motion, or None
    origin_tgt: tuple
    origin_ref: tuple
    size_tgt: tuple
    size_ref: tuple
    slot: int

    def place(self):
        """(origin_tgt + size_tgt + origin_ref + size_ref): a row of the `places` table."""
        ref = (self.origin_ref + self.size_ref) if self.patch_ref is not None else (0, 0, 0, 0)
        return tuple(int(v) for v in self.origin_tgt + self.size_tgt + ref)


def _padded(x, slot, dtype):
    """[1,3,h,w] or [3,h,w] -> [3,slot,slot] of `dtype`, zero outside the h x w corner."""
    x = x.reshape(3, x.shape[-2], x.shape[-1])
    out = torch.zeros(3, slot, slot, dtype=dtype, device=x.device)
    out[:, :x.shape[-2], :x.shape[-1]] = x
    return out


def record_from_canvas(canvas_patch, canvas_mask, x, y, shape, slot):
    """The record of a one-record placement (`circle_transform_device`, `square_transform_device`) cut out of its canvases."""
    h, w = int(shape[-2]), int(shape[-1])
    cut = lambda c: _padded(c[0, :3, y:y + h, x:x + w], slot, torch.float32)
    return PlacementRecord(cut(canvas_patch), cut(canvas_mask), None, None, None, (int(y), int(x)), None, (h, w), None, slot)


def _frame_device(patch, mask, max_angle, norotate):
    """utils_patch._draw_frame with HIP tensors (the patch_init of the reference is not needed by an evaluation, and resampling it
    draws nothing).  RNG: `random()` offset, `random()` zoom factor, `random()` angle unless norotate."""
    patch = torch.clamp(patch + np.random.random() * 0.1 - 0.05, 0.0, 1.0) * mask
    f = 1 + 0.05 * (np.random.random() - 0.5)
    patch = zoom_device(patch.contiguous(), (f, f), 1)
    mask = zoom_device(mask.contiguous(), (f, f), 0)
    angle = None
    if not norotate:
        angle = max_angle * (np.random.random() - 0.5)
        patch = rotate_device(patch.contiguous(), angle)
    return patch, mask, f, angle


def circle_transform_different_device(patch, mask, patch_init, data_shape, patch_shape, margin=0, center=False, norotate=False,
                                      fixed_loc=(-1, -1), moving=False, slot=None):
    """utils_patch.circle_transform_different with HIP tensors: float64 state in, a `PlacementRecord` out -- no canvases.  The same
    numbers are drawn from `np.random` on the host in the same order (offset, zoom, [angle], [x, y], offset, zoom, [angle], u, v),
    the resampling is `ufr_affine_resample_f64`, and the flow of the patch's motion (rotation about the centre of the zoomed
    first-frame patch, translation, times zoom_ref / zoom_tgt, times the first-frame mask) is float64 device arithmetic in the
    reference's operation order.  `patch_init` is accepted for the signature's sake; an evaluation never reads its canvases."""
    from .utils_patch import draw_first_location, draw_translation
    if moving:
        raise NotImplementedError("circle_transform_different(moving=True) is broken in the reference (`patch_tgt` is unbound)")
    if data_shape[0] != 1 or patch.shape[0] != 1:
        raise NotImplementedError("batch 1, like the reference (the second frame uses the last sample's index)")
    L.require_hip(patch, "patch state", contiguous=False)
    image_w, image_h = data_shape[-1], data_shape[-2]
    slot = slot_side(patch.shape[-1]) if slot is None else int(slot)
    p_tgt, m_tgt, f_tgt, _ = _frame_device(patch, mask, 10, norotate)
    x, y = draw_first_location(image_w, image_h, patch.shape[-1], margin, center, fixed_loc)
    h, w = p_tgt.shape[-2:]
    p_ref, m_ref, f_ref, angle = _frame_device(patch, mask, 360, norotate)
    h_ref, w_ref = p_ref.shape[-2:]
    u = draw_translation(x, w_ref, image_w)
    v = draw_translation(y, h_ref, image_h)
    f64 = dict(dtype=torch.float64, device=patch.device)
    flow = torch.zeros(3, h, w, **f64)
    flow[2] = 1.0
    if angle is not None:
        rad = angle * np.pi / 180
        cm1, sn = float(np.cos(rad) - 1), float(np.sin(rad))
        cx = (torch.arange(w, **f64) - w / 2)[None, :].expand(h, w)
        cy = (torch.arange(h, **f64) - h / 2)[:, None].expand(h, w)
        flow[0] = cm1 * cx + sn * cy
        flow[1] = -sn * cx + cm1 * cy
    flow[0] += u
    flow[1] += v
    flow[:2] *= f_ref / f_tgt
    flow = flow * m_tgt[0]
    if max(h, w, h_ref, w_ref) > slot:
        raise ValueError(f"the zoomed patch ({h}x{w}, {h_ref}x{w_ref}) does not fit the {slot}x{slot} slot")
    return PlacementRecord(_padded(p_tgt, slot, torch.float32), _padded(m_tgt, slot, torch.float32),
                           _padded(p_ref, slot, torch.float32), _padded(m_ref, slot, torch.float32), _padded(flow, slot, torch.float64),
                           (int(y), int(x)), (int(y + v), int(x + u)), (int(h), int(w)), (int(h_ref), int(w_ref)), slot)


def square_transform_device(patch, mask, patch_init, data_shape, patch_shape, norotate=False):
    """utils_patch.square_transform (utils_patch.py:781-846) with HIP tensors: float64 state in, float32 canvases out.
    RNG: `choice(4)` quarter turns (unless norotate), `choice(W - S - 1)`, `choice(H - S - 1)`.  The reference rotates
    the caller's arrays in place; tensors are immutable here, so the ROTATED state is returned as well:
    (canvas_patch, canvas_mask, canvas_init, x, y, (patch, mask, patch_init) after the turns)."""
    if data_shape[0] != 1 or patch.shape[0] != 1:
        raise NotImplementedError("batch 1, like the reference (`patch[i]` for i < data_shape[0])")
    image_w, image_h = data_shape[-1], data_shape[-2]
    side = patch_shape[-1]
    if not norotate:
        turns = int(np.random.choice(4))
        patch, mask, patch_init = (torch.rot90(t, turns, (-2, -1)).contiguous() for t in (patch, mask, patch_init))
    x = int(np.random.choice(image_w - side - 1))
    y = int(np.random.choice(image_h - side - 1))
    C = patch.shape[1]
    canvases = [torch.empty(1, C, image_h, image_w, dtype=torch.float32, device=patch.device) for _ in range(3)]
    L.check(L.lib().ufr_patch_place(L.ptr(patch.contiguous()), L.ptr(mask.contiguous()), L.ptr(patch_init.contiguous()), C,
                                    patch.shape[-2], patch.shape[-1], L.ptr(canvases[0]), L.ptr(canvases[1]),
                                    L.ptr(canvases[2]), image_h, image_w, y, x, L.stream()), "patch place")
    return canvases[0], canvases[1], canvases[2], x, y, (patch, mask, patch_init)


def crop_and_restore_device(canvas_patch, canvas_mask, canvas_init, rx, ry, patch_shape, patch_shape_orig):
    """patch_attacks/main.py:408-461 on the device: mask * patch in float32, cut the zoomed patch out of the
    canvas, resample to the original size (order 1; mask order 0).  float64 state out."""
    _, C, H, W = canvas_patch.shape
    h, w = patch_shape[-2], patch_shape[-1]

    def cut(a, b):
        out = torch.empty(1, C, h, w, dtype=torch.float64, device=a.device)
        L.check(L.lib().ufr_patch_crop_f64(L.ptr(a), L.ptr(b) if b is not None else None, L.ptr(out), C, H, W, int(ry),
                                           int(rx), h, w, L.stream()), "patch crop")
        return out
    fy, fx = patch_shape_orig[2] / patch_shape[2], patch_shape_orig[3] / patch_shape[3]
    patch = zoom_device(cut(canvas_patch, canvas_mask), (fy, fx), 1)
    mask = zoom_device(cut(canvas_mask, None), (fy, fx), 0)
    patch_init = zoom_device(cut(canvas_init, None), (fy, fx), 1)
    return patch, mask, patch_init, tuple(patch.shape)
