"""Flow figures: the Middlebury colour coding of flowutils/flowlib.py:269-306 / :469-566, `tensor2array` of
patch_attacks/utils.py:21-56 and the six-panel strip of patch_attacks/test_patch.py:467-621.

Two legs.  The host functions carry the reference's names, run the same numpy statements and return the same bytes (the goldens of
tests/golden/make_golden_figures.py pin that); they are what the GPU tests compare against.  `flow_to_image` of a HIP tensor and
`viz_strip` run the kernels of csrc/flow_viz.hip and stay on the device: the reference's route is seven D2H copies and four float64
numpy passes over the frame per item.

numpy's promotion rules (NEP 50) decide the precision and the kernels restate them: `u**2 + v**2`, the square root and the maximum
run in the flow's own dtype, `maxrad + np.finfo(float).eps` is float64 and so is everything after it.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L

UNKNOWN_FLOW_THRESH = 1e7
VIZ_RECORD = 9           # UFR_VIZ_RECORD (include/ufr_hip.h)


# ---- host mirrors ------------------------------------------------------------------------------------------------------------------
def make_color_wheel():
    """The 55 x 3 Middlebury wheel, float64 in 0 .. 255: six arcs, in each one channel is full and another ramps up or down."""
    arcs = ((15, 0, 1, True), (6, 1, 0, False), (4, 1, 2, True), (11, 2, 1, False), (13, 2, 0, True), (6, 0, 2, False))
    wheel = np.zeros([sum(a[0] for a in arcs), 3])
    row = 0
    for n, full, ramped, rising in arcs:
        ramp = np.floor(255 * np.arange(0, n) / n)
        wheel[row:row + n, full] = 255
        wheel[row:row + n, ramped] = ramp if rising else 255 - ramp
        row += n
    return wheel


def color_values(u, v):
    """Normalised flow components [H,W] -> (255 * col, float64 [H,W,3], the values whose floor `compute_color` stores; the NaN
    mask).  The tests read from them where a byte hangs on the last bit of an `arctan2`."""
    nan = np.isnan(u) | np.isnan(v)
    u, v = np.where(nan, 0, u), np.where(nan, 0, v)
    wheel = make_color_wheel()
    ncols = np.size(wheel, 0)
    rad = np.sqrt(u ** 2 + v ** 2)
    a = np.arctan2(-v, -u) / np.pi
    fk = (a + 1) / 2 * (ncols - 1) + 1
    k0 = np.floor(fk).astype(int)
    k1 = k0 + 1
    k1[k1 == ncols + 1] = 1
    f = fk - k0
    inside = rad <= 1
    values = np.zeros(u.shape + (3,))
    for i in range(np.size(wheel, 1)):
        column = wheel[:, i]
        col = (1 - f) * (column[k0 - 1] / 255) + f * (column[k1 - 1] / 255)
        values[:, :, i] = 255 * np.where(inside, 1 - rad * (1 - col), col * 0.75)
    return values, nan


def compute_color(u, v):
    """Normalised flow components [H,W] -> the colour image [H,W,3] (float64 holding bytes).  Unlike the reference the arguments
    are left as they are (it zeroes their NaNs in place); a NaN gives 0."""
    values, nan = color_values(u, v)
    img = np.zeros(values.shape)
    for i in range(3):
        img[:, :, i] = np.uint8(np.floor(values[:, :, i] * (1 - nan)))
    return img


def _maxrad(u, v):
    """The reference's `np.max(np.sqrt(u**2 + v**2))`, in the dtype of u and v."""
    return np.max(np.sqrt(u ** 2 + v ** 2))


def flow_to_image(flow, maxr=-1, out=None):
    """A flow [H,W,2] (numpy) -> its Middlebury colour image, uint8 [H,W,3], bit-identical with the reference's.  Unlike the reference
    the argument is left as it is (it zeroes the unknown pixels of its argument in place).

    A HIP tensor [K,2,H,W] or [2,H,W] (float32) -> a uint8 HIP tensor [K,H,W,3] computed by `ufr_flow_to_image`; `maxr`: a scalar or
    a [K] tensor, float32 on the device; `out`: where to write, uint8 [K,H,W,3] contiguous on the flow's device."""
    if torch.is_tensor(flow):
        if flow.is_cuda:
            return _flow_to_image_device(flow, maxr, out)
        raise TypeError("flow_to_image: a numpy array [H,W,2] (host) or a HIP tensor [K,2,H,W] (device); this is a CPU tensor")
    u, v, unknown = _normalised(flow, maxr)
    img = compute_color(u, v)
    img[unknown] = 0
    return np.uint8(img)


def _normalised(flow, maxr):
    """flowlib.py:275-299: the components over max(maxr, the largest radius) + eps, unknown pixels zeroed, and the unknown mask."""
    u, v = np.array(flow[:, :, 0]), np.array(flow[:, :, 1])
    unknown = (abs(u) > UNKNOWN_FLOW_THRESH) | (abs(v) > UNKNOWN_FLOW_THRESH)
    u[unknown] = 0
    v[unknown] = 0
    maxrad = max(maxr, _maxrad(u, v))
    return u / (maxrad + np.finfo(float).eps), v / (maxrad + np.finfo(float).eps), unknown


def flow_to_image_values(flow, maxr=-1):
    """The values 255 * col whose floor `flow_to_image(flow, maxr)` stores, float64 [H,W,3] (0 at unknown pixels)."""
    u, v, unknown = _normalised(flow, maxr)
    values, nan = color_values(u, v)
    values[unknown | nan] = 0
    return values


def tensor2array(tensor, max_value=255, colormap="rainbow"):
    """patch_attacks/utils.py:21-56 for CPU tensors.  [3,H,W]: shown as it is when min >= 0 and max <= 1, else 0.5 + 0.5 * t (the
    reference's quirk: an image whose normalised values happen to lie in 0 .. 1 is not mapped back).  [2,H,W]: transposed.
    [H,W] / [1,H,W]: the reference's branch without cv2 (neither machine has it): the grey value over `max_value`, clipped."""
    if max_value is None:
        max_value = tensor.max()
    if tensor.ndimension() == 2 or tensor.size(0) == 1:
        if tensor.ndimension() == 2:
            tensor = tensor.unsqueeze(2)
        return (tensor.expand(tensor.size(0), tensor.size(1), 3).numpy() / max_value).clip(0, 1)
    if tensor.ndimension() == 3 and tensor.size(0) == 3:
        if tensor.min() >= 0 and tensor.max() <= 1:
            return tensor.numpy().transpose(1, 2, 0)
        return 0.5 + tensor.numpy().transpose(1, 2, 0) * 0.5
    if tensor.ndimension() == 3 and tensor.size(0) == 2:
        return tensor.numpy().transpose(1, 2, 0)
    raise ValueError(f"tensor2array: a tensor of shape {tuple(tensor.shape)} has no image")


def frame_panel_host(frame):
    """Panels 1 and 2 (test_patch.py:481-489, :556-560, :617-619): a pasted frame [3,H,W] (float32 CPU tensor or array) -> uint8
    [H,W,3]: custom_transforms.Normalize(0.5, 0.5) channel by channel, tensor2array, (255 * float64).astype(uint8)."""
    t = torch.as_tensor(np.array(frame, dtype=np.float32))
    for c in t:
        c.sub_(0.5).div_(0.5)
    return (255 * tensor2array(t).astype(np.float64)).astype("uint8")


def nearest_resize_host(a, H, W):
    """cv2.INTER_NEAREST of an [h,w,C] array: source index = min(floor(dst * (src / dst)), src - 1)."""
    h, w = a.shape[:2]
    iy = np.minimum(np.floor(np.arange(H) * (h / H)).astype(int), h - 1)
    ix = np.minimum(np.floor(np.arange(W) * (w / W)).astype(int), w - 1)
    return a[iy][:, ix]


def erode3_host(img):
    """cv2.erode with a 3 x 3 kernel of ones and the default border: the minimum over the neighbours that lie inside the image."""
    H, W = img.shape[:2]
    padded = np.pad(img, ((1, 1), (1, 1), (0, 0)), constant_values=255)
    return np.min([padded[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], axis=0)


def gt_panel_flow_host(g, H, W):
    """The scored ground truth [3,Hg,Wg] (float32) -> the flow of panel 6 before colour coding, float32 [H,W,3], and its largest
    radius (test_patch.py:507-524)."""
    g = np.asarray(g, dtype=np.float32)
    Hg, Wg = g.shape[1:]
    gt = np.array(nearest_resize_host(g.transpose(1, 2, 0), H, W))
    gt[:, :, 0] = gt[:, :, 0] * (W / Wg)
    gt[:, :, 1] = gt[:, :, 1] * (H / Hg)
    u, v = gt[:, :, 0], gt[:, :, 1]
    unknown = (abs(u) > UNKNOWN_FLOW_THRESH) | (abs(v) > UNKNOWN_FLOW_THRESH)
    u[unknown] = 0
    v[unknown] = 0
    return gt, _maxrad(u, v)


def viz_strip_host(adv_tgt, adv_ref, flow, adv_flow, g, maxrad_gt=None):
    """One item's strip, uint8 [H,6W,3], from the host mirrors: arrays [3,H,W], [3,H,W], [2,H,W], [2,H,W] and [3,Hg,Wg] (float32).
    `maxrad_gt` replaces the ground-truth panel's own maximum as the `maxr` of the flow panels (the goldens give one)."""
    flow, adv_flow = np.asarray(flow, dtype=np.float32), np.asarray(adv_flow, dtype=np.float32)
    H, W = flow.shape[1:]
    gt, own = gt_panel_flow_host(g, H, W)
    maxrad = own if maxrad_gt is None else np.float32(maxrad_gt)
    hwc = lambda f: f.transpose(1, 2, 0)
    panels = [frame_panel_host(adv_tgt), frame_panel_host(adv_ref), flow_to_image(hwc(flow), maxrad),
              flow_to_image(hwc(adv_flow), maxrad), flow_to_image(hwc(adv_flow - flow), maxrad),
              erode3_host(flow_to_image(gt, maxrad))]
    return np.concatenate(panels, axis=1)


# ---- device ------------------------------------------------------------------------------------------------------------------------
_wheel = None


def _wheel_ptr():
    """The host mirror's wheel as the C entries take it: 165 float64 on the host, by value in their kernel arguments."""
    global _wheel
    if _wheel is None:
        _wheel = np.ascontiguousarray(make_color_wheel(), dtype=np.float64)
    return _wheel.ctypes.data


def _flow_stack(flow, name):
    L.require_hip(flow, name, contiguous=False)
    if flow.dim() == 3:
        flow = flow[None]
    if flow.dim() != 4 or flow.shape[1] != 2 or flow.shape[0] < 1:
        raise ValueError(f"{name} must be [K,2,H,W] or [2,H,W]")
    return flow.detach().to(torch.float32).contiguous()


def _u8_out(out, shape, dev):
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=dev)
    if out.dtype != torch.uint8 or tuple(out.shape) != tuple(shape) or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor {tuple(shape)} on {dev}")
    return out


def _flow_to_image_device(flow, maxr, out):
    flow = _flow_stack(flow, "flow")
    K, _, H, W = (int(s) for s in flow.shape)
    dev = flow.device
    if torch.is_tensor(maxr):
        if maxr.numel() != K:
            raise ValueError(f"maxr must be a scalar or hold one value per item ({K})")
        maxr_d = maxr.detach().to(device=dev, dtype=torch.float32).reshape(K).contiguous()
    else:
        maxr_d = None if maxr == -1 else torch.full((K,), float(maxr), dtype=torch.float32, device=dev)
    lib = L.lib()
    with torch.cuda.device(dev):
        out = _u8_out(out, (K, H, W, 3), dev)
        ws = torch.empty(lib.ufr_flow_to_image_workspace_floats(K), dtype=torch.float32, device=dev)
        L.check(lib.ufr_flow_to_image(L.ptr(flow), L.ptr(maxr_d) if maxr_d is not None else None, _wheel_ptr(), L.ptr(out), K, H, W,
                                      L.ptr(ws), ws.numel(), L.stream()), "flow to image")
    return out


def viz_strip(adv_tgt, adv_ref, flow, adv_flow, g, maxrad_gt=None, out=None, events=None):
    """The six-panel strips of K items on the device, uint8 [K,H,6W,3]: `ufr_viz_ranges`, then `ufr_viz_strip`, no host round trip.
    adv_tgt / adv_ref [K,3,H,W], flow / adv_flow [K,2,H,W] at frame size, g [K,3,Hg,Wg] (the scored ground truth), float32 HIP
    tensors.  `maxrad_gt` (scalar or [K]) replaces the record's own value.  `events`: a `_mark(stage)` to time the two entries."""
    for name, t in (("adv_tgt", adv_tgt), ("adv_ref", adv_ref), ("flow", flow), ("adv_flow", adv_flow), ("g", g)):
        L.require_hip(t, name)
        if t.dtype != torch.float32 or t.dim() != 4:
            raise ValueError(f"{name} must be a float32 tensor of four dimensions")
    K, _, H, W = (int(s) for s in adv_tgt.shape)
    if tuple(adv_tgt.shape) != (K, 3, H, W) or adv_ref.shape != adv_tgt.shape or g.shape[:2] != (K, 3):
        raise ValueError("adv_tgt and adv_ref must be [K,3,H,W] and g [K,3,Hg,Wg]")
    if tuple(flow.shape) != (K, 2, H, W) or adv_flow.shape != flow.shape:
        raise ValueError(f"the flows must be [K,2,H,W] at the frame's size {H}x{W} (a network that answers at quarter resolution "
                         f"is not served): got {tuple(flow.shape)} and {tuple(adv_flow.shape)}")
    Hg, Wg = int(g.shape[2]), int(g.shape[3])
    dev = adv_tgt.device
    lib = L.lib()
    with torch.cuda.device(dev):
        out = _u8_out(out, (K, H, 6 * W, 3), dev)
        ws = torch.empty(lib.ufr_viz_workspace_floats(K), dtype=torch.float32, device=dev)
        record = torch.empty(K, VIZ_RECORD, dtype=torch.float32, device=dev)
        L.check(lib.ufr_viz_ranges(L.ptr(adv_tgt), L.ptr(adv_ref), L.ptr(flow), L.ptr(adv_flow), L.ptr(g), K, H, W, Hg, Wg, L.ptr(ws),
                                   ws.numel(), L.ptr(record), L.stream()), "viz ranges")
        if maxrad_gt is not None:
            record[:, 4] = torch.as_tensor(maxrad_gt, dtype=torch.float32).to(dev)
        if events is not None:
            events("ranges")
        L.check(lib.ufr_viz_strip(L.ptr(adv_tgt), L.ptr(adv_ref), L.ptr(flow), L.ptr(adv_flow), L.ptr(g), L.ptr(record), _wheel_ptr(),
                                  L.ptr(out), K, H, W, Hg, Wg, L.stream()), "viz strip")
        if events is not None:
            events("strip")
    return out
