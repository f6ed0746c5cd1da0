"""Host-side patch initialisation and placement (patch_attacks/utils_patch.py:236-358, :760-766):
`createCircularMask`, `init_patch_square`, `init_patch_circle`, `circle_transform`, and `square_transform` (:781-846); the
hand-crafted patches of the paper's tables (:13-233: `create_random_patch`, `create_correlated_patch`, `get_patch_and_mask`) and the
two-frame placement of `test_patch.py --different_pos` (:499-757, `circle_transform_different`).

These feed the inner loop once per sample; they stay on the host in numpy /
scipy like the reference so that `np.random` is consumed call for call in the same order and the
placement (an index output) is bit-exact.  The on-device transform is the next widening step
(SURVEY.md 8 f2).
"""
from __future__ import annotations

import re

import numpy as np
from scipy.ndimage import rotate, zoom


def createCircularMask(h, w, center=None, radius=None):
    """utils_patch.py:236-247: disc of radius min(distance to the walls) - 2 around the centre."""
    if center is None:
        center = [int(w / 2), int(h / 2)]
    if radius is None:
        radius = min(center[0], center[1], w - center[0], h - center[1]) - 2
    Y, X = np.ogrid[:h, :w]
    return np.sqrt((X - center[0]) ** 2 + (Y - center[1]) ** 2) <= radius


def init_patch_square(image_size, patch_size):
    """utils_patch.py:760-766: uniform [0,1) noise, side int(image_size * patch_size)."""
    side = int(image_size * patch_size)
    patch = np.random.rand(1, 3, side, side)
    return patch, patch.shape


def init_patch_circle(image_size, patch_size):
    """utils_patch.py:250-254."""
    patch, patch_shape = init_patch_square(image_size, patch_size)
    disc = createCircularMask(patch_shape[-2], patch_shape[-1]).astype("float32")
    return patch, np.array([[disc, disc, disc]]), patch.shape


def circle_transform(patch, mask, patch_init, data_shape, patch_shape, margin=0, center=False, norotate=False,
                     fixed_loc=(-1, -1), moving=False):
    """utils_patch.py:257-358.  Random brightness offset (+-0.05), zoom (1 +- 2.5%), per-sample rotation
    (+-5 deg) and placement; returns canvas-sized (patch, mask, patch_init), the corner (x, y) of the LAST
    sample and the zoomed patch shape -- the reference's return convention.  RNG draws, in order:
    offset, zoom factor, then per sample: rotation, x, y."""
    if not moving:
        patch = patch + np.random.random() * 0.1 - 0.05
    patch = np.clip(patch, 0.0, 1.0) * mask
    canvas, canvas_mask, canvas_init = np.zeros(data_shape), np.zeros(data_shape), np.zeros(data_shape)
    image_w, image_h = data_shape[-1], data_shape[-2]
    if not moving:
        f = 1 + 0.05 * (np.random.random() - 0.5)
        patch = zoom(patch, zoom=(1, 1, f, f), order=1)
        mask = zoom(mask, zoom=(1, 1, f, f), order=0)
        patch_init = zoom(patch_init, zoom=(1, 1, f, f), order=1)
    patch_shape = patch.shape
    side = patch.shape[-1]
    random_x = random_y = None
    for i in range(canvas.shape[0]):
        if not norotate:
            angle = 10 * (np.random.random() - 0.5)
            for ch in range(patch[i].shape[0]):
                patch[i][ch] = rotate(patch[i][ch], angle=angle, reshape=False, order=1)
                patch_init[i][ch] = rotate(patch_init[i][ch], angle=angle, reshape=False, order=1)
        if fixed_loc[0] < 0 or fixed_loc[1] < 0:
            if center:
                random_x = (image_w - side) // 2
            else:
                random_x = side + margin + np.random.choice(image_w - 2 * side - 2 * margin - 2)
            assert random_x + side < canvas.shape[-1]
            if center:
                random_y = (image_h - side) // 2
            else:
                random_y = side + np.random.choice(image_h - 2 * side - 2)
            assert random_y + side < canvas.shape[-2]
        else:
            random_x, random_y = fixed_loc
        ys, xs = slice(random_y, random_y + patch_shape[-2]), slice(random_x, random_x + patch_shape[-1])
        canvas[i][:, ys, xs] = patch[i]
        canvas_mask[i][:, ys, xs] = mask[i]
        canvas_init[i][:, ys, xs] = patch_init[i]
    return canvas, canvas_mask, canvas_init, random_x, random_y, patch_shape


def square_transform(patch, mask, patch_init, data_shape, patch_shape, norotate=False):
    """utils_patch.py:781-846 (`--patch_type square`, main.py:383-386): per sample a random quarter-turn count (`choice(4)`,
    applied IN PLACE to the caller's patch / mask / patch_init like the reference) and a random corner
    `choice(W - S - 1)`, `choice(H - S - 1)` (the reference's redraw loop behind it can never trigger: the draw is
    <= W - S - 2).  No brightness offset, no zoom: `patch_shape` is unchanged.  Returns canvas-sized
    (patch, mask, patch_init) and the corner (x, y) of the LAST sample."""
    canvas, canvas_mask, canvas_init = np.zeros(data_shape), np.zeros(data_shape), np.zeros(data_shape)
    image_w, image_h = data_shape[-1], data_shape[-2]
    side = patch_shape[-1]
    random_x = random_y = None
    for i in range(canvas.shape[0]):
        if not norotate:
            turns = np.random.choice(4)
            for ch in range(patch[i].shape[0]):
                patch[i][ch] = np.rot90(patch[i][ch], turns)
                mask[i][ch] = np.rot90(mask[i][ch], turns)
                patch_init[i][ch] = np.rot90(patch_init[i][ch], turns)
        random_x = np.random.choice(image_w - side - 1)
        random_y = np.random.choice(image_h - side - 1)
        ys, xs = slice(random_y, random_y + patch_shape[-2]), slice(random_x, random_x + patch_shape[-1])
        canvas[i][:3, ys, xs] = patch[i][:3]
        canvas_mask[i][:3, ys, xs] = mask[i][:3]
        canvas_init[i][:3, ys, xs] = patch_init[i][:3]
    return canvas, canvas_mask, canvas_init, random_x, random_y


def crop_and_restore(canvas_patch, canvas_mask, canvas_init, rx, ry, patch_shape, patch_shape_orig):
    """patch_attacks/main.py:408-461: cut the (zoomed) patch back out of the canvas and resample it
    to its original size (bilinear for patch / patch_init, nearest for the mask)."""
    ys, xs = slice(ry, ry + patch_shape[-2]), slice(rx, rx + patch_shape[-1])
    cut = lambda a: np.ascontiguousarray(a[:patch_shape[0], :patch_shape[1], ys, xs]).astype(np.float64)
    factors = (1, 1, patch_shape_orig[2] / patch_shape[2], patch_shape_orig[3] / patch_shape[3])
    patch = zoom(cut(canvas_patch), zoom=factors, order=1)
    mask = zoom(cut(canvas_mask), zoom=factors, order=0)
    patch_init = zoom(cut(canvas_init), zoom=factors, order=1)
    return patch, mask, patch_init, patch.shape


# ---------------------------------------------------------------------------------------- hand-crafted patches (utils_patch.py:13-233)
def _nchw(patch):
    """[S,S,3] -> [1,3,S,S], a view like the reference's transpose + newaxis."""
    return np.transpose(patch, (2, 0, 1))[np.newaxis, ...]


def create_random_patch(patch_type: str, patch_size: int):
    """utils_patch.py:38-59: `gaussian` (mean 0.5, variance 0.5) and `uniform` draw [S,S,3] numbers from `np.random`; `black`,
    `white`, `red`, `gray` are constant.  Another name leaves `patch` unbound in the reference: UnboundLocalError."""
    shape = (patch_size, patch_size, 3)
    if patch_type == "gaussian":
        patch = np.random.normal(0.5, 0.5 ** 0.5, shape)
    elif patch_type == "uniform":
        patch = np.random.uniform(0, 1, shape)
    elif patch_type in ("black", "red"):
        patch = np.zeros(shape)
        if patch_type == "red":
            patch[..., 0] = 1
    elif patch_type == "white":
        patch = np.ones(shape)
    elif patch_type == "gray":
        patch = 0.5 * np.ones(shape)
    else:
        raise UnboundLocalError(f"random patch type {patch_type!r}: the reference's `patch` is unbound for it")
    return _nchw(patch)


def get_self_correlated_patches():
    """utils_patch.py:62-74."""
    return ["hstripes", "vstripes", "vstripes_greenWhite", "vstripes_redBlack", "vstripes_redBlue", "vstripes_greenViolett",
            "vstripes_violettOrange", "checkered", "sin", "circle"]


def _columns(patch, value, thickness=2, start=0, channels=slice(None)):
    """Columns start .. start + thickness - 1, then every 2 * thickness further, of `channels` set to `value`."""
    for strip in range(start, patch.shape[1], 2 * thickness):
        patch[:, strip:strip + thickness, channels] = value


# two-colour stripes: background, colour of the strips from column 0, colour of the strips from column 2 (None: background)
_TWO_COLOUR = (("vstripes_greenWhite", 1.0, (0, 1, 0), None), ("vstripes_redBlack", 0.0, (1, 0, 0), None),
               ("vstripes_redBlue", 0.0, (1, 0, 0), (0, 0, 1)), ("vstripes_violettOrange", 0.0, (0.9, 0.7, 0.3), (0.8, 0.1, 0.8)),
               ("vstripes_greenViolett", 0.0, (0.7, 0.8, 0.1), (0.6, 0.0, 0.6)))


def create_correlated_patch(patch_type: str, patch_size: int):
    """utils_patch.py:77-233: the self-similar patterns of the paper.  `hstripes`, `checkered`, `sin`, `circle` match by equality,
    everything else by SUBSTRING in the reference's order (colour pairs, `vstripes_strip<N>`, `vstripes_rot<angle>`,
    `vstripes_Bcol<c>_col<d>`, `vstripes_Bcol<c>`, `vstripes_col<c>`, then any name holding `vstripes`).  `checkered` / `circle`
    use strips of S // 48 and `sin` of S // 24: a smaller S gives `range(0, S, 0)`, a ValueError.  `sin` draws from `np.random`
    (two `randint` per strip) although no draw can change the result.  `circle` needs cv2.circle, which this project does not
    carry: NotImplementedError.  Another name raises the reference's Exception."""
    S = patch_size
    two = next((t for t in _TWO_COLOUR if t[0] in patch_type), None)
    if patch_type == "hstripes":
        patch = np.zeros((S, S, 3))
        for strip in range(0, S, 4):
            patch[strip:strip + 2, :, :] = 1
    elif two is not None:
        _, background, first, second = two
        patch = np.full((S, S, 3), background)
        for c in range(3):
            # greenWhite and redBlack write only the channels that differ from the background; the values agree either way
            _columns(patch, first[c], channels=c)
            if second is not None:
                _columns(patch, second[c], start=2, channels=c)
    elif "vstripes_strip" in patch_type:
        patch = np.zeros((S, S, 3))
        _columns(patch, 1, thickness=int(re.findall(r"\d+", patch_type)[0]))
    elif "vstripes_rot" in patch_type:
        patch = np.zeros((2 * S, 2 * S, 3))
        _columns(patch, 1)
        patch = rotate(patch, angle=int(re.findall(r"\d+", patch_type)[0]), reshape=False, order=1)
        q = 2 * S // 4
        patch = patch[q:q + S, q:q + S, :]
    elif "vstripes_Bcol" in patch_type and "_col" in patch_type:
        numbers = re.findall(r"[-+]?\d*\.\d+|\d+", patch_type)
        patch = np.ones((S, S, 3)) * float(numbers[0])
        _columns(patch, float(numbers[1]))
    elif "vstripes_Bcol" in patch_type:
        patch = np.ones((S, S, 3)) * float(re.findall(r"\d+\.\d+", patch_type)[0])
        _columns(patch, 1)
    elif "vstripes_col" in patch_type:
        patch = np.zeros((S, S, 3))
        _columns(patch, float(re.findall(r"\d+\.\d+", patch_type)[0]))
    elif "vstripes" in patch_type:
        patch = np.zeros((S, S, 3))
        _columns(patch, 1)
    elif patch_type == "checkered":
        patch = np.ones((S, S, 3))
        t = S // 48
        for strip in range(0, S, 2 * t):
            patch[strip:strip + t, :, :] = 0
            patch[:, strip:strip + t, :] = 0
    elif patch_type == "sin":
        patch = np.zeros((S, S, 3))
        t = S // 24
        wave = 5 * np.sin(2 * np.pi * np.arange(0, S) / (0.25 * S)) + 5
        for strip in range(0, S, 2 * t):
            if np.random.randint(0, 2) >= 0:                 # always: the draw is kept for the RNG order
                white = np.random.randint(1, 2)              # always 1
                patch[strip:strip + white, :, :] = 1
            for i, y in enumerate(wave):
                top = int(y) + strip
                if top > S:
                    continue
                if S < top + t:
                    patch[top:, :, :] = 0                    # the reference writes 1, then 0
                patch[top:top + t, i, 2] = 1
                patch[top:top + t, i, 0] = 0
    elif patch_type == "circle":
        raise NotImplementedError("the `circle` pattern is drawn by cv2.circle in the reference; cv2 is not a dependency of this "
                                  "project and no expected values can be made without it")
    else:
        raise Exception("Self correlation type is not implemented")
    return _nchw(patch)


def get_patch_and_mask(args):
    """utils_patch.py:13-35: (patch, patch_shape, mask) from `args.self_correlated_patch`, `args.random_patch` or the checkpoint at
    `args.patch_path`; a disc (`patch_type == "circle"`) or all-ones (`"square"`) mask.  `args.mask_path` calls a `cv2.imresize`
    that does not exist in the reference: NotImplementedError."""
    if getattr(args, "self_correlated_patch", ""):
        patch = create_correlated_patch(args.self_correlated_patch, args.patch_size)
    elif getattr(args, "random_patch", ""):
        patch = create_random_patch(args.random_patch, args.patch_size)
    else:
        from .kitti_io import load_patch
        patch = load_patch(args.patch_path)
    patch_shape = patch.shape
    if getattr(args, "mask_path", ""):
        raise NotImplementedError("mask_path: the reference's branch calls cv2.imresize, which does not exist; use patch_type "
                                  "circle or square")
    if args.patch_type == "circle":
        disc = createCircularMask(patch_shape[-2], patch_shape[-1]).astype("float32")
        mask = np.array([[disc, disc, disc]])
    elif args.patch_type == "square":
        mask = np.ones(patch_shape)
    else:
        raise UnboundLocalError(f"patch_type {args.patch_type!r}: the reference's `mask` is unbound for it (circle or square)")
    return patch, patch_shape, mask


# ---------------------------------------------------------------------------------- two-frame placement (utils_patch.py:499-757)
def _draw_frame(patch, mask, patch_init, max_angle, norotate):
    """One frame's appearance: brightness offset, clip, mask, zoom (mask at order 0, never rotated), rotation of +-max_angle / 2.
    RNG: `random()` offset, `random()` zoom factor, `random()` angle unless norotate.  Returns (patch, mask, patch_init, zoom
    factor, angle or None)."""
    patch = np.clip(patch + np.random.random() * 0.1 - 0.05, 0.0, 1.0) * mask
    f = 1 + 0.05 * (np.random.random() - 0.5)
    patch = zoom(patch, zoom=(1, 1, f, f), order=1)
    mask = zoom(mask, zoom=(1, 1, f, f), order=0)
    patch_init = zoom(patch_init, zoom=(1, 1, f, f), order=1)
    angle = None
    if not norotate:
        angle = max_angle * (np.random.random() - 0.5)
        for ch in range(patch[0].shape[0]):
            patch[0][ch] = rotate(patch[0][ch], angle=angle, reshape=False, order=1)
            patch_init[0][ch] = rotate(patch_init[0][ch], angle=angle, reshape=False, order=1)
    return patch, mask, patch_init, f, angle


def draw_first_location(image_w, image_h, side, margin, center, fixed_loc):
    """utils_patch.py:549-571: the first frame's corner (x, y) from the UNZOOMED side; `choice` twice unless fixed or centred."""
    if fixed_loc[0] < 0 or fixed_loc[1] < 0:
        if center:
            x, y = (image_w - side) // 2, (image_h - side) // 2
        else:
            x = side + margin + np.random.choice(image_w - 2 * side - 2 * margin - 2)
            y = side + np.random.choice(image_h - 2 * side - 2)
        assert x + side < image_w and y + side < image_h
        return x, y
    return fixed_loc[0], fixed_loc[1]


def draw_translation(origin, size, limit):
    """utils_patch.py:666-678: round(+-100 px) from one `random()`, moved back into [0, limit - size] a pixel at a time."""
    t = round(100 * ((np.random.random() - 0.5) / 0.5))
    while t + origin < 0:
        t += 1
    while t + origin + size > limit:
        t -= 1
    return t


def rotation_flow(h, w, angle):
    """utils_patch.py:647-663: the displacement [2,h,w] of a turn by `angle` degrees about (w / 2, h / 2) of the zoomed first-frame
    patch, on the grid `np.mgrid[:w, :h].T` (x = column, y = row)."""
    rad = angle * np.pi / 180
    coords = np.mgrid[:w, :h].T + np.zeros((h, w, 2))
    coords -= np.array([w / 2, h / 2])
    out = np.zeros((h, w, 2))
    out[..., 0] = (np.cos(rad) - 1) * coords[..., 0] + np.sin(rad) * coords[..., 1]
    out[..., 1] = -np.sin(rad) * coords[..., 0] + (np.cos(rad) - 1) * coords[..., 1]
    return (np.zeros((h, w, 2)) + out).transpose(2, 0, 1)


def circle_transform_different(patch, mask, patch_init, data_shape, patch_shape, margin=0, center=False, norotate=False,
                               fixed_loc=(-1, -1), moving=False):
    """utils_patch.py:499-757 (`test_patch.py --different_pos`): two independent appearance draws of the patch -- the first frame
    turns by +-5 deg, the second by +-180 deg -- a translation of +-100 px clipped into the frame, and the flow field of the
    patch's own motion (rotation about the first frame's patch centre, plus translation, times zoom_ref / zoom_tgt; channel 2
    is the first-frame mask).  RNG in order: offset, zoom, [angle], [x, y], offset, zoom, [angle], u, v.  Returns
    ([x_tgt, x_ref], [xm_tgt, xm_ref], out_flow, [xp_tgt, xp_ref], [x, x_ref], [y, y_ref], patch_shape), canvases float64."""
    if moving:
        raise NotImplementedError("circle_transform_different(moving=True) is broken in the reference (`patch_tgt` is unbound)")
    if data_shape[0] != 1 or patch.shape[0] != 1:
        raise NotImplementedError("batch 1, like the reference (the second frame uses the last sample's index)")
    image_w, image_h = data_shape[-1], data_shape[-2]
    p_tgt, m_tgt, i_tgt, f_tgt, _ = _draw_frame(patch, mask, patch_init, 10, norotate)
    x, y = draw_first_location(image_w, image_h, patch.shape[-1], margin, center, fixed_loc)
    h, w = p_tgt.shape[-2:]
    flow = np.zeros_like(p_tgt)
    flow[:, -1, ...] = 1
    p_ref, m_ref, i_ref, f_ref, angle = _draw_frame(patch, mask, patch_init, 360, norotate)
    if angle is not None:
        flow[0, :2] = rotation_flow(h, w, angle)
    h_ref, w_ref = p_ref.shape[-2:]
    u = draw_translation(x, w_ref, image_w)
    v = draw_translation(y, h_ref, image_h)
    x_ref, y_ref = x + u, y + v
    flow[:, 0, ...] += u
    flow[:, 1, ...] += v
    flow[:, :2, ...] *= f_ref / f_tgt

    def place(a, yy, xx):
        canvas = np.zeros(data_shape)
        canvas[0][:3, yy:yy + a.shape[-2], xx:xx + a.shape[-1]] = a[0][:3]
        return canvas
    out_flow = place(flow * m_tgt, y, x)
    return ([place(p_tgt, y, x), place(p_ref, y_ref, x_ref)], [place(m_tgt, y, x), place(m_ref, y_ref, x_ref)], out_flow,
            [place(i_tgt, y, x), place(i_ref, y_ref, x_ref)], [x, x_ref], [y, y_ref], patch_shape)
