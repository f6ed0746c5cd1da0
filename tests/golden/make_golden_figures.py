"""Golden fixtures of the flow figures, produced by running the REFERENCE's own `flowutils/flowlib.py` (`make_color_wheel`,
`flow_to_image`), `patch_attacks/utils.py` (`tensor2array`) and `dataset_utils/custom_transforms.py` (`Normalize`) on the CPU through
ref_harness; see make_golden.py for the contract.

    python tests/golden/make_golden_figures.py

figures_flow_to_image   the colour wheel; `flow_to_image` on 13 x 37 and 24 x 40 flows as float32 and float64, with maxr = -1, a value
                        below the flow's own maximum and one above it.  Every flow holds axis-aligned vectors, zero vectors and an
                        unknown pixel above 1e7.
figures_tensor2array    both 3-channel branches (an image inside 0 .. 1, one outside) and 2 channels.
figures_panels          the five panels of one 24 x 40 item that need neither cv2.resize nor cv2.erode, assembled with the script's
                        expressions (patch_attacks/test_patch.py:481-489, :532-560, :617-619) for a given maxrad.
figures_csv             the lines of the result files for fixed numbers: the format strings are READ from the reference's
                        test_patch.py and test_moving_patch.py (their `main` cannot be called), not restated.

Before anything is written every stored colour byte's value before `floor` (restated here in float64) must lie more than 1e-6 from
an integer, so that no fixture hangs on the last bit of an `atan2`.  Two kinds of value are exact integers by construction and exempt.
Pixels whose normalised vector has a zero component: their angle is one of atan2's exact special cases and nothing transcendental
enters.  And a channel whose two wheel neighbours are equal (every hue has one saturated channel): (1 - f) * c + f * c is c for every
f (for c = 1: 1 - f is exact above one half and off by at most 2**-54 below it, which the sum rounds away), so the 255 of a vector
inside the unit circle does not depend on the angle's last bit.
"""
from __future__ import annotations

import ast
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_harness as rh  # noqa: E402
from make_golden import save  # noqa: E402

MARGIN = 1e-6
SIZES = ((13, 37), (24, 40))
CSV_ITEMS = ((0, 1.23456, 23.456789, 0.98765, -0.123456), (7, 0.00004, 100.00005, -1.0, 0.5), (123, 12.5, 3.25, 0.125, 0.99995))
CSV_AVG = (4.589873333333333, 42.23561333333333, 0.0375499999999999, 0.458831)
MOVING_SCENE = (3, 1.23456, 9.87654, 2.00005, 8.5, 19.99995, 0.98765, 0.12344, -0.5, 0.25, 0.75)
MOVING_TOTAL = (1.5, 9.87655, 2.12345, 8.0, 20.0, 0.9, 0.1, -0.55555, 0.33333, 0.66667)


def flow_case(H, W, seed):
    """A float32 flow [H,W,2] with the special pixels of the issue in its first row."""
    rng = np.random.RandomState(seed)
    flow = (rng.randn(H, W, 2) * 3.0).astype(np.float32)
    flow[0, 0] = (2.5, 0.0)
    flow[0, 1] = (-1.75, 0.0)
    flow[0, 2] = (0.0, 3.25)
    flow[0, 3] = (0.0, -0.5)
    flow[0, 4] = (0.0, 0.0)
    flow[0, 5] = (0.0, 0.0)
    flow[0, 6] = (2.0e7, 1.0)
    flow[1, 0] = (1.0, -3.0e7)
    return flow


def prefloor(flow, maxr):
    """255 * col of every pixel and channel, float64 [H,W,3], and the mask [H,W,3] of the exempt values (the module's docstring)."""
    u, v = np.array(flow[:, :, 0]), np.array(flow[:, :, 1])
    unknown = (abs(u) > 1e7) | (abs(v) > 1e7)
    u[unknown] = 0
    v[unknown] = 0
    maxrad = max(maxr, np.max(np.sqrt(u ** 2 + v ** 2)))
    u, v = u / (maxrad + np.finfo(float).eps), v / (maxrad + np.finfo(float).eps)
    wheel = rh.ref_module("flowutils.flowlib").make_color_wheel()
    rad = np.sqrt(u ** 2 + v ** 2)
    fk = (np.arctan2(-v, -u) / np.pi + 1) / 2 * 54 + 1
    k0 = np.floor(fk).astype(int)
    k1 = np.where(k0 + 1 == 56, 1, k0 + 1)
    f = fk - k0
    out, exempt = np.zeros(u.shape + (3,)), np.zeros(u.shape + (3,), dtype=bool)
    for c in range(3):
        col = (1 - f) * (wheel[k0 - 1, c] / 255) + f * (wheel[k1 - 1, c] / 255)
        out[:, :, c] = 255 * np.where(rad <= 1, 1 - rad * (1 - col), col * 0.75)
        exempt[:, :, c] = unknown | (u == 0) | (v == 0) | ((wheel[k0 - 1, c] == wheel[k1 - 1, c]) & (out[:, :, c] == np.round(out[:, :, c])))
    return out, exempt


class TooClose(Exception):
    pass


def check_margin(name, flow, maxr, image):
    values, exempt = prefloor(flow, maxr)
    assert np.array_equal(np.floor(values)[~exempt], image[~exempt].astype(np.float64)), f"{name}: the restatement disagrees"
    distance = np.abs(values - np.round(values))[~exempt]
    if not distance.min() > MARGIN:
        raise TooClose(f"{name}: a value {distance.min():.3e} from an integer")


def first_seed(start, build):
    """`build(seed)` for the first seed from `start` upward whose every byte keeps the margin (deterministic: same seed every run)."""
    for seed in range(start, start + 200):
        try:
            out = build(seed)
        except TooClose as e:
            print(f"  seed {seed} skipped: {e}")
            continue
        print(f"  seed {seed}")
        return out
    raise AssertionError("no seed keeps the margin")


def gen_flow_to_image():
    fl = rh.ref_module("flowutils.flowlib")
    arrays = {"wheel": fl.make_color_wheel()}

    def cases(H, W, seed):
        arrays = {}
        base = flow_case(H, W, seed)
        known = base[(np.abs(base) <= 1e7).all(axis=2)]
        own = float(np.sqrt((known.astype(np.float64) ** 2).sum(axis=1)).max())
        for dtype in (np.float32, np.float64):
            for tag, maxr in (("own", -1), ("below", np.float32(0.5 * own)), ("above", np.float32(1.5 * own))):
                key = f"{H}x{W}_{np.dtype(dtype).name}_{tag}"
                flow = base.astype(dtype)
                image = fl.flow_to_image(flow.copy(), maxr)                   # the reference zeroes unknown pixels in place
                assert image.dtype == np.uint8 and image.shape == (H, W, 3)
                check_margin(key, flow, maxr, image)
                arrays["flow_" + key], arrays["maxr_" + key], arrays["image_" + key] = flow, np.asarray(maxr), image
        return arrays

    for H, W in SIZES:
        arrays.update(first_seed(H * 100 + W, lambda seed: cases(H, W, seed)))
    save("figures_flow_to_image", **arrays)


def gen_tensor2array():
    t2a = rh.ref_module("patch_attacks.utils").tensor2array
    rng = np.random.RandomState(5)
    inside = torch.from_numpy(rng.rand(3, 13, 37).astype(np.float32))
    outside = torch.from_numpy((rng.rand(3, 13, 37) * 2 - 1).astype(np.float32))
    two = torch.from_numpy(rng.randn(2, 13, 37).astype(np.float32))
    save("figures_tensor2array", inside=inside, inside_out=t2a(inside.clone()), outside=outside, outside_out=t2a(outside.clone()),
         two=two, two_out=t2a(two.clone()))


def gen_panels():
    first_seed(77, _gen_panels)


def _gen_panels(seed):
    fl = rh.ref_module("flowutils.flowlib")
    utils = rh.ref_module("patch_attacks.utils")
    normalize = rh.ref_module("dataset_utils.custom_transforms").Normalize(mean=[0.5, 0.5, 0.5], std=[0.5, 0.5, 0.5])
    flow_to_image, tensor2array, transpose_image = fl.flow_to_image, utils.tensor2array, utils.transpose_image
    H, W = SIZES[1]
    rng = np.random.RandomState(seed)
    adv_tgt = torch.from_numpy(rng.rand(1, 3, H, W).astype(np.float32))                  # min < 0.5: mapped back by 0.5 + 0.5 * n
    adv_ref = torch.from_numpy((0.5 + 0.5 * rng.rand(1, 3, H, W)).astype(np.float32))    # all >= 0.5: the quirk branch, shown as n
    flow_fwd = torch.from_numpy((rng.randn(1, 2, H, W) * 4).astype(np.float32))
    adv_flow_fwd = torch.from_numpy((rng.randn(1, 2, H, W) * 4).astype(np.float32))
    maxrad = np.float32(9.5)                     # below the largest radius of these flows, above that of most pixels
    # the frames' bytes must not hang on a last bit either
    for frame, as_is in ((adv_tgt, False), (adv_ref, True)):
        n = (frame.numpy() - np.float32(0.5)) / np.float32(0.5)
        a = (n if as_is else np.float32(0.5) + n * np.float32(0.5)).astype(np.float64) * 255
        assert (n.min() >= 0 and n.max() <= 1) == as_is
        distance = np.abs(a - np.round(a))
        assert distance[distance > 0].min() > MARGIN                                      # an exact integer is exact everywhere
    for name, f in (("flow", flow_fwd), ("adv", adv_flow_fwd), ("diff", adv_flow_fwd - flow_fwd)):
        f = f[0].numpy().transpose(1, 2, 0)
        check_margin("panels " + name, f, maxrad, flow_to_image(f.copy(), maxrad))
    # ---- the script's expressions ----
    adv_norm_tgt_img = normalize(adv_tgt.clone())
    adv_norm_ref_img = normalize(adv_ref.clone())
    val_Flow_Output = transpose_image(flow_to_image(tensor2array(flow_fwd.data[0].cpu()), maxrad)) / 255.0
    val_adv_Flow_Output = transpose_image(flow_to_image(tensor2array(adv_flow_fwd.data[0].cpu()), maxrad)) / 255.0
    val_Diff_Flow_Output = transpose_image(flow_to_image(tensor2array((adv_flow_fwd - flow_fwd).data[0].cpu()), maxrad)) / 255.0
    val_adv_tgt_image = transpose_image(tensor2array(adv_norm_tgt_img[0]))
    val_adv_ref_image = transpose_image(tensor2array(adv_norm_ref_img[0]))
    val_output_viz = np.concatenate((val_adv_tgt_image, val_adv_ref_image, val_Flow_Output, val_adv_Flow_Output,
                                     val_Diff_Flow_Output), 2)
    strip = (255 * val_output_viz.transpose(1, 2, 0)).astype("uint8")
    assert strip.shape == (H, 5 * W, 3)
    save("figures_panels", adv_tgt=adv_tgt, adv_ref=adv_ref, flow=flow_fwd, adv_flow=adv_flow_fwd, maxrad=maxrad, strip=strip)


def _format_strings(path, joined):
    """The literals that `path` formats its result lines with, in source order: the constants `.format` is called on, or (`joined`)
    the f-strings, as (template, field expressions) with `{}` where a value goes."""
    found = []
    for node in ast.walk(ast.parse(open(path).read())):
        if not joined and isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "format" \
                and isinstance(node.func.value, ast.Constant) and isinstance(node.func.value.value, str):
            found.append((node.lineno, node.func.value.value))
        if joined and isinstance(node, ast.JoinedStr):
            template = "".join(v.value if isinstance(v, ast.Constant) else "{}" for v in node.values)
            fields = [ast.unparse(v.value) for v in node.values if isinstance(v, ast.FormattedValue)]
            found.append((node.lineno, (template, fields)))
    return [f for _, f in sorted(found, key=lambda t: t[0])]


def gen_csv():
    names = ["epe", "adv_epe", "cos_sim", "adv_cos_sim"]
    fmts = [f for f in _format_strings(os.path.join(rh.REF, "patch_attacks/test_patch.py"), False) if f.endswith("\n")]
    header, scene_header, item, avg, scene_avg = fmts                               # test_patch.py:231, :234, :625, :637, :640
    lines = {"header": header.format(*names), "scene_header": scene_header.format(*(["scene"] + names)),
             "items": [item.format(*row) for row in CSV_ITEMS], "avg": avg.format(*CSV_AVG),
             "scene_avg": scene_avg.format(*(["avg"] + list(CSV_AVG)))}
    moving = [f for f in _format_strings(os.path.join(rh.REF, "patch_attacks/test_moving_patch.py"), True)
              if f[0].endswith("\n") and len(f[1]) >= 10]
    # test_moving_patch.py:240, :244 (headers over result_error_names), :503 (scene row), :674 (the one row of moving_results.csv)
    heads = [f for f in moving if all(x.startswith("result_error_names") for x in f[1])]
    scene_row = [f for f in moving if f[1][0] == "i" and len(f[1]) == 11][0][0]
    total_row = [f for f in moving if len(f[1]) == 10 and all(x.startswith("round(") for x in f[1])][0][0]
    assert len(heads) == 2
    src = open(os.path.join(rh.REF, "patch_attacks/test_moving_patch.py")).read()
    tree = ast.parse(src)
    result_names = None
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "result_error_names" for t in node.targets):
            result_names = ast.literal_eval(node.value)
    assert result_names is not None and len(result_names) == 10
    lines["moving_header"] = heads[0][0].format(*result_names)
    lines["moving_scene_header"] = heads[1][0].format(*result_names)
    lines["moving_scene"] = scene_row.format(MOVING_SCENE[0], *[round(x, 4) for x in MOVING_SCENE[1:]])
    lines["moving_total"] = total_row.format(*[round(x, 4) for x in MOVING_TOTAL])
    save("figures_csv", items_in=np.asarray(CSV_ITEMS), avg_in=np.asarray(CSV_AVG), moving_scene_in=np.asarray(MOVING_SCENE),
         moving_total_in=np.asarray(MOVING_TOTAL), result_names=np.asarray(result_names),
         **{k: np.asarray(v) for k, v in lines.items()})
    for k, v in lines.items():
        print(k, repr(v))


if __name__ == "__main__":
    rh.install()
    gen_flow_to_image()
    gen_tensor2array()
    gen_panels()
    gen_csv()
