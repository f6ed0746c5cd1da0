"""CPU suite of the flow figures (understanding_flow_robustness_amd/flowlib.py, the files of patch_eval.py and patch_sweep.py): the
host mirrors return the reference's bytes on every golden of tests/golden/make_golden_figures.py, and the result files carry the
reference's lines character for character."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def test_color_wheel_equals_the_reference():
    from understanding_flow_robustness_amd import flowlib
    wheel = flowlib.make_color_wheel()
    want = _golden("figures_flow_to_image")["wheel"]
    assert wheel.dtype == np.float64 and wheel.shape == (55, 3) and np.array_equal(wheel, want)
    assert flowlib.UNKNOWN_FLOW_THRESH == 1e7


def test_flow_to_image_equals_every_golden():
    from understanding_flow_robustness_amd import flowlib
    g = _golden("figures_flow_to_image")
    keys = sorted(k[len("flow_"):] for k in g.files if k.startswith("flow_"))
    assert len(keys) == 12                                       # two sizes x two dtypes x three maxr
    for key in keys:
        flow, maxr, want = g["flow_" + key], g["maxr_" + key], g["image_" + key]
        maxr = -1 if maxr.dtype.kind == "i" else maxr[()]         # the scalar as it was given: the int -1 or a float32
        before = flow.copy()
        got = flowlib.flow_to_image(flow, maxr)
        assert got.dtype == np.uint8 and np.array_equal(got, want), key
        assert np.array_equal(flow, before)                      # the mirror leaves its argument alone
        unknown = (np.abs(flow) > 1e7).any(axis=2)
        assert unknown.sum() == 2 and not got[unknown].any()
        zero = (flow == 0).all(axis=2)
        assert zero.sum() == 2 and (got[zero] == 255).all()


def test_compute_color_leaves_its_arguments_and_zeroes_nan():
    from understanding_flow_robustness_amd import flowlib
    u, v = np.array([[0.25, np.nan, 0.0]]), np.array([[-0.5, 0.1, 0.0]])
    u0, v0 = u.copy(), v.copy()
    img = flowlib.compute_color(u, v)
    assert np.array_equal(u, u0, equal_nan=True) and np.array_equal(v, v0)
    assert img.shape == (1, 3, 3) and not img[0, 1].any() and (img[0, 2] == 255).all()


def test_tensor2array_equals_every_golden():
    from understanding_flow_robustness_amd import flowlib
    g = _golden("figures_tensor2array")
    for name in ("inside", "outside", "two"):
        got = flowlib.tensor2array(torch.from_numpy(g[name]))
        want = g[name + "_out"]
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), name
    assert g["inside"].min() >= 0 and g["inside"].max() <= 1 and g["outside"].min() < 0      # both 3-channel branches
    assert np.array_equal(g["inside_out"], g["inside"].transpose(1, 2, 0))                   # shown as it is
    # one channel: the reference's branch without cv2
    grey = torch.tensor([[0.0, 127.5], [255.0, 510.0]])
    got = flowlib.tensor2array(grey)
    assert got.shape == (2, 2, 3) and np.array_equal(got[:, :, 0], np.array([[0.0, 0.5], [1.0, 1.0]], dtype=np.float32))
    assert tuple(grey.shape) == (2, 2)                                                        # not unsqueezed in place
    with pytest.raises(ValueError):
        flowlib.tensor2array(torch.zeros(4, 2, 2))


def test_five_panels_equal_the_reference():
    """The panels that need neither cv2.resize nor cv2.erode, against the bytes the script's own expressions gave."""
    from understanding_flow_robustness_amd import flowlib
    g = _golden("figures_panels")
    H, W = g["flow"].shape[2:]
    gt = np.zeros((3, H, W), dtype=np.float32)
    strip = flowlib.viz_strip_host(g["adv_tgt"][0], g["adv_ref"][0], g["flow"][0], g["adv_flow"][0], gt, maxrad_gt=g["maxrad"][()])
    assert strip.dtype == np.uint8 and strip.shape == (H, 6 * W, 3)
    assert np.array_equal(strip[:, :5 * W], g["strip"])
    assert (strip[:, 5 * W:] == 255).all()                                                    # a zero ground truth is white
    # the second frame is all >= 0.5: the quirk branch shows the normalised values themselves
    assert g["adv_ref"].min() >= 0.5 and g["adv_tgt"].min() < 0.5


def test_nearest_resize_and_erode_follow_their_definitions():
    from understanding_flow_robustness_amd import flowlib
    a = np.arange(5 * 7 * 2).reshape(5, 7, 2)
    for H, W in ((3, 4), (5, 7), (11, 20)):
        got = flowlib.nearest_resize_host(a, H, W)
        for y in range(H):
            for x in range(W):
                assert np.array_equal(got[y, x], a[min(int(np.floor(y * (5 / H))), 4), min(int(np.floor(x * (7 / W))), 6)])
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, size=(6, 9, 3)).astype(np.uint8)
    got = flowlib.erode3_host(img)
    for y in range(6):
        for x in range(9):
            want = img[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].reshape(-1, 3).min(axis=0)
            assert np.array_equal(got[y, x], want)


def test_csv_lines_equal_the_reference():
    from understanding_flow_robustness_amd.patch_eval import EvalResult
    g = _golden("figures_csv")
    items = g["items_in"]
    result = EvalResult(items[:, 1:], items[:, 1:].mean(axis=0), [], ["epe", "adv_epe", "cos_sim", "adv_cos_sim"])
    results, scenes = result.csv_text()
    lines = scenes.splitlines(keepends=True)
    assert lines[0] == str(g["scene_header"]) and results.splitlines(keepends=True)[0] == str(g["header"])
    # the golden's items carry the indices 0, 7, 123, the result counts 0, 1, 2: one format for every index
    for i, (line, want, index) in enumerate(zip(lines[1:4], g["items"], items[:, 0])):
        want = str(want)
        assert line[10:] == want[10:] and want[:10] == "%10d" % index and line[:10] == "%10d" % i
    # the average line with the golden's numbers
    avg = EvalResult(g["avg_in"][None], g["avg_in"], [], result.error_names).csv_text()
    assert avg[0].splitlines(keepends=True)[1] == str(g["avg"])
    assert avg[1].splitlines(keepends=True)[2] == str(g["scene_avg"])
    # the running average of this result
    total = [0.0] * 4
    for row in items[:, 1:]:
        total = [t + float(v) for t, v in zip(total, row)]
    assert results.splitlines(keepends=True)[1] == "{:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}\n".format(*[t / 3 for t in total])


def test_write_csv_names_and_output_dirs(tmp_path):
    from argparse import Namespace

    from understanding_flow_robustness_amd import patch_eval as pe
    result = pe.EvalResult(np.array([[1.0, 2.0, 0.5, 0.25]]), np.array([1.0, 2.0, 0.5, 0.25]), [], ["epe", "adv_epe", "cos_sim",
                                                                                                    "adv_cos_sim"])
    a, b = result.write_csv(str(tmp_path / "plain"))
    assert (os.path.basename(a), os.path.basename(b)) == ("test_results.csv", "test_result_scenes.csv")
    assert (open(a).read(), open(b).read()) == result.csv_text()
    a, b = result.write_csv(str(tmp_path / "moved"), different_pos=True)
    assert (os.path.basename(a), os.path.basename(b)) == ("test_results_diff_pos.csv", "test_result_scenes_diff_pos.csv")
    root = str(tmp_path)
    assert pe.output_dirs(root, Namespace()) == (root, os.path.join(root, "images_test"))
    assert pe.output_dirs(root, Namespace(different_pos=True)) == (root, os.path.join(root, "images_test_diff_pos"))
    homog = os.path.join(root, "homogenuous_img")
    assert pe.output_dirs(root, Namespace(HOMOGENUOUS=True, different_pos=True)) == (homog, homog)
    with pytest.raises(ValueError):
        pe.checked_image_format("bmp")
    assert pe.checked_image_format("png") == "png"


def test_moving_csv_lines_equal_the_reference():
    from understanding_flow_robustness_amd import patch_sweep as ps
    g = _golden("figures_csv")
    assert list(g["result_names"]) == ps.RESULT_NAMES
    header, scene_header = ps.moving_headers()
    assert header == str(g["moving_header"]) and scene_header == str(g["moving_scene_header"])
    scene = g["moving_scene_in"]
    assert ps.moving_scene_line(int(scene[0]), [float(v) for v in scene[1:]]) == str(g["moving_scene"])
    assert ps.moving_total_line([float(v) for v in g["moving_total_in"]]) == str(g["moving_total"])


def test_sweep_statistics_equal_numpys_on_a_fixed_map():
    """The statistics `sweep_scenes` reports per scene, from a fixed pair of maps: numpy's mean, minimum, median and maximum (dyadic
    values, so the script's running sum is exact too), in the script's visiting order."""
    from understanding_flow_robustness_amd import patch_sweep as ps
    rng = np.random.RandomState(3)
    adv_epe = rng.randint(1, 4096, size=(3, 5)) / 64.0
    adv_cos = rng.randint(1, 64, size=(3, 5)) / 64.0
    stats = ps.scene_statistics(adv_epe, adv_cos)
    for name, m in (("adv_epe", adv_epe), ("adv_cos_sim", adv_cos)):
        assert stats[name + "_avg"] == np.mean(m) and stats[name + "_min"] == np.min(m)
        assert stats[name + "_median"] == float(np.median(m)) and stats[name + "_max"] == np.max(m)
    # the script's meter starts its maximum at 0 and its minimum at 10e6: a map of negative cosines reports a maximum of 0
    stats = ps.scene_statistics(adv_epe, -adv_cos)
    assert stats["adv_cos_sim_max"] == 0 and stats["adv_cos_sim_min"] == np.min(-adv_cos)
    assert stats["adv_cos_sim_median"] == float(np.median(-adv_cos))


def test_zoomed_map_is_scipys_zoom():
    from scipy.ndimage import zoom

    from understanding_flow_robustness_amd import patch_sweep as ps
    m = np.random.RandomState(1).rand(3, 7)
    got = ps.zoomed_map(m, 64, 128)
    assert got.shape == (64, 128) and np.array_equal(got, zoom(m, zoom=(64 / 3, 128 / 7), order=1))
