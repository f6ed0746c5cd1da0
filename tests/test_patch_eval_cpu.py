"""CPU suite of the patch evaluation (patch_eval.py, csrc/patch_eval.hip, utils_patch.py): the hand-crafted patches and the two-frame
placement against arrays the reference's own functions produced (tests/golden/make_golden_patch_eval.py), the two C entries' refusals
before any launch (no pointer is dereferenced), and the argument handling of the public function."""
import ctypes
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from understanding_flow_robustness_amd import _lib as L
from understanding_flow_robustness_amd import utils_patch as up

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SERVED = ("hstripes", "vstripes", "vstripes_greenWhite", "vstripes_redBlack", "vstripes_redBlue", "vstripes_greenViolett",
          "vstripes_violettOrange", "vstripes_strip3", "vstripes_rot30", "vstripes_Bcol0.3", "vstripes_Bcol0.3_col0.8",
          "vstripes_col0.6", "checkered", "sin", "gaussian", "uniform", "black", "white", "red", "gray")
RANDOM = ("gaussian", "uniform", "black", "white", "red", "gray")


@pytest.fixture(scope="module")
def patterns():
    return np.load(os.path.join(GOLDEN, "patch_eval_patterns.npz"))


@pytest.fixture(scope="module")
def transform():
    return np.load(os.path.join(GOLDEN, "patch_eval_transform.npz"))


# ------------------------------------------------------------------------------------------------------------------ 1. patterns
@pytest.mark.parametrize("size", [51, 102])
@pytest.mark.parametrize("name", SERVED)
def test_pattern_equals_the_reference(patterns, name, size):
    assert list(patterns["names"]) == list(SERVED)
    key = name.replace(".", "p")
    np.random.seed(int(patterns["seed"]))
    got = (up.create_random_patch if name in RANDOM else up.create_correlated_patch)(name, size)
    want = patterns[f"{key}_{size}"]
    assert got.shape == (1, 3, size, size) and got.dtype == np.float64
    assert np.array_equal(got, want)
    assert float(np.ptp(want)) > 0 or name in ("black", "white", "gray")
    if name in ("sin", "gaussian", "uniform"):              # the same numbers were drawn from np.random
        assert np.random.random() == float(patterns[f"{key}_{size}_next"])


def test_pattern_list_and_refusals(patterns):
    assert up.get_self_correlated_patches() == list(patterns["listed"])
    with pytest.raises(ValueError):                          # 25 // 48 == 0: range(0, 25, 0)
        up.create_correlated_patch("checkered", 25)
    with pytest.raises(ValueError):                          # 23 // 24 == 0
        up.create_correlated_patch("sin", 23)
    with pytest.raises(NotImplementedError, match="cv2"):
        up.create_correlated_patch("circle", 51)
    with pytest.raises(Exception, match="Self correlation type is not implemented"):
        up.create_correlated_patch("dots", 51)
    with pytest.raises(UnboundLocalError):
        up.create_random_patch("blue", 51)


def test_get_patch_and_mask(tmp_path):
    args = Namespace(self_correlated_patch="vstripes", random_patch="", patch_size=21, patch_type="circle", mask_path="")
    patch, shape, mask = up.get_patch_and_mask(args)
    assert shape == (1, 3, 21, 21) and np.array_equal(patch, up.create_correlated_patch("vstripes", 21))
    disc = up.createCircularMask(21, 21).astype("float32")
    assert mask.dtype == np.float32 and np.array_equal(mask, np.array([[disc, disc, disc]]))
    args = Namespace(self_correlated_patch="", random_patch="gray", patch_size=9, patch_type="square", mask_path="")
    patch, shape, mask = up.get_patch_and_mask(args)
    assert np.array_equal(patch, np.full((1, 3, 9, 9), 0.5)) and np.array_equal(mask, np.ones((1, 3, 9, 9)))
    from understanding_flow_robustness_amd.kitti_io import save_patch
    stored = np.random.RandomState(3).rand(1, 3, 7, 7)
    save_patch(stored, tmp_path / "patch.pt")
    args = Namespace(self_correlated_patch="", random_patch="", patch_path=str(tmp_path / "patch.pt"), patch_type="square", mask_path="")
    patch, shape, mask = up.get_patch_and_mask(args)
    assert np.array_equal(patch, stored) and shape == (1, 3, 7, 7)
    args.mask_path = "mask.png"
    with pytest.raises(NotImplementedError, match="mask_path"):
        up.get_patch_and_mask(args)


# ------------------------------------------------------------------------------------------------------------------ 2. transform
DATA_SHAPE, S = (1, 3, 96, 160), 21


def _operands(transform):
    patch = np.random.RandomState(int(transform["patch_seed"])).rand(1, 3, S, S) * 1.2 - 0.1
    disc = up.createCircularMask(S, S).astype("float32")
    return patch, np.array([[disc, disc, disc]])


def test_circle_transform_different_equals_the_reference(transform):
    patch, mask = _operands(transform)
    cases = transform["cases"]
    assert len(cases) >= 6 and {int(c[1]) for c in cases} == {0, 1} and {bool(c[2] < 0) for c in cases} == {False, True}
    three_sizes = clipped = False
    for i, (seed, norotate, fx, fy) in enumerate(cases):
        np.random.seed(int(seed))
        p0, m0 = patch.copy(), mask.copy()
        x, xm, flow, xp, rx, ry, shape = up.circle_transform_different(p0, m0, patch.copy(), DATA_SHAPE, patch.shape, 0,
                                                                       norotate=bool(norotate), fixed_loc=(int(fx), int(fy)))
        assert np.random.random() == float(transform[f"c{i}_next"]), f"case {i}: another number of draws"
        assert np.array_equal(p0, patch) and np.array_equal(m0, mask)                     # the caller's arrays are not written
        for got, name in ((x[0], "x_tgt"), (x[1], "x_ref"), (xm[0], "xm_tgt"), (xm[1], "xm_ref"), (flow, "flow"), (xp[0], "xp_tgt"),
                          (xp[1], "xp_ref")):
            want = transform[f"c{i}_{name}"]
            assert got.shape == DATA_SHAPE and got.dtype == np.float64
            assert np.array_equal(got, want), f"case {i}: {name} differs by {np.abs(got - want).max():.3e}"
        assert [int(v) for v in rx] == transform[f"c{i}_rx"].tolist() and [int(v) for v in ry] == transform[f"c{i}_ry"].tolist()
        assert tuple(shape) == tuple(transform[f"c{i}_shape"].tolist()) == (1, 3, S, S)
        assert np.array_equal(flow[0, 2], xm[0][0, 2])                                    # channel 2 of the flow is the mask
        # what the case exercises, from the numbers the maker replayed: the canvases agree with them
        h_tgt, h_ref = (int(v) for v in transform[f"c{i}_sizes"])
        raw_u, raw_v = (int(v) for v in transform[f"c{i}_raw"])
        for canvas, size, ox, oy in ((xm[0], h_tgt, rx[0], ry[0]), (xm[1], h_ref, rx[1], ry[1])):
            rows, cols = np.nonzero(canvas[0, 0].sum(1))[0], np.nonzero(canvas[0, 0].sum(0))[0]
            assert oy <= rows.min() and rows.max() < oy + size and ox <= cols.min() and cols.max() < ox + size
        three_sizes |= len({h_tgt, h_ref, S}) == 3
        moved = (rx[1] != rx[0] + raw_u) or (ry[1] != ry[0] + raw_v)
        if moved:                                                                         # clipped INTO the frame, and onto its edge
            assert 0 <= rx[1] and rx[1] + h_ref <= DATA_SHAPE[-1] and 0 <= ry[1] and ry[1] + h_ref <= DATA_SHAPE[-2]
            assert rx[1] in (0, DATA_SHAPE[-1] - h_ref) or ry[1] in (0, DATA_SHAPE[-2] - h_ref)
        clipped |= moved
        if not norotate:                                                                  # the rotation's flow is not a constant
            inside = xm[0][0, 0] > 0
            assert float(np.ptp(flow[0, 0][inside])) > 1.0
    assert three_sizes, "no case whose two zoomed sizes differ from each other and from 21"
    assert clipped, "no case whose translation had to be clipped"


def test_moving_is_refused_like_the_broken_reference(transform):
    patch, mask = _operands(transform)
    with pytest.raises(NotImplementedError, match="unbound"):
        up.circle_transform_different(patch, mask, patch.copy(), DATA_SHAPE, patch.shape, moving=True)
    from understanding_flow_robustness_amd.patch_transform import circle_transform_different_device
    with pytest.raises(NotImplementedError, match="unbound"):
        circle_transform_different_device(torch.from_numpy(patch), torch.from_numpy(mask), torch.from_numpy(patch), DATA_SHAPE,
                                          patch.shape, moving=True)
    with pytest.raises(NotImplementedError, match="batch 1"):
        up.circle_transform_different(patch, mask, patch.copy(), (2, 3, 96, 160), patch.shape)


# ------------------------------------------------------------------------------------------------------------------ 3. C ABI
def _eval_entries():
    """(name, message prefix, accepted argument list, [(index, bad value), ...]); the pointers are never dereferenced."""
    p = ctypes.c_void_p(4096)
    K, H, W, sh, sw = 2, 64, 96, 12, 12
    host = np.array([[0, 0, 11, 11, 52, 84, 12, 12], [53, 85, 11, 11, 0, 0, 10, 12]], dtype=np.int32)

    def changed(row, col, value):
        a = host.copy()
        a[row, col] = value
        return a

    keep = [host, changed(1, 0, 54), changed(1, 1, 86), changed(0, 0, -1), changed(0, 2, 13), changed(0, 3, 0), changed(1, 4, 55),
            changed(1, 7, 13), changed(0, 5, 85)]
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)
    paste = [p, p, p, p, p, p, p, hp(host), p, p, K, H, W, sh, sw, 0.0, 1.0, None]
    paste_bad = [(i, None) for i in (0, 1, 2, 3, 6, 7, 8, 9)] + [(4, None), (5, None),    # a second-frame patch without its mask
                 (10, 0), (10, -1), (11, 0), (12, 0), (13, 0), (14, 0), (13, H + 1), (14, W + 1),     # a slot larger than the frame
                 (15, 2.0)] + [(7, hp(a)) for a in keep[1:]]            # origins outside the frame, records larger than the slot
    single = [p, p, p, p, None, None, p, hp(keep[6]), p, p, K, H, W, sh, sw, 0.0, 1.0, None]   # the second record is not read
    single_bad = [(7, hp(keep[1])), (7, hp(keep[4])), (10, 0)]
    need = L.lib().ufr_eval_metrics_workspace_doubles(K)
    metrics = [p, p, p, p, p, p, p, hp(host), K, H, W, 60, 90, sh, sw, 0, p, need, p, 0, K, None]
    metrics_bad = [(i, None) for i in (0, 1, 2, 3, 6, 7, 16, 18)] + [(8, 0), (8, -3), (9, 0), (10, 0), (11, 0), (12, 0), (13, 0), (14, 0),
                   (13, H + 1), (14, W + 1), (15, 2), (15, -1), (17, need - 1), (19, -1), (19, 1), (20, K - 1)] + \
                  [(7, hp(a)) for a in keep[1:]]
    plain = [p, p, p, p, None, None, p, hp(keep[6]), K, H, W, 60, 100, sh, sw, 1, p, need, p, 0, K, None]
    plain_bad = [(0, None), (8, 0), (7, hp(keep[2])), (15, 3), (20, 1)]
    return keep, [("ufr_eval_paste", b"eval paste", paste, paste_bad), ("ufr_eval_paste", b"eval paste", single, single_bad),
                  ("ufr_eval_metrics", b"eval metrics", metrics, metrics_bad),
                  ("ufr_eval_metrics", b"eval metrics", plain, plain_bad)]


def test_symbols_and_abi_version():
    lib = L.lib()
    for name in ("ufr_eval_paste", "ufr_eval_metrics"):
        assert name in L.SIGNATURES and getattr(lib, name) is not None
    assert "ufr_eval_metrics_workspace_doubles" in L.PLAIN
    assert lib.ufr_abi_version() == 9 == L.ABI_VERSION
    assert "patch_eval" in dict(ln.split() for ln in lib.ufr_build_manifest().decode().splitlines() if ln.strip())
    assert lib.ufr_eval_metrics_workspace_doubles(0) == -1 and lib.ufr_eval_metrics_workspace_doubles(-2) == -1
    assert lib.ufr_eval_metrics_workspace_doubles(3) > 0


def test_eval_entries_refuse_bad_arguments_before_any_launch():
    """ufr_eval_paste (two records and one) and ufr_eval_metrics (with flow slot and second mask, and without), one bad argument at a
    time: null pointers, K <= 0, empty sizes, a slot larger than the frame, an origin outside the frame, a record larger than its
    slot, lo > hi, an ignore flag of 2, a result row outside the buffer, a short workspace.  Each is refused with -1 and the
    entry's own message."""
    lib = L.lib()
    keep, entries = _eval_entries()
    for name, message, good, bad in entries:
        assert len(good) == len(L.SIGNATURES[name])
        for index, value in bad:
            args = list(good)
            args[index] = value
            lib.ufr_corr_forward(None, None, None, 0, 1, 1, 4, 4, None, None)          # another message in the channel first
            rc = getattr(lib, name)(*args)
            assert rc == -1, f"{name}: argument {index} = {value!r} was accepted (rc {rc})"
            assert lib.ufr_last_error().startswith(message + b":"), (name, index, value, lib.ufr_last_error())
    assert keep


# ------------------------------------------------------------------------------------------------------------------ 4. arguments
def _item(calib=()):
    z = torch.zeros(1, 3, 64, 64)
    return (z, z.clone(), z.clone(), z.clone(), torch.full((1, 64, 64), 7.0), list(calib), [])


def test_evaluate_patch_refuses_what_needs_the_3d_projection_and_what_is_not_on_a_device():
    from understanding_flow_robustness_amd.patch_eval import evaluate_patch
    patch, mask = np.zeros((1, 3, 9, 9)), np.ones((1, 3, 9, 9))
    args = Namespace(flownet="FlowNetC", norotate=True)
    with pytest.raises(NotImplementedError, match="project_patch_3d_scene"):
        evaluate_patch(None, [_item()], patch, mask, patch.shape, Namespace(flownet="FlowNetC", true_motion=True))
    with pytest.raises(NotImplementedError, match="project_patch_3d_scene"):
        evaluate_patch(None, [_item(calib=[torch.eye(3)])], patch, mask, patch.shape, args)
    with pytest.raises(RuntimeError, match="HIP device tensor"):        # calibration is no obstacle with different_pos; no CPU path
        evaluate_patch(None, [_item(calib=[torch.eye(3)])], patch, mask, patch.shape,
                       Namespace(flownet="FlowNetC", norotate=True, different_pos=True))
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        evaluate_patch(None, [_item()[:4]], patch, mask, patch.shape, args)
    with pytest.raises(ValueError, match="chunk"):
        evaluate_patch(None, [_item()], patch, mask, patch.shape, args, chunk=0)
    with pytest.raises(ValueError, match=r"\[1,3,S,S\]"):
        evaluate_patch(None, [_item()], patch, mask[:, :2], patch.shape, args)
    empty = evaluate_patch(None, [], patch, mask, patch.shape, args)
    assert empty.per_item.shape == (0, 4) and empty.locations == [] and empty.error_names == ["epe", "adv_epe", "cos_sim", "adv_cos_sim"]
