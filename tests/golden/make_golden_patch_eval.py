"""Golden fixtures of the patch evaluation (patch_attacks/test_patch.py), produced by running the REFERENCE's own functions of
patch_attacks/utils_patch.py on the CPU; see make_golden.py for the contract.

    python tests/golden/make_golden_patch_eval.py [patterns] [transform]

patterns   `create_correlated_patch` / `create_random_patch` for every name this project serves, at sizes 51 and 102, and for the
           names that draw from `np.random` the next `np.random.random()` after the call (seed PATTERN_SEED before each call).
transform  `circle_transform_different` on a (1,3,96,160) canvas with a 21 x 21 patch, for CASES = (seed, norotate, fixed_loc): all
           seven outputs, the `np.random.random()` that follows, and -- replayed here from the same seed in the function's
           documented draw order -- the zoom factors, the zoomed sizes and the translations BEFORE the function clipped them, so
           that a test can assert that a case with three different sizes and a case with a clipped translation are among them.
"""
from __future__ import annotations

import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402

import ref_harness as rh  # noqa: E402
from make_golden import save  # noqa: E402

PATTERN_SEED = 11
SIZES = (51, 102)
CORRELATED = ("hstripes", "vstripes", "vstripes_greenWhite", "vstripes_redBlack", "vstripes_redBlue", "vstripes_greenViolett",
              "vstripes_violettOrange", "vstripes_strip3", "vstripes_rot30", "vstripes_Bcol0.3", "vstripes_Bcol0.3_col0.8",
              "vstripes_col0.6", "checkered", "sin")
RANDOM = ("gaussian", "uniform", "black", "white", "red", "gray")
DRAWING = ("sin", "gaussian", "uniform")

DATA_SHAPE, S, PATCH_SEED = (1, 3, 96, 160), 21, 5
# (seed, norotate, fixed_loc); seeds 601 / 719 draw the zoomed sizes 20 and 22 (searched: `python make_golden_patch_eval.py search`)
CASES = ((0, False, (-1, -1)), (1, True, (-1, -1)), (2, False, (30, 40)), (3, True, (120, 10)), (601, False, (-1, -1)),
         (719, True, (-1, -1)))


def key(name):
    return name.replace(".", "p")


def patch_and_mask():
    """The 21 x 21 operands of every transform case: values on both sides of [0, 1], the disc of `createCircularMask`."""
    from understanding_flow_robustness_amd.utils_patch import createCircularMask
    patch = np.random.RandomState(PATCH_SEED).rand(1, 3, S, S) * 1.2 - 0.1
    disc = createCircularMask(S, S).astype("float32")
    return patch, np.array([[disc, disc, disc]])


def replay(seed, norotate, fixed_loc):
    """The numbers `circle_transform_different` draws, in its order: (zoom_tgt, zoom_ref, sizes, raw_u, raw_v)."""
    np.random.seed(seed)
    np.random.random()
    f_tgt = 1 + 0.05 * (np.random.random() - 0.5)
    if not norotate:
        np.random.random()
    if fixed_loc[0] < 0 or fixed_loc[1] < 0:
        np.random.choice(DATA_SHAPE[-1] - 2 * S - 2)
        np.random.choice(DATA_SHAPE[-2] - 2 * S - 2)
    np.random.random()
    f_ref = 1 + 0.05 * (np.random.random() - 0.5)
    if not norotate:
        np.random.random()
    raw_u = round(100 * ((np.random.random() - 0.5) / 0.5))
    raw_v = round(100 * ((np.random.random() - 0.5) / 0.5))
    return f_tgt, f_ref, (int(round(S * f_tgt)), int(round(S * f_ref))), raw_u, raw_v


def search():
    for norotate in (False, True):
        for seed in range(5000):
            _, _, (a, b), _, _ = replay(seed, norotate, (-1, -1))
            if a != b and a != S and b != S:
                print(f"norotate={norotate}: seed {seed} draws the sizes {a} and {b}")
                break


def gen_patterns():
    up = rh.ref_module("patch_attacks.utils_patch")
    out = {}
    for size in SIZES:
        for name in CORRELATED + RANDOM:
            np.random.seed(PATTERN_SEED)
            fn = up.create_correlated_patch if name in CORRELATED else up.create_random_patch
            a = fn(name, size)
            assert a.shape == (1, 3, size, size) and a.dtype == np.float64
            out[f"{key(name)}_{size}"] = a
            if name in DRAWING:
                out[f"{key(name)}_{size}_next"] = np.float64(np.random.random())
    assert up.get_self_correlated_patches()[-1] == "circle"
    save("patch_eval_patterns", names=np.array(CORRELATED + RANDOM), listed=np.array(up.get_self_correlated_patches()),
         seed=PATTERN_SEED, **out)


def gen_transform():
    up = rh.ref_module("patch_attacks.utils_patch")
    patch, mask = patch_and_mask()
    out = dict(cases=np.array([(s, int(n), fx, fy) for s, n, (fx, fy) in CASES], dtype=np.int64), patch_seed=PATCH_SEED)
    three_sizes = clipped = False
    for i, (seed, norotate, fixed_loc) in enumerate(CASES):
        np.random.seed(seed)
        x, xm, flow, xp, rx, ry, shape = up.circle_transform_different(patch.copy(), mask.copy(), patch.copy(), DATA_SHAPE, patch.shape,
                                                                       0, norotate=norotate, fixed_loc=fixed_loc)
        nxt = np.random.random()
        f_tgt, f_ref, sizes, raw_u, raw_v = replay(seed, norotate, fixed_loc)
        assert np.random.random() == nxt, "the replay's draw order is not the function's"
        lim = lambda raw, o, size, n: min(max(raw, -o), n - size - o)
        assert rx[1] == rx[0] + lim(raw_u, rx[0], sizes[1], DATA_SHAPE[-1]) and ry[1] == ry[0] + lim(raw_v, ry[0], sizes[1], DATA_SHAPE[-2])
        three_sizes |= len({sizes[0], sizes[1], S}) == 3
        clipped |= rx[1] != rx[0] + raw_u or ry[1] != ry[0] + raw_v
        out.update({f"c{i}_x_tgt": x[0], f"c{i}_x_ref": x[1], f"c{i}_xm_tgt": xm[0], f"c{i}_xm_ref": xm[1], f"c{i}_flow": flow,
                    f"c{i}_xp_tgt": xp[0], f"c{i}_xp_ref": xp[1], f"c{i}_rx": np.array(rx), f"c{i}_ry": np.array(ry),
                    f"c{i}_shape": np.array(shape), f"c{i}_next": np.float64(nxt), f"c{i}_sizes": np.array(sizes),
                    f"c{i}_raw": np.array([raw_u, raw_v]), f"c{i}_zoom": np.array([f_tgt, f_ref])})
        print(f"case {i}: seed {seed} norotate {norotate} fixed {fixed_loc}: x {rx} y {ry} sizes {sizes} raw translation {(raw_u, raw_v)}")
    assert three_sizes and clipped, (three_sizes, clipped)
    save("patch_eval_transform", **out)


GENERATORS = {"patterns": gen_patterns, "transform": gen_transform}

if __name__ == "__main__":
    if sys.argv[1:] == ["search"]:
        search()
        sys.exit(0)
    rh.install()
    for which in sys.argv[1:] or list(GENERATORS):
        print(f"== {which}")
        GENERATORS[which]()
