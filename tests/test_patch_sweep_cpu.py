"""CPU suite of the patch location sweep (patch_sweep.py, csrc/patch_sweep.hip): the grid of test_moving_patch.py:299-306 and :445,
the argument checks of the public function, and the two C entries' refusals before any launch (no pointer is dereferenced)."""
import ctypes
from argparse import Namespace

import numpy as np
import pytest
import torch

from understanding_flow_robustness_amd import _lib as L
from understanding_flow_robustness_amd.patch_sweep import sweep_grid, sweep_patch_locations


@pytest.mark.parametrize("H,W,ph,pw,stride,shape", [(384, 1280, 51, 51, 25, (14, 50)), (128, 256, 19, 19, 32, (4, 8))])
def test_grid_shape_and_visiting_order(H, W, ph, pw, stride, shape):
    ys, xs, locations = sweep_grid(H, W, ph, pw, stride)
    assert (len(ys), len(xs)) == shape == (len(range(0, H - ph, stride)), len(range(0, W - pw, stride)))
    # the reference's loops: x outer, y inner
    expected = []
    for x in range(0, W - pw, stride):
        for y in range(0, H - ph, stride):
            expected.append((y, x))
    assert locations == expected
    assert locations[0] == (0, 0) and locations[1] == (stride, 0) and locations[len(ys)] == (0, stride)
    # every position owns one cell of the map, indexed [y // stride, x // stride]
    cells = {(y // stride, x // stride) for y, x in locations}
    assert len(cells) == len(locations) == shape[0] * shape[1]
    assert max(c[0] for c in cells) == shape[0] - 1 and max(c[1] for c in cells) == shape[1] - 1
    # every placement lies inside the frame
    assert all(y + ph <= H and x + pw <= W for y, x in locations)


def _operands(batch=1, gt_channels=3):
    tgt = torch.zeros(batch, 3, 64, 64)
    gt = torch.zeros(1, gt_channels, 64, 64)
    patch = np.zeros((1, 3, 9, 9))
    return tgt, tgt.clone(), gt, patch, np.ones_like(patch)


def test_public_function_refuses_what_the_reference_loop_does_not_define():
    args = Namespace(flownet="FlowNetC", norotate=True)
    tgt, ref, gt, patch, mask = _operands(batch=2)
    with pytest.raises(ValueError, match="ONE frame pair"):
        sweep_patch_locations(None, tgt, ref, gt, patch, mask, args)
    tgt, ref, gt, patch, mask = _operands(gt_channels=2)
    with pytest.raises(ValueError, match="three channels"):
        sweep_patch_locations(None, tgt, ref, gt, patch, mask, args)
    tgt, ref, gt, patch, mask = _operands()
    with pytest.raises(NotImplementedError, match="norotate"):
        sweep_patch_locations(None, tgt, ref, gt, patch, mask, Namespace(flownet="FlowNetC", norotate=False))
    with pytest.raises(NotImplementedError, match="norotate"):          # the script's default is to rotate
        sweep_patch_locations(None, tgt, ref, gt, patch, mask, Namespace(flownet="FlowNetC"))
    with pytest.raises(RuntimeError, match="HIP device tensor"):        # no CPU path
        sweep_patch_locations(None, tgt, ref, gt, patch, mask, args)


def _sweep_entries():
    """(name, message prefix, accepted argument list, [(index, bad value), ...]); the pointers are never dereferenced."""
    p = ctypes.c_void_p(4096)
    K, H, W, ph, pw = 2, 64, 96, 9, 11
    host = np.array([[0, 0], [H - ph, W - pw]], dtype=np.int32)

    def moved(row, col):
        a = host.copy()
        a[1] = (row, col)
        return a

    keep = [host, moved(H - ph + 1, 0), moved(0, W - pw + 1), moved(-1, 0)]
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)
    chain = L.ConeChain()
    chain.n_layers, chain.n_taps = 1, 1
    chain.kernel[0], chain.stride[0], chain.pad[0] = 3, 2, 1
    bad_chain = L.ConeChain()
    ch, bch = ctypes.pointer(chain), ctypes.pointer(bad_chain)
    paste = [p, p, p, p, p, hp(host), p, p, K, H, W, ph, pw, 0.0, 1.0, None, 0, 0, None, None, None]
    paste_bad = [(i, None) for i in (0, 1, 2, 3, 4, 5, 6, 7)] + [(8, 0), (8, -1), (9, 0), (10, 0), (11, 0), (12, 0),
                 (11, H + 1), (12, W + 1),                              # a patch larger than the frame
                 (5, hp(keep[1])), (5, hp(keep[2])), (5, hp(keep[3])),  # an origin at H - ph + 1, W - pw + 1, -1
                 (13, 2.0),                                             # lo > hi
                 (15, ch), (19, p)]                                     # a chain / window stack without the window table
    window = [p, p, p, p, p, hp(host), None, None, K, H, W, ph, pw, 0.0, 1.0, ch, 32, 32, p, p, None]
    window_bad = [(15, None), (19, None), (15, bch), (16, 0), (16, 33), (17, 31), (16, H + 2), (17, W + 2), (9, 63),
                  (5, hp(keep[1])), (8, 0), (0, None)]
    need = L.lib().ufr_sweep_metrics_workspace_doubles(K)
    metrics = [p, p, p, p, hp(host), K, H, W, 60, 100, ph, pw, 1, p, need, p, 0, K, None]
    metrics_bad = [(i, None) for i in (0, 1, 3, 4, 13, 15)] + [(5, 0), (5, -3), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0), (11, 0),
                   (10, H + 1), (11, W + 1), (4, hp(keep[1])), (4, hp(keep[2])), (12, 2), (12, -1), (14, need - 1), (16, -1), (16, 1),
                   (17, K - 1)]
    clean = [p, p, None, None, None, 1, H, W, 60, 100, 0, 0, 1, p, need, p, 0, 1, None]
    clean_bad = [(0, None), (5, 0), (12, 2), (17, 0)]
    return keep, [("ufr_sweep_paste", b"sweep paste", paste, paste_bad), ("ufr_sweep_paste", b"sweep paste", window, window_bad),
                  ("ufr_sweep_metrics", b"sweep metrics", metrics, metrics_bad),
                  ("ufr_sweep_metrics", b"sweep metrics", clean, clean_bad)]


def test_sweep_entries_refuse_bad_arguments_before_any_launch():
    """ufr_sweep_paste (canvas and window form) and ufr_sweep_metrics (with and without a patch), one bad argument at a time: null
    pointers, K <= 0, empty sizes, a patch larger than the frame, an origin at H - ph + 1, valid_in_patch = 2, a window form
    without a chain, a result row outside the buffer, a short workspace.  Each is refused with -1 and the entry's own message."""
    lib = L.lib()
    keep, entries = _sweep_entries()
    assert lib.ufr_sweep_metrics_workspace_doubles(0) == -1 and lib.ufr_sweep_metrics_workspace_doubles(3) > 0
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
