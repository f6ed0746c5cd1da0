"""CPU suite: the form-selection rule of predict_flow's split form (csrc/engine_small.hip `ufr_flow_head_split_plan`), the size of
its partials buffer, and what the split entries refuse before any launch.  Validation precedes every HIP call, the pointers are
never dereferenced: no GPU."""
import ctypes

import pytest


def _plan(B, H, W, chunks):
    from understanding_flow_robustness_amd.flownetc_engine import pf_split_plan
    return pf_split_plan(B, H, W, chunks)


def _ceil(a, b):
    return -(-a // b)


def _want(B, H, W, chunks):
    """The launcher's rule, restated: tile rows 8 / 4 / 2 by workgroup count, two chunk slices below 512 workgroups (one below four
    chunks), eight one-wave slices on the small grids; starved = fewer than 256 four-row tiles."""
    blocks_of = lambda th: B * _ceil(H, th) * _ceil(W, 32)
    th = 8 if blocks_of(8) >= 512 else 4 if blocks_of(4) >= 256 else 2
    blocks = blocks_of(th)
    s = 1 if blocks >= 512 or chunks < 4 else 2
    mt = _ceil((th + 2) * 34, 16)
    if mt <= 12 and s == 2 and chunks >= 16 and blocks <= 256:
        s = 8
    return s, blocks_of(4) < 256


def test_plan_over_the_grids_of_every_level():
    sizes = [(1, 1), (1, 5), (2, 3), (5, 7), (6, 20), (7, 9), (12, 40), (13, 33), (16, 96), (24, 48), (24, 80), (31, 33), (32, 32),
             (33, 31), (48, 96), (48, 160), (64, 64), (96, 320)]
    for B in (1, 2, 8, 16):
        for H, W in sizes:
            for chunks in (1, 3, 4, 7, 13, 15, 16, 25, 33, 48):
                slices, starved, floats = _plan(B, H, W, chunks)
                assert (slices, starved) == _want(B, H, W, chunks), (B, H, W, chunks)
                assert floats == slices * B * H * W * 18
    # the headline's frame, 8 pairs at 384 x 1280: levels 6, 5 and 4 are starved, 3 and 2 are not
    got = {k: _plan(8, 384 >> k, 1280 >> k, c) for k, c in ((6, 32), (5, 33), (4, 25), (3, 13), (2, 7))}
    assert [got[k][1] for k in (6, 5, 4, 3, 2)] == [True, True, True, False, False]
    assert [got[k][0] for k in (6, 5, 4)] == [8, 8, 2]
    assert max(got[k][2] for k in (6, 5, 4)) * 4 <= 3 << 20           # the engine's one partials buffer: under 3 MB


def test_plan_and_split_entries_refuse_bad_arguments_before_any_launch():
    from understanding_flow_robustness_amd import _lib as L
    lib = L.lib()
    s, t, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
    for bad in ((0, 6, 20, 32), (8, 0, 20, 32), (8, 6, 0, 32), (8, 6, 20, 0), (8, 6, 20, 49)):
        assert lib.ufr_flow_head_split_plan(*bad, ctypes.byref(s), ctypes.byref(t), ctypes.byref(n)) == -1
    assert lib.ufr_flow_head_split_plan(8, 6, 20, 32, None, ctypes.byref(t), ctypes.byref(n)) == -1
    p = ctypes.c_void_p(4096)
    B, H, W, chunks = 8, 6, 20, 32
    stride = chunks * B * H * W * 32
    slices, _, floats = _plan(B, H, W, chunks)
    assert slices == 8
    for asked in (1, 2, 4, 16):                      # another slicing adds other partial sums: refused, with the count that holds
        assert lib.ufr_flow_head_planes_forward_split(p, stride, 0, chunks, p, chunks, p, floats, asked, B, H, W, None) == -1
        assert b"the unsplit form of this grid adds 8" in lib.ufr_last_error()
    assert lib.ufr_flow_head_planes_forward_split(p, stride, 0, chunks, p, chunks, p, floats - 1, slices, B, H, W, None) == -1
    assert b"partials buffer" in lib.ufr_last_error()
    assert lib.ufr_flow_head_planes_forward_split(p, stride, 0, chunks + 1, p, chunks + 1, p, floats, slices, B, H, W, None) == -1
    assert lib.ufr_flow_head_planes_forward_split(p, stride, 0, chunks, p, chunks - 1, p, floats, slices, B, H, W, None) == -1
    assert lib.ufr_flow_head_planes_forward_split(None, stride, 0, chunks, p, chunks, p, floats, slices, B, H, W, None) == -1
    assert lib.ufr_flow_head_split_finish(p, floats - 1, slices, p, p, None, None, None, 0, 0, B, H, W, None) == -1
    assert lib.ufr_flow_head_split_finish(p, floats, 0, p, p, None, None, None, 0, 0, B, H, W, None) == -1
    assert lib.ufr_flow_head_split_finish(p, floats, slices, None, p, None, None, None, 0, 0, B, H, W, None) == -1
    assert lib.ufr_flow_head_split_finish(p, floats, slices, p, p, None, None, p, 4 * stride, 0, B, H, W, None) == -1     # no weights
    fine = B * 2 * H * 2 * W * 32
    assert lib.ufr_flow_head_split_finish(p, floats, slices, p, p, p, None, p, 3 * fine, 3, B, H, W, None) == -1          # chunk 3 of 3
    assert b"leaves the planes operand" in lib.ufr_last_error()
