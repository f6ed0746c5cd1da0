"""`ufr_igemm_tail_plan` / `ufr_igemm_balanced` (csrc/igemm.hip) through ctypes, without a device: the plan that re-cuts the
under-filled last round of a ping-pong launch over K is host arithmetic.

The rule (include/ufr_hip.h): Mt row tiles of 256, Nt = Npad / 128 column tiles, T = Mt * Nt, q = T // R.  The first
q * R // Nt row tiles stay whole; the remaining row tiles become S = min(R // tail_tiles, ktiles // 8, 8) slices of
ceil(ktiles / S) K tiles.  `ktiles // 8` bounds the NOMINAL slice ceil(ktiles / S) from below by 8; the last slice holds
what is left (25 K tiles in 3 slices: 9, 9, 7) and is never empty.  The plan is off when a launch has no full round, no
under-filled round, fewer than two slices, any of the refused descriptor settings, or when the predicted K steps
(rounds x (K tiles + 6), + 10 for the reduce launch) do not go down."""
import ctypes as C
import itertools

import pytest
import torch

from understanding_flow_robustness_amd import _lib as L
from understanding_flow_robustness_amd import igemm as ig


def _desc(M, Npad, taps, KC, **kw):
    d = L.IgemmDesc()
    d.B, d.Hr, d.Wr = 1, 1, M
    d.KC, d.Npad, d.N, d.nphase = KC, Npad, Npad, 1
    d.phase[0].ntaps = taps
    d.splitk, d.products, d.variant = 1, 6, 6
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _rule(M, Npad, ktiles, R):
    """The plan by the rule, in plain Python: None (off) or (full row tiles, tail row tiles, S, slice length)."""
    Mt, Nt = -(-M // 256), Npad // 128
    T = Mt * Nt
    q = T // R
    if q == 0 or T % R == 0:
        return None
    full = q * R // Nt
    tiles = (Mt - full) * Nt
    S = min(R // tiles, ktiles // 8, 8)
    if S < 2:
        return None
    per = -(-ktiles // S)
    if q * (ktiles + 6) + per + 6 + 10 > -(-T // R) * (ktiles + 6):
        return None
    return full, Mt - full, S, per


def test_the_headline_geometry():
    """conv3_1's data gradient on the correlation-reach band, 8 pairs of 384 x 1280: 84 x 4 tiles on 256 CUs."""
    p = ig.tail_plan(_desc(21504, 512, 9, 8), 256)
    assert p.on == 1 and (p.row_tiles, p.col_tiles) == (84, 4)
    assert (p.full_row_tiles, p.tail_row_tiles, p.slices, p.slice_ktiles, p.ktiles) == (64, 20, 3, 24, 72)
    assert (p.tail_row0, p.tail_rows, p.workgroups, p.ws_floats) == (16384, 5120, 256 + 80 * 3, 3 * 5120 * 512)
    assert (p.steps_before, p.steps_after) == (2 * 78, 78 + 30 + 10)
    p0 = ig.tail_plan(_desc(21504, 512, 9, 8), 0)                    # 0 = the MI355X's 256 CUs (no device is asked)
    assert bytes(p0) == bytes(p)


def test_sweep_invariants():
    Ms = (1, 255, 256, 257, 1920, 2400, 4096, 5000, 21504, 21505, 61440, 65537, 131072)
    Ns = (128, 256, 512, 1024)
    Ks = ((1, 1), (1, 8), (9, 1), (9, 2), (9, 3), (9, 5), (9, 8), (25, 1), (25, 4), (1, 16), (1, 17))
    Rs = (1, 3, 8, 12, 16, 17, 64, 255, 256, 304)
    seen_on = 0
    for M, Npad, (taps, KC), R in itertools.product(Ms, Ns, Ks, Rs):
        p, want = ig.tail_plan(_desc(M, Npad, taps, KC), R), _rule(M, Npad, taps * KC, R)
        Mt, Nt, kt = -(-M // 256), Npad // 128, taps * KC
        assert bool(p.on) == (want is not None), (M, Npad, kt, R)
        assert p.full_row_tiles + p.tail_row_tiles == Mt == p.row_tiles                       # full + tail = T (in row tiles of Nt tiles)
        if not p.on:
            assert (p.tail_row_tiles, p.slices, p.ws_floats) == (0, 0, 0)
            continue
        seen_on += 1
        assert (p.full_row_tiles, p.tail_row_tiles, p.slices, p.slice_ktiles) == want
        assert p.tail_row0 == p.full_row_tiles * 256 and p.tail_row0 + p.tail_rows == M        # the tail is the LAST rows
        assert p.full_row_tiles * Nt <= (Mt * Nt // R) * R < (p.full_row_tiles + 1) * Nt        # whole rounds only, as many row tiles as fit
        assert 2 <= p.slices <= 8 and p.slices * p.tail_row_tiles * Nt <= R                     # the slices fill the chip at most once
        assert p.slice_ktiles >= 8 and 0 < kt - (p.slices - 1) * p.slice_ktiles <= p.slice_ktiles   # nominal slice >= 8, last one not empty
        assert p.ws_floats == p.slices * p.tail_rows * Npad
        assert p.workgroups == p.full_row_tiles * Nt + p.tail_row_tiles * Nt * p.slices
        assert p.steps_after <= p.steps_before
    assert seen_on > 100


@pytest.mark.parametrize("what, edit", [
    ("two phases", dict(nphase=2)), ("64-column tiles", dict(Npad=448, N=448)), ("tap-reuse form", dict(variant=7)),
    ("default form", dict(variant=0)), ("three products", dict(products=3)), ("one product", dict(products=1)),
    ("tickets", dict(tickets=4096)), ("no_reduce", dict(no_reduce=1)), ("tail output", dict(tail=4096, tail_n0=32)),
    ("split-K", dict(splitk=2)), ("no full round", dict(Wr=256 * 60)), ("whole rounds", dict(Wr=256 * 128)),
    ("short reduction", dict(KC=1)),
])
def test_refused_configurations_are_off(what, edit):
    d = _desc(21504, 512, 9, 8)
    assert ig.tail_plan(d, 256).on == 1
    for k, v in edit.items():
        setattr(d, k, v)
    p = ig.tail_plan(d, 256)
    assert p.on == 0 and p.ws_floats == 0 and p.tail_row_tiles == 0, what


def test_a_plan_that_does_not_pay_for_its_reduce_launch_is_off():
    """3 x 3 over 64 channels (18 K tiles), 8 x 2 tiles on 12 workgroups: two slices of 9 leave 24 + 15 + 10 = 49 steps against
    2 x 24 = 48 -- off; over 96 channels (27 K tiles) three slices of 9 leave 33 + 15 + 10 = 58 against 66 -- on."""
    p = ig.tail_plan(_desc(1920, 256, 9, 2), 12)
    assert p.on == 0 and p.steps_before == 48
    p = ig.tail_plan(_desc(1920, 256, 9, 3), 12)
    assert p.on == 1 and (p.full_row_tiles, p.tail_row_tiles, p.slices, p.slice_ktiles) == (6, 2, 3, 9)
    assert (p.steps_before, p.steps_after) == (66, 58)


def test_bad_arguments_are_refused():
    lib = L.lib()
    p = L.IgemmTailPlan()
    d = _desc(21504, 512, 9, 8)
    assert lib.ufr_igemm_tail_plan(None, 256, C.byref(p)) == -1
    assert lib.ufr_igemm_tail_plan(C.byref(d), 256, None) == -1
    assert lib.ufr_igemm_tail_plan(C.byref(d), -1, C.byref(p)) == -1
    big = _desc(4, 512, 9, 8, B=1 << 15, Hr=1 << 15)
    assert lib.ufr_igemm_tail_plan(C.byref(big), 256, C.byref(p)) == -1 and b"pixels" in lib.ufr_last_error()


def test_balanced_entry_runs_up_to_the_launch_without_a_device():
    """`ufr_igemm_balanced` on real descriptors that point at host memory, with plans that are on and off: it must get as far as
    asking for the device and fail THERE (UFR_ELAUNCH), never earlier and never by touching an operand; a workspace that is too
    small is refused (UFR_EINVAL) in front of that."""
    lib = L.lib()
    if lib.ufr_device_count() > 0:
        pytest.skip("a HIP device is present: these descriptors point at host memory and must not be launched")
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, 24, 40
    x = ig.Planes(B, H, W, 3, "cpu")                                             # 96 channels
    w3 = torch.randn(256, 96, 3, 3, generator=g)
    wi, wb = ig.conv_forward_weights(w3, 1, 1), ig.conv_backward_weights(torch.randn(96, 256, 3, 3, generator=g), 1, 1)
    out, gx = ig.Planes(B, H, W, 8, "cpu"), ig.GradSum(B, H, W, 8, "cpu")
    bias = torch.zeros(wi.Npad)
    on = ig.make_launch(wi, x, 0, (H, W), (H, W), out_planes=out, bias=bias, variant=6, balance=True, resident=12)
    assert on.tail_plan is not None and (on.tail_plan.full_row_tiles, on.tail_plan.tail_row_tiles, on.tail_plan.slices) == (6, 2, 3)
    ws = on._tail_ws
    assert ws.numel() == on.tail_plan.ws_floats == 3 * (B * H * W - 6 * 256) * 256
    off = ig.make_launch(wi, x, 0, (H, W), (H, W), out_planes=out, bias=bias, variant=6, balance=True, resident=8)
    assert off.tail_plan is None                                                  # 16 tiles on 8 workgroups: whole rounds
    grad = ig.make_launch(wb, x, 0, (H, W), (H, W), out_planes=out, out_f32=gx, mask=out, planes_chunks=1, f32_first_chunk=1,
                          variant=6, balance=True, resident=12)
    assert grad.tail_plan is not None
    for launch, R in ((on, 12), (on, 0), (off, 8), (off, 0), (grad, 12)):
        rc = lib.ufr_igemm_balanced(C.byref(launch.desc), R, L.ptr(ws), ws.numel(), None)
        assert rc == -3, (rc, lib.ufr_last_error())
        assert b"no current device" in lib.ufr_last_error()
    # in front of the device: a plan that is on needs room for its slabs
    assert lib.ufr_igemm_balanced(C.byref(on.desc), 12, L.ptr(ws), ws.numel() - 1, None) == -1 and b"workspace" in lib.ufr_last_error()
    assert lib.ufr_igemm_balanced(C.byref(on.desc), 12, None, ws.numel(), None) == -1 and b"workspace" in lib.ufr_last_error()
    # ... and a plan that is off needs none
    assert lib.ufr_igemm_balanced(C.byref(off.desc), 8, None, 0, None) == -3
