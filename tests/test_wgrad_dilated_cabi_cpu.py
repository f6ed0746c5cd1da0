"""`ufr_igemm_wgrad_dilated` (csrc/igemm_wgrad.hip): the weight gradient's entry with a dilation beside the unchanged descriptor.
It validates before any HIP call: every refusal is UFR_EINVAL (-1) with a message through `ufr_last_error()`.  No GPU is needed
and the pointers are never dereferenced."""
import ctypes

import pytest

from understanding_flow_robustness_amd import _lib as L

P = 4096                                  # a non-null address that nothing reads


def desc(**over):
    """dc_conv4 of PWC-Net, Conv2d(128, 96, 3, 1, 8, 8), on a 1 x 16 x 32 grid, operands at chunk offsets inside wider buffers."""
    d = L.IgemmWgradDesc()
    B, H, W = 1, 16, 32
    d.x, d.x_plane_stride, d.in_chunk0, d.C = P, 6 * B * H * W * 32, 1, 128
    d.gy, d.gy_plane_stride, d.g_chunk0, d.N = P, 6 * B * H * W * 32, 2, 96
    d.B, d.Hi, d.Wi, d.Ho, d.Wo = B, H, W, H, W
    d.kh, d.kw, d.sy, d.sx, d.py, d.px = 3, 3, 1, 1, 8, 8
    d.dw, d.db, d.accumulate = P, None, 0
    d.splitm, d.ws, d.ws_elems = 3, P, 3 * 96 * 128 * 9
    d.products = 6
    for k, v in over.items():
        setattr(d, k, v)
    return d


def refused(d, dy, dx):
    lib = L.lib()
    rc = lib.ufr_igemm_wgrad_dilated(ctypes.byref(d), dy, dx, None)
    return rc, lib.ufr_last_error().decode()


def test_the_symbol_is_exported_and_the_abi_version_stays():
    lib = L.lib()
    assert hasattr(lib, "ufr_igemm_wgrad_dilated") and lib.ufr_abi_version() == 9
    assert "ufr_igemm_wgrad_dilated" in L.SIGNATURES and "ufr_igemm_wgrad" in L.SIGNATURES
    rc = lib.ufr_igemm_wgrad_dilated(None, 1, 1, None)
    assert rc == -1 and b"null descriptor" in lib.ufr_last_error()


def test_the_header_declares_the_entry_and_keeps_the_descriptor():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ufr_hip.h")).read()
    assert "int ufr_igemm_wgrad_dilated(const ufr_igemm_wgrad_desc* d, int dy, int dx, ufr_stream_t stream);" in header
    assert "ky*dy - py" in header and "kx*dx - px" in header                  # the formula sits beside the declaration
    assert "#define UFR_ABI_VERSION 9" in header


@pytest.mark.parametrize("dy,dx", [(0, 1), (1, -1), (0, 0), (-3, 8), (8, 0)])
def test_a_dilation_below_one_is_refused(dy, dx):
    rc, msg = refused(desc(), dy, dx)
    assert rc == -1 and "dilation" in msg and f"{dy} x {dx}" in msg, msg
    with pytest.raises(RuntimeError, match="dilation"):
        L.check(rc, "probe")


def test_a_geometry_that_overflows_only_because_of_the_dilation():
    """(Ho-1)*sy + (kh-1)*dy + 1 must stay below 2^30: with dilation 1 this descriptor passes the geometry check (and stops at the
    null dw); with dilation 2^29 the last tap row is 15 + 2^30 + 1."""
    big = 1 << 29
    rc, msg = refused(desc(dw=None), 1, 1)
    assert rc == -1 and "null pointer" in msg and "geometry" not in msg, msg
    rc, msg = refused(desc(), big, 1)
    assert rc == -1 and "bad geometry" in msg, msg
    rc, msg = refused(desc(), 1, big)
    assert rc == -1 and "bad geometry" in msg, msg
    rc, msg = refused(desc(kh=1, kw=1, py=0, px=0, dw=None), big, big)       # one tap: the dilation multiplies nothing
    assert rc == -1 and "null pointer" in msg, msg
    # the same descriptor through the plain entry is dilation 1: it reaches the pointer check, not the geometry check
    lib = L.lib()
    rc = lib.ufr_igemm_wgrad(ctypes.byref(desc(dw=None)), None)
    assert rc == -1 and b"null pointer" in lib.ufr_last_error()


def test_a_null_dw_is_refused_for_the_pointer():
    rc, msg = refused(desc(dw=None), 8, 8)
    assert rc == -1 and "null pointer" in msg, msg
    assert not any(w in msg for w in ("chunks", "taps", "products", "workspace holds", "grid", "dilation", "geometry"))
    rc, msg = refused(desc(dw=None, splitm=1, ws=None, ws_elems=0), 16, 16)
    assert rc == -1 and "null pointer" in msg and "workspace" not in msg


def test_the_other_refusals_are_those_of_the_plain_entry():
    rc, msg = refused(desc(products=3), 8, 8)
    assert rc == -1 and "products must be 6" in msg, msg
    rc, msg = refused(desc(in_chunk0=3), 8, 8)
    assert rc == -1 and "chunks [3, 7) leave the x planes operand (6 chunks per plane)" in msg, msg
    rc, msg = refused(desc(ws_elems=3 * 96 * 128 * 9 - 1), 8, 8)
    assert rc == -1 and "3 slabs of" in msg, msg
