"""`ufr_igemm_wgrad` (csrc/igemm_wgrad.hip) validates its descriptor before any HIP call: every refusal is UFR_EINVAL (-1) with a
message through `ufr_last_error()`.  No GPU is needed and the pointers are never dereferenced."""
import ctypes

import pytest

from understanding_flow_robustness_amd import _lib as L

P = 4096                                  # a non-null address that nothing reads


def desc(**over):
    """Conv2d(70, 130, 3, 1, 1) on a 2 x 12 x 20 grid, operands at chunk offsets inside wider buffers (5 and 8 chunks per plane)."""
    d = L.IgemmWgradDesc()
    B, H, W = 2, 12, 20
    d.x, d.x_plane_stride, d.in_chunk0, d.C = P, 5 * B * H * W * 32, 1, 70
    d.gy, d.gy_plane_stride, d.g_chunk0, d.N = P, 8 * B * H * W * 32, 2, 130
    d.B, d.Hi, d.Wi, d.Ho, d.Wo = B, H, W, H, W
    d.kh, d.kw, d.sy, d.sx, d.py, d.px = 3, 3, 1, 1, 1, 1
    d.dw, d.db, d.accumulate = P, None, 0
    d.splitm, d.ws, d.ws_elems = 3, P, 3 * 130 * 70 * 9
    d.products = 6
    for k, v in over.items():
        setattr(d, k, v)
    return d


def refused(d):
    lib = L.lib()
    rc = lib.ufr_igemm_wgrad(ctypes.byref(d), None)
    return rc, lib.ufr_last_error().decode()


def test_the_symbol_is_exported_and_the_abi_version_stays():
    lib = L.lib()
    assert hasattr(lib, "ufr_igemm_wgrad") and lib.ufr_abi_version() == 9
    assert "ufr_igemm_wgrad" in L.SIGNATURES
    rc = lib.ufr_igemm_wgrad(None, None)
    assert rc == -1 and b"null descriptor" in lib.ufr_last_error()


@pytest.mark.parametrize("field", ["x", "gy", "dw", "ws"])
def test_null_pointers_are_refused(field):
    rc, msg = refused(desc(**{field: None}))
    assert rc == -1 and "null pointer" in msg, msg
    with pytest.raises(RuntimeError, match="null pointer"):
        L.check(rc, "probe")


def test_a_null_dw_is_refused_for_the_pointer_not_for_the_geometry():
    """The descriptor is well formed in every other field: the refusal names the pointer."""
    rc, msg = refused(desc(dw=None))
    assert rc == -1 and "null pointer" in msg
    assert not any(w in msg for w in ("chunks", "taps", "products", "workspace holds", "grid"))
    # and without a split no workspace is asked for
    rc, msg = refused(desc(dw=None, splitm=1, ws=None, ws_elems=0))
    assert rc == -1 and "null pointer" in msg and "workspace" not in msg


@pytest.mark.parametrize("products", [0, 1, 3, 5, 7])
def test_only_six_products(products):
    rc, msg = refused(desc(products=products))
    assert rc == -1 and "products must be 6" in msg, msg


def test_more_than_49_taps():
    rc, msg = refused(desc(kh=7, kw=8))
    assert rc == -1 and "56 taps" in msg and "at most 49" in msg, msg
    rc, msg = refused(desc(kh=50, kw=1))
    assert rc == -1 and "at most 49" in msg, msg
    rc, msg = refused(desc(kh=7, kw=7, py=3, px=3, dw=None))          # 49 taps pass the tap check (and stop at the null pointer)
    assert rc == -1 and "null pointer" in msg


def test_chunk_ranges_that_leave_an_operand():
    # x: 70 channels = 3 chunks from chunk 1 in a 5-chunk buffer is fine; from chunk 3 it is [3, 6) of 5
    rc, msg = refused(desc(in_chunk0=3))
    assert rc == -1 and "chunks [3, 6) leave the x planes operand (5 chunks per plane)" in msg, msg
    rc, msg = refused(desc(C=161))                                    # 6 chunks from chunk 1
    assert rc == -1 and "chunks [1, 7) leave the x planes operand" in msg, msg
    # gy: 130 channels = 5 chunks from chunk 2 in an 8-chunk buffer is fine; from chunk 4 it is [4, 9) of 8
    rc, msg = refused(desc(g_chunk0=4))
    assert rc == -1 and "chunks [4, 9) leave the gy planes operand (8 chunks per plane)" in msg, msg
    rc, msg = refused(desc(N=225))
    assert rc == -1 and "chunks [2, 10) leave the gy planes operand" in msg, msg
    # the extents follow the operand's own grid: a stride-2 layer's gy grid is a quarter of the pixels
    rc, msg = refused(desc(sy=2, sx=2, Ho=6, Wo=10, gy_plane_stride=6 * 2 * 6 * 10 * 32))
    assert rc == -1 and "chunks [2, 7) leave the gy planes operand (6 chunks per plane)" in msg, msg
    rc, msg = refused(desc(x_plane_stride=0))
    assert rc == -1 and "leave the x planes operand" in msg, msg


def test_a_workspace_smaller_than_splitm_slabs():
    slab = 130 * 70 * 9
    rc, msg = refused(desc(ws_elems=3 * slab - 1))
    assert rc == -1 and f"3 slabs of {slab} are needed" in msg, msg
    rc, msg = refused(desc(db=P, ws_elems=3 * slab))                   # the bias gradient's partial sums ride in the slab
    assert rc == -1 and f"3 slabs of {slab + 130} are needed" in msg, msg
    rc, msg = refused(desc(splitm=0))
    assert rc == -1 and "splitm" in msg, msg
    rc, msg = refused(desc(splitm=257, ws_elems=1 << 40))
    assert rc == -1 and "splitm" in msg, msg
