"""GPU suite: every entry point of csrc/raft_update.hip called on its own through `_lib`, against the plain references of
tests/raft_kernel_refs.py (proved on the CPU by tests/test_raft_update_ref_cpu.py).  What moves or splits numbers is compared
bit for bit; the gate arithmetic is compared with float64 and gated at three times the error of the same expression in torch
float32 on this device (the margin of test_all_pairs_correlation_on_the_igemm: the two sides differ in the order of float32
operations and in expf / tanhf only).  Every buffer is wider than the call needs and filled with a sentinel: what the call does not
own must still hold it.  The last grid has more pixels than one launch has threads (ufr::stream_grid caps it at 2048 x 256), so
every kernel's grid-stride loop runs a second time."""
import pytest
import torch

import raft_kernel_refs as R
from raft_kernel_refs import DEV, F32, Gate, LAUNCH_THREADS, PlaneBuf, device_lib as _lib, device_rand as _rand

pytestmark = pytest.mark.gpu
GRIDS = [(1, 5, 7), (2, 9, 11), (1, 1, 9), (2, 128, 160)]


def _span12(g, *shape):
    """Pre-activations over [-12, 12]: saturated sigmoids and tanh are among them, and the ends themselves."""
    v = (torch.rand(*shape, generator=g) * 24 - 12)
    v.view(-1)[:2] = torch.tensor([-12.0, 12.0])
    return v.to(DEV)


# ------------------------------------------------------------------------------------------------------ bit-exact group
@pytest.mark.parametrize("chunk0", [0, 1])
@pytest.mark.parametrize("B,H,W", GRIDS)
def test_flow_patches_gathers_the_7x7_neighbourhood_exactly(B, H, W, chunk0):
    L, lib = _lib()
    M = B * H * W
    g = torch.Generator().manual_seed(M + chunk0)
    flow = F32(_rand(g, B, 2, H, W, scale=3.0))
    out = PlaneBuf(chunk0 + 5, M, chunk0)
    L.check(lib.ufr_raft_flow_patches(flow.ptr, out.ptr, out.stride, chunk0, B, H, W, L.stream()), "flow patches")
    want = R.flow_patches(flow.t)
    assert torch.equal(out.own(4), R.split3(want))
    assert not bool(out.own(4)[:, 3, :, 2:].float().abs().any()), "channels 98..127 are not zero"
    assert out.rest_holds(4) and flow.guards_hold()
    assert M * 16 > LAUNCH_THREADS or (B, H, W) != GRIDS[-1]


@pytest.mark.parametrize("B,H,W", GRIDS)
def test_motion_finish_copies_the_motion_chunks_and_plants_the_flow(B, H, W):
    L, lib = _lib()
    M, c0 = B * H * W, 2
    g = torch.Generator().manual_seed(M)
    feat = _rand(g, 4, M, 32, scale=2.0)
    flow = F32(_rand(g, B, 2, H, W, scale=5.0))
    p1, p2 = PlaneBuf(7, M, c0, feat), PlaneBuf(8, M, c0)               # different plane strides
    before = p1.t.clone()
    L.check(lib.ufr_raft_motion_finish(p1.ptr, p1.stride, p2.ptr, p2.stride, c0, flow.ptr, B, H, W, L.stream()), "motion finish")
    want = before[:, c0:c0 + 4].clone()
    want[:, 3, :, 30:32] = R.split3(R.flow_rows(flow.t))
    assert torch.equal(p1.own(4), want), "p1: lanes 30, 31 of the last chunk = the flow, everything else as it was"
    assert torch.equal(p2.own(4), p1.own(4))
    assert torch.equal(R.merge3(p2.own(4))[3, :, 30:32], R.flow_rows(flow.t))
    assert p1.rest_holds(4) and p2.rest_holds(4) and flow.guards_hold()


@pytest.mark.parametrize("B,H,W,S,N", [(2, 9, 11, S, N) for S in (1, 3, 4, 6) for N in (126, 100)] + [(1, 1, 9, 3, 100), (1, 5, 7, 6, 126),
                                                                                                      (2, 128, 160, 3, 126)])
def test_motion_finish_from_the_split_k_slabs(B, H, W, S, N):
    L, lib = _lib()
    M, c0 = B * H * W, 1
    g = torch.Generator().manual_seed(M + S * 128 + N)
    slabs = F32(_rand(g, S, M, 128, scale=2.0))                         # (columns N..127 hold numbers too: they must come out as zeros)
    bias = F32(_rand(g, N))
    flow = F32(_rand(g, B, 2, H, W, scale=5.0))
    for slope in (0.0, 0.1):
        p1, p2 = PlaneBuf(6, M, c0), PlaneBuf(9, M, c0)
        L.check(lib.ufr_raft_motion_finish_slabs(slabs.ptr, S, 128, N, bias.ptr, slope, p1.ptr, p1.stride, p2.ptr, p2.stride, c0, flow.ptr,
                                                 B, H, W, L.stream()), "motion finish (slabs)")
        want = R.motion_finish_slabs(slabs.t, bias.t, N, slope, flow.t)
        assert torch.equal(p1.own(4), R.split3(want)), f"slope {slope}"
        assert torch.equal(p2.own(4), p1.own(4))
        got = p1.values(4).permute(1, 0, 2).reshape(M, 128)
        assert not bool(got[:, N:126].any()) and torch.equal(got[:, 126:], R.flow_rows(flow.t))
        assert bool((got[:, :N] < 0).any()) == (slope > 0), "the inputs do not reach the negative side of the LeakyReLU"
        assert p1.rest_holds(4) and p2.rest_holds(4)
    assert slabs.guards_hold() and bias.guards_hold() and flow.guards_hold()


@pytest.mark.parametrize("with_delta", [True, False])
@pytest.mark.parametrize("n", [70, 2 * 2 * 9 * 11, LAUNCH_THREADS + 75_713])
def test_coords_step_is_add_copy_subtract(n, with_delta):
    L, lib = _lib()
    assert n % 256
    g = torch.Generator().manual_seed(n)
    c1, c0, d = F32(_rand(g, n, scale=40.0)), F32(_rand(g, n, scale=40.0)), F32(_rand(g, n))
    saved, flow = F32(shape=(n,)), F32(shape=(n,))
    want_c1, want_saved, want_flow = R.coords_step(c1.t.clone(), d.t if with_delta else None, c0.t)
    L.check(lib.ufr_raft_coords_step(c1.ptr, d.ptr if with_delta else None, c0.ptr, saved.ptr, flow.ptr, n, L.stream()), "coords step")
    assert torch.equal(c1.t, want_c1) and torch.equal(saved.t, want_saved) and torch.equal(flow.t, want_flow)
    assert all(b.guards_hold() for b in (c1, c0, d, saved, flow))


@pytest.mark.parametrize("B,H,W,chunks,off", [(1, 5, 7, 1, 2), (2, 9, 11, 4, 2), (1, 1, 9, 3, 1), (2, 128, 160, 4, 2)])
def test_grad_finalize_consume_masks_splits_and_leaves_zeros(B, H, W, chunks, off):
    L, lib = _lib()
    M = B * H * W
    g = torch.Generator().manual_seed(M + chunks)
    maskv = torch.round(_rand(g, chunks, M, 32, scale=1.5))
    assert bool((maskv == 0).any()) and bool((maskv < 0).any()) and bool((maskv > 0).any())
    mask = PlaneBuf(off + chunks + 1, M, off)
    mask.t[0, off:off + chunks] = maskv.to(torch.bfloat16)              # plane 0 alone is the mask; the engine passes it from chunk `off` on
    gsum0 = _rand(g, chunks, M, 32)
    for slope in (0.0, 0.1):
        gsum = F32(gsum0)
        out = PlaneBuf(chunks + 1, M, 0)
        L.check(lib.ufr_grad_finalize_consume(gsum.ptr, mask.chunk_ptr(off), out.ptr, out.stride, M, chunks, slope, L.stream()), "finalize")
        assert torch.equal(out.own(chunks), R.split3(R.grad_finalize(gsum0, maskv, slope))), f"slope {slope}"
        assert not bool(gsum.t.any()), "the consumed sum is not all zeros"
        assert out.rest_holds(chunks) and gsum.guards_hold()


# ------------------------------------------------------------------------------------------------------ slab forms
SPLITS = (1, 2, 3, 4, 5, 7, 8, 9, 11, 13)        # load_slabs8: scalar tail alone, groups of four (+ tail), the 8-wide path (5..8), 8 < S


def _slab_case(g, S, M, Npad, used, nch_addend):
    slabs = torch.full((S, M, Npad), float("nan"))                      # columns the form does not own: whoever reads them gets NaN
    slabs[:, :, :used] = torch.randn(S, M, used, generator=g) * (6.0 / S ** 0.5)
    bias = torch.full((Npad,), float("nan"))
    bias[:used] = torch.randn(used, generator=g)
    addend = _rand(g, nch_addend, M, 32, scale=3.0) if nch_addend else None
    return F32(slabs.to(DEV)), F32(bias.to(DEV)), (F32(addend) if addend is not None else None)


@pytest.mark.parametrize("with_addend", [False, True])
@pytest.mark.parametrize("B,H,W,chunks,Npad,splits", [(2, 9, 11, 1, 128, SPLITS), (1, 5, 7, 4, 256, SPLITS), (2, 128, 160, 4, 256, (5,))])
def test_gates_reading_slabs_equal_the_plain_form_on_the_float32_sum(B, H, W, chunks, Npad, splits, with_addend):
    L, lib = _lib()
    M, hc0, rc0 = B * H * W, 1, 2
    g = torch.Generator().manual_seed(M + chunks + with_addend)
    h = PlaneBuf(hc0 + chunks + 1, M, hc0, _rand(g, chunks, M, 32))
    for S in splits:
        slabs, bias, addend = _slab_case(g, S, M, Npad, 2 * chunks * 32, 2 * chunks if with_addend else 0)
        pre = R.slab_preact(slabs.t, bias.t, addend.t if addend else None, 0, 2 * chunks)
        assert bool(torch.isfinite(pre).all())
        zr_a, rh_a = F32(pre), PlaneBuf(rc0 + chunks + 1, M, rc0)
        L.check(lib.ufr_gru_gates_cm_forward(zr_a.ptr, h.ptr, h.stride, hc0, rh_a.ptr, rh_a.stride, rc0, M, chunks, L.stream()), "gates")
        zr_b, rh_b = F32(shape=pre.shape), PlaneBuf(rc0 + chunks + 2, M, rc0)
        L.check(lib.ufr_gru_gates_cm_forward_slabs(slabs.ptr, S, Npad, bias.ptr, addend.ptr if addend else None, zr_b.ptr, h.ptr, h.stride, hc0,
                                                   rh_b.ptr, rh_b.stride, rc0, M, chunks, L.stream()), "gates (slabs)")
        assert torch.equal(zr_b.t, zr_a.t), f"S = {S}: the sigmoid values differ"
        assert torch.equal(rh_b.own(chunks), rh_a.own(chunks)), f"S = {S}: the r * h planes differ"
        assert bool(torch.isfinite(zr_b.t).all()) and float(zr_b.t.min()) < 0.02 and float(zr_b.t.max()) > 0.98
        assert rh_a.rest_holds(chunks) and rh_b.rest_holds(chunks) and zr_a.guards_hold() and zr_b.guards_hold()
        assert slabs.guards_hold() and bias.guards_hold() and (addend is None or addend.guards_hold())
    assert h.rest_holds(chunks)


@pytest.mark.parametrize("with_addend", [False, True])
@pytest.mark.parametrize("B,H,W,chunks,Npad,splits", [(2, 9, 11, 1, 128, SPLITS), (1, 5, 7, 4, 128, SPLITS), (2, 128, 160, 4, 128, (7,))])
def test_blend_reading_slabs_equals_the_plain_form_on_the_float32_sum(B, H, W, chunks, Npad, splits, with_addend):
    L, lib = _lib()
    M, hc0, oc0 = B * H * W, 2, 1
    g = torch.Generator().manual_seed(M + chunks + with_addend + 100)
    h = PlaneBuf(hc0 + chunks + 1, M, hc0, _rand(g, chunks, M, 32))
    z = F32(torch.sigmoid(_span12(g, chunks, M, 32)))
    for S in splits:
        slabs, bias, addend = _slab_case(g, S, M, Npad, chunks * 32, chunks if with_addend else 0)
        pre = R.slab_preact(slabs.t, bias.t, addend.t if addend else None, 0, chunks)
        assert bool(torch.isfinite(pre).all())
        q_a, out_a = F32(pre), PlaneBuf(oc0 + chunks + 1, M, oc0)
        L.check(lib.ufr_gru_blend_cm_forward(q_a.ptr, z.ptr, h.ptr, h.stride, hc0, out_a.ptr, out_a.stride, oc0, M, chunks, L.stream()), "blend")
        q_b, out_b = F32(shape=pre.shape), PlaneBuf(oc0 + chunks + 3, M, oc0)
        L.check(lib.ufr_gru_blend_cm_forward_slabs(slabs.ptr, S, Npad, bias.ptr, addend.ptr if addend else None, q_b.ptr, z.ptr, h.ptr, h.stride,
                                                   hc0, out_b.ptr, out_b.stride, oc0, M, chunks, L.stream()), "blend (slabs)")
        assert torch.equal(q_b.t, q_a.t), f"S = {S}: the tanh values differ"
        assert torch.equal(out_b.own(chunks), out_a.own(chunks)), f"S = {S}: the output planes differ"
        assert bool(torch.isfinite(q_b.t).all()) and float(q_b.t.min()) < -0.98 and float(q_b.t.max()) > 0.98
        assert out_a.rest_holds(chunks) and out_b.rest_holds(chunks) and q_a.guards_hold() and q_b.guards_hold()
        assert slabs.guards_hold() and bias.guards_hold() and (addend is None or addend.guards_hold())
    assert h.rest_holds(chunks) and z.guards_hold()


# ------------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("chunks", [1, 4])
@pytest.mark.parametrize("B,H,W", GRIDS)
def test_gate_and_blend_forward_against_float64(B, H, W, chunks):
    L, lib = _lib()
    M, hc0, rc0, oc0 = B * H * W, 2, 1, 3
    g = torch.Generator().manual_seed(M * 8 + chunks)
    zr_pre, q_pre, hv = _span12(g, 2 * chunks, M, 32), _span12(g, chunks, M, 32), _rand(g, chunks, M, 32)
    h = PlaneBuf(hc0 + chunks + 1, M, hc0, hv)
    zr, rh = F32(zr_pre), PlaneBuf(rc0 + chunks + 2, M, rc0)
    L.check(lib.ufr_gru_gates_cm_forward(zr.ptr, h.ptr, h.stride, hc0, rh.ptr, rh.stride, rc0, M, chunks, L.stream()), "gates")
    gate = Gate(f"forward {B}x{H}x{W} chunks={chunks}")
    zr64, rh64 = R.gates_forward(zr_pre.double(), hv.double())
    zr32, rh32 = R.gates_forward(zr_pre, hv)
    gate.add("sigmoid(zr)", zr.t, zr32, zr64)
    gate.add("r*h planes", rh.values(chunks), rh32, rh64)
    assert float(zr.t.min()) < 1e-5 and float(zr.t.max()) > 1 - 1e-5, "no saturated sigmoid among the inputs"
    # the blend on the kernel's own z values, as the engine chains them (float64 from the same float32 values)
    zv = zr.t[:chunks].clone()
    q, out = F32(q_pre), PlaneBuf(oc0 + chunks + 1, M, oc0)
    L.check(lib.ufr_gru_blend_cm_forward(q.ptr, zr.ptr, h.ptr, h.stride, hc0, out.ptr, out.stride, oc0, M, chunks, L.stream()), "blend")
    q64, out64 = R.blend_forward(q_pre.double(), zv.double(), hv.double())
    q32, out32 = R.blend_forward(q_pre, zv, hv)
    gate.add("tanh(q)", q.t, q32, q64)
    gate.add("h' planes", out.values(chunks), out32, out64)
    assert float(q.t.abs().max()) == 1.0, "no saturated tanh among the inputs"
    assert torch.equal(zr.t[:chunks], zv), "the blend changed z"
    assert h.rest_holds(chunks) and torch.equal(h.own(chunks), R.split3(hv)) and rh.rest_holds(chunks) and out.rest_holds(chunks)
    assert zr.guards_hold() and q.guards_hold()
    gate.check()


@pytest.mark.parametrize("chunks", [1, 4])
@pytest.mark.parametrize("B,H,W", GRIDS)
def test_gate_and_blend_adjoint_against_float64(B, H, W, chunks):
    L, lib = _lib()
    M, hc0, qc0, zc0 = B * H * W, 1, 2, 3
    g = torch.Generator().manual_seed(M * 8 + chunks + 1)
    hv = _rand(g, chunks, M, 32)
    h = PlaneBuf(hc0 + chunks + 1, M, hc0, hv)
    zrv, qv = torch.sigmoid(_span12(g, 2 * chunks, M, 32)), torch.tanh(_span12(g, chunks, M, 32))
    gv, g_rhv, g_h0, g_zv = (_rand(g, chunks, M, 32) for _ in range(4))
    acc_q0, acc_zr0 = _rand(g, chunks, M, 32, scale=2.0), _rand(g, 2 * chunks, M, 32, scale=2.0)
    zr, q, gin = F32(zrv), F32(qv), F32(gv)
    gate = Gate(f"adjoint {B}x{H}x{W} chunks={chunks}")
    dbl = lambda *ts: [t.double() for t in ts]

    # ---- blend: g_q_pre planes, g_z, g_h written; the running sum added to
    def blend(acc0):
        gq, g_z, g_h = PlaneBuf(qc0 + chunks + 1, M, qc0), F32(shape=hv.shape), F32(shape=hv.shape)
        acc = F32(acc0) if acc0 is not None else None
        L.check(lib.ufr_gru_blend_cm_backward(q.ptr, zr.ptr, h.ptr, h.stride, hc0, gin.ptr, gq.ptr, gq.stride, qc0, g_z.ptr, g_h.ptr, M, chunks,
                                              acc.ptr if acc else None, L.stream()), "blend backward")
        assert gq.rest_holds(chunks) and g_z.guards_hold() and g_h.guards_hold() and (acc is None or acc.guards_hold())
        return gq, g_z, g_h, acc

    gq, g_z, g_h, acc = blend(acc_q0)
    want64 = R.blend_backward(*dbl(qv, zrv[:chunks], hv, gv, acc_q0))
    want32 = R.blend_backward(qv, zrv[:chunks], hv, gv, acc_q0)
    for name, got, w32, w64 in zip(("g_q_pre planes", "g_z", "g_h (blend)", "acc_gq"), (gq.values(chunks), g_z.t, g_h.t, acc.t), want32, want64):
        gate.add(name, got, w32, w64)
    assert not torch.equal(acc.t, acc_q0)
    gq_n, g_z_n, g_h_n, _ = blend(None)                                 # acc = NULL: nothing else changes
    assert torch.equal(gq_n.own(chunks), gq.own(chunks)) and torch.equal(g_z_n.t, g_z.t) and torch.equal(g_h_n.t, g_h.t)

    # ---- gates: g_zr_pre planes in both halves, g_h updated in place from a non-zero value, g_rh consumed or not
    def gates(acc0, consume):
        gzr, g_rh, gh = PlaneBuf(zc0 + 2 * chunks + 1, M, zc0), F32(g_rhv), F32(g_h0)
        g_zin = F32(g_zv)
        acc = F32(acc0) if acc0 is not None else None
        L.check(lib.ufr_gru_gates_cm_backward(zr.ptr, h.ptr, h.stride, hc0, g_zin.ptr, g_rh.ptr, gzr.ptr, gzr.stride, zc0, gh.ptr, M, chunks,
                                              consume, acc.ptr if acc else None, L.stream()), "gates backward")
        assert gzr.rest_holds(2 * chunks) and g_rh.guards_hold() and gh.guards_hold() and (acc is None or acc.guards_hold())
        assert torch.equal(g_zin.t, g_zv) and g_zin.guards_hold()
        return gzr, g_rh, gh, acc

    gzr, g_rh, gh, acc = gates(acc_zr0, 1)
    want64 = R.gates_backward(*dbl(zrv, hv, g_zv, g_rhv, g_h0, acc_zr0))
    want32 = R.gates_backward(zrv, hv, g_zv, g_rhv, g_h0, acc_zr0)
    got = gzr.values(2 * chunks)
    gate.add("g_z_pre planes", got[:chunks], want32[0][:chunks], want64[0][:chunks])
    gate.add("g_r_pre planes", got[chunks:], want32[0][chunks:], want64[0][chunks:])
    gate.add("g_h (in place)", gh.t, want32[1], want64[1])
    gate.add("acc_gzr [z]", acc.t[:chunks], want32[2][:chunks], want64[2][:chunks])
    gate.add("acc_gzr [r]", acc.t[chunks:], want32[2][chunks:], want64[2][chunks:])
    assert not bool(g_rh.t.any()), "consume_g_rh = 1 must leave zeros in g_rh"
    assert not torch.equal(gh.t, g_h0)
    gzr_n, g_rh_n, gh_n, _ = gates(None, 0)                             # acc = NULL, not consumed: g_rh untouched, nothing else changes
    assert torch.equal(g_rh_n.t, g_rhv), "consume_g_rh = 0 must leave g_rh as it was"
    assert torch.equal(gzr_n.own(2 * chunks), gzr.own(2 * chunks)) and torch.equal(gh_n.t, gh.t)
    assert torch.equal(zr.t, zrv) and torch.equal(q.t, qv) and torch.equal(gin.t, gv) and torch.equal(h.own(chunks), R.split3(hv))
    assert h.rest_holds(chunks) and zr.guards_hold() and q.guards_hold() and gin.guards_hold()
    gate.check()
