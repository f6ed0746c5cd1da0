"""The operator entries of libufr_hip.so write every element of their outputs -- and nothing else.

The Python mirrors allocate outputs with torch.empty and the caching allocator often hands back the previous call's (correct)
result, so an element a kernel leaves unwritten can go unnoticed.  Here the C ABI is called directly: every output buffer is filled
with NaN and lies between two guard bands of 64 sentinel elements.  After the call the return code is 0, the guards are as they
were, and the output is finite and equals the reference under the strict helper (tests/closeness.py: one NaN left fails).  Entries
documented to accumulate (`ufr_corr_lookup_backward`, anything with `accumulate != 0`) get a finite random prefill instead and
must return prefill + result.

References and tolerances are those of the operators' existing tests (test_ops_gpu.py, test_raft_upsample_gpu.py,
test_pwc_warp_gpu.py, test_fn2_glue_gpu.py): the CPU oracle on the same inputs for the correlation, alt_cuda_corr and its pyramid
forms, the lookup's forward, Resample2d and ChannelNorm; the torch spelling in float64 for the others.  Workspaces (scratch the call
writes before it reads) are handed over zeroed.

Each correlation case names the branch of the host dispatcher (csrc/correlation.hip::ufr_corr_forward_fused / ufr_corr_backward)
it reaches and why.  The widths at which the vectorised launches decline, from the constants of csrc/correlation_vec.hip and
csrc/correlation_mfma.hip (kMaxLds = 160 KiB, ufr_common.h):
  forward, correlation_vec.hip::launch_fwd<P, DP, PHB 3, CK 4>: G = ceil(ceil(W / DP) / 4), NT = round_up(3 DP G, 64) must be
    <= kVecMaxThreads = 384.  Patch 21 (DP 2): 6 G <= 384 holds up to G = 64 (W = 512); W = 516 gives G = 65, NT = 448: declined.
    Patch 9 (DP 1): 3 G <= 384 holds up to G = 128 (W = 512); W = 516 gives G = 129, NT = 448: declined.  LDS is far from its limit
    there (39424 and 36096 bytes), so the thread limit is the one that binds, at W = 516 for both.
  backward, patch 21: correlation_mfma.hip::launch<21, 2, ., 32, 2>: UT = ceil(ceil(W / 2) / 16), U16 = 16 UT, LUa = U16 + 20 padded
    to 18 (mod 32), LDS = 4 (2 * 32 * LUa + 2 * U16 * 51) bytes.  W = 448: UT 14, LUa 274, 161536 bytes <= 163840: taken.  W = 452:
    UT 15, U16 240, LUa 274, 168064 bytes: declined (before its thread limit, NT = 64 UT <= 1024, which binds from W = 516 on).  The VALU
    kernels behind it, correlation_vec.hip::launch_bwd<21, 2, 16, 4>, need NT = round_up(8 G, 64) <= 384, G <= 48, W <= 384: declined
    too, so W = 452 is the smallest width whose adjoint runs corr_bwd_fast although W % 4 == 0.
  backward, patch 9: correlation_mfma.hip::launch<9, 1, ., 32, 2>: UT = ceil(W / 16), NT = 64 ceil(UT / 2) <= 1024 holds up to W = 512
    (LDS 147712 bytes there); W = 516: UT 33, NT 1088: declined; launch_bwd<9, 1, 32, 4>: NT = round_up(8 ceil(W / 4), 64) = 1088 >
    1024: declined.  W = 516."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from closeness import assert_close
from conftest import load_golden
from test_oracle_cpu import expand_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = -1234.5
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    from understanding_flow_robustness_amd import _lib
    assert _lib.lib().ufr_device_count() >= 1
    return _lib


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _poisoned(shape, dtype=torch.float32, prefill=None):
    """(buffer, the output view inside it): GUARD sentinels, the output -- NaN, or `prefill` for an accumulating entry --, GUARD
    sentinels.  The view starts 64 elements in, so it keeps the 16-byte alignment of the allocation."""
    n = _numel(shape)
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    out = buf[GUARD:GUARD + n].view(shape)
    if prefill is None:
        out.fill_(NAN)
    else:
        out.copy_(prefill)
    return buf, out


def _ok(L, rc, what):
    assert rc == 0, f"{what}: return code {rc}: {L.lib().ufr_last_error().decode('utf-8', 'replace')}"


def _guards_intact(buf):
    sentinel = torch.tensor(SENTINEL, dtype=buf.dtype, device=buf.device)          # (float16 and bfloat16 round it)
    return bool((buf[:GUARD] == sentinel).all()) and bool((buf[-GUARD:] == sentinel).all())


def _written(buf, out, ref, what, **tol):
    torch.cuda.synchronize()
    assert _guards_intact(buf), f"{what}: a guard band was written"
    assert_close(out.float() if out.dtype == torch.float16 else out, ref, what=what, **tol)


# ---------------------------------------------------------------------------- spatial correlation
FAST21 = (1, 1, 21, 21, 0, 0, 1, 1, 2, 2, 1, 1)
FAST9 = (1, 1, 9, 9, 0, 0, 1, 1, 1, 1, 1, 1)
RECT = expand_params(load_golden("corr_rect_f32")["params"])      # kernel 3 x 1, patch 3 x 5, padding, strides, dilations: not fast-path eligible
CORR_TOL = {torch.float32: dict(rtol=1e-4, atol_scale=2e-6), torch.float64: dict(rtol=1e-9, atol_scale=1e-12),
            torch.float16: dict(rtol=1e-3, atol_scale=1e-3)}       # test_ops_gpu.py: golden / oracle cases, float16 storage

CORR_CASES = [
    # W % 4 == 0: forward corr_fwd_vec (corr_fwd_vec_launch takes it), adjoint on the matrix cores (corr_bwd_mfma_launch takes it)
    pytest.param(torch.float32, (1, 5, 6, 12), FAST21, id="p21-W12-vec-mfma"),
    pytest.param(torch.float32, (1, 5, 6, 12), FAST9, id="p9-W12-vec-mfma"),
    # W % 4 != 0: both vectorised launches return 1; B * H = 6 rows < 256 / 512 -> launch_fwd_fast<21,2,3,8> / <9,1,3,8>; launch_bwd_fast
    pytest.param(torch.float32, (1, 5, 6, 9), FAST21, id="p21-W9-fast-few-rows"),
    pytest.param(torch.float32, (1, 5, 6, 9), FAST9, id="p9-W9-fast-few-rows"),
    # W % 4 != 0 and B * H = 260 >= 256: launch_fwd_fast<21,2,7,8>;  B * H = 520 >= 512: launch_fwd_fast<9,1,9,8>
    pytest.param(torch.float32, (2, 5, 130, 9), FAST21, id="p21-W9-fast-many-rows"),
    pytest.param(torch.float32, (4, 5, 130, 9), FAST9, id="p9-W9-fast-many-rows"),
    # W % 4 == 0 but the vectorised launches decline (module docstring): W = 452, patch 21: forward still corr_fwd_vec, adjoint
    # corr_bwd_fast (two tiles along W); W = 516 (three tiles): forward launch_fwd_fast<.,.,3,8> (thread limit), adjoint corr_bwd_fast
    pytest.param(torch.float32, (1, 5, 3, 452), FAST21, id="p21-W452-mfma-declines-lds"),
    pytest.param(torch.float32, (1, 5, 3, 516), FAST21, id="p21-W516-vec-declines-threads"),
    pytest.param(torch.float32, (1, 5, 3, 516), FAST9, id="p9-W516-vec-declines-threads"),
    # not fast_eligible (kernel 3 x 1, padding, strides): corr_fwd_generic / corr_bwd_generic <float>, <_Float16, float>, <double>
    pytest.param(torch.float32, (2, 3, 9, 11), RECT, id="rect-generic-f32"),
    pytest.param(torch.float16, (2, 3, 9, 11), RECT, id="rect-generic-f16"),
    pytest.param(torch.float64, (2, 3, 9, 11), RECT, id="rect-generic-f64"),
    # fast_eligible parameters in another dtype: the dispatcher asks dtype == UFR_F32 first -> generic kernels
    pytest.param(torch.float64, (1, 5, 6, 12), FAST9, id="p9-W12-f64-generic"),
]


def _corr_operands(dtype, shape, prm, seed):
    """Operands on the CPU in the oracle's dtype (float16: the half-rounded values in float32, as test_corr_float16_storage
    compares) and the output shape."""
    g = torch.Generator().manual_seed(seed)
    odt = torch.float32 if dtype == torch.float16 else dtype
    a, b = (torch.randn(shape, generator=g, dtype=odt) for _ in range(2))
    B, C, H, W = shape
    kH, kW, pH, pW, padH, padW, dilH, dilW, _, _, dH, dW = prm
    oH = (H + 2 * padH - ((kH - 1) * dilH + 1)) // dH + 1
    oW = (W + 2 * padW - ((kW - 1) * dilW + 1)) // dW + 1
    go = torch.randn(B, pH, pW, oH, oW, generator=g, dtype=odt)
    if dtype == torch.float16:
        a, b, go = (v.half().float() for v in (a, b, go))
    return a, b, go


@pytest.mark.parametrize("dtype,shape,prm", CORR_CASES)
def test_corr_entries_write_every_element(L, oracle, dtype, shape, prm):
    a, b, go = _corr_operands(dtype, shape, prm, seed=sum(shape) + prm[2])
    B, C, H, W = shape
    code, tol = L.dtype_code(torch.empty(0, dtype=dtype)), CORR_TOL[dtype]
    p = L.CorrParams(*prm)
    ad, bd, god = (v.to(DEV, dtype) for v in (a, b, go))
    buf, out = _poisoned(go.shape, dtype)
    _ok(L, L.lib().ufr_corr_forward(L.ptr(ad), L.ptr(bd), L.ptr(out), code, B, C, H, W, ctypes.byref(p), L.stream()), "ufr_corr_forward")
    _written(buf, out, oracle.corr_forward(a, b, *prm), "ufr_corr_forward", **tol)
    buf1, g1 = _poisoned(shape, dtype)
    buf2, g2 = _poisoned(shape, dtype)
    _ok(L, L.lib().ufr_corr_backward(L.ptr(ad), L.ptr(bd), L.ptr(god), L.ptr(g1), L.ptr(g2), code, B, C, H, W, ctypes.byref(p), L.stream()),
        "ufr_corr_backward")
    r1, r2 = oracle.corr_backward(a, b, go, *prm)
    _written(buf1, g1, r1, "ufr_corr_backward grad_input1", **tol)
    _written(buf2, g2, r2, "ufr_corr_backward grad_input2", **tol)


@pytest.mark.parametrize("shape,prm", [pytest.param((1, 5, 6, 12), FAST21, id="p21-W12-vec"),            # the epilogue of corr_fwd_vec
                                       pytest.param((1, 5, 6, 9), FAST9, id="p9-W9-fast"),               # ... of corr_fwd_fast
                                       pytest.param((2, 3, 9, 11), RECT, id="rect-generic")])            # ... of corr_fwd_generic
def test_corr_fused_entry_writes_every_element(L, oracle, shape, prm):
    """scale = 1/16, slope = 0.1 (test_corr_fused_epilogue): against leaky(oracle / 16) at the forward's tolerance, and against
    leaky(the plain entry's result / 16) at that test's 1e-6 / 1e-7."""
    a, b, go = _corr_operands(torch.float32, shape, prm, seed=8)
    B, C, H, W = shape
    p = L.CorrParams(*prm)
    ad, bd = a.to(DEV), b.to(DEV)
    bufp, plain = _poisoned(go.shape)
    _ok(L, L.lib().ufr_corr_forward(L.ptr(ad), L.ptr(bd), L.ptr(plain), L.UFR_F32, B, C, H, W, ctypes.byref(p), L.stream()), "ufr_corr_forward")
    buf, fused = _poisoned(go.shape)
    _ok(L, L.lib().ufr_corr_forward_fused(L.ptr(ad), L.ptr(bd), L.ptr(fused), L.UFR_F32, B, C, H, W, ctypes.byref(p), 1.0 / 16, 0.1, L.stream()),
        "ufr_corr_forward_fused")
    _written(buf, fused, F.leaky_relu(oracle.corr_forward(a, b, *prm) / 16, 0.1), "ufr_corr_forward_fused vs oracle", **CORR_TOL[torch.float32])
    _written(bufp, plain, oracle.corr_forward(a, b, *prm), "ufr_corr_forward", **CORR_TOL[torch.float32])
    assert_close(fused, F.leaky_relu(plain / 16, 0.1), rtol=1e-6, atol_scale=1e-7, what="ufr_corr_forward_fused vs the plain entry")


# ---------------------------------------------------------------------------- alt_cuda_corr
def _alt_inputs(B, H, W, C, g, spread):
    f1 = torch.randn(B, H, W, C, generator=g)
    f2 = torch.randn(B, H, W, C, generator=g)
    xs = torch.arange(W).float().view(1, 1, 1, W).expand(B, 1, H, W)
    ys = torch.arange(H).float().view(1, 1, H, 1).expand(B, 1, H, W)
    coords = torch.stack([xs, ys], -1) + spread * torch.randn(B, 1, H, W, 2, generator=g)
    return f1, f2, coords.contiguous()


@pytest.mark.parametrize("spread", [3.0, 60.0], ids=["spread3", "spread60-windows-outside-the-image"])
def test_altcorr_entries_write_every_element(L, oracle, spread):
    """(B, H, W, C, r) = (1, 6, 7, 40, 3): 40 channels are no multiple of the 32-channel slab.  fmap2_grad (the callee zeroes what it
    accumulates into) and coords_grad (zero, as the reference leaves it) are handed over as NaN like everything else."""
    B, H, W, C, r = 1, 6, 7, 40, 3
    g = torch.Generator().manual_seed(int(spread) + H)
    f1, f2, coords = _alt_inputs(B, H, W, C, g, spread)
    rd = 2 * r + 1
    f1d, f2d, cd = f1.to(DEV), f2.to(DEV), coords.to(DEV)
    buf, corr = _poisoned((B, 1, rd * rd, H, W))
    _ok(L, L.lib().ufr_altcorr_forward(L.ptr(f1d), L.ptr(f2d), L.ptr(cd), L.ptr(corr), B, 1, H, W, H, W, C, r, L.stream()), "ufr_altcorr_forward")
    (ref,) = oracle.altcorr_forward(f1, f2, coords, r)
    _written(buf, corr, ref, "ufr_altcorr_forward", rtol=1e-4, atol_scale=2e-6)
    go = torch.randn(ref.shape, generator=g)
    god = go.to(DEV)
    (b1, g1), (b2, g2), (bc, gc) = _poisoned(f1.shape), _poisoned(f2.shape), _poisoned(coords.shape)
    _ok(L, L.lib().ufr_altcorr_backward(L.ptr(f1d), L.ptr(f2d), L.ptr(cd), L.ptr(god), L.ptr(g1), L.ptr(g2), L.ptr(gc), B, 1, H, W, H, W, C,
                                        r, L.stream()), "ufr_altcorr_backward")
    r1, r2, _ = oracle.altcorr_backward(f1, f2, coords, go, r)
    _written(b1, g1, r1, "ufr_altcorr_backward fmap1_grad", rtol=1e-4, atol_scale=2e-6)
    _written(b2, g2, r2, "ufr_altcorr_backward fmap2_grad", rtol=1e-4, atol_scale=1e-5)
    _written(bc, gc, torch.zeros_like(coords), "ufr_altcorr_backward coords_grad", rtol=0.0, atol_scale=0.0)
    assert float(gc.abs().max()) == 0.0


# ---------------------------------------------------------------------------- the pyramid forms and the all-pairs lookup
PYR = dict(B=1, H=8, W=21, C=128, r=4, levels=2)      # two levels; 21 is no multiple of the 16-pixel tile


def _pyramid_inputs(spread=3.0):
    B, H, W, C, nl = PYR["B"], PYR["H"], PYR["W"], PYR["C"], PYR["levels"]
    g = torch.Generator().manual_seed(B * 1000 + H)
    f1 = torch.randn(B, H, W, C, generator=g)
    f2s = [torch.randn(B, H >> i, W >> i, C, generator=g) for i in range(nl)]
    xs = torch.arange(W).float().view(1, 1, 1, W).expand(B, 1, H, W)
    ys = torch.arange(H).float().view(1, 1, H, 1).expand(B, 1, H, W)
    coords = (torch.cat([xs, ys], 1) + spread * torch.randn(B, 2, H, W, generator=g)).contiguous()
    return g, f1, f2s, coords


def _level_coords(coords, i):
    B, _, H, W = coords.shape
    return (coords.permute(0, 2, 3, 1) / 2 ** i).reshape(B, 1, H, W, 2).contiguous()


def _levels_struct(L, f2d, grads=None):
    lv = L.AltCorrLevels()
    lv.num_levels = len(f2d)
    for i, f in enumerate(f2d):
        lv.fmap2[i] = f.data_ptr()
        lv.fmap2_grad[i] = grads[i].data_ptr() if grads is not None else None
        lv.H2[i], lv.W2[i] = int(f.shape[1]), int(f.shape[2])
        lv.coord_scale[i] = 1.0 / 2 ** i
    return lv


def test_altcorr_pyramid_forward_writes_every_element(L, oracle):
    B, H, W, C, r, nl = (PYR[k] for k in ("B", "H", "W", "C", "r", "levels"))
    _, f1, f2s, coords = _pyramid_inputs()
    scale, n = 1.0 / math.sqrt(C), (2 * r + 1) ** 2
    f1d, f2d, cd = f1.to(DEV), [f.to(DEV) for f in f2s], coords.to(DEV)
    lv = _levels_struct(L, f2d)
    buf, out = _poisoned((B, nl * n, H, W))
    _ok(L, L.lib().ufr_altcorr_pyramid_forward(L.ptr(f1d), ctypes.byref(lv), L.ptr(cd), L.ptr(out), B, H, W, C, r, scale, L.stream()),
        "ufr_altcorr_pyramid_forward")
    want = torch.cat([oracle.altcorr_forward(f1, f2s[i], _level_coords(coords, i), r)[0].squeeze(1) * scale for i in range(nl)], 1)
    for i in range(nl):       # per level, as test_altcorr_pyramid_on_the_matrix_cores_vs_oracle compares
        _written(buf, out[:, i * n:(i + 1) * n], want[:, i * n:(i + 1) * n], f"ufr_altcorr_pyramid_forward level {i}", rtol=1e-4, atol_scale=2e-6)


def test_altcorr_planes_forward_writes_every_element(L, oracle):
    """The split planes of `ufr_altcorr_planes_prepare` are outputs too: handed over as NaN, finite afterwards, and their values
    are checked through the lookup that reads them."""
    B, H, W, C, r, nl = (PYR[k] for k in ("B", "H", "W", "C", "r", "levels"))
    _, f1, f2s, coords = _pyramid_inputs()
    scale, n = 1.0 / math.sqrt(C), (2 * r + 1) ** 2
    planes = []
    for f in (f1, *f2s):
        fd, npix = f.to(DEV), f.shape[0] * f.shape[1] * f.shape[2]
        pbuf, p = _poisoned((3, npix * C), torch.bfloat16)
        _ok(L, L.lib().ufr_altcorr_planes_prepare(L.ptr(fd), L.ptr(p), p.stride(0), npix, C, L.stream()), "ufr_altcorr_planes_prepare")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(p.float()).all()), "ufr_altcorr_planes_prepare left elements unwritten"
        assert _guards_intact(pbuf), "ufr_altcorr_planes_prepare: a guard band was written"
        planes.append((pbuf, p))
    lv = L.AltCorrPlaneLevels()
    lv.num_levels = nl
    for i, (_, p) in enumerate(planes[1:]):
        lv.planes[i], lv.plane_stride[i] = p.data_ptr(), p.stride(0)
        lv.H2[i], lv.W2[i], lv.coord_scale[i] = int(f2s[i].shape[1]), int(f2s[i].shape[2]), 1.0 / 2 ** i
    buf, out = _poisoned((B, nl * n, H, W))
    f1p, cd = planes[0][1], coords.to(DEV)
    _ok(L, L.lib().ufr_altcorr_planes_forward(L.ptr(f1p), f1p.stride(0), ctypes.byref(lv), L.ptr(cd), L.ptr(out), B, H, W, C, r, scale,
                                              L.stream()), "ufr_altcorr_planes_forward")
    for i in range(nl):       # per level, as test_altcorr_lookup_on_split_planes_vs_oracle compares
        (ref,) = oracle.altcorr_forward(f1, f2s[i], _level_coords(coords, i), r)
        _written(buf, out[:, i * n:(i + 1) * n], ref.squeeze(1) * scale, f"ufr_altcorr_planes_forward level {i}", rtol=1e-4, atol_scale=2e-6)


@pytest.mark.parametrize("accumulate", [0, 1], ids=["overwrite-nan", "accumulate-onto-prefill"])
def test_altcorr_pyramid_backward_writes_every_element(L, oracle, accumulate):
    """accumulate = 0: the gradient buffers arrive as NaN and come back as the gradients.  accumulate = 1 is documented to add onto
    them (RAFT's 12 lookups share one set): a finite random prefill, and prefill + gradient is expected."""
    B, H, W, C, r, nl = (PYR[k] for k in ("B", "H", "W", "C", "r", "levels"))
    g, f1, f2s, coords = _pyramid_inputs()
    scale, n = 1.0 / math.sqrt(C), (2 * r + 1) ** 2
    go = torch.randn(B, nl * n, H, W, generator=g)
    pre = [torch.randn(t.shape, generator=g) if accumulate else None for t in (f1, *f2s)]
    f1d, f2d, cd, god = f1.to(DEV), [f.to(DEV) for f in f2s], coords.to(DEV), go.to(DEV)
    (b1, g1), lvl = _poisoned(f1.shape, prefill=pre[0]), [_poisoned(f.shape, prefill=q) for f, q in zip(f2s, pre[1:])]
    lv = _levels_struct(L, f2d, [t for _, t in lvl])
    ws = torch.zeros(int(L.lib().ufr_altcorr_pyramid_workspace_bytes(B, H, W, C, r, nl)), dtype=torch.uint8, device=DEV)
    _ok(L, L.lib().ufr_altcorr_pyramid_backward(L.ptr(f1d), ctypes.byref(lv), L.ptr(cd), L.ptr(god), L.ptr(g1), L.ptr(ws), B, H, W,
                                                C, r, scale, accumulate, L.stream()), "ufr_altcorr_pyramid_backward")
    want1 = torch.zeros_like(f1) if pre[0] is None else pre[0].clone()
    for i in range(nl):
        r1, r2, _ = oracle.altcorr_backward(f1, f2s[i], _level_coords(coords, i), (go[:, i * n:(i + 1) * n] * scale).unsqueeze(1).contiguous(), r)
        want1 += r1
        _written(lvl[i][0], lvl[i][1], r2 if pre[i + 1] is None else pre[i + 1] + r2, f"ufr_altcorr_pyramid_backward fmap2_grad level {i}",
                 rtol=1e-4, atol_scale=1e-5)
    _written(b1, g1, want1, "ufr_altcorr_pyramid_backward fmap1_grad", rtol=1e-4, atol_scale=5e-6)


def _lookup_inputs():
    B, H, W, C, nl = PYR["B"], PYR["H"], PYR["W"], PYR["C"], PYR["levels"]
    g, f1, f2s, coords = _pyramid_inputs()
    corr = torch.matmul(f1.view(B, H * W, C), f2s[0].view(B, H * W, C).transpose(1, 2)) / math.sqrt(C)
    pyr = [corr.view(B * H * W, 1, H, W)]
    for _ in range(nl - 1):
        pyr.append(F.avg_pool2d(pyr[-1], 2, stride=2))
    return g, [p.contiguous() for p in pyr], coords


def _pyramid_struct(L, vols, grads=None):
    pyr = L.Pyramid()
    pyr.num_levels = len(vols)
    for i, v in enumerate(vols):
        pyr.vol[i] = v.data_ptr()
        pyr.grad_vol[i] = grads[i].data_ptr() if grads is not None else None
        pyr.Hl[i], pyr.Wl[i] = int(v.shape[-2]), int(v.shape[-1])
    return pyr


def test_corr_lookup_forward_writes_every_element(L, oracle):
    B, H, W, r, nl = (PYR[k] for k in ("B", "H", "W", "r", "levels"))
    _, vols, coords = _lookup_inputs()
    vd, cd = [v.to(DEV) for v in vols], coords.to(DEV)
    pyr = _pyramid_struct(L, vd)
    buf, out = _poisoned((B, nl * (2 * r + 1) ** 2, H, W))
    _ok(L, L.lib().ufr_corr_lookup_forward(ctypes.byref(pyr), L.ptr(cd), L.ptr(out), B, H, W, r, L.stream()), "ufr_corr_lookup_forward")
    _written(buf, out, oracle.corr_lookup(vols, coords, r), "ufr_corr_lookup_forward", rtol=1e-5, atol_scale=1e-6)


def test_corr_lookup_backward_adds_onto_the_prefill(L):
    """Documented to accumulate (+=) into the gradient volumes: a finite random prefill, prefill + adjoint expected; the adjoint from
    float64 autograd through grid_sample, the reference's own formulation (test_lookup_matches_corrblock_golden_and_oracle)."""
    B, H, W, r, nl = (PYR[k] for k in ("B", "H", "W", "r", "levels"))
    g, vols, coords = _lookup_inputs()
    rd = 2 * r + 1
    go = torch.randn(B, nl * rd * rd, H, W, generator=g)
    pre = [torch.randn(v.shape, generator=g) for v in vols]
    vd, cd, god = [v.to(DEV) for v in vols], coords.to(DEV), go.to(DEV)
    grads = [_poisoned(v.shape, prefill=q) for v, q in zip(vols, pre)]
    pyr = _pyramid_struct(L, vd, [t for _, t in grads])
    _ok(L, L.lib().ufr_corr_lookup_backward(ctypes.byref(pyr), L.ptr(cd), L.ptr(god), B, H, W, r, L.stream()), "ufr_corr_lookup_backward")
    v64 = [v.double().requires_grad_(True) for v in vols]
    cperm, outs = coords.double().permute(0, 2, 3, 1), []
    d = torch.linspace(-r, r, rd, dtype=torch.float64)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1)
    for i, cv in enumerate(v64):
        cl = cperm.reshape(B * H * W, 1, 1, 2) / 2 ** i + delta.view(1, rd, rd, 2)
        hh, ww = cv.shape[-2:]
        grid = torch.stack([2 * cl[..., 0] / (ww - 1) - 1, 2 * cl[..., 1] / (hh - 1) - 1], -1)
        outs.append(F.grid_sample(cv, grid, align_corners=True).view(B, H, W, -1))
    torch.cat(outs, -1).permute(0, 3, 1, 2).backward(go.double())
    for i in range(nl):
        _written(grads[i][0], grads[i][1], pre[i].double() + v64[i].grad, f"ufr_corr_lookup_backward level {i}", rtol=1e-4, atol_scale=1e-5)


# ---------------------------------------------------------------------------- Resample2d / ChannelNorm
@pytest.mark.parametrize("lds_mode", ["1", "2", "0", "3"])      # the modes of test_resample2d_vs_oracle; csrc/warp_norm.hip::rs_lds_mode reads it per call
def test_resample2d_entries_write_every_element(L, oracle, monkeypatch, lds_mode):
    """ufr_resample2d_forward: mode 2 -> resample2d_fwd_lds, else resample2d_fwd.  ufr_resample2d_backward: modes 1, 2, 3 ->
    resample2d_bwd_lds, mode 0 -> resample2d_bwd (both behind a memset of grad_input1).  ufr_resample2d_backward_owner: the two
    owner-computes launches, whatever the mode."""
    monkeypatch.setenv("UFR_RESAMPLE_LDS", lds_mode)
    B, C, H, W = 2, 3, 17, 23
    g = torch.Generator().manual_seed(H)
    img = torch.rand(B, C, H, W, generator=g)
    flow = 4.0 * torch.randn(B, 2, H, W, generator=g)
    go = torch.randn(B, C, H, W, generator=g)
    imd, fd, god = img.to(DEV), flow.to(DEV), go.to(DEV)
    buf, out = _poisoned((B, C, H, W))
    _ok(L, L.lib().ufr_resample2d_forward(L.ptr(imd), L.ptr(fd), L.ptr(out), B, C, H, W, H, W, 1, 1, L.stream()), "ufr_resample2d_forward")
    ref = torch.zeros(B, C, H, W)
    oracle.resample2d_forward(img, flow, ref, 1, True)
    _written(buf, out, ref, "ufr_resample2d_forward", rtol=1e-6, atol_scale=1e-7)
    r1, r2 = torch.zeros(B, C, H, W), torch.zeros(B, 2, H, W)
    oracle.resample2d_backward(img, flow, go, r1, r2, 1, True)
    nbytes = int(L.lib().ufr_resample2d_backward_workspace_bytes(B, H, W))
    ws = torch.zeros((nbytes + 15) // 16 * 4, dtype=torch.int32, device=DEV)
    for entry in ("ufr_resample2d_backward", "ufr_resample2d_backward_owner"):
        (b1, g1), (b2, g2) = _poisoned((B, C, H, W)), _poisoned((B, 2, H, W))
        if entry == "ufr_resample2d_backward":
            rc = L.lib().ufr_resample2d_backward(L.ptr(imd), L.ptr(fd), L.ptr(god), L.ptr(g1), L.ptr(g2), B, C, H, W, H, W, 1, 1, L.stream())
        else:
            rc = L.lib().ufr_resample2d_backward_owner(L.ptr(imd), L.ptr(fd), L.ptr(god), L.ptr(g1), L.ptr(g2), L.ptr(ws), nbytes, B, C, H, W, L.stream())
        _ok(L, rc, entry)
        _written(b1, g1, r1, f"{entry} grad_input1", rtol=1e-4, atol_scale=1e-5)
        _written(b2, g2, r2, f"{entry} grad_input2", rtol=1e-5, atol_scale=1e-6)


def test_channelnorm_entries_write_every_element(L, oracle):
    B, C, H, W = 2, 3, 17, 23
    g = torch.Generator().manual_seed(W)
    x = torch.randn(B, C, H, W, generator=g)
    go = torch.randn(B, 1, H, W, generator=g)
    xd, god = x.to(DEV), go.to(DEV)
    buf, out = _poisoned((B, 1, H, W))
    _ok(L, L.lib().ufr_channelnorm_forward(L.ptr(xd), L.ptr(out), B, C, H, W, 2, L.stream()), "ufr_channelnorm_forward")
    ref = torch.zeros(B, 1, H, W)
    oracle.channelnorm_forward(x, ref)
    _written(buf, out, ref, "ufr_channelnorm_forward", rtol=1e-6, atol_scale=1e-7)
    bufg, gi = _poisoned((B, C, H, W))
    _ok(L, L.lib().ufr_channelnorm_backward(L.ptr(xd), L.ptr(out), L.ptr(god), L.ptr(gi), B, C, H, W, 2, L.stream()), "ufr_channelnorm_backward")
    rg = torch.zeros(B, C, H, W)
    oracle.channelnorm_backward(x, ref, go, rg)
    _written(bufg, gi, rg, "ufr_channelnorm_backward", rtol=1e-5, atol_scale=1e-6)


# ---------------------------------------------------------------------------- the torch spelling in float64 for the others
def test_convex_upsample_entries_write_every_element(L):
    """models/raft/raft.py:111-122 in float64; tolerances of test_convex_upsample_matches_torch."""
    N, H, W = 2, 5, 37
    g = torch.Generator().manual_seed(H * 100 + W)
    flow = 5 * torch.randn(N, 2, H, W, generator=g)
    mask = 3 * torch.randn(N, 576, H, W, generator=g)
    gu = torch.randn(N, 2, 8 * H, 8 * W, generator=g)
    f64, m64 = flow.double().requires_grad_(True), mask.double().requires_grad_(True)
    sm = torch.softmax(m64.view(N, 1, 9, 8, 8, H, W), dim=2)
    up = F.unfold(8 * f64, [3, 3], padding=1).view(N, 2, 9, 1, 1, H, W)
    want = torch.sum(sm * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(N, 2, 8 * H, 8 * W)
    gf_w, gm_w = torch.autograd.grad(want, (f64, m64), gu.double())
    fd, md, gud = flow.to(DEV), mask.to(DEV), gu.to(DEV)
    buf, out = _poisoned((N, 2, 8 * H, 8 * W))
    _ok(L, L.lib().ufr_convex_upsample_forward(L.ptr(fd), L.ptr(md), L.ptr(out), N, H, W, L.stream()), "ufr_convex_upsample_forward")
    _written(buf, out, want.detach(), "ufr_convex_upsample_forward", rtol=1e-5, atol_scale=1e-6)
    (bf, gf), (bm, gm) = _poisoned((N, 2, H, W)), _poisoned((N, 576, H, W))
    ws = torch.zeros(N * 2 * 9 * H * W, device=DEV)
    _ok(L, L.lib().ufr_convex_upsample_backward(L.ptr(fd), L.ptr(md), L.ptr(gud), L.ptr(gf), L.ptr(gm), L.ptr(ws), N, H, W, L.stream()),
        "ufr_convex_upsample_backward")
    _written(bf, gf, gf_w, "ufr_convex_upsample_backward grad_flow", rtol=1e-5, atol_scale=1e-5)
    _written(bm, gm, gm_w, "ufr_convex_upsample_backward grad_mask", rtol=1e-5, atol_scale=1e-5)


def test_pwc_warp_entries_write_every_element(L):
    """models/PWCNet.py:164-204 in float64 (flownets/pwcnet.py::_warp_torch); tolerances of test_pwc_warp_matches_torch_spelling.  The
    owner-computes adjoint writes grad_x without a zero fill; the scatter form zero-fills it first: both from NaN."""
    from understanding_flow_robustness_amd.flownets import pwcnet
    B, C, H, W, spread = 1, 3, 7, 9, 12.0
    g = torch.Generator().manual_seed(H * 10 + W)
    x = torch.randn(B, C, H, W, generator=g)
    flo = spread * torch.randn(B, 2, H, W, generator=g)
    go = torch.randn(B, C, H, W, generator=g)
    x64, f64 = x.double().requires_grad_(True), flo.double().requires_grad_(True)
    want = pwcnet._warp_torch(x64, f64)
    gx_w, gf_w = torch.autograd.grad(want, (x64, f64), go.double())
    xd, fd, god = x.to(DEV), flo.to(DEV), go.to(DEV)
    buf, out = _poisoned((B, C, H, W))
    _ok(L, L.lib().ufr_pwc_warp_forward(L.ptr(xd), L.ptr(fd), L.ptr(out), B, C, H, W, L.stream()), "ufr_pwc_warp_forward")
    _written(buf, out, want.detach(), "ufr_pwc_warp_forward", rtol=1e-5, atol_scale=3e-5)
    nbytes = int(L.lib().ufr_pwc_warp_backward_workspace_bytes(B, H, W))
    ws = torch.zeros((nbytes + 15) // 16 * 4, dtype=torch.int32, device=DEV)
    for entry in ("ufr_pwc_warp_backward_owner", "ufr_pwc_warp_backward"):
        (bx, gx), (bf, gf) = _poisoned((B, C, H, W)), _poisoned((B, 2, H, W))
        if entry == "ufr_pwc_warp_backward_owner":
            rc = L.lib().ufr_pwc_warp_backward_owner(L.ptr(xd), L.ptr(fd), L.ptr(god), L.ptr(gx), L.ptr(gf), L.ptr(ws), nbytes, B, C, H, W, L.stream())
        else:
            rc = L.lib().ufr_pwc_warp_backward(L.ptr(xd), L.ptr(fd), L.ptr(god), L.ptr(gx), L.ptr(gf), B, C, H, W, L.stream())
        _ok(L, rc, entry)
        _written(bx, gx, gx_w, f"{entry} grad_x", rtol=1e-5, atol_scale=3e-5)
        _written(bf, gf, gf_w, f"{entry} grad_flow", rtol=1e-4, atol_scale=3e-5)


@pytest.mark.parametrize("bilinear,divide", [(1, 0), (0, 0), (0, 1)], ids=["bilinear", "nearest", "nearest-divide"])
def test_flow_upscale4_entries_write_every_element(L, bilinear, divide):
    """F.interpolate in float64; test_flow_upscale4_matches_interpolate's bounds, max error <= 1e-6 (forward) / 2e-6 (adjoint) of max |ref|."""
    B, h, w = 2, 7, 5
    g = torch.Generator().manual_seed(h * w)
    flow = torch.randn(B, 2, h, w, generator=g)
    go = torch.randn(B, 2, 4 * h, 4 * w, generator=g)
    f64 = flow.double().requires_grad_(True)
    scaled = f64 / 20.0 if divide else f64 * 20.0
    want = F.interpolate(scaled, scale_factor=4, mode="bilinear", align_corners=False) if bilinear else F.interpolate(scaled, scale_factor=4, mode="nearest")
    (gw,) = torch.autograd.grad(want, f64, go.double())
    fd, god = flow.to(DEV), go.to(DEV)
    buf, out = _poisoned((B, 2, 4 * h, 4 * w))
    _ok(L, L.lib().ufr_flow_upscale4_forward(L.ptr(fd), L.ptr(out), B, h, w, bilinear, 20.0, divide, L.stream()), "ufr_flow_upscale4_forward")
    _written(buf, out, want.detach(), "ufr_flow_upscale4_forward", rtol=0.0, atol_scale=1e-6)
    bufg, gf = _poisoned((B, 2, h, w))
    _ok(L, L.lib().ufr_flow_upscale4_backward(L.ptr(god), L.ptr(gf), B, h, w, bilinear, 20.0, divide, L.stream()), "ufr_flow_upscale4_backward")
    _written(bufg, gf, gw, "ufr_flow_upscale4_backward", rtol=0.0, atol_scale=2e-6)
