"""GPU suite: `ufr_igemm_balanced` (csrc/igemm.hip) -- a ping-pong launch whose under-filled last round of 256 x 128 tiles is
re-cut into K slices -- against the two forms of `ufr_igemm` it is made of, bit for bit (torch.equal on the raw output buffers):

    rows of the full part  ==  ufr_igemm with splitk = 1
    rows of the tail       ==  ufr_igemm with splitk = S on the same descriptor   (S = the plan's slices)

so every output element is one an already gated form produces; everything outside the launch's rows keeps its sentinel.
`resident` is passed small so that grids of a few tiles have a tail round.

The shapes follow the plan's own rule (include/ufr_hip.h).  A 3 x 3 launch over 64 channels (18 K tiles) on 8 x 2 tiles and 12
resident workgroups gets two slices of 9 (18 // 8 = 2) and predicts 24 + 15 + 10 = 49 K steps against 48: the plan switches
ITSELF off there, so that shape is a refusal case here, and the cases that run the tail have 96 input channels (27 K tiles:
three slices of 9) and 160 (45 K tiles: four slices of 12, 12, 12 and 9)."""
import ctypes as C
from argparse import Namespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 5.0


def _mods():
    from understanding_flow_robustness_amd import _lib as L
    from understanding_flow_robustness_amd import igemm as ig
    return L, ig


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _row_pixels(B, Hr, Wr, Ho, Wo, x0_cells=None):
    """Output pixel of every row (b, y, x) of a stride-1 row grid whose columns start at x0_cells[b]."""
    b, y, x = torch.meshgrid(torch.arange(B), torch.arange(Hr), torch.arange(Wr), indexing="ij")
    if x0_cells is not None:
        x = x + torch.tensor(x0_cells).view(B, 1, 1)
    return ((b * Ho + y) * Wo + x).reshape(-1).to(DEV)


def _check(run, outputs, pixels, R, expect):
    """run(kwargs) -> fresh output buffers (each pre-filled with SENTINEL) after one launch.  The balanced launch against the
    composite of the plain forms; returns (plan, balanced outputs)."""
    L, ig = _mods()
    launch_out = run(dict(balance=True, resident=R))
    plan = launch_out["launch"].tail_plan
    assert plan is not None, "the plan is off: the test would compare the plain form with itself"
    assert (plan.full_row_tiles, plan.tail_row_tiles, plan.slices, plan.slice_ktiles) == expect
    M = pixels.numel()
    assert plan.tail_row0 + plan.tail_rows == M
    ws = torch.empty(plan.slices * M * launch_out["launch"].desc.Npad, device=DEV)
    one, sliced = run({}), run(dict(splitk=plan.slices, ws=ws))
    again = run(dict(balance=True, resident=R))
    torch.cuda.synchronize()
    tail_px = pixels[plan.tail_row0:]
    for name in outputs:
        got, want = launch_out[name], one[name].clone()
        want[..., tail_px, :] = sliced[name][..., tail_px, :]
        moved = int((one[name][..., tail_px, :] != sliced[name][..., tail_px, :]).sum())
        print(f"{name}: {moved} of {one[name][..., tail_px, :].numel()} tail values differ between splitk = 1 and splitk = {plan.slices}")
        assert torch.equal(got, want), f"{name}: {int((got != want).sum())} values differ from the composite"
        assert torch.equal(again[name], got), f"{name}: two runs differ"
        untouched = torch.ones(got.shape[-2], dtype=torch.bool, device=DEV)
        untouched[pixels] = False
        assert bool((got[..., untouched, :] == SENTINEL).all()), f"{name}: written outside the launch's rows"
    return plan, launch_out


def _forward_case(Cin, H, W, tap_major=False, B=2, Cout=256):
    L, ig = _mods()
    x, w, b = _rand(B, Cin, H, W, seed=1), _rand(Cout, Cin, 3, 3, seed=2, scale=0.05), _rand(Cout, seed=3)
    xin = ig.Planes(B, H, W, ig.pad32(Cin) // 32, DEV).load_nchw(x)
    keep = ig.K_ORDER
    try:
        ig.K_ORDER = 0 if tap_major else 1
        wi = ig.conv_forward_weights(w, 1, 1)
    finally:
        ig.K_ORDER = keep
    assert wi.k_order == (0 if tap_major else 1)

    def run(kw):
        out = ig.Planes(B, H, W, Cout // 32, DEV)
        out.t.fill_(SENTINEL)
        launch = ig.make_launch(wi, xin, 0, (H, W), (H, W), out_planes=out, bias=b, variant=6, **kw)
        launch()
        return dict(launch=launch, planes=out.t, buf=out)

    return run, (x, w, b), _row_pixels(B, H, W, H, W)


@pytest.mark.parametrize("tap_major", [False, True], ids=["chunk-major", "tap-major"])
def test_forward_rows_equal_the_two_gated_forms(tap_major):
    """3 x 3, 2 x 96 -> 256 channels on 24 x 40: 1920 rows = 8 row tiles (the last half full) x 2 column tiles, 27 K tiles, 12
    resident workgroups: 6 whole row tiles, 2 tail row tiles in 3 slices of 9.  Both orders of the K tiles."""
    run, (x, w, b), pixels = _forward_case(96, 24, 40, tap_major)
    plan, got = _check(run, ["planes"], pixels, 12, (6, 2, 3, 9))
    assert (plan.tail_row0, plan.tail_rows, plan.workgroups) == (1536, 384, 12 + 4 * 3)
    want = F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), 1, 1), 0.1)
    err = float((got["buf"].to_nchw(256).double() - want).abs().max()) / float(want.abs().max())
    assert err <= 1e-5, f"{err:.2e} of max |result|"


def test_uneven_slices():
    """160 input channels (45 K tiles) on 2 x 30 x 40 = 2400 rows (10 row tiles, the last 96 rows) and 16 resident workgroups:
    8 whole row tiles, 2 tail row tiles in 4 slices of 12, 12, 12 and 9 K tiles."""
    run, _, pixels = _forward_case(160, 30, 40)
    plan, _ = _check(run, ["planes"], pixels, 16, (8, 2, 4, 12))
    assert plan.ktiles == 45 and plan.tail_rows == 352


@pytest.mark.parametrize("Cin,R,why", [(96, 8, "16 tiles are two whole rounds of 8"), (64, 12, "two slices of 9 do not pay for the reduce launch"),
                                       (96, 16, "one whole round"), (96, 17, "no round is full")])
def test_a_plan_that_is_off_is_ufr_igemm(Cin, R, why):
    """The balanced ENTRY with a plan that is off and no workspace at all: the plain launch, bit for bit (it cannot have
    launched a reduce: there are no slabs)."""
    L, ig = _mods()
    run, _, _ = _forward_case(Cin, 24, 40)
    one = run({})
    d = one["launch"].desc
    plan = ig.tail_plan(d, R)
    assert plan.on == 0, why
    out = ig.Planes(2, 24, 40, 8, DEV)
    out.t.fill_(SENTINEL)
    d2 = type(d).from_buffer_copy(d)
    d2.out_planes = out.t.data_ptr()
    L.check(L.lib().ufr_igemm_balanced(C.byref(d2), R, None, 0, L.stream()), "igemm (balanced)")
    torch.cuda.synchronize()
    assert torch.equal(out.t, one["planes"])


def test_a_small_workspace_is_refused_before_any_launch():
    L, ig = _mods()
    run, _, _ = _forward_case(96, 24, 40)
    got = run(dict(balance=True, resident=12))
    launch = got["launch"]
    before = got["planes"].clone()
    ws = torch.empty(launch.tail_plan.ws_floats - 1, device=DEV)
    assert L.lib().ufr_igemm_balanced(C.byref(launch.desc), 12, L.ptr(ws), ws.numel(), L.stream()) == -1
    assert b"workspace" in L.lib().ufr_last_error()
    torch.cuda.synchronize()
    assert torch.equal(got["planes"], before)


# ---- conv3_1's data gradient in small: 200 columns (Npad = 256), mask, planes for chunk 0 + fp32 from chunk 1 on, a row band inside
# ---- an input band with per-pair origins (cells), one pair touching each frame edge
_B3, _H3, _W3, _RW, _IW = 3, 10, 64, 32, 40
_ROW_X0 = [[0, 32, 13], [32, 0, 21]]          # row-band origins before / after the change on the device
_IN_X0 = [[0, 24, 10], [24, 0, 17]]           # input-band origins: [x0, x0 + 40) holds the row band


def _band_gradient_case():
    L, ig = _mods()
    B, H, W = _B3, _H3, _W3
    Cin, Cout = 200, 256                                              # Conv2d(200, 256, 3, 1, 1): its data gradient has 200 columns
    w, gy, act = _rand(Cout, Cin, 3, 3, seed=2, scale=0.05), _rand(B, Cout, H, W, seed=4), _rand(B, Cin, H, W, seed=6)
    gyp = ig.Planes(B, H, W, Cout // 32, DEV).load_nchw(gy)
    actp = ig.Planes(B, H, W, ig.pad32(Cin) // 32, DEV).load_nchw(act)
    wi = ig.conv_backward_weights(w, 1, 1)
    assert (wi.N, wi.Npad, wi.KC) == (200, 256, 8)
    origins = torch.zeros(B, 4, dtype=torch.int32, device=DEV)

    def set_origins(k):
        origins[:, 1] = torch.tensor(_IN_X0[k], dtype=torch.int32) * 8
        origins[:, 2] = torch.tensor(_ROW_X0[k], dtype=torch.int32) * 8

    bufs = lambda: (ig.Planes(B, H, W, ig.pad32(Cin) // 32, DEV), ig.GradSum(B, H, W, ig.pad32(Cin) // 32, DEV))

    def make(kw, outp, outf):
        return ig.make_launch(wi, gyp, 0, (H, _RW), (H, W), out_planes=outp, out_f32=outf, mask=actp, planes_chunks=1, f32_first_chunk=1,
                              row_band=(origins[:, 2], 4, 8), in_band=(origins[:, 1], 4, 8, _IW), variant=6, **kw)

    def run(kw):
        outp, outf = bufs()
        outp.t.fill_(SENTINEL); outf.t.fill_(SENTINEL)
        launch = make(kw, outp, outf)
        launch()
        return dict(launch=launch, planes=outp.t, f32=outf.t)

    return run, make, bufs, set_origins, (w, gy, act)


def test_band_gradient_with_conv3_1s_epilogue():
    """960 rows = 4 row tiles x 2 column tiles, 72 K tiles, 6 resident workgroups: 3 whole row tiles, 1 tail row tile (the last
    192 rows) in 3 slices of 24 -- the headline's slicing.  Chunk 0 leaves as planes, chunks 1 .. 6 as fp32."""
    run, _, _, set_origins, (w, gy, act) = _band_gradient_case()
    set_origins(0)
    pixels = _row_pixels(_B3, _H3, _RW, _H3, _W3, _ROW_X0[0])
    plan, got = _check(run, ["planes", "f32"], pixels, 6, (3, 1, 3, 24))
    assert (plan.tail_row0, plan.tail_rows) == (768, 192)
    assert bool((got["planes"][:, 1:] == SENTINEL).all()) and bool((got["f32"][0] == SENTINEL).all())     # planes_chunks / f32_first_chunk
    # against torch in float64: gy outside the input band counts as zero, the result exists on the row band
    x0 = torch.zeros(_B3, 200, _H3, _W3, device=DEV, dtype=torch.float64, requires_grad=True)
    gm = torch.zeros_like(gy, dtype=torch.float64)
    for b, o in enumerate(_IN_X0[0]):
        gm[b, :, :, o:o + _IW] = gy[b, :, :, o:o + _IW].double()
    (gx,) = torch.autograd.grad(F.conv2d(x0, w.double(), None, 1, 1), x0, gm)
    want = gx * torch.where(act > 0, 1.0, 0.1).double()
    f32 = got["f32"].view(7, _B3, _H3, _W3, 32).permute(1, 0, 4, 2, 3).reshape(_B3, 224, _H3, _W3)[:, :200]
    for b, o in enumerate(_ROW_X0[0]):
        err = float((f32[b, 32:, :, o:o + _RW].double() - want[b, 32:, :, o:o + _RW]).abs().max()) / float(want.abs().max())
        assert err <= 1e-5, f"pair {b}: {err:.2e} of max |gradient|"


def test_captured_graph_follows_the_band_origins():
    """One captured graph of the balanced launch, replayed after the band origins change ON THE DEVICE: the replay equals the
    plain forms launched with the new origins."""
    L, ig = _mods()
    run, make, bufs, set_origins, _ = _band_gradient_case()
    set_origins(0)
    outp, outf = bufs()
    launch = make(dict(balance=True, resident=6), outp, outf)
    plan = launch.tail_plan
    assert plan is not None and plan.slices == 3
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                                      # (first call: the kernel's LDS limit is raised outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with L.graph_capture(graph):          # (no cyclic collection inside a capture: _lib.graph_capture)
        launch()
    ws = torch.empty(plan.slices * _B3 * _H3 * _RW * 256, device=DEV)
    for k in (0, 1, 0):
        set_origins(k)
        outp.t.fill_(SENTINEL); outf.t.fill_(SENTINEL)
        graph.replay()
        one, sliced = run({}), run(dict(splitk=plan.slices, ws=ws))
        torch.cuda.synchronize()
        tail_px = _row_pixels(_B3, _H3, _RW, _H3, _W3, _ROW_X0[k])[plan.tail_row0:]
        for name, got in (("planes", outp.t), ("f32", outf.t)):
            want = one[name].clone()
            want[..., tail_px, :] = sliced[name][..., tail_px, :]
            assert torch.equal(got, want), f"origins {k}, {name}: {int((got != want).sum())} values differ"


def test_attack_step_with_the_tail_split_against_the_step_without_and_the_oracle():
    """2 pairs at 128 x 768 behind a 20-pixel disc (the shapes of tests/test_attack_glue_gpu.py and test_corr_changed_gpu.py), eager,
    `tail_resident` chosen so that conv3_1's data gradient on the correlation-reach band has ONE tail row tile: `tail_split` on
    against off after three iterations, and one iteration against the CPU oracle's `patch_attack_placed` -- both at 1e-4 of the
    update, the gate of the step tests of tests/test_flownetc_gpu.py.  (On against off is not bit-equal: the tail rows' sums are
    reordered.)"""
    from oracle import flow_oracle as fo
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    from understanding_flow_robustness_amd.patch_attack import PatchAttackStep
    Bn, H, W, S = 2, 128, 768, 20
    net = fetch_model(Namespace(flownet="FlowNetC"), synthetic_seed=0).to(DEV)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    for p in net.parameters():
        p.requires_grad_(False)
    g = torch.Generator().manual_seed(29)
    tgt, ref = torch.rand(Bn, 3, H, W, generator=g), torch.rand(Bn, 3, H, W, generator=g)
    target = torch.randn(Bn, 2, H, W, generator=g)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    disc = (((yy - 9.5) ** 2 + (xx - 9.5) ** 2) <= 10.0 ** 2).float().expand(1, 3, S, S).contiguous()
    patch0 = torch.rand(1, 3, S, S, generator=g)
    origins = [(0, 300), (50, 400)]

    def run(lr, iterations, **kw):
        args = Namespace(flownet="FlowNetC", l2=False, alpha=0.0, lr=lr, max_count=iterations)
        step = PatchAttackStep(net, args, Bn, H, W, device=DEV, patch_hw=(S, S), use_graph=False, **kw)
        step.load(tgt.to(DEV), ref.to(DEV), patch0.to(DEV), disc.to(DEV), patch0.to(DEV), target.to(DEV), origins=origins)
        n, loss = step.run(iterations)
        assert n == iterations and step.eng is not None and step.band.width and step.band.corr_width
        return step, step.patch.detach().cpu().clone()

    probe, p1 = run(1.0, 1)
    assert probe.eng.tail_launches() == []                            # 256 resident workgroups: no launch of this size has a full round
    lr = 0.25 / float(((p1 - patch0) * disc).abs().max())
    row_tiles = -(-(Bn * (H // 8) * (probe.band.corr_width // 8)) // 256)
    assert row_tiles >= 3
    R = 4 * (row_tiles - 1)                                           # 473 -> 512 columns: 4 column tiles; all row tiles but the last are whole rounds
    on, p_on = run(lr, 3, tail_resident=R)
    tails = {(tag, name): plan for tag, name, plan in on.eng.tail_launches()}
    print("launches with a re-cut last round:", {k: (p.full_row_tiles, p.tail_row_tiles, p.slices, p.slice_ktiles) for k, p in tails.items()})
    plan = tails[("band", "conv3_1")]
    assert (plan.full_row_tiles, plan.tail_row_tiles, plan.slices) == (row_tiles - 1, 1, min(R // 4, 8))
    _, p_off = run(lr, 3, tail_resident=R, tail_split=False)
    upd = float(((p_off - patch0) * disc).abs().max())
    diff = float((p_on - p_off).abs().max())
    print(f"tail_split on against off after 3 iterations: {diff:.3e} (update {upd:.3e})")
    assert upd > 0.1 and diff <= 1e-4 * max(upd, 1.0)
    # one iteration against the oracle
    _, g1 = run(lr, 1, tail_resident=R)
    cpu_patch = patch0.clone()
    fo.patch_attack_placed(lambda a, b: fo.flownetc_forward(sd, a, b), tgt, ref, cpu_patch, disc, origins, target, lr=lr, max_count=1)
    upd1 = float((cpu_patch - patch0).abs().max())
    err = float((g1 - cpu_patch).abs().max())
    print(f"one iteration against the oracle: {err:.3e} (update {upd1:.3e})")
    assert upd1 > 0.05 and err <= 1e-4 * max(upd1, 1.0)
