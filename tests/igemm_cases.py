"""The launches whose output BYTES pin csrc/igemm.hip's tile kernels (tests/test_igemm_digests_gpu.py against
tests/golden/igemm_form_digests.json, written by tests/golden/make_igemm_digests.py on the commit before the tile kernels moved onto
one tile walk / cell geometry / activation stager).  The smallest shapes that reach each shared piece:

    fwd_70_128      3 x 3, (2, 70, 128, 13, 29): 128 columns (ping-pong, tap reuse, pipelined, 64 x 128), M = 754 = three ragged
                    256-row tiles, width 29 >= 22 (tap reuse) with row ends inside a tile; also with 3 and 1 products
    fwd_117_32      (3, 117, 32, 13, 29): 64-column tiles, the 256 x 64 tap-reuse form
    fwd_k5s2        (1, 64, 128, 20, 36), k = 5, s = 2, p = 2: 25 taps, input stride 2, width 18 < 22 (form 7 falls through)
    fwd_6_64        (1, 6, 64, 40, 72): the direct 3 x 3 form, and its fall-through under the other variants
    s2_dgrad        stride-2 data gradient, (k, p, S) = (3, 1, 4): four phases, per-phase slices (zoff / sk), the reduce launch
    conv6_1_tickets 512 -> 512 on 2 x 6 x 20 with tickets: the fused split-K reduction's tile_id
    band            per-sample row band (row_x0), then the same with an input band (in_x0)
    tail_uneven     the re-cut last round (tail_tile, tl_per_k): 160 -> 256 on 2 x 30 x 40, 16 resident workgroups

each under both orders of the K tiles (`igemm.K_ORDER` when the weights are packed) and the six kernel variants.  Inputs come from
CPU generators; `Planes.load_nchw` runs csrc/plane_layout.hip, so the digests also pin the three-plane split.  A digest covers the
whole output buffer -- the sentinel around the written chunks included -- and the increment of `igemm.variant_fallbacks()`."""
import hashlib

import torch

DEV = "cuda:0"
VARIANTS = (2, 4, 5, 6, 7, 8)
K_ORDERS = (1, 0)
SENTINEL = 7.0


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _packed(ig, k_order, build, *a):
    keep = ig.K_ORDER
    try:
        ig.K_ORDER = k_order
        wi = build(*a)
    finally:
        ig.K_ORDER = keep
    assert wi.k_order == k_order
    return wi


def _forward(B, Cin, Cout, H, W, k=3, s=1, p=1, **launch_kw):
    def setup(ig, k_order):
        x, w, b = _rand(B, Cin, H, W, seed=1), _rand(Cout, Cin, k, k, seed=2, scale=0.05), _rand(Cout, seed=3)
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        xin = ig.Planes(B, H, W, ig.pad32(Cin) // 32, DEV).load_nchw(x)
        wi = _packed(ig, k_order, ig.conv_forward_weights, w, s, p)

        def run(variant):
            out = ig.Planes(B, Ho, Wo, 1 + ig.pad32(Cout) // 32 + 1, DEV)        # the output lands at chunk 1 of a wider buffer
            out.t.fill_(SENTINEL)
            ig.make_launch(wi, xin, 0, (Ho, Wo), (Ho, Wo), out_planes=out, out_chunk0=1, bias=b, variant=variant, **launch_kw)()
            return [out.t]
        return run
    return setup


def _s2_dgrad(ig, k_order):
    B, Cin, Cout, H, W, S = 2, 64, 96, 24, 40, 4
    Ho, Wo = H // 2, W // 2
    w, gy = _rand(Cout, Cin, 3, 3, seed=2, scale=0.05), _rand(B, Cout, Ho, Wo, seed=4)
    gyp = ig.Planes(B, Ho, Wo, ig.pad32(Cout) // 32, DEV).load_nchw(gy)
    wi = _packed(ig, k_order, ig.conv_backward_weights, w, 2, 1)
    ws = torch.empty(len(wi.phases) * S * B * Ho * Wo * wi.Npad, dtype=torch.float32, device=DEV)

    def run(variant):
        out = ig.GradSum(B, H, W, ig.pad32(Cin) // 32 + 1, DEV)
        out.t.fill_(SENTINEL)
        ig.make_launch(wi, gyp, 0, (Ho, Wo), (H, W), out_f32=out, splitk=S, ws=ws, fuse_reduce=False, variant=variant)()
        return [out.t]
    return run


def _conv6_1_tickets(ig, k_order):
    B, Cn, H, W = 2, 512, 6, 20
    x, w, b = _rand(B, Cn, H, W, seed=1), _rand(Cn, Cn, 3, 3, seed=2, scale=0.02), _rand(Cn, seed=3)
    xin = ig.Planes(B, H, W, Cn // 32, DEV).load_nchw(x)
    wi = _packed(ig, k_order, ig.conv_forward_weights, w, 1, 1)
    S = max(4, ig.splitk_for(B * H * W, wi.Npad, 9 * wi.KC))
    ws = torch.empty(S * B * H * W * wi.Npad, device=DEV)

    def run(variant):
        out = ig.Planes(B, H, W, Cn // 32 + 1, DEV)
        out.t.fill_(SENTINEL)
        launch = ig.make_launch(wi, xin, 0, (H, W), (H, W), out_planes=out, bias=b, splitk=S, ws=ws, fuse_reduce=True, variant=variant)
        assert launch.desc.tickets
        launch()
        return [out.t]
    return run


def _band(ig, k_order):
    B, Cin, Cout, H, W, bw = 3, 64, 96, 10, 48, 16
    x, w, b = _rand(B, Cin, H, W, seed=1), _rand(Cout, Cin, 3, 3, seed=2, scale=0.05), _rand(Cout, seed=3)
    origins = torch.tensor([[0, 8 * 0, 0, 0], [0, 8 * 32, 0, 0], [0, 8 * 17, 0, 0]], dtype=torch.int32, device=DEV)  # pixels, cell = 8
    xin = ig.Planes(B, H, W, 2, DEV).load_nchw(x)
    wi = _packed(ig, k_order, ig.conv_forward_weights, w, 1, 1)
    band = (origins[:, 1], 4, 8)

    def run(variant):
        outs = []
        for kw in (dict(row_band=band), dict(row_band=band, in_band=band + (bw,))):
            out = ig.Planes(B, H, W, 3, DEV)
            out.t.fill_(SENTINEL)
            ig.make_launch(wi, xin, 0, (H, bw), (H, W), out_planes=out, bias=b, variant=variant, **kw)()
            outs.append(out.t)
        return outs
    return run


def _tail_uneven(ig, k_order):
    B, Cin, Cout, H, W, R = 2, 160, 256, 30, 40, 16
    x, w, b = _rand(B, Cin, H, W, seed=1), _rand(Cout, Cin, 3, 3, seed=2, scale=0.05), _rand(Cout, seed=3)
    xin = ig.Planes(B, H, W, ig.pad32(Cin) // 32, DEV).load_nchw(x)
    wi = _packed(ig, k_order, ig.conv_forward_weights, w, 1, 1)

    def run(variant):
        out = ig.Planes(B, H, W, Cout // 32 + 1, DEV)
        out.t.fill_(SENTINEL)
        launch = ig.make_launch(wi, xin, 0, (H, W), (H, W), out_planes=out, bias=b, variant=variant, balance=True, resident=R)
        if variant == 6:                                    # (the plan is for the ping-pong form; the others run the plain launch)
            plan = launch.tail_plan
            assert plan is not None and (plan.full_row_tiles, plan.tail_row_tiles, plan.slices, plan.slice_ktiles) == (8, 2, 4, 12)
        launch()
        return [out.t]
    return run


CASES = {
    "fwd_70_128": _forward(2, 70, 128, 13, 29),
    "fwd_117_32": _forward(3, 117, 32, 13, 29),
    "fwd_k5s2": _forward(1, 64, 128, 20, 36, 5, 2, 2),
    "fwd_6_64": _forward(1, 6, 64, 40, 72),
    "s2_dgrad": _s2_dgrad,
    "conv6_1_tickets": _conv6_1_tickets,
    "band": _band,
    "fwd_70_128_products3": _forward(2, 70, 128, 13, 29, products=3),
    "fwd_70_128_products1": _forward(2, 70, 128, 13, 29, products=1),
    "tail_uneven": _tail_uneven,
}


def digests():
    """{"<case>/k_order=<o>/variant=<v>": {"sha256": of the output buffers' bytes, "fallbacks": variant_fallbacks() increment}}"""
    from understanding_flow_robustness_amd import igemm as ig
    got = {}
    for name, setup in CASES.items():
        for k_order in K_ORDERS:
            run = setup(ig, k_order)
            for variant in VARIANTS:
                before = ig.variant_fallbacks()
                outs = run(variant)
                torch.cuda.synchronize()
                h = hashlib.sha256()
                for t in outs:
                    h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
                got[f"{name}/k_order={k_order}/variant={variant}"] = {"sha256": h.hexdigest(), "fallbacks": ig.variant_fallbacks() - before}
    return got
