"""GPU suite: `ufr_flow_head_planes_backward_regions` (csrc/engine_small.hip) -- predict_flow's data gradient over two chunk
groups, the first on a column band or a window rectangle only -- against the unrestricted `flow_head_planes_bwd` on the same
inputs: bit-identical inside the region, nothing written outside it, the trailing group and its finalised planes unchanged."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W, CHUNKS, HEAD = 2, 6, 40, 5, 3                   # groups [0, 3) and [3, 5); 480 pixels: more than one 64-pixel block
FIN = (3, 2)                                             # the finalised segment = the trailing group
SLOPE = 0.1


@pytest.fixture(scope="module")
def case():
    """Inputs, and the unrestricted kernel's result from the same base (the sentinel) for accumulate 0 / 1, computed once."""
    from understanding_flow_robustness_amd import _lib as L
    from understanding_flow_robustness_amd import igemm as ig
    from understanding_flow_robustness_amd.flownetc_engine import _pack_flow_head
    g = torch.Generator().manual_seed(17)
    gy = torch.randn(B, 2, H, W, generator=g).to(DEV)
    wpk = _pack_flow_head((torch.randn(2, CHUNKS * 32, 3, 3, generator=g) * 0.1).to(DEV))
    mask = ig.Planes(B, H, W, CHUNKS, DEV).load_nchw(torch.randn(B, CHUNKS * 32, H, W, generator=g).to(DEV))
    base = torch.randn(CHUNKS, B * H * W, 32, generator=g).to(DEV)                   # the sentinel: every element its own value
    c = dict(gy=gy, wpk=wpk, mask=mask, base=base, full={})
    for acc in (0, 1):
        G, out = fresh(c)
        L.check(L.lib().ufr_flow_head_planes_backward_finalize(L.ptr(gy), L.ptr(wpk), CHUNKS, L.ptr(G.t), CHUNKS, 0, CHUNKS, B, H, W, acc,
                                                               L.ptr(mask.t), L.ptr(out.t), out.plane_stride, FIN[0], FIN[1], SLOPE,
                                                               L.stream()))
        c["full"][acc] = (G.t.clone(), out.t.clone())
    return c


def fresh(c):
    from understanding_flow_robustness_amd import igemm as ig
    G = ig.GradSum(B, H, W, CHUNKS, DEV)
    G.t.copy_(c["base"])
    out = ig.Planes(B, H, W, CHUNKS, DEV)
    out.t.fill_(-7.0)
    return G, out


def regions(c, acc, kind, origin, stride, div, rh, rw, margin, head_out=None, finalize=True):
    from understanding_flow_robustness_amd import _lib as L
    G, out = fresh(c)
    L.check(L.lib().ufr_flow_head_planes_backward_regions(
        L.ptr(c["gy"]), L.ptr(c["wpk"]), CHUNKS, L.ptr(G.t), CHUNKS, 0, CHUNKS, B, H, W, acc, HEAD, kind, L.ptr(origin), stride, div,
        rh, rw, margin, L.ptr(head_out.t) if head_out is not None else None, head_out.B if head_out is not None else 0,
        L.ptr(c["mask"].t) if finalize else None, L.ptr(out.t) if finalize else None, out.plane_stride if finalize else 0,
        FIN[0] if finalize else 0, FIN[1] if finalize else 0, SLOPE, L.stream()))
    return G.t, out.t


def check(c, acc, got, inside):
    """`inside` [B, H, W] bool: the head group's region."""
    G, out = got
    G_full, out_full = c["full"][acc]
    v = lambda t: t.view(CHUNKS, B, H, W, 32)
    m = inside.to(DEV)[None, :, :, :, None].expand(HEAD, B, H, W, 32)
    assert torch.equal(v(G)[:HEAD][m], v(G_full)[:HEAD][m])                          # inside: the unrestricted kernel's values
    assert torch.equal(v(G)[:HEAD][~m], v(c["base"])[:HEAD][~m])                     # outside: the sentinel is intact
    assert torch.equal(G[HEAD:], G_full[HEAD:])                                      # the trailing group, everywhere
    assert torch.equal(out, out_full)                                                # its finalised planes (and nothing else written)
    assert not torch.equal(G_full[:HEAD], c["base"][:HEAD])


def window_region(win_px, ls, rh, rw, margin):
    """(inside [B, H, W], per-pair clamped origin, rim [B, rh, rw]) by ufr_window_gather's rule."""
    inside = torch.zeros(B, H, W, dtype=torch.bool)
    rim = torch.zeros(B, rh, rw, dtype=torch.bool)
    at = []
    for b, (y, x) in enumerate(win_px):
        y0, x0 = min(max(int(y / ls), 0), H - rh), min(max(int(x / ls), 0), W - rw)      # C division truncates towards zero
        for i in range(rh):
            for j in range(rw):
                rim[b, i, j] = ((i < margin and y0 > 0) or (i >= rh - margin and y0 + rh < H) or (j < margin and x0 > 0)
                                or (j >= rw - margin and x0 + rw < W))
                inside[b, y0 + i, x0 + j] = not rim[b, i, j]
        at.append((y0, x0))
    return inside, at, rim


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("rw", [13, 40])
def test_band_region_equals_the_unrestricted_kernel_inside_and_writes_nothing_outside(case, acc, rw):
    """One pair's band at column 0, the other's flush with the right edge; 6 x 13 cells per pair = 156 pixels, no multiple of
    the block's 64 (and the whole frame as a band: every pixel inside)."""
    from understanding_flow_robustness_amd import _lib as L
    table = torch.zeros(B, 8, dtype=torch.int32)
    table[0, 1], table[1, 1] = 0, (W - rw) * 8                                       # pixels at level stride 8, as the engine's band
    table = table.to(DEV)
    inside = torch.zeros(B, H, W, dtype=torch.bool)
    inside[0, :, :rw] = True
    inside[1, :, W - rw:] = True
    check(case, acc, regions(case, acc, L.UFR_PF_REGION_BAND, table[:, 1], 8, 8, H, rw, 0), inside)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("margin", [0, 1])
def test_window_region_in_place(case, acc, margin):
    """A 4 x 10 window per pair at level stride 4: one origin left and above the frame (clamped into the corner: its rim lies on the
    two interior edges only), one with rims above and below and flush with the right edge."""
    from understanding_flow_robustness_amd import _lib as L
    win_px = [(-8, -12), (4, 30 * 4)]
    win = torch.zeros(B, 8, dtype=torch.int32)
    for b, (y, x) in enumerate(win_px):
        win[b, 0], win[b, 1] = y, x
    inside, at, _ = window_region(win_px, 4, 4, 10, margin)
    assert at == [(0, 0), (1, 30)] and int(inside.sum()) == (80 if margin == 0 else 3 * 9 + 2 * 9)
    check(case, acc, regions(case, acc, L.UFR_PF_REGION_WINDOW, win.to(DEV), 8, 4, 4, 10, margin), inside)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("margin", [0, 1])
def test_window_region_written_as_a_window_tensor_equals_the_gather_of_the_unrestricted_result(case, acc, margin):
    """`head_out`: the head group leaves as [3][3 images * 4 * 10][32] with the rim zeroed -- `ufr_window_gather_chunks` of what
    `flow_head_planes_bwd` writes -- and the gradient sum's head chunks are not touched (`accumulate` concerns the sum only)."""
    from understanding_flow_robustness_amd import _lib as L
    from understanding_flow_robustness_amd import igemm as ig
    rh, rw, ls = 4, 10, 4
    win_px = [(-8, -12), (4, 30 * 4)]
    win = torch.zeros(B, 8, dtype=torch.int32)
    for b, (y, x) in enumerate(win_px):
        win[b, 0], win[b, 1] = y, x
    win = win.to(DEV)
    direct, gathered = ig.GradSum(B + 1, rh, rw, HEAD, DEV), ig.GradSum(B + 1, rh, rw, HEAD, DEV)
    direct.t.fill_(3.25)
    gathered.t.fill_(3.25)
    G, out = regions(case, acc, L.UFR_PF_REGION_WINDOW, win, 8, ls, rh, rw, margin, head_out=direct)
    plain = ig.GradSum(B, H, W, CHUNKS, DEV)                                         # the unrestricted kernel, written (not added)
    L.check(L.lib().ufr_flow_head_planes_backward(L.ptr(case["gy"]), L.ptr(case["wpk"]), CHUNKS, L.ptr(plain.t), CHUNKS, 0, CHUNKS, B, H, W, 0,
                                                  L.stream()))
    L.check(L.lib().ufr_window_gather_chunks(L.ptr(plain.t), L.ptr(gathered.t), L.ptr(win), B, B, B + 1, HEAD, H, W, rh, rw, ls, margin,
                                             L.stream()))
    assert torch.equal(direct.t, gathered.t)
    v = direct.t.view(HEAD, B + 1, rh, rw, 32)
    assert bool((v[:, B] == 3.25).all()) and bool(v[:, :B].abs().sum() > 0)          # the image behind the range is not touched
    _, _, rim = window_region(win_px, ls, rh, rw, margin)
    assert bool((v[:, :B][rim.to(DEV)[None, :, :, :, None].expand(HEAD, B, rh, rw, 32)] == 0).all())
    G_full, out_full = case["full"][acc]
    assert torch.equal(G[:HEAD], case["base"][:HEAD])                                # G's head chunks: neither read nor written
    assert torch.equal(G[HEAD:], G_full[HEAD:]) and torch.equal(out, out_full)


def test_without_finalisation_and_refusals(case):
    from understanding_flow_robustness_amd import _lib as L
    lib = L.lib()
    table = torch.zeros(B, 8, dtype=torch.int32, device=DEV)
    G, out = regions(case, 0, L.UFR_PF_REGION_BAND, table[:, 1], 8, 8, H, 13, 0, finalize=False)
    assert torch.equal(G[HEAD:], case["full"][0][0][HEAD:]) and bool((out == -7.0).all())
    p, o = L.ptr(case["gy"]), L.ptr(table)
    common = lambda head, kind, rh, rw, margin, fin0: lib.ufr_flow_head_planes_backward_regions(
        p, p, CHUNKS, p, CHUNKS, 0, CHUNKS, B, H, W, 0, head, kind, o, 8, 8, rh, rw, margin, None, 0, p, p, CHUNKS * B * H * W * 32, fin0, 1, SLOPE,
        L.stream())
    refused = [common(0, 1, H, 13, 0, 3), common(6, 1, H, 13, 0, 3),                 # the head group: 1 .. chunks
               common(3, 3, H, 13, 0, 3),                                             # no such region kind
               common(3, 1, H, W + 1, 0, 3), common(3, 1, H - 1, 13, 0, 3),          # a band wider than the frame / not every row
               common(3, 2, 4, 10, 3, 3),                                             # rims that meet
               common(3, 1, H, 13, 0, 2)]                                             # finalisation inside the restricted group
    assert refused == [-1] * len(refused), refused
