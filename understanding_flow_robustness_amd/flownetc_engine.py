"""Native FlowNetC head: everything of models/FlowNetC.py:121-197 behind conv1-3 -- correlation, conv_redir, conv3_1 ...
conv6_1, the coarse-to-fine refinement -- forward AND data gradient as an explicit schedule of hand-written gfx950
kernels, with no torch operator between the siamese features and flow2.

    convolutions / deconvolutions   csrc/igemm.hip: implicit GEMMs on bf16 split planes (float32-accurate, six products)
    predict_flow*, upsampled_flow*  csrc/engine_small.hip (HBM-bound passes over the concatenation buffers)
    correlation                     csrc/correlation*.hip (unchanged), cost volume converted once into conv3_1's input

Activations stay in the chunk-major plane layout between layers (igemm.Planes); a `torch.cat` of the reference
(FlowNetC.py:142, :167, :172, :177, :182) is a chunk offset into one buffer:

    in31 = [conv_redir 32 | corr 441]            15 chunks @ 1/8     cat3 = [conv3_1 256 | deconv3 128 | flow4_up 2]  13 chunks @ 1/8
    cat4 = [conv4_1 512 | deconv4 256 | up 2]    25 chunks @ 1/16    cat5 = [conv5_1 512 | deconv5 512 | up 2]        33 chunks @ 1/32
    cat2 = [conv2 128 | deconv2 64 | up 2]        7 chunks @ 1/4

The backward pass is the reverse schedule; a gradient with several consumers is summed in fp32 (igemm.GradSum) and the last
contributing GEMM applies LeakyReLU' and writes the gradient planes of the next GEMM directly (no separate passes where a
GEMM epilogue can do it).  Parameters are frozen: data gradients only (the reference's loss.backward() also computes
every weight gradient, main.py:573).  All buffers are allocated once; a step is a fixed sequence of launches, so the
attack's HIP graph captures it as is.
"""
from __future__ import annotations

import os

import torch
from ._lib import engine_cache as _engine_cache

from . import _lib as L
from . import igemm as ig

_HEADS = ((6, 1024), (5, 1026), (4, 770), (3, 386), (2, 194))


def pf_split_plan(B: int, H: int, W: int, chunks: int):
    """(chunk slices, starved, floats of the partials buffer) of predict_flow on a [B, H, W] grid of `chunks` chunks, from the
    library (csrc/engine_small.hip `ufr_flow_head_split_plan`): the slices are those of the unsplit launch -- the split form must
    add the same partial sums in the same order -- and `starved` says that the unsplit launch leaves CUs without a workgroup."""
    import ctypes
    slices, starved, floats = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_long(0)
    L.check(L.lib().ufr_flow_head_split_plan(int(B), int(H), int(W), int(chunks), ctypes.byref(slices), ctypes.byref(starved),
                                             ctypes.byref(floats)), "predict_flow split plan")
    return slices.value, bool(starved.value), floats.value


def _pack_flow_head(weight: torch.Tensor) -> torch.Tensor:
    """Conv2d(Cin, 2, 3, 1, 1).weight [2,Cin,3,3] -> [chunks][9][2][32] float32 (csrc/engine_small.hip)."""
    cin = weight.shape[1]
    chunks = ig.pad32(cin) // 32
    w = torch.zeros(2, chunks * 32, 9, dtype=torch.float32, device=weight.device)
    w[:, :cin] = weight.detach().float().reshape(2, cin, 9)
    return w.view(2, chunks, 32, 9).permute(1, 3, 0, 2).contiguous()


def _pack_flow_head_mfma(weight: torch.Tensor) -> torch.Tensor:
    """Conv2d(Cin, 2, 3, 1, 1).weight -> bf16 [chunks][3 planes][2][16][32]: plane p of w[o][32 ch + c][k] at n = 2 k + o
    (the B operand of csrc/engine_small.hip `flow_head_planes_fwd_mfma`; columns 18..31 are zero)."""
    cin = weight.shape[1]
    chunks = ig.pad32(cin) // 32
    w = torch.zeros(chunks * 32, 32, dtype=torch.float32, device=weight.device)          # [c][n]
    w[:cin, :18] = weight.detach().float().reshape(2, cin, 9).permute(1, 2, 0).reshape(cin, 18)
    wn = w.view(chunks, 32, 32).permute(0, 2, 1).contiguous()                              # [chunk][n][c]
    planes = ig._split3(wn).view(3, chunks, 32, 32).permute(1, 0, 2, 3).contiguous()      # [chunk][plane][n][c]
    return planes


def _pack_flow_tail_mfma(weight2: torch.Tensor) -> torch.Tensor:
    """The two flow rows of a ConvTranspose2d(Cin, Cout, 4, 2, 1) weight, [2, Cout, 4, 4] -> bf16 [chunks][3][2][16][32] with
    n = 2 (4 ky + kx) + o (csrc/engine_small.hip `flow_head_planes_fwd_mfma<1>`)."""
    cout = weight2.shape[1]
    chunks = ig.pad32(cout) // 32
    w = torch.zeros(chunks * 32, 32, dtype=torch.float32, device=weight2.device)          # [c][n]
    w[:cout] = weight2.detach().float().reshape(2, cout, 16).permute(1, 2, 0).reshape(cout, 32)
    wn = w.view(chunks, 32, 32).permute(0, 2, 1).contiguous()                               # [chunk][n][c]
    return ig._split3(wn).view(3, chunks, 32, 32).permute(1, 0, 2, 3).contiguous()


# Where this engine sizes split-K against another (tile rows, slots) than `igemm.tile_rows_and_slots` says:
_TILE = {7: (128, 768)}                            # the tap-reuse form as the single-stage tile (kept for bit-stability, unmeasured)
_WINDOW_TILE = {**_TILE, 4: (128, 768)}            # window prefix: every form but 5 / 6 as that tile (kept for bit-stability, unmeasured)
_PLAN = dict(min_ktiles=16, tile=_TILE)            # `igemm.plan_splitk` options of every launch of the engine


class FlowNetCHeadEngine:
    def __init__(self, net, B: int, H: int, W: int, device):
        if H % 64 or W % 64:
            raise ValueError("FlowNetC head engine: frame sides must be multiples of 64")
        L.lib()
        self.net, self.B, self.H, self.W, self.dev = net, int(B), int(H), int(W), torch.device(device)
        g = {s: (H // s, W // s) for s in (4, 8, 16, 32, 64)}
        self.grid = g
        P = lambda s, chunks: ig.Planes(B, g[s][0], g[s][1], chunks, self.dev)
        G = lambda s, chunks: ig.GradSum(B, g[s][0], g[s][1], chunks, self.dev)
        # FlowNetC (siamese: correlation + conv_redir in front of conv3_1) or the plain FlowNetS trunk of FlowNet2 / FlowNet2S
        # (models/flownet2/FlowNetS.py:15-104: conv3_1 reads conv3 directly; same layers and names behind it)
        self.siamese = hasattr(net, "conv_redir")
        # ---- activations
        self.c3a_p, self.c3b_p = (P(8, 8), P(8, 8)) if self.siamese else (None, None)
        self.in31, self.cat3, self.cat2 = P(8, 15 if self.siamese else 8), P(8, 13), P(4, 7)
        self.c4a, self.cat4 = P(16, 16), P(16, 25)
        self.c5a, self.cat5 = P(32, 16), P(32, 33)
        self.c6a, self.c6 = P(64, 32), P(64, 32)
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.flow = {k: torch.zeros(B, 2, *g[2 ** k], **f32) for k in (6, 5, 4, 3, 2)}
        # ---- gradients
        self.G_cat2, self.G_cat3, self.G_cat4, self.G_cat5 = G(4, 7), G(8, 13), G(16, 25), G(32, 33)
        self.G_c6, self.G_in31, self.G_c3a = G(64, 32), G(8, 15 if self.siamese else 8), G(8, 8)
        self.gz_cat2, self.gz_cat3, self.gz_cat4, self.gz_cat5 = P(4, 7), P(8, 13), P(16, 25), P(32, 33)
        self.gz_c6, self.gz_c6a, self.gz_c5a, self.gz_c4a = P(64, 32), P(64, 32), P(32, 16), P(16, 16)
        self.gz_in31 = P(8, 15) if self.siamese else None
        self.g_flow = {k: torch.zeros(B, 2, *g[2 ** k], **f32) for k in (6, 5, 4, 3)}
        self.g_corr = torch.zeros(B, 21, 21, *g[8], **f32)
        self.g_c2a = torch.zeros(B, 128, *g[4], **f32)
        self.g_c3a, self.g_c3a_redir, self.g_c3b = (torch.zeros(B, 256, *g[8], **f32) for _ in range(3))
        self.c3_nchw = torch.zeros(2 * B, 256, *g[8], **f32)        # both frames' conv3 for the correlation kernels
        self._prefix = None                                          # full-frame conv1-3 buffers + launches, built on first use
        self.flow_out, self.flow_scale = self.flow[2], float(getattr(net, "div_flow", 20.0))   # what the step's fused loss kernel reads
        self._wprefixes, self._wprefix = {}, None                    # window-prefix state per window size; the one used last
        self._win_m3 = 0                         # conv3 rim of the last window patched into the planes (0: the whole window)
        self._build_launches()

    # ------------------------------------------------------------------------------------------------ set-up
    def _conv(self, name):
        return getattr(self.net, name)[0]

    def _bias(self, conv):
        """The epilogue's bias; a layer without one (the Robust FlowNetC family's deconvolutions) gets zeros, bit-identical."""
        if conv.bias is None:
            return torch.zeros(conv.out_channels, dtype=torch.float32, device=self.dev)
        return conv.bias.detach().float().contiguous()

    def _stem_layers(self):
        """[(name, Conv2d, level)] of the network's prefix chain (plane_graph.stem_stages), conv1 first; level = log2 of the
        output stride.  The taps are the last layers of levels 2 and 3."""
        from .plane_graph import stem_stages
        return [(name, block[0], lvl) for lvl, stage in enumerate(stem_stages(self.net), 1) for name, block in stage]

    def _build_launches(self):
        net, g = self.net, self.grid
        queue = ig.LaunchQueue(self.dev, **_PLAN)       # sized together for one split-K workspace

        def plan(wi, x, in_chunk0, rows, out_hw, **kw):
            kw.setdefault("variant", self._variant_for(wi))
            return queue.add(wi, x, in_chunk0, rows, out_hw, **kw)

        # 128-column launches: csrc/igemm.hip variant 6 (ping-pong: 256 x 128 tiles, two wave groups of one workgroup per CU half a
        # step apart); UFR_IGEMM_PIPE=5: pipelined 128 x 128, two workgroups per CU; UFR_IGEMM_PIPE=0: the single-stage kernel.
        # Same box, one iteration: 6.27 / 6.56 / 6.88 ms (profiles/r2_bench_pingpong_ab.txt).  64-column launches (deconv2
        # forward, conv1, conv_redir) always run the single-stage 128 x 64 tile.
        self._pipe_variant = {"0": 2, "5": 5}.get(os.environ.get("UFR_IGEMM_PIPE", "6"), 6)

        fwd, bwd = {}, {}
        cw = lambda n, s, p: ig.conv_forward_weights(self._conv(n).weight, s, p)
        cb = lambda n, s, p: ig.conv_backward_weights(self._conv(n).weight, s, p)
        bias = lambda n: self._bias(self._conv(n))
        # forward chain (FlowNetC.py:142-160)
        if self.siamese:
            fwd["conv_redir"] = plan(cw("conv_redir", 1, 0), self.c3a_p, 0, g[8], g[8], out_planes=self.in31, out_chunk0=0,
                                     bias=bias("conv_redir"))
        fwd["conv3_1"] = plan(cw("conv3_1", 1, 1), self.in31, 0, g[8], g[8], out_planes=self.cat3, out_chunk0=0, bias=bias("conv3_1"))
        fwd["conv4"] = plan(cw("conv4", 2, 1), self.cat3, 0, g[16], g[16], out_planes=self.c4a, bias=bias("conv4"))
        fwd["conv4_1"] = plan(cw("conv4_1", 1, 1), self.c4a, 0, g[16], g[16], out_planes=self.cat4, out_chunk0=0, bias=bias("conv4_1"))
        fwd["conv5"] = plan(cw("conv5", 2, 1), self.cat4, 0, g[32], g[32], out_planes=self.c5a, bias=bias("conv5"))
        fwd["conv5_1"] = plan(cw("conv5_1", 1, 1), self.c5a, 0, g[32], g[32], out_planes=self.cat5, out_chunk0=0, bias=bias("conv5_1"))
        fwd["conv6"] = plan(cw("conv6", 2, 1), self.cat5, 0, g[64], g[64], out_planes=self.c6a, bias=bias("conv6"))
        fwd["conv6_1"] = plan(cw("conv6_1", 1, 1), self.c6a, 0, g[64], g[64], out_planes=self.c6, bias=bias("conv6_1"))
        # refinement (FlowNetC.py:162-183): deconvK reads the level above, writes the middle segment of catK
        dec = {5: (self.c6, 64, self.cat5, 16), 4: (self.cat5, 32, self.cat4, 16), 3: (self.cat4, 16, self.cat3, 8),
               2: (self.cat3, 8, self.cat2, 4)}
        for k, (src, s_in, dst, chunk0) in dec.items():
            n = f"deconv{k}"
            fwd[n] = plan(ig.deconv_forward_weights(self._conv(n).weight, 1), src, 0, g[s_in], g[s_in // 2], out_planes=dst,
                          out_chunk0=chunk0, bias=bias(n))
        # backward (reverse order of use; see module docstring)
        gz = {5: (self.gz_cat5, 16, 16), 4: (self.gz_cat4, 16, 8), 3: (self.gz_cat3, 8, 4), 2: (self.gz_cat2, 4, 2)}
        Gabove = {2: self.G_cat3, 3: self.G_cat4, 4: self.G_cat5}
        # deconvK's input ends with the two channels of the upsampled flow: 386 / 770 / 1026 columns would pad the GEMM to
        # 512 / 896 / 1152 (and deconv3 / deconv4 to a second round of workgroups); the 384 / 768 / 1024 feature channels go
        # through the igemm and the two flow columns through the 2-channel kernel (`_deconv_tail`)
        self.tail_w, self.tail_args = {}, {}
        for k in (2, 3, 4):
            src, chunk0, _ = gz[k]
            s_in = {2: 8, 3: 16, 4: 32}[k]
            w = self._conv(f"deconv{k}").weight
            main = w.shape[0] - 2
            bwd[f"deconv{k}"] = plan(ig.deconv_backward_weights(w[:main], 1), src, chunk0, g[s_in], g[s_in], out_f32=Gabove[k])
            self.tail_w[k] = _pack_flow_tail_mfma(w[main:])
            self.tail_args[k] = (src, chunk0, ig.pad32(w.shape[1]) // 32, Gabove[k], main // 32, g[s_in])
        bwd["deconv5"] = plan(ig.deconv_backward_weights(self._conv("deconv5").weight, 1), self.gz_cat5, 16, g[64], g[64],
                              add=self.G_c6, mask=self.c6, out_planes=self.gz_c6)
        bwd["conv6_1"] = plan(cb("conv6_1", 1, 1), self.gz_c6, 0, g[64], g[64], mask=self.c6a, out_planes=self.gz_c6a)
        bwd["conv6"] = plan(cb("conv6", 2, 1), self.gz_c6a, 0, g[64], g[32], add=self.G_cat5, mask=self.cat5, out_planes=self.gz_cat5)
        bwd["conv5_1"] = plan(cb("conv5_1", 1, 1), self.gz_cat5, 0, g[32], g[32], mask=self.c5a, out_planes=self.gz_c5a)
        bwd["conv5"] = plan(cb("conv5", 2, 1), self.gz_c5a, 0, g[32], g[16], add=self.G_cat4, mask=self.cat4, out_planes=self.gz_cat4)
        bwd["conv4_1"] = plan(cb("conv4_1", 1, 1), self.gz_cat4, 0, g[16], g[16], mask=self.c4a, out_planes=self.gz_c4a)
        bwd["conv4"] = plan(cb("conv4", 2, 1), self.gz_c4a, 0, g[16], g[8], add=self.G_cat3, mask=self.cat3, out_planes=self.gz_cat3)
        if self.siamese:
            # its 473 columns: chunk 0 (conv_redir's output) is read as planes by conv_redir's adjoint, chunks 1 .. (the cost volume)
            # as fp32 by the correlation's: each leaves the tile once, in the form its reader wants (4.4 instead of 10 B per element)
            bwd["conv3_1"] = plan(cb("conv3_1", 1, 1), self.gz_cat3, 0, g[8], g[8], mask=self.in31, out_planes=self.gz_in31,
                                  out_f32=self.G_in31, planes_chunks=1, f32_first_chunk=1)
            bwd["conv_redir"] = plan(cb("conv_redir", 1, 0), self.gz_in31, 0, g[8], g[8], out_f32=self.G_c3a)
        else:                                   # the trunk's input IS conv3's activation: its gradient leaves unmasked
            bwd["conv3_1"] = plan(cb("conv3_1", 1, 1), self.gz_cat3, 0, g[8], g[8], out_f32=self.G_in31)
        self.ws = queue.build()
        self.fwd = {k: h.launch for k, h in fwd.items()}
        self.plain = {}                         # (table tag, name): the plain twin of a launch that runs with its last round re-cut
        self.bwd = {k: self._with_tail(("full", k), h.launch, h.args, h.kw, h.S) for k, h in bwd.items()}
        # (weights, input planes, first chunk, row grid, output grid, split-K factor, make_launch kwargs without ws)
        self._plans = {("fwd", k): (*h.args, h.S, h.kw) for k, h in fwd.items()}
        self._plans.update({("bwd", k): (*h.args, h.S, h.kw) for k, h in bwd.items()})
        self._band, self.fwd_band, self.bwd_band = None, {}, {}
        self.bwd_band_wide, self.bwd_rest, self._band_plans, self._pf_band, self._split_w = {}, {}, {}, {}, {}
        # 2-channel layers
        self.pf_w = {k: _pack_flow_head(getattr(net, f"predict_flow{k}").weight) for k, _ in _HEADS}
        self.pf_wm = {k: _pack_flow_head_mfma(getattr(net, f"predict_flow{k}").weight) for k, _ in _HEADS}
        self.pf_b = {k: getattr(net, f"predict_flow{k}").bias.detach().float().contiguous() for k, _ in _HEADS}
        self.up = {k: getattr(net, f"upsampled_flow{k}_to_{k - 1}") for k in (6, 5, 4, 3)}
        self.up_w = {k: m.weight.detach().float().contiguous() for k, m in self.up.items()}
        self.up_b = {k: (m.bias.detach().float().contiguous() if m.bias is not None else None) for k, m in self.up.items()}
        self.pf_src = {6: (self.c6, 32), 5: (self.cat5, 33), 4: (self.cat4, 25), 3: (self.cat3, 13), 2: (self.cat2, 7)}
        self.pf_G = {6: self.G_c6, 5: self.G_cat5, 4: self.G_cat4, 3: self.G_cat3, 2: self.G_cat2}
        # upsampled_flowK_to_K-1 writes the last chunk of cat(K-1)
        self.up_dst = {6: (self.cat5, 32), 5: (self.cat4, 24), 4: (self.cat3, 12), 3: (self.cat2, 6)}
        self.up_G = {6: (self.G_cat5, 32), 5: (self.G_cat4, 24), 4: (self.G_cat3, 12), 3: (self.G_cat2, 6)}
        # predict_flowK on a grid too small to fill the chip with one workgroup per tile: the chunk slices spread over the grid
        # (csrc/engine_small.hip `flow_head_split_gemm`), the finishing sum runs with upsampled_flowK in one launch.  The rule is
        # on the workgroup count (ufr_flow_head_split_plan), not on the level; level 2 has no upsampling behind it and stays.
        self.pf_split, floats = {}, 0
        for k in (6, 5, 4, 3):
            src, chunks = self.pf_src[k]
            slices, starved, n = pf_split_plan(self.B, src.H, src.W, chunks)
            if starved:
                self.pf_split[k] = (slices, n)
                floats = max(floats, n)
        self.pf_partials = torch.empty(max(floats, 1), dtype=torch.float32, device=self.dev)   # one level at a time uses it
        self._pf_pending = None                  # the level whose partial sums wait for `_up_forward` to finish them
        self.pf_ran = {}                         # launch record: level -> "split" | "mfma", what its last forward ran

    # ------------------------------------------------------------------------------------------------ conv1-3
    def _with_tail(self, key, plain, args, kw, S, resident=None):
        """`plain`, or -- when `ufr_igemm_tail_plan` says it pays -- the same launch with the tiles of its under-filled last round
        split over K (igemm.make_launch `balance`).  The plain launch then stays in `self.plain[key]` for `backward(tail_split=False)`.
        `resident`: workgroups the chip holds (None: its CU count).  Tests pass a small number so that small grids have a tail; the
        split-K factor `S` was sized for the real chip, so with the override the plan alone decides."""
        self.plain.pop(key, None)
        if S != 1 and resident is None:
            return plain
        wi, x, c0, rows, out_hw = args
        launch = ig.make_launch(wi, x, c0, rows, out_hw, ws=self.ws, balance=True, resident=resident, **kw)
        if launch.tail_plan is None:
            return plain
        self.plain[key] = plain
        return launch

    def tail_launches(self):
        """[(table tag, name, plan)] of the launches that run with a re-cut last round."""
        tables = {"full": self.bwd, "band": self.bwd_band, "rest": self.bwd_rest}
        return [(tag, name, tables[tag][name].tail_plan) for tag, name in sorted(self.plain)]

    def _variant_for(self, wi):
        """The igemm form of a launch: the 128-column forms as `UFR_IGEMM_PIPE` says, 64-column launches single-stage."""
        return self._pipe_variant if wi.Npad % 128 == 0 else 2

    def _build_prefix(self):
        """Full-frame prefix for both frames of every pair (models/FlowNetC.py:100-119; the stages of Robust FlowNetC,
        models/FlowNetC_flexible_larger_field.py:111-176), run once per attack() call, as two chains -- one per frame set -- of
        conv1 and one igemm launch per further layer (`_stem_layers`) that write where the head reads: the first frames'
        stage-2 output (conv2) into cat2's chunks 0-3 (the skip connection) and their stage-3 output (conv3) into c3a_p, the
        second frames' into c3b_p.  (One chain
        over both sets needed three strided copies afterwards, 0.2 ms per call; with 256-row tiles the halves fill the same
        number of rounds: conv2 4 + 4 for 8, conv3 2 + 2 for 4.)"""
        B, dev = self.B, self.dev
        H, W = self.H, self.W
        layers = self._stem_layers()
        # conv2 (K = 25 taps x 2 chunks) at 2 x 8 frames: 1.35 ms on single-stage 128 x 128 tiles, 1.02-1.05 on 64 x 128 tiles
        # (four workgroups per CU), 0.99-1.00 on the pipelined 128 x 128 kernel, 0.89-0.94 on the ping-pong kernel: every
        # 128-column layer of the chain runs the `UFR_IGEMM_PIPE` form, a 64-column one (Robust FlowNetC's 64 -> 64) single-stage
        wis = [None] + [ig.conv_forward_weights(conv.weight, conv.stride[0], conv.padding[0]) for _, conv, _ in layers[1:]]
        # Only the taps must land where the head reads them; every other layer of a level writes one of two buffers of that
        # level, alternating (one level-1 buffer of 8 frames at 384 x 1280 is 377 MB), shared by both chains (one stream)
        scratch = {}

        def level_buffer(lvl, slot, chunks):
            if (lvl, slot) not in scratch:
                scratch[(lvl, slot)] = ig.Planes(B, H >> lvl, W >> lvl, chunks, dev)
            return scratch[(lvl, slot)]
        halves = {}
        for h, taps in (("a", {2: self.cat2, 3: self.c3a_p}), ("b", {3: self.c3b_p})):
            outs = []
            for i, (_, conv, lvl) in enumerate(layers):
                later = sum(1 for _, _, l in layers[i + 1:] if l == lvl)        # layers of the same level after this one
                outs.append(taps[lvl] if later == 0 and lvl in taps else level_buffer(lvl, later % 2, ig.pad32(conv.out_channels) // 32))
            chain = []
            for i in range(1, len(layers)):
                name, conv, lvl = layers[i]
                launch = ig.make_launch(wis[i], outs[i - 1], 0, (H >> lvl, W >> lvl), (H >> lvl, W >> lvl), out_planes=outs[i],
                                        out_chunk0=0, bias=self._bias(conv), variant=self._variant_for(wis[i]))
                chain.append((name, launch, wis[i]))
            conv1 = layers[0][1]
            P = dict(c1=outs[0], layers=chain, b1=self._bias(conv1), w1=conv1.weight.detach())
            P.update({name: launch for name, launch, _ in chain})
            P.update({name + "_wi": wi for name, _, wi in chain})
            P.update(self._conv1_launch(B, H, W, outs[0]))
            halves[h] = P
        self._prefix = halves

    def _conv1_launch(self, n: int, H: int, W: int, c1: ig.Planes) -> dict:
        """conv1 = Conv2d(3, 64, 7, 2, 3) + bias + LeakyReLU as an igemm launch over the packed planes of the raw frames
        (csrc/plane_layout.hip `conv1_pack_kernel`: pixel-unshuffle + two columns per chunk -> 8 taps of one chunk, the mean
        subtraction and the zero padding inside the buffer), writing conv1's planes directly."""
        conv1 = self._stem_layers()[0][1]
        bias = self._bias(conv1)
        if os.environ.get("UFR_CONV1_DIRECT", "1") != "0":
            # round 4: ONE kernel from the raw frames to conv1's planes (csrc/conv1_direct.hip): no packed buffer, no pack pass
            return dict(direct=dict(wimg=ig.conv1_direct_weights(conv1.weight), bias=bias, c1=c1, n=n, hw=(H, W),
                                    gflop=2.0 * n * (H // 2) * (W // 2) * 147 * 64 / 1e9))
        packed = ig.Planes(n, H // 2 + 3, W // 2 + 2, 1, self.dev)
        wi = ig.conv1_packed_weights(conv1.weight)
        launch = ig.make_launch(wi, packed, 0, (H // 2, W // 2), (H // 2, W // 2), out_planes=c1, bias=bias, variant=2)
        return dict(packed=packed, conv1=launch, conv1_wi=wi)

    def _conv1(self, P: dict, a: torch.Tensor, b: torch.Tensor | None):
        """conv1 + bias + LeakyReLU of one or two raw frame stacks into P['c1']."""
        a = a.contiguous()
        L.require_hip(a, "frames")
        nb = 0 if b is None else int(b.shape[0])
        mean = self.net._mean64.reshape(-1).contiguous()
        D = P.get("direct")
        if D is not None:
            c1 = D["c1"]
            L.check(L.lib().ufr_conv1_direct(L.ptr(a), L.ptr(b.contiguous()) if b is not None else None, int(a.shape[0]), nb,
                                             int(a.shape[2]), int(a.shape[3]), L.ptr(mean), L.ptr(D["wimg"]), L.ptr(D["bias"]),
                                             float(ig.LEAKY), L.ptr(c1.t), c1.plane_stride, 0, L.stream()), "conv1 direct")
            return
        pk = P["packed"]
        L.check(L.lib().ufr_conv1_pack_planes(L.ptr(a), L.ptr(b.contiguous()) if b is not None else None, L.ptr(pk.t),
                                              pk.plane_stride, int(a.shape[0]), nb, int(a.shape[2]), int(a.shape[3]),
                                              L.ptr(mean), L.stream()), "conv1 pack")
        P["conv1"]()

    def prefix_full(self, frames_a: torch.Tensor, frames_b: torch.Tensor):
        """New frames: conv2 of the first frames and conv3 of both, for the full frame, straight into the head's plane
        buffers (cat2[0:4], c3a_p, c3b_p) plus conv3 in NCHW for the correlation kernels."""
        if self._prefix is None:
            self._build_prefix()
        B = self.B

        def chain(h, frames, out):
            P = self._prefix[h]
            self._conv1(P, frames, None)
            for _, launch, _ in P["layers"]:
                launch()
            (self.c3a_p if h == "a" else self.c3b_p).to_nchw(256, 0, out=out)
        # (the two chains on two streams, so that one launch's tail is filled by the other chain's workgroups, measured no
        # faster: 5.638 against 5.620 ms in one call, gpurun r4_call5 -- the chains stay on one stream)
        chain("a", frames_a, self.c3_nchw[:B])
        chain("b", frames_b, self.c3_nchw[B:])
        self._c3a, self._c3b = self.c3_nchw[:B], self.c3_nchw[B:]

    def load_prefix_features(self, c2_all: torch.Tensor, c3_all: torch.Tensor):
        """The same from NCHW features the caller already holds (train()'s clean forward seeds the attack's cache)."""
        B = self.B
        self.cat2.load_nchw(c2_all[:B].contiguous(), 0)
        self.c3_nchw.copy_(c3_all[:2 * B])
        self._c3a, self._c3b = self.c3_nchw[:B], self.c3_nchw[B:]
        self.c3a_p.load_nchw(self._c3a, 0)
        self.c3b_p.load_nchw(self._c3b, 0)

    def scatter_window_features(self, c2_w: torch.Tensor, c3_w: torch.Tensor, win: torch.Tensor, wh: int, ww: int, m2: int, m3: int):
        """The windowed prefix's conv2 (first frames) / conv3 (both frames) patched into the cached planes and into the NCHW
        conv3 the correlation reads; `win` = the step's origin table, m2 / m3 = rim margins in cells (cone.py)."""
        lib, B, st = L.lib(), self.B, L.stream()
        h4, w4 = self.grid[4]
        h8, w8 = self.grid[8]
        self._win_m3 = int(m3)
        L.check(lib.ufr_window_scatter_planes(L.ptr(c2_w), L.ptr(self.cat2.t), self.cat2.plane_stride, 0, L.ptr(win), B, B, 128,
                                              h4, w4, wh // 4, ww // 4, 4, m2, st), "window -> planes (conv2)")
        for k, dst in ((0, self.c3a_p), (1, self.c3b_p)):
            L.check(lib.ufr_window_scatter_planes(L.ptr(c3_w[k * B:]), L.ptr(dst.t), dst.plane_stride, 0, L.ptr(win), B, B, 256,
                                                  h8, w8, wh // 8, ww // 8, 8, m3, st), "window -> planes (conv3)")
        L.check(lib.ufr_window_scatter(L.ptr(c3_w), L.ptr(self.c3_nchw), L.ptr(win), B, 2 * B, 256, h8, w8, wh // 8, ww // 8, 8,
                                       m3, st), "window -> nchw (conv3)")

    # ------------------------------------------------------------------------------------------------ windowed conv1-3
    def _build_window_prefix(self, wh: int, ww: int):
        """conv1-3 of both frames on the patch attack's prefix window (patch_attack.py `_forward_cone`: [2B, 3, wh, ww]) and
        their data gradients, all on the igemm: conv2 / conv3 (5x5, stride 2: 92% of the window's FLOPs) as they are, conv1
        (3 input channels) over the packed planes of the raw window stack (`_conv1_launch`), its data gradient with respect
        to those planes followed by the unpacking.  One state per window size, kept for the engine's life: a step's captured
        HIP graphs hold raw pointers into these buffers, and another step on the same network may use another size."""
        B2, dev = 2 * self.B, self.dev
        f32 = dict(dtype=torch.float32, device=dev)
        h2, w2, h4, w4, h8, w8 = wh // 2, ww // 2, wh // 4, ww // 4, wh // 8, ww // 8
        layers = self._stem_layers()
        n = len(layers)
        tap2 = max(i for i, (_, _, lvl) in enumerate(layers) if lvl == 2)      # the skip connection's layer (conv2)
        # every layer's output stays (its LeakyReLU' is the mask of the data gradient that reaches it), and its gradient planes
        acts = [ig.Planes(B2, wh >> lvl, ww >> lvl, ig.pad32(conv.out_channels) // 32, dev) for _, conv, lvl in layers]
        gz = [ig.Planes(B2, wh >> lvl, ww >> lvl, ig.pad32(conv.out_channels) // 32, dev) for _, conv, lvl in layers]
        G_p = ig.GradSum(B2, h2 + 3, w2 + 2, 1, dev)
        G_gw2 = ig.GradSum(B2, h4, w4, 4, dev)       # the conv2 tap's window gradient (first frames; second frames stay 0)
        grid = lambda i: (wh >> layers[i][2], ww >> layers[i][2])
        queue, names = ig.LaunchQueue(dev, tune=False, **dict(_PLAN, tile=_WINDOW_TILE)), []
        plan = lambda wi, x, rows, out_hw, **kw: queue.add(wi, x, 0, rows, out_hw, **{"variant": self._variant_for(wi), **kw})
        # (the window's forward convolutions: 64 x 128 tiles measured 1.3x faster than 128 x 128 at the same split,
        # 0.047 vs 0.055 ms)
        for i in range(1, n):
            name, conv, _ = layers[i]
            plan(ig.conv_forward_weights(conv.weight, conv.stride[0], conv.padding[0]), acts[i - 1], grid(i), grid(i),
                 out_planes=acts[i], bias=self._bias(conv), variant=4)
            names.append(name)
        # data gradients, last layer first: x LeakyReLU'(the layer below) -> its gradient planes; where the conv2 tap's output
        # is reached, the skip connection's gradient is added in the same epilogue
        for i in range(n - 1, 0, -1):
            name, conv, _ = layers[i]
            kw = dict(add=G_gw2, mask=acts[i - 1], out_planes=gz[i - 1]) if i - 1 == tap2 else dict(out_planes=gz[i - 1], mask=acts[i - 1])
            plan(ig.conv_backward_weights(conv.weight, conv.stride[0], conv.padding[0]), gz[i], grid(i), grid(i - 1), **kw)
            names.append(name + "_bwd")
        # conv1's data gradient with respect to the packed planes (the unpacking follows)
        plan(ig.conv1_packed_backward_weights(layers[0][1].weight), gz[0], (h2 + 3, w2 + 2), (h2 + 3, w2 + 2), out_f32=G_p)
        names.append(layers[0][0] + "_bwd")
        ws = queue.build()
        chain = [(name, h.launch, h.wi) for name, h in zip(names, queue.handles)]
        P = dict(hw=(wh, ww), c1=acts[0], c2=acts[tap2], c3=acts[-1], gz_c3=gz[-1], gz_c2=gz[tap2], G_gw2=G_gw2, ws=ws,
                 acts=acts, gz=gz, fwd=chain[:n - 1], bwd=chain[n - 1:],
                 G_p=G_p, gxw=torch.zeros(B2, 3, wh, ww, **f32),
                 c2_nchw=torch.zeros(B2, 128, h4, w4, **f32), c3_nchw=torch.zeros(B2, 256, h8, w8, **f32))
        P.update({name: launch for name, launch, _ in chain})
        P.update({name + "_wi": wi for name, _, wi in chain})
        P.update(self._conv1_launch(B2, wh, ww, acts[0]))
        self._wprefixes[(wh, ww)] = P
        self._bound_wprefixes()
        return P

    MAX_WINDOW_PREFIXES = 4

    def _bound_wprefixes(self):
        """At most MAX_WINDOW_PREFIXES window sizes stay cached (least recently used goes).  A step that captured graphs over a
        state holds the state itself (PatchAttackStep._wp_hold), so dropping it here never frees memory a graph points into."""
        while len(self._wprefixes) > self.MAX_WINDOW_PREFIXES:
            del self._wprefixes[next(iter(self._wprefixes))]

    def window_prefix(self, wh: int, ww: int) -> dict:
        """The window-prefix state for a (wh, ww) window; `_wprefix` = the one used last (launch_table, the backward)."""
        P = self._wprefixes.pop((int(wh), int(ww)), None)
        if P is None:
            P = self._build_window_prefix(int(wh), int(ww))
        else:
            self._wprefixes[(int(wh), int(ww))] = P          # most recently used last
        self._wprefix = P
        return P

    def window_prefix_forward(self, xw: torch.Tensor, win: torch.Tensor, m2: int, m3: int, c2_nchw: bool = True):
        """conv1-3 of the window stack `xw` [2B, 3, wh, ww] (raw frames; first frames, then second frames), patched into the
        cached full-frame features.  The window's convolutions zero-pad at the window's edges exactly like the torch
        prefix they replace; the inexact rim (m2 / m3 cells) is skipped by the scatter.  `c2_nchw=False` leaves P["c2_nchw"]
        (the window's conv2 as NCHW float32, which nothing on the attack's path reads) unwritten."""
        wh, ww = int(xw.shape[2]), int(xw.shape[3])
        P = self.window_prefix(wh, ww)
        self._win_m3 = int(m3)
        self._conv1(P, xw.detach(), None)
        for _, launch, _ in P["fwd"]:
            launch()
        # planes -> planes, + conv3 as float32 for the correlation and (P["c3_nchw"], every cell) for the backward's LeakyReLU'
        c2, c3, H, W = P["c2"], P["c3"], self.H, self.W
        L.check(L.lib().ufr_window_features_planes(
            L.ptr(c2.t), c2.plane_stride, L.ptr(c3.t), c3.plane_stride, L.ptr(self.cat2.t), self.cat2.plane_stride,
            L.ptr(self.c3a_p.t), self.c3a_p.plane_stride, L.ptr(self.c3b_p.t), self.c3b_p.plane_stride, L.ptr(self.c3_nchw),
            L.ptr(P["c3_nchw"]), L.ptr(win), self.B, H, W, wh, ww, int(m2), int(m3), L.stream()), "window features -> planes")
        if c2_nchw:
            c2.to_nchw(128, 0, out=P["c2_nchw"])

    def window_gather_conv2_gradient(self, win: torch.Tensor, m2: int):
        """The conv2 tap's window gradient straight from the head's chunk-major sum of cat2 (chunks 0-3 = conv2 of the
        first frames) into the addend of conv3's data gradient: no full-frame NCHW conversion, no NCHW window."""
        P = self._wprefix
        wh, ww = P["hw"]
        h4, w4 = self.grid[4]
        L.check(L.lib().ufr_window_gather_chunks(L.ptr(self.G_cat2.t), L.ptr(P["G_gw2"].t), L.ptr(win), self.B, self.B, 2 * self.B, 4,
                                                 h4, w4, wh // 4, ww // 4, 4, int(m2), L.stream()), "window gather (chunks)")

    def window_prefix_backward(self, gw3: torch.Tensor, gw2: torch.Tensor | None = None, unpack: bool = True) -> torch.Tensor:
        """d loss / d xw from the window gradients of the two taps: gw3 [2B, 256, wh/8, ww/8] (conv3 of both frames, rim
        zeroed); the conv2 tap's (first frames) was put into `G_gw2` by `window_gather_conv2_gradient`, or is handed over
        here as NCHW [B, 128, wh/4, ww/4].  `unpack=False` returns conv1's packed gradient sum [1, 2B (wh/2+3) (ww/2+2), 32]
        instead (ufr_patch_grad_crop_packed reads it through the unpacking's index map)."""
        P, B = self._wprefix, self.B
        wh, ww = P["hw"]
        if gw2 is not None:                      # NCHW -> chunk-major addend (tests, callers without the engine's sums)
            full = torch.zeros(2 * B, 128, wh // 4, ww // 4, dtype=torch.float32, device=self.dev)
            full[:B] = gw2
            P["G_gw2"].t.copy_(full.view(2 * B, 4, 32, wh // 4, ww // 4).permute(1, 0, 3, 4, 2).reshape(4, -1, 32))
        gz = P["gz_c3"]                          # x LeakyReLU'(conv3), split into the planes conv3's data gradient reads
        L.check(L.lib().ufr_nchw_grad_to_planes(L.ptr(gw3), L.ptr(P["c3_nchw"]), L.ptr(gz.t), gz.plane_stride, 0, 2 * B, 256, wh // 8,
                                                ww // 8, ig.LEAKY, L.stream()), "window gradient -> planes")
        # layer by layer down the chain: x LeakyReLU'(the layer below) -> its gradient planes (epilogue), + G_gw2 where the conv2
        # tap's output is reached; conv1's -> gradient of the packed planes -> gradient of the raw window stack
        for _, launch, _ in P["bwd"]:
            launch()
        if not unpack:
            return P["G_p"].t
        L.check(L.lib().ufr_conv1_unpack_grad(L.ptr(P["G_p"].t), L.ptr(P["gxw"]), 2 * B, wh, ww, L.stream()), "conv1 unpack")
        return P["gxw"]

    # ------------------------------------------------------------------------------------------------ column band
    # (level stride of the ROW grid, of the input grid) of the launches that run on the band's columns only
    _FWD_BAND = {"conv_redir": (8, 8), "conv3_1": (8, 8), "conv4": (16, 8), "conv4_1": (16, 16)}
    # data gradients on the band (band_conv.py's BAND_LAYERS): rows = the gy grid; the input (a gradient that itself exists
    # on the band only) reads as zero outside it
    _BWD_BAND = {"conv5": (32, None), "conv4_1": (16, 16), "conv4": (16, 16), "conv3_1": (8, 8), "conv_redir": (8, 8)}

    def attach_band(self, band):
        """Derive the banded launches for `band` (band_conv.Band: device-resident first column per pair, static width):
        the same descriptors with the tile rows restricted to the band -- taps read the full-frame planes, so there is no
        gather / scatter copy and every computed column is exact."""
        if self._band is band:
            return
        self._band, self.fwd_band, self.bwd_band = band, {}, {}
        self.bwd_band_wide, self.bwd_rest, self._band_plans, self._pf_band = {}, {}, {}, {}
        self.plain = {k: v for k, v in self.plain.items() if k[0] == "full"}
        if not band.width:
            return
        W = self.W
        if band.width % 32 or band.width > W:
            raise ValueError("band width must be a multiple of 32 pixels inside the frame")
        origin = band.win[:, 1]                                   # int32 view, 8 elements per pair
        resident = getattr(band, "tail_resident", None)           # (tests: a small chip, so that small grids have a tail round)

        def derive(kind, name, ls_rows, ls_in):
            wi, x, c0, rows, out_hw, S, kw = self._plans[(kind, name)]
            rows_b = (rows[0], band.width // ls_rows)
            extra = dict(row_band=(origin, 8, ls_rows))
            if ls_in is not None:
                extra["in_band"] = (origin, 8, ls_in, band.width // ls_in)
            h = ig.planned_launch(wi, x, c0, rows_b, out_hw, ws=self.ws, options=dict(_PLAN, tune=False), **kw, **extra)   # (the plan's form)
            if kind == "bwd":
                return self._with_tail(("band", name), h.launch, h.args, h.kw, h.S, resident)
            return h.launch

        for name, (ls_rows, _) in self._FWD_BAND.items():
            if ("fwd", name) in self._plans:
                self.fwd_band[name] = derive("fwd", name, ls_rows, None)   # forward inputs are valid everywhere
        for name, (ls_rows, ls_in) in self._BWD_BAND.items():
            if ("bwd", name) in self._plans:
                self.bwd_band[name] = derive("bwd", name, ls_rows, ls_in)
        if self.siamese:
            self._attach_unread(band, origin)

    # deconvK's data gradients whose leading columns (conv3_1's / conv4_1's output gradient) only the band reads
    _SPLIT_DECONV = {2: ("conv3_1", 8), 3: ("conv4_1", 16)}      # K: (the layer whose output gradient leads cat(K+1), its level stride)

    def _attach_unread(self, band, origin):
        """The launches of `backward(skip_unread=True)`: gradients whose only reader is a banded or windowed launch are produced
        where that reader looks.  (a) deconv2 / deconv3's data gradient as two launches over slices of one weight: the columns of
        conv3_1's / conv4_1's output gradient (`add` of bwd_band["conv4"] / ["conv5"]) on the band's rows, the rest (deconv3's /
        deconv4's segment, read in full by the next deconvolution's gradient) on every row; (b) conv3_1 / conv_redir on the
        correlation-reach band (`band.corr_width` pixels from `band.win[:, 2]`: what the window's correlation adjoint reads), their
        input still masked to the wide band, on which gz_cat3 exists.  The wide forms stay in `bwd_band_wide`."""
        def planned(name, wi, x, c0, rows, out_hw, kw):
            kw.setdefault("variant", self._variant_for(wi))       # (a narrower band of a planned layer keeps that plan's form)
            h = ig.planned_launch(wi, x, c0, rows, out_hw, ws=self.ws, options=_PLAN, **kw)
            self._band_plans[name] = (*h.args, h.kw)
            return self._with_tail(("rest" if name.endswith(" rest") else "band", name), h.launch, h.args, h.kw, h.S,
                                   getattr(band, "tail_resident", None))

        for k, (lead, ls) in self._SPLIT_DECONV.items():
            src, chunk0, _, Gd, _, rows = self.tail_args[k]
            w = self._conv(f"deconv{k}").weight
            main, n_band = w.shape[0] - 2, self._conv(lead).out_channels
            if n_band % 32 or not 0 < n_band < main:
                continue
            name = f"deconv{k}"
            if name not in self._split_w:        # packed once for the engine's life: a step's captured graphs point into them
                self._split_w[name] = (ig.deconv_backward_weights(w[:n_band], 1), ig.deconv_backward_weights(w[n_band:main], 1))
            w_band, w_rest = self._split_w[name]
            self.bwd_band[name] = planned(name, w_band, src, chunk0, (rows[0], band.width // ls), rows,
                                          dict(out_f32=Gd, out_f32_chunk0=0, row_band=(origin, 8, ls)))
            self.bwd_rest[name + " rest"] = planned(name + " rest", w_rest, src, chunk0, rows, rows,
                                                    dict(out_f32=Gd, out_f32_chunk0=n_band // 32))
            self._pf_band[k + 1] = (n_band // 32, ls)
        cw = int(getattr(band, "corr_width", 0))
        if cw:
            if cw % 8 or cw > band.width:
                raise ValueError("correlation band: a multiple of 8 pixels inside the band")
            for name in ("conv3_1", "conv_redir"):
                wi, x, c0, rows, out_hw, _, kw = self._plans[("bwd", name)]
                self.bwd_band_wide[name] = self.plain.get(("band", name), self.bwd_band[name])     # (the comparison leg stays plain)
                kw = dict(kw, row_band=(band.win[:, 2], 8, 8), in_band=(origin, 8, 8, band.width // 8))
                self.bwd_band[name] = planned(name, wi, x, c0, (rows[0], cw // 8), out_hw, kw)

    def replan(self, kind: str, name: str, tag: str):
        """(weights, input planes, first chunk, row grid, output grid, make_launch kwargs) of a prepared launch, band geometry
        included: tools/sweep_igemm_launches.py rebuilds it with other kernel forms / split-K factors."""
        if kind == "bwd" and name in self._band_plans and tag == ("full" if name in self.bwd_rest else "band"):
            wi, x, c0, rows, out_hw, kw = self._band_plans[name]          # (the launches of `_attach_unread`)
            return wi, x, c0, rows, out_hw, dict(kw)
        wi, x, c0, rows, out_hw, _, kw = self._plans[(kind, name)]
        kw = dict(kw)
        if tag == "band":
            band = self._band
            ls_rows, ls_in = (self._FWD_BAND[name][0], None) if kind == "fwd" else self._BWD_BAND[name]
            origin = band.win[:, 1]
            rows = (rows[0], band.width // ls_rows)
            kw["row_band"] = (origin, 8, ls_rows)
            if ls_in is not None:
                kw["in_band"] = (origin, 8, ls_in, band.width // ls_in)
        return wi, x, c0, rows, out_hw, kw

    def launch_table(self):
        """Every prepared igemm launch with its algorithmic work, for bench.py's per-kernel rooflines:
        [(name, 'fwd' | 'bwd', 'full' | 'band', launch, GFLOP)]."""
        rows = []
        for kind, table, tag in (("fwd", self.fwd, "full"), ("bwd", self.bwd, "full"), ("fwd", self.fwd_band, "band"),
                                 ("bwd", self.bwd_band, "band"), ("bwd", self.bwd_rest, "full")):
            for name, launch in table.items():
                # (a launch of `_attach_unread` has weights of its own: a slice of the layer's)
                wi = self._band_plans[name][0] if kind == "bwd" and table is not self.bwd and name in self._band_plans else \
                    self._plans[(kind, name)][0]
                d = launch.desc
                rows.append((name, kind, tag, launch, wi.flops(d.B * d.Hr * d.Wr) / 1e9))
        if self._prefix is not None:           # full-frame conv1-3 of the first / second frames, once per attack() call
            for h, suffix in (("a", ""), ("b", " 2nd frames")):
                F = self._prefix[h]
                packed = [("conv1", F["conv1"], F["conv1_wi"])] if "conv1" in F else []    # (UFR_CONV1_DIRECT=0)
                for key, launch, wi in packed + F["layers"]:
                    d = launch.desc
                    rows.append((key + suffix, "fwd", "prefix", launch, wi.flops(d.B * d.Hr * d.Wr) / 1e9))
        P = getattr(self, "_wprefix", None)
        if P is not None:                      # the prefix chain on the attack's window and its data gradient (every iteration)
            packed = [("conv1", P["conv1"], P["conv1_wi"])] if "conv1" in P else []
            for kind, chain in (("fwd", packed + P["fwd"]), ("bwd", P["bwd"])):
                for key, launch, wi in chain:
                    d = launch.desc
                    rows.append((key[:-4] if kind == "bwd" else key, kind, "window", launch, wi.flops(d.B * d.Hr * d.Wr) / 1e9))
        return rows

    def conv1_direct_table(self):
        """The direct conv1 launches (csrc/conv1_direct.hip) for bench.py's per-kernel rooflines: [(label, tag, fn, algorithmic
        bytes, GFLOP)] -- HBM-bound: the raw frames in, conv1's three bf16 planes out."""
        rows = []
        sets = []
        if self._prefix is not None:
            sets += [("conv1 direct" + sfx, "prefix", self._prefix[h]) for h, sfx in (("a", ""), ("b", " 2nd frames"))]
        if getattr(self, "_wprefix", None) is not None:
            sets.append(("conv1 direct", "window", self._wprefix))
        for label, tag, P in sets:
            D = P.get("direct")
            if D is None:
                continue
            n, (H, W) = D["n"], D["hw"]
            frames = torch.rand(n, 3, H, W, device=self.dev)
            nbytes = n * 3 * H * W * 4 + n * (H // 2) * (W // 2) * 64 * 6
            rows.append((label, tag, (lambda P=P, frames=frames: self._conv1(P, frames, None)), float(nbytes), D["gflop"]))
        return rows

    # ------------------------------------------------------------------------------------------------ small launches
    def _pf_forward(self, k, defer=False):
        """predict_flowK -> flow[k].  `defer` (the schedules, which run `_up_forward(k)` next): a level on the split form leaves
        its partial sums for that launch to finish; without it the call leaves a complete flow[k] behind."""
        src, chunks = self.pf_src[k]
        if k in self.pf_split:
            slices, n = self.pf_split[k]
            L.check(L.lib().ufr_flow_head_planes_forward_split(L.ptr(src.t), src.plane_stride, 0, chunks, L.ptr(self.pf_wm[k]),
                                                               self.pf_wm[k].shape[0], L.ptr(self.pf_partials), n, slices, self.B, src.H,
                                                               src.W, L.stream()), "predict_flow forward (split)")
            self.pf_ran[k] = "split"
            self._pf_pending = k
            if not defer:
                self._pf_finish(k, upsample=False)
            return
        self.pf_ran[k] = "mfma"
        L.check(L.lib().ufr_flow_head_planes_forward_mfma(L.ptr(src.t), src.plane_stride, 0, chunks, L.ptr(self.pf_wm[k]),
                                                          self.pf_wm[k].shape[0], L.ptr(self.pf_b[k]), L.ptr(self.flow[k]), self.B, src.H, src.W,
                                                          L.stream()), "predict_flow forward (mfma)")

    def _pf_backward(self, k, gy, accumulate, finalize=None, region=None):
        """predict_flowK^T; `finalize` = (activation planes, gradient planes, first chunk, chunks) of the segment whose gradient
        sum is complete with this launch (deconvK's output): x LeakyReLU' -> planes in the same kernel (round 4).
        `region` = (head chunks, kind, origin table, ints per pair, divisor, rows, columns, margin, window GradSum | None): the
        leading chunks are read on that region only and are written there only (ufr_flow_head_planes_backward_regions)."""
        src, chunks = self.pf_src[k]
        if region is not None:
            head, kind, origin, stride, div, rh, rw, margin, wout = region
            act, out, c0, n = finalize if finalize is not None else (None, None, 0, 0)
            L.check(L.lib().ufr_flow_head_planes_backward_regions(
                L.ptr(gy), L.ptr(self.pf_w[k]), self.pf_w[k].shape[0], L.ptr(self.pf_G[k].t), self.pf_G[k].chunks, 0, chunks, self.B,
                src.H, src.W, int(accumulate), int(head), int(kind), L.ptr(origin), int(stride), int(div), int(rh), int(rw), int(margin),
                L.ptr(wout.t) if wout is not None else None, wout.B if wout is not None else 0,
                L.ptr(act.t) if act is not None else None, L.ptr(out.t) if out is not None else None,
                out.plane_stride if out is not None else 0, int(c0), int(n), float(ig.LEAKY), L.stream()),
                "predict_flow backward (regions)")
            return
        if finalize is not None:
            act, out, c0, n = finalize
            L.check(L.lib().ufr_flow_head_planes_backward_finalize(L.ptr(gy), L.ptr(self.pf_w[k]), self.pf_w[k].shape[0], L.ptr(self.pf_G[k].t),
                                                                   self.pf_G[k].chunks, 0, chunks, self.B,
                                                                   src.H, src.W, int(accumulate), L.ptr(act.t), L.ptr(out.t), out.plane_stride,
                                                                   int(c0), int(n), float(ig.LEAKY), L.stream()),
                    "predict_flow backward + finalize")
            return
        L.check(L.lib().ufr_flow_head_planes_backward(L.ptr(gy), L.ptr(self.pf_w[k]), self.pf_w[k].shape[0], L.ptr(self.pf_G[k].t),
                                                      self.pf_G[k].chunks, 0, chunks, self.B,
                                                      src.H, src.W, int(accumulate), L.stream()), "predict_flow backward")

    def _pf_finish(self, k, upsample):
        """The split form's finishing sum -> flow[k]; with `upsample`, upsampled_flowK_to_K-1 from the same launch."""
        slices, n = self.pf_split[k]
        f = self.flow[k]
        dst, chunk = self.up_dst[k] if upsample else (None, 0)
        L.check(L.lib().ufr_flow_head_split_finish(L.ptr(self.pf_partials), n, slices, L.ptr(self.pf_b[k]), L.ptr(f), L.ptr(self.up_w[k]),
                                                   L.ptr(self.up_b[k]) if self.up_b[k] is not None else None,
                                                   L.ptr(dst.t) if upsample else None, dst.plane_stride if upsample else 0, chunk, self.B,
                                                   f.shape[2], f.shape[3], L.stream()), "predict_flow finish (split)")
        self._pf_pending = None

    def _up_forward(self, k):
        if self._pf_pending == k:
            self._pf_finish(k, upsample=True)
            return
        dst, chunk = self.up_dst[k]
        f = self.flow[k]
        L.check(L.lib().ufr_flow_up_planes_forward(L.ptr(f), L.ptr(self.up_w[k]), L.ptr(self.up_b[k]) if self.up_b[k] is not None else None,
                                                   L.ptr(dst.t), dst.plane_stride, chunk, self.B, f.shape[2], f.shape[3],
                                                   L.stream()), "upsampled_flow forward")

    def _deconv_tail(self, k):
        src, chunk0, chunks, Gd, out_chunk, (h, w) = self.tail_args[k]
        L.check(L.lib().ufr_deconv_flow_tail_backward_mfma(L.ptr(src.t), src.plane_stride, chunk0, chunks, L.ptr(self.tail_w[k]),
                                                           self.tail_w[k].shape[0], L.ptr(Gd.t), Gd.chunks, out_chunk, self.B, h, w, L.stream()),
                "deconv data gradient, flow channels")

    def _up_backward(self, k):
        G, chunk = self.up_G[k]
        f = self.g_flow[k]
        L.check(L.lib().ufr_flow_up_planes_backward(L.ptr(G.t), chunk, L.ptr(self.up_w[k]), L.ptr(f), self.B, f.shape[2],
                                                    f.shape[3], 0, L.stream()), "upsampled_flow backward")

    def _finalize(self, Gs, mask, out, chunk0, chunks):
        L.check(L.lib().ufr_grad_finalize(L.ptr(Gs.t), chunk0, L.ptr(mask.t), chunk0, L.ptr(out.t), out.plane_stride, chunk0,
                                          Gs.M, chunks, ig.LEAKY, L.stream()), "gradient finalize")

    # ------------------------------------------------------------------------------------------------ the schedule
    def _forward_trunk(self, c2: torch.Tensor, c3: torch.Tensor) -> torch.Tensor:
        """FlowNetS: (conv2 [B,128,H/4,W/4], conv3 [B,256,H/8,W/8]) -> flow2; conv3_1 reads conv3 directly."""
        L.require_hip(c2, "c2")
        L.require_hip(c3, "c3")
        self.cat2.load_nchw(c2, 0)
        self.in31.load_nchw(c3, 0)
        for name in ("conv3_1", "conv4", "conv4_1", "conv5", "conv5_1", "conv6", "conv6_1"):
            self.fwd[name]()
        self._pf_forward(6, defer=True)
        for k in (5, 4, 3, 2):
            self._up_forward(k + 1)
            self.fwd[f"deconv{k}"]()
            self._pf_forward(k, defer=True)
        return self.flow[2]

    def forward_cached(self, band=None, corr_changed: bool = True) -> torch.Tensor:
        """`forward` on the features the engine already holds (prefix_full / load_prefix_features + scatter_window_features)."""
        return self.forward(None, self._c3a, self._c3b, band, corr_changed=corr_changed)

    def forward(self, c2a: torch.Tensor | None, c3a: torch.Tensor, c3b: torch.Tensor, band=None,
                corr_changed: bool = True) -> torch.Tensor:
        """(conv2 of frame 1 [B,128,H/4,W/4], conv3 of both frames [B,256,H/8,W/8]) -> flow2 [B,2,H/4,W/4].
        `band` (band_conv.Band) with `incremental` set: the features differ from the previous call's only inside the
        prefix window, so conv_redir / conv3_1 / conv4 / conv4_1 recompute the band's columns only -- the plane buffers
        still hold the previous iteration's activations everywhere else.  The cost volume then recomputes only the entries
        whose cell or source cell lies in the window without its conv3 rim (`corr_changed`; False: every row and displacement
        of the columns within the correlation's reach of the window, the comparison leg of tests/test_corr_changed_gpu.py)."""
        if not self.siamese:
            return self._forward_trunk(c2a, c3a)
        for t, name in ((c3a, "c3a"), (c3b, "c3b")):
            L.require_hip(t, name)
        self._c3a, self._c3b = c3a, c3b
        inc = False
        if band is not None:
            self.attach_band(band)
            inc = bool(band.width and band.incremental and band.inc_layers)
        if c2a is not None:                      # features handed over in NCHW: convert; None: the planes are up to date
            L.require_hip(c2a, "c2a")
            self.cat2.load_nchw(c2a, 0)
            self.c3a_p.load_nchw(c3a, 0)
            self.c3b_p.load_nchw(c3b, 0)
        # submodules.py:124-138 (`correlate`: /C) + FlowNetC.py:139 LeakyReLU fused into the correlation's epilogue:
        # matrix cores, planes in, conv3_1's input planes out (correlation_planes.hip)
        if inc and band.cone_win is not None and band.cone_hw[1] // 8 <= 23:
            # later iterations of a call: only the window's neighbourhood of the volume changes
            if corr_changed:
                L.check(L.lib().ufr_corr_forward_planes_changed(L.ptr(self.c3a_p.t), L.ptr(self.c3b_p.t), self.c3a_p.plane_stride,
                                                                L.ptr(self.in31.t), self.in31.plane_stride, 1, self.B, 256, *self.grid[8],
                                                                21, 2, 1.0 / 256.0, ig.LEAKY, L.ptr(band.cone_win), 8,
                                                                band.cone_hw[0] // 8, band.cone_hw[1] // 8, self._win_m3, L.stream()),
                        "correlation forward (planes, changed)")
            else:
                L.check(L.lib().ufr_corr_forward_planes_window(L.ptr(self.c3a_p.t), L.ptr(self.c3b_p.t), self.c3a_p.plane_stride,
                                                               L.ptr(self.in31.t), self.in31.plane_stride, 1, self.B, 256, *self.grid[8],
                                                               21, 2, 1.0 / 256.0, ig.LEAKY, L.ptr(band.cone_win), 8,
                                                               band.cone_hw[1] // 8, L.stream()), "correlation forward (planes, window)")
        else:
            L.check(L.lib().ufr_corr_forward_planes(L.ptr(self.c3a_p.t), L.ptr(self.c3b_p.t), self.c3a_p.plane_stride,
                                                    L.ptr(self.in31.t), self.in31.plane_stride, 1, self.B, 256, *self.grid[8], 21, 2,
                                                    1.0 / 256.0, ig.LEAKY, L.stream()), "correlation forward (planes)")
        for name in ("conv_redir", "conv3_1", "conv4", "conv4_1"):
            (self.fwd_band if inc else self.fwd)[name]()
        for name in ("conv5", "conv5_1", "conv6", "conv6_1"):
            self.fwd[name]()
        # refinement (FlowNetC.py:162-183).  (deconvK beside predict_flow(K+1) -> upsampled_flow(K+1) on a second stream inside the
        # graph -- they read cat(K+1) and write disjoint chunks of catK -- measured no faster: 5.773 against 5.729 ms in one call,
        # gpurun r4_call23; the same for the small launches of the backward beside deconvK's data gradient, 5.904 against 5.874,
        # r4_call13: the ping-pong igemm holds every CU's LDS, the small launches wait for its tail either way.  One stream.)
        self._pf_forward(6, defer=True)
        for k in (5, 4, 3, 2):
            self._up_forward(k + 1)
            self.fwd[f"deconv{k}"]()
            self._pf_forward(k, defer=True)
        return self.flow[2]

    def backward(self, g_flow2: torch.Tensor, band=None, fused_window: bool = True, skip_unread: bool = True, tail_split: bool = True):
        """d loss / d flow2 -> (d/d conv2a, d/d conv3a, d/d conv3b), all NCHW float32 (static buffers).
        With a band: the data gradients of conv5, conv4_1, conv4, conv3_1 and conv_redir run on the band's columns and the
        correlation's adjoint on the window's cells (only those are read behind a windowed prefix).  When the band carries
        `g3_window` (the window-sized gradient of conv3, both frames: patch_attack.py) and `fused_window`, the correlation's
        adjoints are written there directly and the last two results are None.
        `skip_unread` (with a band and `fused_window`): gradients that only a banded or windowed launch reads are produced where
        it reads them (`_attach_unread`; predict_flow2's conv2 chunks straight into the window prefix's addend when that prefix
        runs on the engine) -- G_cat2[0:4] is then not written, G_cat3[0:8], G_cat4[0:16], G_in31 and G_c3a outside those regions
        keep stale values.  False: every gradient sum in full, as the autograd Function and the training path need them.
        `tail_split`: launches whose under-filled last round is re-cut over K (`_with_tail`) run in that form; False: their plain
        twins, today's launches (the A/B leg; the tail's rows differ by the order of a float32 sum)."""
        L.require_hip(g_flow2, "g_flow2")
        B = self.B
        run = lambda table, tag, name: (table[name] if tail_split else self.plain.get((tag, name), table[name]))()
        banded = band is not None and bool(band.width)
        if band is not None:
            self.attach_band(band)
        # level 2: predict_flow2 -> gradient of cat2 = [conv2a | deconv2 | flow3_up]
        gz = {2: (self.G_cat2, self.cat2, self.gz_cat2, 4, 2), 3: (self.G_cat3, self.cat3, self.gz_cat3, 8, 4),
              4: (self.G_cat4, self.cat4, self.gz_cat4, 16, 8), 5: (self.G_cat5, self.cat5, self.gz_cat5, 16, 16)}
        # predict_flowK's adjoint is the LAST contributor to deconvK's output gradient (deconv(K-1)'s data gradient and its two
        # flow columns come before it): LeakyReLU' and the split into gradient planes ride in its kernel instead of a
        # `grad_finalize` launch per level (UFR_FUSE_FINALIZE=0: the separate launches)
        fuse = os.environ.get("UFR_FUSE_FINALIZE", "1") != "0"
        fin = lambda k: (gz[k][1], gz[k][2], gz[k][3], gz[k][4]) if fuse else None
        eng_window = bool(fused_window and band is not None and getattr(band, "eng_window", False)
                          and getattr(self, "_wprefix", None) is not None)
        skip = bool(skip_unread and banded and fused_window and self.siamese)
        if skip and eng_window:                  # conv2's chunks on the window's cells, straight into conv3's addend: no gather
            P = self._wprefix
            wh, ww = P["hw"]
            self._pf_backward(2, g_flow2, accumulate=False, finalize=fin(2),
                              region=(4, L.UFR_PF_REGION_WINDOW, band.cone_win, 8, 4, wh // 4, ww // 4, band.g2_margin, P["G_gw2"]))
        else:
            self._pf_backward(2, g_flow2, accumulate=False, finalize=fin(2))
            if eng_window:                       # the window prefix runs on the engine: its conv2 gradient stays chunk-major
                self.window_gather_conv2_gradient(band.cone_win, band.g2_margin)
            else:
                self.G_cat2.to_nchw(128, 0, out=self.g_c2a)
        for k in (2, 3, 4):
            Gs, act, out, chunk0, chunks = gz[k]
            if not fuse:
                self._finalize(Gs, act, out, chunk0, chunks)      # LeakyReLU' of deconvK's output
            self._up_backward(k + 1)                               # -> d/d flow(K+1)
            region = None
            if skip and k + 1 in self._pf_band:                    # cat(K+1)'s leading chunks: only the band is read
                run(self.bwd_band, "band", f"deconv{k}")
                run(self.bwd_rest, "rest", f"deconv{k} rest")
                head, ls = self._pf_band[k + 1]
                region = (head, L.UFR_PF_REGION_BAND, band.win[:, 1], 8, ls, self.grid[ls][0], band.width // ls, 0, None)
            else:
                run(self.bwd, "full", f"deconv{k}")                # writes the gradient sum of cat(K+1)
            self._deconv_tail(k)
            self._pf_backward(k + 1, self.g_flow[k + 1], accumulate=True, finalize=fin(k + 1), region=region)
        Gs, act, out, chunk0, chunks = gz[5]
        if not fuse:
            self._finalize(Gs, act, out, chunk0, chunks)
        self._up_backward(6)
        self._pf_backward(6, self.g_flow[6], accumulate=False)      # G_c6 = predict_flow6^T; deconv5's adjoint adds to it
        for name in ("deconv5", "conv6_1", "conv6", "conv5_1"):
            run(self.bwd, "full", name)
        if not self.siamese:                    # FlowNetS trunk: conv3_1's data gradient IS d/d conv3
            for name in ("conv5", "conv4_1", "conv4", "conv3_1"):
                run(self.bwd, "full", name)
            self.G_in31.to_nchw(256, 0, out=self.g_c3a)
            return self.g_c2a, self.g_c3a, None
        for name in ("conv5", "conv4_1", "conv4", "conv3_1", "conv_redir"):
            if banded and not skip and name in self.bwd_band_wide:
                self.bwd_band_wide[name]()
            elif banded:
                run(self.bwd_band, "band", name)
            else:
                run(self.bwd, "full", name)
        # conv_redir's input and the correlation's two inputs
        gw = getattr(band, "g3_window", None) if (band is not None and fused_window) else None
        h8, w8 = self.grid[8]
        if gw is not None and band.cone_win is not None and band.cone_hw[1] // 8 <= 16 and w8 % 4 == 0:
            # windowed prefix behind the head: the cost volume's adjoints on the window's cells, on the matrix cores, straight
            # from the gradient sums into the window-sized gradient (correlation_window_mfma.hip)
            L.check(L.lib().ufr_corr_backward_window_fused(L.ptr(self._c3a), L.ptr(self._c3b), L.ptr(self.G_in31.t), 1, 1.0 / 256.0,
                                                           L.ptr(self.G_c3a.t), L.ptr(gw), B, 256, h8, w8, 21, 2,
                                                           L.ptr(band.cone_win), 8, band.cone_hw[0] // 8, band.cone_hw[1] // 8,
                                                           int(band.g3_margin), L.stream()), "correlation backward (window, fused)")
            return (None if eng_window else self.g_c2a), None, None
        self.G_c3a.to_nchw(256, 0, out=self.g_c3a_redir)
        self.G_in31.to_nchw(441, 1, scale=1.0 / 256.0, out=self.g_corr.view(B, 441, *self.grid[8]))
        self._corr_backward(self.g_corr, band)
        return (None if eng_window else self.g_c2a), self.g_c3a, self.g_c3b

    def _corr_backward(self, g_corr, band):
        from . import spatial_correlation_sampler_backend as correlation
        import ctypes as C
        h8, w8 = self.grid[8]
        if band is not None and band.cone_win is not None:
            L.check(L.lib().ufr_corr_backward_window(L.ptr(self._c3a), L.ptr(self._c3b), L.ptr(g_corr), L.ptr(self.g_c3a),
                                                     L.ptr(self.g_c3b), self.B, 256, h8, w8, 21, 2, L.ptr(band.cone_win), 8,
                                                     band.cone_hw[0] // 8, band.cone_hw[1] // 8, L.stream()),
                    "correlation backward (window)")
        else:
            p = correlation._params(1, 1, 21, 21, 0, 0, 1, 1, 2, 2, 1, 1)
            L.check(L.lib().ufr_corr_backward(L.ptr(self._c3a), L.ptr(self._c3b), L.ptr(g_corr), L.ptr(self.g_c3a),
                                              L.ptr(self.g_c3b), L.UFR_F32, self.B, 256, h8, w8, C.byref(p), L.stream()),
                    "correlation backward")
        self.g_c3a.add_(self.g_c3a_redir)

    # ------------------------------------------------------------------------------------------------ analysis
    # Feature-map capture and replacement (feature_maps.py; models/utils_model.py:160-626, models/FlowNetC.py:121-155 of the
    # reference).  After a forward every map the analysis scripts read sits in a plane buffer; a replaced map is a chunk range
    # the next forward does not recompute.
    REPLACEABLE = ("conv3a", "conv3b", "corr", "conv_redir", "conv3_1")          # what FlowNetC.py:121-155 reads
    _HEAD_SEGMENTS = {                               # key: (buffer attribute, first chunk, channels)
        "conv_redir": ("in31", 0, 32), "corr": ("in31", 1, 441), "conv3_1": ("cat3", 0, 256), "deconv3": ("cat3", 8, 128),
        "upsampled_flow4_to_3": ("cat3", 12, 2), "conv4": ("c4a", 0, 512), "conv4_1": ("cat4", 0, 512), "deconv4": ("cat4", 16, 256),
        "upsampled_flow5_to_4": ("cat4", 24, 2), "conv5": ("c5a", 0, 512), "conv5_1": ("cat5", 0, 512), "deconv5": ("cat5", 16, 512),
        "upsampled_flow6_to_5": ("cat5", 32, 2), "conv6": ("c6a", 0, 1024), "conv6_1": ("c6", 0, 1024), "deconv2": ("cat2", 4, 64),
        "upsampled_flow3_to_2": ("cat2", 6, 2)}
    _FLOW_KEYS = {"flow6": 6, "flow5": 5, "flow4": 4, "flow3": 3, "predict": 2}

    def segment_map(self, stem=None) -> dict:
        """{reference key: (Planes | NCHW float32 tensor, first chunk (channel), channels, first image, post-processing)} of where
        each of the 28 maps of models/utils_model.py:283-316 sits after a forward.  `stem` = the prefix's PlaneGraph
        (plane_graph.stem_graph over the 2B stacked frames: its c1 / c2 / c3 buffers hold conv1-3 of the first frames in images
        0 .. B-1 and of the second frames in B .. 2B-1); without it the six stem keys are left out.  Post-processing: "unleaky"
        for `corr` (in31 holds LeakyReLU(corr); the reference records the volume in front of the activation), else None."""
        if not self.siamese:
            raise RuntimeError("feature-map segments: the FlowNetC head (the FlowNetS trunk has no correlation)")
        seg = {}
        if stem is not None:
            for lvl, cn in ((1, 64), (2, 128), (3, 256)):
                p = stem.bufs[f"c{lvl}"].planes
                seg[f"conv{lvl}a"], seg[f"conv{lvl}b"] = (p, 0, cn, 0, None), (p, 0, cn, self.B, None)
        for key, (buf, c0, cn) in self._HEAD_SEGMENTS.items():
            seg[key] = (getattr(self, buf), c0, cn, 0, "unleaky" if key == "corr" else None)
        for key, k in self._FLOW_KEYS.items():
            seg[key] = (self.flow[k], 0, 2, 0, None)
        return seg

    def capture(self, keys=None, stem=None) -> dict:
        """{key: NCHW float32 [B,C,h,w]} of the last forward's maps, copies (`Planes.to_nchw`: p0 + p1 + p2, exact).
        `corr` is un-leakied from conv3_1's input planes, not recomputed by the float32 correlation operator: a negative entry x
        becomes a float32 y next to x / 0.1 with fl(y * 0.1) == x (`_unleaky`; x is such a product, so one exists within an ulp),
        which `Planes.load_nchw(slope=LEAKY)` maps back to the same planes bit for bit."""
        seg = self.segment_map(stem)
        out = {}
        for key in (list(seg) if keys is None else keys):
            if key not in seg:
                raise KeyError(f"capture: {key!r} is not a feature map of this forward ({', '.join(seg)})")
            src, c0, cn, img0, post = seg[key]
            if isinstance(src, ig.Planes):
                t = src.to_nchw(cn, c0)[img0:img0 + self.B]
                out[key] = _unleaky(t, ig.LEAKY) if post == "unleaky" else (t if t.shape[0] == src.B else t.clone())
            else:
                out[key] = src[:, c0:c0 + cn].clone()
        return out

    def forward_replaced(self, c2a, c3a, c3b, overwrite=None, keep=(), computed=None) -> torch.Tensor:
        """`forward` (full frame, no band) with feature maps replaced, models/FlowNetC.py:121-155: `overwrite` = {key: NCHW
        float32 [B,C,h,w]} is loaded into the key's chunks (conv3a / conv3b only as a pair, in front of the correlation and
        conv_redir; corr in front of the LeakyReLU; conv_redir; conv3_1) and `keep` names keys whose chunks still hold a DONOR
        forward's values on this engine: they are left as they are (the zero-copy form).  The launch that would have produced a
        replaced segment is skipped -- unless `computed` (a dict) is given: it then runs first and its result is stored there,
        because the reference hands back the computed map even where it overwrites it.  Keys outside REPLACEABLE are ignored, as
        the reference ignores them.  -> flow2 (the static buffer)."""
        if not self.siamese:
            raise RuntimeError("feature-map replacement: the FlowNetC head")
        ow = {k: v for k, v in (overwrite or {}).items() if k in self.REPLACEABLE}
        keep = {k for k in keep if k in self.REPLACEABLE and k not in ow}
        pair = lambda d: "conv3a" in d and "conv3b" in d
        for t, name in ((c2a, "c2a"), (c3a, "c3a"), (c3b, "c3b")):
            L.require_hip(t, name)
        self.generation = getattr(self, "generation", 0) + 1          # a pending autograd backward of this engine is stale now
        self._c3a, self._c3b = c3a, c3b
        self.cat2.load_nchw(c2a, 0)
        if pair(ow):
            self.c3a_p.load_nchw(ow["conv3a"].contiguous(), 0)
            self.c3b_p.load_nchw(ow["conv3b"].contiguous(), 0)
        elif not pair(keep):
            self.c3a_p.load_nchw(c3a, 0)
            self.c3b_p.load_nchw(c3b, 0)

        def stage(key, launch, load):
            if key not in ow and key not in keep:
                launch()
                return
            if computed is not None:
                held = self.capture([key]) if key in keep else None          # the donor's chunks survive the computed pass
                launch()
                computed[key] = self.capture([key])[key]
                if held is not None:
                    load(held[key])
            if key in ow:
                load(ow[key].contiguous())

        corr = lambda: L.check(L.lib().ufr_corr_forward_planes(
            L.ptr(self.c3a_p.t), L.ptr(self.c3b_p.t), self.c3a_p.plane_stride, L.ptr(self.in31.t), self.in31.plane_stride, 1, self.B,
            256, *self.grid[8], 21, 2, 1.0 / 256.0, ig.LEAKY, L.stream()), "correlation forward (planes)")
        stage("corr", corr, lambda v: self.in31.load_nchw(v, 1, slope=ig.LEAKY))
        stage("conv_redir", self.fwd["conv_redir"], lambda v: self.in31.load_nchw(v, 0))
        stage("conv3_1", self.fwd["conv3_1"], lambda v: self.cat3.load_nchw(v, 0))
        for name in ("conv4", "conv4_1", "conv5", "conv5_1", "conv6", "conv6_1"):
            self.fwd[name]()
        self._pf_forward(6, defer=True)
        for k in (5, 4, 3, 2):
            self._up_forward(k + 1)
            self.fwd[f"deconv{k}"]()
            self._pf_forward(k, defer=True)
        return self.flow[2]


def _unleaky(x: torch.Tensor, slope: float) -> torch.Tensor:
    """The float32 y in front of LeakyReLU(slope) of x = fl(y * slope) for x < 0: among the five floats around fl(x / slope), the
    one of smallest magnitude whose product with `slope` rounds back to x (fl(x / slope) when none does) -- the rule of
    csrc/feature_stats.hip `undo_leaky`, so the statistics kernel sums exactly these values."""
    s = torch.tensor(slope, dtype=torch.float32, device=x.device)
    y0 = x / s
    best, found = y0.clone(), x >= 0
    bits = y0.view(torch.int32)
    for d in (-2, -1, 0, 1, 2):
        cand = (bits + d).view(torch.float32)
        ok = ~found & (cand * s == x)
        best = torch.where(ok, cand, best)
        found = found | ok
    return torch.where(x < 0, best, x)


class _EngineHead(torch.autograd.Function):
    """The engine keeps its activations in static buffers, so a forward is only differentiable until the NEXT forward of
    the same engine: `generation` counts forwards, backward refuses a stale one (two grad-mode forwards of one shape before
    a backward -- e.g. loss(flow(a), flow(b)) -- would otherwise silently differentiate the second call twice)."""

    @staticmethod
    def forward(ctx, c2a, c3a, c3b, engine, band):
        ctx.engine, ctx.band = engine, band
        engine.generation = ctx.generation = getattr(engine, "generation", 0) + 1
        # the engine's flow2 is a static buffer: hand autograd its own (2-channel, tiny) tensor -- or, inside a composition that
        # declared every consumer immediate (`_lib.static_handoff`), an alias of it
        ctx.static, ctx.static_grads = L.static_ok(), L.static_grads_ok()
        flow2 = engine.forward(c2a.contiguous(), c3a.contiguous(), c3b.contiguous() if c3b is not None else None, band)
        return flow2.detach() if ctx.static else flow2.clone()

    @staticmethod
    def backward(ctx, g_flow2):
        if ctx.engine.generation != ctx.generation:
            raise RuntimeError("FlowNetC head engine: another forward of this network (same batch and frame size) ran before this "
                               "backward; its activations are gone.  Call backward() before the next forward, or set "
                               "UFR_ENGINE=0 for interleaved forwards")
        g2a, g3a, g3b = ctx.engine.backward(g_flow2.contiguous(), ctx.band, fused_window=False)
        if ctx.static_grads:
            return g2a, g3a, g3b, None, None
        # static buffers as well: autograd (and a caller who retains .grad) gets its own copies
        return (g2a.clone() if g2a is not None else None, g3a.clone() if g3a is not None else None,
                g3b.clone() if g3b is not None else None, None, None)


def _weights_stamp(net):
    """(storage address, in-place version) of every parameter: the engine packs the weights once, so it must notice a
    `load_state_dict` / optimiser step on the module it was built from."""
    return tuple((p.data_ptr(), p._version) for p in net.parameters())


def get_engine(net, B: int, H: int, W: int, device) -> FlowNetCHeadEngine:
    """One engine per batch / frame size, cached on the module; rebuilt when the module's weights have changed since."""
    key = (int(B), int(H), int(W), str(torch.device(device)))
    cache = _engine_cache(net, "_ufr_head_engines")
    stamp = _weights_stamp(net)
    eng = cache.get(key)
    if eng is None or eng.weights_stamp != stamp:
        eng = cache[key] = FlowNetCHeadEngine(net, B, H, W, device)
        eng.weights_stamp = stamp
    return eng


def engine_head(net, c2a, c3a, c3b, band=None):
    """flow2 of FlowNetC's head on the native engine, as an autograd Function of the NCHW features."""
    B, _, h4, w4 = c2a.shape
    return _EngineHead.apply(c2a, c3a, c3b, get_engine(net, B, h4 * 4, w4 * 4, c2a.device), band)
