"""Column-band data gradients for the convolutions behind a windowed prefix (patch_attack.py, cone.py).

When FlowNetC's conv1-3 run on a window around the patch, the rest of the network still needs its adjoint
only where activations depend on that window.  Behind the 21x21 stride-2 correlation that is every row but
less than half of the columns for conv3_1 / conv4 / conv4_1 / conv5 (the most expensive data gradients of
the head).  `band_conv2d` is `F.conv2d` whose backward computes the input gradient on a column band only:
    gather the band of grad_output (origin in device memory: one captured graph serves every placement)
    -> MIOpen backward-data on the band -> scatter the exact columns into a zeroed full-size gradient.
Columns within `kernel - 1 - padding` cells of an interior band edge miss contributions from outside the
band and are left zero; the band is sized (patch_attack.py) so that they are never needed.  Weights get no
gradient: the attack differentiates with respect to the frames only.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib as L


CORR_REACH = 160      # pixels: the 21 x 21 correlation with dilation 2 at 1/8 resolution reaches 20 cells to either side


def corr_band_width(ww: int, reach: int = CORR_REACH) -> int:
    """Width in pixels (a multiple of 32) of the narrowest column band that holds a `ww`-pixel window and `reach` pixels to
    either side of it for every placement, an origin clamped at a frame edge included."""
    return -(-(int(ww) + 2 * reach) // 32) * 32


def corr_band_origin(x0, width: int, W: int, reach: int = CORR_REACH):
    """First pixel column of that band for a window that starts at `x0` (a multiple of 8: an int, or an int32 tensor of
    one origin per pair): `reach` to the left of the window, inside the frame.  A multiple of 8 when x0, reach, W and width are;
    [origin, origin + width) holds [x0 - reach, x0 + ww + reach) cut to the frame for every ww <= width - 2 reach."""
    lo = x0 - reach
    return lo.clamp(0, W - width) if torch.is_tensor(lo) else min(max(lo, 0), W - width)


class Band:
    """A per-sample column band: `win` int32 [B,8] with win[:,1] = first pixel column (win[:,0] = 0), `width`
    pixels wide; both multiples of every level stride the band is used at.  `corr_width` (0 = none): a second, narrower band
    inside it, from win[:,2], for the two data gradients that only the window's correlation adjoint reads (multiples of 8)."""

    def __init__(self, win: torch.Tensor, width: int, cone_win: torch.Tensor | None = None, cone_hw=None):
        self.win, self.width, self.corr_width = win, int(width), 0
        # the prefix window itself (pixels): the correlation's adjoint is needed on its cells only
        self.cone_win, self.cone_hw = cone_win, cone_hw
        # incremental forward (second and later iterations of an attack() call): the blocks named in
        # `inc_layers` recompute the band's columns only and paste them into `caches[name]`, the activations of
        # the previous iteration; `incremental` is switched by the step between its two captured graphs
        self.inc_layers, self.incremental, self.caches = (), False, {}


class _WindowCorrelation(torch.autograd.Function):
    """spatial_correlation_sample(kernel 1, stride 1, padding 0) whose backward fills only the cells of the
    prefix window (csrc/correlation_window.hip); everything else of both input gradients is zero."""

    @staticmethod
    def forward(ctx, input1, input2, patch, dilation_patch, band, in_stride):
        from . import spatial_correlation_sampler_backend as correlation
        ctx.save_for_backward(input1, input2)
        ctx.meta = (int(patch), int(dilation_patch), band, int(in_stride))
        return correlation.forward(input1, input2, 1, 1, patch, patch, 0, 0, 1, 1, dilation_patch, dilation_patch, 1, 1)

    @staticmethod
    def backward(ctx, gout):
        input1, input2 = ctx.saved_tensors
        patch, dil, band, ls = ctx.meta
        B, Cn, H, W = input1.shape
        g1, g2 = torch.empty_like(input1), torch.empty_like(input2)
        L.check(L.lib().ufr_corr_backward_window(L.ptr(input1), L.ptr(input2), L.ptr(gout.contiguous()), L.ptr(g1), L.ptr(g2),
                                                 B, Cn, H, W, patch, dil, L.ptr(band.cone_win), ls, band.cone_hw[0] // ls,
                                                 band.cone_hw[1] // ls, L.stream()), "corr backward window")
        return g1, g2, None, None, None, None


def window_correlation(input1, input2, patch, dilation_patch, band: Band, in_stride: int):
    """Cost volume [B,P,P,H,W] of two feature maps that vary only inside `band.cone_win`."""
    if input1.dtype != torch.float32 or not input1.is_contiguous() or not input2.is_contiguous():
        raise TypeError("window_correlation: contiguous float32 feature maps")
    return _WindowCorrelation.apply(input1, input2, patch, dilation_patch, band, in_stride)


def _conv_forward(x, weight, s, p):
    """conv2d without bias inside the band Functions (no autograd here)."""
    return F.conv2d(x, weight, None, s, p)


class _BandConv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, band, in_stride):
        ctx.save_for_backward(weight)
        ctx.meta = (tuple(x.shape), int(stride), int(padding), band, int(in_stride))
        return F.conv2d(x, weight, bias, stride, padding)

    @staticmethod
    def backward(ctx, gy):
        (weight,) = ctx.saved_tensors
        in_shape, s, p, band, ls_in = ctx.meta
        return _band_data_gradient(gy, weight, in_shape, s, p, band, ls_in), None, None, None, None, None, None


def _band_data_gradient(gy, weight, in_shape, s, p, band, ls_in):
    """Input gradient of conv2d(weight, stride s, padding p) on the band's columns, zero elsewhere."""
    B, Cin, Hi, Wi = in_shape
    k = weight.shape[-1]
    ls_out = ls_in * s
    wib, wob = band.width // ls_in, band.width // ls_out
    _, Cout, Ho, Wo = gy.shape
    lib, st = L.lib(), L.stream()
    gy = gy.contiguous()
    gyb = torch.empty(B, Cout, Ho, wob, dtype=gy.dtype, device=gy.device)
    L.check(lib.ufr_window_gather(L.ptr(gy), L.ptr(gyb), L.ptr(band.win), B, B, Cout, Ho, Wo, Ho, wob, ls_out, 0, st),
            "band gather")
    gxb = torch.ops.aten.convolution_backward(gyb, gyb.new_empty((B, Cin, Hi, wib)), weight, None, (s, s), (p, p),
                                              (1, 1), False, (0, 0), 1, (True, False, False))[0]
    gx = torch.zeros(B, Cin, Hi, Wi, dtype=gy.dtype, device=gy.device)
    L.check(lib.ufr_window_scatter(L.ptr(gxb.contiguous()), L.ptr(gx), L.ptr(band.win), B, B, Cin, Hi, Wi, Hi, wib,
                                   ls_in, k - 1 - p, st), "band scatter")
    return gx


class _IncrementalConvLeaky(torch.autograd.Function):
    """A conv + bias + LeakyReLU block whose input differs from the previous iteration's only inside the band:
    gather the band of x, convolve, apply the epilogue, paste the exact columns into `cache` (the previous
    iteration's activations, updated in place and returned).  Backward = the banded data gradient."""

    @staticmethod
    def forward(ctx, x, cache, weight, bias, stride, padding, slope, band, in_stride):
        B, Cin, Hi, Wi = x.shape
        s, p, k = int(stride), int(padding), weight.shape[-1]
        ls_out = in_stride * s
        wib, wob = band.width // in_stride, band.width // ls_out
        _, Cout, Ho, Wo = cache.shape
        lib, st = L.lib(), L.stream()
        xb = torch.empty(B, Cin, Hi, wib, dtype=x.dtype, device=x.device)
        L.check(lib.ufr_window_gather(L.ptr(x), L.ptr(xb), L.ptr(band.win), B, B, Cin, Hi, Wi, Hi, wib, in_stride, 0, st),
                "band gather")
        yb = _conv_forward(xb, weight, s, p).contiguous()
        L.check(lib.ufr_bias_leaky_forward(L.ptr(yb), L.ptr(bias), B, Cout, Ho * wob, float(slope), st), "bias leaky")
        L.check(lib.ufr_window_scatter(L.ptr(yb), L.ptr(cache), L.ptr(band.win), B, B, Cout, Ho, Wo, Ho, wob, ls_out,
                                       k - 1 - p, st), "band paste")
        ctx.mark_dirty(cache)
        ctx.save_for_backward(weight, cache)
        ctx.meta = ((B, Cin, Hi, Wi), s, p, float(slope), band, int(in_stride))
        return cache

    @staticmethod
    def backward(ctx, gy):
        weight, y = ctx.saved_tensors
        in_shape, s, p, slope, band, ls_in = ctx.meta
        gy = gy.contiguous()
        g_pre = torch.empty_like(gy)
        L.check(L.lib().ufr_leaky_backward(L.ptr(y), L.ptr(gy), L.ptr(g_pre), gy.numel(), slope, L.stream()),
                "leaky backward")
        return _band_data_gradient(g_pre, weight, in_shape, s, p, band, ls_in), None, None, None, None, None, None, None, None


class _BiasLeaky(torch.autograd.Function):
    """y = LeakyReLU(x + bias[c]) in place on x (csrc/bias_act.hip); no gradient for the frozen bias."""

    @staticmethod
    def forward(ctx, x, bias, slope):
        B, Cn = x.shape[0], x.shape[1]
        if bias is None:                       # (a block without bias: the Robust FlowNetC family's deconvolutions)
            bias = torch.zeros(Cn, dtype=x.dtype, device=x.device)
        L.check(L.lib().ufr_bias_leaky_forward(L.ptr(x), L.ptr(bias), B, Cn, x.numel() // (B * Cn), float(slope),
                                               L.stream()), "bias leaky forward")
        ctx.mark_dirty(x)
        ctx.save_for_backward(x)
        ctx.slope = float(slope)
        return x

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gy = gy.contiguous()
        gx = torch.empty_like(gy)
        L.check(L.lib().ufr_leaky_backward(L.ptr(y), L.ptr(gy), L.ptr(gx), gy.numel(), ctx.slope, L.stream()),
                "leaky backward")
        return gx, None, None


class _Conv3x3C2(torch.autograd.Function):
    """Conv2d(Cin, 2, 3, 1, 1) with frozen parameters (csrc/small_cout.hip)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        B, Cin, H, W = x.shape
        y = torch.empty(B, 2, H, W, dtype=x.dtype, device=x.device)
        n_ws = L.lib().ufr_conv3x3_c2_workspace_floats(B, Cin, H, W)
        ws = torch.empty(n_ws, dtype=x.dtype, device=x.device) if n_ws else None
        L.check(L.lib().ufr_conv3x3_c2_forward(L.ptr(x), L.ptr(weight), L.ptr(bias), L.ptr(y), L.ptr(ws) if n_ws else None,
                                               B, Cin, H, W, L.stream()), "conv3x3 c2 forward")
        ctx.save_for_backward(weight)
        ctx.shape = (B, Cin, H, W)
        return y

    @staticmethod
    def backward(ctx, gy):
        (weight,) = ctx.saved_tensors
        B, Cin, H, W = ctx.shape
        gx = torch.empty(B, Cin, H, W, dtype=gy.dtype, device=gy.device)
        L.check(L.lib().ufr_conv3x3_c2_backward_data(L.ptr(gy.contiguous()), L.ptr(weight), L.ptr(gx), B, Cin, H, W,
                                                     L.stream()), "conv3x3 c2 backward")
        return gx, None, None


class _Deconv4x4C2(torch.autograd.Function):
    """ConvTranspose2d(2, 2, 4, 2, 1) with frozen parameters (csrc/small_cout.hip)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        B, _, H, W = x.shape
        y = torch.empty(B, 2, 2 * H, 2 * W, dtype=x.dtype, device=x.device)
        L.check(L.lib().ufr_deconv4x4s2_c2_forward(L.ptr(x), L.ptr(weight), L.ptr(bias) if bias is not None else None,
                                                   L.ptr(y), B, H, W, L.stream()), "deconv4x4s2 c2 forward")
        ctx.save_for_backward(weight)
        ctx.shape = (B, H, W)
        return y

    @staticmethod
    def backward(ctx, gy):
        (weight,) = ctx.saved_tensors
        B, H, W = ctx.shape
        gx = torch.empty(B, 2, H, W, dtype=gy.dtype, device=gy.device)
        L.check(L.lib().ufr_deconv4x4s2_c2_backward_data(L.ptr(gy.contiguous()), L.ptr(weight), L.ptr(gx), B, H, W,
                                                         L.stream()), "deconv4x4s2 c2 backward")
        return gx, None, None


def _frozen(mod):
    return not (mod.weight.requires_grad or (mod.bias is not None and mod.bias.requires_grad))


# ---------------------------------------------------------------------------------------------------- native training
class native_training:
    """`with band_conv.native_training():` -- opt-in: inside, `conv_leaky`, `flow_head` and `flow_upsample` run a block whose
    parameters require gradients on the hand-written kernels (HIP float32 tensors, autograd on): forward and data gradient on the
    igemm (csrc/igemm.hip), weight and bias gradient on csrc/igemm_wgrad.hip, instead of `F.conv2d` / `F.conv_transpose2d` on
    the vendor library.  These are the convolutions of the fine-tuning iteration of adversarial training (training/train.py:225-282
    of the reference); its loss, gradient clipping, AdamW and the iteration itself are `training.py` (`finetune_step`).
    Scope: the FlowNetC family and PWC-Net.  `FlowNetC` is fully served (every block of its stem and head); the Robust FlowNetC
    family and FlowNetS come along as far as their blocks go through these three helpers (square kernels up to 5 x 5, or the
    7 x 7 stride-2 stem on three channels; stride 1 or 2; a square dilation on stride-1 layers only; no groups;
    ConvTranspose2d(., ., 4, 2, 1) without dilation) -- a block outside that raises NotImplementedError instead of leaving the
    kernels quietly.  `PWCDCNet` is fully served on frames whose sides are multiples of 64 (which PWC-Net needs anyway: six
    halvings): the pyramid, the DenseNet decoder, `predict_flow*`, `deconv*`, `upfeat*` (ConvTranspose2d(Cin, 2, 4, 2, 1), a
    `FlowUpsample`) and the context network with its dilations 2, 4, 8 and 16; its cost volume and warp have native adjoints of
    their own.  Each block converts NCHW <-> planes on both sides.  RAFT and FlowNet2 remain out of scope: their training mode
    stays on torch operators.  Thread-local and off by default; outside the context nothing changes.  Inside it
    `_lib.engine_gate` neither warns nor counts a forward that the attack's engines decline for training mode or trainable
    parameters.  Weights are re-split on every call (the optimiser changes them)."""

    def __enter__(self):
        L._NATIVE_TRAINING.depth = getattr(L._NATIVE_TRAINING, "depth", 0) + 1
        return self

    def __exit__(self, *exc):
        L._NATIVE_TRAINING.depth -= 1


def _native_trains(x, mod) -> bool:
    return (L.native_training_on() and x.is_cuda and x.dtype == torch.float32 and torch.is_grad_enabled() and not _frozen(mod))


class _NativeTrainConv(torch.autograd.Function):
    """Conv2d / ConvTranspose2d(., ., 4, 2, 1) + bias + LeakyReLU(slope) (slope 1: no activation) with gradients for the input, the
    weight and the bias, every convolution on the hand-written kernels."""

    @staticmethod
    def forward(ctx, x, weight, bias, transposed, stride, padding, slope, dilation=1):
        from . import igemm as ig
        B, Cin, H, W = x.shape
        dev = x.device
        k = int(weight.shape[-1])
        cout = int(weight.shape[1] if transposed else weight.shape[0])
        b = bias.detach().float().contiguous() if bias is not None else torch.zeros(cout, dtype=torch.float32, device=dev)
        if transposed:
            Ho, Wo = 2 * H, 2 * W
            wi = ig.deconv_forward_weights(weight, padding)
            rows = (H, W)
        else:
            span = (k - 1) * dilation + 1
            Ho, Wo = (H + 2 * padding - span) // stride + 1, (W + 2 * padding - span) // stride + 1
            rows = (Ho, Wo)
        out = ig.Planes(B, Ho, Wo, ig.pad32(cout) // 32, dev)
        if not transposed and k * k > L.UFR_IGEMM_MAX_TAPS:
            # the 7 x 7 stride-2 stem on three channels: eight taps over the pixel-unshuffled, column-paired planes (igemm.conv1_packed_weights)
            packed = ig.Planes(B, H // 2 + 3, W // 2 + 2, 1, dev)
            zero_mean = torch.zeros(3, dtype=torch.float64, device=dev)
            L.check(L.lib().ufr_conv1_pack_planes(L.ptr(x), None, L.ptr(packed.t), packed.plane_stride, B, 0, H, W, L.ptr(zero_mean),
                                                  L.stream()), "conv1 pack")
            ig.make_launch(ig.conv1_packed_weights(weight), packed, 0, rows, rows, out_planes=out, bias=b, slope=slope, variant=2,
                           products=6)()
        else:
            if not transposed:
                wi = ig.conv_forward_weights(weight, stride, padding, dilation)
            xp = ig.Planes(B, H, W, ig.pad32(Cin) // 32, dev).load_nchw(x)
            ig.make_launch(wi, xp, 0, rows, (Ho, Wo), out_planes=out, bias=b, slope=slope, products=6)()
        y = out.to_nchw(cout)
        ctx.save_for_backward(x, weight, y)
        ctx.meta = (bool(transposed), int(stride), int(padding), float(slope), bias is not None, int(dilation))
        return y

    @staticmethod
    def backward(ctx, gy):
        from . import igemm as ig
        x, weight, y = ctx.saved_tensors
        transposed, stride, padding, slope, has_bias, dilation = ctx.meta
        B, Cin, H, W = x.shape
        _, cout, Ho, Wo = y.shape
        k, dev = int(weight.shape[-1]), x.device
        gy = gy.contiguous()
        gp = ig.Planes(B, Ho, Wo, ig.pad32(cout) // 32, dev)          # gy * LeakyReLU'(out)
        if slope != 1.0:
            L.check(L.lib().ufr_nchw_grad_to_planes(L.ptr(gy), L.ptr(y), L.ptr(gp.t), gp.plane_stride, 0, B, cout, Ho, Wo, slope,
                                                    L.stream()), "gradient -> planes")
        else:
            gp.load_nchw(gy)
        gx = None
        if ctx.needs_input_grad[0]:
            wi = ig.deconv_backward_weights(weight, padding) if transposed else ig.conv_backward_weights(weight, stride, padding, dilation)
            gs = ig.GradSum(B, H, W, ig.pad32(Cin) // 32, dev)
            # (a stride-2 data gradient writes the input grid in four phases from the gy grid: rows = the gy grid)
            rows = (Ho, Wo) if (not transposed and stride == 2) else (H, W)
            ig.make_launch(wi, gp, 0, rows, (H, W), out_f32=gs, products=6)()
            gx = gs.to_nchw(Cin)
        gw = gb = None
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            xp = ig.Planes(B, H, W, ig.pad32(Cin) // 32, dev).load_nchw(x)
            gw = torch.empty_like(weight, memory_format=torch.contiguous_format)
            gb = torch.empty(cout, dtype=torch.float32, device=dev) if has_bias and ctx.needs_input_grad[2] else None
            ig.make_wgrad_launch(xp, 0, Cin, gp, 0, cout, k, stride, padding, transposed=transposed, dw=gw, db=gb, dilation=dilation)()
            if not ctx.needs_input_grad[1]:
                gw = None
        return gx, gw, gb, None, None, None, None, None


def _native_train_block(x, conv, slope: float):
    """The block `conv` (+ bias + LeakyReLU(slope)) on `_NativeTrainConv`; geometry outside its scope is an error, not a fallback."""
    transposed = isinstance(conv, torch.nn.ConvTranspose2d)
    k, s, p, d = conv.kernel_size, conv.stride, conv.padding, conv.dilation
    ok = (k[0] == k[1] and s[0] == s[1] and p[0] == p[1] and d[0] == d[1] and d[0] >= 1 and conv.groups == 1
          and conv.weight.dtype == torch.float32)
    # a dilation: stride-1 convolutions of up to 5 x 5 only (what the igemm data gradient takes) -- PWC-Net's dc_conv2 .. dc_conv5
    ok = ok and (d[0] == 1 or (not transposed and s[0] == 1 and k[0] * k[1] <= L.UFR_IGEMM_MAX_TAPS
                               and min(x.shape[2], x.shape[3]) + 2 * p[0] >= (k[0] - 1) * d[0] + 1))
    B, Cin, H, W = x.shape
    if transposed:
        ok = ok and (k[0], s[0], p[0]) == (4, 2, 1) and conv.output_padding == (0, 0)
    elif ok and k[0] * k[1] > L.UFR_IGEMM_MAX_TAPS:
        ok = (Cin, k[0], s[0], p[0]) == (3, 7, 2, 3) and H % 2 == 0 and W % 2 == 0 and not x.requires_grad
    elif ok:
        ok = s[0] == 1 or (s[0] == 2 and 0 <= 2 + 2 * p[0] - k[0] <= 1 and H % 2 == 0 and W % 2 == 0)
    if not ok:
        raise NotImplementedError(f"band_conv.native_training: {conv} on a {H} x {W} input is outside the native training path "
                                  "(square kernels up to 5 x 5 or the 7 x 7 stride-2 stem on three channels, stride 1 or 2 on even "
                                  "sides, a square dilation at stride 1 only (a strided or transposed layer takes none), no groups, "
                                  "ConvTranspose2d(., ., 4, 2, 1))")
    return _NativeTrainConv.apply(x.contiguous(), conv.weight, conv.bias, transposed, s[0], p[0], float(slope), d[0])


def flow_head(x, conv: torch.nn.Conv2d):
    """`predict_flow*` (Conv2d(Cin, 2, 3, 1, 1), models/submodules.py:85-86): one pass over x on the device when
    the parameters are frozen (or autograd is off); the module itself otherwise."""
    ok = (x.is_cuda and x.dtype == torch.float32 and conv.out_channels == 2 and conv.kernel_size == (3, 3)
          and conv.stride == (1, 1) and conv.padding == (1, 1) and conv.dilation == (1, 1) and conv.groups == 1
          and conv.bias is not None and (_frozen(conv) or not torch.is_grad_enabled()))
    if ok:
        return _Conv3x3C2.apply(x.contiguous(), conv.weight, conv.bias)
    if _native_trains(x, conv):
        return _native_train_block(x, conv, 1.0)
    return F.conv2d(x, conv.weight, conv.bias, conv.stride, conv.padding, conv.dilation, conv.groups)


def flow_upsample(x, deconv: torch.nn.ConvTranspose2d):
    """`upsampled_flow*_to_*` (ConvTranspose2d(2, 2, 4, 2, 1), models/submodules.py:89-90), same conditions."""
    ok = (x.is_cuda and x.dtype == torch.float32 and deconv.in_channels == 2 and deconv.out_channels == 2
          and deconv.kernel_size == (4, 4) and deconv.stride == (2, 2) and deconv.padding == (1, 1)
          and deconv.output_padding == (0, 0) and deconv.dilation == (1, 1) and deconv.groups == 1
          and (_frozen(deconv) or not torch.is_grad_enabled()))
    if ok:
        return _Deconv4x4C2.apply(x.contiguous(), deconv.weight, deconv.bias)
    if _native_trains(x, deconv):
        return _native_train_block(x, deconv, 1.0)
    return F.conv_transpose2d(x, deconv.weight, deconv.bias, deconv.stride, deconv.padding, deconv.output_padding,
                              deconv.groups, deconv.dilation)


class FlowHead(torch.nn.Conv2d):
    """`predict_flow*`: a Conv2d (same parameter names, so checkpoints load unchanged) that runs `flow_head`."""

    def forward(self, x):
        return flow_head(x, self)


class FlowUpsample(torch.nn.ConvTranspose2d):
    """`upsampled_flow*` / PWC-Net's `deconv*` and `upfeat*`: a ConvTranspose2d that runs `flow_upsample` (more than two input
    channels: the native training block inside `native_training()`, `F.conv_transpose2d` with the module's own arguments otherwise)."""

    def forward(self, x, output_size=None):
        return flow_upsample(x, self)


def conv_relu(x, conv: torch.nn.Conv2d):
    """`F.relu(conv(x))` of RAFT's motion encoder and heads (models/raft/update.py): convolution without bias,
    then bias + ReLU as one in-place pass, under the same conditions as `conv_leaky`."""
    if (x.is_cuda and x.dtype == torch.float32 and conv.bias is not None
            and (_frozen(conv) or not torch.is_grad_enabled())):
        y = band_conv2d(x, conv, None, 0, with_bias=False)
        return _BiasLeaky.apply(y.contiguous(), conv.bias, 0.0)
    return F.relu(conv(x))


def conv_leaky(x, seq, band: Band | None = None, in_stride: int = 0, name: str | None = None):
    """The reference's `conv` / `deconv` block (models/submodules.py:18-46, :75-82) = Sequential(Conv2d or
    ConvTranspose2d with bias, LeakyReLU): on a HIP float32 tensor the convolution runs without bias and
    bias + activation are one in-place pass; with frozen parameters only.  Otherwise the plain modules.
    A block listed in `band.inc_layers` keeps its activations in `band.caches[name]` and, when
    `band.incremental` is set, recomputes the band's columns only."""
    conv, act = seq[0], seq[1]
    frozen = not (conv.weight.requires_grad or (conv.bias is not None and conv.bias.requires_grad))
    fused = (x.is_cuda and x.dtype == torch.float32 and act.negative_slope > 0
             and (frozen or not torch.is_grad_enabled()))
    if not fused and act.negative_slope > 0 and _native_trains(x, conv):
        return _native_train_block(x, conv, act.negative_slope)
    if not fused:
        return act(band_conv2d(x, conv, band, in_stride)) if isinstance(conv, torch.nn.Conv2d) else act(conv(x))
    tracked = (band is not None and band.width and name in band.inc_layers and x.requires_grad
               and isinstance(conv, torch.nn.Conv2d))
    if tracked and band.incremental:
        # a detached alias: the Function marks its cache argument dirty, the stored tensor itself stays a plain buffer
        return _IncrementalConvLeaky.apply(x.contiguous(), band.caches[name].detach(), conv.weight, conv.bias, conv.stride[0],
                                           conv.padding[0], act.negative_slope, band, in_stride)
    if isinstance(conv, torch.nn.Conv2d):
        y = band_conv2d(x, conv, band, in_stride, with_bias=False)
    else:
        y = F.conv_transpose2d(x, conv.weight, None, conv.stride, conv.padding, conv.output_padding, conv.groups,
                               conv.dilation)
    if not y.is_contiguous():
        y = y.contiguous()
    y = _BiasLeaky.apply(y, conv.bias, act.negative_slope)
    if tracked:                                   # first iteration of a call: remember the activations
        with torch.no_grad():
            cache = band.caches.get(name)
            if cache is None:
                cache = band.caches[name] = torch.empty_like(y)
            cache.copy_(y)
    return y


def band_conv2d(x, conv: torch.nn.Conv2d, band: Band | None, in_stride: int, with_bias: bool = True):
    """`conv(x)`; with a band, the data gradient is computed on the band's columns only.  `in_stride` = pixels
    per cell of x."""
    bias = conv.bias if with_bias else None
    if band is None or not band.width or not x.requires_grad:
        return F.conv2d(x, conv.weight, bias, conv.stride, conv.padding, conv.dilation, conv.groups)
    s, p = conv.stride[0], conv.padding[0]
    if conv.stride[0] != conv.stride[1] or conv.padding[0] != conv.padding[1] or conv.dilation != (1, 1) or conv.groups != 1:
        raise NotImplementedError("band_conv2d: square stride / padding, no dilation or groups")
    if band.width % (in_stride * s) or x.shape[-1] * in_stride < band.width:
        raise ValueError("band width must be a multiple of the output cell size and fit the frame")
    return _BandConv2d.apply(x, conv.weight, bias, s, p, band, in_stride)
