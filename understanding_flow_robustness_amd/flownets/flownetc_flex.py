"""Robust FlowNetC and its relatives (models/FlowNetC_flexible_larger_field.py, models/FlowNetC_predict_bias.py).

`FlowNetCFlex(kernel_size, number_of_reps, dilation)` is the CVPR'22 paper's Robust FlowNetC: FlowNetC whose three stem
layers become three stages (`convs1`, `convs2`, `convs3`) of one strided convolution followed by `number_of_reps`
stride-1 convolutions (FlowNetC_flexible_larger_field.py:111-176).  `FlowNetCPredictBias` is the original FlowNetC trained
with the paper's pipeline.  Both share FlowNetC's head (flownetc.py, flownetc_engine.py) with three differences: the
deconvolutions and flow upsamplers have no bias, and div_flow = 1.  Parameter names, order and shapes equal the
reference's, so its bare state-dict checkpoints load unchanged.

The engine (flownetc_engine.py, plane_graph.stem_graph) runs the stem as a chain of stages read from `stem_stages()`:
conv1 on csrc/conv1_direct.hip, every 3 x 3 layer on the igemm.  It serves kernel_size 3, dilation 1 and 0-3 reps, which
covers every registry name; other constructor arguments run the torch spelling and are reported (`_lib.engine_gate`).
"""
from __future__ import annotations

import torch.nn as nn

from ..cone import ConeSpec
from .flownetc import ConvLeaky, FlowNetC, _conv


def _conv_dil(cin, cout, k, stride, dilation):
    """FlowNetC_flexible_larger_field.py:20-53 (batchNorm=False): conv + bias + LeakyReLU(0.1), padding ((k-1)//2) * dilation."""
    if dilation == 1:
        return _conv(cin, cout, k, stride)
    return ConvLeaky(nn.Conv2d(cin, cout, k, stride, ((k - 1) // 2) * dilation, dilation=dilation, bias=True),
                     nn.LeakyReLU(0.1, inplace=True))


def stage_cone(blocks) -> tuple:
    """(kernel, stride, pad) of ONE convolution equivalent to a chain of convolutions (its receptive field): the chain's
    cone of influence, needed window and rim margins are those of this layer (cone.ConeSpec)."""
    k_eq, p_eq, s_eq = 1, 0, 1
    for k, s, p in blocks:
        k_eq += (k - 1) * s_eq
        p_eq += p * s_eq
        s_eq *= s
    return k_eq, s_eq, p_eq


def _layer_geometry(block):
    conv = block[0]
    k, d = conv.kernel_size[0], conv.dilation[0]
    return (k - 1) * d + 1, conv.stride[0], conv.padding[0]


class FlowNetCPredictBias(FlowNetC):
    """models/FlowNetC_predict_bias.py:84-235: FlowNetC's layers and names (7 / 5 / 5 stem), bias-less deconvolutions and
    flow upsamplers, div_flow = 1.  The stem, CONE and engine are FlowNetC's."""

    def __init__(self, batchNorm=False, div_flow=1, return_feat_maps=False):
        super().__init__(batchNorm, div_flow, return_feat_maps, deconv_bias=False, up_bias=False)

    def _init_weights(self):
        _kaiming_init(self)


def _kaiming_init(net):
    """FlowNetC_flexible_larger_field.py:203-225 / FlowNetC_predict_bias.py: kaiming_normal_(w, 0.1), zero biases."""
    for m in net.modules():
        if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            nn.init.kaiming_normal_(m.weight, 0.1)
            if m.bias is not None:
                nn.init.zeros_(m.bias)


class FlowNetCFlex(FlowNetC):
    """models/FlowNetC_flexible_larger_field.py:91-323 (batchNorm=False)."""

    def __init__(self, batchNorm=False, div_flow=1, kernel_size=5, number_of_reps=1, dilation=1, return_feat_maps=False):
        self.kernel_size, self.number_of_reps, self.dilation = int(kernel_size), int(number_of_reps), int(dilation)
        super().__init__(batchNorm, div_flow, return_feat_maps, deconv_bias=False, up_bias=False)
        # every stage folded into its receptive-field equivalent: a 3-layer chain (the device's cone chain holds 8 layers)
        self.CONE = ConeSpec(layers=tuple(stage_cone([_layer_geometry(b) for b in st]) for st in (self.convs1, self.convs2, self.convs3)),
                             taps=(1, 2), frames=(1, 2))

    def _build_stem(self):
        """(:111-176) the first layer of each stage is strided and dilated, the repetitions are not."""
        k, r, d = self.kernel_size, self.number_of_reps, self.dilation
        self.convs1 = nn.ModuleList([_conv_dil(3, 64, 7, 2, d)] + [_conv_dil(64, 64, k, 1, 1) for _ in range(r)])
        self.convs2 = nn.ModuleList([_conv_dil(64, 128, k, 2, d)] + [_conv_dil(128, 128, k, 1, 1) for _ in range(r)])
        self.convs3 = nn.ModuleList([_conv_dil(128, 256, k, 2, d)] + [_conv_dil(256, 256, k, 1, 1) for _ in range(r)])

    def _init_weights(self):
        _kaiming_init(self)

    def normalize(self, im):
        """:227-233 -- float64 RGB mean subtraction, std 1 (FlowNetC's normalize_correctly)."""
        return self.normalize_correctly(im)

    def layer_cone(self) -> ConeSpec:
        """The same prefix as one ConeSpec layer per convolution (12 layers for k3 / reps3): what `CONE` folds."""
        layers = tuple(_layer_geometry(b) for st in (self.convs1, self.convs2, self.convs3) for b in st)
        n1, n2 = len(self.convs1), len(self.convs2)
        return ConeSpec(layers=layers, taps=(n1 + n2 - 1, len(layers) - 1), frames=(1, 2))

    def stem_stages(self):
        return tuple(tuple((f"convs{i}.{j}", b) for j, b in enumerate(st))
                     for i, st in ((1, self.convs1), (2, self.convs2), (3, self.convs3)))

    def stem_refusal(self):
        """Why the native stem does not serve this construction (None: it does)."""
        if self.dilation != 1:
            return "FlowNetCFlex: dilation > 1 (the native stem serves dilation 1)"
        if self.kernel_size != 3:
            return f"FlowNetCFlex: kernel_size {self.kernel_size} (the native stem serves 3 x 3 layers)"
        if not 0 <= self.number_of_reps <= 3:
            return f"FlowNetCFlex: number_of_reps {self.number_of_reps} (the native stem serves 0-3)"
        return None
