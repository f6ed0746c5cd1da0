"""CPU suite: the correlation-reach band of the attack's banded backward (band_conv.corr_band_width / corr_band_origin) --
the columns on which conv3_1's and conv_redir's data gradients run, because only the window's correlation adjoint reads them
(20 cells to either side of the window at 1/8 resolution)."""
import pytest
import torch

from understanding_flow_robustness_amd.band_conv import CORR_REACH, corr_band_origin, corr_band_width


def test_width_is_the_narrowest_multiple_of_32_that_holds_window_and_reach():
    assert CORR_REACH == 160
    assert corr_band_width(120) == 448 and corr_band_width(128) == 448 and corr_band_width(96) == 416
    for ww in range(8, 400, 8):
        w = corr_band_width(ww)
        assert w % 32 == 0 and w - 32 < ww + 2 * CORR_REACH <= w


@pytest.mark.parametrize("W,ww", [(1280, 120), (1280, 128), (768, 96)])
def test_band_holds_what_the_correlation_adjoint_reads_for_every_placement(W, ww):
    width = corr_band_width(ww)
    assert width <= W
    w8 = W // 8
    xs = list(range(0, W - ww + 1, 8))
    origins = corr_band_origin(torch.tensor(xs, dtype=torch.int32), width, W)          # the tensor form the step uses
    assert origins.dtype == torch.int32
    for x0, o_t in zip(xs, origins.tolist()):
        o = corr_band_origin(x0, width, W)
        assert o == o_t
        assert o % 8 == 0 and 0 <= o and o + width <= W                                 # inside the frame, on the 1/8 grid
        lo, hi = max(x0 // 8 - 20, 0), min(x0 // 8 + ww // 8 + 20, w8)                  # cells the adjoint reads, cut to the frame
        assert o // 8 <= lo and hi <= (o + width) // 8, (x0, o)
