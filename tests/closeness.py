"""The suite's comparison: conftest.assert_close's bound, and nothing that is not finite passes it.

`err > bound` is false for NaN on either side, and one NaN in `expected` turns max|e| -- hence every bound -- into NaN, so the
helper in conftest.py cannot fail on NaN.  This one refuses a reference that is not finite (it cannot judge anything) and a
result that is not finite, and only then compares.  There is no flag that lets NaN through: a caller that legitimately compares
NaN positions masks them itself and asserts the mask separately."""
import torch


def assert_close(actual, expected, rtol=1e-4, atol_scale=1e-5, what=""):
    """|a-e| <= rtol*|e| + atol_scale*max|e|  (fp32 sums in a different order than the oracle); both sides finite."""
    actual = actual.detach().double().cpu()
    expected = expected.detach().double().cpu()
    assert actual.shape == expected.shape, f"{what}: shape {tuple(actual.shape)} vs {tuple(expected.shape)}"
    ref_bad = ~torch.isfinite(expected)
    assert not bool(ref_bad.any()), (
        f"{what}: the reference has {int(ref_bad.sum())}/{ref_bad.numel()} non-finite elements and cannot judge anything")
    nan, inf = torch.isnan(actual), torch.isinf(actual)
    assert not bool(nan.any() | inf.any()), (
        f"{what}: the result has {int(nan.sum())} NaN and {int(inf.sum())} Inf among {actual.numel()} elements")
    atol = atol_scale * float(expected.abs().max().clamp_min(1e-30))
    err = (actual - expected).abs()
    bound = rtol * expected.abs() + atol
    bad = err > bound
    assert not bool(bad.any()), (
        f"{what}: {int(bad.sum())}/{bad.numel()} elements off; max err {float(err.max()):.3e} "
        f"(max |ref| {float(expected.abs().max()):.3e})")
