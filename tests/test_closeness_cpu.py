"""tests/closeness.py::assert_close: what is not finite fails on either side, the verdict on finite inputs is
conftest.assert_close's (the tolerance neither loosened nor tightened), and no test file goes back to the helper in conftest.py,
which cannot fail on NaN."""
import ast
import os

import pytest
import torch

import conftest
from closeness import assert_close


def _pair(seed=0, shape=(3, 5, 7)):
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(shape, generator=g)
    return e.clone(), e


def _verdict(fn, *a, **k):
    try:
        fn(*a, **k)
    except AssertionError:
        return False
    return True


def test_equal_tensors_pass():
    a, e = _pair()
    assert_close(a, e)


@pytest.mark.parametrize("poison,count", [("one NaN", "1 NaN and 0 Inf"), ("all NaN", "105 NaN and 0 Inf"), ("one Inf", "0 NaN and 1 Inf"),
                                          ("one -Inf", "0 NaN and 1 Inf")])
def test_non_finite_actual_fails(poison, count):
    a, e = _pair()
    if poison == "one NaN":
        a[1, 2, 3] = float("nan")
    elif poison == "all NaN":
        a.fill_(float("nan"))
    elif poison == "one Inf":
        a[2, 4, 6] = float("inf")
    else:
        a[0, 0, 0] = -float("inf")
    with pytest.raises(AssertionError, match=count):
        assert_close(a, e, what="poisoned")
    # the hole this helper closes: the old one cannot see it
    if "NaN" in poison:
        conftest.assert_close(a, e)


def test_non_finite_expected_fails():
    a, e = _pair()
    e = e.clone()
    e[0, 1, 2] = float("nan")
    with pytest.raises(AssertionError, match=r"golden: the reference has 1/105 non-finite"):
        assert_close(a, e, what="golden")
    with pytest.raises(AssertionError, match=r"golden: the reference has 1/105 non-finite"):
        assert_close(torch.zeros_like(e), e, what="golden")
    conftest.assert_close(torch.zeros_like(e), e)          # vacuous: every bound is NaN
    e[0, 1, 2] = float("inf")
    with pytest.raises(AssertionError, match="non-finite"):
        assert_close(a, e)


def test_shape_mismatch_fails():
    a, e = _pair()
    with pytest.raises(AssertionError, match="shape"):
        assert_close(a[:2], e)
    with pytest.raises(AssertionError, match="shape"):
        assert_close(a.reshape(5, 3, 7), e)


def test_no_flag_lets_nan_through():
    import inspect
    assert list(inspect.signature(assert_close).parameters) == ["actual", "expected", "rtol", "atol_scale", "what"]


@pytest.mark.parametrize("rtol,atol_scale", [(1e-4, 2e-6), (1e-6, 1e-7), (1e-3, 2e-4)])
def test_verdict_on_finite_inputs_equals_conftest(rtol, atol_scale):
    """A fixed error pattern (random signs; in every trial one element carries the whole error, the others a random share of it),
    scaled from 0.5x to 2x of that element's own bound: below 1x both helpers pass, above both fail, and at every factor the two
    agree."""
    g = torch.Generator().manual_seed(int(1e7 * rtol) + 1)
    e = torch.randn(4, 6, 9, generator=g, dtype=torch.float64) * 3.0
    e[0, 0, 0] = 0.0                                         # an element whose bound is the absolute term alone
    bound = rtol * e.abs() + atol_scale * float(e.abs().max())
    sign = torch.where(torch.rand(e.shape, generator=g) < 0.5, -1.0, 1.0).double()
    share = torch.rand(e.shape, generator=g, dtype=torch.float64) * 0.4
    seen = set()
    for trial in range(8):
        worst = int(torch.randint(e.numel(), (1,), generator=g)) if trial else 0
        pattern = share.clone()
        pattern.view(-1)[worst] = 1.0
        for factor in (0.5, 0.8, 0.95, 0.999, 1.001, 1.05, 1.3, 2.0):
            a = e + factor * sign * pattern * bound
            new, old = _verdict(assert_close, a, e, rtol=rtol, atol_scale=atol_scale), _verdict(conftest.assert_close, a, e, rtol=rtol, atol_scale=atol_scale)
            assert new == old, (trial, factor, new, old)
            assert new == (factor < 1.0), (trial, factor, new)
            seen.add(new)
    assert seen == {True, False}
    # float32 operands, as the suite hands them over: same verdicts
    e32 = e.float()
    for factor in (0.5, 2.0):
        a32 = (e32.double() + factor * sign * bound).float()
        assert _verdict(assert_close, a32, e32, rtol=rtol, atol_scale=atol_scale) == _verdict(conftest.assert_close, a32, e32, rtol=rtol, atol_scale=atol_scale) == (factor < 1.0)


def test_no_test_file_imports_the_blind_helper():
    """`ast` over every source file under tests/: no `from conftest import assert_close`, no `conftest.assert_close` attribute
    (this file excepted, which compares the two helpers on purpose)."""
    here = os.path.dirname(os.path.abspath(__file__))
    offenders, files = [], 0
    for root, _, names in os.walk(here):
        for name in names:
            if not name.endswith(".py"):
                continue
            path = os.path.join(root, name)
            files += 1
            with open(path) as fh:
                tree = ast.parse(fh.read(), path)
            for node in ast.walk(tree):
                if isinstance(node, ast.ImportFrom) and (node.module or "").split(".")[-1] == "conftest":
                    if any(al.name in ("assert_close", "*") for al in node.names):
                        offenders.append(f"{os.path.relpath(path, here)}:{node.lineno}")
                elif (isinstance(node, ast.Attribute) and node.attr == "assert_close" and isinstance(node.value, ast.Name)
                      and node.value.id == "conftest" and os.path.abspath(path) != os.path.abspath(__file__)):
                    offenders.append(f"{os.path.relpath(path, here)}:{node.lineno}")
    assert files > 16 and not offenders, offenders
