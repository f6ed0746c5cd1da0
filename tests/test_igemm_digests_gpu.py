"""GPU suite: the output BYTES of csrc/igemm.hip's tile kernels against the digests of the commit before they moved onto one tile
walk, one cell geometry and one activation stager (tests/igemm_cases.py, tests/golden/make_igemm_digests.py): every kernel form keeps
its arithmetic and its order of additions, so every case hashes to what it hashed to before, under every variant and both K orders;
a launch that falls through to a plain form still does (the `variant_fallbacks()` increment is part of the record)."""
import json
import os

import pytest

import igemm_cases

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "igemm_form_digests.json")


def test_every_form_reproduces_the_recorded_bytes():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = igemm_cases.digests()
    assert len(want) == len(igemm_cases.CASES) * len(igemm_cases.K_ORDERS) * len(igemm_cases.VARIANTS)
    assert sorted(got) == sorted(want)
    wrong = [k for k in sorted(want) if got[k] != want[k]]
    assert not wrong, f"{len(wrong)} of {len(want)} launches differ from the recorded bytes: {wrong}"
