"""Writes `igemm_form_digests.json`, the fixture of tests/test_igemm_digests_gpu.py: per (case, K order, kernel variant) of
tests/igemm_cases.py the SHA-256 of the launch's output buffers and the increment of `igemm.variant_fallbacks()`.

    python tests/golden/make_igemm_digests.py [--out FILE]          # needs an MI355X

The fixture was recorded on the commit BEFORE csrc/igemm.hip's tile kernels moved onto one tile walk, cell geometry and activation
stager, and before the three-plane split moved into csrc/ufr_common.h: it is that commit's arithmetic.  It is not regenerated from a
tree under test; a pull request that changes the arithmetic on purpose re-records it from its own build and says so.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import igemm_cases                                                                           # noqa: E402

FIXTURE = os.path.join(HERE, "igemm_form_digests.json")

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    got = igemm_cases.digests()
    with open(args.out, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} digests -> {args.out}")
