"""`ufr_igemm_tail_plan` (csrc/igemm.hip) under AddressSanitizer and UBSan, as a stand-alone host program
(tests/host/igemm_tail_plan_main.cpp, its own `main`): the host side of the two translation units it needs is instrumented
(`-Xarch_host -fsanitize=address,undefined`), the device code is not, and nothing is loaded into python.  The plan is host
arithmetic and the balanced entry is only called where it is refused before it asks for a device, so the program runs without a GPU."""
import os
import subprocess

import pytest
import torch

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "understanding_flow_robustness_amd", "csrc")


def test_tail_plan_program_runs_clean_under_host_sanitizers(tmp_path):
    if torch.cuda.is_available():
        pytest.skip("sanitizer builds run on the build machine, never beside a GPU")
    exe = str(tmp_path / "igemm_tail_plan")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function"]
    for flag in ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"):
        cmd += ["-Xarch_host", flag]
    cmd += [os.path.join(CSRC, "capi.hip"), os.path.join(CSRC, "igemm.hip"),
            os.path.join(ROOT, "tests", "host", "igemm_tail_plan_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    ran = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr[-2000:]
    assert ", 0 failures" in ran.stdout and "runtime error" not in ran.stderr and "AddressSanitizer" not in ran.stderr
    on = int(ran.stdout.split(" plans on")[0].split()[-1])
    assert on > 100, ran.stdout[-500:]          # (the sweep does reach plans that are on)
