"""The argument validation of the statistics entries (csrc/feature_stats.hip) under AddressSanitizer and UBSan, as a stand-alone
host program (tests/host/feature_stats_validation_main.cpp, its own `main`): the host side of the two translation units it needs
is instrumented (`-Xarch_host -fsanitize=address,undefined`), the device code is not, and nothing is loaded into python.  Every
call of the program is refused before any HIP call, so it runs without a GPU.  (Its first run found `out_col + channels`
leaving `long` for a column offset near 2^63; the entry now compares `out_col <= out_cols - channels`.)"""
import os
import subprocess

import pytest
import torch

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "understanding_flow_robustness_amd", "csrc")


def test_validation_program_runs_clean_under_host_sanitizers(tmp_path):
    if torch.cuda.is_available():
        pytest.skip("sanitizer builds run on the build machine, never beside a GPU")
    exe = str(tmp_path / "feature_stats_validation")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function"]
    for flag in ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"):
        cmd += ["-Xarch_host", flag]
    cmd += [os.path.join(CSRC, "capi.hip"), os.path.join(CSRC, "feature_stats.hip"),
            os.path.join(ROOT, "tests", "host", "feature_stats_validation_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    ran = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr[-2000:]
    assert "all refused, 0 failures" in ran.stdout and "runtime error" not in ran.stderr and "AddressSanitizer" not in ran.stderr
