"""CPU suite of the validation's C entries (csrc/validation.hip): they are exported as include/ufr_hip.h declares them, the ctypes
table mirrors the declarations, every bad argument is refused before any launch, and the stand-alone host program
tests/host/validation_args_main.cpp runs the same refusals clean under AddressSanitizer and UBSan."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ufr_hip.h")
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "understanding_flow_robustness_amd", "csrc")
ENTRIES = ("ufr_validation_pad", "ufr_validation_metrics", "ufr_validation_metrics_workspace_doubles")


def _declared(name):
    """(return type, [ctypes type per parameter]) of `name` as the header declares it."""
    from understanding_flow_robustness_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(int|long)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/ufr_hip.h"
    kinds = []
    for param in m.group(2).split(","):                      # a C parameter list repeats the type for every name
        typ = re.sub(r"\w+\s*$", "", param.strip()).replace("const", "").replace(" ", "")
        kinds.append(L._vp if "*" in typ or typ == "ufr_stream_t" else {"int": L._i, "long": L._l, "float": L._f}[typ])
    return m.group(1), kinds


def test_entries_are_exported_and_match_the_signatures():
    from understanding_flow_robustness_amd import _lib as L
    from understanding_flow_robustness_amd import validation as V
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
    for name in ENTRIES[:2]:
        ret, kinds = _declared(name)
        assert ret == "int" and kinds == L.SIGNATURES[name], (name, kinds)
    ret, kinds = _declared(ENTRIES[2])
    assert ret == "long" and (ctypes.c_long, kinds) == L.PLAIN[ENTRIES[2]]
    assert len(L.SIGNATURES["ufr_validation_pad"]) == 13 and len(L.SIGNATURES["ufr_validation_metrics"]) == 17
    assert L.lib().ufr_abi_version() == 9                                       # additive entries: the ABI version stays
    assert re.search(r"#define\s+UFR_VALIDATION_COLS\s+8\b", open(HEADER).read()) and V.COLS == 8
    ws = L.lib().ufr_validation_metrics_workspace_doubles
    assert ws(0, 5, 7) == ws(1, 0, 7) == ws(1, 5, -1) == -1
    # one workgroup per 256 pixels, 128 at most, per item: a function of K, H and W alone
    assert ws(1, 5, 7) == 8 and ws(4, 5, 7) == 32 and ws(3, 125, 187) == 3 * 92 * 8 and ws(2, 376, 1242) == 2 * 128 * 8
    assert "validation" in L.source_checksums()                                 # the build manifest covers the new file
    assert "validation" in L.lib().ufr_build_manifest().decode()


def _entries():
    from understanding_flow_robustness_amd import _lib as L
    p = ctypes.c_void_p(4096)
    K = 3
    ws = L.lib().ufr_validation_metrics_workspace_doubles(K, 5, 7)
    return [
        #                                          image1 image2 out1 out2 K H W top bottom left right divide stream
        ("ufr_validation_pad", b"validation pad", [p, p, p, p, K, 5, 7, 1, 2, 0, 1, 1, None],
         [((0, None), b"null pointer"), ((1, None), b"null pointer"), ((2, None), b"null pointer"), ((3, None), b"null pointer"),
          ((4, 0), b"bad shape"), ((4, -1), b"bad shape"), ((5, 0), b"bad shape"), ((6, -4), b"bad shape"),     # K < 1, sizes
          ((7, -1), b"negative pad"), ((8, -2), b"negative pad"), ((9, -1), b"negative pad"), ((10, -8), b"negative pad")]),
        #                                                  pred gt valid K Hp Wp top left H W mode ws ws_elems out row0 rows stream
        ("ufr_validation_metrics", b"validation metrics", [p, p, p, K, 8, 8, 1, 0, 5, 7, 0, p, ws, p, 0, K, None],
         [((0, None), b"null pointer"), ((1, None), b"null pointer"), ((11, None), b"null pointer"), ((13, None), b"null pointer"),
          ((3, 0), b"bad shape"), ((3, -2), b"bad shape"), ((4, 0), b"bad shape"), ((5, -1), b"bad shape"), ((8, 0), b"bad shape"),
          ((9, 0), b"bad shape"),
          ((6, -1), b"negative pad"), ((7, -1), b"negative pad"),
          ((6, 4), b"leaves the padded frame"), ((7, 2), b"leaves the padded frame"), ((8, 8), b"leaves the padded frame"),
          ((4, 5), b"leaves the padded frame"),
          ((10, 3), b"mode 3"), ((10, -1), b"mode -1"),
          ((14, 1), b"leave the result buffer"), ((14, -1), b"leave the result buffer"), ((15, 0), b"leave the result buffer"),
          ((15, K - 1), b"leave the result buffer"),
          ((12, ws - 1), b"workspace"), ((12, 0), b"workspace")]),
    ]


def test_entries_refuse_bad_arguments_before_any_launch():
    """Each refusal returns UFR_EINVAL (-1) with the entry's own message; the pointers are never dereferenced, so this runs
    without a GPU (the pattern of test_global_eval_cabi_cpu.py)."""
    from understanding_flow_robustness_amd import _lib as L
    lib = L.lib()
    for name, prefix, good, bad in _entries():
        assert len(good) == len(L.SIGNATURES[name])
        for (index, value), needle in bad:
            args = list(good)
            args[index] = value
            lib.ufr_corr_forward(None, None, None, 0, 1, 1, 4, 4, None, None)      # another message in the channel first
            rc = getattr(lib, name)(*args)
            assert rc == -1, f"{name}: argument {index} = {value!r} was accepted (rc {rc})"
            message = lib.ufr_last_error()
            assert message.startswith(prefix + b":") and needle in message, (name, index, value, message)


def test_args_program_runs_clean_under_host_sanitizers(tmp_path):
    """tests/host/validation_args_main.cpp with the host side of the two translation units it needs under AddressSanitizer and
    UBSan (`-Xarch_host`); the device code is not instrumented and nothing is loaded into python (the pattern of
    test_feature_stats_host_cpu.py)."""
    if torch.cuda.is_available():
        pytest.skip("sanitizer builds run on the build machine, never beside a GPU")
    exe = str(tmp_path / "validation_args")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function"]
    for flag in ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"):
        cmd += ["-Xarch_host", flag]
    cmd += [os.path.join(CSRC, "capi.hip"), os.path.join(CSRC, "validation.hip"),
            os.path.join(ROOT, "tests", "host", "validation_args_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    ran = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr[-2000:]
    assert "all refused, 0 failures" in ran.stdout and "runtime error" not in ran.stderr and "AddressSanitizer" not in ran.stderr
