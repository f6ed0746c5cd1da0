"""CPU suite of the figures' C entries (csrc/flow_viz.hip): they are exported as include/ufr_hip.h declares them, the ctypes table
mirrors the declarations, every bad argument is refused before any HIP call, and the stand-alone host program
tests/host/figures_args_main.cpp runs the same refusals clean under AddressSanitizer and UBSan (the pattern of
test_validation_cabi_cpu.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ufr_hip.h")
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "understanding_flow_robustness_amd", "csrc")
ENTRIES = ("ufr_flow_to_image", "ufr_eval_blend_gt", "ufr_sweep_blend_gt", "ufr_viz_ranges", "ufr_viz_strip")
SIZES = ("ufr_flow_to_image_workspace_floats", "ufr_viz_workspace_floats")


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
    from understanding_flow_robustness_amd import flowlib
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ENTRIES + SIZES:
        assert hasattr(lib, name), f"{name} is not exported"
    for name in ENTRIES:
        ret, kinds = _declared(name)
        assert ret == "int" and kinds == L.SIGNATURES[name], (name, kinds)
    for name in SIZES:
        ret, kinds = _declared(name)
        assert ret == "long" and (ctypes.c_long, kinds) == L.PLAIN[name]
    assert L.lib().ufr_abi_version() == 9                                       # additive entries: the ABI version stays
    assert re.search(r"#define\s+UFR_VIZ_RECORD\s+9\b", open(HEADER).read()) and flowlib.VIZ_RECORD == 9
    for ws, per_item in ((L.lib().ufr_flow_to_image_workspace_floats, 128), (L.lib().ufr_viz_workspace_floats, 128 * 8)):
        assert ws(0) == ws(-3) == -1 and ws(1) == per_item and ws(5) == 5 * per_item
    assert "flow_viz" in L.source_checksums()                                   # the build manifest covers the new file
    assert "flow_viz" in L.lib().ufr_build_manifest().decode()


def _entries():
    from understanding_flow_robustness_amd import _lib as L
    from understanding_flow_robustness_amd import flowlib
    p = ctypes.c_void_p(4096)
    K = 3
    wheel = np.ascontiguousarray(flowlib.make_color_wheel())
    bad_wheel = wheel.copy()
    bad_wheel[17, 1] = 256.0
    places = np.ascontiguousarray(np.tile(np.array([1, 2, 4, 4, 0, 0, 3, 5], dtype=np.int32), (K, 1)))
    high = places.copy()
    high[1, 2] = 9                                           # a record taller than its 6 x 6 slot
    outside = places.copy()
    outside[2, 5] = 30                                       # the second frame's record leaves the 16 x 32 frame
    origins = np.ascontiguousarray(np.array([[0, 0], [3, 5], [11, 27]], dtype=np.int32))
    leaving = origins.copy()
    leaving[2, 1] = 28
    hp = lambda a: a.ctypes.data
    ws_f, ws_v = L.lib().ufr_flow_to_image_workspace_floats(K), L.lib().ufr_viz_workspace_floats(K)
    entries = [
        #                                               flow maxr wheel out K H W ws ws_elems stream
        ("ufr_flow_to_image", b"flow to image", [p, p, hp(wheel), p, K, 13, 37, p, ws_f, None],
         [((0, None), b"null pointer"), ((2, None), b"null pointer"), ((3, None), b"null pointer"), ((7, None), b"null pointer"),
          ((4, 0), b"bad shape"), ((4, -2), b"bad shape"), ((5, 0), b"bad shape"), ((6, -1), b"bad shape"),
          ((8, ws_f - 1), b"workspace"), ((8, 0), b"workspace"), ((2, hp(bad_wheel)), b"colour wheel entry 52")]),
        #                                               gt m_tgt m_ref flow places places_host g K H W Hg Wg sh sw ignore stream
        ("ufr_eval_blend_gt", b"eval blend gt", [p, p, p, p, p, hp(places), p, K, 16, 32, 11, 23, 6, 6, 0, None],
         [((0, None), b"null pointer"), ((1, None), b"null pointer"), ((4, None), b"null pointer"), ((6, None), b"null pointer"),
          ((5, None), b"needed on the host"),
          ((7, 0), b"bad shape"), ((7, -1), b"bad shape"), ((8, 0), b"bad shape"), ((9, -4), b"bad shape"), ((10, 0), b"bad shape"),
          ((11, -1), b"bad shape"), ((12, 0), b"bad shape"), ((13, 0), b"bad shape"),
          ((12, 17), b"larger than"), ((14, 2), b"ignore_mask_flow = 2"),
          ((5, hp(high)), b"does not fit its 6x6 slot"), ((5, hp(outside)), b"leaves the 16x32 frame")]),
        #                                                 gt mask_p origins origins_host g K H W Hg Wg ph pw valid stream
        ("ufr_sweep_blend_gt", b"sweep blend gt", [p, p, p, hp(origins), p, K, 16, 32, 11, 23, 5, 5, 1, None],
         [((0, None), b"null pointer"), ((1, None), b"null pointer"), ((2, None), b"null pointer"), ((3, None), b"null pointer"),
          ((4, None), b"null pointer"),
          ((5, 0), b"bad shape"), ((6, 0), b"bad shape"), ((7, -1), b"bad shape"), ((8, 0), b"bad shape"), ((9, 0), b"bad shape"),
          ((10, 0), b"bad shape"), ((11, -5), b"bad shape"), ((10, 17), b"larger than"), ((12, 2), b"valid_in_patch = 2"),
          ((3, hp(leaving)), b"leaves the 16x32 frame")]),
    ]
    #                                   adv_tgt adv_ref flow adv_flow g K H W Hg Wg ws ws_elems record stream
    ranges = [p, p, p, p, p, K, 16, 32, 11, 23, p, ws_v, p, None]
    entries.append(("ufr_viz_ranges", b"viz ranges", ranges,
                    [((i, None), b"null pointer") for i in (0, 1, 2, 3, 4, 10, 12)]
                    + [((5, 0), b"bad shape"), ((5, -1), b"bad shape"), ((6, 0), b"bad shape"), ((7, -2), b"bad shape"),
                       ((8, 0), b"without its sizes"), ((9, -1), b"without its sizes"),
                       ((11, ws_v - 1), b"workspace"), ((11, 0), b"workspace")]))
    #                                 adv_tgt adv_ref flow adv_flow g record wheel out K H W Hg Wg stream
    strip = [p, p, p, p, p, p, hp(wheel), p, K, 16, 32, 11, 23, None]
    entries.append(("ufr_viz_strip", b"viz strip", strip,
                    [((i, None), b"null pointer") for i in (0, 1, 2, 3, 4, 5, 6, 7)]
                    + [((8, 0), b"bad shape"), ((9, 0), b"bad shape"), ((10, -1), b"bad shape"),
                       ((11, 0), b"without its sizes"), ((12, 0), b"without its sizes"),
                       ((6, hp(bad_wheel)), b"colour wheel entry 52")]))
    return entries, (wheel, bad_wheel, places, high, outside, origins, leaving)


def test_entries_refuse_bad_arguments_before_any_hip_call():
    """Each refusal returns UFR_EINVAL (-1) with the entry's own message; the device pointers are never dereferenced and nothing is
    launched, so this runs without a GPU."""
    from understanding_flow_robustness_amd import _lib as L
    lib = L.lib()
    entries, keep = _entries()
    for name, prefix, good, bad in entries:
        assert len(good) == len(L.SIGNATURES[name])
        for (index, value), needle in bad:
            args = list(good)
            args[index] = value
            lib.ufr_corr_forward(None, None, None, 0, 1, 1, 4, 4, None, None)      # another message in the channel first
            rc = getattr(lib, name)(*args)
            assert rc == -1, f"{name}: argument {index} = {value!r} was accepted (rc {rc})"
            message = lib.ufr_last_error()
            assert message.startswith(prefix + b":") and needle in message, (name, index, value, message)
    assert keep


def test_args_program_runs_clean_under_host_sanitizers(tmp_path):
    """tests/host/figures_args_main.cpp with the host side of the two translation units it needs under AddressSanitizer and UBSan
    (`-Xarch_host`); the device code is not instrumented and nothing is loaded into python."""
    if torch.cuda.is_available():
        pytest.skip("sanitizer builds run on the build machine, never beside a GPU")
    exe = str(tmp_path / "figures_args")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function"]
    for flag in ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"):
        cmd += ["-Xarch_host", flag]
    cmd += [os.path.join(CSRC, "capi.hip"), os.path.join(CSRC, "flow_viz.hip"), os.path.join(ROOT, "tests", "host", "figures_args_main.cpp"),
            "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    ran = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr[-2000:]
    assert "all refused, 0 failures" in ran.stdout and "runtime error" not in ran.stderr and "AddressSanitizer" not in ran.stderr
