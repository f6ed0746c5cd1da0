"""CPU suite of the global-attack evaluation's C entries (csrc/global_eval.hip): they are exported as include/ufr_hip.h declares them,
the ctypes table mirrors the declarations, and every bad argument is refused before any launch."""
import ctypes
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ufr_hip.h")
ENTRIES = ("ufr_global_apply", "ufr_global_metrics", "ufr_global_metrics_workspace_doubles")


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
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
    for name in ENTRIES[:2]:
        ret, kinds = _declared(name)
        assert ret == "int" and kinds == L.SIGNATURES[name], (name, kinds)
    ret, kinds = _declared(ENTRIES[2])
    assert ret == "long" and (ctypes.c_long, kinds) == L.PLAIN[ENTRIES[2]]
    assert len(L.SIGNATURES["ufr_global_apply"]) == 13 and len(L.SIGNATURES["ufr_global_metrics"]) == 19
    assert L.lib().ufr_abi_version() == 9                                       # additive entries: the ABI version stays
    assert L.lib().ufr_global_metrics_workspace_doubles(0) == -1
    one, four = L.lib().ufr_global_metrics_workspace_doubles(1), L.lib().ufr_global_metrics_workspace_doubles(4)
    assert one > 0 and four == 4 * one
    assert "global_eval" in L.source_checksums()                                # the build manifest covers the new file
    assert "global_eval" in L.lib().ufr_build_manifest().decode()


def _entries():
    from understanding_flow_robustness_amd import _lib as L
    p = ctypes.c_void_p(4096)
    K = 3
    ws = L.lib().ufr_global_metrics_workspace_doubles(K)
    return [
        #                                      image0 image1 noise0 noise1 adv0 adv1 K Kn H W lo hi stream
        ("ufr_global_apply", b"global apply", [p, p, p, p, p, p, K, K, 5, 7, 0.0, 1.0, None],
         [(0, None), (1, None), (2, None), (3, None), (4, None), (5, None),       # null pointers, one noise without the other
          (6, 0), (6, -1), (8, 0), (9, -4),                                       # K < 1, non-positive sizes
          (7, 2), (7, 0), (7, 4),                                                 # Kn outside {1, K}
          (10, 1.5), (11, -0.5)]),                                                # lo > hi
        #                                          clean adv gt noise0 noise1 K Kg Kn C H W Hg Wg ws ws_elems out row0 rows stream
        ("ufr_global_metrics", b"global metrics", [p, p, p, p, p, K, K, 1, 3, 5, 7, 6, 8, p, ws, p, 0, K, None],
         [(0, None), (1, None), (2, None), (13, None), (15, None), (3, None), (4, None),
          (5, 0), (5, -2), (9, 0), (10, 0), (11, -1), (12, 0),
          (6, 2), (6, 0), (7, 2), (7, 0),                                         # Kg / Kn outside {1, K}
          (8, 1), (8, 4),                                                         # C outside {2, 3}
          (16, 1), (16, -1), (17, 0), (17, K - 1),                                # rows outside the result buffer
          (14, ws - 1), (14, 0)]),                                                # a workspace that is too small
    ]


def test_entries_refuse_bad_arguments_before_any_launch():
    """Each refusal returns -1 with the entry's own message; the pointers are never dereferenced, so this runs without a GPU (the
    pattern of test_cabi_cpu.py::test_update_block_and_norm_entries_refuse_bad_arguments_before_any_launch)."""
    from understanding_flow_robustness_amd import _lib as L
    lib = L.lib()
    for name, message, good, bad in _entries():
        assert len(good) == len(L.SIGNATURES[name])
        for index, value in bad:
            args = list(good)
            args[index] = value
            lib.ufr_corr_forward(None, None, None, 0, 1, 1, 4, 4, None, None)      # another message in the channel first
            rc = getattr(lib, name)(*args)
            assert rc == -1, f"{name}: argument {index} = {value!r} was accepted (rc {rc})"
            assert lib.ufr_last_error().startswith(message + b":"), (name, index, value, lib.ufr_last_error())
    # both noises NULL is a valid call shape (the noise columns become NaN): only ONE of them missing is refused, by name
    p = ctypes.c_void_p(4096)
    assert lib.ufr_global_metrics(p, p, p, p, None, 3, 3, 3, 3, 5, 7, 6, 8, p, 1 << 20, p, 0, 3, None) == -1
    assert b"both noises or neither" in lib.ufr_last_error()
