"""CPU suite: the C entries of csrc/perturb_step.hip (MI-FGSM and input diversity on the captured step) exist beside an
unchanged ABI version and refuse bad arguments on the host, before any HIP call: the pointers are never dereferenced."""
import ctypes

import pytest
import torch

ENTRIES = ("ufr_abs_sums", "ufr_abs_sums_workspace_doubles", "ufr_momentum_update", "ufr_diverse_table_check",
           "ufr_diverse_workspace_doubles", "ufr_diverse_forward", "ufr_diverse_backward", "ufr_step_advance")


def _lib():
    from understanding_flow_robustness_amd import _lib as L
    return L, L.lib()


def test_symbols_exist_and_the_abi_version_is_unchanged():
    L, lib = _lib()
    assert lib.ufr_abi_version() == 9 == L.ABI_VERSION
    for name in ENTRIES:
        assert hasattr(lib, name) and (name in L.SIGNATURES or name in L.PLAIN), name
    assert "perturb_step" in dict(ln.split() for ln in lib.ufr_build_manifest().decode().splitlines())
    assert L.DIVERSE_COLS == 8


def _refused(lib, name, args, message):
    lib.ufr_corr_forward(None, None, None, 0, 1, 1, 4, 4, None, None)              # another message in the channel first
    rc = getattr(lib, name)(*args)
    assert rc == -1, f"{name}{tuple(args)} was accepted (rc {rc})"
    err = lib.ufr_last_error()
    assert err.startswith(message + b":") and len(err) > len(message) + 2, (name, args, err)
    return err


def _one_replaced(lib, name, message, good, bad):
    for index, value in bad:
        args = list(good)
        args[index] = value
        _refused(lib, name, args, message)


def test_abs_sums_refuses_bad_arguments():
    L, lib = _lib()
    p = ctypes.c_void_p(4096)
    assert lib.ufr_abs_sums_workspace_doubles(0) == -1 and lib.ufr_abs_sums_workspace_doubles(-5) == -1
    n = 2 * 3 * 20 * 30
    need = lib.ufr_abs_sums_workspace_doubles(n)
    assert need == 2 * 4                                                            # ceil(3600 / 1024) pairs
    assert lib.ufr_abs_sums_workspace_doubles(10 ** 9) == 2 * 2048                  # the partial count stops growing
    good = [p, p, n, p, need, p, None]
    assert len(good) == len(L.SIGNATURES["ufr_abs_sums"])
    _one_replaced(lib, "ufr_abs_sums", b"abs sums", good, [(0, None), (1, None), (3, None), (5, None), (2, 0), (2, -1)])
    err = _refused(lib, "ufr_abs_sums", [p, p, n, p, need - 1, p, None], b"abs sums")
    assert b"workspace of 7 doubles, 8 needed" in err


def test_momentum_update_refuses_bad_arguments():
    L, lib = _lib()
    p = ctypes.c_void_p(4096)
    good = [p] * 10 + [2, 1800, 0.47, 0.53, 0.008, 0.02, 0.0, 1.0, 3, 1, None]
    assert len(good) == len(L.SIGNATURES["ufr_momentum_update"])
    _one_replaced(lib, "ufr_momentum_update", b"momentum update", good,
                  [(i, None) for i in range(10)] + [(10, 0), (11, 0), (11, -4), (18, 0), (18, 4)])


def _table(*rows):
    t = torch.zeros(len(rows), 8, dtype=torch.int32)
    for r, row in zip(t, rows):
        r[:len(row)] = torch.tensor(row, dtype=torch.int32)
    return t


def test_table_check_refuses_rows_that_leave_the_frame():
    L, lib = _lib()
    H, W = 20, 30
    ok = _table((0,), (1, 20, 30, 0, 0), (1, 18, 27, 2, 3), (1, 18, 27, 0, 0), (1, 19, 30, 1, 0), (0, 99, 99, 99, 99))
    assert lib.ufr_diverse_table_check(ok.data_ptr(), ok.shape[0], H, W) == 0       # apply == 0 rows are not read further
    _refused(lib, "ufr_diverse_table_check", [None, 1, H, W], b"diverse table")
    _refused(lib, "ufr_diverse_table_check", [ok.data_ptr(), 0, H, W], b"diverse table")
    _refused(lib, "ufr_diverse_table_check", [ok.data_ptr(), 1, 0, W], b"diverse table")
    for row, words in (((1, 21, 30, 0, 0), b"nh > H"), ((1, 20, 31, 0, 0), b"nh > H or nw > W"), ((1, 0, 30, 0, 0), b"resizes"),
                       ((1, 18, 27, 3, 0), b"top + nh > H"), ((1, 18, 27, 0, 4), b"left + nw > W"), ((1, 18, 27, -1, 0), b"leaves"),
                       ((1, 18, 27, 0, -1), b"leaves")):
        bad = _table((0,), row)
        err = _refused(lib, "ufr_diverse_table_check", [bad.data_ptr(), 2, H, W], b"diverse table")
        assert words in err and b"row 1" in err, (row, err)
        assert lib.ufr_diverse_table_check(bad.data_ptr(), 1, H, W) == 0            # only the rows that were asked about


def test_diverse_entries_refuse_bad_arguments():
    L, lib = _lib()
    p = ctypes.c_void_p(4096)
    B, H, W = 2, 20, 30
    assert lib.ufr_diverse_workspace_doubles(B, H, W, 2) == 0
    need = lib.ufr_diverse_workspace_doubles(B, H, W, 3)
    assert need == -(-B * 9 * H * W // 1024)
    for bad in ((0, H, W, 3), (B, 0, W, 3), (B, H, -1, 3), (B, H, W, 1), (B, H, W, 4)):
        assert lib.ufr_diverse_workspace_doubles(*bad) == -1
    good = [p, p, p, p, p, p, B, H, W, 3, p, 4, p, p, p, need, None]
    assert len(good) == len(L.SIGNATURES["ufr_diverse_forward"])
    _one_replaced(lib, "ufr_diverse_forward", b"diverse forward", good,
                  [(i, None) for i in (0, 1, 2, 3, 4, 5, 10, 12, 13, 14)] + [(6, 0), (7, 0), (8, -3), (11, 0), (9, 1), (9, 4), (15, need - 1)])
    assert b"workspace" in _refused(lib, "ufr_diverse_forward", good[:15] + [need - 1, None], b"diverse forward")
    assert b"4 channels" in _refused(lib, "ufr_diverse_forward", good[:9] + [4] + good[10:], b"diverse forward")
    good = [p, p, ctypes.c_void_p(8192), ctypes.c_void_p(12288), B, H, W, p, 4, p, None]
    assert len(good) == len(L.SIGNATURES["ufr_diverse_backward"])
    _one_replaced(lib, "ufr_diverse_backward", b"diverse backward", good,
                  [(i, None) for i in (0, 1, 2, 3, 7, 9)] + [(4, 0), (5, 0), (6, 0), (8, 0), (2, p)])      # (2, p): in place
    _refused(lib, "ufr_step_advance", [None, None], b"step advance")


def test_the_step_refuses_the_shared_perturbation_with_momentum_or_diversity():
    """Out of scope, and said so: one perturbation for a sharded batch has no per-sample momentum or transform."""
    from argparse import Namespace
    from understanding_flow_robustness_amd.universal_perturbation import UniversalPerturbationStep
    args = Namespace(flownet="FlowNetC", flow_loss="l2", perturb_method="ifgsm", perturb_mode="both", learning_rate=0.01,
                     output_norm=0.02)
    for kw in (dict(momentum=0.5), dict(diverse=True)):
        with pytest.raises(NotImplementedError, match="per-sample perturbations only"):
            UniversalPerturbationStep(None, args, 1, 64, 128, device="cpu", shared=True, **kw)
