"""`ufr_raft_sequence_loss` (csrc/raft_train_loss.hip) validates its arguments before any HIP call: every refusal is UFR_EINVAL (-1)
with a message through `ufr_last_error()`.  No GPU is needed and the pointers are never dereferenced."""
import ctypes

import pytest

from understanding_flow_robustness_amd import _lib as L

P = 4096                                  # a non-null address that nothing reads
TABLES = ("flow", "mask", "grad_flow", "grad_mask")


def workspace(B, H, W, npred):
    return L.lib().ufr_raft_sequence_loss_workspace_doubles(B, H, W, npred)


def desc(B=2, H=5, W=40, npred=12, **over):
    d = L.RaftSequenceLossDesc()
    d.gt, d.valid, d.B, d.H, d.W, d.npred = P, P, B, H, W, npred
    for i in range(min(max(npred, 0), L.UFR_RAFT_LOSS_MAX_PREDS)):
        d.flow[i], d.mask[i], d.grad_flow[i], d.grad_mask[i], d.weight[i] = P, P, P, P, 0.8 ** (npred - i - 1)
    d.div_flow, d.max_flow, d.exclude_large = 1.0, 400.0, 1
    d.ws, d.out = P, P
    d.ws_elems = max(workspace(B, H, W, npred), 0)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def refused(d):
    lib = L.lib()
    rc = lib.ufr_raft_sequence_loss(ctypes.byref(d), None)
    return rc, lib.ufr_last_error().decode()


def test_the_symbols_are_exported_and_the_abi_version_stays():
    lib = L.lib()
    assert lib.ufr_abi_version() == 9 and L.ABI_VERSION == 9
    assert hasattr(lib, "ufr_raft_sequence_loss") and "ufr_raft_sequence_loss" in L.SIGNATURES
    assert hasattr(lib, "ufr_raft_sequence_loss_workspace_doubles") and "ufr_raft_sequence_loss_workspace_doubles" in L.PLAIN
    assert L.UFR_RAFT_LOSS_MAX_PREDS == 32
    assert "raft_train_loss" in L.source_checksums()                            # the build manifest covers the new file
    rc = lib.ufr_raft_sequence_loss(None, None)
    assert rc == -1 and b"null descriptor" in lib.ufr_last_error()


def test_the_descriptor_mirrors_the_header():
    # 2 pointers, 4 ints, 4 tables of 32 pointers, 32 doubles, 2 doubles, an int (padded), a pointer, a long, a pointer
    assert ctypes.sizeof(L.RaftSequenceLossDesc) == 16 + 16 + 4 * 32 * 8 + 32 * 8 + 16 + 8 + 8 + 8 + 8
    assert L.RaftSequenceLossDesc.flow.offset == 32 and L.RaftSequenceLossDesc.weight.offset == 32 + 4 * 256


def test_the_workspace_size():
    # the 18 sums a[k][c] of every coarse pixel and prediction + one row of (npred losses + 5 metric sums) per workgroup of 32 columns
    assert workspace(2, 5, 7, 3) == 18 * 3 * 2 * 5 * 7 + 2 * 5 * 1 * (3 + 5)
    assert workspace(1, 3, 33, 12) == 18 * 12 * 3 * 33 + 3 * 2 * (12 + 5)
    assert workspace(1, 48, 160, 12) == 18 * 12 * 48 * 160 + 48 * 5 * 17
    for bad in ((0, 5, 7, 3), (2, 0, 7, 3), (2, 5, -7, 3), (2, 5, 7, 0), (2, 5, 7, 33), (65536, 5, 7, 3), (2, 65536, 7, 3)):
        assert workspace(*bad) == -1, bad
    assert workspace(65535, 1, 1, 1) > 0


@pytest.mark.parametrize("field", ["gt", "valid", "ws", "out"])
def test_null_pointers_are_refused(field):
    rc, msg = refused(desc(**{field: None}))
    assert rc == -1 and "null pointer" in msg, msg
    with pytest.raises(RuntimeError, match="null pointer"):
        L.check(rc, "probe")


@pytest.mark.parametrize("table", TABLES)
def test_a_null_table_entry_below_npred_is_refused(table):
    d = desc()
    getattr(d, table)[11] = None
    rc, msg = refused(d)
    assert rc == -1 and "null pointer" in msg and "prediction 11" in msg, msg
    d = desc(npred=3, ws_elems=0)                                                 # entries at and above npred are not looked at:
    assert all(not getattr(d, t)[3] for t in TABLES)                              # the call gets as far as the workspace test
    rc, msg = refused(d)
    assert rc == -1 and "workspace" in msg, msg


@pytest.mark.parametrize("npred", [0, -1, 33])
def test_a_number_of_predictions_outside_1_to_32(npred):
    rc, msg = refused(desc(npred=npred))
    assert rc == -1 and f"{npred} predictions" in msg, msg


def test_thirty_two_predictions_pass_the_count():
    rc, msg = refused(desc(npred=32, gt=None))
    assert rc == -1 and "null pointer" in msg, msg


@pytest.mark.parametrize("over", [dict(B=0), dict(H=0), dict(W=-40), dict(B=-1)])
def test_sizes_that_are_not_positive(over):
    rc, msg = refused(desc(**over))
    assert rc == -1 and "sizes must be positive" in msg, msg


@pytest.mark.parametrize("over", [dict(B=65536), dict(H=65536)])
def test_more_rows_or_items_than_a_grid_takes(over):
    rc, msg = refused(desc(**over))
    assert rc == -1 and "at most 65535" in msg, msg


def test_a_workspace_that_is_too_small():
    need = workspace(2, 5, 40, 12)
    rc, msg = refused(desc(ws_elems=need - 1))
    assert rc == -1 and f"the workspace holds {need - 1} doubles, {need} are needed" in msg, msg
