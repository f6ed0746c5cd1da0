"""`ufr_train_loss` (csrc/train_loss.hip), `ufr_grad_norm` and `ufr_adamw_step` (csrc/optim.hip) validate their arguments before any
HIP call: every refusal is UFR_EINVAL (-1) with a message through `ufr_last_error()`.  No GPU is needed and the pointers are never
dereferenced."""
import ctypes

import pytest

from understanding_flow_robustness_amd import _lib as L

P = 4096                                  # a non-null address that nothing reads
SIZES = [(64, 128), (32, 64), (16, 32), (8, 16), (4, 8)]


def workspace(B, sizes):
    n = len(sizes)
    h, w = (ctypes.c_int * n)(*[s[0] for s in sizes]), (ctypes.c_int * n)(*[s[1] for s in sizes])
    return L.lib().ufr_train_loss_workspace_doubles(B, n, h, w)


def loss_desc(sizes=SIZES, B=2, H=64, W=128, **over):
    d = L.TrainLossDesc()
    d.gt, d.B, d.H, d.W, d.nscale, d.kind, d.div_flow = P, B, H, W, len(sizes), 0, 1.0
    for i, (h, w) in enumerate(sizes[:L.UFR_TRAIN_LOSS_MAX_SCALES]):
        d.pred[i], d.grad[i], d.h[i], d.w[i], d.weight[i] = P, P, h, w, 0.8 ** i
    d.ws, d.out = P, P
    d.ws_elems = max(workspace(B, sizes[:L.UFR_TRAIN_LOSS_MAX_SCALES]), 0)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def loss_refused(d):
    lib = L.lib()
    rc = lib.ufr_train_loss(ctypes.byref(d), None)
    return rc, lib.ufr_last_error().decode()


def test_the_symbols_are_exported_and_the_abi_version_stays():
    lib = L.lib()
    assert lib.ufr_abi_version() == 9 and L.ABI_VERSION == 9
    for name in ("ufr_train_loss", "ufr_grad_norm", "ufr_adamw_step"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    for name in ("ufr_train_loss_workspace_doubles", "ufr_grad_norm_partials"):
        assert hasattr(lib, name) and name in L.PLAIN
    rc = lib.ufr_train_loss(None, None)
    assert rc == -1 and b"null descriptor" in lib.ufr_last_error()


def test_the_workspace_size():
    # the interpolated ground truths + 256 slots of (2 counts + 6 sums) per scale
    assert workspace(2, SIZES) == 2 * 2 * sum(h * w for h, w in SIZES) + 5 * 256 * 8
    assert workspace(0, SIZES) == -1 and workspace(1, [(4, 0)]) == -1 and workspace(1, [(1, 1)] * 9) == -1


@pytest.mark.parametrize("field", ["gt", "out", "ws"])
def test_null_pointers_are_refused(field):
    rc, msg = loss_refused(loss_desc(**{field: None}))
    assert rc == -1 and "null pointer" in msg, msg
    with pytest.raises(RuntimeError, match="null pointer"):
        L.check(rc, "probe")


@pytest.mark.parametrize("which", ["pred", "grad"])
def test_a_null_prediction_or_gradient_is_refused(which):
    d = loss_desc()
    getattr(d, which)[3] = None
    rc, msg = loss_refused(d)
    assert rc == -1 and "null pointer" in msg and "scale 3" in msg, msg


def test_ratios_that_are_no_integers():
    rc, msg = loss_refused(loss_desc(sizes=[(15, 25), (8, 13)], H=60, W=100))
    assert rc == -1 and "scale 1 (8 x 13) does not divide the ground truth (60 x 100)" in msg, msg
    rc, msg = loss_refused(loss_desc(sizes=[(64, 128), (32, 48)]))
    assert rc == -1 and "scale 1" in msg and "integer ratios" in msg, msg


def test_more_than_eight_scales_and_none():
    rc, msg = loss_refused(loss_desc(sizes=[(64, 128)] * 8, nscale=9))
    assert rc == -1 and "9 scales" in msg, msg
    rc, msg = loss_refused(loss_desc(nscale=0))
    assert rc == -1 and "0 scales" in msg, msg
    rc, msg = loss_refused(loss_desc(sizes=[(64, 128)] * 8, gt=None))           # eight pass the count (and stop at the null pointer)
    assert rc == -1 and "null pointer" in msg


@pytest.mark.parametrize("over", [dict(B=0), dict(H=0), dict(W=-128)])
def test_sizes_that_are_not_positive(over):
    rc, msg = loss_refused(loss_desc(**over))
    assert rc == -1 and "sizes must be positive" in msg, msg


def test_a_scale_that_is_not_positive():
    d = loss_desc()
    d.h[2] = 0
    rc, msg = loss_refused(d)
    assert rc == -1 and "scale 2" in msg and "sizes must be positive" in msg, msg


def test_a_kind_that_is_neither_loss():
    rc, msg = loss_refused(loss_desc(kind=2))
    assert rc == -1 and "kind 2" in msg, msg


def test_a_workspace_that_is_too_small():
    need = workspace(2, SIZES)
    rc, msg = loss_refused(loss_desc(ws_elems=need - 1))
    assert rc == -1 and f"the workspace holds {need - 1} doubles, {need} are needed" in msg, msg


# ---- the optimiser ---------------------------------------------------------------------------------------------------
def segs(*ns, **over):
    a = (L.AdamwSeg * max(len(ns), 1))()
    for i, n in enumerate(ns):
        a[i].p, a[i].g, a[i].m, a[i].v, a[i].n = P, P, P, P, n
    for k, v in over.items():
        setattr(a[0], k, v)
    return a


def hyper(**over):
    h = L.AdamwHyper(1e-4, 0.9, 0.999, 1e-8, 1e-4, 0.1, 0.001)
    for k, v in over.items():
        setattr(h, k, v)
    return h


def norm_refused(a, nseg, partials=P, partial_elems=1 << 20, norm_out=P):
    lib = L.lib()
    rc = lib.ufr_grad_norm(a, nseg, 1.0, partials, partial_elems, norm_out, None)
    return rc, lib.ufr_last_error().decode()


def step_refused(a, nseg, h):
    lib = L.lib()
    rc = lib.ufr_adamw_step(a, nseg, ctypes.byref(h) if h is not None else None, None, None)
    return rc, lib.ufr_last_error().decode()


def test_no_segments_succeed_and_launch_nothing():
    lib = L.lib()
    assert lib.ufr_grad_norm(None, 0, 1.0, None, 0, None, None) == 0
    assert lib.ufr_adamw_step(None, 0, ctypes.byref(hyper()), None, None) == 0
    assert lib.ufr_grad_norm_partials(None, 0) == 0


def test_the_partials_a_norm_needs():
    # one per workgroup: ceil(n / 4096) of them, at most 1024 per segment, none for an empty segment
    lib = L.lib()
    assert lib.ufr_grad_norm_partials(segs(1, 4096, 4097, 0, 39_175_298), 5) == 1 + 1 + 2 + 0 + 1024
    assert lib.ufr_grad_norm_partials(segs(-1), 1) == -1 and lib.ufr_grad_norm_partials(None, 2) == -1


@pytest.mark.parametrize("field", ["p", "g", "m", "v"])
def test_a_null_segment_pointer_with_elements_is_refused(field):
    rc, msg = step_refused(segs(7, 9, **{field: None}), 2, hyper())
    assert rc == -1 and "segment 0 has a null pointer with n = 7" in msg, msg
    if field == "g":                                          # the norm reads the gradients only
        rc, msg = norm_refused(segs(7, **{field: None}), 1)
        assert rc == -1 and "segment 0 has a null pointer with n = 7" in msg, msg


def test_a_negative_length_or_count_and_a_null_array():
    rc, msg = step_refused(segs(7, -2), 2, hyper())
    assert rc == -1 and "segment 1 has n = -2" in msg, msg
    rc, msg = norm_refused(segs(-5), 1)
    assert rc == -1 and "n = -5" in msg, msg
    rc, msg = step_refused(None, 3, hyper())
    assert rc == -1 and "null segment array" in msg, msg
    rc, msg = norm_refused(segs(1), -1)
    assert rc == -1 and "negative" in msg, msg


@pytest.mark.parametrize("over,word", [(dict(beta1=1.0), "beta1"), (dict(beta1=-0.1), "beta1"), (dict(beta2=1.5), "beta2"),
                                       (dict(eps=-1e-8), "eps"), (dict(lr=-1.0), "lr"), (dict(weight_decay=-1.0), "weight_decay"),
                                       (dict(bias1=0.0), "bias corrections"), (dict(bias2=1.5), "bias corrections")])
def test_hyperparameters_outside_their_range(over, word):
    rc, msg = step_refused(segs(7), 1, hyper(**over))
    assert rc == -1 and word in msg, msg
    with pytest.raises(RuntimeError, match=word):
        L.check(rc, "probe")


def test_null_hyperparameters():
    rc, msg = step_refused(segs(7), 1, None)
    assert rc == -1 and "null pointer" in msg, msg


def test_a_partials_buffer_that_is_too_small_or_missing():
    a = segs(4097, 10)                                        # 2 + 1 workgroups
    rc, msg = norm_refused(a, 2, partial_elems=2)
    assert rc == -1 and "partials holds 2 values, 3 are needed" in msg, msg
    rc, msg = norm_refused(a, 2, partials=None)
    assert rc == -1 and "null pointer (partials)" in msg, msg
    rc, msg = norm_refused(a, 2, norm_out=None)
    assert rc == -1 and "null pointer (norm_out)" in msg, msg
