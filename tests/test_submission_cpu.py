"""CPU suite of the submissions (validation.py: `forward_interpolate`, `create_sintel_submission`, `create_kitti_submission`;
kitti_io.py: the `.flo` and KITTI writers; csrc/submission.hip's entries as include/ufr_hip.h declares them).  The fixtures were
recorded from the reference (tests/golden/make_golden_submission.py); the loops run with `fused=False` and a stand-in model that
records the warm start it is handed."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

HEADER = os.path.join(ROOT, "include", "ufr_hip.h")
CASES = ("small", "medium", "sparse", "slices", "sintel", "invalid", "nan")
ENTRIES = ("ufr_forward_interpolate", "ufr_forward_interpolate_sliced", "ufr_flow_encode")


def _V():
    from understanding_flow_robustness_amd import validation as V
    return V


def _same_with_nans(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(np.isnan(got), np.isnan(want)) \
        and np.array_equal(np.nan_to_num(got), np.nan_to_num(want))


# ---------------------------------------------------------------------------------------------------------- 1. forward_interpolate
def test_the_fixture_is_what_its_generator_promises():
    z = load_golden("forward_interpolate")
    meta = json.loads(str(z["meta"]))
    assert set(meta) == set(CASES)
    for name in CASES:
        assert z["in_" + name].shape == z["out_" + name].shape and z["in_" + name].dtype == z["out_" + name].dtype == np.float32
        gap = meta[name]["smallest_gap"]
        assert (gap is None and meta[name]["valid_points"] == 0) or gap > 0          # tie-free: the rule fixes every output
    assert z["in_sintel"].shape == (2, 55, 128) and z["in_slices"].shape == (2, 33, 65) and z["in_sparse"].shape == (2, 17, 23)
    assert np.isnan(z["out_invalid"]).all() and np.isnan(z["in_nan"]).any() and not np.isnan(z["out_nan"]).any()
    assert meta["sparse"]["valid_points"] < 0.06 * meta["sparse"]["points"]


@pytest.mark.parametrize("leg", ["scipy", "brute-force"])
@pytest.mark.parametrize("name", CASES)
def test_host_restatement_reproduces_the_reference(name, leg):
    """Outputs are copies of inputs: equal, with NaNs in the same places."""
    if leg == "scipy":
        import scipy  # noqa: F401  (a dependency of the package, patch_transform.py: without it this leg fails, it does not skip)
    z = load_golden("forward_interpolate")
    got = _V()._interpolate_host(z["in_" + name], use_scipy=(leg == "scipy"))
    assert _same_with_nans(got, z["out_" + name])


def test_forward_interpolate_takes_items_and_batches_on_the_host():
    V = _V()
    z = load_golden("forward_interpolate")
    one = V.forward_interpolate(torch.from_numpy(z["in_small"]))
    assert one.dtype == torch.float32 and one.device.type == "cpu" and _same_with_nans(one.numpy(), z["out_small"])
    both = V.forward_interpolate(torch.from_numpy(np.stack([z["in_small"], z["in_invalid"]])).double())
    assert both.dtype == torch.float32 and tuple(both.shape) == (2, 2, 6, 10)
    assert _same_with_nans(both[0].numpy(), z["out_small"]) and bool(torch.isnan(both[1]).all())
    for bad in (torch.zeros(3, 4, 5), torch.zeros(4, 5), torch.zeros(1, 3, 4, 5)):
        with pytest.raises(ValueError, match=r"\[2,h,w\]"):
            V.forward_interpolate(bad)


def test_the_brute_force_gives_a_tie_to_the_lowest_index():
    """Two points land on (1.5, 1) and (2.5, 1) of a 3 x 4 grid; pixel (2, 1) is 0.25 away from both."""
    flow = np.full((2, 3, 4), 100.0, dtype=np.float32)
    flow[:, 0, 1] = (0.5, 1.0)               # source index 1 -> (1.5, 1.0)
    flow[:, 2, 3] = (-0.5, -1.0)             # source index 11 -> (2.5, 1.0)
    out = _V()._interpolate_host(flow, use_scipy=False)
    assert tuple(out[:, 1, 2]) == (0.5, 1.0) and tuple(out[:, 1, 3]) == (-0.5, -1.0) and tuple(out[:, 1, 1]) == (0.5, 1.0)


# ------------------------------------------------------------------------------------------------------------------ 2. the C entries
def _declared(name):
    """(return type, [ctypes type per parameter]) of `name` as the header declares it (tests/test_validation_cabi_cpu.py)."""
    from understanding_flow_robustness_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(int|long)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/ufr_hip.h"
    kinds = []
    for param in m.group(2).split(","):
        typ = re.sub(r"\w+\s*$", "", param.strip()).replace("const", "").replace(" ", "")
        kinds.append(L._vp if "*" in typ or typ == "ufr_stream_t" else {"int": L._i, "long": L._l, "float": L._f}[typ])
    return m.group(1), kinds


def test_entries_are_exported_and_match_the_signatures():
    from understanding_flow_robustness_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        ret, kinds = _declared(name)
        assert ret == "int" and kinds == L.SIGNATURES[name], (name, kinds)
    assert [len(L.SIGNATURES[n]) for n in ENTRIES] == [6, 7, 11]
    assert L.lib().ufr_abi_version() == 9                                       # additive entries: the ABI version stays
    m = re.search(r"#define\s+UFR_FORWARD_INTERPOLATE_SLICES\s+(\d+)\b", open(HEADER).read())
    assert m and int(m.group(1)) in (1, 4, 16)
    assert "submission" in L.source_checksums() and "submission" in L.lib().ufr_build_manifest().decode()


def _entries():
    p = ctypes.c_void_p(4096)
    return [
        #                                                      flow out B H W stream
        ("ufr_forward_interpolate", b"forward interpolate", [p, p, 2, 5, 7, None],
         [((0, None), b"null pointer"), ((1, None), b"null pointer"), ((2, 0), b"bad shape"), ((2, -3), b"bad shape"),
          ((3, 0), b"bad shape"), ((4, -1), b"bad shape"), ((2, 1 << 16), b"bad shape")]),
        #                                                             flow out B H W slices stream
        ("ufr_forward_interpolate_sliced", b"forward interpolate", [p, p, 2, 5, 7, 4, None],
         [((0, None), b"null pointer"), ((1, None), b"null pointer"), ((2, 0), b"bad shape"), ((3, -2), b"bad shape"),
          ((4, 0), b"bad shape"), ((5, 0), b"slices 0"), ((5, 2), b"slices 2"), ((5, 64), b"slices 64")]),
        #                                      pred out K Hp Wp top left H W mode stream
        ("ufr_flow_encode", b"flow encode", [p, p, 3, 8, 8, 1, 0, 5, 7, 0, None],
         [((0, None), b"null pointer"), ((1, None), b"null pointer"), ((2, 0), b"bad shape"), ((2, -1), b"bad shape"),
          ((3, 0), b"bad shape"), ((4, -1), b"bad shape"), ((7, 0), b"bad shape"), ((8, 0), b"bad shape"),
          ((5, -1), b"negative pad"), ((6, -1), b"negative pad"),
          ((5, 4), b"leaves the padded frame"), ((6, 2), b"leaves the padded frame"), ((7, 8), b"leaves the padded frame"),
          ((3, 5), b"leaves the padded frame"), ((8, 9), b"leaves the padded frame"),
          ((9, 2), b"mode 2"), ((9, -1), b"mode -1")]),
    ]


def test_entries_refuse_bad_arguments_before_any_launch():
    """Each refusal returns UFR_EINVAL (-1) with the entry's own message; the pointers are never dereferenced, so this runs
    without a GPU."""
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
    # H * W beyond the entries' arithmetic, each side acceptable on its own
    big = 1 << 15
    assert lib.ufr_forward_interpolate(ctypes.c_void_p(4096), ctypes.c_void_p(4096), 1, big, big, None) == -1
    assert b"too many pixels" in lib.ufr_last_error()
    assert lib.ufr_flow_encode(ctypes.c_void_p(4096), ctypes.c_void_p(4096), 1, big, big, 0, 0, 4, 4, 0, None) == -1
    assert b"too many pixels" in lib.ufr_last_error()


def test_args_program_runs_clean_under_host_sanitizers(tmp_path):
    """tests/host/submission_args_main.cpp with the host side of the two translation units it needs under AddressSanitizer and
    UBSan (`-Xarch_host`); the device code is not instrumented and nothing is loaded into python (the pattern of
    test_validation_cabi_cpu.py)."""
    import subprocess
    if torch.cuda.is_available():
        pytest.skip("sanitizer builds run on the build machine, never beside a GPU")
    csrc = os.path.join(ROOT, "understanding_flow_robustness_amd", "csrc")
    exe = str(tmp_path / "submission_args")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function"]
    for flag in ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"):
        cmd += ["-Xarch_host", flag]
    cmd += [os.path.join(csrc, "capi.hip"), os.path.join(csrc, "submission.hip"),
            os.path.join(ROOT, "tests", "host", "submission_args_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    ran = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr[-2000:]
    assert "all refused, 0 failures" in ran.stdout and "runtime error" not in ran.stderr and "AddressSanitizer" not in ran.stderr


# ---------------------------------------------------------------------------------------------------------------------- 3. writers
def test_write_flo_writes_the_references_bytes_and_reads_them_back(tmp_path):
    from understanding_flow_robustness_amd import kitti_io
    z = load_golden("submission_writers")
    flow = z["flo_flow"]
    assert flow.shape == (5, 7, 2)
    path = str(tmp_path / "frame0001.flo")
    kitti_io.write_flo(path, flow)
    with open(path, "rb") as f:
        raw = f.read()
    assert raw == z["flo_bytes"].tobytes() and raw[:4] == b"PIEH" and len(raw) == 12 + 5 * 7 * 2 * 4
    back = kitti_io.read_flo(path)
    assert back.dtype == np.float32 and np.array_equal(back, flow.astype(np.float32))
    kitti_io.write_flo(path, flow[:, ::2])                                     # a view that is not contiguous
    assert np.array_equal(kitti_io.read_flo(path), flow[:, ::2].astype(np.float32))
    with pytest.raises(ValueError):
        kitti_io.write_flo(path, flow.transpose(2, 0, 1))
    with open(path, "wb") as f:
        f.write(raw[:-4])
    with pytest.raises(ValueError):
        kitti_io.read_flo(path)


def test_write_flow_kitti_writes_the_references_pixels(tmp_path):
    """`png_read` of the file = the array the reference handed to cv2.imwrite, its BGR order reversed to the file's RGB."""
    from understanding_flow_robustness_amd import kitti_io
    z = load_golden("submission_writers")
    flow, bgr = z["kitti_flow"], z["kitti_imwrite_bgr"]
    assert flow.shape == (5, 7, 2) and float(np.abs(flow).max()) < 400 and bgr.dtype == np.uint16
    path = str(tmp_path / "000000_10.png")
    kitti_io.write_flow_kitti(path, flow)
    rgb = kitti_io.png_read(path)
    assert rgb.dtype == np.uint16 and np.array_equal(rgb, bgr[..., ::-1]) and bool((rgb[..., 2] == 1).all())
    kitti_io.write_flow_kitti(path, np.ascontiguousarray(bgr[..., ::-1]))      # the codes themselves
    assert np.array_equal(kitti_io.png_read(path), bgr[..., ::-1])
    u, v, valid = kitti_io.flow_read_png(path)                                  # and the existing reader decodes them
    assert float(np.abs(np.stack([u, v], -1) - flow).max()) <= 1.0 / 64.0 and bool((valid == 1).all())


def test_kitti_codes_clamp_what_numpy_leaves_undefined():
    from understanding_flow_robustness_amd import kitti_io
    uv = np.array([[[-600.0, 600.0], [np.nan, 0.0], [-512.0, 511.99], [-512.01, 512.0], [np.inf, -np.inf]]], dtype=np.float32)
    codes = kitti_io.flow_kitti_codes(uv)
    assert codes.dtype == np.uint16 and codes.shape == (1, 5, 3)
    assert codes[0, :, :2].tolist() == [[0, 65535], [0, 32768], [0, 65535], [0, 65535], [65535, 0]] and codes[0, :, 2].tolist() == [1] * 5


# ------------------------------------------------------------------------------------------------------------------------ 4. loops
class RecordingStandIn(torch.nn.Module):
    """RAFT's calling convention on padded frames: flow_low [N,2,H/8,W/8] and flow_up [N,2,H,W] from the frames' difference and the
    warm start; every call's `flow_init` is kept."""

    def __init__(self):
        super().__init__()
        self.calls, self.was_training = [], []

    def forward(self, image1, image2, iters=12, flow_init=None, test_mode=False):
        assert test_mode and image1.shape[2] % 8 == 0 and image1.shape[3] % 8 == 0 and not torch.is_grad_enabled()
        self.calls.append((tuple(image1.shape), iters, None if flow_init is None else flow_init.clone()))
        self.was_training.append(self.training)
        difference = image1 - image2                                          # elementwise throughout: stacking items changes no bit
        low = 0.001953125 * difference[:, :2, ::8, ::8]                      # within half a cell: warm starts keep valid points
        if flow_init is not None:
            low = low + 0.5 * flow_init
        up = torch.nn.functional.interpolate(low, scale_factor=8, mode="nearest") + 0.03125 * difference[:, 2:]
        return low, up


def _frames(seed, h, w):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (1, 3, h, w), generator=g).float(), torch.randint(0, 256, (1, 3, h, w), generator=g).float())


def _sintel_loaders(collated):
    """Two sequences of three and two 12 x 20 frames per pass (padded to 16 x 24)."""
    def tail(sequence, frame):
        return ([sequence], torch.tensor([frame])) if collated else (sequence, frame)
    make = lambda base: [_frames(base + i, 12, 20) + (tail(seq, fr),)
                         for i, (seq, fr) in enumerate([("alley", 0), ("alley", 1), ("alley", 2), ("cave", 0), ("cave", 1)])]
    return {"clean": make(10), "final": make(20)}


@pytest.mark.parametrize("collated", [False, True], ids=["plain-items", "collated-items"])
@pytest.mark.parametrize("warm_start", [False, True], ids=["cold", "warm-start"])
def test_sintel_loop_writes_the_references_files(tmp_path, warm_start, collated):
    from understanding_flow_robustness_amd import kitti_io
    V = _V()
    model = RecordingStandIn().train()
    loaders = _sintel_loaders(collated)
    out = str(tmp_path / "sintel")
    assert V.create_sintel_submission(model, 7, warm_start, out, loaders=loaders, fused=False) is None
    assert model.was_training == [False] * 10 and len(model.calls) == 10 and all(c[:2] == ((1, 3, 16, 24), 7) for c in model.calls)
    names = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    assert names == sorted(f"{ds}/{seq}/frame{fr:04d}.flo" for ds in ("clean", "final")
                           for seq, frs in (("alley", (1, 2, 3)), ("cave", (1, 2))) for fr in frs)       # frame + 1
    # the chain, restated: a sequence starts cold; under warm_start the next frame starts from the interpolated flow_low
    replay, k = RecordingStandIn().eval(), 0
    for dstype in ("clean", "final"):
        previous, low = None, None
        for image1, image2, (sequence, frame) in _sintel_loaders(False)[dstype]:
            want_init = V.forward_interpolate(low[0])[None] if warm_start and sequence == previous else None
            got_init = model.calls[k][2]
            assert (got_init is None) == (want_init is None)
            if want_init is not None:
                assert tuple(got_init.shape) == (1, 2, 2, 3) and torch.equal(got_init, want_init) and bool(torch.isfinite(want_init).all())
            padder = V.InputPadder(image1.shape)
            with torch.no_grad():
                low, up = replay(*padder.pad(image1, image2), iters=7, flow_init=want_init, test_mode=True)
            written = kitti_io.read_flo(os.path.join(out, dstype, sequence, "frame%04d.flo" % (frame + 1)))
            assert written.shape == (12, 20, 2) and np.array_equal(written, padder.unpad(up[0]).permute(1, 2, 0).numpy())
            previous, k = sequence, k + 1
    assert any(c[2] is not None for c in model.calls) == warm_start


def test_kitti_loop_writes_the_references_files(tmp_path):
    from understanding_flow_robustness_amd import kitti_io
    V = _V()
    model = RecordingStandIn().train()
    items = [_frames(30, 13, 19) + (("000000_10.png",),), _frames(31, 13, 19) + ((["000001_10.png"],),), _frames(32, 9, 17) + (("000002_10.png",),)]
    out = str(tmp_path / "made" / "kitti")
    assert V.create_kitti_submission(model, 5, out, loader=items, fused=False) is None
    assert sorted(os.listdir(out)) == ["000000_10.png", "000001_10.png", "000002_10.png"]
    assert model.was_training == [False] * 3 and [c[:2] for c in model.calls] == [((1, 3, 16, 24), 5)] * 3 and all(c[2] is None for c in model.calls)
    replay = RecordingStandIn().eval()
    for (image1, image2, _), name in zip(items, sorted(os.listdir(out))):
        padder = V.InputPadder(image1.shape, mode="kitti")
        assert padder._pad[2] == 0                                            # KITTI pads at the bottom only
        with torch.no_grad():
            _, up = replay(*padder.pad(image1, image2), iters=5, test_mode=True)
        flow = padder.unpad(up[0]).permute(1, 2, 0).numpy()
        rgb = kitti_io.png_read(os.path.join(out, name))
        assert rgb.shape == flow.shape[:2] + (3,) and np.array_equal(rgb, kitti_io.flow_kitti_codes(flow))
        assert np.array_equal(rgb[..., :2], (64.0 * flow + 2 ** 15).astype(np.uint16))      # in range: the reference's own cast


def test_a_missing_loader_raises_value_error(tmp_path):
    V = _V()
    model = RecordingStandIn()
    out = str(tmp_path / "nothing")
    with pytest.raises(ValueError, match="create_sintel_submission"):
        V.create_sintel_submission(model, output_path=out)
    with pytest.raises(ValueError, match=r"create_sintel_submission \(final\)"):
        V.create_sintel_submission(model, output_path=out, loaders={"clean": []})
    with pytest.raises(ValueError, match="create_kitti_submission"):
        V.create_kitti_submission(model, output_path=out)
    assert model.calls == [] and not os.path.exists(out)
    with pytest.raises(RuntimeError, match="HIP device tensor"):                # fused=True has no CPU path
        V.create_kitti_submission(model, output_path=out, loader=[_frames(1, 8, 8) + (("a.png",),)])
