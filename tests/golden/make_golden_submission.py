"""Fixtures of the submissions (understanding_flow_robustness_amd/validation.py: `forward_interpolate`, the `.flo` and KITTI writers),
produced by running the REFERENCE on the CPU (see make_golden.py for the contract):

forward_interpolate.npz   inputs and outputs of models/raft/utils/utils.py:33-59 for the cases below.  CONDITION, checked here for
                          every case and every grid pixel: the float64 gap between the nearest and the second-nearest squared
                          distance is > 0 (an input with a tie is replaced by the next seed; the reference's choice at a tie is its
                          KD-tree's), and a float64 brute force -- lowest index first -- reproduces the reference's output exactly.
                          The smallest gap of every case is recorded.
submission_writers.npz    a 5 x 7 flow, the bytes dataset_utils/data_utils.py:228-256 (`writeFlow`) writes for it, and the array
                          `writeFlowKITTI` (:274-278) hands to cv2.imwrite (the stub below records it) for a 5 x 7 flow with
                          |flow| < 400."""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import save  # noqa: E402
import ref_harness as rh  # noqa: E402

#        name        h    w   sigma  what
CASES = (("small", 6, 10, 3.0, None),
         ("medium", 16, 24, 8.0, None),
         ("sparse", 17, 23, 40.0, None),           # ~4 % of the points stay inside: far-away neighbours
         ("slices", 33, 65, 10.0, None),           # more than one LDS slice of source points, more than one target tile
         ("sintel", 55, 128, 10.0, None),          # Sintel's 1/8 grid
         ("invalid", 6, 10, 0.0, "invalid"),       # every point leaves the grid: all outputs NaN
         ("nan", 16, 24, 8.0, "nan"))              # NaN entries: those points are invalid


def make_input(h, w, sigma, what, seed):
    g = torch.Generator().manual_seed(seed)
    if what == "invalid":
        return (1000.0 + torch.rand(2, h, w, generator=g)).float()
    flow = (sigma * torch.randn(2, h, w, generator=g)).float()
    if what == "nan":
        hit = torch.rand(h, w, generator=g) < 0.1
        flow[0][hit] = float("nan")
        flow[1][torch.rand(h, w, generator=g) < 0.05] = float("nan")
    return flow


def brute_force(flow):
    """-> (the rule's output, the smallest gap between the nearest and the second-nearest squared distance; inf without two points)."""
    flow = flow.numpy()
    dx, dy = flow[0].reshape(-1), flow[1].reshape(-1)
    h, w = flow.shape[1:]
    gx, gy = (np.arange(h * w) % w).astype(np.float64), (np.arange(h * w) // w).astype(np.float64)
    x1, y1 = gx + dx.astype(np.float64), gy + dy.astype(np.float64)
    with np.errstate(invalid="ignore"):
        valid = np.nonzero((x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h))[0]
    if valid.size == 0:
        return np.full((2, h, w), np.nan, np.float32), float("inf"), 0
    out, gap = np.empty((2, h * w), np.float32), float("inf")
    for s in range(0, h * w, 256):
        ex, ey = x1[valid][None, :] - gx[s:s + 256, None], y1[valid][None, :] - gy[s:s + 256, None]
        d2 = ex * ex + ey * ey
        near = np.argmin(d2, axis=1)
        if valid.size > 1:
            two = np.partition(d2, 1, axis=1)[:, :2]
            gap = min(gap, float((two[:, 1] - two[:, 0]).min()))
        out[0, s:s + 256], out[1, s:s + 256] = dx[valid[near]], dy[valid[near]]
    return out.reshape(2, h, w), gap, int(valid.size)


def gen_forward_interpolate():
    ref = rh.ref_module("models.raft.utils.utils").forward_interpolate
    arrays, meta = {}, {}
    for index, (name, h, w, sigma, what) in enumerate(CASES):
        for seed in range(100 * index, 100 * index + 20):
            flow = make_input(h, w, sigma, what, seed)
            mine, gap, n_valid = brute_force(flow)
            if gap > 0:
                break
        else:
            raise AssertionError(f"{name}: no tie-free input among 20 seeds")
        theirs = ref(flow)
        assert theirs.dtype == torch.float32 and tuple(theirs.shape) == (2, h, w)
        theirs = theirs.numpy()
        assert np.array_equal(np.isnan(theirs), np.isnan(mine)) and np.array_equal(np.nan_to_num(theirs), np.nan_to_num(mine)), \
            f"{name}: the float64 brute force does not reproduce the reference"
        if what == "invalid":
            assert n_valid == 0 and np.isnan(theirs).all()
        if what == "nan":
            assert np.isnan(flow.numpy()).any() and not np.isnan(theirs).any()
        arrays["in_" + name], arrays["out_" + name] = flow, theirs
        meta[name] = {"seed": seed, "sigma": sigma, "valid_points": n_valid, "points": h * w,
                      "smallest_gap": gap if np.isfinite(gap) else None}
        print(name, meta[name])
    save("forward_interpolate", meta=np.array(json.dumps(meta)), **arrays)


def gen_writers():
    du = rh.ref_module("dataset_utils.data_utils")
    g = torch.Generator().manual_seed(7)
    flow = (20.0 * torch.randn(5, 7, 2, generator=g)).numpy()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "frame0001.flo")
        du.writeFlow(path, flow)
        with open(path, "rb") as f:
            flo_bytes = np.frombuffer(f.read(), dtype=np.uint8)
    kitti = (399.0 * (2.0 * torch.rand(5, 7, 2, generator=g) - 1.0)).numpy()
    handed = []
    du.cv2.imwrite = lambda filename, array: handed.append((filename, np.array(array)))
    du.writeFlowKITTI("000000_10.png", kitti)
    (filename, bgr), = handed
    assert filename == "000000_10.png" and bgr.dtype == np.uint16 and bgr.shape == (5, 7, 3)
    save("submission_writers", flo_flow=flow, flo_bytes=flo_bytes, kitti_flow=kitti, kitti_imwrite_bgr=bgr)


if __name__ == "__main__":
    rh.install()
    gen_forward_interpolate()
    gen_writers()
