"""What tests/golden/make_golden_validation.py and the validation tests share: a closed-form stand-in for a flow network in both
calling conventions of training/evaluate.py, and the seeded generators of the loader items.  The fixtures store seeds and results,
never frames: both sides rebuild the items from here, on the CPU, with the same float32 operations.

Items are the reference's batch-1 items: (image1, image2, flow_gt, valid), frames [1,3,H,W] of integer values 0..255, flow_gt
[1,2,H,W], valid [1,H,W].  The ground truth is a prediction plus noise whose scale varies per pixel over two decades, so that the
1px / 3px / 5px rates and KITTI's outlier share all lie well inside (0, 1); the makers assert it."""
import numpy as np
import torch
import torch.nn.functional as F


class StandIn(torch.nn.Module):
    """A fixed pointwise function of the two frames.  RAFT's convention: `model(image1, image2, iters=, test_mode=True)` with frames
    in 0..255 returns (coarse, flow); FlowNetC's: `model(image1, image2)` with frames in 0..1 returns the flow.  `gain` scales the
    flow (KITTI's outlier rule compares the error with 5 % of the ground truth's magnitude, so its flows are large)."""

    def __init__(self, gain=1.0):
        super().__init__()
        self.gain = float(gain)
        self.calls = []                  # the batch size of every call

    def flow(self, a, b):
        u = 6.0 * (a[:, 0] - b[:, 1]) + 2.0 * a[:, 2]
        v = 5.0 * (b[:, 0] - a[:, 1]) - 2.0 * b[:, 2]
        return torch.stack((u, v), 1) * self.gain

    def forward(self, image1, image2, iters=None, test_mode=False):
        self.calls.append(int(image1.shape[0]))
        if test_mode:
            flow = self.flow(image1 * 0.00390625, image2 * 0.00390625)           # / 256, exact
            return flow[:, :, ::8, ::8], flow
        return self.flow(image1, image2)


def frames(seed, H, W):
    g = torch.Generator().manual_seed(int(seed))
    return tuple(torch.randint(0, 256, (1, 3, H, W), generator=g).float() for _ in range(2))


def blocky_frames(seed, H, W):
    """Frames for a real network: constant 8 x 8 blocks plus a little pixel noise, in integer arithmetic.  A network's flow on white
    noise is itself noise at the pixel scale, and no coarse copy of it could serve as the base of a ground truth."""
    g = torch.Generator().manual_seed(int(seed))
    out = []
    for _ in range(2):
        base = torch.randint(32, 224, (1, 3, (H + 7) // 8, (W + 7) // 8), generator=g)
        base = base.repeat_interleave(8, 2).repeat_interleave(8, 3)[:, :, :H, :W]
        out.append((base + torch.randint(-8, 9, (1, 3, H, W), generator=g)).float())
    return tuple(out)


def noise(seed, H, W, scale):
    """[1,2,H,W]: normal noise times a per-pixel factor scale * (0.05 + 5 r^3), r uniform: two decades, median 0.7 * scale."""
    g = torch.Generator().manual_seed(int(seed) + 7919)
    n = torch.randn(1, 2, H, W, generator=g)
    r = torch.rand(1, 1, H, W, generator=g)
    return n * (scale * (0.05 + 5.0 * (r * r * r)))


def valid_mask(seed, H, W, share=0.5):
    """[1,H,W] of 0 / 1 with about `share` ones; share = 0: an item without a valid pixel."""
    g = torch.Generator().manual_seed(int(seed) + 104729)
    return (torch.rand(1, H, W, generator=g) < share).float()


def standin_items(specs, gain=1.0, flowNetC=False, scale=3.0):
    """specs: [(seed, H, W, share of valid pixels)].  The ground truth is the stand-in's own prediction plus noise."""
    model = StandIn(gain)
    items = []
    for seed, H, W, share in specs:
        image1, image2 = frames(seed, H, W)
        pred = model(image1 / 255.0, image2 / 255.0) if flowNetC else model(image1, image2, test_mode=True)[1]
        items.append((image1, image2, pred + noise(seed, H, W, scale), valid_mask(seed, H, W, share)))
    return items


def coarse_items(specs, coarse, scale):
    """Items for a real network: the ground truth is `coarse` ([N,2,h,w], the reference's prediction averaged over 8 x 8 blocks,
    stored in the fixture) resized to the frame, plus noise."""
    items = []
    for (seed, H, W, share), c in zip(specs, coarse):
        image1, image2 = blocky_frames(seed, H, W)
        c = torch.as_tensor(np.asarray(c, dtype=np.float32))[None]
        base = F.interpolate(c, scale_factor=8, mode="bilinear", align_corners=False)[:, :, :H, :W]
        items.append((image1, image2, base + noise(seed, H, W, scale), valid_mask(seed, H, W, share)))
    return items


def to_device(items, device):
    return [tuple(x.to(device) for x in item) for item in items]


def near_threshold(values, thresholds, rel):
    """How many of `values` lie within a relative `rel` of one of `thresholds`."""
    values = np.asarray(values, dtype=np.float64).ravel()
    return int(sum(np.count_nonzero(np.abs(values - th) <= rel * th) for th in thresholds))


# ---- the cases of tests/golden/validation_*.npz: name -> (validator, flowNetC, gain, specs or {"clean": specs, "final": specs}) ----
SMALL = (13, 19)                         # Sintel pad 1/2 rows and 2/3 columns, KITTI pad 0/3 rows and 2/3 columns
TALL = (380, 12)                         # KITTI pad 0/4 rows: the padded height is 384, which the flowNetC rule keeps
STANDIN_CASES = {
    "chairs": ("chairs", False, 1.0, [(11, 12, 20, 1.0), (12, 12, 20, 1.0), (13, 9, 13, 1.0)]),
    "chairs_fnc": ("chairs", True, 1.0, [(14, 12, 20, 1.0), (15, 12, 20, 1.0), (16, 9, 13, 1.0)]),
    "sintel": ("sintel", False, 1.0, {"clean": [(21, *SMALL, 1.0), (22, *SMALL, 1.0)], "final": [(23, *SMALL, 1.0), (24, *SMALL, 1.0)]}),
    "sintel_fnc": ("sintel", True, 1.0, {"clean": [(25, *SMALL, 1.0), (26, *SMALL, 1.0)], "final": [(27, *SMALL, 1.0), (28, *SMALL, 1.0)]}),
    # the third item has no valid pixel: its end-point error is NaN, and so is kitti-epe
    "kitti": ("kitti", False, 12.0, [(31, *SMALL, 0.5), (32, *SMALL, 0.4), (33, *SMALL, 0.0), (34, 9, 13, 0.6)]),
    "kitti_finite": ("kitti", False, 12.0, [(135, *SMALL, 0.5), (136, *SMALL, 0.4), (137, 9, 13, 0.6)]),
    # the second item's padded height is 16, not 384: flowNetC skips it
    "kitti_fnc": ("kitti", True, 12.0, [(41, *TALL, 0.5), (42, *SMALL, 0.5), (43, *TALL, 0.6)]),
    "kitti_fnc_all_skipped": ("kitti", True, 12.0, [(44, *SMALL, 0.5), (45, 9, 13, 0.5)]),
}
# real networks: RAFT (synthetic weights of seed 2, the network of raft_128x192.npz) on 128 x 192 padded frames, FlowNetC (seed 0)
# on chairs at 64 x 128
MODEL_CASES = {
    "raft_sintel": ("sintel", False, {"clean": [(51, 125, 187, 1.0), (52, 125, 187, 1.0)], "final": [(53, 125, 187, 1.0)]}),
    "raft_kitti": ("kitti", False, [(54, 121, 190, 0.5), (55, 121, 190, 0.6)]),
    "flownetc_chairs": ("chairs", True, [(56, 64, 128, 1.0), (57, 64, 128, 1.0)]),
}
RAFT_ITERS = 1
