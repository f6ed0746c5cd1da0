"""Feature-map capture, replacement and layer embeddings: the two analyses the reference locates a network's vulnerability with.

    feature replacement   patch_attacks/test_replace_features.py: a pair is run with a uniform patch and chosen intermediate
                          features are kept; the pair is run again with the adversarial patch while those features are
                          overwritten; the two flows are compared                                   -> `replace_features`
    layer embeddings      patch_attacks/test_patch_embeddings.py: the spatial mean of every feature map with and without
                          the patch over a dataset, then the maximum mean discrepancy per layer    -> `layer_embeddings`

Both go through `predict_flow(..., return_feat_maps=True, overwrite_feat_maps=...)` and `get_feature_map_keys`
(models/utils_model.py:160-681), which `flownets/utils_model.py` serves with the functions of this file.

Served: FlowNetC and the Robust FlowNetC family (one head engine, the reference's 28 keys, utils_model.py:283-316); overwriting is
FlowNetC's alone (models/FlowNetC.py:121-155 -- the reference's Robust FlowNetC forward takes no `overwrite_feat_maps`).

On the native path (frozen or no-grad, eval, HIP float32, frame sides multiples of 64, UFR_ENGINE=1) nothing is computed for the
analysis: after a forward every map already sits in a plane buffer of the stem graph or the head engine
(`FlowNetCHeadEngine.segment_map`).  Capture converts the chunks it is asked for, the statistics kernel (csrc/feature_stats.hip)
sums them where they lie, and a replaced map is a chunk range the second forward does not recompute.  Everywhere else the torch
spelling (`FlowNetC.forward_torch_maps`) records the same 28 maps.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib as L

# models/utils_model.py:287-316, in the reference's order
FLOWNETC_KEYS = ["conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "corr", "conv_redir", "conv3_1", "conv4", "conv4_1", "conv5",
                 "conv5_1", "conv6", "conv6_1", "flow6", "upsampled_flow6_to_5", "deconv5", "flow5", "upsampled_flow5_to_4", "deconv4",
                 "flow4", "upsampled_flow4_to_3", "deconv3", "flow3", "upsampled_flow3_to_2", "deconv2", "predict"]
# what models/FlowNetC.py:121-155 reads from `overwrite_feat_maps`; conv3a / conv3b only as a pair
EFFECTIVE_KEYS = ("conv3a", "conv3b", "corr", "conv_redir", "conv3_1")
SERVED = "FlowNetC and the Robust FlowNetC family (FlowNetCFlexLarger_*)"


def served(args) -> bool:
    """The reference's own test (utils_model.py:163-166, :283-286)."""
    name = args.flownet
    return name in ("FlowNetC", "FlowNetC_original", "FlowNetCFlexLarger_k3_reps3") or "FlowNetCFlexLarger" in name


def _refuse(args):
    raise NotImplementedError(f"feature maps of {args.flownet!r}: capture, replacement and layer embeddings serve {SERVED}")


def get_feature_map_keys(args) -> list:
    """models/utils_model.py:282-316 for the served networks."""
    if not served(args):
        _refuse(args)
    return list(FLOWNETC_KEYS)


def compute_feature_map(feature_map: np.ndarray, computation_type: str = "mean") -> np.ndarray:
    """models/utils_model.py:439-442."""
    assert computation_type in ["mean"]
    return np.mean(feature_map, axis=(-2, -1))


# ---------------------------------------------------------------------------------------------------- the two spellings
def _is_flownetc_family(net) -> bool:
    from .flownets.flownetc import FlowNetC
    return isinstance(net, FlowNetC)


def native_ok(net, x) -> bool:
    """The analysis path's own gate (the attack's `_engine_ok` / `engine_available` are not involved): the engines serve `net`
    on the frames `x` -- frozen parameters or no autograd, eval mode, HIP float32, sides multiples of 64, UFR_ENGINE=1, a stem
    the native prefix serves."""
    return _is_flownetc_family(net) and net.stem_refusal() is None and L.engine_refusal(net, x, 64) is None


def _native_forward(net, x1, x2, overwrite=None, keep=(), computed=None):
    """One forward of the stem graph and the head engine -> (flow, engine, stem graph); the maps stay in their planes."""
    from .flownetc_engine import get_engine
    from .plane_graph import graph_for, stem_graph
    B, _, H, W = x1.shape
    with torch.no_grad():
        x = net.normalize_correctly(torch.cat((x1, x2), 0))
        n = 2 * B
        stem = graph_for(net, ("stem", n, H, W, str(x.device)), lambda: stem_graph(net, n, H, W, 3, x.device))
        c2, c3 = stem.forward(x)
        eng = get_engine(net, B, H, W, x.device)
        c2a, c3a, c3b = c2[:B].contiguous(), c3[:B].contiguous(), c3[B:].contiguous()
        eng.generation = getattr(eng, "generation", 0) + 1     # a pending autograd backward of this engine is stale now
        if overwrite or keep or computed is not None:
            flow2 = eng.forward_replaced(c2a, c3a, c3b, overwrite, keep, computed)
        else:
            flow2 = eng.forward(c2a, c3a, c3b)
        flow = F.interpolate(flow2 * net.div_flow, scale_factor=4, mode="bilinear", align_corners=False)
    return flow, eng, stem


def _batched(overwrite, B, device):
    """Overwrite values as float32 [B,C,H,W] on `device`: numpy [C,H,W] (the reference's form, sample 0) or tensors [B,C,H,W]."""
    out = {}
    for k, v in (overwrite or {}).items():
        t = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v
        if t.dim() == 3:
            t = t.unsqueeze(0)
        out[k] = t.to(device=device, dtype=torch.float32)
    return out


def forward_with_maps(net, x1, x2, overwrite=None, keys=None):
    """(flow, {key: [B,C,h,w] float32}) with the computed value of every key (all 28 by default), also where `overwrite`
    replaces it afterwards: the reference appends its clones before it overwrites and its hooks see module outputs."""
    if not _is_flownetc_family(net):
        raise NotImplementedError(f"feature maps of {type(net).__name__}: {SERVED}")
    ow = _batched(overwrite, x1.shape[0], x1.device)
    if ow and type(net).__name__ != "FlowNetC":
        raise NotImplementedError(f"{type(net).__name__}: the reference overwrites feature maps in FlowNetC only")
    if native_ok(net, x1):
        computed = {} if ow else None
        flow, eng, stem = _native_forward(net, x1, x2, ow, (), computed)
        want = list(FLOWNETC_KEYS if keys is None else keys)
        maps = eng.capture([k for k in want if k not in (computed or {})], stem)
        maps.update({k: v for k, v in (computed or {}).items() if k in want})
        return flow, {k: maps[k] for k in want}
    with torch.no_grad():
        flow, maps = net.forward_torch_maps(x1, x2, ow)
    return flow, {k: maps[k].clone() for k in (FLOWNETC_KEYS if keys is None else keys)}


def forward_overwritten(net, x1, x2, overwrite):
    """`FlowNetC.forward(x1, x2, overwrite_feat_maps=...)`: the flow, or (flow, the seven copied maps) for a network built with
    return_feat_maps=True (models/FlowNetC.py:194-197)."""
    ow = _batched(overwrite, x1.shape[0], x1.device)
    if type(net).__name__ != "FlowNetC":
        raise NotImplementedError(f"{type(net).__name__}: the reference overwrites feature maps in FlowNetC only")
    copied = ("conv1a", "conv2a", "conv3a", "conv1b", "conv2b", "conv3b", "corr")
    if net.return_feat_maps:
        flow, maps = forward_with_maps(net, x1, x2, ow, copied)
        return flow, [maps[k] for k in copied]
    if native_ok(net, x1):
        return _native_forward(net, x1, x2, ow)[0]
    with torch.no_grad():
        return net.forward_torch_maps(x1, x2, ow)[0]


# ---------------------------------------------------------------------------------------------------- statistics
class _StatsPlan:
    """The segment table of one forward's statistics: every key's columns in one [B, columns] float64 matrix."""

    def __init__(self, segments: dict, keys, B: int, device):
        self.keys, self.B = list(keys), int(B)
        self.cols, table, col = {}, [], 0
        for key in self.keys:
            src, c0, cn, img0, post = segments[key]
            planes = not isinstance(src, torch.Tensor)
            t = src.t if planes else src
            s = L.FeatureStatsSeg()
            s.src, s.kind = t.data_ptr(), 0 if planes else 1
            s.plane_stride = src.plane_stride if planes else t.numel()
            s.pixels, s.images = (src.H * src.W, src.B) if planes else (t.shape[2] * t.shape[3], t.shape[0])
            s.image0, s.B, s.chunk0, s.channels = int(img0), self.B, int(c0), int(cn)
            s.unleaky, s.out_col = (0.1 if post == "unleaky" else 0.0), col
            table.append(s)
            self.cols[key] = (col, cn, float(s.pixels))
            col += cn
        self.width = col
        self.calls = []                                           # UFR_FEATURE_STATS_MAX_SEGS segments per call
        for i in range(0, len(table), L.UFR_FEATURE_STATS_MAX_SEGS):
            part = table[i:i + L.UFR_FEATURE_STATS_MAX_SEGS]
            arr = (L.FeatureStatsSeg * len(part))(*part)
            need = L.lib().ufr_feature_stats_workspace_doubles(arr, len(part))
            if need < 0:
                L.check(-1, "feature stats")
            self.calls.append((arr, len(part), torch.empty(max(int(need), 1), dtype=torch.float64, device=device)))
        self.out = torch.zeros(self.B, max(self.width, 1), dtype=torch.float64, device=device)

    def run(self) -> torch.Tensor:
        for arr, n, ws in self.calls:
            L.check(L.lib().ufr_feature_stats(arr, n, L.ptr(ws), ws.numel(), L.ptr(self.out), self.B, self.width, self.out.stride(0),
                                              L.stream()), "feature stats")
        return self.out


def plane_sums(segments: dict, keys, B: int, device) -> dict:
    """{key: float64 [B, channels] sums over the pixels} of segments given as `FlowNetCHeadEngine.segment_map` gives them:
    (Planes | NCHW float32 tensor, first chunk (channel), channels, first image, "unleaky" | None)."""
    plan = _StatsPlan(segments, keys, B, device)
    out = plan.run()
    return {k: out[:, c:c + n] for k, (c, n, _) in plan.cols.items()}


def feature_means(flow_net, tgt, ref, args=None, keys=None) -> dict:
    """{key: float64 numpy [B, C]} = the spatial mean of every feature map of one forward (what test_patch_embeddings.py:
    compute_feature_map(fm, "mean") takes of each map of `predict_flow(..., return_feat_maps=True)`), for the whole batch.
    Native path: one forward, the statistics kernel over the planes, one host read of [B, sum of channels] doubles -- no feature
    map leaves the device or is converted.  Elsewhere: the torch spelling's maps, averaged in float64."""
    if args is not None and not served(args):
        _refuse(args)
    want = list(FLOWNETC_KEYS if keys is None else keys)
    if native_ok(flow_net, tgt):
        _, eng, stem = _native_forward(flow_net, tgt, ref)
        plans = L.engine_cache(flow_net, "_ufr_feature_stats_plans")
        pkey = (id(eng), id(stem), tuple(want))
        plan = plans.get(pkey)
        if plan is None or plan.eng is not eng or plan.stem is not stem:
            plan = plans[pkey] = _StatsPlan(eng.segment_map(stem), want, eng.B, tgt.device)
            plan.eng, plan.stem = eng, stem                    # (the table points into their buffers)
        host = plan.run().cpu().numpy()
        return {k: host[:, c:c + n] / px for k, (c, n, px) in plan.cols.items()}
    _, maps = forward_with_maps(flow_net, tgt, ref, None, want)
    return {k: maps[k].double().mean((2, 3)).cpu().numpy() for k in want}


# ---------------------------------------------------------------------------------------------------- layer embeddings
def maximum_mean_discrepancy(source, target) -> float:
    """patch_attacks/test_patch_embeddings.py:130-162: the five-bandwidth Gaussian-kernel MMD estimate between two sample clouds
    [n, C] (numpy or tensors; the arithmetic runs in their dtype on the host, as in the reference).  n x n x C: not a hot path.
    NaN when all samples coincide (bandwidth 0), as in the reference; callers map it to 0 like the script (:360)."""
    source = torch.from_numpy(np.ascontiguousarray(source)) if isinstance(source, np.ndarray) else source.detach().cpu()
    target = torch.from_numpy(np.ascontiguousarray(target)) if isinstance(target, np.ndarray) else target.detach().cpu()
    kernel_mul, kernel_num = 2.0, 5
    n = int(source.size(0)) + int(target.size(0))
    total = torch.cat([source, target], dim=0)
    total0 = total.unsqueeze(0).expand(n, n, int(total.size(1)))
    total1 = total.unsqueeze(1).expand(n, n, int(total.size(1)))
    l2 = ((total0 - total1) ** 2).sum(2)
    bandwidth = torch.sum(l2) / (n ** 2 - n)
    bandwidth = bandwidth / kernel_mul ** (kernel_num // 2)
    kernels = sum(torch.exp(-l2 / (bandwidth * (kernel_mul ** i))) for i in range(kernel_num))
    m = int(source.size(0))
    xx, yy, xy, yx = kernels[:m, :m], kernels[m:, m:], kernels[:m, m:], kernels[m:, :m]
    return torch.mean(xx + yy - xy - yx).numpy().item()


def layer_embeddings(flow_net, pairs_clean, pairs_patched, args, keys=None):
    """The loop of test_patch_embeddings.py:240-365 without its plots: `pairs_clean` / `pairs_patched` are iterables of
    (tgt, ref) frame batches (the same scenes without and with the patch).  -> ({key: (with [n,C], without [n,C])} float64,
    {key: MMD(with, without), NaN mapped to 0}) -- the second is what the script writes to embedding_mmds.json.  t-SNE / UMAP of
    the matrices stay with the caller."""
    if not served(args):
        _refuse(args)
    want = list(FLOWNETC_KEYS if keys is None else keys)
    rows = {k: ([], []) for k in want}
    for slot, pairs in ((1, pairs_clean), (0, pairs_patched)):
        for tgt, ref in pairs:
            means = feature_means(flow_net, tgt, ref, args, want)
            for k in want:
                rows[k][slot].append(means[k])
    emb = {k: (np.concatenate(w, 0), np.concatenate(wo, 0)) for k, (w, wo) in rows.items()}
    mmds = {}
    for k, (w, wo) in emb.items():
        v = maximum_mean_discrepancy(w, wo)
        mmds[k] = 0.0 if np.isnan(v) else v
    return emb, mmds


# ---------------------------------------------------------------------------------------------------- feature replacement
def check_replaceable(keys) -> None:
    """A key the model never reads, or half of the conv3 pair, would make the replacement a silent no-op."""
    keys = list(keys)
    unread = [k for k in keys if k not in EFFECTIVE_KEYS]
    if unread:
        raise ValueError(f"replace_features: FlowNetC never reads {', '.join(map(repr, unread))} from overwrite_feat_maps "
                         f"(models/FlowNetC.py:121-155 reads {', '.join(EFFECTIVE_KEYS)})")
    if ("conv3a" in keys) != ("conv3b" in keys):
        raise ValueError("replace_features: conv3a and conv3b take effect only together (models/FlowNetC.py:121-131)")


def replace_features(flow_net, donor_frames, recipient_frames, flow_gt, mask, keys, args=None):
    """The body of test_replace_features.py:304-426 for a batch: `donor_frames` = (tgt, ref) with the uniform patch,
    `recipient_frames` = (tgt, ref) with the adversarial patch, both [B,3,H,W]; the recipient's forward runs with the donor's
    `keys` features.  flow_gt [B,2|3,Hg,Wg]; `mask` [B,1|3,H,W] or None: where it is set the ground truth is blended towards the
    patch's zero motion (valid 1), test_replace_features.py:398-418.
    Native path: the zero-copy form -- the donor's forward leaves its maps in the engine's planes and the recipient's forward,
    on the same engine, skips the launches that would overwrite the `keys` segments; nothing is captured or injected.
    -> dict(flow, adv_flow, epe, adv_epe, cos_sim, adv_cos_sim) (the four metrics as floats, losses.py)."""
    from .losses import compute_cossim, compute_epe
    if args is not None and args.flownet != "FlowNetC":
        raise NotImplementedError(f"replace_features({args.flownet!r}): the reference overwrites feature maps in FlowNetC only")
    if type(flow_net).__name__ != "FlowNetC":
        raise NotImplementedError(f"replace_features: {type(flow_net).__name__}; the reference overwrites feature maps in FlowNetC only")
    check_replaceable(keys)
    (d_tgt, d_ref), (r_tgt, r_ref) = donor_frames, recipient_frames
    if native_ok(flow_net, d_tgt) and d_tgt.shape == r_tgt.shape:
        flow = _native_forward(flow_net, d_tgt, d_ref)[0]
        adv_flow = _native_forward(flow_net, r_tgt, r_ref, None, tuple(keys))[0]
    else:
        flow, maps = forward_with_maps(flow_net, d_tgt, d_ref, None, list(keys))
        adv_flow = forward_overwritten_flow(flow_net, r_tgt, r_ref, maps)
    gt = flow_gt
    if mask is not None:
        bt, _, hg, wg = flow_gt.shape
        m = F.interpolate(mask[:, :1].to(flow_gt.dtype), size=(hg, wg), mode="bilinear", align_corners=False)
        patch_flow = torch.cat((torch.zeros(bt, 2, hg, wg), torch.ones(bt, 1, hg, wg)), 1).to(flow_gt)[:, :flow_gt.shape[1]]
        gt = (1 - m) * flow_gt + m * patch_flow
    return dict(flow=flow, adv_flow=adv_flow, epe=compute_epe(gt, flow), adv_epe=compute_epe(gt, adv_flow),
                cos_sim=compute_cossim(gt, flow), adv_cos_sim=compute_cossim(gt, adv_flow))


def forward_overwritten_flow(net, x1, x2, overwrite):
    """The flow alone of a forward with `overwrite`, whatever `net.return_feat_maps` says."""
    ow = _batched(overwrite, x1.shape[0], x1.device)
    if native_ok(net, x1):
        return _native_forward(net, x1, x2, ow)[0]
    with torch.no_grad():
        return net.forward_torch_maps(x1, x2, ow)[0]
