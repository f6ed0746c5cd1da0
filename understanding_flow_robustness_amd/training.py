"""The rest of the fine-tuning step, after the convolutions: the reference's two training losses, its optimiser and the body of
its inner training iteration (training/utils.py:68-239, training/train.py:225-282), under the reference's names.

  sequence_loss, multiscale_epe   value and gradient of every prediction in ONE pass over all scales (csrc/train_loss.hip) for HIP
                                  float32 tensors of the `flowNetC or pwc` branch whose ground-truth sides are integer multiples of
                                  every prediction's; everything else (CPU, float64, other ratios, the RAFT branch on a list)
                                  runs the plain-torch restatement below, which is also the yardstick of the GPU tests.  RAFT's
                                  branch on a `flownets.raft.RaftPredictions` (the low-resolution flows and masks): convex
                                  upsampling, loss and every gradient in ONE pass (csrc/raft_train_loss.hip).
  ClippedAdamW                    torch.optim.AdamW whose step() is a fused multi-tensor kernel with the gradient clipping of
                                  `clip_grad_norm_` folded in (csrc/optim.hip); state and param_groups are torch's own.
  fetch_optimizer                 that optimiser + torch's OneCycleLR, as the reference configures them.
  finetune_step                   zero_grad, forward, loss, backward, clip, AdamW, scheduler.

Importing this module needs no GPU; the kernels are loaded on first use."""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F

from . import _lib as L

MAX_FLOW = 400
FLOWNETC_WEIGHTS = (0.005, 0.01, 0.02, 0.08, 0.32)
_EPE_EPS = 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# the losses: plain torch (the reference's semantics, NaN quirks included, in every dtype and on every device)
def _valid_mask(flow_gt, valid, max_flow, not_excluding):
    if not_excluding:
        return valid >= 0.5
    return (valid >= 0.5) & (flow_gt.pow(2).sum(dim=1).sqrt() < max_flow)


def _area_gt(flow_gt, pred, scaled=True):
    """The ground truth on a prediction's grid: area interpolation, then (scaled) u times w/W and v times h/H."""
    h, w = pred.shape[-2:]
    gt = F.interpolate(flow_gt, (h, w), mode="area")
    if scaled:
        gt = gt * gt.new_tensor([w / flow_gt.shape[3], h / flow_gt.shape[2]]).view(1, 2, 1, 1)
    return gt


def _mean_without_nan(t):
    return t[~torch.isnan(t)].mean()


def _scale_weight(i, n, gamma, later_is_heavier, flownetc_weighing):
    if flownetc_weighing:
        return FLOWNETC_WEIGHTS[i]
    return gamma ** (n - i - 1) if later_is_heavier else gamma ** i


def _px_metrics(epe):
    return {"epe": epe.mean().item(), "1px": (epe < 1).float().mean().item(), "3px": (epe < 3).float().mean().item(),
            "5px": (epe < 5).float().mean().item()}


def _sequence_loss_torch(flow_preds, flow_gt, valid, gamma, max_flow, flowNetC, pwc, not_excluding, div_flow, flownetc_weighing):
    n = len(flow_preds)
    if div_flow > 1:
        flow_gt = flow_gt / div_flow
    pyramid = flowNetC or pwc
    if pyramid:
        epe = (flow_preds[0] - _area_gt(flow_gt, flow_preds[0])).pow(2).sum(dim=1).sqrt().view(-1)        # no NaN filter here
    else:
        mask = _valid_mask(flow_gt, valid, max_flow, not_excluding)
        epe = (flow_preds[-1] - flow_gt).pow(2).sum(dim=1).sqrt().view(-1)[mask.view(-1)]
    loss = 0.0
    for i, pred in enumerate(flow_preds):
        if pyramid:
            # gamma**i only with flowNetC: PWC-Net alone gets RAFT's ordering (the reference differs between the two)
            weight = _scale_weight(i, n, gamma, not flowNetC, flownetc_weighing)
            loss = loss + weight * _mean_without_nan((pred - _area_gt(flow_gt, pred)).abs())
        else:
            loss = loss + _scale_weight(i, n, gamma, True, False) * (mask[:, None] * (pred - flow_gt).abs()).mean()
    return loss, _px_metrics(epe)


def _multiscale_epe_torch(flow_preds, flow_gt, valid, gamma, max_flow, flowNetC, not_excluding, div_flow, flownetc_weighing, pwc):
    n = len(flow_preds)
    if div_flow > 1:
        flow_gt = flow_gt / div_flow
    pyramid = flowNetC or pwc
    if pyramid:
        epe = (flow_preds[0] - _area_gt(flow_gt, flow_preds[0], scaled=False)).pow(2).sum(dim=1).sqrt().view(-1)
        epe = epe[~torch.isnan(epe)]
    else:
        mask = _valid_mask(flow_gt, valid, max_flow, not_excluding)
        epe = (flow_preds[-1] - flow_gt).pow(2).sum(dim=1).sqrt().view(-1)[mask.view(-1)]
    loss = flow_preds[0].new_zeros(())          # the reference starts from a Python float and cannot report a step without a term
    for i, pred in enumerate(flow_preds):
        if pyramid:
            epe_map = ((pred - _area_gt(flow_gt, pred)).pow(2).sum(dim=1) + _EPE_EPS).sqrt()
            kept = epe_map[~torch.isnan(epe_map)]
            if not kept.numel():
                continue
            loss = loss + _scale_weight(i, n, gamma, False, flownetc_weighing) * kept.mean()
        else:
            loss = loss + _scale_weight(i, n, gamma, True, False) * (mask[:, None] * (pred - flow_gt).abs()).mean()
    metrics = _px_metrics(epe)
    metrics["loss"] = loss.float().mean().item()
    return loss, metrics


# ---------------------------------------------------------------------------------------------------------------------
# the losses: the kernel path
def _kernel_serves(flow_preds, flow_gt) -> bool:
    if not (isinstance(flow_gt, torch.Tensor) and flow_gt.is_cuda and flow_gt.dtype == torch.float32 and flow_gt.dim() == 4
            and flow_gt.shape[1] == 2 and 1 <= len(flow_preds) <= L.UFR_TRAIN_LOSS_MAX_SCALES):
        return False
    B, _, H, W = flow_gt.shape
    for p in flow_preds:
        if not (p.is_cuda and p.device == flow_gt.device and p.dtype == torch.float32 and p.dim() == 4 and p.shape[0] == B
                and p.shape[1] == 2 and p.shape[2] > 0 and p.shape[3] > 0 and H % p.shape[2] == 0 and W % p.shape[3] == 0):
            return False
    return B > 0


class _TrainLoss(torch.autograd.Function):
    """Forward computes the value, the metric sums and the gradient of every prediction; backward scales the gradients."""

    @staticmethod
    def forward(ctx, flow_gt, kind, weights, div_flow, *preds):
        lib = L.lib()
        preds = [p.contiguous() for p in preds]
        gt = flow_gt.contiguous()
        B, _, H, W = gt.shape
        n = len(preds)
        grads = [torch.empty_like(p) for p in preds]
        d = L.TrainLossDesc()
        d.gt, d.B, d.H, d.W, d.nscale, d.kind, d.div_flow = gt.data_ptr(), B, H, W, n, kind, float(div_flow)
        for i, (p, g) in enumerate(zip(preds, grads)):
            d.pred[i], d.grad[i], d.h[i], d.w[i], d.weight[i] = p.data_ptr(), g.data_ptr(), p.shape[2], p.shape[3], float(weights[i])
        need = lib.ufr_train_loss_workspace_doubles(B, n, d.h, d.w)
        ws = torch.empty(need, dtype=torch.float64, device=gt.device)
        out = torch.empty(8, dtype=torch.float64, device=gt.device)
        d.ws, d.ws_elems, d.out = ws.data_ptr(), need, out.data_ptr()
        with torch.cuda.device(gt.device):
            L.check(lib.ufr_train_loss(C.byref(d), L.stream()), "ufr_train_loss")
        ctx.grads = grads
        ctx.mark_non_differentiable(out)
        return out[0].to(torch.float32), out

    @staticmethod
    def backward(ctx, grad_loss, _grad_out):
        return (None, None, None, None) + tuple(g * grad_loss for g in ctx.grads)


def _loss_kernel(kind, flow_preds, flow_gt, weights, div_flow):
    loss, out = _TrainLoss.apply(flow_gt, kind, weights, div_flow, *flow_preds)
    value, epe_sum, epe_n, n1, n3, n5, _, _ = out.cpu().tolist()                  # the one device-to-host copy of the call
    nan = float("nan")
    metrics = {"epe": epe_sum / epe_n if epe_n else nan, "1px": n1 / epe_n if epe_n else nan, "3px": n3 / epe_n if epe_n else nan,
               "5px": n5 / epe_n if epe_n else nan}
    if kind == 1:
        metrics["loss"] = value
    loss._ufr_host_value = value            # finetune_step's NaN test reads this instead of asking the device again
    return loss, metrics


# ---------------------------------------------------------------------------------------------------------------------
# the losses: RAFT's branch from the low-resolution predictions (flownets.raft.RaftPredictions), convex upsampling included
def _is_raft_predictions(flow_preds) -> bool:
    from .flownets.raft import RaftPredictions
    return isinstance(flow_preds, RaftPredictions)


def _raft_kernel_serves(preds, flow_gt, valid) -> bool:
    """Everything HIP float32 and contiguous on one device, gt [B,2,8H,8W], valid [B,8H,8W], 1 .. 32 pairs of [B,2,H,W] / [B,576,H,W]."""
    def dense(t, shape):
        return (isinstance(t, torch.Tensor) and t.is_cuda and t.device == flow_gt.device and t.dtype == torch.float32
                and tuple(t.shape) == shape and t.is_contiguous())
    n = len(preds)
    if not (1 <= n <= L.UFR_RAFT_LOSS_MAX_PREDS and isinstance(flow_gt, torch.Tensor) and flow_gt.dim() == 4
            and isinstance(preds.flows[0], torch.Tensor) and preds.flows[0].dim() == 4):
        return False
    B, _, H, W = preds.flows[0].shape
    if not (B > 0 and H > 0 and W > 0 and dense(flow_gt, (B, 2, 8 * H, 8 * W)) and dense(valid, (B, 8 * H, 8 * W))):
        return False
    return all(dense(f, (B, 2, H, W)) and dense(m, (B, 576, H, W)) for f, m in zip(preds.flows, preds.masks))


class _RaftTrainLoss(torch.autograd.Function):
    """Forward computes the value, the metric sums and the gradient of every flow and mask (csrc/raft_train_loss.hip); backward scales
    the gradients, in place: they are the size of the masks, and like autograd's saved tensors they are gone after one backward."""

    @staticmethod
    def forward(ctx, flow_gt, valid, weights, div_flow, max_flow, exclude_large, *tensors):
        lib = L.lib()
        n = len(tensors) // 2
        flows, masks = tensors[:n], tensors[n:]
        B, _, H, W = flows[0].shape
        grads = [torch.empty_like(t) for t in tensors]
        d = L.RaftSequenceLossDesc()
        d.gt, d.valid, d.B, d.H, d.W, d.npred = flow_gt.data_ptr(), valid.data_ptr(), B, H, W, n
        for i in range(n):
            d.flow[i], d.mask[i], d.grad_flow[i], d.grad_mask[i] = (flows[i].data_ptr(), masks[i].data_ptr(), grads[i].data_ptr(),
                                                                    grads[n + i].data_ptr())
            d.weight[i] = float(weights[i])
        d.div_flow, d.max_flow, d.exclude_large = float(div_flow), float(max_flow), int(bool(exclude_large))
        need = lib.ufr_raft_sequence_loss_workspace_doubles(B, H, W, n)
        ws = torch.empty(need, dtype=torch.float64, device=flow_gt.device)
        out = torch.empty(8, dtype=torch.float64, device=flow_gt.device)
        d.ws, d.ws_elems, d.out = ws.data_ptr(), need, out.data_ptr()
        with torch.cuda.device(flow_gt.device):
            L.check(lib.ufr_raft_sequence_loss(C.byref(d), L.stream()), "ufr_raft_sequence_loss")
        ctx.grads = grads
        ctx.mark_non_differentiable(out)
        return out[0].to(torch.float32), out

    @staticmethod
    def backward(ctx, grad_loss, _grad_out):
        grads, ctx.grads = ctx.grads, None
        if grads is None:
            raise RuntimeError("the fused RAFT loss keeps its gradients for one backward only (they are scaled in place)")
        torch._foreach_mul_(grads, grad_loss)
        return (None, None, None, None, None, None) + tuple(grads)


def _raft_loss_kernel(kind, preds, flow_gt, valid, gamma, max_flow, not_excluding, div_flow):
    n = len(preds)
    weights = [_scale_weight(i, n, gamma, True, False) for i in range(n)]
    loss, out = _RaftTrainLoss.apply(flow_gt, valid, weights, div_flow, max_flow, not not_excluding, *preds.flows, *preds.masks)
    value, epe_sum, epe_n, n1, n3, n5, _, _ = out.cpu().tolist()                  # the one device-to-host copy of the call
    nan = float("nan")
    metrics = {"epe": epe_sum / epe_n if epe_n else nan, "1px": n1 / epe_n if epe_n else nan, "3px": n3 / epe_n if epe_n else nan,
               "5px": n5 / epe_n if epe_n else nan}
    if kind == 1:
        metrics["loss"] = value
    loss._ufr_host_value = value            # finetune_step's NaN test reads this instead of asking the device again
    return loss, metrics


def sequence_loss(flow_preds, flow_gt, valid, gamma=0.8, max_flow=MAX_FLOW, flowNetC=False, pwc=False, not_excluding=False,
                  div_flow=1, flownetc_weighing=False):
    """The reference's `sequence_loss` (training/utils.py:148-222): (loss, metrics).  With `flowNetC or pwc`: per scale the L1
    distance to the area-interpolated, rescaled ground truth, averaged over the elements that are not NaN.  A RaftPredictions in
    place of the list: RAFT's branch with the upsampling folded in, where `_raft_kernel_serves`; its `upsampled()` list elsewhere."""
    if _is_raft_predictions(flow_preds):
        if not (flowNetC or pwc) and _raft_kernel_serves(flow_preds, flow_gt, valid):
            return _raft_loss_kernel(0, flow_preds, flow_gt, valid, gamma, max_flow, not_excluding, div_flow)
        flow_preds = flow_preds.upsampled()
    flow_preds = list(flow_preds)
    if (flowNetC or pwc) and _kernel_serves(flow_preds, flow_gt):
        n = len(flow_preds)
        weights = [_scale_weight(i, n, gamma, not flowNetC, flownetc_weighing) for i in range(n)]
        return _loss_kernel(0, flow_preds, flow_gt, weights, div_flow)
    return _sequence_loss_torch(flow_preds, flow_gt, valid, gamma, max_flow, flowNetC, pwc, not_excluding, div_flow, flownetc_weighing)


def multiscale_epe(flow_preds, flow_gt, valid, gamma=0.8, max_flow=MAX_FLOW, flowNetC=False, not_excluding=False, div_flow=1,
                   flownetc_weighing=False, pwc=False):
    """The reference's `multiscale_epe` (training/utils.py:68-145): (loss, metrics).  With `flowNetC or pwc`: per scale the
    end-point error (+ 1e-5 under the root) to the area-interpolated, rescaled ground truth, averaged over the pixels that are not
    NaN; a scale without such a pixel is skipped.  A RaftPredictions in place of the list: as in `sequence_loss`."""
    if _is_raft_predictions(flow_preds):
        if not (flowNetC or pwc) and _raft_kernel_serves(flow_preds, flow_gt, valid):
            return _raft_loss_kernel(1, flow_preds, flow_gt, valid, gamma, max_flow, not_excluding, div_flow)
        flow_preds = flow_preds.upsampled()
    flow_preds = list(flow_preds)
    if (flowNetC or pwc) and _kernel_serves(flow_preds, flow_gt):
        n = len(flow_preds)
        weights = [_scale_weight(i, n, gamma, False, flownetc_weighing) for i in range(n)]
        return _loss_kernel(1, flow_preds, flow_gt, weights, div_flow)
    return _multiscale_epe_torch(flow_preds, flow_gt, valid, gamma, max_flow, flowNetC, not_excluding, div_flow, flownetc_weighing, pwc)


# ---------------------------------------------------------------------------------------------------------------------
# the optimiser
class ClippedAdamW(torch.optim.AdamW):
    """torch.optim.AdamW (constructor, param_groups, per-parameter state `step` / `exp_avg` / `exp_avg_sq`: state dicts interchange
    with torch's) whose `step(clip=...)` runs `clip_grad_norm_` and the update as fused multi-tensor kernels on HIP float32
    parameters with dense gradients.  `self.grad_norm`: the last total gradient norm, a device tensor (None before the first
    clipped step).  Nothing else is served and nothing falls back: `amsgrad`, `maximize`, `capturable`, `differentiable`, `fused`,
    sparse gradients and other dtypes or devices raise NotImplementedError."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None):
        for name, on in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable), ("differentiable", differentiable),
                         ("fused", fused)):
            if on:
                raise NotImplementedError(f"ClippedAdamW: {name}=True is not implemented (use torch.optim.AdamW)")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                         foreach=foreach, capturable=False, differentiable=False, fused=None)
        self.grad_norm = None
        self._norm = None
        self._partials = None

    def _segments(self, group):
        """(rows of ufr_adamw_seg, their number, the tensors they point into) of the group's parameters that have a gradient."""
        for name in ("amsgrad", "maximize", "capturable", "differentiable", "fused"):      # a loaded state dict can switch them on
            if group.get(name):
                raise NotImplementedError(f"ClippedAdamW: {name}=True is not implemented (use torch.optim.AdamW)")
        rows, keep = [], []
        for p in group["params"]:
            if p.grad is None:
                continue
            g = p.grad
            if g.is_sparse:
                raise NotImplementedError("ClippedAdamW: sparse gradients are not implemented")
            if not (p.is_cuda and p.dtype == torch.float32 and g.dtype == torch.float32 and g.device == p.device):
                raise NotImplementedError(f"ClippedAdamW: a {p.dtype} parameter on {p.device} (HIP float32 parameters only)")
            if not p.is_contiguous():
                raise NotImplementedError("ClippedAdamW: a parameter that is not contiguous")
            g = g.contiguous()
            state = self.state[p]
            if len(state) == 0:                                   # torch's own initial state (Adam._init_group)
                state["step"] = torch.tensor(0.0, dtype=torch.get_default_dtype())
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            m, v = state["exp_avg"], state["exp_avg_sq"]
            if not (m.is_contiguous() and v.is_contiguous() and m.dtype == v.dtype == torch.float32 and m.device == v.device == p.device):
                raise NotImplementedError("ClippedAdamW: optimizer state that is not contiguous HIP float32")
            rows.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()))
            keep.append((p, g, state["step"]))
        return rows, len(rows), keep

    @torch.no_grad()
    def step(self, closure=None, *, clip=None):
        """One AdamW update; with `clip`, the gradients count as scaled by min(1, clip / (their total L2 norm + 1e-6)) without
        being rewritten, and the norm is left in `self.grad_norm`."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        plans = [self._segments(group) for group in self.param_groups]
        device = next((keep[0][0].device for _, n, keep in plans if n), None)
        if device is None:
            return loss
        lib = L.lib()
        norm_ptr = None
        with torch.cuda.device(device):
            if clip is not None:
                if any(k[0].device != device for _, _, keep in plans for k in keep):
                    raise NotImplementedError("ClippedAdamW: parameters on more than one device")
                rows = [r for group_rows, _, _ in plans for r in group_rows]
                every = (L.AdamwSeg * len(rows))(*rows)
                need = lib.ufr_grad_norm_partials(every, len(rows))
                if self._partials is None or self._partials.numel() < need or self._partials.device != device:
                    self._partials = torch.empty(max(need, 1), dtype=torch.float64, device=device)
                self._norm = torch.empty(2, dtype=torch.float32, device=device)
                L.check(lib.ufr_grad_norm(every, len(rows), float(clip), self._partials.data_ptr(), self._partials.numel(),
                                          self._norm.data_ptr(), L.stream()), "ufr_grad_norm")
                self.grad_norm = self._norm[0]
                norm_ptr = self._norm.data_ptr()
            for group, (rows, n, keep) in zip(self.param_groups, plans):
                if not n:
                    continue
                counters = [k[2] for k in keep]                  # torch's per-parameter `step` tensors (on the host)
                torch._foreach_add_(counters, 1)
                steps = set(torch.stack(counters).tolist())
                if len(steps) != 1:
                    raise NotImplementedError("ClippedAdamW: parameters of one group at different step counts")
                t = steps.pop()
                segs = (L.AdamwSeg * n)(*rows)
                beta1, beta2 = (float(b) for b in group["betas"])
                h = L.AdamwHyper(float(group["lr"]), beta1, beta2, float(group["eps"]), float(group["weight_decay"]),
                                 1.0 - beta1 ** t, 1.0 - beta2 ** t)
                L.check(lib.ufr_adamw_step(segs, n, C.byref(h), norm_ptr, L.stream()), "ufr_adamw_step")
        return loss


def fetch_optimizer(args, model, inner_iteration: int = 1):
    """The reference's optimiser and schedule (training/utils.py:225-239): AdamW and a linear one-cycle learning rate."""
    optimizer = ClippedAdamW(model.parameters(), lr=args.lr, weight_decay=args.wdecay, eps=args.epsilon)
    scheduler = torch.optim.lr_scheduler.OneCycleLR(optimizer, args.lr, args.num_steps * inner_iteration + 100, pct_start=0.05,
                                                    cycle_momentum=False, anneal_strategy="linear")
    return optimizer, scheduler


# ---------------------------------------------------------------------------------------------------------------------
def _flag(args, name, default=False):
    return getattr(args, name, default)


def _fused_raft(model, image1, image2) -> bool:
    from .flownets.raft import RAFT
    return isinstance(model, RAFT) and all(t.is_cuda and t.dtype == torch.float32 for t in (image1, image2))


def finetune_step(model, optimizer, scheduler, image1, image2, flow, valid, args, fused_raft_loss=True):
    """One inner training iteration of the reference (training/train.py:225-282) without its GradScaler: zero_grad, forward,
    loss, backward, clipped AdamW step, scheduler step; (loss, metrics).  A NaN loss returns before the backward, as there.
    `band_conv.native_training()` is the caller's choice: inside it the FlowNetC family and PWC-Net run their convolutions on the
    hand-written kernels, outside it (and for RAFT) on torch operators; the loss and the optimiser are the ones above either way.
    `optimizer` is a ClippedAdamW (`fetch_optimizer`); any other torch optimiser gets `clip_grad_norm_` and its own step().
    `fused_raft_loss`: this package's RAFT on HIP float32 frames hands the loss its low-resolution predictions, and upsampling,
    loss and their gradients run as one pass (csrc/raft_train_loss.hip); False: the list of upsampled predictions, as before."""
    flownetc = bool(_flag(args, "flowNetC") or _flag(args, "flowNetCFlexible"))
    pwc = bool(_flag(args, "pwc"))
    optimizer.zero_grad()
    raft_kw = {"lowres_predictions": True} if fused_raft_loss and not (flownetc or pwc) and _fused_raft(model, image1, image2) else {}
    if _flag(args, "adv_train") or _flag(args, "finetune"):
        if flownetc or pwc:
            flow_predictions = model(image1, image2)
        else:                                                       # RAFT
            flow_predictions = model(image1 * 255.0, image2 * 255.0, iters=_flag(args, "iters", 12), **raft_kw)
    else:
        if flownetc:
            flow_predictions = model(image1 / 255.0, image2 / 255.0)
        else:                                                       # RAFT (and, as in the reference, PWC-Net)
            flow_predictions = model(image1, image2) if pwc else model(image1, image2, iters=_flag(args, "iters", 12), **raft_kw)
    loss_fn = multiscale_epe if _flag(args, "multiscaleEPE") else sequence_loss
    loss, metrics = loss_fn(flow_predictions, flow, valid, _flag(args, "gamma", 0.8), flowNetC=flownetc,
                            not_excluding=_flag(args, "no_excluding"), div_flow=_flag(args, "div_flow", 1),
                            flownetc_weighing=_flag(args, "flownetc_weighing"), pwc=pwc)
    value = getattr(loss, "_ufr_host_value", None)
    if value is None:
        value = float(loss)
    if value != value:
        return loss, metrics
    if loss.requires_grad:
        loss.backward()
    clip = _flag(args, "clip", None)
    if isinstance(optimizer, ClippedAdamW):
        optimizer.step(clip=clip)
    else:
        if clip is not None:
            torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
        optimizer.step()
    scheduler.step()
    return loss, metrics
