"""Universal-perturbation / I-FGSM inner loop (global_attacks/universal_perturbation.py:452-530,
:667-675; loss from global_attacks/perturb_model.py:102-145) as a fused, graph-captured step.

Reference step (x n_step, default 10):  re-leaf both frames -> predict_flow -> compute_flow_loss ->
backward(retain_graph=True, weights included) -> sign -> lr*sign -> adv -/+ -> clamp[0,1] ->
noise = clamp(adv - img, +-output_norm) -> adv = img + noise.
Here: forward -> ufr_flow_loss_ex (loss + d loss/d flow) -> data-gradient backward ->
ufr_universal_update (everything after the backward, both frames, one kernel); one HIP graph per step.

Batch semantics: with B = 1 and no exchange the arithmetic is the reference's, sample by sample
(`shared=False`, delta [B,2,3,H,W]).  `shared=True` is the build's extension for a sharded batch
(BASELINE config 5): ONE perturbation [2,3,H,W]; the step direction is the sign of the gradient
SUMMED over all samples of all ranks (all-reduced before the sign), so every rank applies the
identical update.  For B = 1 its adversarial frames equal the reference's wherever the [0,1]
image-range clamp does not bind (clamping to [0,1] then to img+-eps is clamping to the
intersection); where it binds, the reference folds the clamp into its per-sample noise while the
shared delta stays image-independent (tests/test_models_cpu.py pins both statements).

Per-sample steps take two keyword-only options for `perturb_model.PerturbationsModel` (csrc/perturb_step.hip):
`momentum=mu` replaces ufr_universal_update by ufr_abs_sums + ufr_momentum_update (MI-FGSM, perturb_model.py:621-757),
`diverse=True` puts ufr_diverse_forward in front of the network and ufr_diverse_backward behind its data gradient (input
diversity, :759-821), the transform of each step read from a device table through a device-resident step index.
"""
from __future__ import annotations

from argparse import Namespace

import numpy as np
import torch
from ._lib import engine_cache as _engine_cache

from . import _lib as L
from .flownets.utils_model import predict_flow
from .patch_attack import ShardedExchange

_KINDS = {"cossim": 0, "l2": 1, "l1": 2}
_FRAMES = {"both": 3, "left": 1, "right": 2}


def add_universal_perturbation(image0, image1, universal_perturbation, lower_bound=0.0, upper_bound=1.0):
    """universal_perturbation.py:667-675, including its asymmetric indexing ([0,0] vs [:,1])."""
    if universal_perturbation.shape[1] != 2:
        raise Exception("Universarial perturbation: first dimension must be 2!")
    return (torch.clamp(image0 + universal_perturbation[0, 0], lower_bound, upper_bound),
            torch.clamp(image1 + universal_perturbation[:, 1], lower_bound, upper_bound))


class UniversalPerturbationStep:
    MAX_ROWS = 1024                     # rows of the device table of input-diversity transforms (steps of one run)

    def __init__(self, model, args, batch, height, width, gt_channels=2, device="cuda:0", shared=False,
                 exchange: ShardedExchange | None = None, use_graph=True, warmup=2, *, momentum=None, diverse=False):
        """`momentum` = mu turns the step into MI-FGSM's (perturb_model.py:621-757: an L1-normalised running gradient, the step
        along its sign); `diverse` puts the input-diversity transform (:759-821) in front of the network, its parameters read per
        step from a device table that `run` uploads (csrc/perturb_step.hip).  Without them the step is what it always was."""
        L.lib()
        if (momentum is not None or diverse) and (shared or exchange is not None):
            raise NotImplementedError("momentum and input diversity exist for per-sample perturbations only, not for the shared "
                                      "(multi-rank) perturbation")
        self.model, self.args = model, args
        self.B, self.H, self.W, self.Cg = batch, height, width, gt_channels
        self.dev = torch.device(device)
        self.shared = shared
        self.exchange = exchange
        self.world = exchange.world if exchange is not None else 1
        if self.world > 1 and not shared:
            raise ValueError("a sharded batch needs the shared perturbation")
        if args.flow_loss not in _KINDS:
            raise NotImplementedError(f"flow_loss {args.flow_loss!r}")
        method = args.perturb_method.lower()
        if "ifgsm" in method:
            self.use_sign = 1
        elif method == "ifgm":
            self.use_sign = 0
        else:
            raise NotImplementedError(method)
        self.kind = _KINDS[args.flow_loss]
        self.frames = _FRAMES[args.perturb_mode]
        self.lr, self.eps = float(args.learning_rate), float(args.output_norm)
        self.ascent = 1 if getattr(args, "add_gaussian", False) else 0
        self.CHW = 3 * height * width
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.img0 = torch.zeros(batch, 3, height, width, **f32)
        self.img1 = torch.zeros_like(self.img0)
        self.gt = torch.zeros(batch, gt_channels, height, width, **f32)
        self.adv0 = torch.zeros_like(self.img0).requires_grad_(True)
        self.adv1 = torch.zeros_like(self.img0).requires_grad_(True)
        self.g_flow = torch.zeros(batch, 2, height, width, **f32)
        self.delta = torch.zeros((2, 3, height, width) if shared else (batch, 2, 3, height, width), **f32)
        self.packed = torch.zeros(2 * self.CHW + 1, **f32)      # [grad sum frame 0 | frame 1 | loss]
        self.loss_cur = self.packed[2 * self.CHW:]
        self.scale_t = torch.ones(1, **f32)     # 1/normaliser of the loss, device-resident
        self.loss_ws = torch.zeros(L.LOSS_PARTIALS, **f32)     # workgroup partials of the fixed-order loss reduction
        self.mu, self.diverse = (None if momentum is None else float(momentum)), bool(diverse)
        if self.mu is not None:
            self.m0, self.m1 = torch.zeros_like(self.img0), torch.zeros_like(self.img0)
            self.abs_sums = torch.zeros(2, **f32)
            n = batch * self.CHW
            self.abs_ws = torch.zeros(L.lib().ufr_abs_sums_workspace_doubles(n), dtype=torch.float64, device=self.dev)
        if self.diverse:
            self.x0 = torch.zeros_like(self.img0).requires_grad_(True)      # what the network reads: leaves written in place
            self.x1 = torch.zeros_like(self.img0).requires_grad_(True)
            self.gt_d = torch.zeros_like(self.gt)
            self.gd0, self.gd1 = torch.zeros_like(self.img0), torch.zeros_like(self.img0)
            self.table = torch.zeros(self.MAX_ROWS, L.DIVERSE_COLS, dtype=torch.int32, device=self.dev)
            self.step_index = torch.zeros(1, dtype=torch.int32, device=self.dev)
            ws = L.lib().ufr_diverse_workspace_doubles(batch, height, width, gt_channels)
            if ws < 0:
                raise ValueError(f"input diversity: bad shape {batch} x {height} x {width}, {gt_channels} ground-truth channels")
            self.diverse_ws = torch.zeros(max(ws, 1), dtype=torch.float64, device=self.dev)
        L.freeze_parameters(self.model)                         # patch_attack.release() restores the caller's flags
        self.model.eval()
        self.graph = self.graph_b = None
        self.use_graph, self._warmup, self._captured = use_graph, warmup, False

    def _update(self, g0, g1, mode):
        L.check(L.lib().ufr_universal_update(
            L.ptr(self.img0), L.ptr(self.img1), L.ptr(g0) if g0 is not None else None,
            L.ptr(g1) if g1 is not None else None, L.ptr(self.packed), L.ptr(self.adv0), L.ptr(self.adv1),
            L.ptr(self.delta), self.B, self.CHW, self.lr, self.eps, 0.0, 1.0, self.use_sign, self.frames,
            self.ascent, int(self.shared), mode, L.stream()), "universal update")

    def _momentum_update(self, g0, g1):
        """:673-710: sum|g| of each frame over the whole batch, then momentum and update in one launch."""
        lib = L.lib()
        L.check(lib.ufr_abs_sums(L.ptr(g0), L.ptr(g1), self.B * self.CHW, L.ptr(self.abs_ws), self.abs_ws.numel(),
                                 L.ptr(self.abs_sums), L.stream()), "abs sums")
        L.check(lib.ufr_momentum_update(L.ptr(self.img0), L.ptr(self.img1), L.ptr(g0), L.ptr(g1), L.ptr(self.abs_sums),
                                        L.ptr(self.m0), L.ptr(self.m1), L.ptr(self.adv0), L.ptr(self.adv1), L.ptr(self.delta),
                                        self.B, self.CHW, self.mu, 1.0 - self.mu, self.lr, self.eps, 0.0, 1.0, self.frames,
                                        self.ascent, L.stream()), "momentum update")

    def _part_a(self):
        self.loss_cur.zero_()
        in0, in1, gt = self.adv0, self.adv1, self.gt
        if self.diverse:          # the step's row of the table: frames and ground truth resized and padded, scale_t with a mask
            in0, in1, gt = self.x0, self.x1, self.gt_d
            L.check(L.lib().ufr_diverse_forward(L.ptr(self.adv0), L.ptr(self.adv1), L.ptr(self.gt), L.ptr(in0), L.ptr(in1),
                                                L.ptr(gt), self.B, self.H, self.W, self.Cg, L.ptr(self.table), self.MAX_ROWS,
                                                L.ptr(self.step_index), L.ptr(self.scale_t), L.ptr(self.diverse_ws),
                                                self.diverse_ws.numel(), L.stream()), "diverse forward")
        flow = predict_flow(self.model, None, in0, in1, self.args).contiguous()
        L.check(L.lib().ufr_flow_loss_ex(L.ptr(flow), L.ptr(gt), L.ptr(self.g_flow), L.ptr(self.loss_cur), self.B,
                                         self.H * self.W, self.Cg, self.kind, 0.0, L.ptr(self.scale_t), L.ptr(self.loss_ws),
                                         L.stream()), "flow loss")
        g0, g1 = torch.autograd.grad(flow, (in0, in1), self.g_flow, allow_unused=True)
        g0 = torch.zeros_like(self.img0) if g0 is None else g0.contiguous()
        g1 = torch.zeros_like(self.img1) if g1 is None else g1.contiguous()   # :479-483
        if self.diverse:          # back through the resize to the adversarial frames
            L.check(L.lib().ufr_diverse_backward(L.ptr(g0), L.ptr(g1), L.ptr(self.gd0), L.ptr(self.gd1), self.B, self.H, self.W,
                                                 L.ptr(self.table), self.MAX_ROWS, L.ptr(self.step_index), L.stream()),
                    "diverse backward")
            g0, g1 = self.gd0, self.gd1
        if self.mu is not None:
            self._momentum_update(g0, g1)
        else:
            self._update(g0, g1, 1 if self.world > 1 else 0)
        if self.diverse:
            L.check(L.lib().ufr_step_advance(L.ptr(self.step_index), L.stream()), "step advance")

    def _iteration(self):
        if self.graph is not None:
            self.graph.replay()
        else:
            self._part_a()
        if self.world > 1:
            self.exchange(self.packed)
            if self.graph_b is not None:
                self.graph_b.replay()
            else:
                self._update(None, None, 2)

    def _capture(self):
        side = torch.cuda.Stream(device=self.dev)
        side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side):
            for _ in range(max(self._warmup, 1)):
                self._iteration()
        torch.cuda.current_stream(self.dev).wait_stream(side)
        torch.cuda.synchronize(self.dev)
        if self.use_graph:
            graph = torch.cuda.CUDAGraph()
            with L.graph_capture(graph):
                self._part_a()
            graph_b = None
            if self.world > 1:
                graph_b = torch.cuda.CUDAGraph()
                with L.graph_capture(graph_b):
                    self._update(None, None, 2)
            self.graph, self.graph_b = graph, graph_b
        self._captured = True

    def load(self, img0, img1, universal_perturbation, target):
        """Operands of one attack() call + the initial add_universal_perturbation (:461-463)."""
        with torch.no_grad():
            self.img0.copy_(img0); self.img1.copy_(img1); self.gt.copy_(target)
            if self.shared:
                self.delta.copy_(universal_perturbation.reshape(-1, 2, 3, self.H, self.W)[0])
                a0 = torch.clamp(self.img0 + self.delta[0], 0.0, 1.0)
                a1 = torch.clamp(self.img1 + self.delta[1], 0.0, 1.0)
            else:
                a0, a1 = add_universal_perturbation(self.img0, self.img1, universal_perturbation)
            self.adv0.copy_(a0); self.adv1.copy_(a1)
            if self.Cg == 3:      # 1 / (sum(valid) + eps), perturb_model.py:141-143, computed on the device
                valid = self.gt[:, 2].sum().reshape(1)
                if self.world > 1:
                    self.exchange.dist.all_reduce(valid)
                self.scale_t.copy_(1.0 / (valid + 1e-8))
            else:
                per_pix = 2 if self.kind == 2 else 1
                self.scale_t.fill_(1.0 / (self.B * self.world * self.H * self.W * per_pix))
            if self.mu is not None:
                self.m0.zero_(); self.m1.zero_()
            if self.diverse:
                self.step_index.zero_()

    def _upload_table(self, n_step, table):
        """The transforms of the next `n_step` steps: host int32 [n_step, 8] rows (apply, nh, nw, top, left, 0, 0, 0), checked on
        the host (csrc/perturb_step.hip refuses a row that leaves the frame), uploaded once; the step index restarts at row 0."""
        if table is None:
            raise ValueError("a step with input diversity needs the table of its transforms: run(n_step, table)")
        table = torch.as_tensor(table, dtype=torch.int32).contiguous()
        if table.is_cuda or tuple(table.shape) != (int(n_step), L.DIVERSE_COLS):
            raise ValueError(f"the table of transforms is a host tensor of exactly [{int(n_step)}, {L.DIVERSE_COLS}] for "
                             f"{int(n_step)} steps, got {tuple(table.shape)} on {table.device}")
        if int(n_step) > self.MAX_ROWS:
            raise ValueError(f"{int(n_step)} steps with input diversity: the device table holds {self.MAX_ROWS} rows")
        if int(n_step) > 0:
            L.check(L.lib().ufr_diverse_table_check(table.data_ptr(), int(n_step), self.H, self.W), "diverse table")
        with torch.no_grad():
            self.table.zero_()
            self.table[:int(n_step)].copy_(table)
            self.step_index.zero_()

    def run(self, n_step, table=None):
        with torch.cuda.device(self.dev):
            if self.diverse:
                self._upload_table(n_step, table)
            elif table is not None:
                raise ValueError("this step was built without input diversity and takes no table")
            if not self._captured:
                state = [self.img0, self.img1, self.delta, self.gt, self.adv0, self.adv1, self.scale_t]
                if self.mu is not None:
                    state += [self.m0, self.m1]
                if self.diverse:
                    state += [self.step_index]
                saved = [x.detach().clone() for x in state]
                self._capture()
                with torch.no_grad():
                    for x, keep in zip(state, saved):
                        x.copy_(keep)
            for _ in range(int(n_step)):
                self._iteration()

    enqueue = run


_CACHE = "_ufr_universal_steps"


def attack(model, img0_var, img1_var, universal_perturbation_var, target_var, args: Namespace, use_graph=True):
    """Drop-in for global_attacks/universal_perturbation.py::attack (:452-530):
    returns (adv_img0, None, adv_img1, universal_perturbation [B,2,3,H,W])."""
    L.require_hip(img0_var, "img0_var", contiguous=False)
    B, _, H, W = img0_var.shape
    key = (B, H, W, target_var.shape[1], args.flow_loss, args.perturb_method, args.perturb_mode,
           float(args.learning_rate), float(args.output_norm), bool(getattr(args, "add_gaussian", False)),
           args.flownet, bool(use_graph))
    cache = _engine_cache(model, _CACHE)
    step = cache.get(key)
    if step is None:
        step = cache[key] = UniversalPerturbationStep(model, args, B, H, W, gt_channels=target_var.shape[1],
                                                      device=img0_var.device, shared=False, use_graph=use_graph)
    step.load(img0_var, img1_var, universal_perturbation_var, target_var)
    step.run(args.n_step)
    return step.adv0.detach().clone(), None, step.adv1.detach().clone(), step.delta.detach().clone()


def validation(universal_perturbation, val_loader, model, epoch, args: Namespace, chunk=4):
    """Drop-in for global_attacks/universal_perturbation.py::validation (:533-566, :664) without its writer and logger: the
    per-epoch check of a universal perturbation [1,2,3,H,W].  Per chunk of up to `chunk` consecutive 7-tuple items
    `(ref_past, tgt, ref_future, flow_gt, _, _, _)` of equal sizes: `add_universal_perturbation` as ONE ufr_global_apply (its
    asymmetric indexing kept: frame 0 takes `[0, 0]`, frame 1 `[:, 1]`), ONE forward of the 2K clean and perturbed pairs, ONE
    ufr_global_metrics (global_eval.py); the host reads once.  Returns `(errors_avg, ["epe", "adv_epe", "cos_sim", "adv_cos_sim"])`.
    `epoch` only labelled the reference's images."""
    from .chunked_eval import freeze
    from .global_eval import NAMES, Chunks
    error_names = ["epe", "adv_epe", "cos_sim", "adv_cos_sim"]
    if universal_perturbation.dim() != 5 or universal_perturbation.shape[1] != 2:
        raise Exception("Universarial perturbation: first dimension must be 2!")
    if universal_perturbation.shape[0] != 1:
        raise ValueError("validation takes ONE universal perturbation [1,2,3,H,W]: with more, `[:, 1]` gives the second frame another "
                         "batch size than the first")
    freeze(model)
    ev = Chunks(model, args, chunk, with_noise=False)
    noise = None
    for data in val_loader:
        _, tgt_img, ref_img_future, flow_gt = data[0], data[1], data[2], data[3]
        L.require_hip(tgt_img, "tgt_img", contiguous=False)
        if noise is None or noise[0].device != tgt_img.device:
            up = universal_perturbation.detach().to(tgt_img.device, torch.float32)
            noise = (up[0, 0][None].contiguous(), up[:, 1].contiguous())
        if tuple(noise[0].shape) != tuple(tgt_img.shape):
            raise ValueError(f"the universal perturbation is {tuple(noise[0].shape)}, the item is {tuple(tgt_img.shape)}")
        ev.add(tgt_img, ref_img_future, flow_gt, noise, None)
    per_item, _ = ev.read()
    cols = [NAMES.index(n) for n in ("epe_clean", "epe_adv", "cossim_clean", "cossim_adv")]
    avg = per_item[:, cols].mean(axis=0) if len(per_item) else np.zeros(4)
    return [float(v) for v in avg], error_names


def train(universal_perturbation, train_loader, model, args: Namespace):
    """Drop-in for global_attacks/universal_perturbation.py::train (:354-397) without its writer and logger: the sequential loop
    over `attack` that carries the perturbation from sample to sample.  Items are `(tgt, [ref_past, ref_future])` or
    `(tgt, ref, _, _)`; the target is minus the clean prediction, or with `add_gaussian` the clean prediction plus one host
    `torch.randn` draw of its shape.  Returns the carried perturbation [B,2,3,H,W]."""
    model.eval()
    for data in train_loader:
        if len(data) == 2:
            tgt_img, ref_img = data
        elif len(data) == 4:
            tgt_img, ref_img, _, _ = data
            ref_img = [ref_img, ref_img]
        else:
            raise NotImplementedError
        tgt_img, ref_past, ref_future = tgt_img.cuda(), ref_img[0].cuda(), ref_img[1].cuda()
        flow_pred = predict_flow(model, ref_past, tgt_img, ref_future, args)
        universal_perturbation = universal_perturbation.cuda()
        if not getattr(args, "add_gaussian", False):
            target = -1 * flow_pred.detach().clone()
        else:
            target = flow_pred.detach().clone()
            target = target + 1 * torch.randn(target.shape).cuda()
        _, _, _, universal_perturbation = attack(model, tgt_img, ref_future, universal_perturbation, target_var=target, args=args)
    return universal_perturbation
