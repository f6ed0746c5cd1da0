"""The evaluation of the global attacks (global_attacks/perturb_main.py:466-812, flow branch, and its final table,
global_attacks/log_utils.py:226-528 `validate`): per validation item a clean forward, the attack -- `perturb_model.PerturbationsModel`,
or a fixed perturbation (`--universal_evaluation`, `--arbitrary_noise_index`) -- an attacked forward, and per item the two noise
norms of both frames and the end-point error, L1 and cosine similarity of both predictions.

Reference, per item: two batch-1 forwards, five D2H copies (both noises, both flows, the ground truth), five `FloatTensor` uploads
inside `validate`, six metric calls that each resize the prediction and end in `.item()`, four numpy norms.  Here up to `chunk`
consecutive items of equal sizes are stacked, and per chunk

    the attacks, item by item (or ONE ufr_global_apply, csrc/global_eval.hip)  ->  ONE forward of the 2K clean and perturbed pairs
    ->  ONE ufr_global_metrics

run; the host reads the results once, at the end.  The attack itself stays at batch 1 and in loader order: MI-FGSM's L1 normalisation,
the loss's division by the valid count and the one input-diversity draw per step all couple the items of a batch, so a batched
attack would not be the reference's, and `torch`, `random` and `np.random` end where the literal loop leaves them whatever `chunk` is.
"""
from __future__ import annotations

import json
import os
from argparse import Namespace
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib as L
from .chunked_eval import ChunkedEval, check_pair

NAMES = ["noise0_L0", "noise0_L1", "noise1_L0", "noise1_L1", "epe_clean", "epe_adv", "l1_clean", "l1_adv", "cossim_clean",
         "cossim_adv"]
ARBITRARY_NAMES = ["epe_true", "epe_any", "adv_epe_true", "adv_epe_any", "cos_true", "cos_any", "adv_cos_true", "adv_cos_any"]
_CORRUPTIONS = ("gaussian_noise", "shot_noise", "impulse_noise", "defocus_blur", "glass_blur", "motion_blur", "zoom_blur", "snow",
                "frost", "fog", "brightness", "contrast", "elastic_transform", "pixelate", "jpeg_compression", "speckle_noise",
                "gaussian_blur", "spatter", "saturate")


def results_dict(per_item: np.ndarray) -> dict:
    """log_utils.py:330-523 from the [N,10] table: `validate`'s nested dict, key for key; `np.std` is the population form."""
    col = {n: per_item[:, i] for i, n in enumerate(NAMES)}
    side = lambda epe, l1, cos: {"EPE_mean": np.mean(col[epe]), "EPE_std": np.std(col[epe]), "L1_mean": np.mean(col[l1]),
                                 "L1_std": np.std(col[l1]), "CosSim_mean": np.mean(col[cos]), "CosSim_std": np.std(col[cos])}
    return {
        "noise0": {"L0_Pixel": np.mean(col["noise0_L0"]), "L1_Pixel": np.mean(col["noise0_L1"])},
        "noise1": {"L0_Pixel": np.mean(col["noise1_L0"]), "L1_Pixel": np.mean(col["noise1_L1"])},
        "flow": {"Unattacked": side("epe_clean", "l1_clean", "cossim_clean"), "Attacked": side("epe_adv", "l1_adv", "cossim_adv")},
    }


# ---- torch / numpy mirrors of the reference's metrics: the comparison leg of the tests and of tools/bench_global_eval.py -----------
def _at_gt_size(gt, pred):
    """perturb_model.py:43-45, :66-68, :89-91: bilinear to the ground truth's size, u times Wg/W, v times Hg/H."""
    (h, w), (hg, wg) = pred.shape[-2:], gt.shape[-2:]
    p = F.interpolate(pred, size=(hg, wg), mode="bilinear", align_corners=False)
    return torch.stack((p[:, 0] * (wg / w), p[:, 1] * (hg / h)), 1)


def _over_valid(per_pixel, gt):
    if gt.shape[1] == 3:
        valid = gt[:, 2]
        return (per_pixel * valid).sum() / (valid.sum() + 1e-8)
    return per_pixel.sum() / (gt.shape[0] * gt.shape[2] * gt.shape[3])


def compute_epe(gt, pred):
    """perturb_model.py:38-59."""
    p = _at_gt_size(gt, pred)
    return _over_valid(torch.sqrt(torch.pow(gt[:, 0] - p[:, 0], 2) + torch.pow(gt[:, 1] - p[:, 1], 2)), gt).item()


def compute_cossim(gt, pred):
    """perturb_model.py:62-81: of the RESCALED prediction (patch_attacks/losses.py takes the resized one as it is)."""
    return _over_valid(F.cosine_similarity(gt[:, :2], _at_gt_size(gt, pred)), gt).item()


def compute_l1(gt, pred):
    """perturb_model.py:84-99 with its quirk: the mean over every non-NaN entry, which `valid` does not weight."""
    diff = (_at_gt_size(gt, pred) - gt[:, :2]).abs()
    mean = torch.mean(diff[torch.logical_not(torch.isnan(diff))])
    if gt.shape[1] == 3:
        valid = gt[:, 2]
        return ((mean * valid).sum() / (valid.sum() + 1e-8)).item()
    return mean.item()


def lp_norm(T, p=1.0, axis=None):
    """eval_utils.lp_norm: p = 0 is max |T|; with an axis the mean of the p-norms along it; else mean |T|."""
    if p == 0:
        return np.max(np.abs(T))
    if axis is None:
        return np.mean(np.abs(T))
    return np.mean(np.sum(np.abs(T) ** p, axis=axis) ** (1.0 / p))


def validate_rows(noises0_output, noises1_output, origins, outputs, ground_truths, dtype=torch.float32):
    """log_utils.py:266-328 on the host lists perturb_main.run collects (noises [H,W,3], flows [2,H,W], ground truths [C,Hg,Wg],
    numpy): the [N,10] table in the order of NAMES, `FloatTensor`s like the reference unless another dtype is asked for."""
    rows = []
    for n0, n1, origin, output, gt in zip(noises0_output, noises1_output, origins, outputs, ground_truths):
        t = lambda a: torch.as_tensor(np.asarray(a)[None, ...]).to(dtype)
        rows.append((lp_norm(n0, p=0), lp_norm(n0, p=1, axis=-1), lp_norm(n1, p=0), lp_norm(n1, p=1, axis=-1),
                     compute_epe(gt=t(gt), pred=t(origin)), compute_epe(gt=t(gt), pred=t(output)),
                     compute_l1(gt=t(gt), pred=t(origin)), compute_l1(gt=t(gt), pred=t(output)),
                     compute_cossim(gt=t(gt), pred=t(origin)), compute_cossim(gt=t(gt), pred=t(output))))
    return np.asarray(rows, dtype=np.float64).reshape(len(rows), len(NAMES))


@dataclass
class GlobalEvalResult:
    per_item: np.ndarray                 # float64 [N,10] in the order of `names`
    names: list
    results_dict: dict                   # `validate`'s nested dict (means and np.std over items)
    arbitrary_rows: np.ndarray | None = None     # float64 [M,8] in the order of `arbitrary_names`: items other than arbitrary_gt_index
    arbitrary_mean: np.ndarray | None = None     # their mean (perturb_main.py:780-798)
    arbitrary_index: list | None = None          # the loader index of every row
    arbitrary_names: list = field(default_factory=lambda: list(ARBITRARY_NAMES))

    def write_json(self, output_path, seed):
        """log_utils.py:525-528: `results{seed}.json` under `output_path`."""
        path = os.path.join(output_path, f"results{seed}.json")
        with open(path, "w", encoding="utf-8") as fp:
            json.dump(self.results_dict, fp, indent=4)
        return path


def refuse_out_of_scope(args, perturb_model=None):
    """What perturb_main.run does beyond the flow table is refused where a flag asks for it."""
    flag = lambda name: bool(getattr(args, name, False))
    if flag("disparity"):
        raise NotImplementedError("disparity: stereo models are not part of this project's flow path")
    method = getattr(perturb_model, "method", None) or getattr(args, "perturb_method", None)
    if method == "self":
        raise NotImplementedError('perturb_method "self" (the clean prediction as the attack\'s ground truth) is not evaluated here')
    if method in _CORRUPTIONS:
        raise NotImplementedError(f"perturb_method {method!r}: the imagecorruptions methods are CPU image-library code, out of scope")
    if flag("return_feat_maps"):
        raise NotImplementedError("return_feat_maps: the evaluation reads the flow only")
    for name in ("write_out", "write_out_npy", "show_evolve", "flow_noise_output"):
        if flag(name):
            raise NotImplementedError(f"{name}: images, GIFs, text logs and the flow of the normalised noise (which only the "
                                      "written-out samples read) are not produced")
    if isinstance(getattr(args, "arbitrary_gt_index", None), str):
        raise NotImplementedError('building the arbitrary ground truth ("fun", "uniform_N" or a dataset index) is the caller\'s: pass '
                                  "the tensor as arbitrary_gt")


class Chunks(ChunkedEval):
    """The chunk's (apply,) forward and metrics launch (chunked_eval.py: the waiting items, the results on the device)."""

    def __init__(self, flow_net, args, chunk, arbitrary_gt=None, with_noise=True):
        super().__init__(chunk)
        self.net, self.args = flow_net, args
        self.any_gt, self.with_noise = arbitrary_gt, with_noise

    def add(self, image0, image1, gt, noise=None, adv=None):
        """One item: noise = (n0, n1) [1,3,H,W] of this item with adv = its perturbed frames, or adv None and noise the fixed
        perturbation every item shares (then applied per chunk)."""
        super().add((tuple(image0.shape), tuple(gt.shape), adv is None), image0, image1, gt, noise, adv)

    def _metrics(self, clean, advf, gt, n0, n1, K, Kn, H, W):
        lib = L.lib()
        dev = clean.device
        ws = self.workspace(lib.ufr_global_metrics_workspace_doubles(self.chunk), dev)
        out = torch.zeros(K, len(NAMES), dtype=torch.float64, device=dev)
        opt = lambda t: L.ptr(t) if t is not None else None
        L.check(lib.ufr_global_metrics(L.ptr(clean), L.ptr(advf), L.ptr(gt), opt(n0), opt(n1), K, int(gt.shape[0]), Kn,
                                       int(gt.shape[1]), H, W, int(gt.shape[2]), int(gt.shape[3]), L.ptr(ws), ws.numel(),
                                       L.ptr(out), 0, K, L.stream()), "global metrics")
        return out

    def run_chunk(self, items):
        """One chunk: (apply,) ONE forward of the clean and the perturbed pairs, metrics."""
        from .flownets.utils_model import predict_flow
        K = len(items)
        dev = items[0][1].device
        f32 = lambda ts: self.stack_f32(ts, dev)
        img0, img1, gt = f32([it[1] for it in items]), f32([it[2] for it in items]), f32([it[3] for it in items])
        H, W = int(img0.shape[2]), int(img0.shape[3])
        self._mark("start")
        if items[0][5] is None:              # the fixed perturbation
            n0, n1 = (n.detach().to(torch.float32).contiguous() for n in items[0][4])
            adv0, adv1 = torch.empty_like(img0), torch.empty_like(img1)
            L.check(L.lib().ufr_global_apply(L.ptr(img0), L.ptr(img1), L.ptr(n0), L.ptr(n1), L.ptr(adv0), L.ptr(adv1), K, 1, H, W,
                                             0.0, 1.0, L.stream()), "global apply")
            Kn = 1
        else:
            n0, n1 = f32([it[4][0] for it in items]), f32([it[4][1] for it in items])
            adv0, adv1 = f32([it[5][0] for it in items]), f32([it[5][1] for it in items])
            Kn = K
        self._mark("apply")
        flows = predict_flow(self.net, None, torch.cat((img0, adv0)), torch.cat((img1, adv1)), self.args)
        flows = self.checked_flow(flows, 2 * K, H, W).to(torch.float32).contiguous()
        Hp, Wp = int(flows.shape[2]), int(flows.shape[3])
        self._mark("forward")
        if not self.with_noise:
            n0 = n1 = None
        out = self._metrics(flows[:K], flows[K:], gt, n0, n1, K, Kn, Hp, Wp)
        if self.any_gt is not None:
            out = (out, self._metrics(flows[:K], flows[K:], self.any_gt, None, None, K, 0, Hp, Wp))
        self._mark("metrics")
        return out

    def read(self):
        """The one host synchronisation: ([N,10], [N,10] against the arbitrary ground truth or None)."""
        tables = super().read() or [np.zeros((0, len(NAMES)))] * 2
        return tables[0], (tables[1] if self.any_gt is not None else None)


def _unpack(data):
    """perturb_main.py:467-475: (image0, image1, ground_truth, ground_truth_downsampled or None)."""
    if len(data) == 4:
        return data[0], data[1], data[2], data[3]
    if len(data) == 5:
        return data[0], data[1], data[2], torch.cat((data[3], data[4][:, None, ...]), dim=1)
    if len(data) == 7:
        return data[1], data[2], data[3], None
    raise ValueError(f"a loader item is the reference's 4-, 5- or 7-tuple, got {len(data)} entries")


def evaluate_perturbation(flow_net, loader, args: Namespace, *, perturb_model=None, noise=None, arbitrary_gt=None,
                          arbitrary_gt_index=None, chunk=4) -> GlobalEvalResult:
    """perturb_main.run's loop (:466-812, `disparity=False`) and `validate`'s table without their images, GIFs and logs.

    loader yields the reference's batch-1 items as HIP tensors: `(image0, image1, ground_truth, ground_truth_downsampled)`,
    `(image0, image1, ground_truth, flow_downsampled, valid_downsampled)` or the 7-tuple `(_, image0, image1, ground_truth, _, _, _)`;
    frames [1,3,H,W], ground truths [1,C,Hg,Wg] with C = 3 (u, v, valid) or 2.  Exactly one of
      perturb_model  a `PerturbationsModel`: its `forward` runs per item at batch 1, in loader order, against
                     `ground_truth_downsampled` -- or `arbitrary_gt` when given (:570-574); the noise is what `forward` returns;
      noise          `(n0, n1)`, [1,3,H,W] each: `--universal_evaluation` (:546-550) and `--arbitrary_noise_index` (:551-553,
                     :618-623); the frames become clamp(image + n, 0, 1) and the noise metrics are those of n itself.
    `args.homogeneous`: image1 = image0, a zero ground truth, and the loop stops after the first item (:477-481, :777-778).
    `arbitrary_gt` ([C,Hg,Wg] or [1,C,Hg,Wg]) adds `arbitrary_rows` (:699-708) for every item whose index differs from
    `arbitrary_gt_index`.  The parameters are frozen like the attack steps freeze them (`patch_attack.release(flow_net)` gives the
    flags back); the host synchronises once."""
    refuse_out_of_scope(args, perturb_model)
    if (perturb_model is None) == (noise is None):
        raise ValueError("exactly one of perturb_model (a per-image attack) and noise (a fixed perturbation) is needed")
    if noise is not None:
        n0, n1 = noise
        check_pair(n0, n1, "noise is (n0, n1), [1,3,H,W] each")
        L.require_hip(n0, "noise0", contiguous=False)
        L.require_hip(n1, "noise1", contiguous=False)
    if arbitrary_gt is not None:
        if arbitrary_gt.dim() == 3:
            arbitrary_gt = arbitrary_gt[None]
        if arbitrary_gt.dim() != 4 or arbitrary_gt.shape[0] != 1 or arbitrary_gt.shape[1] not in (2, 3):
            raise ValueError("arbitrary_gt must be [C,Hg,Wg] or [1,C,Hg,Wg] with C = 2 or 3")
        L.require_hip(arbitrary_gt, "arbitrary_gt", contiguous=False)
        arbitrary_gt = arbitrary_gt.detach().to(torch.float32).contiguous()
    homogeneous = bool(getattr(args, "homogeneous", False))
    ev = Chunks(flow_net, args, chunk, arbitrary_gt)
    ev.events = getattr(evaluate_perturbation, "_debug_events", None)     # tools/bench_global_eval.py: device events around the entries
    count = 0
    for data in loader:
        image0, image1, gt, gt_down = _unpack(data)
        if homogeneous:
            image1, gt = image0, torch.zeros_like(gt)
        check_pair(image0, image1, "the loader yields batch-1 items: image0 and image1 [1,3,H,W]")
        if gt.dim() != 4 or gt.shape[0] != 1 or gt.shape[1] not in (2, 3):
            raise ValueError("ground_truth must be [1,C,Hg,Wg] with C = 2 or 3")
        for t, name in ((image0, "image0"), (image1, "image1"), (gt, "ground_truth")):
            L.require_hip(t, name, contiguous=False)
        ev.freeze_once(flow_net)
        with torch.cuda.device(image0.device):          # the attack's; a chunk runs under the guard of its own items
            if perturb_model is not None:
                target = arbitrary_gt if arbitrary_gt is not None else gt_down
                if target is None:
                    raise ValueError("a 7-tuple item carries no downsampled ground truth for the attack: pass arbitrary_gt, or use "
                                     "the 4- or 5-tuple items")
                n0, n1, adv0, adv1 = perturb_model.forward(flow_net, image0, image1, target)
                ev.add(image0, image1, gt, (n0.detach(), n1.detach()), (adv0.detach(), adv1.detach()))
            else:
                if tuple(noise[0].shape) != tuple(image0.shape):
                    raise ValueError(f"the fixed noise is {tuple(noise[0].shape)}, item {count} is {tuple(image0.shape)}")
                ev.add(image0, image1, gt, noise, None)
        count += 1
        if homogeneous:
            break
    per_item, per_item_any = ev.read()
    res = GlobalEvalResult(per_item, list(NAMES), results_dict(per_item) if len(per_item) else {})
    if arbitrary_gt is not None:
        keep = [i for i in range(len(per_item)) if arbitrary_gt_index is None or i != int(arbitrary_gt_index)]
        cols = [NAMES.index(n) for n in ("epe_clean", "epe_adv", "cossim_clean", "cossim_adv")]
        rows = np.stack([np.stack((per_item[keep][:, c], per_item_any[keep][:, c]), 1) for c in cols], 1).reshape(len(keep), 8)
        res.arbitrary_rows, res.arbitrary_index = rows, keep
        res.arbitrary_mean = rows.mean(axis=0) if len(keep) else np.zeros(8)
    return res
