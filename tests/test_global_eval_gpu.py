"""GPU suite of the global-attack evaluation (global_eval.py, csrc/global_eval.hip, universal_perturbation.validation / train): the
apply entry against torch (bit for bit), the metrics entry against a float64 restatement, and `evaluate_perturbation`,
`validation` and `train` against the reference's literal loops (perturb_main.py:466-812 with log_utils.validate,
universal_perturbation.py:533-566 and :354-397, restated at batch 1 with this project's mirrors and host copies)."""
import random
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = dict(dtype=torch.float32, device=DEV)
H, W, HG, WG = 128, 256, 120, 250


def _L():
    from understanding_flow_robustness_amd import _lib as L
    return L


def _ge():
    from understanding_flow_robustness_amd import global_eval as ge
    return ge


# ------------------------------------------------------------------------------------------------------------------ 1. apply
def _shifted(t, off, fill=None):
    """A copy of `t` (or `fill` of its shape) that starts `off` elements into a NaN-filled buffer with 16 guard elements behind:
    (the view, the whole buffer)."""
    whole = torch.full((off + t.numel() + 16,), float("nan"), **F32)
    view = whole[off:off + t.numel()].view(t.shape)
    if fill is None:
        view.copy_(t)
    return view, whole


@pytest.mark.parametrize("shifted", ["none", "all", "adv1"])                    # a pointer offset by one element: the scalar path
@pytest.mark.parametrize("kn", [1, 3])
@pytest.mark.parametrize("h,w", [(5, 7), (8, 12)])                              # 3*H*W % 4 != 0 (scalar) and == 0 (16-byte accesses)
def test_apply_is_bit_equal_to_torch(h, w, kn, shifted):
    L = _L()
    K = 3
    g = torch.Generator().manual_seed(100 * h + kn)
    img0, img1 = (torch.rand(K, 3, h, w, generator=g) * 1.4 - 0.2 for _ in range(2))       # values on both sides of [lo, hi]
    n0, n1 = (torch.rand(kn, 3, h, w, generator=g) * 0.8 - 0.4 for _ in range(2))
    off = 1 if shifted == "all" else 0
    (img0, _), (img1, _), (n0, _), (n1, _) = (_shifted(t.to(DEV), off) for t in (img0, img1, n0, n1))
    for lo, hi in ((0.0, 1.0), (0.25, 0.75)):
        adv0, whole0 = _shifted(img0, off, fill="nan")
        adv1, whole1 = _shifted(img1, 1 if shifted != "none" else 0, fill="nan")
        assert (adv0.data_ptr() % 16 == 0) == (shifted != "all") and (adv1.data_ptr() % 16 == 0) == (shifted == "none")
        L.check(L.lib().ufr_global_apply(L.ptr(img0), L.ptr(img1), L.ptr(n0), L.ptr(n1), L.ptr(adv0), L.ptr(adv1), K, kn, h, w, lo, hi,
                                         L.stream()), "global apply")
        want0, want1 = torch.clamp(img0 + n0, lo, hi), torch.clamp(img1 + n1, lo, hi)
        assert torch.equal(adv0, want0) and torch.equal(adv1, want1)
        assert float(want0.min()) == lo and float(want0.max()) == hi and float((want0 - img0).abs().max()) > 0.1
        for view, whole in ((adv0, whole0), (adv1, whole1)):                    # nothing in front of the output, nothing behind it
            inside = torch.zeros_like(whole, dtype=torch.bool)
            start = (view.data_ptr() - whole.data_ptr()) // 4
            inside[start:start + view.numel()] = True
            assert bool(torch.isnan(whole[~inside]).all()) and int((~inside).sum()) == whole.numel() - view.numel() >= 16


# ------------------------------------------------------------------------------------------------------------------ 2. metrics
MK, MH, MW = 3, 24, 40
# ground-truth sizes: smaller, equal (the resize is the identity; 960 pixels are several workgroups of one item), larger, and 9 x 13,
# which fills less than one workgroup
MSIZES = [(23, 37), (24, 40), (31, 53), (9, 13), (130, 254)]          # the last: 129 > 128 workgroups, a second pixel per thread


def _metric_operands(hg, wg, C, nan_pixels=False):
    """Host tensors.  The clean prediction follows the ground truth, the attacked one does not (so swapping them is seen); where the
    valid channel is 0 the ground truth is far off (so the L1 column, which `valid` does not weight, is not the weighted one)."""
    g = torch.Generator().manual_seed(1000 * hg + C)
    pred_c, pred_a = (torch.randn(MK, 2, MH, MW, generator=g) * 4.0 for _ in range(2))
    pred_c = pred_c[:1] + 0.25 * pred_c                      # the items' clean predictions are alike: one ground truth can serve all
    uv = F.interpolate(pred_c, size=(hg, wg), mode="bilinear", align_corners=False) + torch.randn(MK, 2, hg, wg, generator=g)
    valid = (torch.rand(MK, 1, hg, wg, generator=g) > 0.3).float()
    uv = uv + 10.0 * (1.0 - valid)
    if nan_pixels:
        uv[0, 0, 1, 2] = uv[1, 1, 3, 4] = uv[2, 0, hg - 1, wg - 1] = uv[2, 1, 0, 0] = float("nan")
    gt = torch.cat((uv, valid), 1) if C == 3 else uv
    n0, n1 = (torch.rand(MK, 3, MH, MW, generator=g) * 0.04 - 0.02 for _ in range(2))
    return pred_c, pred_a, gt.contiguous(), n0, n1


def _restated(pred_c, pred_a, gt, n0, n1, dtype):
    """`validate` item by item in `dtype` through the project's mirrors; gt [Kg,...] and the noises [Kn,...] with Kg, Kn in {1, K};
    noise None: NaN columns."""
    ge = _ge()
    rows = []
    for k in range(pred_c.shape[0]):
        g = gt[k if gt.shape[0] > 1 else 0]
        if n0 is None:
            a = b = np.full((MH, MW, 3), np.nan)
        else:
            a, b = (n[k if n.shape[0] > 1 else 0].permute(1, 2, 0).cpu().numpy() for n in (n0, n1))
            if dtype == torch.float64:
                a, b = a.astype(np.float64), b.astype(np.float64)
        rows.append(ge.validate_rows([a], [b], [pred_c[k].cpu().numpy()], [pred_a[k].cpu().numpy()], [g.cpu().numpy()], dtype=dtype)[0])
    return np.asarray(rows)


def _run_metrics(pred_c, pred_a, gt, n0, n1):
    L = _L()
    lib = L.lib()
    K = pred_c.shape[0]
    ws = torch.zeros(lib.ufr_global_metrics_workspace_doubles(K), dtype=torch.float64, device=DEV)
    out = torch.full((K + 2, 10), -7.0, dtype=torch.float64, device=DEV)
    opt = lambda t: L.ptr(t) if t is not None else None
    L.check(lib.ufr_global_metrics(L.ptr(pred_c), L.ptr(pred_a), L.ptr(gt), opt(n0), opt(n1), K, gt.shape[0],
                                   n0.shape[0] if n0 is not None else 0, gt.shape[1], MH, MW, gt.shape[2], gt.shape[3], L.ptr(ws),
                                   ws.numel(), L.ptr(out), 1, K + 2, L.stream()), "global metrics")
    assert bool((out[0] == -7.0).all()) and bool((out[-1] == -7.0).all())       # only the caller's row range is written
    return out[1:-1].clone()


def _judge(out, want, f32, what, nan_cols=()):
    """Bound per value: the larger of 1e-6 * |value| and 4 x the error of the float32 torch spelling against the same float64
    values (the rule of test_patch_eval_gpu.py::test_metrics_against_float64_restatement); noise_L0 exactly equal; the columns
    in `nan_cols` are NaN on both sides, asserted explicitly."""
    got = out.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape
    cols = [c for c in range(10) if c not in nan_cols]
    for c in nan_cols:
        assert np.isnan(got[:, c]).all() and np.isnan(want[:, c]).all(), (what, c, got[:, c], want[:, c])
    assert np.isfinite(got[:, cols]).all() and np.isfinite(want[:, cols]).all() and np.isfinite(f32[:, cols]).all(), what
    err, err32 = np.abs(got - want)[:, cols], np.abs(f32 - want)[:, cols]
    bound = np.maximum(1e-6 * np.abs(want[:, cols]), 4.0 * err32)
    report = (f"{what}: columns {cols}: kernel error {err.max(0).tolist()}; float32 torch error {err32.max(0).tolist()}; "
              f"values {want[:, cols].tolist()}")
    print(report)
    assert (err <= bound).all(), report
    for c in (0, 2):
        if c in cols:
            assert (got[:, c] == want[:, c]).all(), f"{what}: noise_L0 is a maximum of float32 values: exactly equal"


@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("hg,wg", MSIZES)
def test_metrics_against_float64_restatement(hg, wg, C):
    pred_c, pred_a, gt, n0, n1 = (t.to(DEV).contiguous() for t in _metric_operands(hg, wg, C))
    for kg in (1, MK):
        for kn in (1, MK, None):
            g = gt[:kg].contiguous()
            a, b = (None, None) if kn is None else (n0[:kn].contiguous(), n1[:kn].contiguous())
            want = _restated(pred_c, pred_a, g, a, b, torch.float64)
            f32 = _restated(pred_c, pred_a, g, a, b, torch.float32)
            out = _run_metrics(pred_c, pred_a, g, a, b)
            again = _run_metrics(pred_c, pred_a, g, a, b)
            assert torch.equal(out.view(torch.int64), again.view(torch.int64)), "two runs differ"
            _judge(out, want, f32, f"Hg x Wg = {hg}x{wg}, C = {C}, Kg = {kg}, Kn = {kn}", nan_cols=(0, 1, 2, 3) if kn is None else ())
            if kn is not None:                               # noise one element off 16-byte alignment: the scalar walk over the noise
                a1, b1 = _shifted(a, 1)[0], _shifted(b, 1)[0]
                assert a1.data_ptr() % 16 == 4 and torch.equal(a1, a)
                scalar = _run_metrics(pred_c, pred_a, g, a1, b1)
                _judge(scalar, want, f32, f"Hg x Wg = {hg}x{wg}, C = {C}, Kg = {kg}, Kn = {kn}, scalar noise walk")
                # the alignment picks the walk, not the workgroup count: the flow sums keep their order
                assert torch.equal(scalar[:, 4:], out[:, 4:]) and torch.equal(scalar[:, [0, 2]], out[:, [0, 2]])
            # the operands discriminate: swapping the predictions changes every flow column of every item by more than 1e-3
            for clean, adv in ((4, 5), (6, 7), (8, 9)):
                assert (np.abs(want[:, clean] - want[:, adv]) > 1e-3).all(), (clean, want[:, clean], want[:, adv])
            swapped = _run_metrics(pred_a, pred_c, g, a, b).cpu().numpy()
            assert np.array_equal(swapped[:, [5, 4, 7, 6, 9, 8]], out.cpu().numpy()[:, 4:])
            if C == 3:                                       # the quirk: the L1 column is not the valid-weighted L1
                for k in range(MK):
                    gk = g[k if kg > 1 else 0][None].double()
                    for col, pred in ((6, pred_c), (7, pred_a)):
                        p = F.interpolate(pred[k:k + 1].double(), size=(hg, wg), mode="bilinear", align_corners=False)
                        p = torch.stack((p[:, 0] * (wg / MW), p[:, 1] * (hg / MH)), 1)
                        weighted = float(((p - gk[:, :2]).abs().sum(1) * gk[:, 2]).sum() / (2.0 * gk[:, 2].sum()))
                        assert abs(weighted - want[k, col]) > 1e-3


def test_metrics_with_nan_in_the_ground_truth():
    """A few NaN pixels in gt: the L1 columns exclude them and match the restatement; the EPE columns (and the cosine similarity,
    whose per-pixel value is NaN there too) are NaN on both sides."""
    pred_c, pred_a, gt, n0, n1 = (t.to(DEV).contiguous() for t in _metric_operands(23, 37, 3, nan_pixels=True))
    assert int(torch.isnan(gt).sum()) == 4
    want = _restated(pred_c, pred_a, gt, n0, n1, torch.float64)
    f32 = _restated(pred_c, pred_a, gt, n0, n1, torch.float32)
    out = _run_metrics(pred_c, pred_a, gt, n0, n1)
    _judge(out, want, f32, "NaN in gt", nan_cols=(4, 5, 8, 9))
    clean, _, gt_clean, _, _ = _metric_operands(23, 37, 3)
    without = _restated(pred_c, pred_a, gt_clean.to(DEV), n0, n1, torch.float64)
    assert np.isfinite(without).all() and (np.abs(without[:, 6] - want[:, 6]) > 1e-6).all()    # excluding them moved the mean


# ------------------------------------------------------------------------------------------------------------------ 3. literal loops
@pytest.fixture(scope="module")
def net():
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    return fetch_model(Namespace(flownet="FlowNetC"), synthetic_seed=0).to(DEV)


def _args(**kw):
    return Namespace(flownet="FlowNetC", flow_loss="l2", **kw)


SIGMA = 0.05


def _items(model, args, n, h=H, w=W, hg=HG, wg=WG, seed=41, channels=3):
    """The reference's 4-tuples (image0, image1, ground_truth, ground_truth_downsampled) on the device.  The ground truth is the
    network's own clean prediction, resized and rescaled, plus noise of standard deviation SIGMA, with holes in its valid channel
    (`channels` = 2: without one).  When the prediction moves by d, the end-point error against prediction + independent noise
    moves by about |d|^2 / sigma only while |d| < sigma, and by |d| beyond: the noise has to be SMALLER than what an attack of
    0.02 does to the prediction for the attack to be seen in the error at all, so it is 0.05 and not 1."""
    from understanding_flow_robustness_amd.flownets.utils_model import predict_flow
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        image0, image1 = (torch.rand(1, 3, h, w, generator=g).to(DEV) for _ in range(2))
        with torch.no_grad():
            clean = predict_flow(model, None, image0, image1, args).float().cpu()
        full = F.interpolate(clean, size=(hg, wg), mode="bilinear", align_corners=False)
        full = torch.stack((full[:, 0] * (wg / clean.shape[3]), full[:, 1] * (hg / clean.shape[2])), 1)
        full = full + SIGMA * torch.randn(1, 2, hg, wg, generator=g)
        down = F.interpolate(clean, size=(h, w), mode="bilinear", align_corners=False) + SIGMA * torch.randn(1, 2, h, w, generator=g)
        valid = lambda a, b: (torch.rand(1, 1, a, b, generator=g) > 0.3).float()
        full = torch.cat((full, valid(hg, wg)), 1) if channels == 3 else full
        out.append((image0, image1, full.to(DEV), torch.cat((down, valid(h, w)), 1).to(DEV)))
    return out


@pytest.fixture(scope="module")
def items(net):
    return _items(net, _args(), 5)


@pytest.fixture(scope="module")
def items_two_channels(net):
    """`homogeneous` zeroes the WHOLE ground truth (perturb_main.py:481): with a valid channel every flow metric is 0 / 1e-8 = 0,
    clean and attacked.  Only a 2-channel ground truth lets that case see the attack."""
    return _items(net, _args(), 2, seed=45, channels=2)


def _seed(seed=1234):
    torch.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)


def _generators():
    """Where the three generators stand (read AFTER a run: it moves them)."""
    return float(torch.rand(1)), random.random(), float(np.random.random())


def _literal_loop(model, args, loader, make_pm=None, noise=None, arbitrary_gt=None, arbitrary_gt_index=None):
    """perturb_main.py:466-812 (flow branch) at batch 1 with this project's PerturbationsModel and predict_flow, the host copies of
    :653-667 and the float32 `validate`.  Returns ([N,10], arbitrary rows [M,8])."""
    from understanding_flow_robustness_amd.flownets.utils_model import predict_flow
    ge = _ge()
    noises0, noises1, origins, outputs, gts, errors = [], [], [], [], [], []
    for idx, data in enumerate(loader):
        image0, image1, ground_truth, ground_truth_downsampled = data
        if getattr(args, "homogeneous", False):
            image1 = image0
            ground_truth = torch.zeros_like(ground_truth)
        gts.append(np.squeeze(ground_truth.cpu().numpy()))
        perturb_model = make_pm() if make_pm is not None else None
        with torch.no_grad():
            flow_origin = predict_flow(model, None, image0, image1, args)
        if noise is not None:
            image0_output = torch.clamp(image0 + noise[0], 0.0, 1.0)
            image1_output = torch.clamp(image1 + noise[1], 0.0, 1.0)
            noise0_output, noise1_output = torch.clone(noise[0]), torch.clone(noise[1])
        else:
            _ground_truth = ground_truth_downsampled if arbitrary_gt is None else arbitrary_gt.clone()[None, ...]
            noise0_output, noise1_output, image0_output, image1_output = perturb_model.forward(model, image0, image1, _ground_truth)
        with torch.no_grad():
            flow_output = predict_flow(model, None, image0_output, image1_output, args)
        noises0.append(np.transpose(np.squeeze(noise0_output.detach().cpu().numpy()), (1, 2, 0)))
        noises1.append(np.transpose(np.squeeze(noise1_output.detach().cpu().numpy()), (1, 2, 0)))
        origins.append(np.squeeze(flow_origin.detach().cpu().numpy()))
        outputs.append(np.squeeze(flow_output.detach().cpu().numpy()))
        if arbitrary_gt is not None and arbitrary_gt_index != idx:
            true_gt, any_gt = ground_truth, arbitrary_gt.clone()[None, ...]
            errors.append([ge.compute_epe(gt=true_gt, pred=flow_origin), ge.compute_epe(gt=any_gt, pred=flow_origin),
                           ge.compute_epe(gt=true_gt, pred=flow_output), ge.compute_epe(gt=any_gt, pred=flow_output),
                           ge.compute_cossim(gt=true_gt, pred=flow_origin), ge.compute_cossim(gt=any_gt, pred=flow_origin),
                           ge.compute_cossim(gt=true_gt, pred=flow_output), ge.compute_cossim(gt=any_gt, pred=flow_output)])
        if getattr(args, "homogeneous", False):
            break
    with torch.no_grad():
        rows = ge.validate_rows(noises0, noises1, origins, outputs, gts)
    return rows, np.asarray(errors, dtype=np.float64).reshape(len(errors), 8)


def _assert_rows(got, want, what):
    """The project's parity gate (test_patch_eval_gpu.py::_assert_rows): EPE and L1 within 1e-4 relative, cosine similarity within
    1e-4 absolute; the noise columns within 1e-6 relative (the attack is the same batch-1 code on both sides)."""
    assert got.shape == want.shape and got.dtype == np.float64 and np.isfinite(got).all() and np.isfinite(want).all(), what
    n, e, c = np.abs(got[:, :4] - want[:, :4]), np.abs(got[:, 4:8] - want[:, 4:8]), np.abs(got[:, 8:] - want[:, 8:])
    rel = lambda d, w: float(np.where(d > 0, d / np.maximum(np.abs(w), 1e-300), 0.0).max())
    print(f"{what}: noise differs by {rel(n, want[:, :4]):.2e} relative, EPE / L1 by {rel(e, want[:, 4:8]):.2e} relative, "
          f"cos-sim by {c.max():.2e} absolute")
    assert (n <= 1e-6 * np.abs(want[:, :4])).all(), f"{what}: noise norms {got[:, :4].tolist()} against {want[:, :4].tolist()}"
    assert (e <= 1e-4 * np.abs(want[:, 4:8])).all(), f"{what}: EPE / L1 {got[:, 4:8].tolist()} against {want[:, 4:8].tolist()}"
    assert c.max() <= 1e-4, f"{what}: cos-sim differs by {c.max():.2e} absolute"


def _assert_dicts(got, want, what):
    """results_dict within the same gates, key for key."""
    assert list(got) == list(want) == ["noise0", "noise1", "flow"]
    for name in ("noise0", "noise1"):
        assert list(got[name]) == list(want[name])
        for key in want[name]:
            assert np.isfinite(got[name][key]) and abs(got[name][key] - want[name][key]) <= 1e-6 * abs(want[name][key]), (what, name, key)
    scale = {side: max(abs(want["flow"][side]["EPE_mean"]), abs(want["flow"][side]["L1_mean"])) for side in want["flow"]}
    for side in ("Unattacked", "Attacked"):
        assert list(got["flow"][side]) == list(want["flow"][side])
        for key, w in want["flow"][side].items():
            v = got["flow"][side][key]
            # a standard deviation of values that are each within 1e-4 relative is within 1e-4 of their magnitude
            tol = 1e-4 if key.startswith("CosSim") else 1e-4 * (abs(w) if key.endswith("_mean") else scale[side])
            assert np.isfinite(v) and abs(v - w) <= tol, (what, side, key, v, w)


def _pm(args, method, **kw):
    from understanding_flow_robustness_amd.perturb_model import PerturbationsModel
    opts = dict(perturb_method=method, perturb_mode="both", output_norm=0.02, n_step=3, learning_rate=0.005, momentum=0.47,
                probability_diverse_input=0.0, args=args)
    opts.update(kw)
    return lambda: PerturbationsModel(**opts)


def _fixed_noise(h=H, w=W, eps=0.05, seed=77):
    g = torch.Generator().manual_seed(seed)
    return tuple((torch.rand(1, 3, h, w, generator=g) * 2 * eps - eps).to(DEV) for _ in range(2))


def _arbitrary_gt(seed=9):
    g = torch.Generator().manual_seed(seed)
    return torch.cat((torch.randn(2, H, W, generator=g) * 3.0, (torch.rand(1, H, W, generator=g) > 0.3).float())).to(DEV)


LOOP_CASES = {
    "fixed_universal_noise": dict(noise=True),
    "ifgsm": dict(method="ifgsm"),
    "mifgsm_diverse": dict(method="mifgsm", pm=dict(probability_diverse_input=0.5)),
    "fgsm": dict(method="fgsm"),
    "targeted_arbitrary_gt": dict(method="ifgsm", pm=dict(targeted=True), arbitrary=True),
    "homogeneous": dict(method="ifgsm", homogeneous=True),
}


def _run_both(model, loader, case, chunk, args=None):
    spec = LOOP_CASES[case]
    args = args or _args(homogeneous=bool(spec.get("homogeneous", False)))
    make_pm = _pm(args, spec["method"], **spec.get("pm", {})) if "method" in spec else None
    noise = _fixed_noise(*loader[0][0].shape[2:]) if spec.get("noise") else None
    any_gt, any_index = (_arbitrary_gt(), 1) if spec.get("arbitrary") else (None, None)
    _seed()
    want, want_any = _literal_loop(model, args, loader, make_pm, noise, any_gt, any_index)
    want_state = _generators()
    _seed()
    res = _ge().evaluate_perturbation(model, loader, args, perturb_model=make_pm() if make_pm else None, noise=noise,
                                      arbitrary_gt=any_gt, arbitrary_gt_index=any_index, chunk=chunk)
    got_state = _generators()
    return res, want, want_any, got_state, want_state


@pytest.mark.parametrize("case", sorted(LOOP_CASES))
def test_evaluate_perturbation_equals_the_literal_loop(net, items, items_two_channels, case):
    """Five items with chunk = 2: two full chunks and a ragged one."""
    ge = _ge()
    if case == "homogeneous":
        items = items_two_channels
    res, want, want_any, got_state, want_state = _run_both(net, items, case, chunk=2)
    n = 1 if case == "homogeneous" else 5
    assert res.names == ge.NAMES and res.per_item.shape == (n, 10) and want.shape == (n, 10)
    _assert_rows(res.per_item, want, case)
    assert got_state == want_state, "torch / random / np.random were consumed differently"
    _assert_dicts(res.results_dict, ge.results_dict(want), case)
    # the case discriminates, in the literal loop's own values: attacked and clean EPE differ by more than ten times the gate
    assert (np.abs(want[:, 5] - want[:, 4]) > 1e-3 * np.abs(want[:, 4])).all(), (want[:, 4].tolist(), want[:, 5].tolist())
    assert (want[:, 0] > 0).all() and (want[:, 3] > 0).all()
    if case == "targeted_arbitrary_gt":
        assert res.arbitrary_index == [0, 2, 3, 4] and res.arbitrary_rows.shape == want_any.shape == (4, 8)
        assert res.arbitrary_names == ["epe_true", "epe_any", "adv_epe_true", "adv_epe_any", "cos_true", "cos_any", "adv_cos_true",
                                       "adv_cos_any"]
        e, c = np.abs(res.arbitrary_rows[:, :4] - want_any[:, :4]), np.abs(res.arbitrary_rows[:, 4:] - want_any[:, 4:])
        print(f"arbitrary rows: EPE differs by {(e / np.abs(want_any[:, :4])).max():.2e} relative, cos-sim by {c.max():.2e} absolute")
        assert np.isfinite(res.arbitrary_rows).all() and (e <= 1e-4 * np.abs(want_any[:, :4])).all() and c.max() <= 1e-4
        assert np.array_equal(res.arbitrary_mean, res.arbitrary_rows.mean(axis=0))
        assert (np.abs(want_any[:, 1] - want_any[:, 0]) > 1e-3).all()           # the other ground truth is another one
        assert (want_any[:, 3] < want_any[:, 1]).all()                           # and the targeted attack moves towards it
    else:
        assert res.arbitrary_rows is None
    if case == "homogeneous":
        assert (want[:, 4] > 0).all()


def test_chunk_one_equals_chunk_four(net, items):
    ge = _ge()
    args = _args()
    runs = {}
    for chunk in (1, 4):
        _seed()
        res = ge.evaluate_perturbation(net, items, args, perturb_model=_pm(args, "mifgsm", probability_diverse_input=0.5)(), chunk=chunk)
        runs[chunk] = (res, _generators())
    _assert_rows(runs[4][0].per_item, runs[1][0].per_item, "chunk 4 against chunk 1")
    assert runs[4][1] == runs[1][1]
    _seed()
    assert _generators() != runs[1][1]                                          # the attack did draw


def test_items_of_another_size_start_a_new_chunk(net):
    """Chunks hold consecutive items of equal frame and ground-truth size; the order of the results is the loader's."""
    args = _args()
    loader = _items(net, args, 2, seed=50) + _items(net, args, 1, h=128, w=192, hg=100, wg=180, seed=51) + _items(net, args, 1, seed=52)
    _seed()
    want, _ = _literal_loop(net, args, loader, _pm(args, "fgsm"))
    _seed()
    res = _ge().evaluate_perturbation(net, loader, args, perturb_model=_pm(args, "fgsm")(), chunk=4)
    _assert_rows(res.per_item, want, "mixed sizes")


def test_second_network_on_the_generic_path():
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    args = Namespace(flownet="PWCNet", flow_loss="l2", homogeneous=False)
    pwc = fetch_model(args, synthetic_seed=0).to(DEV)
    loader = _items(pwc, args, 3, h=128, w=192, hg=120, wg=180, seed=43)
    res, want, _, got_state, want_state = _run_both(pwc, loader, "ifgsm", chunk=2, args=args)
    _assert_rows(res.per_item, want, "PWC-Net")
    assert got_state == want_state
    assert (np.abs(want[:, 5] - want[:, 4]) > 1e-3 * np.abs(want[:, 4])).all()


# ------------------------------------------------------------------------------------------------------------------ 4. universal
def _universal_args(**kw):
    opts = dict(flownet="FlowNetC", flow_loss="l2", perturb_method="ifgsm", perturb_mode="both", learning_rate=0.005, output_norm=0.02,
                n_step=2, add_gaussian=False)
    opts.update(kw)
    return Namespace(**opts)


def test_universal_validation_equals_its_literal_loop(net, items):
    """universal_perturbation.py:533-566 at batch 1: the four metrics, averaged."""
    from understanding_flow_robustness_amd import universal_perturbation as up
    from understanding_flow_robustness_amd.flownets.utils_model import predict_flow
    ge = _ge()
    args = _universal_args()
    n0, n1 = _fixed_noise()
    universal = torch.stack((n0, n1), 1)                                        # [1,2,3,H,W]
    loader = [(torch.zeros_like(a), a, b, gt, None, None, None) for a, b, gt, _ in items]
    rows = []
    with torch.no_grad():
        for ref_past, tgt, ref_future, flow_gt, _, _, _ in loader:
            flow_fwd = predict_flow(net, ref_past, tgt, ref_future, args)
            adv_tgt, adv_ref = up.add_universal_perturbation(tgt, ref_future, universal)
            adv_flow_fwd = predict_flow(net, None, adv_tgt, adv_ref, args)
            rows.append([ge.compute_epe(gt=flow_gt, pred=flow_fwd), ge.compute_epe(gt=flow_gt, pred=adv_flow_fwd),
                         ge.compute_cossim(flow_gt, flow_fwd), ge.compute_cossim(flow_gt, adv_flow_fwd)])
    want = np.asarray(rows, dtype=np.float64).mean(axis=0)
    got, names = up.validation(universal, loader, net, 0, args, chunk=2)
    assert names == ["epe", "adv_epe", "cos_sim", "adv_cos_sim"] and len(got) == 4 and all(isinstance(v, float) for v in got)
    got = np.asarray(got)
    print(f"validation: {got.tolist()} against {want.tolist()}")
    assert np.isfinite(got).all() and np.isfinite(want).all()
    assert (np.abs(got[:2] - want[:2]) <= 1e-4 * np.abs(want[:2])).all() and np.abs(got[2:] - want[2:]).max() <= 1e-4
    assert abs(want[1] - want[0]) > 1e-3 * want[0]                               # the perturbation is seen


@pytest.mark.parametrize("add_gaussian", [False, True])
def test_universal_train_equals_chained_attacks_bit_for_bit(net, items, add_gaussian):
    """universal_perturbation.py:354-397 over three items: the carried perturbation of three chained `attack` calls; with
    `add_gaussian` torch's generator ends where the literal loop leaves it."""
    from understanding_flow_robustness_amd import universal_perturbation as up
    from understanding_flow_robustness_amd.flownets.utils_model import predict_flow
    args = _universal_args(add_gaussian=add_gaussian)
    loader = [(a, [torch.zeros_like(b), b]) for a, b, _, _ in items[:3]]
    start = torch.zeros(1, 2, 3, H, W, **F32)
    torch.manual_seed(5)
    want = start.clone()
    for tgt, (ref_past, ref_future) in loader:
        flow_pred = predict_flow(net, ref_past, tgt, ref_future, args)
        if not add_gaussian:
            target = -1 * flow_pred.data.clone()
        else:
            target = flow_pred.data.clone() + 1 * torch.randn(flow_pred.shape).cuda()
        _, _, _, want = up.attack(net, tgt, ref_future, want, target_var=target, args=args)
    want_state = float(torch.rand(1))
    torch.manual_seed(5)
    got = up.train(start.clone(), loader, net, args)
    got_state = float(torch.rand(1))
    assert got.shape == want.shape == (1, 2, 3, H, W) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want) and got_state == want_state
    assert float(got.abs().max()) > 0.0 and float(start.abs().max()) == 0.0
    torch.manual_seed(5)
    assert (float(torch.rand(1)) != want_state) == add_gaussian                 # only the gaussian target draws
