"""CPU suite of the global-attack evaluation (global_eval.py): the float32 torch restatement of `validate`'s six metrics and two
norms reproduces values recorded from the reference's own compute_epe / compute_cossim / compute_l1 / lp_norm, the results dict has
the reference's keys, and its standard deviation is numpy's population form."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = [(2, 12, 20), (2, 15, 23), (3, 12, 20), (3, 15, 23)]       # (channels, Hg, Wg); the predictions are 12 x 20


@pytest.mark.parametrize("C,hg,wg", CASES)
def test_restatement_reproduces_the_recorded_reference_values(C, hg, wg):
    """The fixtures hold inputs and the ten values the reference's functions returned for them (float32 tensors, numpy norms).
    The restatement runs the same float32 torch operators: equal to the last bits that the summation order leaves open."""
    from understanding_flow_robustness_amd import global_eval as ge
    z = np.load(os.path.join(GOLDEN, f"global_eval_validate_c{C}_{hg}x{wg}.npz"))
    assert z["gt"].shape == (1, C, hg, wg) and z["pred_clean"].shape == (1, 2, 12, 20) and z["noise0"].shape == (12, 20, 3)
    got = ge.validate_rows([z["noise0"]], [z["noise1"]], [z["pred_clean"][0]], [z["pred_adv"][0]], [z["gt"][0]])
    want = z["expected"]
    assert got.shape == (1, 10) and want.shape == (10,) and np.isfinite(want).all() and np.isfinite(got).all()
    err = np.abs(got[0] - want)
    print(f"C = {C}, {hg}x{wg}: restatement against the recorded values, |difference| = {err.tolist()}")
    assert (err <= 1e-6 * np.abs(want)).all(), (got[0].tolist(), want.tolist())
    assert (got[0, :4] == want[:4]).all(), "the norms are numpy on the same arrays: exactly equal"
    # the fixtures discriminate: the attacked prediction is another one, and the L1 is not the valid-weighted one
    assert abs(want[4] - want[5]) > 1e-3 and abs(want[6] - want[7]) > 1e-3 and abs(want[8] - want[9]) > 1e-3


def test_l1_is_the_unweighted_mean_and_skips_nan():
    from understanding_flow_robustness_amd import global_eval as ge
    g = torch.Generator().manual_seed(3)
    pred = torch.randn(1, 2, 6, 8, generator=g)
    gt = torch.cat((torch.randn(1, 2, 6, 8, generator=g) * 4.0, (torch.rand(1, 1, 6, 8, generator=g) > 0.5).float()), 1)
    gt[0, 0, 2, 3] = float("nan")
    diff = (pred - gt[:, :2]).abs()
    keep = ~torch.isnan(diff)
    want = float(diff[keep].mean() * gt[:, 2].sum() / (gt[:, 2].sum() + 1e-8))
    weighted = float((torch.nan_to_num(diff).sum(1) * gt[:, 2]).sum() / (2 * gt[:, 2].sum()))
    got = ge.compute_l1(gt=gt, pred=pred)
    assert np.isfinite(got) and abs(got - want) <= 1e-6 * abs(want) and abs(got - weighted) > 1e-3
    assert np.isnan(ge.compute_epe(gt=gt, pred=pred))                          # the end-point error keeps the NaN


def test_results_dict_has_the_reference_keys_and_population_std(tmp_path):
    from understanding_flow_robustness_amd import global_eval as ge
    per_item = np.random.RandomState(0).rand(5, 10)
    d = ge.results_dict(per_item)
    assert list(d) == ["noise0", "noise1", "flow"]
    assert list(d["noise0"]) == list(d["noise1"]) == ["L0_Pixel", "L1_Pixel"]
    assert list(d["flow"]) == ["Unattacked", "Attacked"]
    keys = ["EPE_mean", "EPE_std", "L1_mean", "L1_std", "CosSim_mean", "CosSim_std"]
    assert list(d["flow"]["Unattacked"]) == list(d["flow"]["Attacked"]) == keys
    col = {n: per_item[:, i] for i, n in enumerate(ge.NAMES)}
    assert ge.NAMES == ["noise0_L0", "noise0_L1", "noise1_L0", "noise1_L1", "epe_clean", "epe_adv", "l1_clean", "l1_adv",
                        "cossim_clean", "cossim_adv"]
    assert d["noise0"]["L0_Pixel"] == col["noise0_L0"].mean() and d["noise1"]["L1_Pixel"] == col["noise1_L1"].mean()
    for side, (epe, l1, cos) in (("Unattacked", ("epe_clean", "l1_clean", "cossim_clean")), ("Attacked", ("epe_adv", "l1_adv", "cossim_adv"))):
        for key, name in (("EPE", epe), ("L1", l1), ("CosSim", cos)):
            x = col[name]
            assert d["flow"][side][key + "_mean"] == x.mean()
            population = np.sqrt(((x - x.mean()) ** 2).sum() / len(x))
            sample = np.sqrt(((x - x.mean()) ** 2).sum() / (len(x) - 1))
            assert abs(d["flow"][side][key + "_std"] - population) <= 1e-15 and abs(d["flow"][side][key + "_std"] - sample) > 1e-3
    res = ge.GlobalEvalResult(per_item, list(ge.NAMES), d)
    path = res.write_json(str(tmp_path), 7)
    assert os.path.basename(path) == "results7.json"
    with open(path) as f:
        back = json.load(f)
    assert back["flow"]["Attacked"]["EPE_std"] == d["flow"]["Attacked"]["EPE_std"] and list(back) == list(d)


def test_out_of_scope_flags_are_refused():
    from argparse import Namespace

    from understanding_flow_robustness_amd import global_eval as ge
    for kw in (dict(disparity=True), dict(perturb_method="self"), dict(perturb_method="fog"), dict(write_out=True),
               dict(show_evolve=True), dict(arbitrary_gt_index="fun"), dict(return_feat_maps=True)):
        with pytest.raises(NotImplementedError):
            ge.refuse_out_of_scope(Namespace(flownet="FlowNetC", **kw))
    ge.refuse_out_of_scope(Namespace(flownet="FlowNetC", perturb_method="ifgsm", arbitrary_gt_index=3))
    with pytest.raises(ValueError):
        ge.evaluate_perturbation(None, [], Namespace(flownet="FlowNetC"))       # neither an attack nor a fixed noise
