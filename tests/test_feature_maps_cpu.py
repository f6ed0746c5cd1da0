"""CPU suite of the feature-map analyses (feature_maps.py, flownets/utils_model.py): the key lists, the torch spelling's capture
and overwriting against fixtures the reference's own `predict_flow` / `setup_hooks` wrote (tests/golden/
make_golden_feature_maps.py), the maximum mean discrepancy, the refusals, and the argument validation of the statistics entries
(csrc/feature_stats.hip), which precedes every HIP call.

The product has no CPU correlation (tests/test_cabi_cpu.py::test_no_cpu_fallback), so the torch spelling runs here with the
oracle's in its place (`flownetc.correlate` patched for the test): everything else -- which map is recorded where, what an
overwritten key feeds -- is the product's."""
import ctypes
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from closeness import assert_close
from conftest import GOLDEN, load_golden, t

KEY_SETS = {"conv3ab": ("conv3a", "conv3b"), "corr": ("corr",), "conv_redir": ("conv_redir",), "conv3_1": ("conv3_1",),
            "conv3a_alone": ("conv3a",), "conv4": ("conv4",)}
BLOCK = (20, 40, 50, 70, 0.5)


def frames(seed, B=1, hw=(64, 128)):
    """make_golden_feature_maps.frames."""
    g = torch.Generator().manual_seed(int(seed))
    x1, x2 = torch.rand(B, 3, *hw, generator=g), torch.rand(B, 3, *hw, generator=g)
    y0, y1, c0, c1, v = BLOCK
    p1, p2 = x1.clone(), x2.clone()
    p1[:, :, y0:y1, c0:c1] = v
    p2[:, :, y0:y1, c0:c1] = v
    return (x1, x2), (p1, p2)


def golden_flownetc():
    z = {}
    for tag in "abcd":
        z.update(load_golden(f"feature_maps_flownetc_64x128_{tag}"))
    return z, load_golden("feature_maps_flownetc_64x128_donor")


def golden_flex():
    z = {}
    for tag in "abc":
        z.update(load_golden(f"feature_maps_flex_k3r3_64x128_{tag}"))
    return z


def fetch(name, seed=0):
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    net = fetch_model(Namespace(flownet=name), synthetic_seed=seed)
    for p in net.parameters():
        p.requires_grad_(False)
    return net


@pytest.fixture()
def cpu_correlation(oracle, monkeypatch):
    from oracle import flow_oracle as fo
    from understanding_flow_robustness_amd.flownets import flownetc
    monkeypatch.setattr(flownetc, "correlate", lambda a, b, band=None: fo.correlate(a, b))


def test_key_lists_equal_the_references():
    from understanding_flow_robustness_amd.flownets import utils_model as um
    with open(os.path.join(GOLDEN, "feature_map_keys.json")) as f:
        want = json.load(f)
    assert len(want["FlowNetC"]) == 28
    for name, keys in want.items():
        assert um.get_feature_map_keys(Namespace(flownet=name)) == keys, name
    x = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    assert np.array_equal(um.compute_feature_map(x, "mean"), x.mean(axis=(-2, -1)))


def test_torch_spelling_captures_the_references_28_maps(cpu_correlation):
    from understanding_flow_robustness_amd.flownets import utils_model as um
    from understanding_flow_robustness_amd.flownets.weights import state_dict_digest
    z, _ = golden_flownetc()
    args = Namespace(flownet="FlowNetC")
    net = fetch("FlowNetC", int(z["weight_seed"]))
    assert state_dict_digest(net.state_dict()) == float(z["weight_digest"])
    _, (p1, p2) = frames(z["seed"])
    assert float(p1.double().sum()) == float(z["p1_sum"]) and float(p2.double().sum()) == float(z["p2_sum"])
    flow, maps = um.predict_flow(net, None, p1, p2, args, return_feat_maps=True)
    assert list(maps) == um.get_feature_map_keys(args)
    assert_close(flow, t(z["flow"]), rtol=1e-5, atol_scale=1e-6, what="flow")
    for k, v in maps.items():
        assert isinstance(v, np.ndarray) and v.shape == z[k].shape, k            # numpy [C,H,W] of sample 0
        assert_close(t(v), t(z[k]), rtol=1e-5, atol_scale=1e-6, what=k)
    # device-tensor form, and a network built with return_feat_maps=True gives the same
    flow_t, maps_t = um.predict_flow(fetch_with_maps(), None, p1, p2, args, return_feat_maps=True, feat_maps_to_numpy=False)
    assert torch.equal(flow_t, flow)
    for k, v in maps_t.items():
        assert torch.is_tensor(v) and v.shape == (1,) + z[k].shape and np.array_equal(v[0].numpy(), maps[k]), k


def fetch_with_maps():
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    return fetch_model(Namespace(flownet="FlowNetC"), return_feat_maps=True, synthetic_seed=0)


def test_flex_torch_spelling_captures_the_references_maps(cpu_correlation):
    from understanding_flow_robustness_amd.flownets import utils_model as um
    z = golden_flex()
    args = Namespace(flownet="FlowNetCFlexLarger_k3_reps3")
    net = fetch(args.flownet, int(z["weight_seed"]))
    _, (p1, p2) = frames(z["seed"])
    assert float(p1.double().sum()) == float(z["p1_sum"])
    flow, maps = um.predict_flow(net, None, p1, p2, args, return_feat_maps=True)
    assert len(maps) == 28
    assert_close(flow, t(z["flow"]), rtol=1e-5, atol_scale=1e-6, what="flow")
    for k in ("conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "corr", "conv3_1", "conv6_1", "predict"):
        assert_close(t(maps[k]), t(z[k]), rtol=1e-5, atol_scale=1e-6, what=k)
    with pytest.raises(NotImplementedError, match="FlowNetC only"):
        um.predict_flow(net, None, p1, p2, args, return_feat_maps=True, overwrite_feat_maps={"corr": maps["corr"]})


def test_overwritten_flows_equal_the_references(cpu_correlation):
    """The six key sets of the fixture: the four that take effect move the flow as in the reference, a lone conv3a and conv4
    reproduce the unreplaced flow bit for bit, and the maps handed back are the computed ones."""
    from understanding_flow_robustness_amd.flownets import utils_model as um
    z, donor = golden_flownetc()
    args = Namespace(flownet="FlowNetC")
    net = fetch("FlowNetC", int(z["weight_seed"]))
    _, (p1, p2) = frames(z["seed"])
    flow, maps = um.predict_flow(net, None, p1, p2, args, return_feat_maps=True)
    for tag, keys in KEY_SETS.items():
        ow = {k: donor[k] for k in keys}                                          # numpy [C,H,W]: the reference's form
        got, got_maps = um.predict_flow(net, None, p1, p2, args, return_feat_maps=True, overwrite_feat_maps=ow)
        assert_close(got, t(z["flow_" + tag]), rtol=1e-5, atol_scale=1e-6, what=tag)
        moved = float((t(z["flow_" + tag]) - t(z["flow"])).abs().max())
        if tag in ("conv3a_alone", "conv4"):
            assert moved == 0.0 and torch.equal(got, flow), tag
        else:
            assert moved > 1e-4 and float((got - flow).abs().max()) > 0.5 * moved, tag
        for k in keys:
            assert np.array_equal(got_maps[k], maps[k]), (tag, k)                 # computed, not the overwriting value
        as_tensor = net(p1, p2, overwrite_feat_maps={k: t(v)[None] for k, v in ow.items()})     # tensors [B,C,H,W]
        assert torch.equal(as_tensor, got), tag


def test_mmd_equals_the_references():
    from understanding_flow_robustness_amd.feature_maps import maximum_mean_discrepancy
    z = load_golden("feature_maps_mmd")
    assert maximum_mean_discrepancy(z["a"], z["b"]) == pytest.approx(float(z["mmd_distinct"]), rel=1e-6)
    assert float(z["mmd_distinct"]) > 0.1
    assert maximum_mean_discrepancy(z["a"], z["a"].copy()) == pytest.approx(float(z["mmd_identical"]), abs=1e-6)
    assert np.isnan(float(z["mmd_all_rows_equal"])) and np.isnan(maximum_mean_discrepancy(z["same"], z["same"].copy()))
    assert maximum_mean_discrepancy(t(z["a"]), t(z["b"])) == maximum_mean_discrepancy(z["a"], z["b"])


def test_layer_embeddings_on_the_torch_spelling(cpu_correlation):
    from understanding_flow_robustness_amd import feature_maps as fm
    args = Namespace(flownet="FlowNetC")
    net = fetch("FlowNetC")
    pairs = [frames(s) for s in (1, 2, 3)]
    keys = ["conv1a", "corr", "conv3_1", "predict"]
    emb, mmds = fm.layer_embeddings(net, [c for c, _ in pairs], [p for _, p in pairs], args, keys)
    _, maps = fm.forward_with_maps(net, *pairs[1][1], None, keys)
    for k in keys:
        w, wo = emb[k]
        assert w.dtype == np.float64 and w.shape == wo.shape == (3, maps[k].shape[1])
        assert np.array_equal(w[1], maps[k][0].double().mean((1, 2)).numpy())
        v = fm.maximum_mean_discrepancy(w, wo)
        assert mmds[k] == (0.0 if np.isnan(v) else v)
    assert mmds["conv1a"] > 0.0


def test_replace_features_names_keys_the_model_never_reads():
    from understanding_flow_robustness_amd.feature_maps import replace_features
    net = fetch("FlowNetC")
    (x1, x2), (p1, p2) = frames(5)
    gt = torch.zeros(1, 3, 64, 128)
    with pytest.raises(ValueError, match="conv4"):
        replace_features(net, (x1, x2), (p1, p2), gt, None, ["corr", "conv4"])
    with pytest.raises(ValueError, match="conv3a and conv3b"):
        replace_features(net, (x1, x2), (p1, p2), gt, None, ["conv3a"])
    with pytest.raises(NotImplementedError, match="FlowNetC only"):
        replace_features(fetch("FlowNetCFlexLarger_k3_reps3"), (x1, x2), (p1, p2), gt, None, ["corr"])


def test_replace_features_on_the_torch_spelling(cpu_correlation):
    from understanding_flow_robustness_amd import feature_maps as fm
    from understanding_flow_robustness_amd.losses import compute_epe
    z, donor = golden_flownetc()
    net = fetch("FlowNetC", int(z["weight_seed"]))
    clean, patched = frames(z["seed"])
    gt = torch.cat((torch.randn(1, 2, 64, 128, generator=torch.Generator().manual_seed(3)), torch.ones(1, 1, 64, 128)), 1)
    mask = torch.zeros(1, 3, 64, 128)
    mask[:, :, 20:40, 50:70] = 1.0
    r = fm.replace_features(net, clean, patched, gt, mask, ["conv3a", "conv3b"], Namespace(flownet="FlowNetC"))
    assert_close(r["adv_flow"], t(z["flow_conv3ab"]), rtol=1e-5, atol_scale=1e-6, what="replaced flow")
    blended = gt.clone()
    blended[:, :2, 20:40, 50:70] = 0.0                                            # the patch's zero motion, valid
    assert r["adv_epe"] == pytest.approx(compute_epe(blended, r["adv_flow"]), rel=1e-6)
    assert r["epe"] != r["adv_epe"] and -1.0 <= r["cos_sim"] <= 1.0 and -1.0 <= r["adv_cos_sim"] <= 1.0


@pytest.mark.parametrize("name", ["FlowNetS", "PWCNet", "RAFT", "FlowNet2"])
def test_unserved_networks_say_what_is_served(name):
    from understanding_flow_robustness_amd import feature_maps as fm
    from understanding_flow_robustness_amd.flownets import utils_model as um
    args = Namespace(flownet=name)
    x = torch.zeros(1, 3, 64, 64)
    for call in (lambda: um.get_feature_map_keys(args), lambda: um.predict_flow(torch.nn.Identity(), None, x, x, args, return_feat_maps=True),
                 lambda: fm.feature_means(torch.nn.Identity(), x, x, args), lambda: fm.layer_embeddings(None, [], [], args)):
        with pytest.raises(NotImplementedError, match="FlowNetC and the Robust FlowNetC family"):
            call()


def _seg(L, **kw):
    base = dict(src=4096, plane_stride=13 * 2 * 48 * 160 * 32, pixels=48 * 160, kind=0, images=2, image0=0, B=2, chunk0=0,
                channels=13 * 32, unleaky=0.0, out_col=0)
    base.update(kw)
    s = L.FeatureStatsSeg()
    for k, v in base.items():
        setattr(s, k, v)
    return s


def test_statistics_entries_refuse_bad_arguments_before_any_launch():
    """Validation precedes every HIP call, so this runs without a GPU; the pointers are never dereferenced."""
    from understanding_flow_robustness_amd import _lib as L
    lib = L.lib()
    p = ctypes.c_void_p(4096)

    def call(seg, ws=p, ws_elems=1 << 40, out=p, rows=2, cols=416, stride=416, n=1):
        arr = (L.FeatureStatsSeg * 1)(seg)
        return lib.ufr_feature_stats(arr, n, ws, ws_elems, out, rows, cols, stride, None)

    def refused(match, *a, **kw):
        assert call(*a, **kw) == -1
        assert match in lib.ufr_last_error(), lib.ufr_last_error()

    assert lib.ufr_feature_stats(None, 1, p, 8, p, 1, 1, 1, None) == -1 and b"null pointer" in lib.ufr_last_error()
    refused(b"null pointer", _seg(L), ws=None)
    refused(b"null pointer", _seg(L), out=None)
    refused(b"null pointer", _seg(L, src=None))
    refused(b"segments", _seg(L), n=0)
    refused(b"segments", _seg(L), n=33)
    refused(b"kind", _seg(L, kind=2))
    refused(b"bad shape", _seg(L, pixels=0))
    refused(b"bad shape", _seg(L, chunk0=-1))
    refused(b"leave the planes operand (13 chunks per plane)", _seg(L, channels=14 * 32))
    refused(b"leave the planes operand (13 chunks per plane)", _seg(L, chunk0=3, channels=11 * 32))
    refused(b"leave the planes operand", _seg(L, chunk0=12, channels=33))          # a 2nd chunk for one more lane
    refused(b"leave its buffer of 2 images", _seg(L, image0=1))
    refused(b"16-byte aligned", _seg(L, src=4100))
    refused(b"unleaky", _seg(L, unleaky=-0.1))
    refused(b"unleaky", _seg(L, unleaky=float("nan")))
    refused(b"leave the tensor (2 channels)", _seg(L, kind=1, plane_stride=2 * 2 * 48 * 160, chunk0=1, channels=2))
    refused(b"rows", _seg(L), rows=1)
    refused(b"leave the result matrix (416 columns)", _seg(L, out_col=1))
    refused(b"leave the result matrix", _seg(L), cols=415, stride=415)
    refused(b"row stride", _seg(L), stride=400)
    refused(b"column", _seg(L, out_col=-1))
    need = 2 * 13 * 4 * 32                                                        # images x chunks x slabs(7680 px) x lanes
    arr = (L.FeatureStatsSeg * 1)(_seg(L))
    assert lib.ufr_feature_stats_workspace_doubles(arr, 1) == need
    refused(b"workspace", _seg(L), ws_elems=need - 1)
    assert lib.ufr_feature_stats_workspace_doubles(None, 1) == -1
    assert lib.ufr_feature_stats_workspace_doubles((L.FeatureStatsSeg * 1)(_seg(L, channels=14 * 32)), 1) == -1
    flow = (L.FeatureStatsSeg * 1)(_seg(L, kind=1, plane_stride=2 * 2 * 48 * 160, channels=2))
    assert lib.ufr_feature_stats_workspace_doubles(flow, 1) == 2 * 2 * 4
