"""GPU suite of the validation (validation.py, csrc/validation.hip): the pad entry against torch on the device (bit for bit), the
metrics entry against a float32-per-pixel, float64-sum restatement and against the reference's recorded numbers, and the three
validators (`fused=True`) against the literal loop on the same device and against the CPU-reference fixtures.  Every output of an
entry is written into a NaN-filled view between sentinel guard bands, as tests/test_ops_written_gpu.py does."""
import json
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import validation_standin as S
from closeness import assert_close
from conftest import load_golden
from test_validation_cpu import REL, _same, check_against_fixture, model_items, run, standin_items

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = -1234.5
MODEL_REL = 1e-4                         # tests/test_models_gpu.py: the gate of a network's flow against its golden


def _L():
    from understanding_flow_robustness_amd import _lib as L
    return L


def _V():
    from understanding_flow_robustness_amd import validation as V
    return V


def _poisoned(shape, dtype=torch.float32, shift=0):
    """(buffer, the output view inside it): GUARD sentinels, the NaN-filled output, GUARD sentinels; `shift` elements further in,
    the view loses the 16-byte alignment of the allocation."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + shift,), SENTINEL, dtype=dtype, device=DEV)
    out = buf[GUARD + shift:GUARD + shift + n].view(shape)
    out.fill_(float("nan"))
    return buf, out


def _guards_intact(buf, out):
    start = (out.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:start] == SENTINEL).all()) and bool((buf[start + out.numel():] == SENTINEL).all()) and start >= GUARD


def _fixture(name):
    z = load_golden("validation_" + name)
    return json.loads(str(z["meta"])), z


# ------------------------------------------------------------------------------------------------------------------------ 1. pad
def _pads(h, w, mode):
    return _V().InputPadder((1, 3, h, w), mode=mode)._pad


PAD_CASES = [
    # K, H, W, the padder's mode or [left, right, top, bottom], pointers shifted by one element
    pytest.param(1, 5, 7, "sintel", False, id="5x7-sintel-rows1/2-cols0/1"),
    pytest.param(1, 5, 7, "kitti", False, id="5x7-kitti-rows0/3"),
    pytest.param(3, 16, 24, "sintel", False, id="16x24-no-pad-16-byte-loads"),
    pytest.param(2, 21, 35, "sintel", False, id="21x35-sintel"),
    pytest.param(2, 21, 35, "kitti", False, id="21x35-kitti"),
    pytest.param(2, 5, 7, "sintel", True, id="5x7-misaligned-pointers-scalar"),          # 3 * H * W % 4 != 0 and a shifted base
    pytest.param(2, 5, 7, [1, 1, 2, 0], False, id="5x7-padded-row-of-9-scalar"),
    pytest.param(2, 16, 24, [4, 4, 0, 8], False, id="16x24-left4-16-byte-loads-inside"),
    pytest.param(2, 16, 24, [3, 5, 1, 7], False, id="16x24-left3-gathered-loads"),
    pytest.param(1, 3, 2, [9, 5, 6, 7], False, id="3x2-pads-wider-than-the-frame"),
]


@pytest.mark.parametrize("divide", [False, True], ids=["plain", "div255"])
@pytest.mark.parametrize("K,h,w,pad,shifted", PAD_CASES)
def test_pad_is_bit_equal_to_torch(K, h, w, pad, shifted, divide):
    L = _L()
    left, right, top, bottom = _pads(h, w, pad) if isinstance(pad, str) else pad
    g = torch.Generator().manual_seed(100 * h + w)
    images = []
    for _ in range(2):
        whole = torch.empty(K * 3 * h * w + 1, dtype=torch.float32, device=DEV)
        view = whole[1 if shifted else 0:][:K * 3 * h * w].view(K, 3, h, w)
        view.copy_(torch.randint(0, 256, (K, 3, h, w), generator=g).float() + torch.rand(K, 3, h, w, generator=g))
        images.append(view)
    shape = (K, 3, h + top + bottom, w + left + right)
    (buf1, out1), (buf2, out2) = _poisoned(shape, shift=1 if shifted else 0), _poisoned(shape, shift=1 if shifted else 0)
    assert (out1.data_ptr() % 16 == 0) != shifted and (images[0].data_ptr() % 16 == 0) != shifted
    L.check(L.lib().ufr_validation_pad(L.ptr(images[0]), L.ptr(images[1]), L.ptr(out1), L.ptr(out2), K, h, w, top, bottom, left, right,
                                       1 if divide else 0, L.stream()), "validation pad")
    torch.cuda.synchronize()
    for image, out, buf in ((images[0], out1, buf1), (images[1], out2, buf2)):
        want = F.pad(image, [left, right, top, bottom], mode="replicate")
        if divide:
            want = want / 255.0
        assert tuple(want.shape) == shape and torch.equal(out, want)
        assert _guards_intact(buf, out), "the memory around the output was written"
    assert not torch.equal(out1, out2)


def test_the_division_is_torchs_device_rule_not_the_hosts():
    """include/ufr_hip.h: on the device `x / 255.0` is x * fl(1 / 255); a correctly rounded division differs for most values."""
    x = torch.arange(0, 256, dtype=torch.float32, device=DEV) + 0.37
    assert torch.equal(x / 255.0, x * float(np.float32(1.0) / np.float32(255.0)))
    assert int(((x / 255.0) != (x.double() / 255.0).float()).sum()) > 16


# -------------------------------------------------------------------------------------------------------------------- 2. metrics
def _sqrt32(x):
    """The correctly rounded float32 square root: float64's, rounded once more (53 >= 2 * 24 + 2 bits, so the two roundings agree
    with one).  torch's own sqrt is not this function on either device: for large tensors its CPU kernel goes through a vector
    maths library and its device kernel through the native instruction, both within one unit in the last place."""
    return np.sqrt(x.astype(np.float64)).astype(np.float32)


def _restated(pred, top, left, gt, valid, mode):
    """[K,8] float64: float32 per pixel, every operation rounded on its own (numpy float32; square root and division through
    float64, which rounds them correctly), float64 sums."""
    pred, gt = pred.cpu().numpy(), gt.cpu().numpy()
    K, _, H, W = gt.shape
    p = pred[:, :, top:top + H, left:left + W]
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == 0:
            d = p - gt
            e = _sqrt32(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])[:, None]
        else:
            d = (p if mode == 1 else p[:, :1]) - gt
            e = _sqrt32(d * d)
        assert e.dtype == np.float32
        mag = np.broadcast_to(_sqrt32(gt[:, 0] * gt[:, 0] + gt[:, 1] * gt[:, 1])[:, None], e.shape)
        val = np.broadcast_to((valid.cpu().numpy() >= 0.5 if valid is not None else np.ones((K, H, W), dtype=bool))[:, None], e.shape)
        ratio = (e.astype(np.float64) / mag.astype(np.float64)).astype(np.float32)
        out = (e > np.float32(3.0)) & (ratio > np.float32(0.05)) & val
    e64 = e.astype(np.float64)
    rows = [[e64[k].sum(), e[k].size, (e[k] < 1).sum(), (e[k] < 3).sum(), (e[k] < 5).sum(), e64[k][val[k]].sum(), val[k].sum(),
             out[k].sum()] for k in range(K)]
    return torch.tensor([[float(x) for x in r] for r in rows], dtype=torch.float64)


def _run_metrics(pred, top, left, gt, valid, mode, row0=1, extra_rows=2):
    L = _L()
    lib = L.lib()
    K, _, H, W = gt.shape
    need = lib.ufr_validation_metrics_workspace_doubles(K, H, W)
    assert need > 0
    wbuf, ws = _poisoned((need,), torch.float64)
    rows = row0 + K + extra_rows
    obuf, out = _poisoned((rows, 8), torch.float64)
    L.check(lib.ufr_validation_metrics(L.ptr(pred), L.ptr(gt), L.ptr(valid) if valid is not None else None, K, int(pred.shape[2]),
                                       int(pred.shape[3]), top, left, H, W, mode, L.ptr(ws), need, L.ptr(out), row0, rows, L.stream()),
            "validation metrics")
    torch.cuda.synchronize()
    assert _guards_intact(wbuf, ws) and _guards_intact(obuf, out)
    mine = torch.zeros(rows, dtype=torch.bool)
    mine[row0:row0 + K] = True
    assert bool(torch.isnan(out.cpu()[~mine]).all()), "a row of another chunk was written"
    return out[row0:row0 + K].cpu()


def _assert_rows(got, want, what):
    """Counts exact; sums within 1e-9 relative (a float64 sum of a million terms errs by about 1e-10); NaN where the restatement's is."""
    assert got.shape == want.shape
    for col in (1, 2, 3, 4, 6, 7):
        assert torch.equal(got[:, col], want[:, col]), (what, col, got[:, col], want[:, col])
    for col in (0, 5):
        nan = torch.isnan(want[:, col])
        assert torch.equal(torch.isnan(got[:, col]), nan), (what, col, got[:, col], want[:, col])
        if bool((~nan).any()):
            assert_close(got[:, col][~nan], want[:, col][~nan], rtol=1e-9, atol_scale=0.0, what=f"{what} column {col}")


def _metric_operands(h, w, with_valid):
    """K = 3 padded predictions, ground truths with a NaN pixel, zero-magnitude pixels and (with a mask) an item without a valid
    pixel.  The ground truth follows the prediction plus noise, so every threshold has entries on both sides."""
    K, top, left, bottom, right = 3, 2, 3, 1, 4
    g = torch.Generator().manual_seed(1000 * h + w)
    pred = torch.randn(K, 2, h + top + bottom, w + left + right, generator=g) * 20.0
    gt = pred[:, :, top:top + h, left:left + w] + torch.cat([S.noise(7 * k + h, h, w, 3.0) for k in range(K)])
    gt[0, :, 1, 2] = 0.0                                               # |gt| = 0 with an error above 3: e / 0 = inf counts
    gt[1, :, 0, 0] = 0.0
    gt[1, 0, 2, 3] = float("nan")
    valid = None
    if with_valid:
        valid = (torch.rand(K, h, w, generator=g) < 0.5).float()
        valid[0, 1, 2] = valid[1, 0, 0] = valid[1, 2, 3] = 1.0
        valid[1, 1, 1] = 0.5                                           # valid >= 0.5
        valid[0, 0, 0] = float("nan")                                  # compares false
        valid[2] = 0.0
    return pred.contiguous(), top, left, gt.contiguous(), valid


@pytest.mark.parametrize("with_valid", [False, True], ids=["no-mask", "mask"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("h,w", [(5, 7), (21, 35), (125, 187), (129, 257)])  # workgroups: 1, 3, 92, 130 > 128 (a second pixel per thread)
def test_metrics_against_the_restatement(h, w, mode, with_valid):
    pred, top, left, gt, valid = _metric_operands(h, w, with_valid)
    want = _restated(pred, top, left, gt, valid, mode)
    dev = lambda t: t.to(DEV) if t is not None else None
    got = _run_metrics(dev(pred), top, left, dev(gt), dev(valid), mode)
    _assert_rows(got, want, f"{h}x{w} mode {mode}")
    again = _run_metrics(dev(pred), top, left, dev(gt), dev(valid), mode, row0=0, extra_rows=0)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64)), "two runs differ"
    # what the cases are for
    assert bool(torch.isnan(got[1, 0])) and not bool(torch.isnan(got[0, 0])) and not bool(torch.isnan(got[2, 0]))
    assert 0 < got[0, 2] < got[0, 3] < got[0, 4] < got[0, 1]
    if with_valid:
        assert got[2, 6] == 0 and got[2, 5] == 0 and got[0, 7] > 0 and 0 < got[0, 6] < got[0, 1]


CASE_MODES = {"chairs": ("chairs", 0, None), "sintel": ("sintel", 1, "sintel"), "kitti_finite": ("kitti", 0, "kitti")}


@pytest.mark.parametrize("name", list(CASE_MODES))
def test_metrics_reproduce_the_references_recorded_numbers(name):
    """The stand-in's predictions of the fixture's items (closed form, rebuilt on the CPU) through the entry: the reference's means
    within 5e-6, its counts -- from the recorded per-item arrays -- exactly."""
    meta, z = _fixture("standin_" + name)
    validator, flowNetC, model, items = standin_items(name)
    key, mode, pad_mode = CASE_MODES[name]
    sets = items if isinstance(items, dict) else {key: items}
    for set_name, its in sets.items():
        totals = np.zeros(8)
        for image1, image2, flow_gt, valid in its:
            left, right, top, bottom = _V().InputPadder(image1.shape, mode=pad_mode)._pad if pad_mode else (0, 0, 0, 0)
            a, b = (F.pad(x, [left, right, top, bottom], mode="replicate") for x in (image1, image2))
            pred = model(a, b, test_mode=True)[1]
            row = _run_metrics(pred.to(DEV).contiguous(), top, left, flow_gt.to(DEV).contiguous(),
                               valid.to(DEV).contiguous() if name == "kitti_finite" else None, mode)
            totals += row[0].numpy()
        recorded = z["kitti_entries"] if name == "kitti_finite" else z["entries_" + set_name]
        assert totals[1] == recorded.size == meta["entries"][set_name if name != "kitti_finite" else "kitti"]
        assert [int(totals[2]), int(totals[3]), int(totals[4])] == [int((recorded < px).sum()) for px in (1, 3, 5)]
        assert _same(totals[0] / totals[1], float(np.mean(recorded.astype(np.float64))), 1e-6)
        if name == "kitti_finite":
            assert int(totals[6]) == sum(meta["valid_counts"]) and int(totals[7]) == sum(meta["outlier_counts"])
            assert _same(100.0 * totals[7] / totals[6], meta["results"]["kitti-f1"], REL)
        else:
            assert _same(totals[0] / totals[1], meta["results"][set_name], REL)


# ------------------------------------------------------------------------------------------------------------- 3. the validators
def _compare(fused, literal, rel, slack=0):
    """Keys and order equal; means within `rel`; every count equal, or within `slack` entries."""
    assert list(fused) == list(literal) and set(fused.details) == set(literal.details)
    for key in literal:
        g, w = float(fused[key]), float(literal[key])
        moved = 100.0 * slack / literal.details["kitti"]["valid"] if key == "kitti-f1" else 0.0
        assert _same(g, w, rel) or abs(g - w) <= moved, (key, g, w)
        assert type(fused[key]) is type(literal[key]), (key, type(fused[key]), type(literal[key]))
    for key, rates in literal.details.items():
        n = rates["entries"]
        assert fused.details[key]["entries"] == n
        for name in ("1px", "3px", "5px"):
            g, w = fused.details[key][name] * n, rates[name] * n
            assert abs(g - round(g)) < 1e-6 * n and abs(round(g) - round(w)) <= slack, (key, name, g, w)
        assert _same(float(fused.details[key]["epe"]), float(rates["epe"]), rel)
        if "epe_list" in rates:
            assert fused.details[key]["valid"] == rates["valid"] and abs(fused.details[key]["outliers"] - rates["outliers"]) <= slack
            g, w = np.asarray(fused.details[key]["epe_list"]), np.asarray(rates["epe_list"])
            assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w))
            assert np.all(np.abs(g - w)[~np.isnan(w)] <= rel * np.abs(w[~np.isnan(w)]))


def _on_device(items):
    return {k: S.to_device(v, DEV) for k, v in items.items()} if isinstance(items, dict) else S.to_device(items, DEV)


@pytest.mark.parametrize("name", [n for n in S.STANDIN_CASES if n != "kitti_fnc_all_skipped"])
def test_fused_equals_the_literal_loop_at_chunk_one_standin(name):
    """The pad is bit-equal and the forward is the same call, so the predictions are identical: every count equal, means within
    5e-6 -- and both legs reproduce the reference's recorded numbers."""
    meta, z = _fixture("standin_" + name)
    validator, flowNetC, model, items = standin_items(name)
    items = _on_device(items)
    literal, _ = run(validator, model, flowNetC, items, fused=False)
    calls = list(model.calls)
    fused, printed = run(validator, model, flowNetC, items, fused=True, chunk=1)
    assert model.calls == calls + calls and set(calls) == {1}
    _compare(fused, literal, REL)
    check_against_fixture(meta, z, fused, printed)


def test_fused_raises_like_the_reference_for_an_empty_set():
    meta, _ = _fixture("standin_kitti_fnc_all_skipped")
    validator, flowNetC, model, items = standin_items("kitti_fnc_all_skipped")
    with pytest.raises(ValueError) as e:
        run(validator, model, flowNetC, _on_device(items), fused=True)
    assert [type(e.value).__name__, str(e.value)] == meta["raises"] and model.calls == []


def test_chunks_flush_on_a_change_of_shape_and_keep_the_order():
    """Seven chairs items of three shapes at chunk 4: forwards of 4, 1 and 2 pairs.  The stand-in is pointwise, so stacking changes
    nothing: counts equal, means within 5e-6; and KITTI's per-item list is in loader order."""
    specs = [(61, 12, 20, 1.0)] * 2 + [(62, 12, 20, 1.0), (63, 12, 20, 1.0), (64, 9, 13, 1.0), (65, 16, 24, 1.0), (66, 16, 24, 1.0)]
    model = S.StandIn()
    items = S.to_device(S.standin_items(specs), DEV)
    literal, _ = run("chairs", model, False, items, fused=False)
    model.calls.clear()
    fused, _ = run("chairs", model, False, items, fused=True, chunk=4)
    assert model.calls == [4, 1, 2]
    _compare(fused, literal, REL)
    kspecs = [(71, 13, 19, 0.5), (72, 13, 19, 0.4), (73, 9, 13, 0.6), (74, 13, 19, 0.5), (75, 21, 35, 0.5), (76, 21, 35, 0.0), (77, 21, 35, 0.4)]
    model = S.StandIn(12.0)
    items = S.to_device(S.standin_items(kspecs, gain=12.0), DEV)
    literal, _ = run("kitti", model, False, items, fused=False)
    model.calls.clear()
    fused, _ = run("kitti", model, False, items, fused=True, chunk=2)
    assert model.calls == [2, 1, 1, 2, 1]
    _compare(fused, literal, REL)
    assert np.isnan(fused.details["kitti"]["epe_list"][5]) and np.isnan(fused["kitti-epe"])
    # Sintel items of different sizes: numpy refuses the ragged list at evaluate.py:341, on both legs
    ragged = {"clean": items[:3], "final": items[:2]}
    for leg in (False, True):
        with pytest.raises(ValueError, match="inhomogeneous"):
            run("sintel", model, False, ragged, fused=leg)


# ---- the real networks on the engines
@pytest.fixture(scope="module")
def nets():
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    made = {}

    def get(flowNetC):
        if flowNetC not in made:
            name, seed = ("FlowNetC", 0) if flowNetC else ("RAFT", 2)
            args = Namespace(flownet=name)
            net = fetch_model(args, synthetic_seed=seed).to(DEV).eval()
            if not flowNetC:
                # RAFT reads its iteration count from its own configuration and ignores the argument (models/raft/raft.py:126);
                # the fixture's network was built with RAFT_ITERS, in float32
                args.mixed_precision, args.iters = False, S.RAFT_ITERS
                assert net.args is args
            made[flowNetC] = net.requires_grad_(False)                 # frozen, as after a fine-tuning step's evaluation switch
        return made[flowNetC]
    return get


class _engines_only:
    """No forward inside may leave the hand-written engines for the vendor library (tests/test_models_gpu.py)."""

    def __enter__(self):
        self.before = dict(_L().VENDOR_FALLBACKS)

    def __exit__(self, *exc):
        if exc[0] is None:
            now = _L().VENDOR_FALLBACKS
            grown = {k: v - self.before.get(k, 0) for k, v in now.items() if v != self.before.get(k, 0)}
            assert not grown, f"a forward left the engines: {grown}"


def _literal_entries(validator, model, flowNetC, items):
    """The literal loop's error arrays and the largest |flow|, by the test's own batch-1 loop."""
    V = _V()
    out, top_flow = [], 0.0
    sets = items.values() if isinstance(items, dict) else [items]
    with torch.no_grad():
        for its in sets:
            for image1, image2, flow_gt, _ in its:
                padder = V.InputPadder(image1.shape, mode="kitti" if validator == "kitti" else "sintel")
                a, b = padder.pad(image1, image2) if validator != "chairs" else (image1, image2)
                flow = model(a / 255.0, b / 255.0) if flowNetC else model(a, b, iters=S.RAFT_ITERS, test_mode=True)[1]
                flow = padder.unpad(flow) if validator != "chairs" else flow
                d = flow - flow_gt
                e = d.abs() if validator == "sintel" else d.pow(2).sum(1).sqrt()
                out.append(e.reshape(-1).cpu().numpy())
                top_flow = max(top_flow, float(flow.abs().max()))
    return np.concatenate(out), top_flow


@pytest.mark.parametrize("name", list(S.MODEL_CASES))
def test_fused_with_the_networks_on_the_engines(name, nets):
    """chunk = 1 against the literal loop on the same device (identical predictions: counts equal, means within 5e-6), both against
    the CPU-reference fixture at the networks' golden gate, and chunk = 4 (every item twice, so that forwards of 4 pairs run)
    within the gate of a batched forward: means within 1e-4, counts within the number of literal-loop entries that lie within
    1e-4 of the largest |flow| of a threshold, which must stay under 0.1 % of the entries."""
    meta, z = _fixture(name)
    validator, flowNetC, items = model_items(name, z)
    items = _on_device(items)
    model = nets(flowNetC)
    with _engines_only():
        literal, _ = run(validator, model, flowNetC, items, fused=False)
        fused, printed = run(validator, model, flowNetC, items, fused=True, chunk=1)
        _compare(fused, literal, REL)
        slack = {k: v["0.001"] for k, v in meta["near"].items()}
        check_against_fixture(meta, z, fused, printed, rel=MODEL_REL, slack=slack)
        twice = {k: v + v for k, v in items.items()} if isinstance(items, dict) else items + items
        literal2, _ = run(validator, model, flowNetC, twice, fused=False)
        fused4, _ = run(validator, model, flowNetC, twice, fused=True, chunk=4)
        entries, top_flow = _literal_entries(validator, model, flowNetC, twice)
    band = MODEL_REL * top_flow * (1.0 if validator == "sintel" else 2.0 ** 0.5)
    near = int(sum(np.count_nonzero(np.abs(entries - th) <= band) for th in (1.0, 3.0, 5.0)))
    print(f"{name}: {near} of {entries.size} entries within {band:.2e} of a threshold (largest |flow| {top_flow:.3f})")
    assert near <= 1e-3 * entries.size
    _compare(fused4, literal2, MODEL_REL, slack=near)
