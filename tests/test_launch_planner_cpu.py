"""The launch planner of igemm.py (`tile_rows_and_slots`, `plan_splitk`, `LaunchQueue`) without a device: the tile table against
its literal, the plan against the inline formula the engines used to carry, the queue on CPU `Planes`, and every engine's plan at
64 x 128 against the fixture recorded before the engines moved onto the planner (tests/golden/make_launch_plans.py)."""
import importlib.util
import json
import os
import threading

import pytest
import torch

from conftest import ROOT
from understanding_flow_robustness_amd import flownetc_engine as fe
from understanding_flow_robustness_amd import igemm as ig

GOLDEN = os.path.join(ROOT, "tests", "golden")
VARIANTS = (0, 2, 4, 5, 6, 7, 8)
# (tile rows, resident workgroups) by output columns (a multiple of 128 or not) and kernel form
TABLE = {128: {0: (128, 768), 2: (128, 768), 4: (64, 1024), 5: (128, 512), 6: (256, 256), 7: (256, 256), 8: (128, 768)},
         64: {0: (128, 768), 2: (128, 768), 4: (128, 768), 5: (128, 768), 6: (128, 768), 7: (256, 256), 8: (128, 768)}}


def test_tile_table_and_the_two_flownetc_deviations():
    for N in (64, 128):
        for v in VARIANTS:
            assert ig.tile_rows_and_slots(N, v) == TABLE[N][v], (N, v)
            # FlowNetC: the tap-reuse form is sized like the single-stage tile; its window prefix: every form but 5 / 6 is
            head = (128, 768) if v == 7 else TABLE[N][v]
            window = TABLE[N][v] if v in (5, 6) else (128, 768)
            assert ig.tile_rows_and_slots(N, v, fe._TILE) == head, (N, v)
            assert ig.tile_rows_and_slots(N, v, fe._WINDOW_TILE) == window, (N, v)
    assert fe._TILE == {7: (128, 768)} and fe._PLAN["min_ktiles"] == 16
    assert ig.tile_rows_and_slots(128, 7) != (128, 768) != ig.tile_rows_and_slots(128, 4)      # (both deviate from the table)


def _weights():
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"stride-1 forward": ig.conv_forward_weights(r(256, 96, 3, 3), 1, 1),
            "stride-2 data gradient": ig.conv_backward_weights(r(256, 128, 3, 3), 2, 1),
            "deconvolution data gradient": ig.deconv_backward_weights(r(256, 128, 4, 4), 1)}


def test_plan_splitk_equals_the_inline_formula(monkeypatch):
    monkeypatch.setattr(ig, "_TUNING", {})
    W = _weights()
    assert [len(t) for _, _, t in W["stride-2 data gradient"].phases] == [1, 2, 2, 4]
    seen = set()
    for name, wi in W.items():
        for (B, Hr, Wr), v, mk in ((b, v, mk) for b in ((1, 6, 20), (1, 48, 160), (8, 48, 160)) for v in (2, 6) for mk in (4, 16)):
            M = B * Hr * Wr
            pk = [len(t) * wi.KC for _, _, t in wi.phases]
            bm, target = TABLE[128][v]
            S = ig.splitk_for(M, wi.Npad, max(pk), len(wi.phases), phase_ktiles=pk, bm=bm, target=target, min_ktiles=mk)
            kw = dict(out_planes=object(), variant=v)
            assert ig.plan_splitk(wi, M, kw, rows=(Hr, Wr), min_ktiles=mk) == (v, S), (name, M, v, mk)
            seen.add(S)
            # the RAFT update engine counts one phase; the correlation adjoints pass K as one number and a fixed tile
            S1 = ig.splitk_for(M, wi.Npad, max(pk), 1, phase_ktiles=pk, bm=bm, target=target, min_ktiles=mk)
            assert ig.plan_splitk(wi, M, kw, rows=(Hr, Wr), min_ktiles=mk, phases=1) == (v, S1)
            Sk = ig.splitk_for(M, wi.Npad, wi.KC, 1, bm=256, target=256, min_ktiles=mk)
            assert ig.plan_splitk(wi, M, kw, min_ktiles=mk, tile=(256, 256), phases=1, ktiles=wi.KC) == (v, Sk)
            assert ig.plan_splitk(wi, M, kw, min_ktiles=mk, tile={v: (64, 1024)}) == \
                (v, ig.splitk_for(M, wi.Npad, max(pk), len(wi.phases), phase_ktiles=pk, bm=64, target=1024, min_ktiles=mk))
    assert len(seen) > 2 and 1 in seen                       # (the shapes reach split and unsplit plans)
    # the tuning table: asked with tune=True only, the long form only with the row grid
    wi, kw = W["stride-1 forward"], dict(out_planes=object(), variant=6)
    rule = ig.plan_splitk(wi, 7680, kw, rows=(48, 160), min_ktiles=4)
    short, long_ = ig.launch_signature(wi, 7680, kw), ig.launch_signature(wi, 7680, kw, (48, 160))
    monkeypatch.setattr(ig, "_TUNING", {short: (4, rule[1] * 2)})
    assert ig.plan_splitk(wi, 7680, kw, rows=(48, 160), min_ktiles=4) == (4, rule[1] * 2) != rule
    assert ig.plan_splitk(wi, 7680, kw, rows=(48, 160), min_ktiles=4, tune=False) == rule
    monkeypatch.setattr(ig, "_TUNING", {short: (4, 2), long_: (8, 1)})
    assert ig.plan_splitk(wi, 7680, kw, rows=(48, 160), min_ktiles=4) == (8, 1)
    assert ig.plan_splitk(wi, 7680, kw, rows=(24, 320), min_ktiles=4) == (4, 2)
    assert ig.plan_splitk(wi, 7680, kw, min_ktiles=4) == (4, 2)
    assert ig.plan_splitk(wi, 7680, kw, rows=(48, 160), min_ktiles=4, tune=False) == rule


def test_launch_queue_on_cpu_planes(monkeypatch):
    monkeypatch.setattr(ig, "_TUNING", {})
    g = torch.Generator().manual_seed(4)
    w3 = ig.conv_forward_weights(torch.randn(128, 256, 3, 3, generator=g), 1, 1)       # 72 K tiles: splits on small grids
    w1 = ig.conv_forward_weights(torch.randn(128, 32, 1, 1, generator=g), 1, 0)        # one K tile: never splits
    grids = ((8, 16), (16, 16), (4, 8))
    order, real = [], ig.make_launch
    monkeypatch.setattr(ig, "make_launch", lambda wi, x, *a, **kw: (order.append((wi, x)), real(wi, x, *a, **kw))[1])

    def queue():
        q = ig.LaunchQueue("cpu", min_ktiles=4)
        hs = [q.add(w3, ig.Planes(1, *hw, 8, "cpu"), 0, hw, hw, out_planes=ig.Planes(1, *hw, 4, "cpu"), variant=6) for hw in grids]
        hs.append(q.add(w1, ig.Planes(1, 8, 16, 1, "cpu"), 0, (8, 16), (8, 16), out_planes=ig.Planes(1, 8, 16, 4, "cpu"), variant=6))
        return q, hs

    q, hs = queue()
    assert all(h.launch is None for h in hs)
    ws = q.build()
    need = []
    for h, hw in zip(hs[:3], grids):
        S = ig.splitk_for(hw[0] * hw[1], 128, 72, 1, phase_ktiles=[72], bm=256, target=256, min_ktiles=4)
        assert h.S == S > 1 and h.launch.desc.splitk == S and h.launch.desc.ws == ws.data_ptr()
        need.append(1 * S * 1 * hw[0] * hw[1] * 128)                                   # nphase * S * B * Hr * Wr * Npad
    assert ws.dtype == torch.float32 and ws.device.type == "cpu" and ws.numel() == max(need) and len(set(need)) == 3
    assert hs[3].S == 1 and hs[3].launch.desc.splitk == 1 and not hs[3].launch.desc.ws    # unsplit: no workspace pointer
    assert [(wi, x) for wi, x in order] == [(h.wi, h.x) for h in hs]                  # make_launch in queue order
    assert all(callable(h) and isinstance(h.launch, ig.Launch) for h in hs)            # (the handles stand in for their launches)
    # a given workspace that holds all but the largest need: that launch alone runs unsplit
    q2, hs2 = queue()
    given = torch.empty(sorted(need)[1], dtype=torch.float32)
    assert q2.build(given) is given
    big = need.index(max(need))
    for i, (h, h0) in enumerate(zip(hs2, hs)):
        assert h.S == (1 if i == big else h0.S) and h.launch.desc.splitk == h.S
        assert h.launch.desc.ws == (given.data_ptr() if h.S > 1 else None)
    q3 = ig.LaunchQueue("cpu", min_ktiles=4)
    q3.add(w1, hs[3].x, 0, (8, 16), (8, 16), out_planes=hs[3].kw["out_planes"], variant=6)
    assert q3.build().numel() == 1                                                     # nothing splits: never less than one float


with open(os.path.join(GOLDEN, "launch_plans_small.json")) as _f:
    PLANS = json.load(_f)


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("make_launch_plans", os.path.join(GOLDEN, "make_launch_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", sorted(PLANS))
def test_small_shape_plans_match_the_recorded_fixture(recorder, name):
    """Every make_launch call of the engine set `name` at 64 x 128, in call order: signature, kernel form, split-K factor, workspace
    size, balance / resident, products, chunk offsets and whether the tail plan is on."""
    got = json.loads(json.dumps(recorder.record(only=[name])[name]))
    want = PLANS[name]
    assert len(got) == len(want) > 20
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (name, i)


def test_products_stack_is_per_thread():
    seen = []
    with ig.products(1):
        t = threading.Thread(target=lambda: seen.append(ig.current_products()))
        t.start(), t.join()
        assert ig.current_products() == 1
    assert seen == [6] and ig.current_products() == 6
