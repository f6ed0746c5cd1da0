"""GPU suite, end to end: the patch attack's step with predict_flow6/5/4/3 on the split form and the loss on the fast launch against
the same step on the launches it ran before (the unsplit ufr_flow_head_planes_forward_mfma + ufr_flow_up_planes_forward and
ufr_flow2_upsampled_loss): patch, pasted frames, gradient rows and loss with torch.equal, first and later iteration of a call."""
from argparse import Namespace

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W, S = 2, 128, 768, 20          # the frames of tests/test_attack_glue_gpu.py: a 96-pixel window and a column band


@pytest.mark.parametrize("use_graph", [False, True])
def test_step_equals_the_step_on_the_launches_it_replaced(use_graph, monkeypatch):
    from understanding_flow_robustness_amd import _lib as L
    from understanding_flow_robustness_amd.flownets.utils_model import fetch_model
    from understanding_flow_robustness_amd.patch_attack import PatchAttackStep
    net = fetch_model(Namespace(flownet="FlowNetC"), synthetic_seed=0).to(DEV)
    for p in net.parameters():
        p.requires_grad_(False)
    g = torch.Generator().manual_seed(29)
    tgt, ref = torch.rand(B, 3, H, W, generator=g).to(DEV), torch.rand(B, 3, H, W, generator=g).to(DEV)
    target = torch.randn(B, 2, H, W, generator=g).to(DEV)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    disc = (((yy - 9.5) ** 2 + (xx - 9.5) ** 2) <= 10.0 ** 2).float().expand(1, 3, S, S).contiguous().to(DEV)
    patch0 = torch.rand(1, 3, S, S, generator=g).to(DEV)
    origins = [(0, 300), (50, 400)]

    def run(lr, iterations):
        args = Namespace(flownet="FlowNetC", l2=False, alpha=0.0, lr=lr, max_count=iterations)
        step = PatchAttackStep(net, args, B, H, W, device=DEV, patch_hw=(S, S), use_graph=use_graph, sum_groups=2)
        outs = []
        for _ in range(2):                                  # two calls: the second replays what the first captured
            step.load(tgt, ref, patch0, disc, patch0, target, origins=origins)
            n, loss = step.run(iterations)
            outs.append((step.patch.clone(), step.adv_tgt.detach().clone(), step.adv_ref.detach().clone(), step.rows_local.clone(),
                         step.eng.flow_out.clone(), n, loss))
        return step, outs

    step, probe = run(1.0, 1)
    lr = 0.25 / float(((probe[0][0] - patch0) * disc).abs().max())          # updates of a quarter: visible, unclamped
    step, new = run(lr, 3)
    eng = step.eng
    assert sorted(eng.pf_split) == [3, 4, 5, 6] and all(eng.pf_ran[k] == "split" for k in (6, 5, 4, 3)) and eng.pf_ran[2] == "mfma"
    # the launches it replaced: no level split, the reference loss launch behind the fast entry's name
    lib = L.lib()
    monkeypatch.setattr(eng, "pf_split", {})
    monkeypatch.setattr(lib, "ufr_flow2_upsampled_loss_fast", lib.ufr_flow2_upsampled_loss)
    step_old, old = run(lr, 3)
    assert step_old.eng is eng and all(eng.pf_ran[k] == "mfma" for k in (6, 5, 4, 3, 2))
    for call, (a, b) in enumerate(zip(new, old)):
        assert a[5] == b[5] == 3 and a[6] == b[6], (call, a[5:], b[5:])
        for name, x, y in zip(("patch", "first frames", "second frames", "gradient rows", "flow2"), a, b):
            assert torch.equal(x, y), (call, name)
    assert float(((new[0][0] - patch0) * disc).abs().max()) > 0.1
