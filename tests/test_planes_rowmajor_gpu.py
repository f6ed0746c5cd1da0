"""`Planes.load_rowmajor` (igemm.py) on a matrix of ONE column: such a view has no column stride to speak of -- torch keeps
whatever the view had, e.g. (1, 256) after `.t().contiguous()` of a [1,256] row -- and only the row stride reaches the kernel.  The
dense adjoint of AlternateCorrBlock (flownets/raft_corr.py) loads such a matrix for a 1 x 1 pyramid level (64 x 96 frames)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _loaded(src):
    from understanding_flow_robustness_amd import igemm as ig
    planes = ig.Planes(1, 1, src.shape[0], 1, DEV).load_rowmajor(src)
    torch.cuda.synchronize()
    return planes.t


def test_a_single_column_loads_whatever_its_column_stride():
    g = torch.Generator().manual_seed(3)
    values = torch.randn(256, generator=g).to(DEV)
    plain = values.clone().view(256, 1)
    assert plain.stride() == (1, 1)
    want = _loaded(plain)
    total = want[0].float() + want[1].float() + want[2].float()              # [chunks, M, 32]: the three planes add up exactly
    assert torch.equal(total[0, :, 0], values) and not bool(total[0, :, 1:].any())
    wide = torch.zeros(256, 4, device=DEV)
    wide[:, 0] = values
    for view in (torch.as_strided(values, (256, 1), (1, 256)),                # what `.t().contiguous()` of a row leaves
                 values.view(1, 256).t().contiguous(),
                 wide[:, ::4],                                                # strides (4, 4)
                 wide[:, :1]):                                                # strides (4, 1)
        assert tuple(view.shape) == (256, 1)
        assert torch.equal(_loaded(view).view(torch.int16), want.view(torch.int16)), view.stride()


def test_a_strided_matrix_of_several_columns_is_still_refused():
    wide = torch.zeros(256, 4, device=DEV)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        _loaded(wide[:, ::2])                                                 # [256, 2] with strides (4, 2)
