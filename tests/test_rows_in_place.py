"""CPU-side contract of the in-place row lists (K19): the list overloads of
colsel / gram / mean_rows validate before they touch the device, the
eligibility helper declines what the kernels cannot read in place, and
``aggregate()`` on CPU lists is what it was."""
import numpy as np
import pytest
import torch

from byzpy_amd import hip
from byzpy_amd.aggregators import CoordinateWiseMedian, MultiKrum
from byzpy_amd.ops import functional as F
from byzpy_amd.utils.flatten import rows_in_place

IDX = torch.tensor([0, 1], dtype=torch.int32)


def _calls(rows):
    ext = hip.require()
    return [lambda: ext.colsel(rows, 0, 0), lambda: ext.gram(rows),
            lambda: ext.mean_rows(rows, IDX)]


BAD_LISTS = {
    "cpu": [torch.randn(8) for _ in range(3)],
    "mixed_dtypes": [torch.randn(8), torch.randn(8).to(torch.bfloat16)],
    "unequal_lengths": [torch.randn(8), torch.randn(9)],
    "non_contiguous": [torch.randn(8), torch.randn(16)[::2]],
    "n0": [],
    "n65": [torch.randn(8) for _ in range(65)],
}


@pytest.mark.parametrize("case", sorted(BAD_LISTS))
def test_list_overloads_validate_before_the_device(case):
    for call in _calls(BAD_LISTS[case]):
        with pytest.raises(RuntimeError):
            call()


@pytest.mark.parametrize("case", sorted(BAD_LISTS) + ["matrix", "param_lists", "ndarrays"])
def test_helper_declines(case):
    other = {
        "matrix": torch.randn(3, 8),
        "param_lists": [[torch.randn(2, 2), torch.randn(4)] for _ in range(3)],
        "ndarrays": [np.zeros(8, dtype=np.float32) for _ in range(3)],
    }
    assert rows_in_place(BAD_LISTS.get(case, other.get(case))) is None


def test_aggregate_on_cpu_lists_is_unchanged():
    grads = [torch.randn(4, 5) for _ in range(7)]
    X = torch.stack([g.reshape(-1) for g in grads])
    out = CoordinateWiseMedian().aggregate(grads)
    assert out.shape == (4, 5) and torch.equal(out.reshape(-1), F.median(X))
    out = MultiKrum(2, 3).aggregate(grads)
    assert torch.equal(out.reshape(-1), F.multi_krum(X, 2, 3))
