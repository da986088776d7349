"""CPU side of the mixed column statistics: the membership matrices of NNM
and Bucketing describe what ``_pre_aggregate`` computes, ``PreAggregated``
off the device is the plain composition, and the ``mix=`` overload of the
binding refuses CPU tensors."""
import asyncio
import random

import pytest
import torch

from byzpy_amd import aggregators as A
from byzpy_amd import hip, run_operator
from byzpy_amd.graph.pool import ActorPoolConfig
from byzpy_amd.hip import dispatch as D
from byzpy_amd.pre_aggregators import Bucketing, NearestNeighborMixing

X = torch.randn(11, 37, generator=torch.Generator().manual_seed(0))
X += torch.arange(11.0)[:, None]


@pytest.mark.parametrize(
    "make,counts",
    [
        (lambda: NearestNeighborMixing(3), [8] * 11),
        (lambda: Bucketing(4, perm=[5, 0, 9, 2, 7, 10, 1, 3, 8, 6, 4]), [4, 4, 3]),
        (lambda: Bucketing(3, rng=random.Random(7)), [3, 3, 3, 2]),  # drawn
    ],
)
def test_membership_describes_the_pre_aggregation(make, counts):
    mix = make().membership(X)
    assert mix.dtype == torch.uint8 and mix.shape == (len(counts), 11)
    W = mix.float()
    assert W.sum(1).tolist() == counts
    torch.testing.assert_close((W @ X) / W.sum(1, keepdim=True), make()._pre_aggregate(X))


@pytest.mark.parametrize("inner", [A.CoordinateWiseMedian(), A.CoordinateWiseTrimmedMean(2)])
def test_pre_aggregated_on_cpu_is_the_composition(inner):
    assert "PreAggregated" in A.__all__ and not A.PreAggregated.supports_subtasks
    pre = NearestNeighborMixing(3)
    agg = A.PreAggregated(pre, inner)
    want = inner._aggregate(pre._pre_aggregate(X))
    assert torch.equal(agg.aggregate(list(X)), want)
    pooled = asyncio.run(
        run_operator(
            agg,
            {"gradients": list(X)},
            pool_config=ActorPoolConfig(backend="thread", count=2),
        )
    )
    assert torch.equal(pooled, want)
    # the dispatch functions off the device: Y in f32, then the plain rule
    mixed = D.mixed_median if isinstance(inner, A.CoordinateWiseMedian) else (
        lambda X, mix: D.mixed_trimmed_mean(X, mix, 2)
    )
    torch.testing.assert_close(mixed(X, pre.membership(X)), want)


def test_mix_overload_rejects_cpu_tensors():
    with pytest.raises(RuntimeError, match="device"):
        hip.require().colsel(
            X.bfloat16(), 0, 0, mix=torch.ones(4, 11, dtype=torch.uint8)
        )
