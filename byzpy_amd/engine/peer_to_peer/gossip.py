"""One gossip round over resident node states.

All N node states are rows of one (N, d) matrix, so a round of
NNM + GeometricMedian(solver="gram", init="mean") for every node is three
device steps on that matrix (hip/dispatch.py, K23): one Gram, one solver
launch for all neighbourhoods, one batched combine. The coordinate-wise rules
(CoordinateWiseMedian, CoordinateWiseTrimmedMean, MeanOfMedians) without a
pre-aggregator have a one-step route (K24): every node's statistic in one pass
over the matrix, each row read once. On the device it is taken only for the
(dtype, rule, neighbourhood size) regions where it measured faster than the
per-node loop (_GROUPED_FASTER below); on CPU tensors the two are the same
computation. Any other rule, and any rule behind a pre-aggregator that has no
fused route, runs the per-node pre_aggregate / aggregate loop, so the function
is always usable.
"""
from __future__ import annotations

from typing import Any, Optional

import torch

from byzpy_amd.aggregators import (
    CoordinateWiseMedian,
    CoordinateWiseTrimmedMean,
    GeometricMedian,
    MeanOfMedians,
)
from byzpy_amd.hip import dispatch as D
from byzpy_amd.pre_aggregators import NearestNeighborMixing


def _fused_rule(aggregator: Any, pre_aggregator: Any) -> bool:
    """GeometricMedian(solver="gram", init="mean") alone or after a plain
    NearestNeighborMixing(f): exactly, not subclasses with other maths."""
    if type(aggregator) is not GeometricMedian:
        return False
    if aggregator.solver != "gram" or aggregator.init != "mean":
        return False
    if pre_aggregator is None:
        return True
    return type(pre_aggregator) is NearestNeighborMixing and not pre_aggregator.centered


# Neighbourhood sizes (inclusive ranges) at which the grouped kernel measured
# faster on MI355X than the per-node loop by more than the run-to-run spread
# (benchmarks/RESULTS_MI355X_gossip_colsel.md: m = 5, 17 and 32 were measured).
# A range never leaves the network width (m padded to 8 / 32) of the size it
# was measured at, and within a width the kernel's cost is flat while the
# loop's grows with m. Everything else (sizes never measured included) keeps
# the loop: the kernel sorts one f32 column per lane, the loop's bf16 kernels
# two packed columns, and the loop's repeated row reads mostly hit the cache.
_GROUPED_FASTER = {
    (torch.float32, CoordinateWiseMedian): ((5, 8), (17, 32)),
    (torch.float32, CoordinateWiseTrimmedMean): ((5, 8), (32, 32)),
    (torch.float32, MeanOfMedians): ((5, 8),),
    (torch.bfloat16, CoordinateWiseMedian): ((5, 8),),
}


def _grouped_rule(aggregator: Any, rows, theta: torch.Tensor) -> Optional[Any]:
    """The grouped dispatch call of a coordinate-wise rule (exactly these
    classes, not subclasses with other maths) as a function of (theta,
    groups), if every neighbourhood is legal for its f and, on the device,
    their sizes lie in one range of _GROUPED_FASTER; else None."""
    sizes = [len(r) for r in rows]
    lo, hi = min(sizes), max(sizes)
    kind = type(aggregator)
    if theta.is_cuda and not any(
        a <= lo and hi <= b for a, b in _GROUPED_FASTER.get((theta.dtype, kind), ())
    ):
        return None
    if kind is CoordinateWiseMedian:
        return lambda theta, groups: D.median(theta, groups=groups)
    if kind is CoordinateWiseTrimmedMean and 2 * aggregator.f < lo:
        return lambda theta, groups: D.trimmed_mean(theta, aggregator.f, groups=groups)
    if kind is MeanOfMedians and aggregator.f < lo:
        return lambda theta, groups: D.mean_of_medians(theta, aggregator.f, groups=groups)
    return None


def gossip_round(
    theta: torch.Tensor,
    topology: Any,
    aggregator: Any,
    pre_aggregator: Optional[Any] = None,
) -> torch.Tensor:
    """The states after one round: row i is the rule over
    ``theta[[i] + topology.in_neighbors(i)]``, for the ``topology.n`` nodes.
    ``theta`` is (N, d) with N >= topology.n; rows past topology.n (Byzantine
    vectors, say) are aggregated only where the topology lists them."""
    if theta.dim() != 2 or theta.shape[0] < topology.n:
        raise ValueError("theta must be (N, d) with N >= topology.n")
    rows = [[i] + list(topology.in_neighbors(i)) for i in range(topology.n)]
    if _fused_rule(aggregator, pre_aggregator):
        m = max(len(r) for r in rows)
        f = None if pre_aggregator is None else pre_aggregator.f
        if f is None or (f < m and all(len(r) - f >= 1 for r in rows)):
            return D.gossip_geometric_median(
                theta, D.gossip_groups(rows, theta.device), nnm_f=f,
                fixed_iters=aggregator.fixed_iters, tol=aggregator.tol,
                max_iter=aggregator.max_iter, eps=aggregator.eps,
                centered=aggregator.centered,
            )
    grouped = _grouped_rule(aggregator, rows, theta) if pre_aggregator is None else None
    if grouped is not None:
        return grouped(theta, D.gossip_groups(rows, theta.device)).to(theta.dtype)
    out = []
    for r in rows:
        vecs = [theta[j] for j in r]
        if pre_aggregator is not None:
            vecs = pre_aggregator.pre_aggregate(vecs)
        out.append(aggregator.aggregate(vecs))
    return torch.stack(out).to(theta.dtype)
