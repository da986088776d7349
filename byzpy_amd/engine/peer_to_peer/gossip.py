"""One gossip round over resident node states.

All N node states are rows of one (N, d) matrix, so a round of
NNM + GeometricMedian(solver="gram", init="mean") for every node is three
device steps on that matrix (hip/dispatch.py, K23): one Gram, one solver
launch for all neighbourhoods, one batched combine. Any other rule runs the
per-node pre_aggregate / aggregate loop, so the function is always usable.
"""
from __future__ import annotations

from typing import Any, Optional

import torch

from byzpy_amd.aggregators import GeometricMedian
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
    out = []
    for r in rows:
        vecs = [theta[j] for j in r]
        if pre_aggregator is not None:
            vecs = pre_aggregator.pre_aggregate(vecs)
        out.append(aggregator.aggregate(vecs))
    return torch.stack(out).to(theta.dtype)
