"""A pre-aggregator and an aggregator as one aggregator.

The literature pairs a mixing pre-aggregator with a coordinate-wise rule:
NNM then trimmed mean (Allouah et al. 2023), Bucketing then median
(Karimireddy et al. 2022). Both pre-aggregators are row maps Y = W X with a
tiny 0/1 membership matrix W over its row counts, so on the device the pair
needs no mixed matrix Y at all: ``colsel(X, mode, f, mix=W)`` (K18,
colsel_mix.hip) rebuilds every mixed column in registers and runs the rule's
selection network on it.
"""
from __future__ import annotations

import torch

from byzpy_amd.aggregators.base import Aggregator
from byzpy_amd.aggregators.coordinate_wise import (
    CoordinateWiseMedian,
    CoordinateWiseTrimmedMean,
)
from byzpy_amd.aggregators.geometric_wise import GeometricMedian
from byzpy_amd.hip import dispatch as D


class PreAggregated(Aggregator):
    """``aggregator`` applied to the output of ``pre_aggregator``.

    A pre-aggregator with a ``membership(X)`` method (NearestNeighborMixing,
    Bucketing) in front of CoordinateWiseMedian or CoordinateWiseTrimmedMean
    takes the fused device route where ``D.mixed_colsel_fused_ok(X)``; in
    front of ``GeometricMedian(solver="gram", init="mean")`` the rule runs on
    the mixed Gram W G W^T and the coefficients pull back as W^T a, so no
    mixed matrix is formed on any device (``centered=True`` on either part
    puts that route on the column-centred Gram); everything else is
    ``aggregator._aggregate(pre_aggregator._pre_aggregate(X))``."""

    name = "pre-aggregated"
    supports_subtasks = False

    def __init__(self, pre_aggregator, aggregator: Aggregator) -> None:
        self.pre_aggregator = pre_aggregator
        self.aggregator = aggregator

    def _aggregate(self, X: torch.Tensor) -> torch.Tensor:
        pre, agg = self.pre_aggregator, self.aggregator
        if hasattr(pre, "membership") and D.mixed_colsel_fused_ok(X):
            if type(agg) is CoordinateWiseMedian:
                return D.mixed_median(X, pre.membership(X))
            if type(agg) is CoordinateWiseTrimmedMean:
                return D.mixed_trimmed_mean(X, pre.membership(X), agg.f)
        if (
            hasattr(pre, "membership")
            and type(agg) is GeometricMedian
            and agg.solver == "gram"
            and agg.init == "mean"
        ):
            # Gram of Y = W X is W G W^T and coefficients pull back as W^T a:
            # the rule runs on the mixed rows with no mixed matrix (K20).
            # ``centered=True`` on either part takes the centred Gram (K22)
            # for both: W's rows and the Weiszfeld coefficients sum to 1, so
            # W Gc W^T is the Gram of the mixed rows less the same mu, with
            # the same distances, and W^T a still combines the raw rows.
            centered = getattr(pre, "centered", False) or agg.centered
            G = D.solver_gram(X, centered)
            if hasattr(pre, "membership_from_gram"):
                mix = pre.membership_from_gram(G)
            else:
                mix = pre.membership(X)
            return D.mixed_geometric_median(
                X, mix, gram=G, tol=agg.tol, max_iter=agg.max_iter,
                eps=agg.eps, fixed_iters=agg.fixed_iters,
            )
        return agg._aggregate(pre._pre_aggregate(X))
