"""K23 on CPU tensors: F.gossip_coeffs against the per-node composition it
stands for, and gossip_round against the per-node aggregator loop, in f64."""
import pytest
import torch

from byzpy_amd.aggregators import CoordinateWiseMedian, GeometricMedian
from byzpy_amd.aggregators.pre_aggregated import PreAggregated
from byzpy_amd.engine.peer_to_peer import Topology, gossip_round
from byzpy_amd.hip import dispatch as D
from byzpy_amd.ops import functional as F
from byzpy_amd.pre_aggregators import NearestNeighborMixing

STEPS, EPS = 6, 1e-12


def _theta(n=9, d=64):
    X = torch.randn(n, d, generator=torch.Generator().manual_seed(n), dtype=torch.float64)
    X[0] *= 5.0
    return X


@pytest.mark.parametrize("f", [None, 1, 2])
def test_gossip_coeffs_equal_the_per_node_composition(f):
    X = _theta()
    G = X @ X.T
    rows = [[0, 3, 4, 8], [1, 0, 2], [5, 6, 7, 8, 2], [4, 1, 7]]
    groups = D.gossip_groups(rows)
    assert groups.dtype == torch.int32 and groups[1].tolist() == [1, 0, 2, -1, -1]
    A, steps = F.gossip_coeffs(G, groups, f, iters=STEPS, eps=EPS)
    assert steps.tolist() == [STEPS] * 4
    for i, r in enumerate(rows):
        S = G[r][:, r]
        a0 = torch.full((len(r),), 1.0 / len(r), dtype=torch.float64)
        if f is None:
            c = F.gram_fixed_point(S, a0, rule="weiszfeld", iters=STEPS, eps=EPS)[0]
        else:
            mix = NearestNeighborMixing(f).membership_from_gram(S)
            GY, W = D.mixed_gram(S, mix)
            a = F.gram_fixed_point(GY, a0, rule="weiszfeld", iters=STEPS, eps=EPS)[0]
            c = W.T @ a
        ref = torch.zeros(9, dtype=torch.float64)
        ref[r] = c
        assert (A[i] - ref).abs().max() <= 1e-12


def test_gossip_coeffs_dead_rows_and_tol_stop():
    G = (_theta() @ _theta().T).float()
    G[2, :] = G[:, 2] = float("inf")
    groups = D.gossip_groups([[0, 1, 2, 3], [2], [4, 5, 2, 6, 7]])
    A, steps = F.gossip_coeffs(G, groups, 1, iters=50, eps=EPS, tol=1e-3)
    assert bool((A[:, 2] == 0).all()) and bool(torch.isfinite(A).all())
    assert (A[[0, 2]].sum(dim=1) - 1.0).abs().max() <= 1e-12 and float(A[1].sum()) == 0.0
    assert all(1 <= int(s) < 50 for s in steps)


@pytest.mark.parametrize("f", [None, 1])
def test_gossip_round_equals_the_per_node_loop(f):
    theta, topo = _theta(), Topology.ring(8, 2)
    agg = GeometricMedian(solver="gram", init="mean", fixed_iters=STEPS, eps=EPS)
    pre = None if f is None else NearestNeighborMixing(f)
    rule = agg if pre is None else PreAggregated(pre, agg)
    got = gossip_round(theta, topo, agg, pre)
    assert got.shape == (8, 64) and got.dtype == theta.dtype
    for i in range(8):
        ref = rule.aggregate(theta[[i] + topo.in_neighbors(i)])
        assert (got[i] - ref).abs().max() <= 1e-10


def test_gossip_round_falls_back_for_other_rules(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the fused route was taken")

    monkeypatch.setattr(D, "gossip_geometric_median", refuse)
    theta, topo = _theta(), Topology.ring(8, 1)
    for agg in (CoordinateWiseMedian(), GeometricMedian(fixed_iters=STEPS)):
        got = gossip_round(theta, topo, agg, NearestNeighborMixing(1))
        for i in (0, 7):
            rows = [theta[j] for j in [i] + topo.in_neighbors(i)]
            ref = agg.aggregate(NearestNeighborMixing(1).pre_aggregate(rows))
            assert torch.equal(got[i], ref)
    with pytest.raises(ValueError):
        D.gossip_groups([[0, 1, 1]])
