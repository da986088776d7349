"""CPU side of the column-centred Gram (K22): the torch fallback of
``gram(X, center=True)``, the agreement of the centred and raw rules where
both resolve, and the refusals."""
import pytest
import torch

from byzpy_amd.aggregators import Bulyan, GeometricMedian, Krum, MultiKrum, PreAggregated
from byzpy_amd.hip import dispatch as D
from byzpy_amd.pre_aggregators import NearestNeighborMixing


def near_equal_rows(n, d, dtype, rel):
    g = torch.Generator().manual_seed(7)
    X = torch.randn(d, generator=g)[None, :] + rel * torch.randn(n, d, generator=g)
    return X.to(dtype)


@pytest.mark.parametrize(
    "dtype, rel, tol", [(torch.float32, 2.0**-12, 1e-3), (torch.bfloat16, 2.0**-8, 2.0**-7)]
)
def test_fallback_matches_f64_through_distances(dtype, rel, tol):
    X = near_equal_rows(17, 4099, dtype, rel)
    X[3, 11] = float("inf")
    Gc = D.gram(X, center=True).double()
    assert not torch.isfinite(Gc[3, 3])
    keep = torch.tensor([i for i in range(17) if i != 3])
    Xd = X.double()
    fin = torch.isfinite(Xd)
    Y = Xd - torch.where(fin, Xd, torch.zeros_like(Xd)).sum(0) / fin.sum(0)
    ref = D.sq_dists_from_gram(Y[keep] @ Y[keep].T)
    got = D.sq_dists_from_gram(Gc[keep][:, keep])
    off = ~torch.eye(16, dtype=torch.bool)
    assert float(((got - ref).abs()[off] / ref[off]).max()) <= tol
    # the raw Gram does not resolve these rows: that is what centring is for
    raw = D.sq_dists_from_gram(D.gram(X)[keep][:, keep].double())
    assert float(((raw - ref).abs()[off] / ref[off]).max()) > tol


@pytest.mark.parametrize(
    "make",
    [
        lambda **kw: MultiKrum(2, 3, **kw),
        lambda **kw: Krum(2, **kw),
        lambda **kw: Bulyan(1, **kw),
        lambda **kw: GeometricMedian(solver="gram", init="mean", **kw),
        lambda **kw: NearestNeighborMixing(2, **kw),
        lambda **kw: PreAggregated(
            NearestNeighborMixing(2, **kw), GeometricMedian(solver="gram", init="mean", **kw)
        ),
    ],
    ids=["multi-krum", "krum", "bulyan", "geometric-median", "nnm", "nnm+geometric-median"],
)
def test_centered_rules_agree_with_the_raw_ones_on_well_spread_rows(make):
    """On rows with no common component both Grams resolve every distance, so
    the flag must not change the answer. (That the default itself is unchanged
    is what the existing suite guards.)"""
    rows = list(torch.randn(9, 33, generator=torch.Generator().manual_seed(3)))
    run = lambda op: getattr(op, "aggregate", None) or op.pre_aggregate
    raw, centred = run(make())(rows), run(make(centered=True))(rows)
    assert torch.allclose(torch.stack(list(centred)), torch.stack(list(raw)), atol=1e-5)


def test_refusals():
    X = torch.randn(6, 16)
    with pytest.raises(ValueError):
        D.gram(list(X), center=True)
    with pytest.raises(ValueError):
        D.geometric_median(X, solver="gram", init="median", centered=True)
    with pytest.raises(ValueError):
        D.geometric_median(X, solver="gram", init="mean", init_z=X[0], centered=True)
    with pytest.raises(ValueError):
        D.geometric_median(X, centered=True)
    with pytest.raises(ValueError):
        D.centered_clipping(X, c_tau=1.0, solver="gram", centered=True)
    with pytest.raises(ValueError):
        D.caf(X, 1, solver="gram", centered=True)
    with pytest.raises(ValueError):
        GeometricMedian(solver="gram", init="median", centered=True)
    with pytest.raises(ValueError):
        GeometricMedian(init="mean", centered=True)
