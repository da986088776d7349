"""The column-centred MFMA Gram (K22, csrc/gram_centered.hip) against f64 on
the stored values, on rows that share a large common component, and the
distance rules that take it (``centered=True``) against the functional
reference on the f64-centred rows."""
import itertools

import pytest
import torch

from byzpy_amd.aggregators import Bulyan, GeometricMedian, Krum, MultiKrum, PreAggregated
from byzpy_amd.hip import dispatch as D
from byzpy_amd.ops import functional as F
from byzpy_amd.pre_aggregators import NearestNeighborMixing as NNM

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
# max |D^ - D| / D. bf16: the one rounding of y = x - mu moves a distance by
# about 2^-9 (||y_i|| + ||y_j||) ~ 2^-9 sqrt(2) ||y_i - y_j||, twice that in
# the square. f32: d 2^-24 per Gram entry, three entries, d <= 65,544.
TOL = {"f32": 1e-3, "bf16": 2.0**-7}
REL = {"f32": 2.0**-12, "bf16": 2.0**-8}
BAD = (5, 9)  # rows of the non-finite case


def near_equal_rows(n, d, dt, outliers=0, bad=False):
    """(X, Y): one N(0, 1) vector plus REL noise per row, the last ``outliers``
    rows displaced by four times that spread, as stored in dtype dt; and the
    f64 rows less the mean of each column's finite entries. ``bad`` puts +inf
    into row 5 and NaN into row 9."""
    g = torch.Generator().manual_seed(1000 * n + d)
    X = torch.randn(d, generator=g)[None, :] + REL[dt] * torch.randn(n, d, generator=g)
    if outliers:
        X[n - outliers:] += 4.0 * REL[dt] * torch.randn(outliers, d, generator=g)
    if bad:
        X[BAD[0], 17], X[BAD[1], 600] = float("inf"), float("nan")
    X = X.to(DTYPES[dt])
    Xd = X.double()
    fin = torch.isfinite(Xd)
    mu = torch.where(fin, Xd, torch.zeros_like(Xd)).sum(0) / fin.sum(0).clamp(min=1)
    return X, Xd - mu


SHAPES = list(itertools.product([1, 2, 17, 33, 64, 65, 100, 128],
                                [1, 31, 1000, 4099, 65536 + 8], [False]))


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("n, d, bad", SHAPES + [(33, 1000, True)])
def test_centred_gram_resolves_near_equal_rows(n, d, bad, dt):
    X, Y = near_equal_rows(n, d, dt, bad=bad)
    Gc = D.gram(X.cuda(), center=True).cpu()
    assert Gc.dtype == torch.float32 and Gc.shape == (n, n)
    rows = torch.tensor([i for i in range(n) if not (bad and i in BAD)])
    if bad:  # the bad rows show on the diagonal and stay in their row / column
        assert not torch.isfinite(torch.diagonal(Gc)[list(BAD)]).any()
    Gc, ref = Gc[rows][:, rows], Y[rows] @ Y[rows].T
    assert torch.isfinite(Gc).all() and torch.equal(Gc, Gc.T)
    if n > 1 and d > 1:  # through distances, off the diagonal
        off = ~torch.eye(len(rows), dtype=torch.bool)
        want = D.sq_dists_from_gram(ref)[off]
        worst = float(((D.sq_dists_from_gram(Gc.double())[off] - want).abs() / want).max())
    else:  # no meaningful distance: entry by entry, relative to max ||y||^2
        worst = float((Gc - ref).abs().max() / torch.diagonal(ref).max().clamp(min=1e-300))
    print(f"n={n} d={d} {dt} bad={bad}: worst relative error {worst:.3e} (bound {TOL[dt]:.3e})")
    assert worst <= TOL[dt]


def test_more_than_128_rows_is_refused_by_the_binding():
    from byzpy_amd import hip

    with pytest.raises(RuntimeError, match="128"):
        hip.require().gram(torch.zeros(129, 64, device="cuda"), center=True)


N, NF, Q, DIM = 17, 3, 5, 4099
GM = dict(solver="gram", init="mean", centered=True, tol=1e-9)
RULES = {
    "krum": lambda: Krum(NF, centered=True),
    "multi-krum": lambda: MultiKrum(NF, Q, centered=True),
    "bulyan": lambda: Bulyan(NF, centered=True),
    "nnm": lambda: NNM(NF, centered=True),
    "geometric-median": lambda: GeometricMedian(**GM),
    "nnm+geometric-median": lambda: PreAggregated(NNM(NF, centered=True), GeometricMedian(**GM)),
}


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(RULES))
def test_rules_on_the_centred_gram_match_the_f64_reference(name, dt):
    """The reference is the functional rule on the f64-centred rows Y, moved
    back by mu: every rule here moves with a common shift of its rows."""
    X, Y = near_equal_rows(N, DIM, dt, outliers=NF)
    Xd, mu, op = X.cuda(), (X.double() - Y)[0], RULES[name]()
    got = torch.stack(op.pre_aggregate(list(Xd))) if name == "nnm" else op.aggregate(list(Xd))
    if name in ("krum", "multi-krum", "bulyan"):  # selections: index sets
        Gc = D.gram(Xd, center=True)
        if name == "bulyan":
            want, have = F.bulyan_select(Y, NF), D.bulyan_select_from_gram(Gc, NF)
        else:
            q = 1 if name == "krum" else Q
            want = torch.topk(F.multi_krum_scores(Y, NF), k=q, largest=False).indices
            have = D.krum_winners_from_gram(Gc, NF, q)
        assert sorted(have.tolist()) == sorted(want.tolist())
        if name == "bulyan":
            # the class took those picks: its column step on them, bit for bit
            # (ties in |x - median| are the column kernel's, not under test)
            sel = want.to(torch.int32).cuda()
            assert torch.equal(got, D.mean_of_medians(Xd, 2 * NF, rows=sel))
            return
        ref = X.double()[want].mean(0)
    elif name == "nnm":
        ref = F.nnm(Y, NF).double() + mu
    else:
        mixed = F.nnm(Y, NF) if "nnm" in name else Y
        ref = F.geometric_median(mixed, init="mean", tol=1e-9).double() + mu
    # the dtype's resolution: one ulp of a bf16 output (2^-7 of its value);
    # f32 outputs carry the f32 arithmetic of the reference rule too (2^-20)
    res = 2.0**-7 if dt == "bf16" else 2.0**-20
    err = float(((got.double().cpu() - ref).abs() / ref.abs().clamp(min=1.0)).max())
    print(f"{name} {dt}: max error {err:.3e} of max(|ref|, 1) (bound {res:.3e})")
    assert err <= res
