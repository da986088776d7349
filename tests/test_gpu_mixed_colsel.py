"""Mixed column selection (K18, colsel_mix.hip): ``colsel(X, mode, f, mix=)``
and its public route ``PreAggregated`` against a plain f64 reference,
Y = (mix @ X) / mix.sum(1), columns sorted, two-middle median or trimmed mean.

Tolerance: |got - ref| <= 2^-8 |ref| + 2^-16 max|X|: one bf16 ulp of output
rounding, plus twice the worst-case f32 error of two chained sums of at most
64 terms (2 * 63 * 2^-24 max|X| ~ 2^-17 max|X|). Rows are centred at
i - n/2, so a wrong member, a dropped row or a bad pad lands far outside.

Where X holds infinities or NaNs the reference sums each y_i over exactly its
members (0 x inf in the matmul form would reach rows that are no members);
for finite X the two forms are the same numbers."""
import types

import pytest
import torch

from byzpy_amd import hip
from byzpy_amd.aggregators import (
    CoordinateWiseMedian,
    CoordinateWiseTrimmedMean,
    MeanOfMedians,
    PreAggregated,
)
from byzpy_amd.hip import dispatch as D
from byzpy_amd.pre_aggregators import Bucketing, NearestNeighborMixing

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEDIAN, TRIMMED = 0, 1
INF, NAN = float("inf"), float("nan")


def _inputs(n, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, d, generator=g) + (torch.arange(n)[:, None] - n / 2)
    return X.to(torch.bfloat16)


def _random_mix(m, n, seed=1):
    g = torch.Generator().manual_seed(seed)
    mix = (torch.rand(m, n, generator=g) < 0.5).to(torch.uint8)
    mix[torch.arange(m), torch.randint(n, (m,), generator=g)] = 1  # no empty row
    return mix


def _stat(Y, mode, f):
    S, m = Y.sort(dim=0).values, Y.shape[0]
    if mode == MEDIAN:
        return 0.5 * (S[(m - 1) // 2] + S[m // 2])
    return S[f : m - f].mean(dim=0)


def _ref(X, mix, mode, f):
    W = mix.double()
    return _stat((W @ X.double()) / W.sum(1, keepdim=True), mode, f)


def _ref_members(X, mix, mode, f):
    Xd = X.double()
    Y = torch.stack([Xd[r.bool()].sum(0) / r.sum() for r in mix])
    return _stat(Y, mode, f)


def _check(got, ref, X):
    got = got.double().cpu()
    xmax = X.double()[X.isfinite()].abs().max()
    err, tol = (got - ref).abs(), 2.0**-8 * ref.abs() + 2.0**-16 * xmax
    fin = ref.isfinite()
    worst = (err[fin] / tol[fin]).max().item() if fin.any() else 0.0
    print(f"worst error / tolerance: {worst:.3f}")
    assert (err[fin] <= tol[fin]).all(), worst
    # infinities exact, NaN where the reference has NaN
    assert torch.equal(got[~fin].nan_to_num(nan=0.0), ref[~fin].nan_to_num(nan=0.0))
    assert torch.equal(got[~fin].isnan(), ref[~fin].isnan())


def _modes(m):
    return [(MEDIAN, 0), (TRIMMED, (m - 1) // 2), (TRIMMED, 0)]


# 140_001 columns are 2,188 strips of 64: more than the 2,048 waves of the
# kernel's persistent grid on 256 CUs, so its stride wraps
@pytest.mark.parametrize("d", [1, 63, 65, 4098, 70_001, 140_001])
@pytest.mark.parametrize(
    "n,m", [(1, 1), (7, 7), (31, 5), (32, 32), (33, 33), (63, 16), (64, 32), (64, 64)]
)
def test_kernel_matches_reference_on_random_membership(n, m, d):
    X, mix = _inputs(n, d), _random_mix(m, n)
    Xd, mixd = X.to(DEV), mix.to(DEV)
    for mode, f in _modes(m):
        got = hip.require().colsel(Xd, mode, f, mix=mixd)
        assert got.dtype == torch.bfloat16 and got.shape == (d,)
        _check(got, _ref(X, mix, mode, f), X)


@pytest.mark.parametrize("bad", ["pinf", "ninf", "nan", "all"])
@pytest.mark.parametrize("n,m,d", [(64, 64, 257), (33, 33, 130)])
def test_non_finite_members_behave_like_the_gather(n, m, d, bad):
    X, mix = _inputs(n, d), _random_mix(m, n)
    if bad in ("pinf", "all"):
        X[3] = INF
    if bad in ("ninf", "all"):
        X[n - 2] = -INF
    if bad in ("nan", "all"):
        g = torch.Generator().manual_seed(2)
        X[torch.rand(n, d, generator=g) < 0.02] = NAN
    for mode, f in _modes(m):
        got = hip.require().colsel(X.to(DEV), mode, f, mix=mix.to(DEV))
        _check(got, _ref_members(X, mix, mode, f), X)


@pytest.mark.parametrize("n,m,d", [(64, 64, 257), (33, 33, 130)])
def test_rows_that_are_no_members_never_touch_the_result(n, m, d):
    X, mix = _inputs(n, d), _random_mix(m, n)
    rows = [3, 17, n - 2]
    mix[:, rows] = 0
    mix[:, 0] = 1  # keeps every row non-empty
    clean = X.clone()
    clean[rows] = 0
    X[3], X[17], X[n - 2] = INF, NAN, -INF
    for mode, f in _modes(m):
        got = hip.require().colsel(X.to(DEV), mode, f, mix=mix.to(DEV))
        assert got.isfinite().all()
        _check(got, _ref(clean, mix, mode, f), clean)


@pytest.fixture
def spied(monkeypatch):
    """Routing threshold low, and a record of the keywords of every colsel
    call that reaches the extension."""
    monkeypatch.setattr(D, "MIXED_COLSEL_FUSED_MIN_D", 1)
    monkeypatch.delenv("BYZPY_MIXED_COLSEL", raising=False)
    ext, calls = hip.require(), []
    names = {k: getattr(ext, k) for k in dir(ext) if not k.startswith("_")}
    names["colsel"] = lambda *a, **kw: (calls.append(set(kw)), ext.colsel(*a, **kw))[1]
    monkeypatch.setattr(hip, "require", lambda: types.SimpleNamespace(**names))
    return calls


@pytest.mark.parametrize("case", ["nnm-33", "nnm-64", "bucketing-63"])
def test_public_route_takes_the_fused_kernel(case, spied):
    kind, n = case.split("-")
    n, d = int(n), 2050
    X = _inputs(n, d, seed=3)
    if kind == "nnm":
        f = n // 4
        pre, inner, mode = NearestNeighborMixing(f), CoordinateWiseTrimmedMean(f), TRIMMED
    else:
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(4)).tolist()
        f = 0
        pre, inner, mode = Bucketing(4, perm=perm), CoordinateWiseMedian(), MEDIAN
    out = PreAggregated(pre, inner).aggregate([row.to(DEV) for row in X])
    assert {"mix"} in spied
    mix = pre.membership(X.to(DEV)).cpu()
    assert mix.shape == ((n, n) if kind == "nnm" else (16, n))
    _check(out, _ref(X, mix, mode, f), X)


@pytest.mark.parametrize("case", ["f32", "meamed", "cpu"])
def test_fallbacks_return_the_composition_bit_for_bit(case, spied):
    n, d, f = 33, 1026, 8
    X = _inputs(n, d, seed=5)
    X = X.float().to(DEV) if case == "f32" else X if case == "cpu" else X.to(DEV)
    pre = NearestNeighborMixing(f)
    inner = MeanOfMedians(f) if case == "meamed" else CoordinateWiseTrimmedMean(f)
    out = PreAggregated(pre, inner).aggregate(list(X))
    assert {"mix"} not in spied
    assert torch.equal(out, inner._aggregate(pre._pre_aggregate(X)))


def _rejections():
    X = torch.zeros(8, 16, dtype=torch.bfloat16, device=DEV)
    mix = torch.ones(4, 8, dtype=torch.uint8, device=DEV)
    big = torch.zeros(65, 16, dtype=torch.bfloat16, device=DEV)
    return {
        "cpu X": (X.cpu(), 0, 0, mix),
        "cpu mix": (X, 0, 0, mix.cpu()),
        "f32 X": (X.float(), 0, 0, mix),
        "int32 mix": (X, 0, 0, mix.int()),
        "1-D mix": (X, 0, 0, mix[0]),
        "strided mix": (X, 0, 0, torch.ones(8, 4, dtype=torch.uint8, device=DEV).t()),
        "mix columns != n": (X, 0, 0, mix[:, :7].contiguous()),
        "n = 65": (big, 0, 0, torch.ones(4, 65, dtype=torch.uint8, device=DEV)),
        "m = 65": (X, 0, 0, torch.ones(65, 8, dtype=torch.uint8, device=DEV)),
        "m = 0": (X, 0, 0, mix[:0]),
        "mode 2": (X, 2, 1, mix),
        "2f >= m": (X, 1, 2, mix),
        "f < 0": (X, 1, -1, mix),
    }


@pytest.mark.parametrize(
    "case",
    ["cpu X", "cpu mix", "f32 X", "int32 mix", "1-D mix", "strided mix",
     "mix columns != n", "n = 65", "m = 65", "m = 0", "mode 2", "2f >= m", "f < 0"],
)
def test_binding_rejects(case):
    X, mode, f, mix = _rejections()[case]
    with pytest.raises(RuntimeError):
        hip.require().colsel(X, mode, f, mix=mix)
