"""The exact-arithmetic colsel checker (tests/_colsel_exact.py) checked on
the CPU: the torch oracle has to be accepted in every column at the derived
tolerances, and every off-by-one mutant of the three statistics has to be
rejected on the `distinct` family. Without the second half a checker that
accepts everything would pass for a test."""
import pytest
import torch

import _colsel_exact as CE
from byzpy_amd.ops import functional as F

D = 512
NS = [1, 2, 3, 5, 8, 9, 16, 17, 33, 64, 100, 257, 1000]
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]


def _oracle(X, mode, f):
    if mode == CE.MEDIAN:
        return F.median(X)
    if mode == CE.TRIMMED:
        return F.trimmed_mean(X, f)
    return F.mean_of_medians(X, f)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", NS)
def test_inputs_are_exact_integers_in_range(n, dtype):
    bound = 1024 if dtype == torch.float32 else (255 if n <= 255 else 2 ** 14)
    for family in CE.FAMILIES:
        X = CE.make(family, n, 64, dtype, seed=n)
        Xd = X.double()
        assert X.shape == (n, 64) and X.dtype == dtype
        assert torch.equal(Xd, Xd.round()) and float(Xd.abs().max()) <= bound
        assert n * float(Xd.abs().max()) <= 2 ** 24  # partial sums exact in f32
        if family == "distinct":
            s = Xd.sort(dim=0).values
            assert bool((s[1:] > s[:-1]).all())
        if family == "balanced":
            c = Xd.sort(dim=0).values
            centre = c + c.flip(0)  # 2c in every row if symmetric
            assert bool((centre == centre[:1]).all())
            assert float(centre.abs().max()) <= 4


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", NS)
def test_oracle_accepted_in_every_column(n, dtype):
    for family in CE.FAMILIES:
        X = CE.make(family, n, D, dtype, seed=100 + n)
        ex = CE.Exact(X)
        for mode in CE.MODES:
            for f in CE.f_values(n, mode):
                CE.check(_oracle(X, mode, f), ex, mode, f, what=f"oracle {family}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [8, 33, 257])
def test_nearest_candidates_agree_with_the_dense_table(n, dtype):
    """rejected() only looks at the valid values next to the result; the
    dense table of all of them has to give the same verdicts, on results
    that are valid, near misses and far off."""
    tol = CE.TOL[dtype]
    X = CE.make("ties", n, D, dtype, seed=n)
    ex = CE.Exact(X)
    widest = 0
    for f in CE.f_values(n, CE.MEAMED):
        table = ex.valid_values(CE.MEAMED, f)
        widest = max(widest, table.shape[0])
        got = _oracle(X, CE.MEAMED, f)
        for shift in (0.0, 0.3 / (n - f), -1.0 / (n - f), 7.0):
            g = (got.double() + shift).to(dtype)
            dense_ok = ((g.double()[None] - table).abs() <= tol * table.abs()).any(dim=0)
            assert torch.equal(~dense_ok, ex.rejected(g, CE.MEAMED, f)), (f, shift)
    assert widest > 2  # the set really has several members on this family


def _mutants(ex, mode, f):
    """(name, float64 value) of every off-by-one variant that exists at
    this (n, f), built from the float64 sort."""
    n, s = ex.n, ex.s
    out = []
    if mode == CE.MEDIAN:
        lo, hi = (n - 1) // 2, n // 2
        if hi + 1 < n:
            out.append(("rank+1", 0.5 * (s[lo + 1] + s[hi + 1])))
        if lo >= 1:
            out.append(("rank-1", 0.5 * (s[lo - 1] + s[hi - 1])))
    elif mode == CE.TRIMMED:
        k = n - 2 * f
        if f >= 1:
            out.append(("shift+1", s[f + 1:n - f + 1].mean(dim=0)))
            out.append(("shift-1", s[f - 1:n - f - 1].mean(dim=0)))
            out.append(("wide", s[f - 1:n - f + 1].mean(dim=0)))
            out.append(("swap-left", (s[f:n - f].sum(0) - s[f] + s[f - 1]) / k))
            out.append(("swap-right", (s[f:n - f].sum(0) - s[n - f - 1] + s[n - f]) / k))
        if k >= 3:
            out.append(("narrow", s[f + 1:n - f - 1].mean(dim=0)))
    else:
        k = n - f
        if f + 1 < n:
            out.append(("f+1", ex.valid_values(mode, f + 1)[0]))
        if f >= 1:
            out.append(("f-1", ex.valid_values(mode, f - 1)[0]))
            # the kept value farthest from the median swapped for the
            # nearest dropped one. (Not for even n, k = 1: the two middle
            # values are equally far from their own mean, so either is valid.)
            if not (n % 2 == 0 and k == 1):
                order = (ex.X - ex.med[None]).abs().argsort(dim=0, stable=True)
                by_dev = ex.X.gather(0, order)
                out.append(("swap", (by_dev[:k].sum(0) - by_dev[k - 1] + by_dev[k]) / k))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", NS)
def test_mutants_rejected_on_distinct(n, dtype):
    X = CE.make("distinct", n, D, dtype, seed=200 + n)
    ex = CE.Exact(X)
    seen = 0
    for mode in CE.MODES:
        for f in CE.f_values(n, mode):
            for name, value in _mutants(ex, mode, f):
                got = value.to(dtype)  # rounded as a kernel's output is
                bad = ex.rejected(got, mode, f)
                assert bool(bad.any()), (name, mode, n, f)
                seen += 1
    assert seen > 0 or n == 1


def test_balanced_alone_misses_symmetric_window_errors():
    """why `distinct` is required: on a symmetric multiset a window that is
    one too narrow or too wide on BOTH sides has the same mean"""
    X = CE.make("balanced", 33, D, torch.float32, seed=1)
    ex = CE.Exact(X)
    narrow = ex.s[5:33 - 5].mean(dim=0)
    assert not bool(ex.rejected(narrow.float(), CE.TRIMMED, 4).any())
    Xd = CE.make("distinct", 33, D, torch.float32, seed=1)
    exd = CE.Exact(Xd)
    assert bool(exd.rejected(exd.s[5:33 - 5].mean(dim=0).float(), CE.TRIMMED, 4).any())


def test_extreme_rows_keep_the_expected_value_finite():
    X = CE.make("distinct", 24, D, torch.bfloat16, seed=3)
    for kind in ("+big", "-big", "mixbig", "+inf", "-inf", "mixinf"):
        Y = CE.plant_extremes(X, 8, kind, seed=4)
        assert int((Y.float().abs() > 1e29).sum()) == 8 * D
        ex = CE.Exact(Y)
        for mode, f in ((CE.TRIMMED, 8), (CE.MEAMED, 8), (CE.MEAMED, 11)):
            v = ex.valid_values(mode, f)[0]
            assert bool(torch.isfinite(v).all()) and float(v.abs().max()) <= 255
            CE.check(_oracle(Y, mode, f), ex, mode, f, what=f"oracle {kind}")
        # and the mutant that keeps one extreme row is rejected
        leaky = ex.s[7:24 - 9].mean(dim=0).to(torch.bfloat16)
        if kind != "+big" and kind != "+inf":
            assert bool(ex.rejected(leaky, CE.TRIMMED, 8).all())
