"""The grouped column-selection kernel (colsel_groups.hip, K24) against exact
float64 expected values (tests/_colsel_exact.py: 2^-21 relative for f32
outputs, 2^-8 for bf16, no absolute term, valid-value sets for
mean-around-median ties, no column masked out). Shapes are the smallest at
which the kernel can go wrong: d = 1, 63 (tail lanes), 322 and 323 (more than
one strip, even and odd)."""
import pytest
import torch

import _colsel_exact as CE
from byzpy_amd import hip as _hip
from byzpy_amd.aggregators import (
    CoordinateWiseMedian,
    CoordinateWiseTrimmedMean,
    MeanOfMedians,
)
from byzpy_amd.engine.peer_to_peer import Topology, gossip_round
from byzpy_amd.hip import dispatch as D

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]


def _run(X, mode, f, **kw):
    if mode == CE.MEDIAN:
        return D.median(X, **kw)
    if mode == CE.TRIMMED:
        return D.trimmed_mean(X, f, **kw)
    return D.mean_of_medians(X, f, **kw)


def _random_rows(N, M, m, seed):
    """M lists of m distinct rows of N in random (non-monotone) order"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randperm(N, generator=g)[:m].tolist() for _ in range(M)]


def _check_nodes(X, rows, cases, what=""):
    """every (mode, f) of ``cases`` for every node, the float64 sort of a
    node's rows shared by its cases"""
    groups = D.gossip_groups(rows, X.device)
    exact = [CE.Exact(X[g]) for g in rows]
    for mode, f in cases:
        got = _run(X, mode, f, groups=groups)
        assert got.dtype == X.dtype and got.shape == (len(rows), X.shape[1])
        for i, ex in enumerate(exact):
            CE.check(got[i], ex, mode, f, what=f"{what} node {i}")


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_pad_count(dtype, m):
    rows = _random_rows(40, 6, m, seed=m)
    cases = [(mode, f) for mode in CE.MODES for f in CE.f_values(m, mode)]
    for family in CE.FAMILIES:
        X = CE.make(family, 40, 323, dtype, seed=m, device=DEV)
        _check_nodes(X, rows, cases, family)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ragged_nodes_at_the_caps(dtype):
    """N = M = 128, m_i = 1 + i % 32; node 31 reads rows 0 and 127 among its
    32, node 63 only rows >= 64"""

    def rows_of(i):
        lo = 64 if i == 63 else 0
        r = [lo + j for j in _random_rows(128 - lo, 1, 1 + i % 32, seed=i)[0]]
        return [127, 0] + [j for j in r if j not in (0, 127)][:30] if i == 31 else r

    X = CE.make("distinct", 128, 322, dtype, seed=7, device=DEV)
    _check_nodes(X, [rows_of(i) for i in range(128)], [(CE.MEDIAN, 0), (CE.TRIMMED, 0)])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize(
    "N,d,rows",
    [(9, 1, [[4, 0, 8, 2, 6]]), (12, 63, [[i, 8 + i % 4, 8 + (i + 1) % 4] for i in range(8)])],
    ids=["one-node", "rows-past-the-nodes"],
)
def test_node_count_differs_from_row_count(N, d, rows, dtype):
    X = CE.make("distinct", N, d, dtype, seed=N, device=DEV)
    _check_nodes(X, rows, [(CE.MEDIAN, 0), (CE.TRIMMED, 1), (CE.MEAMED, 1)])


@pytest.mark.parametrize("kind", ["+inf", "mixinf", "mixbig"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_extreme_rows_leave_the_honest_value(dtype, kind):
    """8 extremes in every column of node 1's 24 rows (the other nodes share
    some of them and are not looked at): f >= 8 drops them all"""
    rows = _random_rows(40, 3, 24, seed=3)
    X = CE.make("distinct", 40, 322, dtype, seed=5, device=DEV)
    X[rows[1]] = CE.plant_extremes(X[rows[1]], 8, kind)
    groups, ex = D.gossip_groups(rows, DEV), CE.Exact(X[rows[1]])
    for mode, f in ((CE.TRIMMED, 8), (CE.TRIMMED, 11), (CE.MEAMED, 8), (CE.MEAMED, 13)):
        got = _run(X, mode, f, groups=groups)[1]
        assert bool(torch.isfinite(got).all())
        CE.check(got, ex, mode, f, what=kind)


@pytest.mark.parametrize("m", [7, 31])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bit_patterns_give_the_middle_element(dtype, m):
    """inputs uniform over all non-NaN bit patterns; odd m, so the median and
    the trimmed mean at f = (m - 1) / 2 are one input element, bit for bit"""
    g = torch.Generator().manual_seed(m)
    if dtype == torch.float32:
        bits = torch.randint(-(2 ** 31), 2 ** 31, (40, 322), generator=g, dtype=torch.int64)
        X = bits.to(torch.int32).view(torch.float32)
    else:
        bits = torch.randint(-(2 ** 15), 2 ** 15, (40, 322), generator=g, dtype=torch.int64)
        X = bits.to(torch.int16).view(torch.bfloat16)
    X = torch.where(torch.isnan(X), torch.ones_like(X), X).to(DEV)
    rows = _random_rows(40, 5, m, seed=m)
    groups = D.gossip_groups(rows, DEV)
    med = D.median(X, groups=groups)
    trim = D.trimmed_mean(X, (m - 1) // 2, groups=groups)
    for i, r in enumerate(rows):
        mid = X[r].float().sort(dim=0).values[m // 2].to(dtype)
        assert torch.equal(med[i], mid) and torch.equal(trim[i], mid)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_agrees_with_the_indexed_kernel(dtype):
    rows = _random_rows(40, 6, 9, seed=11)
    X = CE.make("distinct", 40, 323, dtype, seed=11, device=DEV)
    groups = D.gossip_groups(rows, DEV)
    med, trim = D.median(X, groups=groups), D.trimmed_mean(X, 2, groups=groups)
    for i, r in enumerate(rows):
        idx = torch.tensor(r, device=DEV)
        assert torch.equal(med[i], D.median(X, rows=idx))
        assert torch.equal(trim[i], D.trimmed_mean(X, 2, rows=idx))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gossip_round_equals_the_per_node_loop(dtype):
    theta, topo = CE.make("distinct", 8, 323, dtype, seed=2, device=DEV), Topology.ring(8, 2)
    for rule, mode, f in (
        (CoordinateWiseMedian(), CE.MEDIAN, 0),
        (CoordinateWiseTrimmedMean(1), CE.TRIMMED, 1),
        (MeanOfMedians(2), CE.MEAMED, 2),
    ):
        got = gossip_round(theta, topo, rule)
        assert got.shape == theta.shape and got.dtype == dtype
        for i in range(8):
            r = [i] + topo.in_neighbors(i)
            if mode == CE.MEAMED:
                CE.check(got[i], CE.Exact(theta[r]), mode, f)
            else:
                assert torch.equal(got[i], rule.aggregate([theta[j] for j in r]))


def test_binding_refusals():
    ops = _hip.require()
    X = torch.zeros(129, 8, device=DEV)

    def table(M, m, dtype=torch.int32):
        return torch.zeros(M, m, dtype=dtype, device=DEV)

    for Xb, groups in ((X[:40], table(2, 33)), (X, table(2, 3)), (X[:40], table(2, 3, torch.int64))):
        with pytest.raises(RuntimeError):
            ops.colsel(Xb.contiguous(), 0, 0, groups=groups, min_m=3)
