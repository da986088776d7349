"""Bulyan on the GPU: the row-indexed colsel variants against the gathered
call (bit-identical: same kernel body, same values, only addressing
differs), the fused iterative selection against the oracle run on the same
device Gram, and the end-to-end rule."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from byzpy_amd.aggregators import Bulyan
from byzpy_amd.hip import dispatch as D
from byzpy_amd.hip import require
from byzpy_amd.ops import functional as F

DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def ext():
    return require()


def _tol(dtype):  # as in test_gpu_kernels.py
    return dict(atol=1e-4, rtol=1e-4) if dtype == torch.float32 else dict(atol=5e-2, rtol=5e-2)


# -- indexed colsel ---------------------------------------------------------

# (n, m, d): one case per kernel / pad branch
ROW_CASES = [
    (16, 5, 33),      # m < 8 pad branch; odd d keeps bf16 off the packed path
    (64, 34, 4098),   # packed bf16, P = 64, partial tile
    (64, 64, 1024),   # full-tile n == P walk; rows is a permutation of all n
    (40, 32, 1000),   # P = 32, full
    (100, 80, 777),   # LDS path, P = 128
    (600, 300, 130),  # LDS path, P = 512; source n above the colsel cap
]


@functools.lru_cache(maxsize=None)
def _row_case(n, m, d, dtype):
    g = torch.Generator().manual_seed(7 * n + m)
    X = torch.randn(n, d, generator=g).to("cuda", dtype)
    rows = torch.randperm(n, generator=g)[:m].to("cuda", torch.int32)
    return X, rows, X[rows.long()].contiguous()


@pytest.mark.parametrize("n,m,d", ROW_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_indexed_colsel_equals_gathered(ext, n, m, d, dtype, mode):
    X, rows, gathered = _row_case(n, m, d, dtype)
    assert rows.tolist() != sorted(rows.tolist())  # non-monotone
    # f: none for the median, a quarter trimmed per side, and for
    # mean-around-median both a third and Bulyan's regime 2f >= m
    fs = {0: [0], 1: [max(1, m // 4)], 2: [max(1, m // 3), (2 * m) // 3]}[mode]
    for f in fs:
        got = ext.colsel(X, mode, f, rows)
        ref = ext.colsel(gathered, mode, f)
        assert got.dtype == dtype and got.shape == (d,)
        assert torch.equal(got, ref), (mode, f)


def _window_meamed(Xsel, f):
    """Mean-around-median as a contiguous window of the sorted column:
    shrink from whichever end is farther from the median, the right end on
    a tie — the kernels' rule. The m - f values closest to the median
    always form such a window; only deviation ties leave a choice, and
    bf16 data is full of them, which is why this and not F's topk is the
    reference for bf16."""
    m, d = Xsel.shape
    s = torch.sort(Xsel.float().cpu(), dim=0).values
    med = 0.5 * (s[(m - 1) // 2] + s[m // 2])
    lo = torch.zeros(d, dtype=torch.long)
    hi = torch.full((d,), m, dtype=torch.long)
    for _ in range(f):
        vl = s.gather(0, lo[None])[0]
        vr = s.gather(0, (hi - 1)[None])[0]
        left = (med - vl) > (vr - med)
        lo += left.long()
        hi -= (~left).long()
    c = torch.cat([torch.zeros(1, d, dtype=torch.float64), s.double().cumsum(0)])
    return ((c.gather(0, hi[None]) - c.gather(0, lo[None]))[0] / (m - f)).float()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("n,m,d", [(64, 34, 4098), (16, 10, 2048), (100, 80, 777)])
def test_indexed_meamed_in_bulyan_regime_matches_window_reference(ext, n, m, d, dtype):
    # 2f >= m: the regime only Bulyan asks of mean-around-median
    X, rows, gathered = _row_case(n, m, d, dtype)
    f = m - 4
    got = ext.colsel(X, 2, f, rows)
    assert torch.allclose(got.float().cpu(), _window_meamed(gathered, f), **_tol(dtype))


def test_indexed_dispatch_routes_and_matches(ext):
    X, rows, gathered = _row_case(100, 80, 777, torch.float32)
    assert torch.equal(D.median(X, rows=rows), D.median(gathered))
    assert torch.equal(D.trimmed_mean(X, 9, rows=rows), D.trimmed_mean(gathered, 9))
    assert torch.equal(
        D.mean_of_medians(X, 9, rows=rows.long()), D.mean_of_medians(gathered, 9)
    )
    # m > 64 at d >= 32768: gathers, so the radix engine serves it
    g = torch.Generator().manual_seed(5)
    Xw = torch.randn(90, 32768, generator=g).cuda()
    r = torch.randperm(90, generator=g)[:70].cuda()
    assert torch.equal(D.median(Xw, rows=r), D.median(Xw[r].contiguous()))
    # ... including mean-around-median with 2f >= m, Bulyan's regime
    got = D.mean_of_medians(Xw, 45, rows=r)
    ref = F.mean_of_medians(Xw.cpu()[r.cpu()], 45)
    assert torch.allclose(got.cpu(), ref, **_tol(torch.float32))


def test_indexed_colsel_rejections(ext):
    X = torch.randn(600, 16).cuda()
    with pytest.raises(RuntimeError):
        ext.colsel(X, 0, 0, torch.arange(513, dtype=torch.int32).cuda())
    with pytest.raises(RuntimeError):
        ext.colsel(X, 0, 0, torch.arange(8).cuda())  # int64
    with pytest.raises(RuntimeError):
        ext.colsel(X, 0, 0, torch.arange(8, dtype=torch.int32))  # CPU rows
    rows = torch.arange(8, dtype=torch.int32).cuda()
    with pytest.raises(RuntimeError):
        ext.colsel(X, 1, 4, rows)  # 2f >= m, although 2f < n
    with pytest.raises(RuntimeError):
        ext.colsel(X, 0, 4, rows)
    with pytest.raises(RuntimeError):
        ext.colsel(X, 2, 8, rows)  # mean-around-median keeps m - f >= 1
    assert ext.colsel(X, 2, 7, rows).shape == (16,)


# -- fused selection --------------------------------------------------------

SELECT_CASES = [(11, 2, 1000), (23, 5, 2050), (64, 15, 4097), (67, 16, 512), (100, 10, 777)]


def _scaled_permuted(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, d, generator=g) * (1 + 0.1 * torch.arange(n))[:, None]
    # unpermuted, the answer is nearly arange(theta): a wrong kernel could pass
    return X[torch.randperm(n, generator=g)]


@functools.lru_cache(maxsize=None)
def _select_case(n, f, d, dtype):
    X = _scaled_permuted(n, d, 1000 + n).to("cuda", dtype)
    G = D.gram(X)
    oracle = F.bulyan_select_from_gram(G.cpu(), f)
    return X, G, oracle


@pytest.mark.parametrize("n,f,d", SELECT_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_device_selection_matches_oracle_on_same_gram(ext, n, f, d, dtype):
    _, G, oracle = _select_case(n, f, d, dtype)
    got = ext.krum_select(G, f, n - 2 * f, True)
    assert got.dtype == torch.int32 and got.is_cuda
    assert got.cpu().tolist() == oracle.tolist()
    assert D.bulyan_select_from_gram(G, f).cpu().tolist() == oracle.tolist()


def test_default_krum_select_unchanged_by_flag(ext):
    _, G, _ = _select_case(64, 15, 4097, torch.float32)
    assert torch.equal(ext.krum_select(G, 15, 8), ext.krum_select(G, 15, 8, False))


def test_iterative_selection_rejections(ext):
    G = torch.eye(12).cuda()
    with pytest.raises(RuntimeError):
        ext.krum_select(G, 2, 10, True)  # last pick would have k = 0
    assert ext.krum_select(G, 2, 9, True).shape == (9,)


@pytest.mark.parametrize("n,f,d", SELECT_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_bulyan_end_to_end(n, f, d, dtype):
    X, _, oracle = _select_case(n, f, d, dtype)
    sel = oracle.cuda()
    out = D.bulyan(X, f)
    assert out.dtype == dtype and out.shape == (d,)
    assert torch.equal(out, D.mean_of_medians(X[sel].contiguous(), 2 * f))
    if dtype == torch.float32:
        ref = F.mean_of_medians(X.cpu()[oracle], 2 * f)
        assert torch.allclose(out.cpu(), ref, **_tol(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_aggregator_on_device_tensors(dtype):
    X, _, _ = _select_case(23, 5, 2050, dtype)
    out = Bulyan(5).aggregate(list(X))
    assert out.is_cuda and out.dtype == dtype and out.shape == (2050,)
    assert torch.equal(out, D.bulyan(X, 5))


def test_robust_to_non_finite_and_huge_rows(ext):
    # Exact agreement with the oracle is a fair demand here too: 49 honest
    # rows outnumber the 34 picks and an honest row's k nearest survivors
    # are all honest, so only honest scores ever compete. In f64 on the CPU
    # the smallest best/runner-up relative gap over the picks is 1.2e-4
    # for this input, against f32 summation error near k * 2^-24 = 3e-6.
    n, f, d = 64, 15, 2048
    X = _scaled_permuted(n, d, 77)
    g = torch.Generator().manual_seed(78)
    bad = torch.randperm(n, generator=g)[:f]
    X[bad[:5]] = float("inf")
    X[bad[5:10]] = 1.0e6
    X[bad[10:]] = 1.0e4 * torch.randn(5, d, generator=g)
    X = X.cuda()
    G = D.gram(X)
    oracle = F.bulyan_select_from_gram(G.cpu(), f)
    sel = ext.krum_select(G, f, n - 2 * f, True).cpu()
    assert sel.tolist() == oracle.tolist()
    assert not set(sel.tolist()) & set(bad[:5].tolist())
    out = D.bulyan(X, f)
    assert torch.isfinite(out).all()
    ref = F.mean_of_medians(X.cpu()[oracle], 2 * f)
    assert torch.allclose(out.cpu(), ref, **_tol(torch.float32))


def test_above_the_iterative_cap_falls_back_to_torch(ext):
    # smallest relative score gap over the 126 picks, f64 on the CPU:
    # 1.7e-4, against f32 summation error near k * 2^-24 = 8e-6
    n, f, d = 130, 2, 64
    assert n > D.BULYAN_SELECT_MAX_N
    X = _scaled_permuted(n, d, 1000 + n).cuda()
    G = D.gram(X)
    with pytest.raises(RuntimeError):
        ext.krum_select(G, f, n - 2 * f, True)
    oracle = F.bulyan_select_from_gram(G.cpu(), f)
    assert D.bulyan_select_from_gram(G, f).cpu().tolist() == oracle.tolist()
    out = D.bulyan(X, f)
    ref = F.mean_of_medians(X.cpu()[oracle], 2 * f)
    assert torch.allclose(out.cpu(), ref, **_tol(torch.float32))
