"""One-pass median + Gram (colsel.hip: median_gram_bf16_kernel) through the
binding, ``ext.colsel(X, 0, 0, gram=G)``, so that small d reaches the fused
kernel too (D.median_and_gram only routes to it from
MEDIAN_GRAM_FUSED_MIN_D columns up).

Median: bitwise equal to the separate kernel, ``ext.colsel(X, 0, 0)``.
Gram: within TestFusedGramMedian.test_parity's bound,
0.3 * max(1, max|G_ref| / 100), of the float64 CPU product of the bf16
values.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from _median_gram_cases import ext, fused, gram_bound, gram_ref  # noqa: F401
from byzpy_amd.hip import dispatch as D

TILE_COLS = 512  # columns per tile of the fused kernel


def _rand(n, d, seed):
    """bf16 (n, d) on the device; row i has std 1 + i / n, so no two rows
    (and no two Gram entries) are interchangeable"""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, d, generator=g)
    X *= (1.0 + torch.arange(n, dtype=torch.float32) / n)[:, None]
    return X.to("cuda", torch.bfloat16)


def _check(ext, X):
    med, G = fused(ext, X)
    G_ref = gram_ref(X)
    err = (G.cpu().double() - G_ref).abs().max().item()
    print(f"n={X.shape[0]} d={X.shape[1]} gram err {err:.4g} "
          f"bound {gram_bound(G_ref):.4g}")
    assert torch.equal(med, ext.colsel(X, 0, 0))
    assert err < gram_bound(G_ref)
    return G, G_ref


@pytest.mark.parametrize("n", [33, 48, 63, 64])
@pytest.mark.parametrize("d", [2, 510, 512, 514, 1022])
def test_small_shapes(ext, n, d):
    _check(ext, _rand(n, d, seed=1000 * n + d))


def test_multi_tile_multi_block_with_partial_last_tile(ext):
    # 2 * 512 blocks' worth of full tiles, then 514 columns: every block of
    # the persistent grid accumulates more than one tile, the last tile is
    # partial (one full lane plus tail lanes)
    d = 2 * 512 * TILE_COLS + 514
    g = torch.Generator(device="cuda").manual_seed(77)
    X = torch.randn(64, d, generator=g, device="cuda")
    X *= (1.0 + torch.arange(64, device="cuda", dtype=torch.float32) / 64)[:, None]
    _check(ext, X.to(torch.bfloat16))


def test_inf_rows_keep_the_median_bits(ext):
    X = _rand(64, 8192, seed=11)
    X[3] = float("inf")
    X[5] = float("-inf")
    med, _ = fused(ext, X)
    assert torch.equal(med, ext.colsel(X, 0, 0))


def test_gram_is_overwritten_not_accumulated(ext):
    X = _rand(48, 1022, seed=5)
    G_ref = gram_ref(X)
    _, G = fused(ext, X)
    first = G.clone()
    fused(ext, X, G)
    diff = (G - first).abs().max().item()
    print(f"second call differs by {diff:.4g}, bound {gram_bound(G_ref):.4g}")
    assert diff < gram_bound(G_ref)
    assert (G.cpu().double() - G_ref).abs().max().item() < gram_bound(G_ref)


def test_split_toggle_gives_the_same_median(monkeypatch):
    d = 262_144 + 2
    assert d >= D.MEDIAN_GRAM_FUSED_MIN_D
    X = _rand(64, d, seed=21)
    monkeypatch.delenv("BYZPY_MEDIAN_GRAM", raising=False)
    med_fused, G_fused = D.median_and_gram(X)
    monkeypatch.setenv("BYZPY_MEDIAN_GRAM", "split")
    med_split, G_split = D.median_and_gram(X)
    assert torch.equal(med_fused, med_split)
    G_ref = gram_ref(X)
    for G in (G_fused, G_split):
        assert (G.cpu().double() - G_ref).abs().max().item() < gram_bound(G_ref)


@pytest.mark.parametrize(
    "n,d,dtype",
    [(16, 514, torch.bfloat16), (40, 513, torch.bfloat16),
     (40, 512, torch.float32), (80, 512, torch.bfloat16)],
)
def test_keyword_means_the_same_where_the_fused_kernel_does_not_apply(
    ext, n, d, dtype
):
    g = torch.Generator().manual_seed(n + d)
    X = torch.randn(n, d, generator=g).to("cuda", dtype)
    med, G = fused(ext, X)
    assert torch.equal(med, ext.colsel(X, 0, 0))
    G_ref = gram_ref(X)
    assert (G.cpu().double() - G_ref).abs().max().item() < gram_bound(G_ref)


def test_bad_arguments_are_refused_by_name(ext):
    X = _rand(40, 64, seed=3)
    G = torch.zeros(40, 40, device="cuda")
    rows = torch.arange(40, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="mode 0"):
        ext.colsel(X, 1, 1, gram=G)
    with pytest.raises(RuntimeError, match="rows"):
        ext.colsel(X, 0, 0, rows, gram=G)
    with pytest.raises(RuntimeError, match="gram"):
        ext.colsel(X, 0, 0, gram=torch.zeros(39, 39, device="cuda"))
    with pytest.raises(RuntimeError, match="gram"):
        ext.colsel(X, 0, 0, gram=torch.zeros(40, 40))
