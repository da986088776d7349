"""Per-wave Gram slabs of the one-pass median + Gram kernel (colsel.hip:
median_gram_bf16_kernel), through the binding ``ext.colsel(X, 0, 0, gram=G)``.

In the kernel a wave works on strips of 64 rows x 128 columns: it stores a
strip into its own LDS slab, reads it back as four k-steps of 16-byte slots
and accumulates the 10 upper-triangle 16x16 blocks of the slab's Gram; the
block's epilogue sums its four waves and writes (i, j) and (j, i). Strips
reach the waves as one even share each or, from 2^25 columns up, in chunks
of 8 drawn from a work counter; ``BYZPY_MEDIAN_GRAM_TICKET=1`` / ``0``
forces either, so that both loops run at test sizes (the ``split``
fixture).

The data are integers in {-2..2} held in bf16, so every product and every
partial sum is an integer below 2^24 (|G| <= 4 d, d <= 4,000,002 here) and
exact in f32 whatever the summation order: the Gram is compared with the
float64 product by equality, not within a bound. Only the random-data case
uses the bound of tests/test_gpu_median_gram.py.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from _median_gram_cases import (ext, fused, gram_bound, gram_ref,  # noqa: F401
                                 split)

TILE_COLS = 512  # columns that one block of four waves takes at a time
WAVE_COLS = 128  # columns of a strip

NS = [33, 48, 63, 64]
DS = [2, 126, 128, 130, 510, 512, 514, 1022]


def _assert_exact(G, X):
    G_ref = gram_ref(X)
    assert float(G_ref.abs().max()) < 2.0**24
    Gd = G.cpu().double()
    wrong = (Gd != G_ref).nonzero()
    assert wrong.numel() == 0, (
        f"{wrong.shape[0]} wrong Gram entries, first at {wrong[0].tolist()}: "
        f"got {Gd[tuple(wrong[0])].item()}, "
        f"expected {G_ref[tuple(wrong[0])].item()}"
    )


def _int_matrix(n, d, seed, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    X = torch.randint(-2, 3, (n, d), generator=g, device=device)
    return X.to("cuda", torch.bfloat16)


def _two_rows_per_column(n, d):
    """column c is nonzero only in rows c % n and (7 c + 3) % n"""
    c = torch.arange(d)
    X = torch.zeros(n, d)
    X[c % n, c] = (1 + c % 2).float()            # 1 or 2
    X[(7 * c + 3) % n, c] = -(1 + (c // 2) % 2).float()  # -1 or -2
    return X.to("cuda", torch.bfloat16)


@pytest.mark.parametrize("w", range(TILE_COLS // WAVE_COLS))
def test_slab_ownership(ext, w):
    # d = 512 is four strips, one per wave of the only block, and only one
    # of them is nonzero: a wave that read another wave's slab, or missed
    # part of its own, gets a different Gram
    X = torch.zeros(64, TILE_COLS, dtype=torch.bfloat16, device="cuda")
    cols = slice(WAVE_COLS * w, WAVE_COLS * (w + 1))
    X[:, cols] = _int_matrix(64, WAVE_COLS, seed=40 + w)
    assert float(X[:, cols].abs().max()) == 2.0
    med, G = fused(ext, X)
    _assert_exact(G, X)
    assert torch.equal(G, G.T)
    assert torch.equal(med, ext.colsel(X, 0, 0))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", DS)
def test_k_slot_coverage(ext, n, d):
    # every column feeds at most four Gram entries, so a 16-byte slot that
    # is dropped or read twice shows up as a wrong count
    X = _two_rows_per_column(n, d)
    med, G = fused(ext, X)
    _assert_exact(G, X)
    assert torch.equal(G, G.T)
    assert torch.equal(med, ext.colsel(X, 0, 0))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", DS)
def test_dense_integer_data(ext, split, n, d):
    X = _int_matrix(n, d, seed=1000 * n + d)
    med, G = fused(ext, X)
    _assert_exact(G, X)
    assert torch.equal(G, G.T)
    assert torch.equal(med, ext.colsel(X, 0, 0))


def test_many_tiles_per_block_with_partial_last_tile(ext, split):
    # 4,101 strips: with the even split every wave of the persistent grid
    # walks two or three strips without a block barrier; with the counter
    # the first 513 waves walk their first chunk of 8 and every draw lands
    # past the end. The last strip is partial (one full lane, tail lanes).
    d = 2 * 512 * TILE_COLS + 514
    X = _int_matrix(64, d, seed=77, device="cuda")
    med, G = fused(ext, X)
    _assert_exact(G, X)
    assert torch.equal(G, G.T)
    assert torch.equal(med, ext.colsel(X, 0, 0))


def test_drawn_chunks(ext, monkeypatch):
    # 31,251 strips with the counter forced: the grid's first chunks (8 per
    # wave, at most 2 * 304 CUs * 4 waves * 8 = 19,456 strips on the largest
    # part) leave the rest to chunks DRAWN from the counter, so a wrong
    # offset, a duplicated or a skipped chunk shows in the Gram and in the
    # median. 4 d = 16,000,008 < 2^24 keeps the sums exact. The float64
    # reference runs on the device in column blocks (the host copy would be
    # 2 GB).
    monkeypatch.setenv("BYZPY_MEDIAN_GRAM_TICKET", "1")
    n, d = 64, 4_000_002
    X = _int_matrix(n, d, seed=78, device="cuda")
    med, G = fused(ext, X)
    G_ref = torch.zeros(n, n, dtype=torch.float64, device="cuda")
    step = 500_000
    for c in range(0, d, step):
        Xd = X[:, c:c + step].double()
        G_ref += Xd @ Xd.T
    assert float(G_ref.abs().max()) < 2.0**24
    assert torch.equal(G.double(), G_ref)
    assert torch.equal(G, G.T)
    monkeypatch.setenv("BYZPY_MEDIAN_GRAM_TICKET", "0")
    assert torch.equal(med, ext.colsel(X, 0, 0))
    med_even, G_even = fused(ext, X)
    assert torch.equal(med_even, med)
    assert torch.equal(G_even, G)


def test_two_calls_give_the_same_bits(ext, split):
    X = _int_matrix(64, 4 * TILE_COLS + 130, seed=9)
    med1, G1 = fused(ext, X)
    med2, G2 = fused(ext, X)
    assert torch.equal(G1, G2)
    assert torch.equal(med1, med2)
    _assert_exact(G1, X)


def test_random_data(ext, split):
    n, d = 64, 8192
    g = torch.Generator().manual_seed(123)
    X = torch.randn(n, d, generator=g)
    X *= (1.0 + torch.arange(n, dtype=torch.float32) / n)[:, None]
    X = X.to("cuda", torch.bfloat16)
    med, G = fused(ext, X)
    G_ref = gram_ref(X)
    bound = gram_bound(G_ref)
    err = (G.cpu().double() - G_ref).abs().max().item()
    print(f"n={n} d={d} gram err {err:.4g} bound {bound:.4g}")
    assert err < bound
    assert torch.equal(med, ext.colsel(X, 0, 0))
