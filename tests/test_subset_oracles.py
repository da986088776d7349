"""The brute-force subset oracles (tests/_subset_oracles.py) checked on the CPU
against the project's two host searches and its batched-eigvalsh SMEA, on the
input families that test_gpu_subset_search.py then puts to the device
kernels. No GPU anywhere in this file."""
import time

import numpy as np
import pytest
import torch

import _subset_oracles as SO
from byzpy_amd import hip
from byzpy_amd.ops import functional as F

CASES = [
    (n, f, name)
    for (n, f) in SO.MDA_SHAPES + [SO.MDA_F0_SHAPE]
    for name, (_, applies) in SO.MDA_FAMILIES.items()
    if applies(n, f)
]


@pytest.fixture(scope="module")
def ext():
    return hip.require()


def test_every_family_is_symmetric_f32_with_zero_diagonal():
    for n, f, name in CASES:
        D2 = SO.MDA_FAMILIES[name][0](n, f)
        assert D2.dtype == np.float32 and D2.shape == (n, n), (n, f, name)
        assert (D2 == D2.T).all() and (np.diag(D2) == 0).all(), (n, f, name)
        assert not np.isnan(D2).any()


def test_mda_oracle_by_hand():
    # rows 1, 2, 3 are pairwise at 1; row 0 is at 5 from them
    D2 = np.array(
        [[0, 5, 5, 5], [5, 0, 1, 1], [5, 1, 0, 1], [5, 1, 1, 0]], dtype=np.float32
    )
    assert SO.mda_oracle(D2, 1) == (1, 2, 3)
    assert SO.mda_diameter(D2, (1, 2, 3)) == np.float32(1.0)
    assert SO.mda_oracle(D2, 2) == (1, 2)  # three pairs tie at 1: the first
    assert SO.mda_oracle(D2, 0) == (0, 1, 2, 3)
    assert SO.mda_oracle(SO.mda_all_inf(5, 2), 2) == (0, 1, 2)


def test_mda_oracle_compares_f32_values():
    # 1 and its f32 successor differ; as the same value the subsets would tie
    one_up = np.nextafter(np.float32(1.0), np.float32(2.0))
    D2 = np.array([[0, one_up, 9], [one_up, 0, 1], [9, 1, 0]], dtype=np.float32)
    assert SO.mda_oracle(D2, 1) == (1, 2)


def test_mda_oracle_refuses_large_searches():
    with pytest.raises(ValueError):
        SO.mda_oracle(np.zeros((24, 24), dtype=np.float32), 12)


def test_planted_families_hold_what_they_promise():
    for n, f in SO.MDA_SHAPES:
        m = n - f
        rows = tuple(int(r) for r in SO.planted_rows(n, m))
        assert rows != tuple(range(m))
        D2 = SO.mda_planted_clique(n, f)
        assert SO.mda_diameter(D2, rows) == 1.0
        assert SO.mda_diameter(D2, SO.mda_oracle(D2, f)) == 1.0
        if m >= 3:
            D2 = SO.mda_no_clique(n, f)
            assert SO.mda_oracle(D2, f) == tuple(range(m))
            assert SO.mda_diameter(D2, tuple(range(m))) == 2.0
    D2, rows = SO.mda_planted_64_16()
    out = np.setdiff1d(np.arange(64), rows)
    assert len(rows) == 48 and rows != tuple(range(48))
    assert SO.mda_diameter(D2, rows) <= 1.0
    assert D2[out][:, rows].min() >= 100.0
    assert (D2[np.ix_(out, out)] + 1e9 * np.eye(16)).min() >= 100.0


@pytest.mark.parametrize("n,f,name", CASES)
def test_mda_oracle_matches_host_search(ext, n, f, name):
    D2 = SO.MDA_FAMILIES[name][0](n, f)
    want = SO.mda_oracle(D2, f)
    got = tuple(int(i) for i in ext.mda_search(torch.from_numpy(D2), f))
    assert got == want


@pytest.mark.parametrize("n,f,name", CASES)
def test_mda_oracle_matches_python_dfs(monkeypatch, n, f, name):
    D2 = SO.MDA_FAMILIES[name][0](n, f)
    want = SO.mda_oracle(D2, f)
    monkeypatch.setattr(hip, "extension", lambda: None)
    assert F.mda_subset(torch.from_numpy(D2), f) == want


def _guarded_planted(search, n, m):
    """A small planted cluster within SO.PLANTED_GUARD_SECONDS: a search that
    cuts on positions left is slow here, and would not come back from the
    planted 48 of 64."""
    D2, rows = SO.mda_planted_small(n, m)
    t0 = time.perf_counter()
    got = search(torch.from_numpy(D2), n - m)
    seconds = time.perf_counter() - t0
    assert got == rows
    assert seconds < SO.PLANTED_GUARD_SECONDS, f"planted {m} of {n} took {seconds:.3f} s"


def test_host_search_finds_the_planted_clusters(ext):
    def search(D2, f):
        return tuple(int(i) for i in ext.mda_search(D2, f))

    _guarded_planted(search, *SO.PLANTED_GUARD_NATIVE)  # fails here, or hangs below
    D2, rows = SO.mda_planted_64_16()
    assert search(torch.from_numpy(D2), 16) == rows


def test_python_dfs_finds_the_planted_cluster(monkeypatch):
    # the small case only: with no greedy seed the Python search needs 9 s for
    # the 48 of 64
    monkeypatch.setattr(hip, "extension", lambda: None)
    _guarded_planted(F.mda_subset, *SO.PLANTED_GUARD_PYTHON)


def test_smea_oracle_by_hand():
    # three collinear points at 0, 1, 3: the pair (0, 1) has the least spread.
    # Centred pair Gram has the single eigenvalue (gap)^2 / 2.
    x = np.array([0.0, 1.0, 3.0], dtype=np.float32)
    G = np.outer(x, x).astype(np.float32)
    lam, win = SO.smea_oracle(G, SO.all_combos(3, 2))
    assert win == 0
    np.testing.assert_allclose(lam, [0.5, 4.5, 2.0], rtol=1e-12)


@pytest.mark.parametrize("n,m", [(10, 7), (8, 5)])
def test_smea_oracle_matches_functional(n, m):
    X = SO.smea_rows(n, m)
    combos = SO.all_combos(n, m)
    lam, win = SO.smea_oracle(SO.gram_f32(X), combos)
    assert SO.relative_gap(lam) >= 1e-3
    want = X[combos[win]].astype(np.float64).mean(axis=0)
    got = F.smea(torch.from_numpy(X), n - m)
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-5, atol=1e-6)
