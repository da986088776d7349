"""The two device subset searches of subsets.hip against brute-force oracles
(tests/_subset_oracles.py, checked on the CPU by test_subset_oracles.py).

MDA: mda_dfs_kernel does only fmaxf and comparisons on the D2 it is given, so
the index tuple must be IDENTICAL to the oracle's, with no tolerance. Every
case runs through dispatch.mda_subset_device (the production bound seed and
first-found reduction), through ext.mda_select with no bound, and with the
bound set to the optimum itself (the exact-tie seed); each twice, since pass
1's atomics may change the node count but never the answer.

SMEA: smea_select_kernel's packed key is decoded into (lam, combo). The
winner must be the oracle's wherever the oracle's relative gap between best
and second best is >= 1e-3, which every case asserts first: that is a
condition on the inputs, ~250 m u at m = 64 (u = 2^-24), which a correct f32
eigen-solve cannot cross. lam must lie within 8 m u ||H G_S H||_F of the
oracle's value for that combo, Jacobi's backward error with a factor 8 for
the ten sweeps. Scaling G by 2^k is exact and must change nothing.

Measured on an MI355X. Largest |lam error| / bound: 0.053, at the mild
(10, 7); 0.047 at (5, 5), 0.021 at (10, 7), 0.014 at (16, 8), 0.001 at
(66, 64). Before the rotation skip became relative, every scale case failed
at k = -60 and k = -44: lam was the largest diagonal entry, 24 % to 32 % low,
and on the two mild inputs the winner was wrong (combo 90 for 5, 5821 for
9253), as in the end-to-end mild case at 2^-22; the mild (10, 7) also missed
the bound at k = -30 (2.2 times); k = 0, 30, 60 held.
Timings: this file's GPU tests take 4 s together; the slowest are the first
one (0.8 s, it loads the code object), SMEA (66, 64) (0.24 s) and the MDA
cases at (19, 8) (0.05 s each, most of it the oracle); the planted 48-of-64
takes 0.04 s for its six searches. The slowest of TestDeviceSubsetSearch in
test_gpu_kernels.py on the same machine: 0.25 s (the first), then 0.05 s.
The host search (ext.mda_search) takes under 3 ms on every case here,
tie families at mid-depth included, and 0.6 ms on the planted 48-of-64 (it
did not return on that one while nodes were cut on positions left alone).
"""
import functools
import math
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _subset_oracles as SO
from byzpy_amd.hip import dispatch as D
from byzpy_amd.hip import require
from byzpy_amd.ops import functional as F

U32 = 2.0**-24  # f32 unit roundoff
MIN_GAP = 1e-3


@pytest.fixture(scope="module")
def ext():
    return require()


# ---------------------------------------------------------------------------
# MDA
# ---------------------------------------------------------------------------


def _gaussian_d2(n, f):
    """Squared distances of Gaussian rows as the device computes them, copied
    back: the oracle sees the bits the kernel sees."""
    g = torch.Generator().manual_seed(977 * n + f)
    X = torch.randn(n, 96, generator=g).cuda()
    return D.pairwise_sq_dists(X).cpu().numpy()


FAMILIES = dict(SO.MDA_FAMILIES, gaussian=(_gaussian_d2, lambda n, f: True))

MDA_CASES = [
    (n, f, name)
    for (n, f) in SO.MDA_SHAPES + [SO.MDA_F0_SHAPE]
    for name, (_, applies) in FAMILIES.items()
    if applies(n, f)
]


@functools.lru_cache(maxsize=None)
def _mda_case(n, f, name):
    D2 = FAMILIES[name][0](n, f)
    want = SO.mda_oracle(D2, f)
    return D2, want, SO.mda_diameter(D2, want)


def _first_found(found, subsets):
    """The first found prefix in lexicographic order holds the winner."""
    hit = np.flatnonzero(found.cpu().numpy())
    assert hit.size > 0, "no prefix found a subset"
    return tuple(int(i) for i in subsets[int(hit[0])].cpu())


def _check_mda(ext, D2, f, want, diam, device_may_decline=False):
    n = D2.shape[0]
    D2d = torch.from_numpy(D2).cuda()
    ub = torch.tensor(float(diam), dtype=torch.float32, device="cuda")
    for rep in range(2):
        if 2 <= n - f < n:
            got = D.mda_subset_device(D2d, f)
            if not (device_may_decline and got is None):
                assert got is not None and got.dtype == torch.int32
                assert tuple(int(i) for i in got.cpu()) == want, f"dispatch, run {rep}"
        assert _first_found(*ext.mda_select(D2d, f, None)) == want, f"ub=None, run {rep}"
        assert _first_found(*ext.mda_select(D2d, f, ub)) == want, f"ub=optimum, run {rep}"


@pytest.mark.parametrize("n,f,name", MDA_CASES)
def test_mda_exact(ext, n, f, name):
    D2, want, diam = _mda_case(n, f, name)
    # with every distance at +inf the dispatcher may leave it to the host
    _check_mda(ext, D2, f, want, diam, device_may_decline=(name == "all_inf"))


def test_mda_f0_is_all_rows():
    n, f = SO.MDA_F0_SHAPE
    assert _mda_case(n, f, "small_ints")[1] == tuple(range(n))


def test_mda_planted_48_of_64(ext):
    """Mid-range f at the n cap, out of brute force's reach: the optimum is
    known by construction and the host search must agree."""
    # the small cluster first: a host search that cuts on positions left is
    # slow there and fails, where it would hang on the 48 of 64
    n, m = SO.PLANTED_GUARD_NATIVE
    D2, rows = SO.mda_planted_small(n, m)
    t0 = time.perf_counter()
    host = tuple(int(i) for i in ext.mda_search(torch.from_numpy(D2), n - m))
    assert host == rows and time.perf_counter() - t0 < SO.PLANTED_GUARD_SECONDS
    D2, rows = SO.mda_planted_64_16()
    host = tuple(int(i) for i in ext.mda_search(torch.from_numpy(D2), 16))
    assert host == rows
    _check_mda(ext, D2, 16, rows, SO.mda_diameter(D2, rows))


def test_mda_all_inf_end_to_end():
    """Rows of a scaled centred simplex: norms^2 near 1.6e38 and pairwise dot
    products below 0, so every squared distance overflows to +inf while the
    diagonal stays 0."""
    n, f = 8, 3
    a = math.sqrt(1.8e38)
    X = torch.zeros(n, 64)
    X[:, :n] = a * (torch.eye(n) - 1.0 / n)
    D2 = D.pairwise_sq_dists(X.cuda()).cpu()
    off = ~torch.eye(n, dtype=torch.bool)
    assert bool(torch.isinf(D2[off]).all()) and bool((D2.diagonal() == 0).all())
    out = D.minimum_diameter_averaging(X.cuda(), f).cpu()
    ref = F.minimum_diameter_averaging(X, f)
    assert float((out - ref).norm() / ref.norm()) < 1e-5


# ---------------------------------------------------------------------------
# SMEA
# ---------------------------------------------------------------------------


def _decode(best):
    """(lam, combo index) from the packed u64 key: the low word is the combo,
    the high word the monotone key of f32_key in subsets.hip."""
    key = int(best.cpu()[0]) & 0xFFFFFFFFFFFFFFFF
    idx, kb = key & 0xFFFFFFFF, key >> 32
    bits = (kb ^ 0x80000000) if (kb & 0x80000000) else (~kb & 0xFFFFFFFF)
    return float(np.array([bits], dtype=np.uint32).view(np.float32)[0]), idx


# (16, 8): C = 12870 > the 8192-block cap; a tight set that starts at row 2
# has a combo index >= C(15,7) + C(14,7) = 9867, found on a block's second trip
TIGHT_16_8 = (2, 4, 5, 7, 9, 11, 12, 15)
# (128, 64): both caps at once. C(128, 64) cannot be listed, and the binding
# takes any combo list, so this case hands it 128 chosen ones (_combos_128_64).
# (128, 127), C = 128, is above the m cap: test_smea_refuses_m_above_64.
SMEA_SHAPES = [(10, 7), (16, 8), (12, 1), (5, 5), (66, 64), (128, 64)]
# The graded outliers above leave oracle gaps of several hundred percent: the
# winner then survives an eigenvalue that is 30 % off. These two push the
# outliers out by less than the noise's own norm, (push, seed) picked on the
# CPU for a gap of 2.3 % and 5.7 % and for a winner that ranking by the largest
# diagonal entry of H G_S H (what a solve that rotates nothing returns) misses:
# it takes combo 90 for 5 and 5821 for 9253. 9253 is again past the block cap.
MILD = {(10, 7): dict(push=(0.4, 0.2), seed=6), (16, 8): dict(push=(0.6, 0.3), seed=2)}
MILD_MAX_GAP = 0.1
SMEA_CASES = [(n, m, False) for n, m in SMEA_SHAPES] + [(n, m, True) for n, m in MILD]
SCALE_CASES = [(n, m, mild) for mild in (False, True) for n, m in MILD]


def _combos_128_64(X):
    """128 subsets of 64 rows: the tight rows with one row swapped for each of
    the 64 outliers, 63 seeded random subsets, and the tight rows themselves
    at position 37."""
    n, m = 128, 64
    norms = np.linalg.norm(X, axis=1)
    tight = np.sort(np.argsort(norms)[:m])
    out = np.setdiff1d(np.arange(n), tight)
    rng = np.random.default_rng(12864)
    combos = [np.sort(np.concatenate([np.delete(tight, i), out[i : i + 1]])) for i in range(m)]
    combos += [np.sort(rng.choice(n, size=m, replace=False)) for _ in range(m - 1)]
    combos.insert(37, tight)
    return np.array(combos, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _smea_case(n, m, mild=False):
    if mild:
        X = SO.smea_rows(n, m, **MILD[(n, m)])
    else:
        X = SO.smea_rows(n, m, tight=TIGHT_16_8 if (n, m) == (16, 8) else None)
    G = SO.gram_f32(X)
    combos = _combos_128_64(X) if (n, m) == (128, 64) else SO.all_combos(n, m)
    lam, win = SO.smea_oracle(G, combos)
    bound = 8 * m * U32 * float(np.linalg.norm(SO.smea_centred(G, combos[win])))
    return X, G, combos, lam, win, bound


def _select(ext, G, combos):
    return _decode(ext.smea_select(torch.from_numpy(G).cuda(), torch.from_numpy(combos).cuda()))


def _check_gap(lam, mild):
    gap = SO.relative_gap(lam)
    assert gap >= MIN_GAP
    if mild:
        assert gap <= MILD_MAX_GAP  # or the winner check has no teeth


@pytest.mark.parametrize("n,m,mild", SMEA_CASES)
def test_smea_winner_and_eigenvalue(ext, n, m, mild):
    X, G, combos, lam, win, bound = _smea_case(n, m, mild)
    if (n, m) == (128, 64):
        assert len(combos) == 128 and win == 37
    else:
        assert len(combos) == math.comb(n, m)
    if m == 1:
        assert (lam == 0.0).all() and win == 0  # a single row has no spread
    elif len(combos) > 1:
        _check_gap(lam, mild)
    if (n, m) == (16, 8):
        assert win > 8192
    got_lam, got = _select(ext, G, combos)
    ratio = abs(got_lam - lam[win]) / bound if bound > 0 else 0.0
    print(f"smea n={n} m={m} mild={mild} C={len(combos)} winner={win} lam={lam[win]:.6g} "
          f"device lam={got_lam:.6g} |diff|/bound={ratio:.3f}")
    assert got == win
    assert abs(got_lam - lam[win]) <= bound


def test_smea_refuses_m_above_64(ext):
    """(128, 127): n at D.smea's cap, but one wave stages at most 64 rows, so
    the binding must refuse before the kernel runs and D.smea takes the host
    path (n - f <= 64 is part of its device condition)."""
    n, m = 128, 127
    G = torch.eye(n, device="cuda")
    combos = torch.from_numpy(SO.all_combos(n, m)).cuda()
    assert combos.shape == (128, 127)
    with pytest.raises(RuntimeError, match=r"1 <= m <= 64 rows per combo.*got m = 127"):
        ext.smea_select(G, combos)


def test_smea_exact_tie_takes_the_first_combo(ext):
    n, m = 10, 7
    G = np.full((n, n), 4.0, dtype=np.float32)  # all rows identical
    got_lam, got = _select(ext, G, SO.all_combos(n, m))
    assert got == 0 and got_lam == 0.0


@pytest.mark.parametrize("n,m,mild", SCALE_CASES)
def test_smea_scale(ext, n, m, mild):
    """G * 2^k is exact, so the winner stays and lam scales by 2^k."""
    X, G, combos, lam, win, bound = _smea_case(n, m, mild)
    assert 0.1 < float(np.abs(G).max()) < 1000.0  # well scaled at k = 0
    _check_gap(lam, mild)
    lam0, got0 = _select(ext, G, combos)
    assert got0 == win
    failed = []
    for k in (-60, -44, -30, 0, 30, 60):
        Gk = G * np.float32(2.0**k)
        assert (Gk.astype(np.float64) == G.astype(np.float64) * 2.0**k).all()
        lam_k, got = _select(ext, Gk, combos)
        err = abs(lam_k / 2.0**k - lam0)
        print(f"smea scale n={n} m={m} mild={mild} k={k}: combo {got} (oracle {win}) "
              f"lam/2^k={lam_k / 2.0**k:.6g} lam0={lam0:.6g} |diff|/bound={err / bound:.3f}")
        if got != win or err > bound:
            failed.append(k)
    assert not failed, f"k in {failed}: wrong combo or lam off by more than the bound"


@pytest.mark.parametrize("mild", [False, True])
def test_smea_small_rows_end_to_end(mild):
    n, m = 10, 7
    X, G, combos, lam, win, _ = _smea_case(n, m, mild)
    Xs = X * np.float32(2.0**-22)
    out = D.smea(torch.from_numpy(Xs).cuda(), n - m).cpu().numpy()
    want = Xs[combos[win]].astype(np.float64).mean(axis=0)
    np.testing.assert_allclose(out, want, rtol=1e-5, atol=1e-6 * 2.0**-22)
