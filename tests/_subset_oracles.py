"""Brute-force oracles for the two subset searches (MDA, SMEA) and the crafted
inputs their tests share. Plain numpy and itertools: nothing here touches a
GPU or the extension, and tests/test_subset_oracles.py checks it on the CPU.

MDA's device search does only fmaxf and comparisons on the D2 it is given, so
its answer is a function of D2's bits: ``mda_oracle`` compares the f32 values
themselves and the tests demand the identical index tuple."""
import itertools
import math

import numpy as np

MDA_MAX_SUBSETS = 200_000
_CHUNK_ELEMS = 1 << 22  # entries of one (B, m, m) gather


def _combo_chunks(n, m, rows_per_chunk):
    it = itertools.combinations(range(n), m)
    while True:
        flat = np.fromiter(
            itertools.chain.from_iterable(itertools.islice(it, rows_per_chunk)),
            dtype=np.int64,
        )
        if flat.size == 0:
            return
        yield flat.reshape(-1, m)


def mda_oracle(D2, f):
    """The lexicographically smallest m-subset, m = n - f, among those that
    minimise max_{i<j in S} D2[i, j]. D2 is (n, n) f32; +inf entries are
    allowed. Brute force, refused above MDA_MAX_SUBSETS subsets."""
    D2 = np.asarray(D2)
    assert D2.dtype == np.float32 and D2.ndim == 2 and D2.shape[0] == D2.shape[1]
    n = D2.shape[0]
    m = n - int(f)
    assert 1 <= m <= n
    total = math.comb(n, m)
    if total > MDA_MAX_SUBSETS:
        raise ValueError(f"C({n},{m}) = {total} > {MDA_MAX_SUBSETS}: not brute-forceable")
    off = np.triu(np.ones((m, m), dtype=bool), 1)  # i < j only, as the definition says
    best_d, best_s = None, None
    for combos in _combo_chunks(n, m, max(1, _CHUNK_ELEMS // (m * m))):
        sub = D2[combos[:, :, None], combos[:, None, :]]  # (B, m, m) f32
        diam = np.where(off[None], sub, np.float32(0.0)).max(axis=(1, 2))
        b = int(np.argmin(diam))  # first index at the minimum: chunks are in lex order
        if best_d is None or diam[b] < best_d:
            best_d, best_s = diam[b], tuple(int(i) for i in combos[b])
    return best_s


def mda_diameter(D2, subset):
    """max_{i<j in subset} D2[i, j] as an f32 scalar (0 for a single row)."""
    s = np.asarray(subset, dtype=np.int64)
    sub = np.asarray(D2)[np.ix_(s, s)]
    upper = np.triu(np.ones((s.size, s.size), dtype=bool), 1)
    return np.float32(np.where(upper, sub, np.float32(0.0)).max())


def smea_oracle(G, combos):
    """(lam, winner): lam[c] is the largest eigenvalue of the centred subset
    Gram H G_S H of combo c, formed in float64 from the f32 G; winner is the
    first index at the minimum."""
    G = np.asarray(G)
    assert G.dtype == np.float32
    combos = np.asarray(combos, dtype=np.int64)
    C, m = combos.shape
    Gd = G.astype(np.float64)
    H = np.eye(m) - np.full((m, m), 1.0 / m)
    lam = np.empty(C)
    step = max(1, _CHUNK_ELEMS // (m * m))
    for lo in range(0, C, step):
        c = combos[lo : lo + step]
        sub = Gd[c[:, :, None], c[:, None, :]]
        lam[lo : lo + step] = np.linalg.eigvalsh(H @ sub @ H)[:, -1]
    return lam, int(np.argmin(lam))


def smea_centred(G, rows):
    """H G_S H in float64 for one subset."""
    rows = np.asarray(rows, dtype=np.int64)
    m = rows.size
    H = np.eye(m) - np.full((m, m), 1.0 / m)
    return H @ np.asarray(G, dtype=np.float64)[np.ix_(rows, rows)] @ H


def all_combos(n, m):
    return np.array(list(itertools.combinations(range(n), m)), dtype=np.int32).reshape(-1, m)


# ---------------------------------------------------------------------------
# MDA inputs: every family is symmetric f32 with a zero diagonal
# ---------------------------------------------------------------------------


def _sym(U):
    D2 = np.triu(U, 1)
    return (D2 + D2.T).astype(np.float32)


def _rng(n, f, salt):
    return np.random.default_rng(100_003 * n + 101 * f + salt)


def mda_small_ints(n, f):
    """Entries in {1, 2, 3}: many exact ties."""
    return _sym(_rng(n, f, 1).integers(1, 4, size=(n, n)).astype(np.float32))


def planted_rows(n, m, salt=2):
    """m sorted rows that are not the first m (needs m < n)."""
    assert m < n
    rng = np.random.default_rng(7919 * n + m + salt)
    while True:
        rows = np.sort(rng.choice(n, size=m, replace=False))
        if rows[0] != 0 or rows[-1] != m - 1:
            return rows


def mda_planted_clique(n, f):
    """Entries in {1, 2}; a clique of 1s on ``planted_rows(n, m)`` and 1s
    elsewhere with probability 0.3. Needs f >= 1."""
    m = n - f
    D2 = _sym(np.where(_rng(n, f, 2).random((n, n)) < 0.3, 1.0, 2.0))
    rows = planted_rows(n, m)
    D2[np.ix_(rows, rows)] = 1.0
    np.fill_diagonal(D2, 0.0)
    return D2


def mda_no_clique(n, f):
    """Entries in {1, 2} whose 1-edges form a star around one row: with
    m >= 3 no m-clique of 1s exists, the optimum is 2 and every subset ties."""
    assert n - f >= 3
    D2 = np.full((n, n), 2.0, dtype=np.float32)
    hub = n // 2
    D2[hub, :] = 1.0
    D2[:, hub] = 1.0
    np.fill_diagonal(D2, 0.0)
    return D2


def mda_zeros(n, f):
    return np.zeros((n, n), dtype=np.float32)


def mda_duplicated_rows(n, f):
    """Squared distances of points of which only about n / 3 are distinct."""
    rng = _rng(n, f, 3)
    k = max(2, n // 3)
    pts = rng.integers(-4, 5, size=(k, 3)).astype(np.float32)[rng.integers(0, k, size=n)]
    diff = pts[:, None, :] - pts[None, :, :]
    return (diff * diff).sum(axis=2).astype(np.float32)  # small integers: exact


def mda_inf_row(n, f):
    """``mda_small_ints`` with one row at +inf from all the others."""
    D2 = mda_small_ints(n, f)
    r = (2 * n) // 3
    D2[r, :] = np.inf
    D2[:, r] = np.inf
    D2[r, r] = 0.0
    return D2


def mda_all_inf(n, f):
    D2 = np.full((n, n), np.inf, dtype=np.float32)
    np.fill_diagonal(D2, 0.0)
    return D2


# name -> (builder, applies(n, f)); the Gaussian family needs the device and
# lives with the GPU tests
MDA_FAMILIES = {
    "small_ints": (mda_small_ints, lambda n, f: True),
    "planted_clique": (mda_planted_clique, lambda n, f: f >= 1),
    "no_clique": (mda_no_clique, lambda n, f: n - f >= 3),
    "zeros": (mda_zeros, lambda n, f: True),
    "duplicated_rows": (mda_duplicated_rows, lambda n, f: True),
    "inf_row": (mda_inf_row, lambda n, f: True),
    "all_inf": (mda_all_inf, lambda n, f: True),
}

# (n, f), each the smallest that reaches its path in mda_dfs_kernel
MDA_SHAPES = [
    (5, 2), (7, 3),                      # P == 2, m >= 3
    (6, 4), (9, 7), (64, 62),            # m == 2
    (8, 5), (12, 9), (64, 61),           # m == 3 under P == 3 (need == 0); 41664 prefixes stride
    (47, 1), (48, 1), (64, 1), (64, 2),  # m = n - 1, n - 2 around the 16384-block cap
    (10, 3), (16, 4), (20, 6), (19, 8),  # mid-depth
]
MDA_F0_SHAPE = (9, 0)  # through the binding only: the dispatcher never searches at f = 0


def mda_planted_64_16():
    """(D2, rows): n = 64, f = 16, out of brute force's reach. 48 planted rows
    with pairwise D2 in [0.5, 1] and 16 rows at D2 in [100, 200] from
    everything, so ``rows`` is the unique optimum by construction."""
    return _planted_cluster(64, planted_rows(64, 48), np.random.default_rng(6416))


def _planted_cluster(n, rows, rng):
    D2 = _sym(100.0 + 100.0 * rng.random((n, n)))
    inner = _sym(0.5 + 0.5 * rng.random((n, n)))
    D2[np.ix_(rows, rows)] = inner[np.ix_(rows, rows)]
    np.fill_diagonal(D2, 0.0)
    return D2, tuple(int(r) for r in rows)


# A search that gives a node up only when too few POSITIONS are left, not too
# few viable rows, walks the subsets of a planted cluster that is a row short.
# On 48 of 64 it does not come back; on a smaller cluster it is merely slow.
# Measured before and after the searches counted viable rows: mda_search on
# 30 of 40, 1.6 s and 0.8 ms; the pure-Python DFS on 27 of 36, 4.3 s and 8 ms.
# A test that runs a host search on a planted case first holds that search to
# this wall time on its small case, and so fails there instead of hanging.
PLANTED_GUARD_SECONDS = 0.2
PLANTED_GUARD_NATIVE = (40, 30)
PLANTED_GUARD_PYTHON = (36, 27)


def mda_planted_small(n, m):
    """(D2, rows): as ``mda_planted_64_16`` with m planted rows of n."""
    rng = np.random.default_rng(100 * n + m)
    return _planted_cluster(n, np.sort(rng.choice(n, size=m, replace=False)), rng)


# ---------------------------------------------------------------------------
# SMEA inputs
# ---------------------------------------------------------------------------


def smea_rows(n, m, d=96, seed=0, tight=None, push=(3.0, 1.5)):
    """(n, d) f32 rows: m tight rows (unit-variance noise around a common
    mean) at ``tight`` (default: a seeded choice) and n - m outliers pushed
    out along their own directions by graded amounts push[0] + k push[1], so
    the oracle's winner is the tight set. The default push leaves a gap of
    several hundred percent to the runner-up; a push well below the noise's
    own norm of 1 leaves a few percent, where a wrong eigenvalue moves the
    winner."""
    rng = np.random.default_rng(1000 * n + m + seed)
    X = rng.standard_normal((n, d)) / math.sqrt(d) + 0.5 / math.sqrt(d)
    if tight is None:
        tight = np.sort(rng.choice(n, size=m, replace=False))
    out = np.setdiff1d(np.arange(n), np.asarray(tight))
    for k, r in enumerate(out):
        u = rng.standard_normal(d)
        X[r] += (push[0] + push[1] * k) * u / np.linalg.norm(u)
    return X.astype(np.float32)


def gram_f32(X):
    X = np.asarray(X, dtype=np.float32)
    return (X.astype(np.float64) @ X.astype(np.float64).T).astype(np.float32)


def relative_gap(lam):
    s = np.sort(lam)
    return float((s[1] - s[0]) / s[0])
