"""Tailored attacks on the coordinate-wise rules, on the CPU: the functional
oracle (explicit attacked matrix, a sort per trial) against the batched torch
composition of hip/dispatch.py (the honest rows sorted once, clamps and the
kept-rank rule), an exact-arithmetic family on which the two must agree to
the bit, the maximisation schedule, additivity over column shards, degenerate
inputs, argument checks and the operator class."""
import functools

import pytest
import torch

from byzpy_amd.attacks import CoordinateTailoredAttack
from byzpy_amd.hip import dispatch as D
from byzpy_amd.ops import functional as F

PERTURBATIONS = ["unit", "std", "sign"]
RULES = ["trimmed-mean", "median"]

# (n, f): small, odd and even n + f, 2f < n, 2f >= n (10, 9), more copies
# than honest rows (7, 12: median only), n - f = f (64, 32), past the device
# kernel's row cap (65), a single row (median only)
RANDOM_NF = [(9, 1), (23, 7), (64, 15), (10, 9), (7, 12), (64, 32), (65, 5), (1, 1), (1, 3)]
# n - f a power of two: the trimmed mean's division is exact
EXACT_NF = [(9, 1), (20, 4), (23, 7), (47, 15), (64, 32)]
EXACT_D = 2050


def _valid(n, f, agr):
    return agr == "median" or f < n


RANDOM_CASES = [(n, f, agr) for n, f in RANDOM_NF for agr in RULES if _valid(n, f, agr)]
EXACT_CASES = [(n, f, agr) for n, f in EXACT_NF for agr in RULES]


@pytest.fixture(scope="module", autouse=True)
def _one_torch_thread():
    """The oracle is many small CPU ops in Python loops: intra-op threads only
    add wake-ups to them."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


@functools.lru_cache(maxsize=None)
def _random_case(n, d=257):
    """f32 values on a grid of 1/4, so that columns hold ties."""
    g = torch.Generator().manual_seed(1000 * n + d)
    X = torch.randn(n, d, generator=g) * (1 + 0.1 * torch.arange(n))[:, None] + 0.3
    return ((X * 4).round() / 4).contiguous()


@functools.lru_cache(maxsize=None)
def _exact_case(n, d=EXACT_D):
    """X integers in [-4, 4], mu multiples of 1/16 in [-4, 4], p in {-1, 0, 1},
    gammas k / 4: every step of the objective is exact in f32, and the f64
    sum of the squares (multiples of 2^-18 below 2^8, 2050 of them) is exact
    in any order."""
    g = torch.Generator().manual_seed(7 * n + 1)
    X = torch.randint(-4, 5, (n, d), generator=g).float()
    mu = torch.randint(-64, 65, (d,), generator=g).float() / 16
    p = torch.randint(-1, 2, (d,), generator=g).float()
    gammas = torch.arange(32).float() / 4
    return X, mu, p, gammas


@functools.lru_cache(maxsize=None)
def _exact_oracle(n, f, agr):
    X, mu, p, gammas = _exact_case(n)
    return torch.tensor(
        [F.agr_coord_objective(X, float(g), f, agr, mu=mu, p=p) for g in gammas],
        dtype=torch.float64,
    )


def _bits(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("n,f,agr", RANDOM_CASES)
@pytest.mark.parametrize("perturbation", PERTURBATIONS)
def test_composition_equals_oracle_on_random_data(n, f, agr, perturbation):
    """rtol 1e-12: both sides are f64 with sums of at most n + f terms per
    column and d = 257 squares."""
    X = _random_case(n)
    mu, p = F.attack_perturbation(X, perturbation)
    scale = float((X.double() - mu).abs().max()) / max(float(p.abs().max()), 1e-30)
    gammas = torch.tensor(
        [0.0, 1e-3 * scale, 0.1 * scale, 0.37 * scale, scale, 2.5 * scale, 1e3 * scale],
        dtype=torch.float64,
    )
    got = D.agr_coord_objective(X, mu, p, gammas, f, agr)
    assert got.dtype == torch.float64 and got.shape == (7,)
    ref = torch.tensor(
        [F.agr_coord_objective(X, float(g), f, agr, perturbation) for g in gammas],
        dtype=torch.float64,
    )
    assert torch.allclose(got, ref, rtol=1e-12, atol=0.0), (got, ref)
    # the trials do not all sit on one branch of the arithmetic
    assert len(set(ref.tolist())) > 1 or n == 1


@pytest.mark.parametrize("n,f,agr", EXACT_CASES)
def test_exact_family_is_self_checking_and_composition_is_bitwise(n, f, agr):
    X, mu, p, gammas = _exact_case(n)
    ref = _exact_oracle(n, f, agr)
    step32 = torch.tensor(
        [
            F.agr_coord_objective(X, float(g), f, agr, mu=mu, p=p, dtype=torch.float32)
            for g in gammas
        ],
        dtype=torch.float64,
    )
    assert torch.equal(_bits(step32), _bits(ref))
    got = D.agr_coord_objective(X, mu, p, gammas, f, agr)
    assert torch.equal(_bits(got), _bits(ref))
    assert len(set(ref.tolist())) > 8  # the family does move with gamma


@pytest.mark.parametrize("n,f,agr", EXACT_CASES)
def test_objective_is_additive_over_column_shards(n, f, agr):
    X, mu, p, gammas = _exact_case(n)
    h = 1027
    whole = D.agr_coord_objective(X, mu, p, gammas, f, agr)
    left = D.agr_coord_objective(X[:, :h].contiguous(), mu[:h], p[:h], gammas, f, agr)
    right = D.agr_coord_objective(X[:, h:].contiguous(), mu[h:], p[h:], gammas, f, agr)
    assert torch.equal(_bits(left + right), _bits(whole))


def test_composition_chunks_its_columns(monkeypatch):
    """More than one column chunk gives the same bits as one."""
    X, mu, p, gammas = _exact_case(23)
    for agr in RULES:
        one = D.agr_coord_objective(X, mu, p, gammas, 7, agr)
        monkeypatch.setattr(D, "_AGR_COORD_CHUNK_ELEMS", 1)
        many = D.agr_coord_objective(X, mu, p, gammas, 7, agr)
        monkeypatch.undo()
        assert torch.equal(_bits(one), _bits(many))


def _stats(X, mu, p):
    diff = mu.double()[None, :] - X.double()
    return (diff * diff).sum(dim=1), (p.double() * p.double()).sum()


@pytest.mark.parametrize("n,f,agr", EXACT_CASES)
@pytest.mark.parametrize("gamma0", [0.5, 2.0])
def test_schedule_matches_oracle_bitwise_on_exact_family(n, f, agr, gamma0):
    X, mu, p, _ = _exact_case(n)
    a, c = _stats(X, mu, p)
    ref = F.agr_coord_gamma(X, f, agr, gamma0=gamma0, mu=mu, p=p)
    got = D.agr_coord_gamma(X, mu, p, a, c, f, agr, gamma0=gamma0)
    assert got.dim() == 0
    assert float(got) == ref
    assert float(torch.tensor(ref).float()) == ref  # an f32 value


def _gaussian(n=23, d=300):
    g = torch.Generator().manual_seed(5)
    return torch.randn(n, d, generator=g).contiguous()


@pytest.mark.parametrize("agr,f", [("trimmed-mean", 5), ("median", 5)])
def test_smallest_gamma_wins_on_the_plateau(agr, f):
    """Symmetric data, "std": D rises to its plateau, which starts where the
    last column's v stops being kept: below the column's minimum for the
    trimmed mean, below the lower clamp sorted[(n + f - 1) // 2 - f] for the
    median, at edge = max_j (mu_j - bound_j) / sigma_j. Every point past it
    ties exactly, so the schedule returns the first one it has: within its
    final spacing, 3 / 33^2 of gamma, of edge."""
    X = _gaussian()
    n = X.shape[0]
    mu, p = F.attack_perturbation(X, "std")
    rank = 0 if agr == "trimmed-mean" else (n + f - 1) // 2 - f
    bound = X.double().sort(dim=0).values[rank]
    edge = float(((mu - bound) / (-p)).max())
    plateau = F.agr_coord_objective(X, 1e6 * edge, f, agr)
    for g in (F.agr_coord_gamma(X, f, agr), float(D.agr_coord_gamma(X, mu, p, *_stats(X, mu, p), f, agr))):
        assert F.agr_coord_objective(X, g, f, agr) == plateau
        assert edge <= g <= edge * 1.01
        for k in range(1, 40):  # and the plateau is the maximum
            assert F.agr_coord_objective(X, g * k / 40.0, f, agr) < plateau
    # a perturbation that moves nothing ties everywhere: gamma = 0
    zero_p = torch.zeros_like(p)
    assert F.agr_coord_gamma(X, f, agr, gamma0=1.0, p=zero_p) == 0.0
    a, _ = _stats(X, mu, p)
    got = D.agr_coord_gamma(X, mu, zero_p, a, torch.tensor(1.0), f, agr, gamma0=1.0)
    assert float(got) == 0.0


SKEWED = torch.tensor([100.0, 100.0, 100.0, 100.0, 0.0])


def test_maximiser_at_zero_and_strictly_inside():
    """The two inputs that make this a maximisation and not a boundary search;
    both conditions are asserted so the inputs cannot stop exercising them.

    Skewed column {100 x 4, 0}, f = 1, "std" (mu = 80, p = -40): the trimmed
    mean of the six values is (300 + clamp(v, 0, 100)) / 4, so |mu - A| is 15
    at gamma = 0, falls to 0 and ends at 5: gamma = 0 is the maximum.

    With that column moving slowly (p = -1) next to a symmetric column that
    moves fast (p = -100, past its range at gamma = 0.02), D peaks where the
    fast columns have just saturated and the slow ones have hardly begun to
    fall: strictly inside."""
    X = SKEWED[:, None].repeat(1, 64).contiguous()
    mu, p = F.attack_perturbation(X, "std")
    a, c = _stats(X, mu, p)
    assert F.agr_coord_gamma(X, 1, "trimmed-mean") == 0.0
    assert float(D.agr_coord_gamma(X, mu, p, a, c, 1, "trimmed-mean")) == 0.0
    d0 = F.agr_coord_objective(X, 0.0, 1, "trimmed-mean")
    assert d0 == 64 * 15.0**2
    assert all(F.agr_coord_objective(X, g, 1, "trimmed-mean") < d0 for g in (0.01, 0.5, 1.5, 2.0, 50.0))

    sym = torch.tensor([-2.0, -1.0, 0.0, 1.0, 2.0])
    X = torch.cat([SKEWED[:, None].repeat(1, 32), sym[:, None].repeat(1, 32)], dim=1).contiguous()
    mu = X.double().mean(dim=0)
    p = torch.cat([torch.full((32,), -1.0), torch.full((32,), -100.0)]).double()
    a, c = _stats(X, mu, p)
    ref = F.agr_coord_gamma(X, 1, "trimmed-mean", gamma0=1.0, mu=mu, p=p)
    got = float(D.agr_coord_gamma(X, mu, p, a, c, 1, "trimmed-mean", gamma0=1.0))
    plateau_from = 80.0  # the slow columns' v reaches 0
    for g in (ref, got):
        assert abs(g - 0.02) <= 0.02 * 0.01  # the grid point next to the peak
        dg = F.agr_coord_objective(X, g, 1, "trimmed-mean", mu=mu, p=p)
        assert dg > F.agr_coord_objective(X, 0.0, 1, "trimmed-mean", mu=mu, p=p)
        assert dg > F.agr_coord_objective(X, plateau_from, 1, "trimmed-mean", mu=mu, p=p)
        assert dg > F.agr_coord_objective(X, 2.0 * g, 1, "trimmed-mean", mu=mu, p=p)
        assert dg > F.agr_coord_objective(X, 0.5 * g, 1, "trimmed-mean", mu=mu, p=p)


@pytest.mark.parametrize("agr", RULES)
@pytest.mark.parametrize("perturbation", PERTURBATIONS)
def test_identical_rows_return_the_mean(perturbation, agr):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(64, generator=g) + 0.3
    X = x[None, :].repeat(8, 1)
    mu = X.double().mean(dim=0).float()
    assert F.agr_coord_gamma(X, 1, agr, perturbation) == 0.0
    assert torch.equal(F.agr_coord(X, 1, agr, perturbation), mu)
    assert torch.equal(D.agr_coord(X, 1, agr, perturbation), mu)


@pytest.mark.parametrize("agr", RULES)
def test_non_finite_statistics_give_zero(agr):
    X = _random_case(9)
    mu, p = F.attack_perturbation(X, "std")
    a, c = _stats(X, mu, p)
    assert float(D.agr_coord_gamma(X, mu, p, a, c, 2, agr)) > 0.0
    for bad in (float("nan"), float("inf")):
        a2 = a.clone()
        a2[3] = bad
        assert float(D.agr_coord_gamma(X, mu, p, a2, c, 2, agr)) == 0.0
        assert float(D.agr_coord_gamma(X, mu, p, a, c * bad, 2, agr)) == 0.0
    assert float(D.agr_coord_gamma(X, mu, p, a, c * 0.0, 2, agr)) == 0.0
    # and in the data: no error, a D that is not finite, gamma = 0
    Xb = X.clone()
    Xb[2, 5] = float("nan")
    assert F.agr_coord_gamma(Xb, 2, agr) == 0.0
    mub = mu.clone()
    mub[4] = float("inf")
    Dv = D.agr_coord_objective(X, mub, p, torch.tensor([0.0, 1.0]), 2, agr)
    assert not bool(torch.isfinite(Dv).any())


def _nonfinite_columns(n, f):
    """One-column problems (so that one bad column cannot hide the others)
    around values that are not finite or leave the f32 range: (label, X
    (n, 1), mu (1,), p (1,)), f32, and the trial gammas."""
    g = torch.Generator().manual_seed(31 * n + f)
    base = torch.randn(n, generator=g) + 0.3
    inf, nan = float("inf"), float("nan")

    def col(label, edits=(), p=-0.7, mu=None):
        x = base.clone()
        for i, val in edits:
            x[i] = val
        m = float(base.double().mean()) if mu is None else mu
        return label, x[:, None].contiguous(), torch.tensor([m]), torch.tensor([p])

    cols = [
        col("clean"),
        col("x +inf", [(0, inf)]),
        col("x -inf", [(1, -inf)]),
        col("x nan", [(2, nan)]),
        col("x f+1 +inf", [(i, inf) for i in range(f + 1)]),
        col("x f+1 -inf", [(i, -inf) for i in range(f + 1)]),
        col("x nan and +inf", [(0, inf), (1, nan)]),
        col("p -inf", p=-inf),
        col("p +inf", p=inf),
        col("p 1e30", p=1e30),
        col("p -1e30", p=-1e30),
        col("x -inf, p -inf", [(3, -inf)], p=-inf),
        col("x nan, p +inf", [(3, nan)], p=inf),
        col("mu nan", mu=nan),
        col("mu inf", mu=inf),
    ]
    gammas = torch.tensor([0.0, 0.5, 2.0, 1e30, nan])
    return cols, gammas


@pytest.mark.parametrize("agr", RULES)
@pytest.mark.parametrize("n,f", [(23, 7), (23, 8), (10, 9), (9, 1)])
def test_non_finite_values_rank_as_in_the_oracle(n, f, agr):
    """The composition against the oracle column by column: D is finite in
    exactly the same trials (a NaN ranks above +inf, as torch.sort has it; a
    dropped extreme does no harm, a kept one does), and equal where finite."""
    cols, gammas = _nonfinite_columns(n, f)
    seen = set()
    for label, X, mu, p in cols:
        got = D.agr_coord_objective(X, mu, p, gammas, f, agr)
        ref = torch.tensor(
            [F.agr_coord_objective(X, float(g), f, agr, mu=mu, p=p) for g in gammas],
            dtype=torch.float64,
        )
        fin = torch.isfinite(ref)
        assert torch.equal(torch.isfinite(got), fin), (label, got, ref)
        assert torch.allclose(got[fin], ref[fin], rtol=1e-12, atol=0.0), (label, got, ref)
        seen.update(fin.tolist())
    assert seen == {True, False}


def test_invalid_arguments_raise_value_error():
    X = _random_case(9)
    mu, p = F.attack_perturbation(X, "std")
    a, c = _stats(X, mu, p)
    g = torch.zeros(3)
    for args in (
        (0, "median"),         # f >= 1
        (2, "krum"),           # not a coordinate-wise rule
        (9, "trimmed-mean"),   # f < n
        (12, "trimmed-mean"),
    ):
        with pytest.raises(ValueError):
            F.agr_coord_check(9, *args)
        for fn in (F.agr_coord, F.agr_coord_gamma, D.agr_coord):
            with pytest.raises(ValueError):
                fn(X, *args)
        with pytest.raises(ValueError):
            F.agr_coord_objective(X, 1.0, *args)
        with pytest.raises(ValueError):
            D.agr_coord_objective(X, mu, p, g, *args)
        with pytest.raises(ValueError):
            D.agr_coord_gamma(X, mu, p, a, c, *args)
    F.agr_coord_check(9, 12, "median")  # any f >= 1
    for fn in (F.agr_coord, F.agr_coord_gamma, D.agr_coord):
        with pytest.raises(ValueError):
            fn(X, 2, "median", "variance")
    # the selection rules' checks still refuse the coordinate-wise names
    for agr in RULES:
        with pytest.raises(ValueError):
            F.agr_check(9, 2, agr)
    for kwargs in (
        dict(f=0),
        dict(f=2, agr="krum"),
        dict(f=2, perturbation="variance"),
    ):
        with pytest.raises(ValueError):
            CoordinateTailoredAttack(**kwargs)


def test_operator_accepts_a_list_and_a_matrix():
    X = _random_case(23)
    assert CoordinateTailoredAttack.name == "attack/agr-coordinate"
    assert CoordinateTailoredAttack.uses_honest_grads
    assert D.AGR_COORD_RULES == F.AGR_COORD_RULES == ("trimmed-mean", "median")
    assert D.AGR_COORD_MAX_N == 64
    for agr in RULES:
        ref = F.agr_coord(X, 5, agr, "sign")
        assert not torch.equal(ref, X.double().mean(dim=0).float())
        for grads in ([X[i] for i in range(len(X))], X):
            out = CoordinateTailoredAttack(5, agr, perturbation="sign").apply(honest_grads=grads)
            assert out.dtype == X.dtype and out.shape == (257,)
            assert torch.equal(out, ref)
    default = CoordinateTailoredAttack(5).apply(honest_grads=X)
    assert torch.equal(default, F.agr_coord(X, 5, "trimmed-mean", "std"))


def test_attack_moves_the_rule_further_than_the_untailored_attacks():
    """What the attack is for: on the rule it targets it does at least as
    much damage as Min-Max and Min-Sum, whose gammas lie on its schedule's
    axis (same mu and p)."""
    X = _gaussian()
    f = 5
    for agr in RULES:
        g = F.agr_coord_gamma(X, f, agr)
        best = F.agr_coord_objective(X, g, f, agr)
        for other in (F.min_max_gamma(X), F.min_sum_gamma(X)):
            assert best >= F.agr_coord_objective(X, other, f, agr)


def test_cli_lists_the_new_attack(capsys):
    from byzpy_amd import cli

    assert cli.main(["list", "attacks"]) == 0
    assert "CoordinateTailoredAttack" in capsys.readouterr().out
