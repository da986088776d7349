"""Aggregator-tailored attacks on the CPU: the functional oracle (explicit
attacked matrix, bisection), the closed-form scores and the batched grid
search of hip/dispatch.py against it, the attack's effect on Krum, Multi-Krum
and Bulyan, degenerate inputs, argument checks and the operator class."""
import functools

import pytest
import torch

from byzpy_amd.attacks import AGRTailoredAttack
from byzpy_amd.hip import dispatch as D
from byzpy_amd.ops import functional as F

PERTURBATIONS = ["unit", "std", "sign"]
RULES = ["krum", "multi-krum", "bulyan"]

# (n, f, d): Bulyan at its minimum N = 4f + 3 with an odd d, just above it,
# and a wider case
SMALL = [(9, 2, 33), (11, 2, 300), (23, 5, 2050)]


@pytest.fixture(scope="module", autouse=True)
def _one_torch_thread():
    """The oracle is thousands of tiny CPU ops in Python loops: intra-op
    threads only add wake-ups to them, and whatever ran earlier in the
    process may have left torch with more threads than there are CPUs."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


@functools.lru_cache(maxsize=None)
def _case(n, d):
    """As test_gpu_minmax_attacks._case, on the CPU in f64 (of f32 values)."""
    g = torch.Generator().manual_seed(100 * n + d)
    X = torch.randn(n, d, generator=g) * (1 + 0.1 * torch.arange(n))[:, None] + 0.3
    return X[torch.randperm(n, generator=g)].contiguous().double()


@functools.lru_cache(maxsize=None)
def _gamma(n, f, d, agr, perturbation):
    return F.agr_tailored_gamma(_case(n, d), f, agr, None, perturbation)


@functools.lru_cache(maxsize=None)
def _terms(n, d, perturbation):
    """Honest Gram and the statistics a, b, c, all f64."""
    H = _case(n, d)
    _, _, a, b, c = F._attack_terms(H, perturbation)
    return H @ H.T, a, b, torch.tensor(c, dtype=torch.float64)


@pytest.mark.parametrize("n,f,d", SMALL)
@pytest.mark.parametrize("perturbation", PERTURBATIONS)
@pytest.mark.parametrize("agr", RULES)
def test_feasible_set_is_one_interval_ending_at_gamma(n, f, d, agr, perturbation):
    """The precondition of every other test here: a coarse scan finds the
    feasible set to be [0, gamma*], and gamma* is its end to 1e-6."""
    H = _case(n, d)
    gs = _gamma(n, f, d, agr, perturbation)
    assert gs > 0.0
    for k in range(0, 25):
        g = gs * k / 12.0  # 0 .. 2 gamma*, gamma* itself at k = 12
        want = k <= 12
        if k == 12:
            g = gs * (1.0 - 1e-9)
        assert F.agr_feasible(H, g, f, agr, None, perturbation) == want, (k, g)
    assert F.agr_feasible(H, gs * (1.0 - 1e-6), f, agr, None, perturbation)
    assert not F.agr_feasible(H, gs * (1.0 + 1e-6), f, agr, None, perturbation)


def _exact_case():
    """Integer data on which f32 arithmetic is exact: 9 rows of 12 entries in
    [-3, 3], the last row set so that every column mean is +1 or -1. With the
    "sign" perturbation and an integer gamma the malicious row is integer
    too, every squared distance stays below 2^24, and F.multi_krum_scores
    (which forms an f32 Gram) makes no rounding error at all."""
    g = torch.Generator().manual_seed(3)
    n, d = 9, 12
    X = torch.randint(-3, 4, (n, d), generator=g).double()
    k = torch.where(torch.rand(d, generator=g) < 0.5, -1.0, 1.0).double()
    X[n - 1] = n * k - X[: n - 1].sum(dim=0)
    assert torch.equal(X.mean(dim=0), k)
    return X


@pytest.mark.parametrize("f", [1, 2, 4])
def test_closed_form_scores_equal_multi_krum_scores_exactly_representable(f):
    """Closed-form scores against F.multi_krum_scores on the explicit
    attacked matrix, rtol 1e-9. multi_krum_scores casts to f32 inside, so
    that bound can only hold where f32 is exact: see _exact_case."""
    H = _exact_case()
    n = H.shape[0]
    _, _, a, b, c = F._attack_terms(H, "sign")
    gammas = torch.tensor([0.0, 1.0, 2.0, 5.0], dtype=torch.float64)
    hs, ms = D.agr_krum_scores(H @ H.T, a, b, torch.tensor(c).double(), f, gammas)
    for k, g in enumerate(gammas.tolist()):
        ref = F.multi_krum_scores(F._agr_attacked(H, g, f, "sign"), f).double()
        assert torch.allclose(hs[k], ref[:n], rtol=1e-9, atol=0.0)
        assert torch.allclose(ms[k].expand(f), ref[n:], rtol=1e-9, atol=0.0)


@pytest.mark.parametrize("n,f,d", SMALL)
@pytest.mark.parametrize("perturbation", PERTURBATIONS)
def test_closed_form_scores_equal_explicit_scores(n, f, d, perturbation):
    """On the suite's inputs: rtol 1e-9 against the same definition carried
    out in f64 on explicit differences of the attacked matrix, and the f32
    bound d * 2^-24 (worst-case f32 Gram accumulation over d <= 2050 terms,
    1.2e-4) against F.multi_krum_scores itself."""
    H = _case(n, d)
    G, a, b, c = _terms(n, d, perturbation)
    gs = _gamma(n, f, d, "multi-krum", perturbation)
    gammas = torch.tensor([0.0, 0.5 * gs, gs, 3.0 * gs], dtype=torch.float64)
    hs, ms = D.agr_krum_scores(G, a, b, c, f, gammas)
    for k, g in enumerate(gammas.tolist()):
        A = F._agr_attacked(H, g, f, perturbation)
        D2 = F._pairwise_sq_dists_explicit(A)
        D2.fill_diagonal_(float("inf"))
        ref = torch.topk(D2, k=n - 1, dim=1, largest=False).values.sum(dim=1)
        assert torch.allclose(hs[k], ref[:n], rtol=1e-9, atol=0.0)
        assert torch.allclose(ms[k].expand(f), ref[n:], rtol=1e-9, atol=0.0)
        ref32 = F.multi_krum_scores(A, f).double()
        got = torch.cat([hs[k], ms[k].expand(f)])
        assert torch.allclose(got, ref32, rtol=d * 2.0**-24, atol=0.0)


@pytest.mark.parametrize("n,f,d", SMALL)
@pytest.mark.parametrize("perturbation", PERTURBATIONS)
@pytest.mark.parametrize("agr", ["krum", "multi-krum"])
def test_torch_composition_gamma_matches_oracle(n, f, d, agr, perturbation):
    G, a, b, c = _terms(n, d, perturbation)
    got = float(D.agr_tailored_gamma(G, a, b, c, f, agr))
    ref = _gamma(n, f, d, agr, perturbation)
    rel = abs(got - ref) / ref
    print(f"{agr} n={n} f={f} d={d} {perturbation}: {got:.6f} vs {ref:.6f}, rel {rel:.2e}")
    assert rel <= 2.0**-15
    # q is honoured: q winners against the default's n
    if agr == "multi-krum":
        fewer = float(D.agr_tailored_gamma(G, a, b, c, f, agr, q=f))
        ref_fewer = F.agr_tailored_gamma(_case(n, d), f, agr, f, perturbation)
        assert abs(fewer - ref_fewer) / ref_fewer <= 2.0**-15
        krum = _gamma(n, f, d, "krum", perturbation)
        assert abs(ref_fewer - krum) / krum <= 1e-12  # q <= f: Krum's condition


@pytest.mark.parametrize("n,f,d", SMALL)
@pytest.mark.parametrize("perturbation", PERTURBATIONS)
def test_attack_is_selected_by_the_rule_it_targets(n, f, d, perturbation):
    H = _case(n, d)
    idx = set(range(n, n + f))
    m = F.agr_tailored(H, f, "krum", None, perturbation)
    A = torch.cat([H, m[None, :].expand(f, -1)])
    assert torch.equal(F.krum(A, f), m)
    m = F.agr_tailored(H, f, "multi-krum", None, perturbation)
    A = torch.cat([H, m[None, :].expand(f, -1)])
    winners = torch.topk(F.multi_krum_scores(A, f), k=n, largest=False).indices
    assert idx <= set(winners.tolist())
    m = F.agr_tailored(H, f, "bulyan", None, perturbation)
    A = torch.cat([H, m[None, :].expand(f, -1)])
    assert idx <= set(F.bulyan_select(A, f).tolist())


def _degenerate_cases():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(64, generator=g) + 0.3
    const_cols = torch.arange(64, dtype=torch.float32)[None, :].repeat(8, 1) * 0.25
    return [
        ("identical_rows", x[None, :].repeat(8, 1), PERTURBATIONS),
        ("constant_columns", const_cols, ["std"]),
    ]


DEGENERATE = [(name, X, p) for name, X, perts in _degenerate_cases() for p in perts]


@pytest.mark.parametrize("agr", RULES)
@pytest.mark.parametrize(
    "name,X,perturbation", DEGENERATE, ids=[f"{c[0]}-{c[2]}" for c in DEGENERATE]
)
def test_degenerate_inputs_return_the_mean(name, X, perturbation, agr):
    mu = X.double().mean(dim=0).float()
    assert F.agr_tailored_gamma(X, 1, agr, None, perturbation) == 0.0
    assert torch.equal(F.agr_tailored(X, 1, agr, None, perturbation), mu)
    assert torch.equal(D.agr_tailored(X, 1, agr, None, perturbation), mu)
    if agr != "bulyan":
        H = X.double()
        _, _, a, b, c = F._attack_terms(H, perturbation)
        got = D.agr_tailored_gamma(H @ H.T, a, b, torch.tensor(c).double(), 1, agr)
        assert float(got) == 0.0


def test_non_finite_statistics_give_zero():
    G, a, b, c = _terms(9, 33, "std")
    for bad in (float("nan"), float("inf")):
        a2 = a.clone()
        a2[3] = bad
        assert float(D.agr_tailored_gamma(G, a2, b, c, 2, "krum")) == 0.0
        assert float(D.agr_tailored_gamma(G, a, b, c * bad, 2, "multi-krum")) == 0.0


def test_invalid_arguments_raise_value_error():
    H = _case(9, 33)
    G, a, b, c = _terms(9, 33, "std")
    for fn in (F.agr_tailored, F.agr_tailored_gamma, D.agr_tailored):
        for args in (
            (H, 0, "krum"),            # f >= 1
            (H, 2, "median"),          # unknown rule
            (H, 3, "bulyan"),          # n = 9 < 3f + 3 = 12
            (H, 10, "krum"),           # f > n
            (H, 2, "multi-krum", 0),   # q >= 1
            (H, 2, "multi-krum", 12),  # q <= n + f
            (H, 2, "krum", None, "variance"),
        ):
            with pytest.raises(ValueError):
                fn(*args)
    with pytest.raises(ValueError):
        F.agr_feasible(H, 1.0, 0, "krum")
    with pytest.raises(ValueError):
        D.agr_tailored_gamma(G, a, b, c, 0, "krum")
    with pytest.raises(ValueError):
        D.agr_tailored_gamma(G, a, b, c, 2, "trimmed-mean")
    # the statistics form of Bulyan exists on the device only
    with pytest.raises(ValueError):
        D.agr_tailored_gamma(G, a, b, c, 2, "bulyan")
    for kwargs in (
        dict(f=0),
        dict(f=2, agr="median"),
        dict(f=2, perturbation="variance"),
        dict(f=2, q=0),
    ):
        with pytest.raises(ValueError):
            AGRTailoredAttack(**kwargs)


def test_operator_accepts_a_list_and_a_matrix():
    X = _case(11, 300).float()
    assert AGRTailoredAttack.name == "attack/agr-tailored"
    assert AGRTailoredAttack.uses_honest_grads
    for agr in RULES:
        ref = F.agr_tailored(X, 2, agr, None, "sign")
        for grads in ([X[i] for i in range(len(X))], X):
            out = AGRTailoredAttack(2, agr, perturbation="sign").apply(honest_grads=grads)
            assert out.dtype == X.dtype and out.shape == (300,)
            assert torch.equal(out, ref)
    few = AGRTailoredAttack(2, q=2).apply(honest_grads=X)
    assert torch.equal(few, F.agr_tailored(X, 2, "multi-krum", 2, "std"))
    assert not torch.equal(few, AGRTailoredAttack(2).apply(honest_grads=X))
