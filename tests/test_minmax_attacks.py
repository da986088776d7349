"""Min-Max / Min-Sum attacks (Shejwalkar & Houmansadr 2021) on CPU: the
functional oracle (bisection), the closed-form gamma helpers of
hip/dispatch.py and the operator classes. Every property is recomputed here
from explicit f64 differences, independently of both implementations."""
import pytest
import torch

from byzpy_amd.attacks import MinMaxAttack, MinSumAttack
from byzpy_amd.hip import dispatch as D
from byzpy_amd.ops import functional as F

SHAPES = [(5, 33), (8, 64), (23, 2050), (64, 4097), (100, 777)]
PERTURBATIONS = ["unit", "std", "sign"]
ATTACKS = {"min_max": (D.min_max, F.min_max_gamma), "min_sum": (D.min_sum, F.min_sum_gamma)}


def _honest(n, d):
    """Rows of growing scale around a non-zero mean, in permuted order:
    unpermuted or zero-mean inputs would let a wrong sign or row pass."""
    g = torch.Generator().manual_seed(100 * n + d)
    X = torch.randn(n, d, generator=g) * (1 + 0.1 * torch.arange(n))[:, None] + 0.3
    return X[torch.randperm(n, generator=g)].contiguous()


_INPUTS = {s: _honest(*s) for s in SHAPES}
_D2 = {}


def _pairwise(shape):
    """(n, n) explicit f64 squared distances, computed once per shape."""
    if shape not in _D2:
        H = _INPUTS[shape].double()
        _D2[shape] = torch.stack([((H - H[i]) ** 2).sum(dim=1) for i in range(len(H))])
    return _D2[shape]


def _bound_and_value(attack, shape, m):
    """The attack's bound on the honest rows and the constraint value of m."""
    H = _INPUTS[shape].double()
    dist = ((m.double()[None, :] - H) ** 2).sum(dim=1)
    D2 = _pairwise(shape)
    if attack == "min_max":
        return float(D2.max()), float(dist.max())
    return float(D2.sum(dim=1).max()), float(dist.sum())


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("perturbation", PERTURBATIONS)
@pytest.mark.parametrize("attack", sorted(ATTACKS))
def test_feasible_and_tight(attack, perturbation, shape):
    X = _INPUTS[shape]
    m = ATTACKS[attack][0](X, perturbation)
    assert m.shape == (shape[1],) and m.dtype == X.dtype
    bound, value = _bound_and_value(attack, shape, m)
    print(f"{attack} {perturbation} {shape}: value/bound - 1 = {value / bound - 1:.3e}")
    assert value <= bound * (1 + 1e-5)  # inside the cloud
    assert value >= bound * (1 - 1e-4)  # and gamma is maximal, not merely feasible


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("perturbation", PERTURBATIONS)
def test_min_sum_lands_at_the_farthest_row_distance(perturbation, shape):
    X = _INPUTS[shape]
    mu = X.double().mean(dim=0)
    m = D.min_sum(X, perturbation).double()
    far = (X.double() - mu[None, :]).norm(dim=1).max()
    assert float((m - mu).norm()) == pytest.approx(float(far), rel=1e-5)


def _degenerate_cases():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(64, generator=g) + 0.3
    const_cols = torch.arange(64, dtype=torch.float32)[None, :].repeat(8, 1) * 0.25
    return [
        ("identical_rows", x[None, :].repeat(8, 1), PERTURBATIONS),
        ("one_row", x[None, :].clone(), PERTURBATIONS),
        ("x_and_minus_x", torch.stack([x, -x]), ["unit", "sign"]),
        ("constant_columns", const_cols, ["std"]),
    ]


DEGENERATE = [
    (name, X, p) for name, X, perts in _degenerate_cases() for p in perts
]


@pytest.mark.parametrize("attack", sorted(ATTACKS))
@pytest.mark.parametrize(
    "name,X,perturbation", DEGENERATE, ids=[f"{c[0]}-{c[2]}" for c in DEGENERATE]
)
def test_degenerate_inputs_return_the_mean(name, X, perturbation, attack):
    m = ATTACKS[attack][0](X, perturbation)
    assert torch.isfinite(m).all()
    assert torch.equal(m, X.double().mean(dim=0).to(X.dtype))


@pytest.mark.parametrize("cls", [MinMaxAttack, MinSumAttack])
def test_operator_plumbing(cls):
    X = _INPUTS[(8, 64)]
    fn = D.min_max if cls is MinMaxAttack else D.min_sum
    op = cls()
    assert op.uses_honest_grads and op.perturbation == "std"
    assert cls.name == ("attack/min-max" if cls is MinMaxAttack else "attack/min-sum")
    from_list = op.apply(honest_grads=[X[i] for i in range(len(X))])
    from_matrix = op.apply(honest_grads=X)
    assert from_list.shape == from_matrix.shape == (64,)
    assert from_list.dtype == torch.float32
    assert torch.equal(from_list, fn(X, "std")) and torch.equal(from_matrix, from_list)
    shaped = cls("sign").apply(honest_grads=[X[i].reshape(8, 8) for i in range(len(X))])
    assert shaped.shape == (8, 8)
    assert torch.equal(shaped.reshape(-1), fn(X, "sign"))
    Xb = X.to(torch.bfloat16)
    out = cls("unit").apply(honest_grads=[Xb[i] for i in range(len(Xb))])
    assert out.dtype == torch.bfloat16 and out.shape == (64,)
    assert torch.equal(out, fn(Xb, "unit"))
    with pytest.raises(ValueError):
        cls("variance")
    with pytest.raises(ValueError):
        fn(X, "variance")
    with pytest.raises(ValueError):
        F.attack_perturbation(X, "variance")


def test_cli_lists_the_new_attacks(capsys):
    from byzpy_amd import cli

    assert cli.main(["list", "attacks"]) == 0
    out = capsys.readouterr().out
    assert "MinMaxAttack" in out and "MinSumAttack" in out


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("perturbation", PERTURBATIONS)
def test_closed_form_gamma_matches_bisection(perturbation, shape):
    X = _INPUTS[shape]
    H = X.double()
    mu, p = F.attack_perturbation(X, perturbation)
    diff = mu[None, :] - H
    a = (diff * diff).sum(dim=1)
    b = (diff * p[None, :]).sum(dim=1)
    c = (p * p).sum()
    D2 = _pairwise(shape)
    g_max = D.min_max_gamma(a, b, c, D2.max())
    g_sum = D.min_sum_gamma(a, c)
    assert g_max.dtype == torch.float64 and g_max.dim() == 0
    assert float(g_max) == pytest.approx(F.min_max_gamma(X, perturbation), rel=1e-6)
    assert float(g_sum) == pytest.approx(F.min_sum_gamma(X, perturbation), rel=1e-6)


def test_closed_form_gamma_degenerate_terms():
    z = torch.zeros(4, dtype=torch.float64)
    zero, one = torch.tensor(0.0, dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64)
    # c = 0: no direction to move in
    assert float(D.min_max_gamma(z + 1.0, z, zero, one * 4)) == 0.0
    assert float(D.min_sum_gamma(z + 1.0, zero)) == 0.0
    # tau = a_i, b_i = 0: 0 / 0 in the cancellation-free form must give 0
    assert float(D.min_max_gamma(z, z, one, zero)) == 0.0
    # b_i < 0 with tau = a_i: the row allows gamma up to -2 b_i / c
    b = torch.tensor([-1.0, -3.0], dtype=torch.float64)
    assert float(D.min_max_gamma(z[:2] + 2.0, b, one * 2, one * 2)) == pytest.approx(1.0)
