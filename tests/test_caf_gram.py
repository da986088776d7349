"""CAF on the Gram (K21) without a device: F.caf_gram in f64 against the plain
d-space filter loop, and the CPU route of CAF(solver="gram")."""
import math

import pytest
import torch

from byzpy_amd import hip
from byzpy_amd.aggregators import CAF
from byzpy_amd.hip import dispatch as D
from byzpy_amd.ops import functional as F


def dspace_caf(Xd, f, seeds, power_iters):
    """F.caf's loop in f64 on the rows without inf / NaN, started from
    v0 = seeds[r] @ Y (Y the centred rows), not a d-long draw: (mu, rounds)."""
    n = Xd.shape[0]
    live = torch.isfinite(Xd).all(dim=1)
    X, S = Xd[live], seeds.double()[:, live]
    w = torch.ones(X.shape[0], dtype=torch.float64)
    best_lambda, best_mu, rounds = math.inf, X.mean(dim=0), 0
    for r in range(n):
        rounds += 1
        wsum = w.sum()
        mu = (w[:, None] * X).sum(dim=0) / wsum
        Y = X - mu
        v = S[r] @ Y
        v = v / v.norm().clamp_min(1e-20)
        for _ in range(max(1, power_iters)):
            t = (w * (Y @ v)) @ Y / wsum
            lam = t.norm()
            v = t / lam.clamp_min(1e-20)
        if lam < best_lambda:
            best_lambda, best_mu = lam, mu
        proj = (Y @ v) ** 2
        w_next = (w * (1.0 - proj / proj.max().clamp_min(1e-20))).clamp_min(0.0)
        if wsum <= n - 2 * f or w_next.sum() <= 0:
            break
        w = w_next
    return best_mu, rounds


def _rows(n, d=256):
    X = torch.randn(n, d, generator=torch.Generator().manual_seed(n), dtype=torch.float64)
    X[: n // 4] += 3.0 * torch.ones(d, dtype=torch.float64)
    return X


@pytest.mark.parametrize("power_iters", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 17, 64])
@pytest.mark.parametrize("half", [False, True])
def test_caf_gram_matches_the_d_space_loop(half, n, power_iters):
    Xd, f = _rows(n), (n - 1) // 2 if half else 0
    seeds = F.caf_gram_seeds(n)
    a, lam, rounds = F.caf_gram(Xd @ Xd.T, f, seeds, power_iters=power_iters)
    ref, ref_rounds = dspace_caf(Xd, f, seeds, power_iters)
    assert rounds == ref_rounds
    assert (a @ Xd - ref).abs().max() <= 1e-9 * ref.abs().max()
    if f == 0:  # the first round already meets the target: the plain mean
        assert rounds == 1 and torch.equal(a, torch.full((n,), 1.0 / n, dtype=torch.float64))


def test_public_class_validation_and_cpu_route():
    with pytest.raises(ValueError):
        CAF(1, solver="newton")
    with pytest.raises(ValueError):
        D.caf(_rows(5), 1, solver="newton")
    with pytest.raises(ValueError):
        D.caf(_rows(4), 2, solver="gram")
    assert CAF(1).solver == "iterative"
    X = _rows(17).float()
    out = CAF(4, solver="gram").aggregate(X)
    ref, _ = dspace_caf(X.double(), 4, F.caf_gram_seeds(17), 3)
    assert (out.double() - ref).abs().max() <= 2.0**-23 * ref.abs().max()
    rows = [r.clone() for r in X]
    assert torch.equal(CAF(4, solver="gram").aggregate(rows), out)


def test_the_gram_overload_refuses_cpu_tensors():
    with pytest.raises(RuntimeError):
        hip.require().caf_matvec(torch.eye(4), F.caf_gram_seeds(4), f=1, power_iters=3)
