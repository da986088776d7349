"""Byzantine attacks.

Reference parity: attacks/{empire,sign_flip,label_flip,little,gaussian,
inf,mimic}.py. All are cheap elementwise/reduction math; on GPU they run
as device torch ops over the resident honest-gradient matrix (single
launches — no fan-out needed). Min-Max and Min-Sum have no
reference counterpart.
"""
from __future__ import annotations

from typing import Any, Dict, Optional

import torch
from torch import nn

from byzpy_amd.attacks.base import Attack
from byzpy_amd.hip import dispatch as D
from byzpy_amd.ops import functional as F
from byzpy_amd.utils.flatten import to_like


class EmpireAttack(Attack):
    """scale * mean(honest gradients) (inner-product-manipulation analogue)."""

    name = "attack/empire"
    uses_honest_grads = True

    def __init__(self, scale: float = -1.0, *, chunk_size: int = 8) -> None:
        self.scale = float(scale)
        self.chunk_size = int(chunk_size)

    def apply(self, *, honest_grads: Any) -> Any:
        X, like = self._stack(honest_grads)
        return to_like(F.empire(X, self.scale), like)


class SignFlipAttack(Attack):
    """scale * base_grad (default -1: flipped sign)."""

    name = "attack/sign-flip"
    uses_base_grad = True

    def __init__(self, scale: float = -1.0, *, chunk_size: int = 8192) -> None:
        self.scale = float(scale)
        self.chunk_size = int(chunk_size)

    def apply(self, *, base_grad: Any) -> Any:
        X, like = self._stack([base_grad])
        return to_like(X[0] * self.scale, like)


class LittleAttack(Attack):
    """'A Little Is Enough' (Baruch et al. 2019): mu + z * sigma with
    s = floor(N/2)+1-f and z = Phi^{-1}((N-s)/N)."""

    name = "attack/little"
    uses_honest_grads = True

    def __init__(
        self, f: int, N: Optional[int] = None, *, chunk_size: int = 8192
    ) -> None:
        if f < 0:
            raise ValueError("f must be >= 0")
        self.f = int(f)
        self.N = None if N is None else int(N)
        self.chunk_size = int(chunk_size)

    def apply(self, *, honest_grads: Any) -> Any:
        X, like = self._stack(honest_grads)
        return to_like(D.little(X, self.f, self.N), like)


class _CloudBoundAttack(Attack):
    """mu + gamma * p with the largest gamma that keeps the vector inside the
    honest cloud (Shejwalkar & Houmansadr 2021); subclasses name the bound.
    ``perturbation``: "unit" (-mu/||mu||), "std" (-sigma, the paper's
    default) or "sign" (-sign(mu))."""

    uses_honest_grads = True
    _op = None  # dispatch function (X, perturbation) -> (d,)

    def __init__(self, perturbation: str = "std", *, chunk_size: int = 8192) -> None:
        D._perturb_code(perturbation)  # ValueError on an unknown name
        self.perturbation = perturbation
        self.chunk_size = int(chunk_size)

    def apply(self, *, honest_grads: Any) -> Any:
        X, like = self._stack(honest_grads)
        return to_like(type(self)._op(X, self.perturbation), like)


class MinMaxAttack(_CloudBoundAttack):
    """Min-Max: max_i ||m - x_i|| stays within the largest honest pairwise
    distance."""

    name = "attack/min-max"
    _op = staticmethod(D.min_max)


class MinSumAttack(_CloudBoundAttack):
    """Min-Sum: sum_i ||m - x_i||^2 stays within the largest such sum of an
    honest row."""

    name = "attack/min-sum"
    _op = staticmethod(D.min_sum)


class AGRTailoredAttack(Attack):
    """Aggregator-tailored attack (Shejwalkar & Houmansadr 2021): the f
    Byzantine workers all send mu + gamma * p with the largest gamma for
    which ``agr`` ("krum", "multi-krum" with ``q`` winners, default all
    honest rows' count, or "bulyan"), run with parameter f on the honest
    gradients plus those f copies, still selects them."""

    name = "attack/agr-tailored"
    uses_honest_grads = True

    def __init__(
        self,
        f: int,
        agr: str = "multi-krum",
        *,
        q: Optional[int] = None,
        perturbation: str = "std",
        chunk_size: int = 8192,
    ) -> None:
        if f < 1:
            raise ValueError("f must be >= 1")
        if agr not in F.AGR_RULES:
            raise ValueError(f"agr must be one of {F.AGR_RULES}, got {agr!r}")
        if q is not None and q < 1:
            raise ValueError("q must be >= 1")
        D._perturb_code(perturbation)  # ValueError on an unknown name
        self.f = int(f)
        self.agr = agr
        self.q = None if q is None else int(q)
        self.perturbation = perturbation
        self.chunk_size = int(chunk_size)

    def apply(self, *, honest_grads: Any) -> Any:
        X, like = self._stack(honest_grads)
        out = D.agr_tailored(X, self.f, self.agr, self.q, self.perturbation)
        return to_like(out, like)


class CoordinateTailoredAttack(Attack):
    """Tailored attack on the coordinate-wise rules (Shejwalkar & Houmansadr
    2021): the f Byzantine workers all send mu + gamma * p with the gamma
    that moves ``agr`` ("trimmed-mean" or "median"), run on the honest
    gradients plus those f copies, farthest from the honest mean."""

    name = "attack/agr-coordinate"
    uses_honest_grads = True

    def __init__(
        self,
        f: int,
        agr: str = "trimmed-mean",
        *,
        perturbation: str = "std",
        chunk_size: int = 8192,
    ) -> None:
        if f < 1:
            raise ValueError("f must be >= 1")
        if agr not in F.AGR_COORD_RULES:
            raise ValueError(f"agr must be one of {F.AGR_COORD_RULES}, got {agr!r}")
        D._perturb_code(perturbation)  # ValueError on an unknown name
        self.f = int(f)
        self.agr = agr
        self.perturbation = perturbation
        self.chunk_size = int(chunk_size)

    def apply(self, *, honest_grads: Any) -> Any:
        X, like = self._stack(honest_grads)
        return to_like(D.agr_coord(X, self.f, self.agr, self.perturbation), like)


class GaussianAttack(Attack):
    """iid N(mu, sigma^2) noise vector; seedable for determinism."""

    name = "attack/gaussian"
    uses_honest_grads = True

    def __init__(
        self,
        mu: float = 0.0,
        sigma: float = 1.0,
        *,
        seed: Optional[int] = None,
        chunk_size: int = 8192,
    ) -> None:
        if sigma < 0:
            raise ValueError("sigma must be >= 0")
        self.mu, self.sigma = float(mu), float(sigma)
        self.seed = seed
        self.chunk_size = int(chunk_size)

    def apply(self, *, honest_grads: Any) -> Any:
        X, like = self._stack(honest_grads)
        return to_like(D.gaussian_attack(X, self.mu, self.sigma, self.seed), like)


class InfAttack(Attack):
    """All-infinity vector."""

    name = "attack/inf"
    uses_honest_grads = True

    def __init__(self, *, chunk_size: int = 8192) -> None:
        self.chunk_size = int(chunk_size)

    def apply(self, *, honest_grads: Any) -> Any:
        X, like = self._stack(honest_grads)
        return to_like(F.inf_attack(X), like)


class MimicAttack(Attack):
    """Copy honest worker #epsilon's vector."""

    name = "attack/mimic"
    uses_honest_grads = True

    def __init__(self, epsilon: int = 0, *, chunk_size: int = 8192) -> None:
        if epsilon < 0:
            raise ValueError("epsilon must be >= 0")
        self.epsilon = int(epsilon)
        self.chunk_size = int(chunk_size)

    def apply(self, *, honest_grads: Any) -> Any:
        X, like = self._stack(honest_grads)
        return to_like(F.mimic(X, self.epsilon), like)


class LabelFlipAttack(Attack):
    """Gradient of the loss on flipped labels (mirror K-1-y or explicit
    mapping); runs a forward+backward on the provided model."""

    name = "attack/label-flip"
    uses_model_batch = True

    def __init__(
        self,
        *,
        num_classes: Optional[int] = None,
        mapping: Optional[Dict[int, int]] = None,
        loss_fn: Optional[nn.Module] = None,
        scale: float = 1.0,
    ) -> None:
        if mapping is None and num_classes is None:
            raise ValueError("Provide either `mapping` or `num_classes`.")
        self.num_classes = num_classes
        self.mapping = mapping
        self.loss_fn = loss_fn or nn.CrossEntropyLoss(reduction="mean")
        self.scale = float(scale)

    def _flip(self, y: torch.Tensor) -> torch.Tensor:
        if self.mapping is not None:
            flipped = y.clone()
            for src, dst in self.mapping.items():
                flipped[y == src] = dst
            return flipped
        return (self.num_classes - 1) - y

    def apply(self, *, model: nn.Module, batch: Any) -> Any:
        x, y = batch
        flipped = self._flip(y)
        model.zero_grad(set_to_none=True)
        loss = self.loss_fn(model(x), flipped) * self.scale
        grads = torch.autograd.grad(loss, [p for p in model.parameters() if p.requires_grad])
        return torch.cat([g.reshape(-1) for g in grads])
