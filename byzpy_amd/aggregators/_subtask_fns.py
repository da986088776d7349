"""Module-level (picklable) subtask functions for the CPU pool paths.

Each fn resolves its matrix reference (tensor view for thread pools, shm
handle for process pools), computes on a slice with the pure-torch
functional ops, and returns a small partial. Reference parity: the
per-aggregator ``_*_chunk`` fns in aggregators/*/*.py.
"""
from __future__ import annotations

from typing import Any, Tuple

import torch

from byzpy_amd.ops import functional as F
from byzpy_amd.storage.shared_store import close_ref, resolve_matrix


def median_chunk(ref: Any, lo: int, hi: int) -> torch.Tensor:
    X, c = resolve_matrix(ref)
    try:
        return F.median(X[:, lo:hi]).clone()
    finally:
        close_ref(c)


def trimmed_mean_chunk(ref: Any, lo: int, hi: int, f: int) -> torch.Tensor:
    X, c = resolve_matrix(ref)
    try:
        return F.trimmed_mean(X[:, lo:hi], f).clone()
    finally:
        close_ref(c)


def meamed_chunk(ref: Any, lo: int, hi: int, f: int) -> torch.Tensor:
    X, c = resolve_matrix(ref)
    try:
        return F.mean_of_medians(X[:, lo:hi], f).clone()
    finally:
        close_ref(c)


def row_sqnorm_chunk(ref: Any, lo: int, hi: int) -> torch.Tensor:
    """Partial per-row squared norms over feature slice [lo, hi)."""
    X, c = resolve_matrix(ref)
    try:
        Xf = X[:, lo:hi].float()
        return (Xf * Xf).sum(dim=1)
    finally:
        close_ref(c)


def gram_row_chunk(ref: Any, rlo: int, rhi: int) -> torch.Tensor:
    """Rows [rlo, rhi) of the Gram matrix X @ X.T (f32)."""
    X, c = resolve_matrix(ref)
    try:
        Xf = X.float()
        return Xf[rlo:rhi] @ Xf.T
    finally:
        close_ref(c)


def gram_feature_chunk(ref: Any, lo: int, hi: int) -> torch.Tensor:
    """Partial Gram contribution of feature slab [lo, hi) (NNM-style)."""
    X, c = resolve_matrix(ref)
    try:
        Xs = X[:, lo:hi].float()
        return Xs @ Xs.T
    finally:
        close_ref(c)


def dnc_gram_chunk(
    ref: Any, coords: torch.Tensor
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(partial centred Grams (niters, n, n), bad flags (niters, n)) of one
    chunk ``coords`` (niters, bc) of DnC's sampled coordinates. Centring is
    per column, so both are additive over the chunks."""
    from byzpy_amd.hip import dispatch as D

    X, c = resolve_matrix(ref)
    try:
        Gc, bad = D.dnc_gram(X, coords)
        return Gc.clone(), bad.clone()
    finally:
        close_ref(c)


def ref_dist_chunk(ref: Any, rlo: int, rhi: int, ref_index: int) -> torch.Tensor:
    """Squared distances of rows [rlo, rhi) to the reference row (MoNNA)."""
    X, c = resolve_matrix(ref)
    try:
        Xf = X[rlo:rhi].float()
        r = X[ref_index].float()
        return ((Xf - r[None, :]) ** 2).sum(dim=1)
    finally:
        close_ref(c)


def weiszfeld_chunk(
    ref: Any, rlo: int, rhi: int, center_ref: Any, eps: float
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sum_i w_i x_i, sum_i w_i) over row chunk against the current center."""
    X, c = resolve_matrix(ref)
    z, cz = resolve_matrix(center_ref)
    try:
        Xf = X[rlo:rhi].float()
        zf = z.reshape(-1).float()
        d = (Xf - zf[None, :]).norm(dim=1).clamp_(min=eps)
        w = 1.0 / d
        return (w[:, None] * Xf).sum(dim=0), w.sum()
    finally:
        close_ref(c)
        close_ref(cz)


def cc_chunk(
    ref: Any, rlo: int, rhi: int, center_ref: Any, c_tau: float, eps: float
) -> torch.Tensor:
    """sum_i clip(x_i - v, c_tau) over row chunk against the current center."""
    X, c = resolve_matrix(ref)
    v, cv = resolve_matrix(center_ref)
    try:
        Xf = X[rlo:rhi].float()
        vf = v.reshape(-1).float()
        diff = Xf - vf[None, :]
        norms = diff.norm(dim=1).clamp_(min=eps)
        alpha = torch.clamp(c_tau / norms, max=1.0)
        return (alpha[:, None] * diff).sum(dim=0)
    finally:
        close_ref(c)
        close_ref(cv)


def mda_combo_chunk(ref: Any, combos, m: int) -> Tuple[float, tuple]:
    """Best (min max-pairwise-D2) subset among a batch of combos; D2 ships
    as the tensor/handle ``ref`` (n x n, f32)."""
    D2, c = resolve_matrix(ref)
    try:
        best_diam, best = float("inf"), None
        D = D2.float()
        for combo in combos:
            idx = torch.tensor(combo, dtype=torch.long)
            sub = D[idx][:, idx]
            diam = float(sub.max())
            if diam < best_diam:
                best_diam, best = diam, tuple(combo)
        return best_diam, best
    finally:
        close_ref(c)


def smea_combo_chunk(ref: Any, combos, m: int) -> Tuple[float, tuple]:
    """Best (min max-eigenvalue of centered Gram) subset among combos; the
    Gram matrix ships as ``ref``."""
    G, c = resolve_matrix(ref)
    try:
        best_ev, best = float("inf"), None
        Gf = G.float()
        for combo in combos:
            idx = torch.tensor(combo, dtype=torch.long)
            sub = Gf[idx][:, idx]
            centered = (
                sub
                - sub.mean(dim=0, keepdim=True)
                - sub.mean(dim=1, keepdim=True)
                + sub.mean()
            )
            ev = float(torch.linalg.eigvalsh(centered)[-1])
            if ev < best_ev:
                best_ev, best = ev, tuple(combo)
        return best_ev, best
    finally:
        close_ref(c)


def little_stats_chunk(ref: Any, lo: int, hi: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sum, sum of squares) over feature slice for the Little attack."""
    X, c = resolve_matrix(ref)
    try:
        Xf = X[:, lo:hi].float()
        return Xf.sum(dim=0), (Xf * Xf).sum(dim=0)
    finally:
        close_ref(c)


def clip_rows_chunk(ref: Any, rlo: int, rhi: int, threshold: float) -> torch.Tensor:
    X, c = resolve_matrix(ref)
    try:
        return F.clip_rows(X[rlo:rhi], threshold).clone()
    finally:
        close_ref(c)


def scale_rows_chunk(ref: Any, rlo: int, rhi: int, scales) -> torch.Tensor:
    X, c = resolve_matrix(ref)
    try:
        s = torch.as_tensor(scales, dtype=torch.float32)
        return (X[rlo:rhi].float() * s[:, None]).to(X.dtype).clone()
    finally:
        close_ref(c)


def bucket_mean_chunk(ref: Any, bucket_rows) -> torch.Tensor:
    """Mean of one bucket's rows (bucketing pre-agg)."""
    X, c = resolve_matrix(ref)
    try:
        idx = torch.tensor(bucket_rows, dtype=torch.long)
        return X.float()[idx].mean(dim=0).to(X.dtype).clone()
    finally:
        close_ref(c)


def group_mean_chunk(ref: Any, groups) -> torch.Tensor:
    """Stack of means over row-index groups (NNM mixing step)."""
    X, c = resolve_matrix(ref)
    try:
        Xf = X.float()
        outs = [Xf[torch.tensor(g, dtype=torch.long)].mean(dim=0) for g in groups]
        return torch.stack(outs).to(X.dtype)
    finally:
        close_ref(c)
