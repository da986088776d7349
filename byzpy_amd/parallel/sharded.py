"""d-sharded robust aggregation over RCCL (the multi-GPU engine).

Layout: every rank holds the SAME n worker gradients restricted to its own
contiguous d-shard — the 288 GB-HBM-native layout for huge d (SURVEY.md
§5.7; BASELINE config 5 needs it: 32 x 8B-param bf16 grads = 512 GB > one
GPU). Coordinate-wise ops then need NO communication at all; geometry/norm
ops need only tiny (n,) / (n,n) all-reduces; the aggregate stays d-sharded
(all-gather only if the caller wants it assembled).

Every function takes the LOCAL shard (n, d_local) and returns the LOCAL
shard of the aggregate.
"""
from __future__ import annotations

from typing import Sequence

import torch

from byzpy_amd.hip import dispatch as D
from byzpy_amd.hip import require
from byzpy_amd.ops import functional as F
from byzpy_amd.parallel.dist import all_reduce_


# -- coordinate-wise: pure local --------------------------------------------

def median(X_local: torch.Tensor) -> torch.Tensor:
    return D.median(X_local)


def trimmed_mean(X_local: torch.Tensor, f: int) -> torch.Tensor:
    return D.trimmed_mean(X_local, f)


def mean_of_medians(X_local: torch.Tensor, f: int) -> torch.Tensor:
    return D.mean_of_medians(X_local, f)


# -- geometry: partial Gram + (n,n) all-reduce ------------------------------

def _global_gram(X_local: torch.Tensor) -> torch.Tensor:
    G = D.gram(X_local)
    return all_reduce_(G)


def median_and_multi_krum(X_local: torch.Tensor, f: int, q: int):
    """Both flagship aggregates with ONE collective: the local median
    shard and the partial Gram (D.median_and_gram: one pass over the shard
    where the fused kernel applies, see profiles/r03_median_gram_fused.md),
    then one (n, n) all-reduce yields a Krum selection identical on
    every rank (RCCL all-reduce returns bitwise-identical sums on all
    ranks, so the winner set never diverges)."""
    med, G = D.median_and_gram(X_local)
    winners = D.krum_winners_from_gram(all_reduce_(G), f, q)
    return med, D.mean_rows(X_local, winners)


def multi_krum(X_local: torch.Tensor, f: int, q: int) -> torch.Tensor:
    winners = D.krum_winners_from_gram(_global_gram(X_local), f, q)
    return D.mean_rows(X_local, winners)


def bulyan(X_local: torch.Tensor, f: int) -> torch.Tensor:
    """Bulyan on a d-shard: one (n, n) all-reduce, then the selection —
    identical on every rank for the same reason as the Krum winners in
    median_and_multi_krum — and the column step over the selected rows of
    the local shard. No other communication."""
    sel = D.bulyan_select_from_gram(_global_gram(X_local), f)
    return D.mean_of_medians(X_local, 2 * f, rows=sel)


def dnc(
    X_local: torch.Tensor, f: int, coords_local: torch.Tensor, c: float = 1.0
) -> torch.Tensor:
    """DnC on a d-shard. ``coords_local`` (niters, b_local) indexes the
    LOCAL shard: every rank samples its own coordinates (the global sample
    is their union; ranks agree on niters). Columns are centred one by one,
    so the centred Gram is additive over ranks: one all-reduce of the
    (niters, n, n) partials and one of the bad flags, then the selection —
    identical on every rank, as the all-reduce returns the same bits to
    all — and the counted mean of the local shard."""
    keep = F.dnc_keep(X_local.shape[0], f, c)
    Gc, bad = D.dnc_gram(X_local, coords_local)
    idx, count = D.dnc_select_from_gram(all_reduce_(Gc), all_reduce_(bad), keep)
    return D.mean_rows_counted(X_local, idx, count)


def afa(
    X_local: torch.Tensor, weights=None, xi: float = 2.0, delta_xi: float = 0.5
) -> torch.Tensor:
    """AFA on a d-shard: one (n, n) all-reduce of the partial Gram, the
    selection on it — identical on every rank, as the all-reduce returns the
    same bits to all — and the counted (weighted) mean of the local shard."""
    idx, count = D.afa_select_from_gram(
        _global_gram(X_local), weights, xi, delta_xi
    )
    if weights is None:
        return D.mean_rows_counted(X_local, idx, count)
    w = D._afa_device_weights(weights, X_local.shape[0], X_local.device)
    return D.mean_rows_counted(X_local, idx, count, weights=w)


def krum(X_local: torch.Tensor, f: int) -> torch.Tensor:
    scores = D.krum_scores_from_gram(_global_gram(X_local), f)
    return X_local[int(torch.argmin(scores))].clone()


def nnm(X_local: torch.Tensor, f: int) -> torch.Tensor:
    G = _global_gram(X_local)
    idx = D.nearest_rows_from_gram(G, X_local.shape[0] - f)
    return D.group_mean_rows(X_local, idx)


# -- norm-wise: (n,) all-reduce ---------------------------------------------

def _global_row_sqnorms(X_local: torch.Tensor) -> torch.Tensor:
    return all_reduce_(D.row_sqnorms(X_local))


def cge(X_local: torch.Tensor, f: int) -> torch.Tensor:
    norms = _global_row_sqnorms(X_local)
    idx = torch.argsort(norms, stable=True)[: X_local.shape[0] - f]
    return D.mean_rows(X_local, idx.to(torch.int32))


def clip_rows(X_local: torch.Tensor, threshold: float) -> torch.Tensor:
    norms = _global_row_sqnorms(X_local).sqrt_().clamp_min_(1e-20)
    scale = torch.clamp(threshold / norms, max=1.0)
    return D.row_scale(X_local, scale)


def arc_clip(X_local: torch.Tensor, f: int) -> torch.Tensor:
    n = X_local.shape[0]
    k = int(2 * f / n * (n - f))
    if k <= 0:
        return X_local.clone()
    norms = _global_row_sqnorms(X_local).sqrt_()
    order = torch.argsort(norms, descending=True)
    threshold = norms[order[k]]
    scale = torch.clamp(threshold / norms.clamp_min(1e-20), max=1.0)
    return D.row_scale(X_local, scale)


def bucketing(
    X_local: torch.Tensor, bucket_size: int, perm: Sequence[int]
) -> torch.Tensor:
    """perm must be identical on all ranks (caller broadcasts the seed)."""
    return D.bucketing(X_local, bucket_size, perm)


# -- iterative fixed-point: per-iteration (n,) all-reduce -------------------

# The fused update kernels stage one weight per row in LDS and the bindings
# reject n above this cap; larger n runs the torch formulas on the device
# (same routing as hip/dispatch.py).
_LDS_MAX_ROWS = 1024


def _fused_rows_ok(X_local: torch.Tensor) -> bool:
    return X_local.is_cuda and X_local.shape[0] <= _LDS_MAX_ROWS


def geometric_median(
    X_local: torch.Tensor,
    *,
    tol: float = 1e-6,
    max_iter: int = 256,
    eps: float = 1e-12,
    init: str = "median",
    fixed_iters: "int | None" = None,
) -> torch.Tensor:
    """``fixed_iters`` runs exactly that many iterations with NO
    convergence polls — drops the per-poll shift all-reduce AND the host
    sync, leaving one (n,) all-reduce per iteration (the minimum for the
    d-sharded layout)."""
    if not _fused_rows_ok(X_local):
        return _geometric_median_torch(
            X_local, tol=tol, max_iter=max_iter, eps=eps, init=init,
            fixed_iters=fixed_iters,
        )
    ext = require()
    Xc = X_local.contiguous()
    z = (D.median(Xc) if init == "median" else Xc.float().mean(dim=0)).float()
    shift = torch.zeros((), device=Xc.device, dtype=torch.float32)
    if fixed_iters is not None:
        for _ in range(int(fixed_iters)):
            dist2 = all_reduce_(ext.row_center_sqdists(Xc, z))
            z = ext.weiszfeld_apply(Xc, z, dist2, float(eps), shift)
        return z.to(X_local.dtype)
    poll = 4
    it = 0
    while it < max_iter:
        for _ in range(min(poll, max_iter - it)):
            dist2 = all_reduce_(ext.row_center_sqdists(Xc, z))
            z = ext.weiszfeld_apply(Xc, z, dist2, float(eps), shift)
            it += 1
        total_shift = all_reduce_(shift.clone())
        if float(total_shift) <= tol * tol:
            break
    return z.to(X_local.dtype)


def _geometric_median_torch(X, *, tol, max_iter, eps, init, fixed_iters=None):
    """Device-agnostic torch Weiszfeld: CPU shards, and device shards with
    more rows than the fused kernel's LDS stage holds."""
    Xf = X.float()
    z = (F.median(Xf) if init == "median" else Xf.mean(dim=0)).float()
    iters = int(fixed_iters) if fixed_iters is not None else max_iter
    for _ in range(iters):
        dist2 = all_reduce_(((Xf - z[None, :]) ** 2).sum(dim=1))
        d = dist2.sqrt().clamp_(min=eps)
        w = 1.0 / d
        z_new = (w[:, None] * Xf).sum(dim=0) / w.sum()
        if fixed_iters is None:
            shift2 = all_reduce_(((z_new - z) ** 2).sum())
            z = z_new
            if float(shift2) <= tol * tol:
                break
        else:
            z = z_new
    return z.to(X.dtype)


def centered_clipping(
    X_local: torch.Tensor,
    *,
    c_tau: float,
    M: int = 10,
    eps: float = 1e-12,
    init: str = "mean",
) -> torch.Tensor:
    if not _fused_rows_ok(X_local):
        return _centered_clipping_torch(X_local, c_tau, M, eps, init)
    ext = require()
    Xc = X_local.contiguous()
    if init == "mean":
        v = Xc.float().mean(dim=0)
    elif init == "median":
        v = D.median(Xc).float()
    else:
        v = torch.zeros(Xc.shape[1], device=Xc.device, dtype=torch.float32)
    for _ in range(M):
        dist2 = all_reduce_(ext.row_center_sqdists(Xc, v))
        v = ext.cc_apply(Xc, v, dist2, float(c_tau), float(eps))
    return v.to(X_local.dtype)


def _centered_clipping_torch(X, c_tau, M, eps, init):
    """Device-agnostic torch form (see _geometric_median_torch)."""
    n = X.shape[0]
    Xf = X.float()
    if init == "mean":
        v = Xf.mean(dim=0)
    elif init == "median":
        v = F.median(Xf).float()
    else:
        v = torch.zeros_like(Xf[0])
    for _ in range(M):
        dist2 = all_reduce_(((Xf - v[None, :]) ** 2).sum(dim=1))
        norms = dist2.sqrt().clamp_(min=eps)
        alpha = torch.clamp(c_tau / norms, max=1.0)
        v = v + (alpha[:, None] * (Xf - v[None, :])).sum(dim=0) / n
    return v.to(X.dtype)
