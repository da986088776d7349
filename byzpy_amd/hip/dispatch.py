"""Device dispatch for the robust-aggregation hot ops.

CPU tensors -> byzpy_amd.ops.functional (pure torch, the parity oracle).
CUDA(ROCm) tensors -> hand-written gfx950 kernels in byzpy_amd/_hip_ops
(SURVEY.md §2.7 kernel inventory K1-K14, plus K15 for DnC and K16 for
AFA). Ops whose GPU path composes
library GEMMs / batched eig (SMEA combos, attacks) run the functional
torch path on-device — rocBLAS library GEMMs are the sanctioned path for
plain GEMM shapes. CAF runs on the fused K9 matvec/colsum kernel pair.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import torch

from byzpy_amd import hip as _hip
from byzpy_amd.ops import functional as F

_COLSEL_MEDIAN = 0
_COLSEL_TRIMMED = 1
_COLSEL_MEAMED = 2

# Column order-statistic caps: registers to n=64, LDS-staged sort to
# n=512, streaming radix-select (every mode x dtype) to n=65535
# (colsel.hip + rsel.hip). Larger n falls back to torch.
COLSEL_MAX_N = 65535


def _gpu(X: torch.Tensor) -> bool:
    return X.is_cuda


# -- coordinate-wise (K1-K3) ------------------------------------------------


# Row-indexed colsel (`rows=`): the statistic over X[rows] with no (m, d)
# gather. The binding serves it from colsel.hip only (register kernels to
# m = 64, LDS sort to m = 512), never from the radix engine.
COLSEL_ROWS_MAX_M = 512
_COLSEL_RADIX_MIN_D = 32768


def _colsel_rows(X: torch.Tensor, mode: int, f: int, rows: torch.Tensor):
    """Device `rows=` routing. The indexed kernel runs exactly where the
    un-indexed call on X[rows] would stay in colsel.hip too: m <= 64, or
    m <= 512 at d < 32768. Larger m at large d gathers and takes the
    un-indexed op, so the radix engine (rsel.hip) keeps serving it — the
    LDS sort loses to it there by more than the gather costs."""
    m, d = int(rows.numel()), X.shape[1]
    if m <= 64 or (m <= COLSEL_ROWS_MAX_M and d < _COLSEL_RADIX_MIN_D):
        rows32 = rows.to(device=X.device, dtype=torch.int32).contiguous()
        return _hip.require().colsel(X.contiguous(), mode, int(f), rows32)
    return None


def median(X: torch.Tensor, rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``rows`` (m distinct row indices) restricts the statistic to those
    rows, as if on X[rows]; same for trimmed_mean and mean_of_medians."""
    if rows is not None:
        out = _colsel_rows(X, _COLSEL_MEDIAN, 0, rows) if _gpu(X) else None
        return out if out is not None else median(X[rows.long()])
    if _gpu(X) and X.shape[0] <= COLSEL_MAX_N:
        return _hip.require().colsel(X.contiguous(), _COLSEL_MEDIAN, 0)
    return F.median(X)


def trimmed_mean(
    X: torch.Tensor, f: int, rows: Optional[torch.Tensor] = None
) -> torch.Tensor:
    if rows is not None:
        out = _colsel_rows(X, _COLSEL_TRIMMED, f, rows) if _gpu(X) else None
        return out if out is not None else trimmed_mean(X[rows.long()], f)
    if _gpu(X) and X.shape[0] <= COLSEL_MAX_N:
        return _hip.require().colsel(X.contiguous(), _COLSEL_TRIMMED, int(f))
    return F.trimmed_mean(X, f)


def mean_of_medians(
    X: torch.Tensor, f: int, rows: Optional[torch.Tensor] = None
) -> torch.Tensor:
    if rows is not None:
        out = _colsel_rows(X, _COLSEL_MEAMED, f, rows) if _gpu(X) else None
        return out if out is not None else mean_of_medians(X[rows.long()], f)
    if _gpu(X) and X.shape[0] <= COLSEL_MAX_N:
        return _hip.require().colsel(X.contiguous(), _COLSEL_MEAMED, int(f))
    return F.mean_of_medians(X, f)


# -- pairwise distances / Krum (K4, K5) -------------------------------------


def gram(X: torch.Tensor) -> torch.Tensor:
    """X @ X.T with f32 accumulation; MFMA split-K kernel on device."""
    if _gpu(X):
        return _hip.require().gram(X.contiguous())
    Xf = X.float()
    return Xf @ Xf.T


# Column count from which median_and_gram takes the one-pass kernel
# (colsel.hip: median_gram_bf16_kernel). Measured on MI355X at n = 64 and
# n = 33, d = 64K ... 16M (profiles/r03_median_gram_fused.md, "d_min
# sweep"): the fused call took 0.33-0.78 of the pair's time at EVERY size,
# 64K included (11.2 vs 24.0 us at 64 x 65,536 — one launch against two).
# 65,536 is the smallest size measured; below it the pair stays.
MEDIAN_GRAM_FUSED_MIN_D = 65_536

# BYZPY_MEDIAN_GRAM=split forces the two-kernel pair (A/B runs)
_MEDIAN_GRAM_ENV = "BYZPY_MEDIAN_GRAM"


def _median_gram_fused_ok(X: torch.Tensor) -> bool:
    n, d = X.shape
    return (
        _gpu(X)
        and X.dtype == torch.bfloat16
        and 32 < n <= 64
        and d % 2 == 0
        and d >= MEDIAN_GRAM_FUSED_MIN_D
        and os.environ.get(_MEDIAN_GRAM_ENV, "") != "split"
    )


def median_and_gram(X: torch.Tensor):
    """Both flagship aggregates: (median, gram). bf16 device matrices with
    32 < n <= 64 rows and an even d >= MEDIAN_GRAM_FUSED_MIN_D take ONE
    pass over X (``colsel(X, 0, 0, gram=G)``): every lane keeps its column
    pair in registers and runs the separate kernel's selection network on
    the RAW bf16 words with the packed f16 min/max pair (no key transform:
    read as f16, bf16 patterns below 2^121 in magnitude order as their
    values do) and drops the raw words into its wave's private
    LDS slab (64 rows x 128 columns) on the way; the wave accumulates the
    upper triangle of that slab's Gram with MFMAs placed inside its own
    selection network, so the loop has no block barrier, and waves draw
    their 128-column strips from a work counter
    (profiles/r04_median_gram_wave.md, r03_median_gram_fused.md; the six
    organizations that lost are in profiles/r02_fusion_negative.md). The
    median is bitwise
    the separate kernel's for EVERY input: a word of 2^121 or more, an
    infinity or a NaN leaves a non-finite entry on G's diagonal, which a
    second launch on the same stream checks on the device (no host sync;
    a few microseconds when there is nothing to do) before it recomputes
    the median with the separate kernel
    (profiles/r05_median_gram_rawbits.md). The Gram differs from
    ``gram(X)`` only in f32 summation order. Everything else, and
    ``BYZPY_MEDIAN_GRAM=split``, runs ``median(X), gram(X)``."""
    if _median_gram_fused_ok(X):
        Xc = X.contiguous()
        G = torch.empty((X.shape[0], X.shape[0]), dtype=torch.float32,
                        device=X.device)
        med = _hip.require().colsel(Xc, _COLSEL_MEDIAN, 0, gram=G)
        return med, G
    return median(X), gram(X)


# Gram -> squared distances -> Krum scores -> winners. Device-agnostic
# torch on the tiny (n, n) Gram, written ONCE: cross-rank Krum winner-set
# consistency rests on every rank and every engine (direct, chunked pool,
# d-sharded) evaluating exactly these expressions. ops/functional.py keeps
# its own independent text as the oracle.


def sq_dists_from_gram(G: torch.Tensor) -> torch.Tensor:
    """||a||^2 + ||b||^2 - 2 a.b clamped at 0, from an (n, n) Gram or a
    batch (B, n, n) of them."""
    norms = torch.diagonal(G, dim1=-2, dim2=-1)
    return (norms[..., :, None] + norms[..., None, :] - 2.0 * G).clamp_(min=0.0)


def krum_scores_from_gram(G: torch.Tensor, f: int) -> torch.Tensor:
    """score_i = sum of the n-f-1 smallest squared distances from row i to
    the others (the self-distance is masked with +inf)."""
    n = G.shape[0]
    D2 = sq_dists_from_gram(G)
    D2 = D2 + torch.diag(
        torch.full((n,), float("inf"), device=G.device, dtype=G.dtype)
    )
    return torch.topk(D2, k=n - f - 1, dim=1, largest=False).values.sum(dim=1)


def krum_winners_from_gram(G: torch.Tensor, f: int, q: int) -> torch.Tensor:
    """int32 indices of the q best-scored rows: the fused krum_select
    kernel on device up to its n = 512 cap, else topk over the scores."""
    if _gpu(G) and G.shape[0] <= 512:
        return _hip.require().krum_select(G, int(f), int(q))
    scores = krum_scores_from_gram(G, f)
    return torch.topk(scores, k=q, largest=False).indices.to(torch.int32)


# Row cap of krum_select(iterative=True): the kernel keeps every sorted
# distance row in LDS (KRUM_ITER_MAX_N in csrc/launchers.h).
BULYAN_SELECT_MAX_N = 128


def _check_bulyan(n: int, f: int) -> None:
    if f < 0 or n < 4 * f + 3:
        raise ValueError(f"Bulyan needs n >= 4f + 3, got n={n}, f={f}")


def bulyan_select_from_gram(G: torch.Tensor, f: int) -> torch.Tensor:
    """int32 (n - 2f,) Bulyan selection in pick order: n - 2f rounds of
    Krum among the rows still alive (score = sum of the alive - f - 1
    smallest squared distances to other alive rows; ties to the smallest
    index; non-finite distances count as +inf), each winner leaving the
    pool. One fused launch on device up to BULYAN_SELECT_MAX_N rows; past
    it, and on CPU, the same picks as sync-free torch ops on the Gram."""
    n = G.shape[0]
    _check_bulyan(n, f)
    theta = n - 2 * f
    if f == 0:
        return torch.arange(n, device=G.device, dtype=torch.int32)
    if _gpu(G) and n <= BULYAN_SELECT_MAX_N:
        return _hip.require().krum_select(G, int(f), int(theta), True)
    return _bulyan_select_torch(G, f)


def _bulyan_select_torch(G: torch.Tensor, f: int) -> torch.Tensor:
    """The Bulyan picks as torch ops on the Gram, any device, no host
    sync: about ten small launches per pick."""
    n = G.shape[0]
    theta = n - 2 * f
    inf = float("inf")
    D2 = sq_dists_from_gram(G)
    D2 = torch.where(torch.isfinite(D2), D2, torch.full_like(D2, inf))
    D2.fill_diagonal_(inf)
    alive = torch.ones(n, dtype=torch.bool, device=G.device)
    picks = torch.empty(theta, dtype=torch.int64, device=G.device)
    for p in range(theta):
        k = n - p - f - 1
        # dead columns cost +inf: with k <= alive - 1 they never enter a
        # k-smallest sum ahead of a finite alive distance
        near = torch.topk(
            D2.masked_fill(~alive[None, :], inf), k=k, dim=1, largest=False
        ).values
        scores = near.sum(dim=1).masked_fill_(~alive, inf)
        # first alive row at the minimum (argmin alone could name a dead
        # row when every alive score is +inf)
        hit = alive & (scores == scores.min())
        i = torch.argmax(hit.to(torch.int32))
        picks[p] = i
        alive[i] = False
    return picks.to(torch.int32)


def nearest_rows_from_gram(G: torch.Tensor, k: int) -> torch.Tensor:
    """Per row, the indices of its k nearest rows (itself included)."""
    return torch.topk(sq_dists_from_gram(G), k=k, dim=-1, largest=False).indices


def pairwise_sq_dists(X: torch.Tensor) -> torch.Tensor:
    if _gpu(X):
        return sq_dists_from_gram(gram(X))
    return F.pairwise_sq_dists(X)


def multi_krum_scores(X: torch.Tensor, f: int) -> torch.Tensor:
    n = X.shape[0]
    if n - f - 1 < 1:
        raise ValueError(f"need n - f - 1 >= 1, got n={n}, f={f}")
    if _gpu(X):
        return krum_scores_from_gram(gram(X), f)
    return F.multi_krum_scores(X, f)


def multi_krum(X: torch.Tensor, f: int, q: int) -> torch.Tensor:
    if _gpu(X):
        return mean_rows(X, krum_winners_from_gram(gram(X), f, q))
    return F.multi_krum(X, f, q)


def krum(X: torch.Tensor, f: int) -> torch.Tensor:
    if _gpu(X) and X.shape[0] <= 512:
        idx = krum_winners_from_gram(gram(X), f, 1)
        return X[idx.long()[0]].clone()
    scores = multi_krum_scores(X, f)
    return X[int(torch.argmin(scores))].clone()


def bulyan(X: torch.Tensor, f: int) -> torch.Tensor:
    """Bulyan (El Mhamdi et al. 2018): Gram -> n - 2f rows by iterated Krum
    -> per coordinate the mean of the n - 4f selected values closest to
    their median. On device: MFMA Gram, one selection launch, one indexed
    mean-around-median launch reading the selected rows in place — no
    (theta, d) gather and no host sync."""
    n = X.shape[0]
    _check_bulyan(n, f)
    if f == 0:
        return mean_of_medians(X, 0)
    sel = bulyan_select_from_gram(gram(X), f)
    return mean_of_medians(X, 2 * f, rows=sel)


def mean_rows(X: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """Mean of the selected rows, f32 accumulation (K10 gather-mean)."""
    if _gpu(X):
        return _hip.require().mean_rows(X.contiguous(), idx.to(torch.int32))
    return X.float()[idx].mean(dim=0).to(X.dtype)


# Longest idx of mean_rows(count=, weights=): the kernel stages the weights in
# LDS (MAX_N_LDS in csrc/launchers.h).
MEAN_ROWS_WEIGHTED_MAX_K = 1024


def mean_rows_counted(
    X: torch.Tensor,
    idx: torch.Tensor,
    count: torch.Tensor,
    weights: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Mean of rows idx[:count] with ``count`` an int32 scalar tensor that a
    device X reads on the device (no host sync); zeros when it is 0. Bitwise
    ``mean_rows(X, idx[:count])`` otherwise. With ``weights`` (one per row of
    X) the weighted mean sum_k w[idx[k]] x[idx[k]] / sum_k w[idx[k]], f32
    accumulation, zeros when the weight sum is 0; a kernel of its own on
    device to MEAN_ROWS_WEIGHTED_MAX_K indices, torch ops (which sync) past
    that and on CPU."""
    if weights is None:
        if _gpu(X):
            return _hip.require().mean_rows(
                X.contiguous(), idx.to(torch.int32), count=count.to(torch.int32)
            )
        k = int(count)
        if k == 0:
            return torch.zeros_like(X[0])
        return X.float()[idx[:k].long()].mean(dim=0).to(X.dtype)
    if _gpu(X) and 1 <= idx.numel() <= MEAN_ROWS_WEIGHTED_MAX_K:
        w = weights.to(device=X.device, dtype=torch.float32).contiguous()
        return _hip.require().mean_rows(
            X.contiguous(), idx.to(torch.int32).contiguous(),
            count=count.to(torch.int32), weights=w,
        )
    rows = idx[: int(count)].long()
    w = weights.to(device=X.device, dtype=torch.float32)[rows]
    den = w.sum()
    if rows.numel() == 0 or not float(den) > 0.0:
        return torch.zeros_like(X[0])
    return ((w[:, None] * X.float()[rows]).sum(dim=0) / den).to(X.dtype)


# -- DnC (K15) ---------------------------------------------------------------
#
# Divide-and-Conquer (Shejwalkar & Houmansadr 2021): per iteration a sample of
# b coordinates, the centred sample's top singular direction, the rows with
# the largest squared projection on it dropped; the rows kept by every
# iteration are averaged. Everything after the (niters, n, n) sampled centred
# Grams is O(n^2): lambda u_i^2 from the Gram's top eigenpair IS the squared
# projection, so no d-sized vector is formed. ops/functional.py keeps its own
# text as the oracle.

# Row cap of gram(X, cols=) and smea_select(Gc3, bad, keep) (DNC_MAX_N in
# csrc/launchers.h).
DNC_MAX_N = 128


def _dnc_fused(T: torch.Tensor, n: int) -> bool:
    return _gpu(T) and 1 <= n <= DNC_MAX_N


def dnc_gram(X: torch.Tensor, coords: torch.Tensor):
    """(Gc (niters, n, n), bad int32 (niters, n)) of the samples
    X[:, coords[t]]: Gc[t] = C C^T with C centred per column by the mean of
    its finite entries (|x| <= 2^48) and 0 where an entry is not; bad marks
    the rows holding such an entry. Additive over column chunks of coords.
    One fused launch pair to DNC_MAX_N rows on device (f32, bitwise
    repeatable); else f64 torch ops."""
    if _dnc_fused(X, X.shape[0]):
        cols = coords.to(device=X.device, dtype=torch.int32).contiguous()
        Gc, bad = _hip.require().gram(X.contiguous(), cols=cols)
        return Gc, bad
    return _dnc_gram_torch(X, coords)


def _dnc_gram_torch(X: torch.Tensor, coords: torch.Tensor):
    """dnc_gram as f64 torch ops, any device."""
    S = X[:, coords.to(X.device).long()].permute(1, 0, 2).double()  # (t, n, b)
    ok = torch.isfinite(S) & (S.abs() <= F.DNC_MAX_ABS)
    Sz = torch.where(ok, S, torch.zeros_like(S))
    mu = Sz.sum(dim=1, keepdim=True) / ok.sum(dim=1, keepdim=True).clamp_min(1)
    C = torch.where(ok, S - mu, torch.zeros_like(S))
    bad = (~ok.all(dim=2)).to(torch.int32)
    return torch.bmm(C, C.transpose(1, 2)), bad


def dnc_select_from_gram(Gc: torch.Tensor, bad: torch.Tensor, keep: int):
    """(idx int32 (n,), count int32 ()) from the sampled centred Grams:
    idx[:count] are the ascending indices of the rows that every iteration
    keeps (its ``keep`` lowest lambda u_i^2, ties to the smaller index, bad
    rows never), the rest of idx is padding. One fused launch pair on device
    for f32 Grams to DNC_MAX_N rows, no host sync; else torch ops with an
    f64 ``eigh`` (which syncs)."""
    niters, n = bad.shape
    if not 1 <= keep <= n:
        raise ValueError(f"DnC needs 1 <= keep <= n, got keep={keep}, n={n}")
    if _dnc_fused(Gc, n) and Gc.dtype == torch.float32:
        idx, count = _hip.require().smea_select(
            Gc.contiguous(), bad.to(torch.int32).contiguous(), int(keep)
        )
        return idx, count
    return _dnc_select_torch(Gc, bad, keep)


def _dnc_select_torch(Gc: torch.Tensor, bad: torch.Tensor, keep: int):
    """dnc_select_from_gram as torch ops, any device; eigh syncs the host."""
    G = Gc.double()
    lam, U = torch.linalg.eigh(G)
    top, u = lam[:, -1], U[:, :, -1]
    # G u summed row by row: identical Gram rows get identical scores
    y = (G * u[:, None, :]).sum(dim=2)
    score = torch.where(
        top[:, None] > 0, y * y / top[:, None].clamp_min(1e-300),
        torch.zeros_like(y),
    )
    isbad = bad != 0
    score = score.masked_fill(isbad, float("inf"))
    order = torch.argsort(score, dim=1, stable=True)
    kept = torch.zeros_like(isbad)
    kept.scatter_(1, order[:, :keep], True)
    good = (kept & ~isbad).all(dim=0)
    idx = torch.argsort((~good).to(torch.int8), stable=True).to(torch.int32)
    idx = torch.where(good[idx.long()], idx, torch.zeros_like(idx))
    return idx, good.sum().to(torch.int32)


def _dnc_idx(X: torch.Tensor, f: int, coords: torch.Tensor, c: float):
    keep = F.dnc_keep(X.shape[0], f, c)
    Gc, bad = dnc_gram(X, coords)
    return dnc_select_from_gram(Gc, bad, keep)


def dnc_select(
    X: torch.Tensor, f: int, coords: torch.Tensor, c: float = 1.0
) -> torch.Tensor:
    """DnC's good set as a bool (n,) mask (see ``dnc``)."""
    if not _gpu(X):
        return F.dnc_select(X, f, coords, c)
    n = X.shape[0]
    idx, count = _dnc_idx(X, f, coords, c)
    live = (torch.arange(n, device=X.device) < count).to(torch.int32)
    hits = torch.zeros(n, dtype=torch.int32, device=X.device)
    return hits.scatter_add_(0, idx.long(), live) > 0


def dnc(
    X: torch.Tensor, f: int, coords: torch.Tensor, c: float = 1.0
) -> torch.Tensor:
    """DnC: the mean of the rows that survive every iteration's spectral
    filter on the sample X[:, coords[t]]; zeros if none does (skip the
    round). ``coords`` is int (niters, b), each row sorted, duplicates
    allowed. On device to DNC_MAX_N rows: sampled centred Grams, spectral
    selection, counted gather-mean — three binding calls, no host sync,
    capturable into a hipGraph when coords is an int32 device tensor. Past
    it the same steps as torch ops on the device."""
    if not _gpu(X):
        return F.dnc(X, f, coords, c)
    idx, count = _dnc_idx(X, f, coords, c)
    return mean_rows_counted(X, idx, count)


# -- AFA (K16) ---------------------------------------------------------------
#
# Adaptive Federated Averaging (Muñoz-González, Co, Lupu 2019): drop, pass
# after pass, the rows whose cosine to the weighted mean g of the rows still
# alive is an outlier, then average the rest. With w masked to the alive rows,
# u = G w and q = w^T G w give cos(x_i, g) = u_i / sqrt(G_ii q): the whole
# loop lives on the (n, n) Gram and nothing d-sized is formed before the final
# mean. ops/functional.py keeps its own text (explicit mean vector and norms)
# as the oracle.

# Row cap of smea_select(G, weights=, xi=, delta_xi=) (AFA_MAX_N in
# csrc/launchers.h).
AFA_MAX_N = 128


def _afa_device_weights(weights, n: int, device) -> torch.Tensor:
    """The (n,) f32 weight vector on ``device``. Host weights are checked
    (``ValueError``); a device tensor is only checked for its length, so that
    nothing syncs: there a weight that is negative, NaN or inf marks its row
    dead."""
    if weights is None:
        return torch.ones(n, dtype=torch.float32, device=device)
    if isinstance(weights, torch.Tensor) and weights.is_cuda:
        if weights.numel() != n:
            raise ValueError(f"weights: expected {n} entries, got {weights.numel()}")
        return weights.detach().flatten().to(device=device, dtype=torch.float32)
    return F._afa_weights(weights, n).to(device=device, dtype=torch.float32)


def _afa_select_torch(G: torch.Tensor, w: torch.Tensor, xi: float, delta_xi: float):
    """The AFA loop as f64 torch ops on the Gram, any device: (idx, count,
    rounds). Every pass syncs the host (the loop ends on the data)."""
    n = G.shape[0]
    Gd, wd = G.double(), w.double()
    diag = Gd.diagonal()
    alive = torch.isfinite(diag) & torch.isfinite(wd) & (wd > 0)
    Gz = torch.where(torch.isfinite(Gd), Gd, torch.zeros_like(Gd))
    zero = torch.zeros_like(wd)
    xi = float(xi)
    rounds = 0
    for _ in range(n):
        m = int(alive.sum())
        if m == 0:
            break
        rounds += 1
        wm = torch.where(alive, wd, zero)
        u = Gz @ wm
        q = wm @ u
        ok = alive & (diag > 0) & (q > 0)
        s = torch.where(ok, u / (diag * q).clamp_min(1e-300).sqrt(), zero)
        sa = s[alive]
        mean = sa.mean()
        srt = torch.sort(sa).values
        med = 0.5 * (srt[(m - 1) // 2] + srt[m // 2])
        sd = ((sa - mean) ** 2).mean().sqrt()
        if bool(mean < med):
            removed = alive & (s < med - xi * sd)
        else:
            removed = alive & (s > med + xi * sd)
        if not bool(removed.any()):
            break
        alive = alive & ~removed
        xi += float(delta_xi)
    idx = torch.argsort((~alive).to(torch.int8), stable=True).to(torch.int32)
    idx = torch.where(alive[idx.long()], idx, torch.zeros_like(idx))
    return idx, alive.sum().to(torch.int32), rounds


def afa_select_from_gram(
    G: torch.Tensor, weights=None, xi: float = 2.0, delta_xi: float = 0.5
):
    """(idx int32 (n,), count int32 ()) of AFA's good set from the Gram
    G = X X^T: idx[:count] are the ascending indices of the rows still alive
    when a pass drops nothing (see ``functional.afa_select`` for the rule),
    the rest of idx is padding 0. Rows with a non-finite G_ii or a weight
    that is not positive start dead. One fused launch on device for f32 Grams
    to AFA_MAX_N rows, no host sync; otherwise the same passes as f64 torch
    ops on G's device, which sync the host once per pass."""
    F._afa_check(xi, delta_xi)
    n = G.shape[0]
    w = _afa_device_weights(weights, n, G.device)
    if _gpu(G) and 1 <= n <= AFA_MAX_N and G.dtype == torch.float32:
        idx, count, _ = _hip.require().smea_select(
            G.contiguous(), weights=w.contiguous(), xi=float(xi),
            delta_xi=float(delta_xi),
        )
        return idx, count
    idx, count, _ = _afa_select_torch(G, w, xi, delta_xi)
    return idx, count


def afa_select(
    X: torch.Tensor, weights=None, xi: float = 2.0, delta_xi: float = 0.5
) -> torch.Tensor:
    """AFA's good set as a bool (n,) mask (see ``afa``)."""
    if not _gpu(X):
        return F.afa_select(X, weights, xi, delta_xi)
    n = X.shape[0]
    idx, count = afa_select_from_gram(gram(X), weights, xi, delta_xi)
    live = (torch.arange(n, device=X.device) < count).to(torch.int32)
    hits = torch.zeros(n, dtype=torch.int32, device=X.device)
    return hits.scatter_add_(0, idx.long(), live) > 0


def afa(
    X: torch.Tensor, weights=None, xi: float = 2.0, delta_xi: float = 0.5
) -> torch.Tensor:
    """AFA: the weighted mean of the rows that survive the cosine-outlier
    passes, zeros if none does (skip the round). ``weights`` (n,) >= 0,
    default all ones. On device to AFA_MAX_N rows: MFMA Gram, one selection
    launch, counted gather-mean (the un-weighted kernel when ``weights`` is
    None) — three binding calls, no host sync, capturable into a hipGraph.
    Past the cap the selection runs as torch ops on the device and syncs.
    CPU tensors take the functional path."""
    if not _gpu(X):
        return F.afa(X, weights, xi, delta_xi)
    idx, count = afa_select_from_gram(gram(X), weights, xi, delta_xi)
    if weights is None:
        return mean_rows_counted(X, idx, count)
    w = _afa_device_weights(weights, X.shape[0], X.device)
    return mean_rows_counted(X, idx, count, weights=w)


def group_mean_rows(X: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """Row g of the result is the mean of rows idx[g] (K10, NNM mixing)."""
    if _gpu(X):
        return _hip.require().group_mean_rows(X.contiguous(), idx.to(torch.int32))
    return X.float()[idx.long()].mean(dim=1).to(X.dtype)


# -- row norms / scaling (K8, K12) ------------------------------------------


def row_sqnorms(X: torch.Tensor) -> torch.Tensor:
    if _gpu(X):
        return _hip.require().row_sqnorms(X.contiguous())
    Xf = X.float()
    return (Xf * Xf).sum(dim=1)


def row_scale(X: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    if _gpu(X):
        return _hip.require().row_scale(X.contiguous(), scales.float())
    return (X.float() * scales.float()[:, None]).to(X.dtype)


def clip_rows(X: torch.Tensor, threshold: float) -> torch.Tensor:
    if _gpu(X):
        norms = row_sqnorms(X).sqrt_().clamp_min_(1e-20)
        scale = torch.clamp(threshold / norms, max=1.0)
        return row_scale(X, scale)
    return F.clip_rows(X, threshold)


def arc_clip(X: torch.Tensor, f: int) -> torch.Tensor:
    n = X.shape[0]
    k = int(2 * f / n * (n - f))
    if k <= 0:
        return X.clone()
    if _gpu(X):
        norms = row_sqnorms(X).sqrt_()
        order = torch.argsort(norms, descending=True)
        threshold = norms[order[k]]
        scale = torch.clamp(threshold / norms.clamp_min(1e-20), max=1.0)
        return row_scale(X, scale)
    return F.arc_clip(X, f)


def cge(X: torch.Tensor, f: int) -> torch.Tensor:
    n = X.shape[0]
    k = n - f
    if _gpu(X):
        norms = row_sqnorms(X)
        idx = torch.argsort(norms, stable=True)[:k]
        return mean_rows(X, idx)
    return F.cge(X, f)


# -- iterative fixed-point ops (K6, K7) -------------------------------------


def geometric_median(
    X: torch.Tensor,
    *,
    tol: float = 1e-6,
    max_iter: int = 256,
    eps: float = 1e-12,
    init: str = "median",
    fixed_iters: Optional[int] = None,
    init_z: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Weiszfeld fixed point. ``fixed_iters`` runs exactly that many
    iterations with NO convergence polls — fully async (no host sync), so
    per-node streams overlap and the whole call is hipGraph-capture-safe
    (the polls serialized config-4 gossip in round 1). ``init_z`` warm-
    starts from a caller-provided center (e.g. the previous gossip
    round's output — the fixed point barely moves between rounds, so a
    handful of iterations replaces a cold median init + long descent)."""
    if not _gpu(X) or X.shape[0] > 1024:
        # extension's weiszfeld_iter TORCH_CHECKs n <= 1024; the torch
        # functional path runs fine on-device for larger n
        if init_z is not None:
            Xf = X.float()
            z = init_z.detach().to(device=X.device, dtype=torch.float32)
            iters = int(fixed_iters) if fixed_iters is not None else max_iter
            for _ in range(iters):
                dist = (Xf - z[None, :]).norm(dim=1).clamp_(min=eps)
                w = 1.0 / dist
                z_new = (w[:, None] * Xf).sum(dim=0) / w.sum()
                if fixed_iters is None and float((z_new - z).norm()) <= tol:
                    z = z_new
                    break
                z = z_new
            return z.to(X.dtype)
        if fixed_iters is not None:
            return F.geometric_median(
                X, tol=0.0, max_iter=int(fixed_iters), eps=eps, init=init
            )
        return F.geometric_median(X, tol=tol, max_iter=max_iter, eps=eps, init=init)
    ext = _hip.require()
    Xc = X.contiguous()
    if init_z is not None:
        z = init_z.detach().to(device=X.device, dtype=torch.float32)
    else:
        z = (median(Xc) if init == "median" else Xc.float().mean(dim=0)).float()
    shift = torch.zeros((), device=X.device, dtype=torch.float32)
    if fixed_iters is not None:
        for _ in range(int(fixed_iters)):
            z = ext.weiszfeld_iter(Xc, z, float(eps), shift)
        return z.to(X.dtype)
    # fused per-iteration kernel pair; convergence polled every `poll`
    # iters, with the poll readback PIPELINED one block deep (same
    # pattern as the CAF loop): block b+1's kernels launch while block
    # b's pinned copy of `shift` is in flight, so the host never stalls
    # on a sync — value-identical, speculative blocks past the break
    # point are discarded (each iteration returns a fresh z tensor, so
    # the pre-break z is simply kept by reference).
    # `shift` holds the last iteration's SQUARED step ||dz||^2 (rowops.hip
    # weiszfeld_iter resets + atomicAdds it), so compare against tol^2 to
    # match the CPU oracle's ||dz|| <= tol and parallel/sharded.py.
    poll = 4
    stat_pin = [torch.empty((), pin_memory=True) for _ in range(2)]
    stat_ev = [torch.cuda.Event() for _ in range(2)]
    pending: list = []  # (z_after_block, slot)
    it = 0
    blk = 0
    result_z = None
    while it < max_iter:
        steps = min(poll, max_iter - it)
        for _ in range(steps):
            z = ext.weiszfeld_iter(Xc, z, float(eps), shift)
        it += steps
        slot = blk & 1
        blk += 1
        stat_pin[slot].copy_(shift, non_blocking=True)
        stat_ev[slot].record()
        pending.append((z, slot))
        if len(pending) == 2:
            z_b, sb = pending.pop(0)
            stat_ev[sb].synchronize()
            if float(stat_pin[sb]) <= tol * tol:
                result_z = z_b
                break
    if result_z is None:
        while pending:
            z_b, sb = pending.pop(0)
            stat_ev[sb].synchronize()
            if float(stat_pin[sb]) <= tol * tol:
                result_z = z_b
                break
        if result_z is None:
            result_z = z
    return result_z.to(X.dtype)


def geometric_median_grouped(
    X3: torch.Tensor,
    *,
    iters: int = 8,
    eps: float = 1e-12,
    init_z: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Geometric medians of G independent (m, d) groups in one kernel
    pair per iteration (gossip rounds: all nodes advance together —
    replaces per-node streams + 2*G*iters launches). Fixed iteration
    count (poll-free); warm-start with ``init_z`` (G, d)."""
    G, m, d = X3.shape
    if not _gpu(X3) or m > 32:
        Z = []
        for g in range(G):
            z0 = init_z[g] if init_z is not None else None
            Z.append(
                geometric_median(
                    X3[g], fixed_iters=int(iters), eps=eps, init_z=z0
                ).float()
            )
        return torch.stack(Z)
    ext = _hip.require()
    Xc = X3.contiguous()
    if init_z is not None:
        Z = init_z.detach().to(dtype=torch.float32).contiguous()
    else:
        # per-group colsel medians (G fast launches — torch's dim-median
        # on a (G, m, 25M) tensor measured ~945 ms)
        Z = torch.stack([median(Xc[g]).float() for g in range(G)]).contiguous()
    for _ in range(int(iters)):
        Z = ext.weiszfeld_iter_grouped(Xc, Z, float(eps))
    return Z


def nnm_grouped(X3: torch.Tensor, f: int) -> torch.Tensor:
    """NNM for G independent (m, d) groups: per-group f32 Grams on the
    exactly-once MFMA kernel (tiny launches) + ONE (1/k)-mask bmm that
    mixes neighbors without materializing gathered/f32 copies."""
    G, m, d = X3.shape
    k = m - f
    if _gpu(X3):
        Gm = torch.stack([gram(X3[g]) for g in range(G)])  # (G, m, m) f32
    else:
        Xf = X3.float()
        Gm = torch.bmm(Xf, Xf.transpose(1, 2))
    idx = nearest_rows_from_gram(Gm, k)
    mask = torch.zeros_like(Gm)
    mask.scatter_(2, idx, 1.0 / k)
    return torch.bmm(mask.to(X3.dtype), X3)


def centered_clipping(
    X: torch.Tensor,
    *,
    c_tau: float,
    M: int = 10,
    eps: float = 1e-12,
    init: str = "mean",
) -> torch.Tensor:
    if not _gpu(X) or X.shape[0] > 1024:
        # extension's cc_iter TORCH_CHECKs n <= 1024; fall back on-device
        return F.centered_clipping(X, c_tau=c_tau, M=M, eps=eps, init=init)
    ext = _hip.require()
    Xc = X.contiguous()
    if init == "mean":
        v = Xc.float().mean(dim=0)
    elif init == "median":
        v = median(Xc).float()
    else:
        v = torch.zeros(X.shape[1], device=X.device, dtype=torch.float32)
    for _ in range(M):
        v = ext.cc_iter(Xc, v, float(c_tau), float(eps))
    return v.to(X.dtype)


# -- pre-aggregators --------------------------------------------------------


def bucketing(
    X: torch.Tensor, bucket_size: int, perm: Optional[Sequence[int]] = None
) -> torch.Tensor:
    if _gpu(X):
        n = X.shape[0]
        if perm is None:
            perm_t = torch.randperm(n, device=X.device, dtype=torch.int32)
        else:
            perm_t = torch.as_tensor(list(perm), device=X.device, dtype=torch.int32)
        return _hip.require().bucket_mean(X.contiguous(), perm_t, int(bucket_size))
    return F.bucketing(X, bucket_size, perm)


def nnm(X: torch.Tensor, f: int) -> torch.Tensor:
    if _gpu(X):
        idx = nearest_rows_from_gram(gram(X), X.shape[0] - f)
        return group_mean_rows(X, idx)
    return F.nnm(X, f)


# -- attack math (K14) ------------------------------------------------------


def little(X: torch.Tensor, f: int, N: Optional[int] = None) -> torch.Tensor:
    """'A Little Is Enough': mu + z*sigma, fused single pass on device
    (reference little.py:219-224 chunked sum/sum-sq decomposition)."""
    if not _gpu(X):
        return F.little(X, f, N)
    import math

    n = X.shape[0]
    N_total = N if N is not None else n + f
    s = N_total // 2 + 1 - f
    phi_arg = (N_total - s) / N_total
    # inverse normal CDF via erfinv (host scalar math, no torch RNG)
    z = math.sqrt(2.0) * torch.special.erfinv(
        torch.tensor(2.0 * phi_arg - 1.0, dtype=torch.float64)
    ).item()
    return _hip.require().little_fused(X.contiguous(), float(z))


def gaussian_attack(
    like: torch.Tensor,
    mu: float = 0.0,
    sigma: float = 1.0,
    seed: Optional[int] = None,
) -> torch.Tensor:
    """Philox4x32-10 + Box-Muller device fill — no torch RNG on the hot
    path. Seeded calls are deterministic per (seed, index); the stream is
    the kernel's own, not torch's CPU sequence (callers who need the CPU
    sequence use the functional path)."""
    if not _gpu(like):
        return F.gaussian_attack(like, mu, sigma, seed)
    d = like.shape[-1]
    if seed is None:
        seed = int(torch.randint(0, 2**62, (1,)).item())
    return _hip.require().gaussian_fill(int(d), int(seed), float(mu),
                                        float(sigma), like)


# Min-Max / Min-Sum (Shejwalkar & Houmansadr 2021): m = mu + gamma * p with
# the largest gamma >= 0 that keeps m inside the honest cloud. With
#   a_i = ||mu - x_i||^2,  b_i = p . (mu - x_i),  c = ||p||^2
# the distance ||m - x_i||^2 = a_i + 2 gamma b_i + gamma^2 c is a quadratic in
# gamma, so the optimum is a root, not a search: the formulas below are torch
# ops on the O(n) statistics, any device and dtype, no host sync.
# ops/functional.py keeps its own text (explicit differences, bisection).

_PERTURB_CODES = {"unit": 0, "std": 1, "sign": 2}

# Row cap of little_fused(X, z, perturb) (MAX_N_LDS in csrc/launchers.h).
ATTACK_STATS_MAX_N = 1024


def _perturb_code(perturbation: str) -> int:
    if perturbation not in _PERTURB_CODES:
        raise ValueError(
            f"perturbation must be one of {tuple(_PERTURB_CODES)}, "
            f"got {perturbation!r}"
        )
    return _PERTURB_CODES[perturbation]


def min_max_gamma(
    a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, tau: torch.Tensor
) -> torch.Tensor:
    """Largest gamma with max_i (a_i + 2 gamma b_i + gamma^2 c) <= tau.
    Row i allows [0, gamma_i], gamma_i = (-b_i + sqrt(b_i^2 + c D_i)) / c
    with D_i = max(tau - a_i, 0); for b_i >= 0 that difference cancels, so
    it is evaluated as D_i / (b_i + sqrt(b_i^2 + c D_i)). c = 0 gives 0."""
    delta = (tau - a).clamp_min(0.0)
    root = torch.sqrt(b * b + c * delta)
    den = b + root
    one = torch.ones_like(den)
    pos = delta / torch.where(den > 0, den, one)  # den = 0 only if delta = 0
    neg = (root - b) / torch.where(c > 0, c, torch.ones_like(c))
    gamma = torch.where(b >= 0, pos, neg).min()
    return torch.where(c > 0, gamma, torch.zeros_like(gamma))


def min_sum_gamma(a: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """Largest gamma with sum_i (a_i + 2 gamma b_i + gamma^2 c) <= tau_s.
    sum_i b_i = 0 and sum_j ||x_i - x_j||^2 = n a_i + sum_j a_j, so the
    constraint is n gamma^2 c <= n max_i a_i. c = 0 gives 0."""
    gamma = torch.sqrt(a.max() / torch.where(c > 0, c, torch.ones_like(c)))
    return torch.where(c > 0, gamma, torch.zeros_like(gamma))


def attack_stats(X: torch.Tensor, perturbation: str = "std"):
    """(mu, p, a, b, c) of a device matrix, f32: one fused pass to n = 64,
    three kernels to n = 1024. "unit" returns the unnormalised p = -mu (m
    does not change when p is rescaled)."""
    n = X.shape[0]
    mu, p, stats = _hip.require().little_fused(
        X.contiguous(), 0.0, _perturb_code(perturbation)
    )
    return mu, p, stats[:n], stats[n : 2 * n], stats[2 * n]


def _attack_device(X: torch.Tensor) -> bool:
    return _gpu(X) and 1 <= X.shape[0] <= ATTACK_STATS_MAX_N


def min_max(X: torch.Tensor, perturbation: str = "std") -> torch.Tensor:
    """Min-Max attack: the farthest m = mu + gamma p whose largest distance to
    an honest row stays within the largest honest pairwise distance. On
    device: the statistics pass, the MFMA Gram for tau, gamma as a device
    scalar — no host sync, capturable into a hipGraph."""
    _perturb_code(perturbation)
    if not _attack_device(X):
        return F.min_max(X, perturbation)
    mu, p, a, b, c = attack_stats(X, perturbation)
    tau = sq_dists_from_gram(gram(X)).max()
    return torch.addcmul(mu, min_max_gamma(a, b, c, tau), p).to(X.dtype)


def min_sum(X: torch.Tensor, perturbation: str = "std") -> torch.Tensor:
    """Min-Sum attack: the farthest m = mu + gamma p whose summed squared
    distance to the honest rows stays within the largest such sum of an
    honest row. Needs no Gram: gamma = sqrt(max_i a_i / c)."""
    _perturb_code(perturbation)
    if not _attack_device(X):
        return F.min_sum(X, perturbation)
    mu, p, a, _, c = attack_stats(X, perturbation)
    return torch.addcmul(mu, min_sum_gamma(a, c), p).to(X.dtype)


# Aggregator-tailored attacks (Shejwalkar & Houmansadr 2021): f copies of
# m = mu + gamma p with the largest gamma for which Krum / Multi-Krum / Bulyan,
# run with parameter f on the n honest rows followed by the copies, still
# selects them. Honest-honest distances come off the honest Gram, honest-
# malicious ones are e_i(gamma) = max(a_i + 2 gamma b_i + gamma^2 c, 0),
# malicious-malicious ones are 0: the search never touches X. It is a grid
# search: gamma = 0 and gamma0 2^-20 .. gamma0 2^20 (gamma0 = sqrt(max a / c),
# the Min-Sum value), then two linear grids of 256 interior points inside the
# gap below the first infeasible point, which leaves a bracket 1 / 257^2 <
# 2^-16 of its lower end wide; that (feasible) lower end is the answer.
# ops/functional.py keeps its own text (explicit attacked matrix, bisection).

# Row cap n + f of krum_select(G, f, q, stats=, rule=) (KRUM_ITER_MAX_N).
AGR_MAX_N = 128
_AGR_RULE_CODES = {"krum": 0, "multi-krum": 0, "bulyan": 1}
_AGR_GEO_POINTS = 42
_AGR_LIN_POINTS = 256


def agr_krum_scores(
    G: torch.Tensor,
    a: torch.Tensor,
    b: torch.Tensor,
    c: torch.Tensor,
    f: int,
    gammas: torch.Tensor,
):
    """Krum scores (parameter f) of the attacked set at each of B trial
    gammas, from the honest Gram and the statistics alone: (honest (B, n),
    malicious (B,)). An honest row sums the n - 1 smallest of its n - 1 honest
    distances and f copies of e_i; a malicious row f - 1 zeros and the n - f
    smallest of e. Any device and float dtype, no host sync."""
    n = G.shape[0]
    B = gammas.numel()
    inf = float("inf")
    D2 = sq_dists_from_gram(G)
    D2 = torch.where(torch.isfinite(D2), D2, torch.full_like(D2, inf))
    D2.fill_diagonal_(inf)
    g = gammas.reshape(B, 1)
    e = a[None, :] + 2.0 * g * b[None, :] + g * g * c
    e = torch.where(torch.isfinite(e), e.clamp_min(0.0), torch.full_like(e, inf))
    aug = torch.cat(
        [D2[None, :, :].expand(B, n, n), e[:, :, None].expand(B, n, f)], dim=2
    )
    honest = aug.sort(dim=2).values[:, :, : n - 1].sum(dim=2)
    malicious = e.sort(dim=1).values[:, : n - f].sum(dim=1)
    return honest, malicious


def _agr_krum_flags(G, a, b, c, f: int, q: int, gammas: torch.Tensor):
    """bool (B,): Krum / Multi-Krum with q winners still selects the
    malicious rows — at most max(q - f, 0) honest rows score no worse than a
    malicious one. Anything non-finite is infeasible."""
    honest, malicious = agr_krum_scores(G, a, b, c, f, gammas)
    ok = torch.isfinite(a).all() & torch.isfinite(b).all() & torch.isfinite(c)
    beaten = (~(honest > malicious[:, None])).sum(dim=1)
    return (beaten <= max(q - f, 0)) & ok & torch.isfinite(gammas)


def _agr_gamma_torch(G, a, b, c, f: int, q: int) -> torch.Tensor:
    """The device kernel's grid schedule as torch ops batched over the grid,
    Krum / Multi-Krum only: any device, no host sync."""
    dev, dt = a.device, a.dtype
    zero = torch.zeros((), device=dev, dtype=dt)

    def first_infeasible(flags):
        B = flags.numel()
        k = torch.arange(B, device=dev)
        return torch.where(flags, torch.full_like(k, B), k).min()

    def at(pts, k):  # pts[k] for a 0-dim index tensor, without a host sync
        return pts.index_select(0, k.clamp(0, pts.numel() - 1).reshape(1)).reshape(())

    BG, BL = _AGR_GEO_POINTS, _AGR_LIN_POINTS
    gamma0 = torch.where(
        c > 0, torch.sqrt(a.max().clamp_min(0.0) / torch.where(c > 0, c, 1.0)), zero
    )
    pts = gamma0 * torch.cat(
        [zero[None], 2.0 ** torch.arange(-20, 21, device=dev, dtype=dt)]
    )
    j = first_infeasible(_agr_krum_flags(G, a, b, c, f, q, pts))
    lo = torch.where(j <= 1, zero, at(pts, j - 1))  # j = BG: the top, twice
    hi = torch.where(j <= 1, zero, at(pts, j))
    frac = torch.arange(1, BL + 1, device=dev, dtype=dt) / (BL + 1)
    for _ in range(2):
        pts = lo + (hi - lo) * frac
        j = first_infeasible(_agr_krum_flags(G, a, b, c, f, q, pts))
        lo, hi = (
            torch.where(j == 0, lo, at(pts, j - 1)),
            torch.where(j == BL, hi, at(pts, j)),
        )
    return lo


def _agr_fused(G: torch.Tensor, f: int) -> bool:
    return _gpu(G) and G.dtype == torch.float32 and G.shape[0] + f <= AGR_MAX_N


def agr_tailored_gamma(
    G: torch.Tensor,
    a: torch.Tensor,
    b: torch.Tensor,
    c: torch.Tensor,
    f: int,
    agr: str,
    q: Optional[int] = None,
) -> torch.Tensor:
    """0-dim gamma of the tailored attack from the honest Gram (n, n) and the
    statistics a (n,), b (n,), c () of ``attack_stats``: the feasible end of a
    bracket at most 2^-16 (relative) wide around the largest feasible gamma;
    0 when gamma = 0 is infeasible, c = 0 or a statistic is not finite. On
    device to n + f <= AGR_MAX_N: three grid launches and a finish, no host
    sync. Past that, and on CPU, Krum / Multi-Krum take the same schedule as
    batched torch ops; Bulyan has the device kernel and the functional path
    (``agr_tailored``) only. ``q`` defaults to n for Multi-Krum."""
    n = G.shape[0]
    q = F.agr_check(n, int(f), agr, q)
    if _agr_fused(G, f):
        stats = torch.cat([a.reshape(-1), b.reshape(-1), c.reshape(1)]).float()
        return _hip.require().krum_select(
            G.contiguous(), int(f), int(q), stats=stats.contiguous(),
            rule=_AGR_RULE_CODES[agr],
        )
    if agr == "bulyan":
        raise ValueError(
            "the statistics form of the Bulyan search runs on the device "
            f"kernel only (f32 device Gram, n + f <= {AGR_MAX_N})"
        )
    return _agr_gamma_torch(G, a, b, c, int(f), q)


def agr_tailored(
    X: torch.Tensor,
    f: int,
    agr: str = "multi-krum",
    q: Optional[int] = None,
    perturbation: str = "std",
) -> torch.Tensor:
    """Aggregator-tailored attack vector m = mu + gamma p against ``agr`` in
    "krum" | "multi-krum" | "bulyan" run with f Byzantine rows on the n honest
    rows of X plus f copies of m. On device: the statistics pass, the MFMA
    Gram, the grid search on those O(n^2) numbers, one addcmul — no host sync,
    capturable into a hipGraph. CPU tensors, and Bulyan past n + f =
    AGR_MAX_N, take the functional path."""
    _perturb_code(perturbation)
    n = X.shape[0]
    F.agr_check(n, int(f), agr, q)
    if not _attack_device(X) or (agr == "bulyan" and n + f > AGR_MAX_N):
        return F.agr_tailored(X, int(f), agr, q, perturbation)
    mu, p, a, b, c = attack_stats(X, perturbation)
    gamma = agr_tailored_gamma(gram(X), a, b, c, f, agr, q)
    return torch.addcmul(mu, gamma, p).to(X.dtype)


# Tailored attacks on the coordinate-wise rules (Shejwalkar & Houmansadr
# 2021): f copies of m = mu + gamma p with the gamma that maximises
# D(gamma) = sum_j (mu_j - A_j(gamma))^2, A_j the trimmed mean / median of
# column j's n honest values plus the f copies. Unlike the selection rules
# this objective is a sum over all d columns, so each trial gamma needs a pass
# over X; the device kernel serves 32 trials with one pass: the honest column
# is sorted once, rank k of the attacked column is max(s_{k-f}, min(v, s_k)),
# and the trimmed mean keeps honest rank i iff (s_i < v ? i > f : i <= n - f).
# The search is the fixed schedule written out in ops/functional.py, which
# keeps its own text (explicit attacked matrix, a sort per trial).

AGR_COORD_RULES = ("trimmed-mean", "median")
# Row cap of colsel(X, mode, f, mu=, p=, gammas=) (COORD_MAX_N in
# csrc/launchers.h) and its trials per launch (COORD_MAX_TRIALS).
AGR_COORD_MAX_N = 64
_AGR_COORD_POINTS = 32
_AGR_COORD_ZOOMS = 2
_AGR_COORD_MODES = {"median": _COLSEL_MEDIAN, "trimmed-mean": _COLSEL_TRIMMED}
# The composition works on column chunks sized to keep its (T, 2m, chunk)
# temporaries near this many elements.
_AGR_COORD_CHUNK_ELEMS = 1 << 25


def _agr_coord_objective_torch(X, mu, p, gammas, f: int, agr: str):
    """The kernel's per-column arithmetic as batched torch ops in f64, a
    column chunk at a time: any device, any float dtype, no host sync."""
    n, d = X.shape
    T = gammas.numel()
    g = gammas.double().reshape(T, 1)
    inf = float("inf")
    m = min(f, n - f)
    width = max(2 * m, 4) if agr == "trimmed-mean" else 4
    chunk = max(256, _AGR_COORD_CHUNK_ELEMS // (T * width))
    out = torch.zeros(T, dtype=torch.float64, device=X.device)
    zero = torch.zeros((), dtype=torch.float64, device=X.device)
    for c0 in range(0, d, chunk):
        S = X[:, c0 : c0 + chunk].double().sort(dim=0).values
        muc = mu[c0 : c0 + chunk].double()[None, :]
        v = muc + g * p[c0 : c0 + chunk].double()[None, :]
        if agr == "median":
            # 0-based middle positions q of the n + f values; position q lies
            # between the honest sorted[q - f] and sorted[q]
            def rank(idx, fill):
                if 0 <= idx < n:
                    return S[idx][None, :]
                return torch.full_like(muc, fill)

            cl = []
            for q in ((n + f - 1) // 2, (n + f) // 2):
                lo = rank(q - f, -inf if q - f < 0 else inf)
                hi = rank(q, inf)
                # a NaN ranks last (torch.sort): the smaller of v and hi is
                # NaN only if both are (fmin), the larger if either is
                cl.append(torch.maximum(lo, torch.fmin(v, hi)))
            A = (cl[0] + cl[1]) * 0.5
        else:
            mid = S[f : n - f].sum(dim=0)[None, :]  # always kept; empty: 0
            lo, hi = S[:m][None, :, :], S[n - m :][None, :, :]
            # in the compares a NaN v ranks last, as torch.sort has it
            vt = torch.where(torch.isnan(v), torch.full_like(v, inf), v)[:, None, :]
            kl, kh = ~(lo < vt), hi < vt
            tail = torch.where(kl, lo, zero).sum(dim=1) + torch.where(
                kh, hi, zero
            ).sum(dim=1)
            copies = m - (kl.sum(dim=1) + kh.sum(dim=1))
            vsum = torch.where(copies > 0, copies * v, zero)
            A = (mid + tail + vsum) / float(n - f)
        diff = muc - A
        out += (diff * diff).sum(dim=1)
    return out


def agr_coord_objective(
    X: torch.Tensor,
    mu: torch.Tensor,
    p: torch.Tensor,
    gammas: torch.Tensor,
    f: int,
    agr: str,
) -> torch.Tensor:
    """f64 (T,) vector D[t] = sum_j (mu_j - A_j(gammas[t]))^2 for the honest
    rows X (n, d), given mu and p (d,) — mu need not be the column mean. On
    device for f32 / bf16 X with n <= AGR_COORD_MAX_N: one kernel pass over X
    per 32 trials. Otherwise, and on CPU, the same arithmetic as batched torch
    ops. No host sync either way. Values that are not finite rank as
    torch.sort ranks them (NaN above +inf) on both paths, as in the oracle:
    D is non-finite where such a value, or a non-finite mu, is kept."""
    n = X.shape[0]
    f = int(f)
    F.agr_coord_check(n, f, agr)
    gammas = gammas.reshape(-1)
    if (
        _gpu(X)
        and n <= AGR_COORD_MAX_N
        and X.dtype in (torch.float32, torch.bfloat16)
    ):
        ops = _hip.require()
        Xc = X.contiguous()
        mu32, p32 = mu.float().contiguous(), p.float().contiguous()
        g32 = gammas.to(device=X.device, dtype=torch.float32).contiguous()
        parts = [
            ops.colsel(
                Xc, _AGR_COORD_MODES[agr], f, mu=mu32, p=p32,
                gammas=g32[t0 : t0 + _AGR_COORD_POINTS],
            )
            for t0 in range(0, g32.numel(), _AGR_COORD_POINTS)
        ]
        return parts[0] if len(parts) == 1 else torch.cat(parts)
    return _agr_coord_objective_torch(X, mu, p, gammas.to(X.device), f, agr)


def agr_coord_gamma(
    X: torch.Tensor,
    mu: torch.Tensor,
    p: torch.Tensor,
    a: torch.Tensor,
    c: torch.Tensor,
    f: int,
    agr: str,
    gamma0=None,
) -> torch.Tensor:
    """0-dim gamma of the coordinate-wise tailored attack from the honest rows
    and the statistics mu, p, a (n,), c () of ``attack_stats``: the schedule of
    ops/functional.py (round 0 at 0 and gamma0 2^-15 .. gamma0 2^15, two zoom
    rounds of 32 interior points) as device ops around three objective calls,
    no host sync. The anchor gamma0 defaults to sqrt(max a / c), the Min-Sum
    value, and gamma is then 0 when c = 0 or a statistic is not finite; with
    ``gamma0=`` given a and c are not read (as in the oracle) and gamma is 0
    when gamma0 is not finite. Either way gamma is 0 when no trial's D is
    finite. Every trial is an f32 value, worked out in f64."""
    f = int(f)
    F.agr_coord_check(X.shape[0], f, agr)
    dev = X.device
    f64 = dict(device=dev, dtype=torch.float64)
    zero = torch.zeros((), **f64)
    ninf = torch.full((), -float("inf"), **f64)
    if gamma0 is None:
        a64, c64 = a.to(**f64), c.to(**f64).reshape(())
        ok = (c64 > 0) & torch.isfinite(c64)
        g0 = torch.sqrt(a64.max() / torch.where(ok, c64, torch.ones_like(c64)))
    else:  # as in the oracle: a given anchor is taken as it is, a and c unread
        g0 = torch.as_tensor(gamma0, **f64).reshape(())
        ok = torch.ones((), dtype=torch.bool, device=dev)
    g0 = g0.float().double()
    ok = ok & torch.isfinite(g0)
    g0 = torch.where(ok, g0, zero)

    def better(D, g, best_D, best_g):
        return torch.isfinite(D) & ((D > best_D) | ((D == best_D) & (g < best_g)))

    def evaluate(trials, best_g, best_D):
        """Best of the incumbent and the ascending trials."""
        D = agr_coord_objective(X, mu, p, trials.float(), f, agr).double()
        Dm = torch.where(torch.isfinite(D), D, ninf)
        top = Dm.max()
        # the first (smallest gamma) trial that reaches the round's maximum
        k = torch.arange(trials.numel(), device=dev)
        first = torch.where(Dm == top, k, torch.full_like(k, trials.numel())).min()
        g = trials.index_select(0, first.clamp_max(trials.numel() - 1).reshape(1))
        g = g.reshape(())
        take = better(top, g, best_D, best_g)
        return torch.where(take, g, best_g), torch.where(take, top, best_D)

    geo = 2.0 ** torch.arange(-15, 16, **f64)
    trials = torch.cat([zero[None], (g0 * geo).float().double()])
    nodes = trials
    best_g, best_D = zero, ninf
    frac = torch.arange(1, _AGR_COORD_POINTS + 1, **f64)
    for r in range(1 + _AGR_COORD_ZOOMS):
        best_g, best_D = evaluate(trials, best_g, best_D)
        if r == _AGR_COORD_ZOOMS:
            break
        below = torch.where(nodes < best_g, nodes, ninf).max()
        above = torch.where(nodes > best_g, nodes, -ninf).min()
        lo = torch.where(torch.isfinite(below), below, best_g)
        hi = torch.where(torch.isfinite(above), above, best_g)
        trials = (lo + (hi - lo) * frac / (_AGR_COORD_POINTS + 1)).float().double()
        nodes = torch.cat([lo[None], trials, hi[None]])
    return torch.where(ok, best_g, zero).to(a.dtype)


def agr_coord(
    X: torch.Tensor,
    f: int,
    agr: str = "trimmed-mean",
    perturbation: str = "std",
) -> torch.Tensor:
    """Attack vector m = mu + gamma p against ``agr`` in "trimmed-mean" |
    "median" run on the n honest rows of X plus f copies of m. On device: the
    statistics pass, three objective passes, one addcmul — no host sync,
    capturable into a hipGraph. CPU tensors take the functional path."""
    _perturb_code(perturbation)
    F.agr_coord_check(X.shape[0], int(f), agr)
    if not _attack_device(X):
        return F.agr_coord(X, int(f), agr, perturbation)
    mu, p, a, _, c = attack_stats(X, perturbation)
    gamma = agr_coord_gamma(X, mu, p, a, c, f, agr)
    return torch.addcmul(mu, gamma.to(mu.dtype), p).to(X.dtype)


# -- remaining ops: torch composition on either device ----------------------


def minimum_diameter_averaging(X: torch.Tensor, f: int) -> torch.Tensor:
    n = X.shape[0]
    m = n - f
    if _gpu(X):
        D2 = pairwise_sq_dists(X)
        if n <= 64 and 2 <= m < n:
            # fully device-side two-pass branch-and-bound (subsets.hip):
            # no host D2 copy, no host sync — the winning (lex-smallest
            # optimal) subset is selected with a cumsum one-hot mask.
            # Seed the shared bound with a cheap anchor-greedy upper
            # bound (diameter of each row's m nearest rows) so pass 1
            # prunes like the host B&B instead of starting from +inf.
            idxn = torch.topk(D2, k=m, dim=1, largest=False).indices
            sub = D2[idxn[:, :, None], idxn[:, None, :]]  # (n, m, m)
            ub = sub.amax(dim=(1, 2)).min()
            found, subsets = _hip.require().mda_select(D2, int(f), ub)
            if not bool(found.any()):  # degenerate (e.g. all-inf D2)
                subset = F.mda_subset(D2, f)
                idx = torch.tensor(subset, device=X.device, dtype=torch.long)
                return mean_rows(X, idx)
            first = ((found.cumsum(0) == 1) & (found == 1)).to(subsets.dtype)
            subset_t = (subsets * first[:, None]).sum(dim=0).to(torch.int32)
            return mean_rows(X, subset_t)
        subset = F.mda_subset(D2, f)
        idx = torch.tensor(subset, device=X.device, dtype=torch.long)
        return mean_rows(X, idx)
    return F.minimum_diameter_averaging(X, f)


def monna(X: torch.Tensor, f: int, reference_index: int = 0) -> torch.Tensor:
    n = X.shape[0]
    k = n - f
    if _gpu(X):
        # ||x - r||^2 = ||x||^2 + ||r||^2 - 2 x.r ; reuse the norm kernel
        norms = row_sqnorms(X)
        dots = (X.float() @ X.float()[reference_index]).flatten()
        d2 = norms + norms[reference_index] - 2.0 * dots
        d2[reference_index] = -1.0
        idx = torch.argsort(d2, stable=True)[:k]
        return mean_rows(X, idx)
    return F.monna(X, f, reference_index)


_SMEA_COMBOS: dict = {}
_SMEA_COMBOS_MAX_CACHED = 4  # FIFO cap: a combos tensor can be ~33 MB
_SMEA_MAX_COMBOS = 1 << 17


def smea(X: torch.Tensor, f: int) -> torch.Tensor:
    import itertools
    import math

    n = X.shape[0]
    m = n - f
    if (
        _gpu(X)
        and 1 <= m <= 64
        and n <= 128
        and math.comb(n, m) <= _SMEA_MAX_COMBOS
    ):
        # device path (subsets.hip): one wave per subset runs a cyclic
        # Jacobi eigensolve on the centered subset Gram in LDS; the
        # packed (eig, combo) atomicMin reproduces the oracle's
        # lex-smallest tie-break. Combos cached per shape.
        key = (n, m, X.device.index)
        combos = _SMEA_COMBOS.get(key)
        if combos is None:
            if len(_SMEA_COMBOS) >= _SMEA_COMBOS_MAX_CACHED:
                _SMEA_COMBOS.pop(next(iter(_SMEA_COMBOS)))
            combos = torch.tensor(
                list(itertools.combinations(range(n), m)),
                dtype=torch.int32,
                device=X.device,
            )
            _SMEA_COMBOS[key] = combos
        G = gram(X)
        best = _hip.require().smea_select(G, combos)
        idx = (best[0] & 0xFFFFFFFF).long()
        rows = combos[idx].to(torch.int32)
        return mean_rows(X, rows)
    return F.smea(X, f)


class _CafGraphBlock:
    """R CAF rounds captured into one hipGraph (torch.cuda.CUDAGraph is
    hipGraph on ROCm) with DEVICE-side best-lambda/active tracking — the
    eager loop's one-host-sync-per-round made CAF only ~8x the CPU
    reference at 64x65k (round-1 weakness; NOTES_R02 item 3). One replay =
    R rounds = zero Python dispatch and one sync per R rounds.

    Round semantics match F.caf exactly: wsum/mu/power-iteration/best
    tracking per reference caf.py:133-184; rounds after the stop condition
    (weight mass <= n-2f, or the n-round cap via ``rounds_left``) are
    masked out with ``active`` so replaying a full block never corrupts
    the result."""

    def __init__(self, n: int, d: int, dtype, f: int, power_iters: int,
                 R: int, device) -> None:
        ext = _hip.require()
        self.R, self.n, self.d = R, n, d
        self.power_iters = max(1, int(power_iters))
        self.target = float(n - 2 * f)
        self.X = torch.zeros(n, d, dtype=dtype, device=device)
        self.seeds = torch.zeros(R, d, dtype=torch.float32, device=device)
        self.w = torch.ones(n, device=device)
        self.best_lambda = torch.full((), float("inf"), device=device)
        self.best_mu = torch.zeros(d, device=device)
        self.active = torch.ones((), dtype=torch.bool, device=device)
        self.rounds_left = torch.full((), float(n), device=device)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._block(ext)  # warmup (allocator pools the intermediates)
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._block(ext)

    def _block(self, ext) -> None:
        X = self.X
        for r in range(self.R):
            w = self.w
            active_in = self.active.clone()
            rl = self.rounds_left.clone()
            wsum = w.sum()
            inv_wsum = torch.reciprocal(wsum.clamp_min(1e-30))
            mu = ext.caf_colsum(X, w, None, inv_wsum)
            v = self.seeds[r]
            v = v / v.norm().clamp_min(1e-20)
            lam = torch.zeros((), device=X.device)
            for _ in range(self.power_iters):
                s_ = ext.caf_matvec(X, mu, v)
                t_ = ext.caf_colsum(X, w * s_, mu, inv_wsum)
                lam = t_.norm()
                v = t_ / lam.clamp_min(1e-20)
            proj = ext.caf_matvec(X, mu, v) ** 2
            pmax = proj.max().clamp_min(1e-20)
            w_next = (w * (1.0 - proj / pmax)).clamp_min(0.0)
            better = (lam < self.best_lambda) & active_in
            self.best_mu.copy_(torch.where(better, mu, self.best_mu))
            self.best_lambda.copy_(torch.where(better, lam, self.best_lambda))
            stop = (wsum <= self.target) | (w_next.sum() <= 0)
            active_next = active_in & ~stop & (rl > 1.0)
            self.w.copy_(torch.where(active_next, w_next, w))
            self.active.copy_(active_next)
            self.rounds_left.copy_(rl - 1.0)

    def run(self, X: torch.Tensor) -> torch.Tensor:
        gen = torch.Generator(device="cpu")
        gen.manual_seed(0)
        self.X.copy_(X)
        self.w.fill_(1.0)
        self.best_lambda.fill_(float("inf"))
        self.best_mu.copy_(self.X.mean(dim=0, dtype=torch.float32))
        self.active.fill_(True)
        self.rounds_left.fill_(float(self.n))
        # seeds drawn in the ORACLE's block pattern (rng stream parity with
        # F.caf, which draws min(block_rows, n-r) rows at a time)
        block_rows = max(1, min(4, (1 << 27) // max(self.d, 1)))
        pending: list = []
        drawn = 0
        total = 0
        self.last_replays = 0
        while total < self.n:
            self.last_replays += 1
            need = min(self.R, self.n - total)
            while sum(p.shape[0] for p in pending) < need and drawn < self.n:
                rows = min(block_rows, self.n - drawn)
                pending.append(torch.randn(rows, self.d, generator=gen))
                drawn += rows
            flat = torch.cat(pending, dim=0) if len(pending) > 1 else pending[0]
            self.seeds[:need].copy_(flat[:need])
            pending = [flat[need:]] if flat.shape[0] > need else []
            self.graph.replay()
            total += self.R  # a partial tail block is masked by rounds_left
            if not bool(self.active):  # one sync per R rounds
                break
        return self.best_mu.to(X.dtype)


_CAF_GRAPHS: dict = {}
_CAF_GRAPHS_MAX = 4  # FIFO cap: each block pins X + seeds device buffers

# graph path bounds: seeds are staged per replay (R*d f32 H2D), so cap d;
# n caps the round count (and kernel TORCH_CHECKs n <= 1024)
_CAF_GRAPH_MAX_D = 1 << 21


def _caf_graph_ok(X: torch.Tensor, f: int) -> bool:
    # OFF by default: measured on MI355X, a replayed 8-round block runs
    # ~3x slower per round than the eager loop (2.1 ms/replay at 64x65k
    # vs ~85 us/round eager; graph 1.9 vs eager 0.97 ms even at 32x2048),
    # so capture only pays when Python dispatch is the true bottleneck —
    # opt in with BYZPY_CAF_GRAPH=1. The block stays parity-tested.
    import os

    if os.environ.get("BYZPY_CAF_GRAPH", "0") != "1":
        return False
    n, d = X.shape
    return n <= 256 and d <= _CAF_GRAPH_MAX_D


def caf(X: torch.Tensor, f: int, *, power_iters: int = 3) -> torch.Tensor:
    """Covariance-agnostic filter on fused K9 kernels (reference
    caf.py:133-184): caf_matvec computes s = (X - mu) @ v, caf_colsum
    computes weighted centered column sums — neither materializes the
    (n, d) f32 diffs matrix and both replace rocblas gemvt (~260 GB/s on
    this skinny shape). Same algorithm and seeded-rng contract as the
    functional oracle. Steady-state shapes run the hipGraph block path
    (_CafGraphBlock); others fall back to the eager loop below."""
    import math
    import os

    n = X.shape[0]
    if not (_gpu(X) and n <= 1024 and n - 2 * f > 0):
        return F.caf(X, f, power_iters=power_iters)
    if _caf_graph_ok(X, f):
        d = X.shape[1]
        R = min(8, n)
        key = (n, d, X.dtype, int(f), int(power_iters), R, X.device.index)
        blk = _CAF_GRAPHS.get(key)
        if blk is None:
            if len(_CAF_GRAPHS) >= _CAF_GRAPHS_MAX:
                _CAF_GRAPHS.pop(next(iter(_CAF_GRAPHS)))
            blk = _CafGraphBlock(n, d, X.dtype, int(f), power_iters, R, X.device)
            _CAF_GRAPHS[key] = blk
        return blk.run(X.contiguous())
    ext = _hip.require()
    d = X.shape[1]
    dev = X.device
    w = torch.ones(n, device=dev)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(0)
    best_lambda = math.inf
    best_mu = X.float().mean(dim=0)
    target = float(n - 2 * f)
    block_rows = max(1, min(4, (1 << 27) // max(d, 1)))
    # At the steady-state shapes (n<=1024, d~65k) the per-round kernel
    # work is a few us — the round cost is host latency: the 3-scalar
    # break-condition sync and the pageable seed-block H2D. Both are
    # hidden without changing any computed value: round r+1's kernels
    # launch while round r's stat readback rides an async pinned copy
    # (speculative rounds launched past a break point are discarded —
    # they only ever consumed RNG stream, never affected the output),
    # and seed blocks stage through double-buffered pinned memory.
    sync_mode = os.environ.get("BYZPY_CAF_SYNC", "0") == "1"  # A/B probe aid
    nopin = os.environ.get("BYZPY_CAF_NOPIN", "0") == "1"  # A/B probe aid
    pin_seeds = (
        not sync_mode and not nopin and block_rows * d * 4 <= (64 << 20)
    )
    if pin_seeds:
        seed_pin = [
            torch.empty(block_rows, d, pin_memory=True) for _ in range(2)
        ]
        seed_dev = [torch.empty(block_rows, d, device=dev) for _ in range(2)]
        seed_ev = [torch.cuda.Event() for _ in range(2)]
    stat_pin = [torch.empty(3, pin_memory=True) for _ in range(2)]
    stat_ev = [torch.cuda.Event() for _ in range(2)]
    pending: list = []  # (mu, slot) rounds not yet validated for break

    def consume_oldest() -> bool:
        nonlocal best_lambda, best_mu
        mu_p, sp = pending.pop(0)
        stat_ev[sp].synchronize()
        wsum_f, wnext_f, lam_f = stat_pin[sp].tolist()
        if lam_f < best_lambda:
            best_lambda = lam_f
            best_mu = mu_p
        return wsum_f <= target or wnext_f <= 0

    seeds = torch.empty(0)
    broke = False
    for r in range(n):
        if r % block_rows == 0:
            rows = min(block_rows, n - r)
            if pin_seeds:
                blk = (r // block_rows) % 2
                seed_ev[blk].synchronize()  # prior H2D out of this slot done
                torch.randn(rows, d, generator=gen, out=seed_pin[blk][:rows])
                seed_dev[blk][:rows].copy_(seed_pin[blk][:rows], non_blocking=True)
                seed_ev[blk].record()
                seeds = seed_dev[blk]
            else:
                seeds = torch.randn(rows, d, generator=gen).to(dev)
        wsum = w.sum()
        inv_wsum = torch.reciprocal(wsum.clamp_min(1e-30))
        mu = ext.caf_colsum(X, w, None, inv_wsum)
        v = seeds[r % block_rows]
        v = v / v.norm().clamp_min(1e-20)
        lam = torch.zeros((), device=dev)
        for _ in range(max(1, power_iters)):
            s = ext.caf_matvec(X, mu, v)
            t = ext.caf_colsum(X, w * s, mu, inv_wsum)
            lam = t.norm()
            v = t / lam.clamp_min(1e-20)
        proj = ext.caf_matvec(X, mu, v) ** 2
        pmax = proj.max().clamp_min(1e-20)
        w_next = (w * (1.0 - proj / pmax)).clamp_min(0.0)
        slot = r % 2
        stat_pin[slot].copy_(
            torch.stack([wsum, w_next.sum(), lam]), non_blocking=True
        )
        stat_ev[slot].record()
        pending.append((mu, slot))
        w = w_next
        if len(pending) == (1 if sync_mode else 2) and consume_oldest():
            broke = True  # the still-pending round is speculative: discard
            break
    while not broke and pending:
        if consume_oldest():
            break
    return best_mu.to(X.dtype)
