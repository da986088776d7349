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


# Row lists (K19): ``median``, ``trimmed_mean``, ``mean_of_medians``, ``gram``,
# ``mean_rows``, ``multi_krum`` and ``krum`` also take, in place of the (n, d)
# matrix, a list or tuple of n <= ROW_LIST_MAX_N flat device tensors (one
# dtype, f32 or bf16, one length, one device, each contiguous) and read the
# rows where they are: the kernels get the n pointers as a by-value kernel
# argument, so no (n, d) copy is stacked and nothing is allocated but the
# result (csrc/rowptrs.hip, the ROWS_PTRS kernels of csrc/colsel.hip). The
# binding checks the list. Measured on MI355X against stacking first
# (benchmarks/RESULTS_MI355X_rows.md): the public call in place took 0.21-0.92
# of the stacked call's time at EVERY measured shape (64 x 64K, 1M, 16M and
# 33 x 16M, bf16 and f32), so the route has no d threshold.
ROW_LIST_MAX_N = 64


def _row_list(X) -> bool:
    return isinstance(X, (list, tuple))


def _colsel_row_list(rows, mode: int, f: int) -> torch.Tensor:
    return _hip.require().colsel(list(rows), mode, int(f))


def _group_counts(groups: torch.Tensor):
    """Valid entries per row of a groups table. gossip_groups leaves them on
    the tensor it builds; any other device table is copied to the host."""
    counts = getattr(groups, "valid_counts", None)
    if counts is None:
        counts = (groups >= 0).sum(dim=1).tolist()
    return counts


def _colsel_groups(X, mode: int, f: int, groups, rows, per_node):
    """``groups=`` of median / trimmed_mean / mean_of_medians (K24): the
    statistic for every row set of an (M, m) table (gossip_groups, or a list
    of row lists) at once, (M, d). A device f32 / bf16 matrix of N <=
    COLSEL_GROUPS_MAX_N rows with M <= COLSEL_GROUPS_MAX_N and m <=
    COLSEL_GROUPS_MAX_M is one pass over X (colsel_groups.hip); anything else
    is ``per_node`` on X[g] per node, stacked."""
    if rows is not None or _row_list(X):
        raise ValueError("groups= goes with one (N, d) matrix and without rows=")
    if not isinstance(groups, torch.Tensor):
        groups = gossip_groups(groups, X.device)
    if groups.dim() != 2 or groups.shape[0] < 1 or groups.shape[1] < 1:
        raise ValueError("groups must be a non-empty (M, m) table")
    counts = _group_counts(groups)
    f = int(f)
    need = f + 1 if mode == _COLSEL_MEAMED else 2 * f + 1
    if f < 0 or min(counts) < need:
        raise ValueError(
            f"f={f} needs at least {need} rows per node, the smallest has {min(counts)}"
        )
    M, m = groups.shape
    if (
        _gpu(X)
        and X.dtype in (torch.float32, torch.bfloat16)
        and X.shape[0] <= COLSEL_GROUPS_MAX_N
        and M <= COLSEL_GROUPS_MAX_N
        and m <= COLSEL_GROUPS_MAX_M
    ):
        grp = groups.to(device=X.device, dtype=torch.int32).contiguous()
        return _hip.require().colsel(
            X.contiguous(), mode, f, groups=grp, min_m=int(min(counts))
        )
    lists = [[j for j in g if j >= 0] for g in groups.tolist()]
    return torch.stack([per_node(X[g]) for g in lists])


def median(
    X: torch.Tensor, rows: Optional[torch.Tensor] = None, groups=None
) -> torch.Tensor:
    """``rows`` (m distinct row indices) restricts the statistic to those
    rows, as if on X[rows]; ``groups`` (an (M, m) table of row sets, -1 pads)
    gives the (M, d) statistics of all its sets; same for trimmed_mean and
    mean_of_medians."""
    if groups is not None:
        return _colsel_groups(X, _COLSEL_MEDIAN, 0, groups, rows, median)
    if _row_list(X):
        return _colsel_row_list(X, _COLSEL_MEDIAN, 0)
    if rows is not None:
        out = _colsel_rows(X, _COLSEL_MEDIAN, 0, rows) if _gpu(X) else None
        return out if out is not None else median(X[rows.long()])
    if _gpu(X) and X.shape[0] <= COLSEL_MAX_N:
        return _hip.require().colsel(X.contiguous(), _COLSEL_MEDIAN, 0)
    return F.median(X)


def trimmed_mean(
    X: torch.Tensor, f: int, rows: Optional[torch.Tensor] = None, groups=None
) -> torch.Tensor:
    if groups is not None:
        return _colsel_groups(
            X, _COLSEL_TRIMMED, f, groups, rows, lambda Y: trimmed_mean(Y, f)
        )
    if _row_list(X):
        return _colsel_row_list(X, _COLSEL_TRIMMED, f)
    if rows is not None:
        out = _colsel_rows(X, _COLSEL_TRIMMED, f, rows) if _gpu(X) else None
        return out if out is not None else trimmed_mean(X[rows.long()], f)
    if _gpu(X) and X.shape[0] <= COLSEL_MAX_N:
        return _hip.require().colsel(X.contiguous(), _COLSEL_TRIMMED, int(f))
    return F.trimmed_mean(X, f)


def mean_of_medians(
    X: torch.Tensor, f: int, rows: Optional[torch.Tensor] = None, groups=None
) -> torch.Tensor:
    if groups is not None:
        return _colsel_groups(
            X, _COLSEL_MEAMED, f, groups, rows, lambda Y: mean_of_medians(Y, f)
        )
    if _row_list(X):
        return _colsel_row_list(X, _COLSEL_MEAMED, f)
    if rows is not None:
        out = _colsel_rows(X, _COLSEL_MEAMED, f, rows) if _gpu(X) else None
        return out if out is not None else mean_of_medians(X[rows.long()], f)
    if _gpu(X) and X.shape[0] <= COLSEL_MAX_N:
        return _hip.require().colsel(X.contiguous(), _COLSEL_MEAMED, int(f))
    return F.mean_of_medians(X, f)


# -- pairwise distances / Krum (K4, K5) -------------------------------------


# Row cap of gram(X, center=True) (GRAM_CENTERED_MAX_N in csrc/launchers.h).
GRAM_CENTERED_MAX_N = 128


def _gram_centered_torch(X: torch.Tensor) -> torch.Tensor:
    """The centred Gram as torch ops: the kernel's arithmetic in kind (f32,
    finite-aware column mean, one bf16 rounding of x - mu for bf16 input), at
    the cost of three more passes over X and two (n, d) f32 temporaries."""
    Xf = X.float()
    fin = torch.isfinite(Xf)
    mu = torch.where(fin, Xf, torch.zeros_like(Xf)).sum(dim=0)
    mu = mu / fin.sum(dim=0).clamp(min=1)
    Xc = Xf - mu[None, :]
    if X.dtype == torch.bfloat16:
        Xc = Xc.bfloat16().float()
    return Xc @ Xc.T


def gram(X: torch.Tensor, center: bool = False) -> torch.Tensor:
    """X @ X.T with f32 accumulation; MFMA split-K kernel on device.

    ``center=True`` (K22, csrc/gram_centered.hip): the Gram of the rows
    centred by their column mean, Gc = (X - 1 mu^T)(X - 1 mu^T)^T. Squared
    distances G_ii + G_jj - 2 G_ij are the same on either Gram, but on the
    raw one their f32 cancellation error is relative to ||x||^2, and rows
    that share a large component (parameter vectors, momenta, late
    gradients) are then told apart by summation noise; on the centred one it
    is relative to ||y||^2, y_i = x_i - mu. Accuracy model: f32 input leaves
    accumulation error only, relative to ||y||^2. bf16 input rounds y once
    (an element moves by 2^-9 of itself in the mean, 2^-8 at worst), so a
    distance is off by about 2^-9 (||y_i|| + ||y_j||): under 2^-7 of D_ij for rows scattered round
    their mean; a pair far closer to each other than to the mean (a mimic
    pair) is resolved only down to 2^-9 of its distance from the mean.
    mu_j is the mean over column j's finite entries (0 if none) and a
    non-finite entry stays non-finite: a row holding inf or NaN has a
    non-finite Gc_ii and row / column of Gc, every other entry is clean, so
    "non-finite diagonal = dead row" keeps working downstream.

    Device matrices of n <= GRAM_CENTERED_MAX_N rows (f32 or bf16, any d)
    take one pass over X in one kernel. More rows, other dtypes and CPU
    tensors take ``_gram_centered_torch``: three more passes over X and two
    (n, d) f32 temporaries. Row lists are not taken: stack them first."""
    if center:
        if _row_list(X):
            raise ValueError("gram(center=True) takes an (n, d) matrix, not a row list")
        if (
            _gpu(X)
            and X.dtype in (torch.float32, torch.bfloat16)
            and 1 <= X.shape[0] <= GRAM_CENTERED_MAX_N
            and X.shape[1] >= 1
        ):
            return _hip.require().gram(X.contiguous(), center=True)
        return _gram_centered_torch(X)
    if _row_list(X):
        return _hip.require().gram(list(X))
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


# ``centered=True`` on the distance rules below takes the distances from
# gram(X, center=True) and feeds the same helpers: the rule is unchanged, the
# distances of near-equal rows are resolved (see gram). CPU tensors then take
# the same chain on gram's torch fallback, not the functional oracle.


def pairwise_sq_dists(X: torch.Tensor, centered: bool = False) -> torch.Tensor:
    if _gpu(X) or centered:
        return sq_dists_from_gram(gram(X, center=centered))
    return F.pairwise_sq_dists(X)


def multi_krum_scores(X: torch.Tensor, f: int, centered: bool = False) -> torch.Tensor:
    n = X.shape[0]
    if n - f - 1 < 1:
        raise ValueError(f"need n - f - 1 >= 1, got n={n}, f={f}")
    if _gpu(X) or centered:
        return krum_scores_from_gram(gram(X, center=centered), f)
    return F.multi_krum_scores(X, f)


def multi_krum(X: torch.Tensor, f: int, q: int, centered: bool = False) -> torch.Tensor:
    if _row_list(X) or _gpu(X) or centered:
        G = gram(X, center=centered)
        return mean_rows(X, krum_winners_from_gram(G, f, q))
    return F.multi_krum(X, f, q)


def krum(X: torch.Tensor, f: int, centered: bool = False) -> torch.Tensor:
    if _row_list(X):
        # the q = 1 mean is the winner itself, and it never visits the host
        G = gram(X, center=centered)
        return mean_rows(X, krum_winners_from_gram(G, f, 1))
    if _gpu(X) and X.shape[0] <= 512:
        idx = krum_winners_from_gram(gram(X, center=centered), f, 1)
        return X[idx.long()[0]].clone()
    scores = multi_krum_scores(X, f, centered)
    return X[int(torch.argmin(scores))].clone()


def bulyan(X: torch.Tensor, f: int, centered: bool = False) -> torch.Tensor:
    """Bulyan (El Mhamdi et al. 2018): Gram -> n - 2f rows by iterated Krum
    -> per coordinate the mean of the n - 4f selected values closest to
    their median. On device: MFMA Gram, one selection launch, one indexed
    mean-around-median launch reading the selected rows in place — no
    (theta, d) gather and no host sync."""
    n = X.shape[0]
    _check_bulyan(n, f)
    if f == 0:
        return mean_of_medians(X, 0)
    sel = bulyan_select_from_gram(gram(X, center=centered), f)
    return mean_of_medians(X, 2 * f, rows=sel)


def mean_rows(X: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """Mean of the selected rows, f32 accumulation (K10 gather-mean)."""
    if _row_list(X):
        idx32 = idx.to(device=X[0].device, dtype=torch.int32).contiguous()
        return _hip.require().mean_rows(list(X), idx32)
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


# -- fixed points on the Gram (K20) -------------------------------------------
#
# ``solver="gram"`` of geometric_median and centered_clipping. A Weiszfeld
# update is a convex combination of the rows whatever the centre is, and a
# clipping update keeps v in the row span when v starts as the mean or zero.
# So the iterate is z = sum_i a_i x_i, and with G = X X^T
#   ||x_i - z||^2 = G_ii - 2 (G a)_i + a^T G a,
#   ||z' - z||^2  = (a' - a)^T G (a' - a):
# the whole loop, convergence test included, runs on n numbers in one launch
# (csrc/gramfp.hip) and X is read twice in all, once for the Gram and once
# to form sum_i a_i x_i (``mean_rows(X, coeffs=a)``, csrc/rowptrs.hip),
# against two passes per step for the iterative kernels. Opt-in, because the
# distances come from an f32 Gram: a row closer to the centre than roughly
# 2^-11 of its own norm is not resolved (the cancellation in
# G_ii - 2 u_i + q leaves an error of about 2^-23 ||x_i||^2 in d_i^2), and its
# weight saturates at that floor, not at eps. A row with a non-finite G_ii is
# dead: coefficient 0, never read by the combine.
#
# The device route takes f32 / bf16 device matrices of n <= GRAMFP_MAX_N rows
# and row lists (n <= ROW_LIST_MAX_N); everything else runs the same
# arithmetic as f64 torch ops (F.gram_fixed_point), which may sync.

# Row cap of weiszfeld_iter(G, a0, ...), cc_iter(G, a0, ...) and
# mean_rows(X, coeffs=) (GRAMFP_MAX_N in csrc/launchers.h).
GRAMFP_MAX_N = 128
SOLVERS = ("iterative", "gram")


def _check_solver(solver: str) -> None:
    if solver not in SOLVERS:
        raise ValueError("solver must be 'iterative' or 'gram'")


def _gramfp_fused(X) -> bool:
    if _row_list(X):
        return len(X) <= ROW_LIST_MAX_N and all(r.is_cuda for r in X)
    return (
        _gpu(X)
        and X.dtype in (torch.float32, torch.bfloat16)
        and 1 <= X.shape[0] <= GRAMFP_MAX_N
        and X.shape[1] >= 1
    )


def gram_fixed_point(
    G: torch.Tensor,
    a0: torch.Tensor,
    *,
    rule: str,
    iters: int,
    eps: float = 1e-12,
    tol: float = 0.0,
    c_tau: float = 0.0,
):
    """(a, steps, shift2) of F.gram_fixed_point: one launch and no host sync
    for an f32 device Gram of n <= GRAMFP_MAX_N rows (steps and shift2 stay
    device scalars), the f64 torch loop otherwise."""
    if _gpu(G) and G.dtype == torch.float32 and G.shape[0] <= GRAMFP_MAX_N:
        ext = _hip.require()
        a0 = a0.to(device=G.device, dtype=torch.float32).contiguous()
        if rule == "weiszfeld":
            return tuple(ext.weiszfeld_iter(
                G.contiguous(), a0, eps=float(eps), tol=float(tol), iters=int(iters)
            ))
        if rule != "cc":
            raise ValueError("rule must be 'weiszfeld' or 'cc'")
        a = ext.cc_iter(
            G.contiguous(), a0, c_tau=float(c_tau), eps=float(eps), iters=int(iters)
        )
        return a, int(iters), None
    return F.gram_fixed_point(
        G, a0, rule=rule, iters=iters, eps=eps, tol=tol, c_tau=c_tau
    )


def combine_rows(X, a: torch.Tensor) -> torch.Tensor:
    """sum_i a_i x_i in X's dtype, not normalised; rows with a_i == 0 are not
    read. f32 accumulation in row order on the device (a list and its stacked
    matrix give the same bits), f64 elsewhere."""
    if _gramfp_fused(X):
        dev = X[0].device if _row_list(X) else X.device
        a32 = a.to(device=dev, dtype=torch.float32).contiguous()
        rows = list(X) if _row_list(X) else X.contiguous()
        return _hip.require().mean_rows(rows, coeffs=a32)
    keep = a != 0
    return (a[keep].double() @ X[keep].double()).to(X.dtype)


def solver_gram(X, centered: bool = False) -> torch.Tensor:
    """The Gram the K20 / K21 solvers run on. ``centered=True``: the centred
    one (gram(X, center=True)), which is exact for a loop whose coefficients
    sum to 1 throughout, since then sum_i a_i (x_i - mu) = z - mu and every
    distance and shift is that of the raw rows. Only Weiszfeld from the mean
    is such a loop here; the callers refuse the rest."""
    if centered:
        if _row_list(X):
            X = torch.stack(list(X))
        if _gramfp_fused(X):
            return gram(X, center=True)
        Xd = X.double()
        fin = torch.isfinite(Xd)
        mu = torch.where(fin, Xd, torch.zeros_like(Xd)).sum(dim=0)
        Xd = Xd - (mu / fin.sum(dim=0).clamp(min=1))[None, :]
        return Xd @ Xd.T
    if _gramfp_fused(X):
        return gram(X)
    Xd = X.double()
    return Xd @ Xd.T


def _live_uniform(G: torch.Tensor) -> torch.Tensor:
    """The coefficients of the mean of the rows with a finite G_ii."""
    live = torch.isfinite(torch.diagonal(G)).to(G.dtype)
    return live / live.sum().clamp(min=1.0)


def mixed_gram(G: torch.Tensor, mix: torch.Tensor):
    """(G_Y, W) for the mixed rows Y = W X, W = mix / its row counts in f64:
    G_Y = W G W^T in G's dtype, and coefficients a over the rows of Y pull
    back to W^T a over the rows of X. A mixed row that contains a dead row of
    X (non-finite G_ii) gets an infinite diagonal entry, so it is dead too."""
    W = mix.to(device=G.device, dtype=torch.float64)
    W = W / W.sum(dim=1, keepdim=True)
    Gd = G.double()
    dead = ~torch.isfinite(torch.diagonal(Gd))
    Gd = torch.where(torch.isfinite(Gd), Gd, torch.zeros_like(Gd))
    GY = W @ Gd @ W.T
    dead_y = (W * dead.double()[None, :]).sum(dim=1) > 0
    inf = torch.full_like(dead_y, float("inf"), dtype=torch.float64)
    GY = GY + torch.diag(torch.where(dead_y, inf, torch.zeros_like(inf)))
    return GY.to(G.dtype), W


def _geometric_median_gram(
    X, *, tol, max_iter, eps, init, fixed_iters, init_z, mix=None, G=None,
    centered=False,
) -> torch.Tensor:
    """geometric_median(solver="gram"). ``init="mean"``: a0 is uniform over
    the live rows. ``init="median"`` / ``init_z``: z0 is outside the span but
    the first update is not, so that step uses real distances
    (row_center_sqdists, one more pass) and the solver runs the rest; its
    shift is not tested. ``mix`` (m, n) runs the rule on the mixed rows
    (mixed_gram) without forming them; ``G`` passes a Gram already at hand.
    ``centered`` solves on the centred Gram (solver_gram): mean init only,
    where the distances resolve rows down to 2^-11 of ||x_i - mu||, not of
    ||x_i||; the combine still reads the raw rows, right because sum a = 1."""
    if init not in ("median", "mean"):
        raise ValueError("init must be 'median' or 'mean'")
    if centered and (init != "mean" or init_z is not None):
        raise ValueError(
            "centered=True needs init='mean' and no init_z: the coefficients "
            "must sum to 1 from the first step"
        )
    if _row_list(X) and not _gramfp_fused(X):
        X = torch.stack(list(X))
    fused = _gramfp_fused(X)
    iters = int(fixed_iters) if fixed_iters is not None else int(max_iter)
    tol = 0.0 if fixed_iters is not None else float(tol)
    z0 = None
    if init_z is not None:
        z0 = init_z.detach()
    elif init == "median" and mix is None:
        if fused and not _row_list(X) and G is None and _median_gram_fused_ok(X):
            z0, G = median_and_gram(X)
        else:
            z0 = median(X)
    if G is None:
        G = solver_gram(X, centered)
    W = None
    if mix is not None:
        G, W = mixed_gram(G, mix)
    if z0 is None:
        a = _live_uniform(G)
    else:
        if fused:
            Xm = torch.stack(list(X)) if _row_list(X) else X.contiguous()
            z0 = z0.to(device=Xm.device, dtype=torch.float32).contiguous()
            s = _hip.require().row_center_sqdists(Xm, z0)
        else:
            s = ((X.double() - z0.to(X.device).double()[None, :]) ** 2).sum(dim=1)
        w = 1.0 / s.double().sqrt().clamp(min=eps)
        live = torch.isfinite(torch.diagonal(G)) & torch.isfinite(w)
        w = torch.where(live, w, torch.zeros_like(w))
        a = (w / w.sum()).to(G.dtype)
        iters -= 1
    a = gram_fixed_point(G, a, rule="weiszfeld", eps=eps, tol=tol, iters=iters)[0]
    if W is not None:
        a = W.T @ a.double()
    return combine_rows(X, a)


def mixed_geometric_median(
    X: torch.Tensor,
    mix: torch.Tensor,
    *,
    gram: Optional[torch.Tensor] = None,
    tol: float = 1e-6,
    max_iter: int = 256,
    eps: float = 1e-12,
    fixed_iters: Optional[int] = None,
) -> torch.Tensor:
    """The geometric median (solver="gram", mean init) of the mixed rows
    (mix @ X) / mix.sum(1), with no mixed matrix: Gram, solver, combine — the
    two passes over X of the unmixed rule. ``gram`` is X's Gram if the
    caller already has it (NNM builds its membership from it)."""
    return _geometric_median_gram(
        X, tol=tol, max_iter=max_iter, eps=eps, init="mean",
        fixed_iters=fixed_iters, init_z=None, mix=mix, G=gram,
    )


# -- a gossip round on one shared Gram (K23) ----------------------------------
#
# All node states are rows of one (N, d) matrix, so ONE Gram of it holds every
# node's neighbourhood sub-Gram. A round for all nodes is that Gram (one pass),
# weiszfeld_iter(G, groups=...) (one launch, N m^2 numbers) and
# mean_rows(theta, coeffs=A) with the (M, N) coefficient matrix (one pass):
# no (M, m, d) gather, no mixed matrix, no pass per Weiszfeld step.

# Neighbourhood cap of weiszfeld_iter(G, groups=) (GOSSIP_MAX_M in
# csrc/launchers.h); its node count and mean_rows(X, coeffs=A)'s M share
# GRAMFP_MAX_N.
GOSSIP_MAX_M = 32
# Caps of colsel(X, mode, f, groups=) (csrc/colsel_groups.hip, K24): rows of X
# and nodes, and rows per node. The K23 caps, so one table serves both.
COLSEL_GROUPS_MAX_N = GRAMFP_MAX_N
COLSEL_GROUPS_MAX_M = GOSSIP_MAX_M


def gossip_groups(rows, device=None) -> torch.Tensor:
    """The int32 (M, m) groups tensor of a list of per-node row lists, ragged
    ones padded with -1. Checked on the host, before any device copy: the
    entries of a list must be distinct and >= 0. The tensor carries the list
    lengths as ``valid_counts``, for callers that need them without reading
    the device copy back."""
    rows = [[int(j) for j in r] for r in rows]
    m = max((len(r) for r in rows), default=0)
    if m < 1:
        raise ValueError("every node needs at least one row")
    for r in rows:
        if not r or len(set(r)) != len(r) or min(r) < 0:
            raise ValueError("a node's rows must be distinct, >= 0 and not empty")
    padded = [r + [-1] * (m - len(r)) for r in rows]
    groups = torch.tensor(padded, dtype=torch.int32, device=device)
    groups.valid_counts = [len(r) for r in rows]
    return groups


def _gossip_fused(G: torch.Tensor, groups: torch.Tensor) -> bool:
    return (
        _gpu(G)
        and G.dtype == torch.float32
        and 1 <= G.shape[0] <= GRAMFP_MAX_N
        and 1 <= groups.shape[0] <= GRAMFP_MAX_N
        and 1 <= groups.shape[1] <= GOSSIP_MAX_M
    )


def gossip_coeffs(
    G: torch.Tensor,
    groups: torch.Tensor,
    nnm_f: Optional[int] = None,
    *,
    iters: int,
    eps: float = 1e-12,
    tol: float = 0.0,
):
    """(A, steps) of F.gossip_coeffs: one launch and no host sync for an f32
    device Gram of n <= GRAMFP_MAX_N rows, M <= GRAMFP_MAX_N nodes and
    neighbourhoods of m <= GOSSIP_MAX_M rows (A is f32, steps a device
    tensor), the f64 loop otherwise."""
    if nnm_f is not None and not 0 <= int(nnm_f) < groups.shape[1]:
        raise ValueError("need 0 <= nnm_f < m")
    if _gossip_fused(G, groups):
        grp = groups.to(device=G.device, dtype=torch.int32).contiguous()
        return tuple(_hip.require().weiszfeld_iter(
            G.contiguous(), groups=grp, nnm_f=-1 if nnm_f is None else int(nnm_f),
            eps=float(eps), tol=float(tol), iters=int(iters),
        ))
    return F.gossip_coeffs(G, groups, nnm_f, iters=iters, eps=eps, tol=tol)


def combine_rows_batched(X: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """A @ X in X's dtype for an (M, n) coefficient matrix: one pass over the
    rows of X that some row of A reads, f32 accumulation on the matrix pipe
    (combine_batched.hip), for n, M <= GRAMFP_MAX_N on the device; the f64
    product over the read rows elsewhere."""
    if _gramfp_fused(X) and not _row_list(X) and 1 <= A.shape[0] <= GRAMFP_MAX_N:
        A32 = A.to(device=X.device, dtype=torch.float32).contiguous()
        return _hip.require().mean_rows(X.contiguous(), coeffs=A32)
    A = A.to(X.device)
    keep = (A != 0).any(dim=0)
    return (A[:, keep].double() @ X[keep].double()).to(X.dtype)


def gossip_geometric_median(
    theta: torch.Tensor,
    groups: torch.Tensor,
    *,
    nnm_f: Optional[int] = None,
    fixed_iters: Optional[int] = None,
    tol: float = 1e-6,
    max_iter: int = 256,
    eps: float = 1e-12,
    centered: bool = False,
) -> torch.Tensor:
    """One gossip round of GeometricMedian(solver="gram", init="mean"), after
    NNM(nnm_f) if given, for every node at once: row i of the (M, d) result is
    the rule over the rows theta[groups[i]] (-1 pads). Gram, solver and combine
    are three device steps with no host sync (capture-safe with
    ``fixed_iters``); CPU tensors and shapes past the kernels' caps take the
    f64 route. ``centered`` solves on the centred Gram of theta: valid, the
    coefficients sum to 1 from the first step. Rows of theta that hold inf or
    NaN get coefficient 0 everywhere and are not read by the combine."""
    iters = int(fixed_iters) if fixed_iters is not None else int(max_iter)
    tol = 0.0 if fixed_iters is not None else float(tol)
    G = solver_gram(theta, centered)
    A, _ = gossip_coeffs(G, groups, nnm_f, iters=iters, eps=eps, tol=tol)
    return combine_rows_batched(theta, A)


def _centered_clipping_gram(X, *, c_tau, M, eps, init) -> torch.Tensor:
    if init not in ("mean", "zero"):
        raise ValueError(
            "solver='gram' needs init 'mean' or 'zero': from the median v "
            "keeps a component outside the span of the rows"
        )
    if _row_list(X) and not _gramfp_fused(X):
        X = torch.stack(list(X))
    G = solver_gram(X)
    a0 = _live_uniform(G) if init == "mean" else torch.zeros_like(G[0])
    a = gram_fixed_point(G, a0, rule="cc", c_tau=c_tau, eps=eps, iters=M)[0]
    return combine_rows(X, a)


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
    solver: str = "iterative",
    centered: bool = False,
) -> torch.Tensor:
    """Weiszfeld fixed point. ``fixed_iters`` runs exactly that many
    iterations with NO convergence polls — fully async (no host sync), so
    per-node streams overlap and the whole call is hipGraph-capture-safe
    (the polls serialized config-4 gossip in round 1). ``init_z`` warm-
    starts from a caller-provided center (e.g. the previous gossip
    round's output — the fixed point barely moves between rounds, so a
    handful of iterations replaces a cold median init + long descent).
    ``solver="gram"`` runs the loop on the Gram instead (K20, above);
    with ``init="mean"`` it may run on the centred Gram (``centered=True``,
    K22). Any other use of ``centered`` is a ValueError."""
    _check_solver(solver)
    if centered and solver != "gram":
        raise ValueError("centered=True needs solver='gram'")
    if solver == "gram":
        return _geometric_median_gram(
            X, tol=tol, max_iter=max_iter, eps=eps, init=init,
            fixed_iters=fixed_iters, init_z=init_z, centered=centered,
        )
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
    solver: str = "iterative",
    centered: bool = False,
) -> torch.Tensor:
    _check_solver(solver)
    if centered:
        # a clipping step's coefficients do not sum to 1
        raise ValueError("centered clipping does not run on the centred Gram")
    if solver == "gram":
        return _centered_clipping_gram(X, c_tau=c_tau, M=M, eps=eps, init=init)
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


def nnm(X: torch.Tensor, f: int, centered: bool = False) -> torch.Tensor:
    if _gpu(X) or centered:
        idx = nearest_rows_from_gram(gram(X, center=centered), X.shape[0] - f)
        return group_mean_rows(X, idx)
    return F.nnm(X, f)


# -- mixing pre-aggregator + coordinate-wise rule (K18) ----------------------

# NNM and Bucketing are row maps Y = W X, W an (m, n) 0/1 membership matrix
# over its row counts. ``colsel(X, mode, f, mix=)`` (colsel_mix.hip) takes
# the median / trimmed mean of W X column by column with the matrix pipe and
# never writes the (m, d) matrix Y that the composition stores (rounded to
# bf16) and reads back.
MIXED_COLSEL_MAX = 64

# Column count from which the fused kernel is the default route. Measured on
# MI355X at n = 33 and n = 64, d = 64K ... 16M, NNM -> trimmed mean, the mix
# + select step alone with the membership given
# (benchmarks/RESULTS_MI355X_mixed.md, "d sweep"): the fused call took
# 0.06-0.52 of the composition's time at EVERY size, 64K included (11.9 vs
# 23.1 us at 33 x 65,536, 15.6 vs 36.7 us at 64 x 65,536), with a run-to-run
# spread under 1 % on either side. 65,536 is the smallest size measured;
# below it the composition stays.
MIXED_COLSEL_FUSED_MIN_D = 65_536

# BYZPY_MIXED_COLSEL=split forces the composition, =fused the kernel
# wherever it applies (A/B runs)
_MIXED_COLSEL_ENV = "BYZPY_MIXED_COLSEL"


def mixed_colsel_fused_ok(X: torch.Tensor) -> bool:
    """Whether a mixed statistic of X's rows takes the fused kernel: bf16 on
    the device, n <= 64 (so m <= 64 for NNM and Bucketing), d past the
    routing threshold."""
    n, d = X.shape
    if not (_gpu(X) and X.dtype == torch.bfloat16 and 1 <= n <= MIXED_COLSEL_MAX and d >= 1):
        return False
    env = os.environ.get(_MIXED_COLSEL_ENV, "")
    if env == "split":
        return False
    if env == "fused":
        return True
    return d >= MIXED_COLSEL_FUSED_MIN_D


def _mixed_colsel(X: torch.Tensor, mix: torch.Tensor, mode: int, f: int):
    """Median / trimmed mean over the rows of Y = (mix @ X) / mix.sum(1):
    the fused kernel where mixed_colsel_fused_ok, else Y in f32, rounded to
    X's dtype as the pre-aggregators round theirs, and the plain rule."""
    if mixed_colsel_fused_ok(X) and mix.shape[0] <= MIXED_COLSEL_MAX:
        mix8 = mix.to(device=X.device, dtype=torch.uint8).contiguous()
        return _hip.require().colsel(X.contiguous(), mode, int(f), mix=mix8)
    W = mix.to(device=X.device, dtype=torch.float32)
    Y = ((W @ X.float()) / W.sum(dim=1, keepdim=True)).to(X.dtype)
    return median(Y) if mode == _COLSEL_MEDIAN else trimmed_mean(Y, f)


def mixed_median(X: torch.Tensor, mix: torch.Tensor) -> torch.Tensor:
    return _mixed_colsel(X, mix, _COLSEL_MEDIAN, 0)


def mixed_trimmed_mean(X: torch.Tensor, mix: torch.Tensor, f: int) -> torch.Tensor:
    return _mixed_colsel(X, mix, _COLSEL_TRIMMED, f)


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


def mda_subset_device(D2: torch.Tensor, f: int) -> Optional[torch.Tensor]:
    """The lexicographically smallest minimum-diameter (n - f)-subset of the
    device f32 (n, n) D2 as an int32 index tensor, found by the two-pass
    branch-and-bound of subsets.hip: no host D2 copy, one host sync. None
    where the search does not apply (n > 64, or n - f outside 2 .. n - 1) or
    found nothing (a NaN in D2): the caller falls back to the host search."""
    n = D2.shape[0]
    m = n - f
    if not (n <= 64 and 2 <= m < n):
        return None
    # Seed the shared bound with a cheap anchor-greedy upper bound (diameter
    # of each row's m nearest rows) so pass 1 prunes like the host B&B
    # instead of starting from +inf.
    idxn = torch.topk(D2, k=m, dim=1, largest=False).indices
    sub = D2[idxn[:, :, None], idxn[:, None, :]]  # (n, m, m)
    ub = sub.amax(dim=(1, 2)).min()
    found, subsets = _hip.require().mda_select(D2, int(f), ub)
    if not bool(found.any()):
        return None
    # the first found prefix holds the winner: a cumsum one-hot mask
    first = ((found.cumsum(0) == 1) & (found == 1)).to(subsets.dtype)
    return (subsets * first[:, None]).sum(dim=0).to(torch.int32)


def minimum_diameter_averaging(X: torch.Tensor, f: int) -> torch.Tensor:
    if _gpu(X):
        D2 = pairwise_sq_dists(X)
        subset_t = mda_subset_device(D2, f)
        if subset_t is not None:
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


# -- CAF on the Gram (K21) ------------------------------------------------------
#
# ``solver="gram"`` of caf. Every quantity of the filter loop lives in the
# span of the centred rows (F.caf_gram), so the loop runs on the (n, n) Gram
# in one launch (caf_gram_kernel, csrc/gramfp.hip) between the two passes over
# X of K20: the MFMA Gram and ``mean_rows(X, coeffs=)``. No host sync, no
# d-long random vectors, device row lists read in place. Opt-in: the power
# iteration starts in the row span (n Gaussians per round, not d), so it is
# the same filter on another random stream, and the projections come from an
# f32 Gram.

_CAF_GRAM_SEEDS: dict = {}
_CAF_GRAM_SEEDS_MAX = 8  # FIFO cap: an entry is at most 64 KB


def _caf_gram_device_seeds(n: int, device) -> torch.Tensor:
    key = (n, device.type, device.index)
    seeds = _CAF_GRAM_SEEDS.get(key)
    if seeds is None:
        if len(_CAF_GRAM_SEEDS) >= _CAF_GRAM_SEEDS_MAX:
            _CAF_GRAM_SEEDS.pop(next(iter(_CAF_GRAM_SEEDS)))
        seeds = F.caf_gram_seeds(n).to(device)
        _CAF_GRAM_SEEDS[key] = seeds
    return seeds


def caf_gram(G: torch.Tensor, f: int, *, power_iters: int = 3):
    """(a, lam, rounds) of F.caf_gram on the seeds F.caf_gram_seeds(n): one
    launch and no host sync for an f32 device Gram of n <= GRAMFP_MAX_N rows
    (lam and rounds stay device scalars), the f64 torch loop otherwise."""
    n = G.shape[0]
    if n - 2 * f <= 0:
        raise ValueError(f"need n - 2f > 0, got n={n}, f={f}")
    if _gpu(G) and G.dtype == torch.float32 and 1 <= n <= GRAMFP_MAX_N:
        return tuple(_hip.require().caf_matvec(
            G.contiguous(), _caf_gram_device_seeds(n, G.device),
            f=int(f), power_iters=int(power_iters),
        ))
    return F.caf_gram(G, f, F.caf_gram_seeds(n), power_iters=power_iters)


def _caf_on_gram(X, f: int, power_iters: int) -> torch.Tensor:
    if _row_list(X) and not _gramfp_fused(X):
        X = torch.stack(list(X))
    a = caf_gram(solver_gram(X), f, power_iters=power_iters)[0]
    return combine_rows(X, a)


def caf(
    X: torch.Tensor, f: int, *, power_iters: int = 3, solver: str = "iterative",
    centered: bool = False,
) -> torch.Tensor:
    """Covariance-agnostic filter on fused K9 kernels (reference
    caf.py:133-184): caf_matvec computes s = (X - mu) @ v, caf_colsum
    computes weighted centered column sums — neither materializes the
    (n, d) f32 diffs matrix and both replace rocblas gemvt (~260 GB/s on
    this skinny shape). Same algorithm and seeded-rng contract as the
    functional oracle. Steady-state shapes run the hipGraph block path
    (_CafGraphBlock); others fall back to the eager loop below.
    ``solver="gram"`` runs the loop on the Gram instead (K21, above)."""
    import math
    import os

    _check_solver(solver)
    if centered:
        # the filter re-centres by its own weighted mean every round
        raise ValueError("CAF does not run on the centred Gram")
    if solver == "gram":
        return _caf_on_gram(X, int(f), int(power_iters))
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
