"""Pure-torch reference implementations of every robust-aggregation op.

Every function operates on a 2-D ``(n, d)`` torch tensor (one gradient per
row) and returns either a ``(d,)`` aggregate or an ``(n', d)`` matrix.
These run on any device and are the numerical oracle the HIP kernels are
tested against (SURVEY.md §4 pattern 2). Device dispatch to the gfx950
kernels lives in byzpy_amd/hip/dispatch.py — NOT here.

Algorithm parity notes (cites into /root/reference):
- median: true per-coordinate median (mean of the two middles for even n).
  The reference's chunked path returned the lower middle
  (aggregators/coordinate_wise/median.py:160-171) while its direct path did
  not — we deliberately make both paths the true median.
- krum: Blanchard et al. 2017 scoring (krum.py:183-194).
- geometric_median: Weiszfeld fixed point (geometric_median.py:69-104).
- centered_clipping: Karimireddy et al. 2021 (center_clipping.py:107-156).
- mda: exact (n-f)-subset min-diameter search (minimum_diameter_average.py).
- smea: min max-eigenvalue subset (smea.py:63-107).
- caf: covariance-agnostic filter w/ seeded power iteration (caf.py:133-184).
"""
from __future__ import annotations

import itertools
import math
from typing import List, Optional, Sequence, Tuple

import torch

# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------


def pairwise_sq_dists(X: torch.Tensor) -> torch.Tensor:
    """Full n x n matrix of squared euclidean distances via the Gram trick
    ``||a||^2 + ||b||^2 - 2 a.b`` with f32 accumulation."""
    Xf = X.float()
    norms = (Xf * Xf).sum(dim=1)
    G = Xf @ Xf.T
    D2 = norms[:, None] + norms[None, :] - 2.0 * G
    return D2.clamp_(min=0.0)


# ---------------------------------------------------------------------------
# coordinate-wise aggregators
# ---------------------------------------------------------------------------


def median(X: torch.Tensor) -> torch.Tensor:
    """True per-coordinate median; for even n the mean of the two middles."""
    n = X.shape[0]
    s, _ = torch.sort(X.float(), dim=0)
    if n % 2 == 1:
        out = s[n // 2]
    else:
        out = (s[n // 2 - 1] + s[n // 2]) * 0.5
    return out.to(X.dtype)


def trimmed_mean(X: torch.Tensor, f: int) -> torch.Tensor:
    """Sort each coordinate, drop f from each end, mean the middle n-2f
    (Yin et al. 2018; reference trimmed_mean.py:80-115)."""
    n = X.shape[0]
    if 2 * f >= n:
        raise ValueError(f"need n > 2f, got n={n}, f={f}")
    s, _ = torch.sort(X.float(), dim=0)
    out = s[f : n - f].mean(dim=0)
    return out.to(X.dtype)


def mean_of_medians(X: torch.Tensor, f: int) -> torch.Tensor:
    """MeaMed: per coordinate keep the n-f values closest to the median,
    mean them (reference mean_of_medians.py:53-81)."""
    n = X.shape[0]
    if f < 0 or f >= n:
        raise ValueError(f"need 0 <= f < n, got n={n}, f={f}")
    Xf = X.float()
    med = median(Xf)
    dev = (Xf - med[None, :]).abs()
    # indices of the n-f smallest deviations per column
    idx = torch.topk(dev, k=n - f, dim=0, largest=False).indices
    kept = torch.gather(Xf, 0, idx)
    return kept.mean(dim=0).to(X.dtype)


# ---------------------------------------------------------------------------
# geometric aggregators
# ---------------------------------------------------------------------------


def multi_krum_scores(X: torch.Tensor, f: int) -> torch.Tensor:
    """score_i = sum of the n-f-1 smallest squared distances from i to the
    others (self-distance 0 excluded)."""
    n = X.shape[0]
    k = n - f - 1
    if k < 1:
        raise ValueError(f"need n - f - 1 >= 1, got n={n}, f={f}")
    D2 = pairwise_sq_dists(X)
    D2 = D2 + torch.diag(torch.full((n,), float("inf"), device=X.device))
    smallest = torch.topk(D2, k=k, dim=1, largest=False).values
    return smallest.sum(dim=1)


def multi_krum(X: torch.Tensor, f: int, q: int) -> torch.Tensor:
    """Mean of the q vectors with the best (lowest) Krum scores."""
    n = X.shape[0]
    if q < 1 or q > n:
        raise ValueError(f"need 1 <= q <= n, got q={q}, n={n}")
    scores = multi_krum_scores(X, f)
    winners = torch.topk(scores, k=q, largest=False).indices
    return X.float()[winners].mean(dim=0).to(X.dtype)


def krum(X: torch.Tensor, f: int) -> torch.Tensor:
    """The single vector with the best Krum score (= MultiKrum q=1,
    returning the winner itself, reference krum.py:346-368)."""
    scores = multi_krum_scores(X, f)
    return X[int(torch.argmin(scores))].clone()


def bulyan_select_from_gram(G: torch.Tensor, f: int) -> torch.Tensor:
    """Bulyan's selection phase (El Mhamdi et al. 2018) on an (n, n) Gram:
    theta = n - 2f picks; each pick is the surviving row with the smallest
    Krum score among the survivors (sum of its r - f - 1 smallest squared
    distances to other survivors, r = survivors left; ties to the smallest
    index), which then leaves the pool. Returns the picks in order (int64).

    Written row by row in f64 straight from the definition — this is the
    oracle, deliberately not the vectorised text of hip/dispatch.py."""
    n = G.shape[0]
    if f < 0 or n < 4 * f + 3:
        raise ValueError(f"Bulyan needs n >= 4f + 3, got n={n}, f={f}")
    if f == 0:
        return torch.arange(n, dtype=torch.int64)
    Gd = G.detach().double().cpu()
    inf = float("inf")
    D2 = [[inf] * n for _ in range(n)]
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            v = float(Gd[i, i] + Gd[j, j] - 2.0 * Gd[i, j])
            D2[i][j] = max(v, 0.0) if math.isfinite(v) else inf
    alive = list(range(n))
    picks: List[int] = []
    for _ in range(n - 2 * f):
        k = len(alive) - f - 1
        best_i, best_s = -1, inf
        for i in alive:
            nearest = sorted(D2[i][j] for j in alive if j != i)[:k]
            s = math.fsum(nearest) if math.isfinite(nearest[-1]) else inf
            if best_i < 0 or s < best_s:
                best_i, best_s = i, s
        picks.append(best_i)
        alive.remove(best_i)
    return torch.tensor(picks, dtype=torch.int64)


def bulyan_select(X: torch.Tensor, f: int) -> torch.Tensor:
    """Bulyan's selected rows, in pick order, from the f32-accumulated Gram
    of X (see bulyan_select_from_gram)."""
    Xf = X.float()
    return bulyan_select_from_gram(Xf @ Xf.T, f)


def bulyan(X: torch.Tensor, f: int) -> torch.Tensor:
    """Bulyan: theta = n - 2f rows chosen by iterated Krum, then per
    coordinate the mean of the beta = theta - 2f selected values closest to
    their median."""
    sel = bulyan_select(X, f).to(X.device)
    return mean_of_medians(X[sel], 2 * f)


# DnC (Shejwalkar & Houmansadr, NDSS 2021, Algorithm 2). A sampled entry is
# "finite" up to this magnitude; past it (and for inf / NaN) its row is bad:
# the square of a larger value does not fit the f32 Gram of the device path.
DNC_MAX_ABS = float(2**48)


def dnc_keep(n: int, f: int, c: float = 1.0) -> int:
    """Rows each DnC iteration keeps: n - floor(c f)."""
    if f < 0 or c < 0:
        raise ValueError(f"DnC needs f >= 0 and c >= 0, got f={f}, c={c}")
    keep = n - int(math.floor(c * f))
    if keep < 1:
        raise ValueError(
            f"DnC needs n - floor(c f) >= 1, got n={n}, f={f}, c={c}"
        )
    return keep


def _dnc_kept(S: torch.Tensor, keep: int) -> torch.Tensor:
    """One DnC iteration on the (n, b) sample S: bool (n,) of kept rows."""
    n = S.shape[0]
    Sd = S.detach().float().double().cpu()
    ok = torch.isfinite(Sd) & (Sd.abs() <= DNC_MAX_ABS)
    Sz = torch.where(ok, Sd, torch.zeros_like(Sd))
    cnt = ok.sum(dim=0)
    mu = Sz.sum(dim=0) / cnt.clamp_min(1)
    C = torch.where(ok, Sd - mu[None, :], torch.zeros_like(Sd))
    bad = ~ok.all(dim=1)
    lam, U = torch.linalg.eigh(C @ C.T)
    top, u = float(lam[-1]), U[:, -1]
    # lambda u_i^2 is the squared projection of row i on the top right
    # singular vector r = C^T u / sqrt(lambda). Projecting row by row, each
    # row summed alone, gives identical rows identical scores (eigh's u_i
    # agree only to rounding), so the index tie-break below is exact.
    if top > 0.0:
        r = (C * u[:, None]).sum(dim=0)
        score = (C * r[None, :]).sum(dim=1) ** 2 / top
    else:
        score = torch.zeros(n, dtype=torch.float64)
    score = torch.where(bad, torch.full_like(score, float("inf")), score)
    order = sorted(range(n), key=lambda i: (float(score[i]), i))
    kept = torch.zeros(n, dtype=torch.bool)
    kept[order[:keep]] = True
    return kept & ~bad


def dnc_select(
    X: torch.Tensor, f: int, coords: torch.Tensor, c: float = 1.0
) -> torch.Tensor:
    """DnC's good set, bool (n,): per row t of ``coords`` (int (niters, b)
    column indices, duplicates allowed) the n - floor(c f) rows with the
    lowest outlier score on the sample X[:, coords[t]] — the squared
    projection of the centred row on the sample's top right singular
    vector — and the intersection over t. Columns are centred by the mean of
    their finite entries, a non-finite entry counts 0, and a row with one in
    the sample is never kept. f64 throughout; this is the oracle."""
    keep = dnc_keep(X.shape[0], f, c)
    good = torch.ones(X.shape[0], dtype=torch.bool)
    for row in coords.detach().cpu().long():
        good &= _dnc_kept(X[:, row.to(X.device)], keep)
    return good


def dnc(
    X: torch.Tensor, f: int, coords: torch.Tensor, c: float = 1.0
) -> torch.Tensor:
    """DnC: the mean (f32) of the rows of dnc_select; the zero vector when
    no row survives every iteration (skip the round). Rows outside the good
    set are not read, so an inf in one never reaches the result."""
    good = dnc_select(X, f, coords, c).to(X.device)
    if not bool(good.any()):
        return torch.zeros_like(X[0])
    return X[good].float().mean(dim=0).to(X.dtype)


# AFA, Adaptive Federated Averaging (Muñoz-González, Co, Lupu 2019,
# Algorithm 1) without its cross-round state: the reputation that the paper
# carries from round to round enters as ``weights`` (aggregators.AFAReputation
# keeps it).


def _afa_weights(weights, n: int) -> torch.Tensor:
    """The (n,) f64 CPU weight vector after the argument checks."""
    if weights is None:
        return torch.ones(n, dtype=torch.float64)
    w = torch.as_tensor(weights).detach().double().cpu().flatten()
    if w.numel() != n:
        raise ValueError(f"weights: expected {n} entries, got {w.numel()}")
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
        raise ValueError("weights must be finite and >= 0")
    return w


def _afa_check(xi: float, delta_xi: float) -> None:
    if not (xi >= 0 and math.isfinite(xi)):
        raise ValueError(f"AFA needs a finite xi >= 0, got {xi}")
    if not (delta_xi >= 0 and math.isfinite(delta_xi)):
        raise ValueError(f"AFA needs a finite delta_xi >= 0, got {delta_xi}")


def afa_trace(
    X: torch.Tensor, weights=None, xi: float = 2.0, delta_xi: float = 0.5
) -> Tuple[torch.Tensor, List[dict]]:
    """AFA's selection with its working: (alive bool (n,), one record per
    loop pass). A record holds ``alive`` (the set the pass started from),
    ``s`` (f64 (n,) cosines, 0 outside alive), ``mean``, ``med``, ``sd``,
    ``lower`` (the branch taken), ``threshold`` and ``removed`` (bool (n,)).
    The last record of a run that ends by finding nothing to remove has an
    all-false ``removed``. Everything is f64 on the CPU, from the explicit
    weighted mean vector and explicit norms."""
    _afa_check(xi, delta_xi)
    n = X.shape[0]
    w = _afa_weights(weights, n)
    Xd = X.detach().float().double().cpu()
    alive = torch.isfinite(Xd).all(dim=1) & (w > 0)
    norms = torch.zeros(n, dtype=torch.float64)
    norms[alive] = Xd[alive].pow(2).sum(dim=1).sqrt()
    xi = float(xi)
    trace: List[dict] = []
    for _ in range(n):
        if not bool(alive.any()):
            break
        rows = torch.nonzero(alive).flatten()
        wa = w[rows]
        g = (wa[:, None] * Xd[rows]).sum(dim=0) / wa.sum()
        gn = float(g.pow(2).sum().sqrt())
        s = torch.zeros(n, dtype=torch.float64)
        for i in rows.tolist():
            if gn > 0.0 and float(norms[i]) > 0.0:
                s[i] = float((g * Xd[i]).sum()) / (gn * float(norms[i]))
        sa = s[rows]
        m = int(sa.numel())
        mean = float(sa.sum()) / m
        srt = torch.sort(sa).values
        med = 0.5 * (float(srt[(m - 1) // 2]) + float(srt[m // 2]))
        sd = math.sqrt(float(((sa - mean) ** 2).sum()) / m)
        lower = mean < med
        threshold = med - xi * sd if lower else med + xi * sd
        removed = alive & ((s < threshold) if lower else (s > threshold))
        trace.append(dict(
            alive=alive.clone(), s=s, mean=mean, med=med, sd=sd, lower=lower,
            threshold=threshold, removed=removed,
        ))
        if not bool(removed.any()):
            break
        alive = alive & ~removed
        xi += float(delta_xi)
    return alive, trace


def afa_select(
    X: torch.Tensor, weights=None, xi: float = 2.0, delta_xi: float = 0.5
) -> torch.Tensor:
    """AFA's good set, bool (n,). Start from the finite rows of positive
    weight; each pass takes the weighted mean g of the rows still alive,
    their cosines s_i to g (0 where a norm is 0), and the mean, true median
    and population sd of s; if mean < median it drops the rows with
    s_i < med - xi sd, else those with s_i > med + xi sd (strict, so sd = 0
    drops nothing); xi grows by delta_xi after every pass that dropped a
    row, and the first pass that drops none ends the loop. This is the
    oracle."""
    return afa_trace(X, weights, xi, delta_xi)[0]


def afa(
    X: torch.Tensor, weights=None, xi: float = 2.0, delta_xi: float = 0.5
) -> torch.Tensor:
    """AFA: the weighted mean of the rows of afa_select, the zero vector when
    there is none (skip the round). Rows outside the good set are not read."""
    good = afa_select(X, weights, xi, delta_xi)
    if not bool(good.any()):
        return torch.zeros_like(X[0])
    w = _afa_weights(weights, X.shape[0])[good]
    rows = X[good.to(X.device)].detach().float().double().cpu()
    out = (w[:, None] * rows).sum(dim=0) / w.sum()
    return out.to(dtype=X.dtype, device=X.device)


def geometric_median(
    X: torch.Tensor,
    *,
    tol: float = 1e-6,
    max_iter: int = 256,
    eps: float = 1e-12,
    init: str = "median",
) -> torch.Tensor:
    """Weiszfeld fixed point: z <- sum(x_i/d_i) / sum(1/d_i), d_i clamped
    >= eps; stops when ||dz|| <= tol."""
    if init not in ("median", "mean"):
        raise ValueError("init must be 'median' or 'mean'")
    Xf = X.float()
    z = median(Xf) if init == "median" else Xf.mean(dim=0)
    z = z.float()
    for _ in range(max_iter):
        d = (Xf - z[None, :]).norm(dim=1).clamp_(min=eps)
        w = 1.0 / d
        z_new = (w[:, None] * Xf).sum(dim=0) / w.sum()
        shift = (z_new - z).norm()
        z = z_new
        if shift <= tol:
            break
    return z.to(X.dtype)


def mda_subset(D2: torch.Tensor, f: int) -> Tuple[int, ...]:
    """Exact minimum-diameter (n-f)-subset search on a squared-distance
    matrix. Branch-and-bound DFS with prefix-max pruning — runs on the host
    over the tiny n x n matrix (the D2 itself is computed on device)."""
    n = D2.shape[0]
    m = n - f
    if m < 1:
        raise ValueError(f"need n - f >= 1, got n={n}, f={f}")
    from byzpy_amd import hip as _hip

    ext = _hip.extension()
    if ext is not None:  # native C++ branch-and-bound (host)
        idx = ext.mda_search(D2.detach().float().cpu(), int(f))
        return tuple(int(i) for i in idx)
    D = D2.detach().cpu().double().numpy()
    best_diam = math.inf
    best: Tuple[int, ...] = tuple(range(m))

    # order candidates so tight subsets are found early (better pruning)
    order = list(range(n))

    def dfs(start: int, chosen: List[int], diam: float) -> None:
        nonlocal best_diam, best
        if diam >= best_diam:
            return
        if len(chosen) == m:
            best_diam = diam
            best = tuple(sorted(chosen))
            return
        # not enough remaining to complete the subset
        remaining = n - start
        if remaining < m - len(chosen):
            return
        for j in range(start, n):
            dj = diam
            ok = True
            for c in chosen:
                dc = D[c][order[j]]
                if dc >= best_diam:
                    ok = False
                    break
                if dc > dj:
                    dj = dc
            if ok:
                chosen.append(order[j])
                dfs(j + 1, chosen, dj)
                chosen.pop()

    dfs(0, [], 0.0)

    # canonicalize to the lexicographically smallest optimal subset (ties
    # are generic: every subset containing the binding edge can tie)
    bound = best_diam
    lex: List[int] = []

    def dfs2(start: int) -> bool:
        if len(lex) == m:
            return True
        need = m - len(lex)
        for j in range(start, n - need + 1):
            if all(D[c][j] <= bound for c in lex):
                lex.append(j)
                if dfs2(j + 1):
                    return True
                lex.pop()
        return False

    if dfs2(0):
        return tuple(lex)
    return best


def minimum_diameter_averaging(X: torch.Tensor, f: int) -> torch.Tensor:
    D2 = pairwise_sq_dists(X)
    subset = mda_subset(D2, f)
    idx = torch.tensor(subset, device=X.device, dtype=torch.long)
    return X.float()[idx].mean(dim=0).to(X.dtype)


def monna(X: torch.Tensor, f: int, reference_index: int = 0) -> torch.Tensor:
    """Mean of the n-f nearest neighbours of a trusted reference row
    (reference-first tiebreak, monna.py:142-145)."""
    n = X.shape[0]
    k = n - f
    if k < 1 or reference_index < 0 or reference_index >= n:
        raise ValueError("bad monna parameters")
    Xf = X.float()
    ref = Xf[reference_index]
    d2 = ((Xf - ref[None, :]) ** 2).sum(dim=1)
    # reference row first regardless of float noise in its self-distance
    d2 = d2.clone()
    d2[reference_index] = -1.0
    idx = torch.argsort(d2, stable=True)[:k]
    return Xf[idx].mean(dim=0).to(X.dtype)


def smea(X: torch.Tensor, f: int) -> torch.Tensor:
    """Among all (n-f)-subsets pick the one whose sample covariance has the
    smallest max eigenvalue; return its mean. Eigenvalues come from the
    centered Gram H G H (m x m), a device-batched eigvalsh."""
    n = X.shape[0]
    m = n - f
    if m < 1:
        raise ValueError(f"need n - f >= 1, got n={n}, f={f}")
    Xf = X.float()
    G = Xf @ Xf.T
    # enumerate subsets in bounded blocks: materializing all C(n, m)
    # (m, m) Grams at once OOMs for larger n (the search stays exact and
    # exponential-time by definition — same as the reference smea.py:63-107)
    BLOCK = 1 << 16
    best_ev = math.inf
    best_rows: Optional[torch.Tensor] = None
    it = itertools.combinations(range(n), m)
    while True:
        combos = list(itertools.islice(it, BLOCK))
        if not combos:
            break
        idx = torch.tensor(combos, device=X.device, dtype=torch.long)  # (B, m)
        # batched centered Gram: HGH with H = I - 1/m
        sub = G[idx[:, :, None], idx[:, None, :]]  # (B, m, m)
        row_mean = sub.mean(dim=2, keepdim=True)
        col_mean = sub.mean(dim=1, keepdim=True)
        all_mean = sub.mean(dim=(1, 2), keepdim=True)
        centered = sub - row_mean - col_mean + all_mean
        ev = torch.linalg.eigvalsh(
            centered.cpu() if X.device.type == "cpu" else centered
        )
        max_ev = ev[..., -1]
        b = int(torch.argmin(max_ev))
        v = float(max_ev[b])
        # ties resolve to the lexicographically-smallest subset (blocks are
        # generated in lexicographic order, so strict < suffices)
        if v < best_ev:
            best_ev = v
            best_rows = idx[b]
    assert best_rows is not None
    return Xf[best_rows].mean(dim=0).to(X.dtype)


# ---------------------------------------------------------------------------
# norm-wise aggregators
# ---------------------------------------------------------------------------


def centered_clipping(
    X: torch.Tensor,
    *,
    c_tau: float,
    M: int = 10,
    eps: float = 1e-12,
    init: str = "mean",
) -> torch.Tensor:
    """v <- v + (1/n) sum_i clip(x_i - v, c_tau) for M iterations."""
    Xf = X.float()
    n = Xf.shape[0]
    if init == "mean":
        v = Xf.mean(dim=0)
    elif init == "median":
        v = median(Xf).float()
    elif init == "zero":
        v = torch.zeros_like(Xf[0])
    else:
        raise ValueError("init must be one of {'mean','median','zero'}")
    for _ in range(M):
        diff = Xf - v[None, :]
        norms = diff.norm(dim=1).clamp_(min=eps)
        alpha = torch.clamp(c_tau / norms, max=1.0)
        v = v + (alpha[:, None] * diff).sum(dim=0) / n
    return v.to(X.dtype)


def cge(X: torch.Tensor, f: int) -> torch.Tensor:
    """Comparative gradient elimination: mean of the n-f smallest-L2-norm
    rows."""
    n = X.shape[0]
    k = n - f
    if k < 1:
        raise ValueError(f"need n - f >= 1, got n={n}, f={f}")
    Xf = X.float()
    norms = (Xf * Xf).sum(dim=1)
    idx = torch.argsort(norms, stable=True)[:k]
    return Xf[idx].mean(dim=0).to(X.dtype)


def caf(X: torch.Tensor, f: int, *, power_iters: int = 3) -> torch.Tensor:
    """Covariance-agnostic filter: iteratively downweight along the dominant
    eigvec of the weighted covariance until the weight mass <= n - 2f;
    return the best-lambda weighted mean (reference caf.py:133-184, seeded
    rng(0) power iteration)."""
    Xf = X.float()
    n = Xf.shape[0]
    if n - 2 * f <= 0:
        raise ValueError(f"need n - 2f > 0, got n={n}, f={f}")
    d = Xf.shape[1]
    w = torch.ones(n, device=Xf.device)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(0)
    best_lambda = torch.full((), math.inf, device=Xf.device)
    best_mu = Xf.mean(dim=0)
    target = float(n - 2 * f)
    # power-iteration seeds pre-generated per block (one CPU randn + one
    # H2D per block, capped ~512 MB for huge d; falls back to per-round)
    block_rows = max(1, min(4, (1 << 27) // max(d, 1)))
    seeds: torch.Tensor = torch.empty(0)
    for r in range(n):  # at most n rounds of downweighting
        if r % block_rows == 0:
            rows = min(block_rows, n - r)
            seeds = torch.randn(rows, d, generator=gen).to(Xf.device)
        wsum = w.sum()
        mu = (w[:, None] * Xf).sum(dim=0) / wsum
        diffs = Xf - mu[None, :]
        # dominant eigenpair of (1/wsum) * diffs^T W diffs via power iteration
        # (seeded CPU rng is part of the determinism contract)
        v = seeds[r % block_rows]
        v = v / v.norm().clamp_min(1e-20)
        lam = torch.zeros((), device=Xf.device)
        for _ in range(max(1, power_iters)):
            s = diffs @ v  # (n,)
            t = (w * s)[None, :] @ diffs  # (1, d)
            t = t[0] / wsum
            lam = t.norm()
            v = t / lam.clamp_min(1e-20)
        # device-side best tracking (no extra host sync)
        better = lam < best_lambda
        best_lambda = torch.where(better, lam, best_lambda)
        best_mu = torch.where(better, mu, best_mu)
        # downweight along v proportionally to projection^2
        proj = (diffs @ v) ** 2
        pmax = proj.max().clamp_min(1e-20)
        w_next = (w * (1.0 - proj / pmax)).clamp_min(0.0)
        # one host sync per round for the two break conditions (A/B'd:
        # batching the check 4 rounds deep ran inert full rounds past the
        # break and LOST ~1 ms at 64x65536)
        wsum_f, wnext_f = torch.stack([wsum, w_next.sum()]).tolist()
        if wsum_f <= target or wnext_f <= 0:
            break
        w = w_next
    return best_mu.to(X.dtype)


# ---------------------------------------------------------------------------
# pre-aggregators (list -> list semantics; matrix in, matrix out here)
# ---------------------------------------------------------------------------


def clip_rows(X: torch.Tensor, threshold: float) -> torch.Tensor:
    """Scale each row to have L2 norm at most ``threshold``."""
    Xf = X.float()
    norms = Xf.norm(dim=1).clamp_min(1e-20)
    scale = torch.clamp(threshold / norms, max=1.0)
    return (Xf * scale[:, None]).to(X.dtype)


def arc_clip(X: torch.Tensor, f: int) -> torch.Tensor:
    """Adaptive robust clipping: clip the k = floor(2f/n * (n-f)) largest-norm
    rows to the largest remaining (k+1-th largest) norm (arc.py:36-61)."""
    n = X.shape[0]
    k = int(2 * f / n * (n - f))
    if k <= 0:
        return X.clone()
    Xf = X.float()
    norms = Xf.norm(dim=1)
    order = torch.argsort(norms, descending=True)
    threshold = norms[order[k]]  # largest norm NOT clipped
    scale = torch.clamp(threshold / norms.clamp_min(1e-20), max=1.0)
    return (Xf * scale[:, None]).to(X.dtype)


def bucketing(
    X: torch.Tensor, bucket_size: int, perm: Optional[Sequence[int]] = None
) -> torch.Tensor:
    """Random permutation -> consecutive buckets of ``bucket_size`` ->
    per-bucket mean. ``perm`` injectable for determinism (bucketing.py:93-94)."""
    n = X.shape[0]
    if perm is None:
        perm_t = torch.randperm(n, device=X.device)
    else:
        perm_t = torch.as_tensor(list(perm), device=X.device, dtype=torch.long)
    Xp = X.float()[perm_t]
    nb = (n + bucket_size - 1) // bucket_size
    out = torch.empty((nb, X.shape[1]), device=X.device, dtype=torch.float32)
    for b in range(nb):
        out[b] = Xp[b * bucket_size : min(n, (b + 1) * bucket_size)].mean(dim=0)
    return out.to(X.dtype)


def nnm(X: torch.Tensor, f: int) -> torch.Tensor:
    """Nearest-neighbor mixing: replace x_i by the mean of its n-f nearest
    neighbours (including itself) (nnm.py:82-97)."""
    n = X.shape[0]
    k = n - f
    if k < 1:
        raise ValueError(f"need n - f >= 1, got n={n}, f={f}")
    D2 = pairwise_sq_dists(X)
    idx = torch.topk(D2, k=k, dim=1, largest=False).indices  # (n, k)
    Xf = X.float()
    # mixing as a 0/1-mask matmul (one GEMM) rather than a gather that
    # materializes an (n, k, d) tensor
    mask = torch.zeros((n, n), device=X.device, dtype=torch.float32)
    mask.scatter_(1, idx, 1.0)
    out = (mask @ Xf) / k
    return out.to(X.dtype)


# ---------------------------------------------------------------------------
# attacks
# ---------------------------------------------------------------------------


def empire(honest: torch.Tensor, scale: float = -1.0) -> torch.Tensor:
    return (honest.float().mean(dim=0) * scale).to(honest.dtype)


def sign_flip(base_grad: torch.Tensor, scale: float = -1.0) -> torch.Tensor:
    return base_grad * scale


def little(honest: torch.Tensor, f: int, N: Optional[int] = None) -> torch.Tensor:
    """'A Little Is Enough': mu + z * sigma with s = floor(N/2)+1-f,
    z = Phi^{-1}((N-s)/N) (little.py:81-231)."""
    n = honest.shape[0]
    N_total = N if N is not None else n + f
    s = N_total // 2 + 1 - f
    phi_arg = (N_total - s) / N_total
    z = float(
        torch.distributions.Normal(0.0, 1.0).icdf(torch.tensor(float(phi_arg)))
    )
    Hf = honest.float()
    mu = Hf.mean(dim=0)
    sigma = Hf.std(dim=0, unbiased=False)
    return (mu + z * sigma).to(honest.dtype)


def gaussian_attack(
    like: torch.Tensor, mu: float = 0.0, sigma: float = 1.0, seed: Optional[int] = None
) -> torch.Tensor:
    d = like.shape[-1]
    if seed is not None:
        gen = torch.Generator(device="cpu")
        gen.manual_seed(seed)
        out = torch.normal(mu, sigma, size=(d,), generator=gen)
        return out.to(device=like.device, dtype=like.dtype)
    return torch.normal(
        mu, sigma, size=(d,), device=like.device, dtype=torch.float32
    ).to(like.dtype)


def inf_attack(like: torch.Tensor) -> torch.Tensor:
    return torch.full(
        (like.shape[-1],), float("inf"), device=like.device, dtype=like.dtype
    )


def mimic(honest: torch.Tensor, epsilon: int = 0) -> torch.Tensor:
    return honest[epsilon].clone()


# Min-Max / Min-Sum (Shejwalkar & Houmansadr, NDSS 2021): m = mu + gamma * p
# with the largest gamma >= 0 that keeps m inside the honest cloud. This is
# the oracle's own text: explicit differences, explicit pairwise distances
# and gamma by bisection on the constraint, all in f64. The device path
# (hip/dispatch.py) uses a fused statistics pass and the closed-form root.

PERTURBATIONS = ("unit", "std", "sign")


def attack_perturbation(honest: torch.Tensor, perturbation: str = "std"):
    """(mu, p) in f64: the column mean and the perturbation direction,
    "unit" -mu/||mu||, "std" -sigma (population), "sign" -sign(mu)."""
    if perturbation not in PERTURBATIONS:
        raise ValueError(
            f"perturbation must be one of {PERTURBATIONS}, got {perturbation!r}"
        )
    H = honest.double()
    mu = H.mean(dim=0)
    if perturbation == "unit":
        norm = mu.norm()
        p = -mu / norm if float(norm) > 0.0 else torch.zeros_like(mu)
    elif perturbation == "std":
        p = -H.std(dim=0, unbiased=False)
    else:
        p = -torch.sign(mu)
    return mu, p


def _largest_feasible(feasible) -> float:
    """Largest gamma >= 0 with feasible(gamma), for a constraint that holds
    on an interval [0, gamma*]: bracket [hi/2, hi] by doubling (or halving)
    from 1, then 64 bisection steps."""
    if not feasible(0.0):
        return 0.0
    hi = 1.0
    if feasible(hi):
        while feasible(hi):
            hi *= 2.0
            if hi > 1e300:
                raise ValueError("constraint never binds")
    else:
        while not feasible(0.5 * hi):
            hi *= 0.5
            if hi < 1e-300:
                return 0.0
    lo = 0.5 * hi
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        if feasible(mid):
            lo = mid
        else:
            hi = mid
    return lo


def _attack_terms(honest: torch.Tensor, perturbation: str):
    """mu, p and the terms of ||mu + gamma p - x_i||^2 = a_i + 2 gamma b_i +
    gamma^2 c, from explicit differences in f64."""
    mu, p = attack_perturbation(honest, perturbation)
    diff = mu[None, :] - honest.double()
    a = (diff * diff).sum(dim=1)
    b = (diff * p[None, :]).sum(dim=1)
    c = float((p * p).sum())
    return mu, p, a, b, c


def _pairwise_sq_dists_explicit(honest: torch.Tensor) -> torch.Tensor:
    """(n, n) squared distances from explicit differences, f64, a row at a
    time (no (n, n, d) temporary)."""
    H = honest.double()
    return torch.stack([((H - H[i][None, :]) ** 2).sum(dim=1) for i in range(len(H))])


def min_max_gamma(honest: torch.Tensor, perturbation: str = "std") -> float:
    """Largest gamma with max_i ||m - x_i||^2 <= max_ij ||x_i - x_j||^2."""
    _, _, a, b, c = _attack_terms(honest, perturbation)
    if c == 0.0:
        return 0.0
    tau = float(_pairwise_sq_dists_explicit(honest).max())
    return _largest_feasible(
        lambda g: float((a + 2.0 * g * b + g * g * c).max()) <= tau
    )


def min_sum_gamma(honest: torch.Tensor, perturbation: str = "std") -> float:
    """Largest gamma with sum_i ||m - x_i||^2 <= max_i sum_j ||x_i - x_j||^2."""
    _, _, a, b, c = _attack_terms(honest, perturbation)
    if c == 0.0:
        return 0.0
    tau_s = float(_pairwise_sq_dists_explicit(honest).sum(dim=1).max())
    return _largest_feasible(
        lambda g: float((a + 2.0 * g * b + g * g * c).sum()) <= tau_s
    )


def min_max(honest: torch.Tensor, perturbation: str = "std") -> torch.Tensor:
    mu, p = attack_perturbation(honest, perturbation)
    gamma = min_max_gamma(honest, perturbation)
    return (mu + gamma * p).to(honest.dtype)


def min_sum(honest: torch.Tensor, perturbation: str = "std") -> torch.Tensor:
    mu, p = attack_perturbation(honest, perturbation)
    gamma = min_sum_gamma(honest, perturbation)
    return (mu + gamma * p).to(honest.dtype)


# Aggregator-tailored attacks (Shejwalkar & Houmansadr, NDSS 2021, section
# IV-B): the adversary knows the server's rule and sends f copies of
# m = mu + gamma * p with the largest gamma for which the rule still selects
# them. The oracle's own text: the explicit (n + f, d) attacked matrix, the
# existing Krum scores / Bulyan selection run on it, gamma by bisection. The
# device path (hip/dispatch.py) works on the Gram and the quadratic
# a_i + 2 gamma b_i + gamma^2 c instead.

AGR_RULES = ("krum", "multi-krum", "bulyan")


def agr_check(n: int, f: int, agr: str, q: Optional[int] = None) -> int:
    """Validate the arguments of a tailored attack on n honest rows; returns
    the winner count q (1 for Krum, n by default for Multi-Krum, unused by
    Bulyan)."""
    if agr not in AGR_RULES:
        raise ValueError(f"agr must be one of {AGR_RULES}, got {agr!r}")
    if f < 1:
        raise ValueError(f"a tailored attack needs f >= 1, got f={f}")
    if agr == "bulyan":
        if n < 3 * f + 3:
            raise ValueError(
                f"Bulyan needs n + f >= 4f + 3, got n={n} honest rows, f={f}"
            )
        return n - f
    if n < 2 or f > n:
        raise ValueError(f"Krum needs n >= 2 and f <= n, got n={n}, f={f}")
    if agr == "krum":
        return 1
    q = n if q is None else int(q)
    if q < 1 or q > n + f:
        raise ValueError(f"need 1 <= q <= n + f, got q={q}, n={n}, f={f}")
    return q


def _agr_attacked(honest: torch.Tensor, gamma: float, f: int, perturbation: str):
    """cat(honest, f copies of mu + gamma p) in f64."""
    mu, p = attack_perturbation(honest, perturbation)
    m = mu + float(gamma) * p
    return torch.cat([honest.double(), m[None, :].expand(f, -1)], dim=0)


def agr_feasible(
    honest: torch.Tensor,
    gamma: float,
    f: int,
    agr: str,
    q: Optional[int] = None,
    perturbation: str = "std",
) -> bool:
    """Whether the rule, run with parameter f on the n honest rows followed
    by f copies of mu + gamma p, selects the malicious rows: all f of them
    for Bulyan; for Krum / Multi-Krum at most max(q - f, 0) honest rows score
    no worse than a malicious one (ties go to the honest, smaller, index).
    Anything NaN is infeasible."""
    n = honest.shape[0]
    q = agr_check(n, f, agr, q)
    A = _agr_attacked(honest, gamma, f, perturbation)
    if not bool(torch.isfinite(A).all()):
        return False
    if agr == "bulyan":
        picks = bulyan_select(A, f)
        return int((picks >= n).sum()) == f
    scores = multi_krum_scores(A, f)
    if bool(torch.isnan(scores).any()):
        return False
    s_m = scores[n:].max()
    return int((scores[:n] <= s_m).sum()) <= max(q - f, 0)


def agr_tailored_gamma(
    honest: torch.Tensor,
    f: int,
    agr: str,
    q: Optional[int] = None,
    perturbation: str = "std",
) -> float:
    """Upper end of the feasible interval that starts at gamma = 0; 0 when
    gamma = 0 is already infeasible or the perturbation vanishes."""
    agr_check(honest.shape[0], f, agr, q)
    _, p = attack_perturbation(honest, perturbation)
    c = float((p * p).sum())
    if c == 0.0 or not math.isfinite(c):
        return 0.0
    return _largest_feasible(
        lambda g: agr_feasible(honest, g, f, agr, q, perturbation)
    )


def agr_tailored(
    honest: torch.Tensor,
    f: int,
    agr: str = "multi-krum",
    q: Optional[int] = None,
    perturbation: str = "std",
) -> torch.Tensor:
    mu, p = attack_perturbation(honest, perturbation)
    gamma = agr_tailored_gamma(honest, f, agr, q, perturbation)
    return (mu + gamma * p).to(honest.dtype)


# Tailored attacks on the coordinate-wise rules (Shejwalkar & Houmansadr,
# NDSS 2021, section IV-B): against the trimmed mean and the median the
# adversary sends f copies of m = mu + gamma * p with the gamma that moves the
# rule's output farthest from the honest mean, D(gamma) = ||mu - A(gamma)||^2.
# D is bounded and not monotone, so gamma comes from a fixed maximisation
# schedule, not a boundary search. The oracle's own text: the explicit
# (n + f, d) attacked matrix, a sort, the rule read off the sorted rows. The
# device path (hip/dispatch.py) sorts the honest rows once and never builds
# the attacked matrix.

AGR_COORD_RULES = ("trimmed-mean", "median")

# The schedule, shared in words with hip/dispatch.py: round 0 tries gamma = 0
# and gamma0 2^k, k = -15 .. 15; each of the two zoom rounds places 32 equally
# spaced points strictly inside (lo, hi), the evaluated points next below and
# next above the incumbent (the incumbent itself where there is none). The
# largest D wins, equal D goes to the smaller gamma, a D that is not finite
# never wins. Every trial gamma is an f32 value (what the device kernel
# takes), worked out in f64 and rounded.
_COORD_GEO = tuple(range(-15, 16))
_COORD_POINTS = 32
_COORD_ZOOMS = 2


def agr_coord_check(n: int, f: int, agr: str) -> None:
    if agr not in AGR_COORD_RULES:
        raise ValueError(f"agr must be one of {AGR_COORD_RULES}, got {agr!r}")
    if f < 1:
        raise ValueError(f"a tailored attack needs f >= 1, got f={f}")
    if agr == "trimmed-mean" and f >= n:
        raise ValueError(
            f"the trimmed mean of n + f rows drops 2f: need f < n, got n={n}, f={f}"
        )


def _coord_rule(A: torch.Tensor, f: int, agr: str) -> torch.Tensor:
    """The rule on the rows of A in A's own dtype: the text of ``median`` /
    ``trimmed_mean`` above without their casts to f32."""
    N = A.shape[0]
    s, _ = torch.sort(A, dim=0)
    if agr == "median":
        if N % 2 == 1:
            return s[N // 2]
        return (s[N // 2 - 1] + s[N // 2]) * 0.5
    return s[f : N - f].mean(dim=0)


def agr_coord_objective(
    honest: torch.Tensor,
    gamma: float,
    f: int,
    agr: str,
    perturbation: str = "std",
    *,
    mu: Optional[torch.Tensor] = None,
    p: Optional[torch.Tensor] = None,
    dtype: torch.dtype = torch.float64,
) -> float:
    """D(gamma) = sum_j (mu_j - A_j)^2, A the rule's output on the honest rows
    followed by f copies of mu + gamma p. ``mu`` and ``p`` default to
    ``attack_perturbation``; given, they are used as they are (mu need not be
    the column mean). ``dtype`` is the arithmetic of every step up to mu - A;
    the squares are summed in f64 either way."""
    agr_coord_check(honest.shape[0], int(f), agr)
    if mu is None or p is None:
        mu0, p0 = attack_perturbation(honest, perturbation)
        mu = mu0 if mu is None else mu
        p = p0 if p is None else p
    mu, p = mu.to(dtype), p.to(dtype)
    m = mu + torch.tensor(float(gamma), dtype=dtype) * p
    A = torch.cat([honest.to(dtype), m[None, :].expand(int(f), -1)], dim=0)
    diff = (mu - _coord_rule(A, int(f), agr)).double()
    return float((diff * diff).sum())


def _f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float64).float())


def _coord_better(D: float, g: float, best_D: float, best_g: float) -> bool:
    if not math.isfinite(D):
        return False
    return D > best_D or (D == best_D and g < best_g)


def agr_coord_gamma(
    honest: torch.Tensor,
    f: int,
    agr: str,
    perturbation: str = "std",
    *,
    gamma0: Optional[float] = None,
    mu: Optional[torch.Tensor] = None,
    p: Optional[torch.Tensor] = None,
) -> float:
    """The gamma of the schedule above. The anchor gamma0 defaults to the
    Min-Sum value sqrt(max_i a_i / c), and gamma is then 0 when c = 0 or a
    statistic is not finite; a given ``gamma0`` is taken as it is (c is not
    looked at) and gives 0 when it is not finite. gamma is 0 when no trial's
    D is finite."""
    agr_coord_check(honest.shape[0], int(f), agr)
    mu0, p0 = attack_perturbation(honest, perturbation)
    mu = mu0 if mu is None else mu
    p = p0 if p is None else p
    if gamma0 is None:
        diff = mu.double()[None, :] - honest.double()
        a_max = float((diff * diff).sum(dim=1).max())
        c = float((p.double() * p.double()).sum())
        if not (c > 0.0 and math.isfinite(c)):
            return 0.0
        gamma0 = math.sqrt(a_max / c) if a_max >= 0.0 else float("nan")
    gamma0 = _f32(float(gamma0))
    if not math.isfinite(gamma0):
        return 0.0

    def D(g):
        return agr_coord_objective(honest, g, f, agr, perturbation, mu=mu, p=p)

    best_g, best_D = 0.0, -math.inf
    trials = [0.0] + [_f32(gamma0 * 2.0**k) for k in _COORD_GEO]
    nodes = trials  # the points that can bound the next round's interval
    for r in range(1 + _COORD_ZOOMS):
        for g in trials:
            Dg = D(g)
            if _coord_better(Dg, g, best_D, best_g):
                best_g, best_D = g, Dg
        if r == _COORD_ZOOMS:
            break
        lo = max([x for x in nodes if x < best_g], default=best_g)
        hi = min([x for x in nodes if x > best_g], default=best_g)
        trials = [
            _f32(lo + (hi - lo) * j / (_COORD_POINTS + 1))
            for j in range(1, _COORD_POINTS + 1)
        ]
        nodes = [lo] + trials + [hi]
    return best_g


def agr_coord(
    honest: torch.Tensor,
    f: int,
    agr: str = "trimmed-mean",
    perturbation: str = "std",
) -> torch.Tensor:
    mu, p = attack_perturbation(honest, perturbation)
    gamma = agr_coord_gamma(honest, f, agr, perturbation)
    return (mu + gamma * p).to(honest.dtype)
