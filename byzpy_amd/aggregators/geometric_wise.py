"""Geometry-based robust aggregators (Krum family, GeoMedian, MDA, MoNNA,
SMEA).

Reference parity: aggregators/geometric_wise/*.py. GPU path: the pairwise
Gram runs on the MFMA split-K kernel (K4); selection/scoring on small
(n, n) tensors; Weiszfeld as fused per-iteration kernels (K6).
"""
from __future__ import annotations

import itertools
import math
from typing import Any, List, Sequence

import torch

from byzpy_amd.aggregators import _subtask_fns as SF
from byzpy_amd.aggregators._chunking import chunk_ranges
from byzpy_amd.aggregators.base import Aggregator
from byzpy_amd.graph.subtask import SubTask
from byzpy_amd.hip import dispatch as D
from byzpy_amd.ops import functional as F
from byzpy_amd.ops.base import OpContext
from byzpy_amd.storage.shared_store import register_tensor, write_handle
from byzpy_amd.utils.flatten import stack_gradients, to_like


class MultiKrum(Aggregator):
    """Pairwise sq-dists -> score_i = sum of n-f-1 nearest -> mean of the q
    best (Blanchard et al. 2017). Row-chunked Gram on CPU pools."""

    name = "multi-krum"
    supports_subtasks = True
    max_subtasks_inflight = 0

    def __init__(self, f: int, q: int, *, chunk_size: int = 32) -> None:
        if f < 0 or q < 1:
            raise ValueError("need f >= 0 and q >= 1")
        self.f, self.q = int(f), int(q)
        self.chunk_size = int(chunk_size)

    def _aggregate(self, X: torch.Tensor) -> torch.Tensor:
        return D.multi_krum(X, self.f, self.q)

    def create_subtasks(self, ctx: OpContext, **inputs: Any) -> Sequence[SubTask]:
        gradients = inputs[self.input_key]
        ref, X, like, handles = self._matrix_ref(ctx, gradients)
        if X.is_cuda:
            return []
        ctx.metadata["_op_pending"] = (X, like, handles)
        n = X.shape[0]
        chunk = max(1, min(self.chunk_size, n))
        return [
            SubTask(fn=SF.gram_row_chunk, args=(ref, lo, hi), name=f"gram[{lo}:{hi}]")
            for lo, hi in chunk_ranges(n, chunk)
        ]

    def reduce_subtasks(self, ctx: OpContext, results: List[Any], **inputs: Any) -> Any:
        X, like, handles = ctx.metadata.pop("_op_pending")
        try:
            G = torch.cat(results, dim=0)
            winners = D.krum_winners_from_gram(G, self.f, self.q)
            return to_like(D.mean_rows(X, winners), like)
        finally:
            self._cleanup(handles)


class Krum(MultiKrum):
    """MultiKrum(q=1) returning the single winner itself."""

    name = "krum"

    def __init__(self, f: int, *, chunk_size: int = 32) -> None:
        super().__init__(f, 1, chunk_size=chunk_size)

    def _aggregate(self, X: torch.Tensor) -> torch.Tensor:
        return D.krum(X, self.f)

    def reduce_subtasks(self, ctx: OpContext, results: List[Any], **inputs: Any) -> Any:
        X, like, handles = ctx.metadata.pop("_op_pending")
        try:
            scores = D.krum_scores_from_gram(torch.cat(results, dim=0), self.f)
            return to_like(X[int(torch.argmin(scores))].clone(), like)
        finally:
            self._cleanup(handles)


class Bulyan(Aggregator):
    """Bulyan (El Mhamdi, Guerraoui, Rouault 2018): n - 2f rows chosen by
    iterated Krum, then per coordinate the mean of the n - 4f selected
    values closest to their median. Needs n >= 4f + 3. Row-chunked Gram on
    CPU pools; Gram + one selection launch + one indexed column launch on
    GPU."""

    name = "bulyan"
    supports_subtasks = True
    max_subtasks_inflight = 0

    def __init__(self, f: int, *, chunk_size: int = 32) -> None:
        if f < 0:
            raise ValueError("f must be >= 0")
        self.f = int(f)
        self.chunk_size = int(chunk_size)

    def _check(self, n: int) -> None:
        if n < 4 * self.f + 3:
            raise ValueError(
                f"Bulyan needs n >= 4f + 3, got n={n}, f={self.f}"
            )

    def _aggregate(self, X: torch.Tensor) -> torch.Tensor:
        self._check(X.shape[0])
        return D.bulyan(X, self.f)

    def create_subtasks(self, ctx: OpContext, **inputs: Any) -> Sequence[SubTask]:
        gradients = inputs[self.input_key]
        ref, X, like, handles = self._matrix_ref(ctx, gradients)
        if X.is_cuda:
            return []
        n = X.shape[0]
        try:
            self._check(n)
        except ValueError:
            self._cleanup(handles)
            raise
        ctx.metadata["_op_pending"] = (X, like, handles)
        chunk = max(1, min(self.chunk_size, n))
        return [
            SubTask(fn=SF.gram_row_chunk, args=(ref, lo, hi), name=f"gram[{lo}:{hi}]")
            for lo, hi in chunk_ranges(n, chunk)
        ]

    def reduce_subtasks(self, ctx: OpContext, results: List[Any], **inputs: Any) -> Any:
        X, like, handles = ctx.metadata.pop("_op_pending")
        try:
            G = torch.cat(results, dim=0)
            sel = D.bulyan_select_from_gram(G, self.f)
            return to_like(D.mean_of_medians(X, 2 * self.f, rows=sel), like)
        finally:
            self._cleanup(handles)


class DnC(Aggregator):
    """Divide-and-Conquer (Shejwalkar & Houmansadr, NDSS 2021): ``niters``
    times, sample b = min(subsample, d) coordinates, score every row by its
    squared projection on the centred sample's top singular direction and
    keep the n - floor(c f) lowest; average the rows kept every time. An
    empty intersection returns zeros (skip the round).

    Two departures from the paper: a row with a non-finite sampled entry
    (inf, NaN, or |x| > 2^48) is never kept and does not enter the column
    means; and coordinates are drawn WITH replacement (``torch.randint``,
    sorted), so a draw is b integers, not a permutation of d.

    ``coords`` fixes the sample: an int (niters, b) tensor, each row sorted
    ascending, duplicates allowed. Otherwise every call draws from a CPU
    generator (seeded by ``seed``, else torch's global one) and moves the
    draw to the input's device, so one seed gives one sample on CPU and GPU.
    For hipGraph capture pass ``coords`` as an int32 device tensor.

    GPU: sampled centred Grams, spectral selection, counted gather-mean —
    no host sync up to 128 rows. CPU pools: partial Grams over chunks of
    ``chunk_size`` sampled coordinates."""

    name = "dnc"
    supports_subtasks = True
    max_subtasks_inflight = 0

    def __init__(
        self,
        f: int,
        *,
        niters: int = 5,
        subsample: int = 10_000,
        c: float = 1.0,
        coords: "torch.Tensor | None" = None,
        seed: "int | None" = None,
        chunk_size: int = 2048,
    ) -> None:
        if f < 0:
            raise ValueError("f must be >= 0")
        if c < 0:
            raise ValueError("c must be >= 0")
        if niters < 1:
            raise ValueError("niters must be >= 1")
        if subsample < 1:
            raise ValueError("subsample must be >= 1")
        self.f, self.c = int(f), float(c)
        self.niters, self.subsample = int(niters), int(subsample)
        self.chunk_size = max(1, int(chunk_size))
        self.coords = None
        if coords is not None:
            coords = torch.as_tensor(coords)
            if coords.dim() != 2 or coords.shape[0] < 1 or coords.shape[1] < 1:
                raise ValueError("coords must be (niters, b)")
            if coords.dtype not in (torch.int32, torch.int64):
                raise ValueError("coords must be int32 or int64")
            if not coords.is_cuda and bool(
                (coords[:, 1:] < coords[:, :-1]).any()
            ):
                raise ValueError("each row of coords must be sorted ascending")
            self.coords = coords
            self.niters = int(coords.shape[0])
        self._gen = None
        if seed is not None:
            self._gen = torch.Generator(device="cpu")
            self._gen.manual_seed(int(seed))

    def _coords_for(self, X: torch.Tensor) -> torch.Tensor:
        """The call's (niters, b) sample on X's device, after the checks that
        need the shape of X."""
        n, d = X.shape
        F.dnc_keep(n, self.f, self.c)
        if self.coords is not None:
            co = self.coords
            if not co.is_cuda and bool(((co < 0) | (co >= d)).any()):
                raise ValueError(f"coords must lie in [0, {d})")
            return co.to(X.device)
        b = min(self.subsample, d)
        draw = torch.randint(0, d, (self.niters, b), generator=self._gen)
        return torch.sort(draw, dim=1).values.to(X.device)

    def _aggregate(self, X: torch.Tensor) -> torch.Tensor:
        return D.dnc(X, self.f, self._coords_for(X), self.c)

    def create_subtasks(self, ctx: OpContext, **inputs: Any) -> Sequence[SubTask]:
        gradients = inputs[self.input_key]
        ref, X, like, handles = self._matrix_ref(ctx, gradients)
        if X.is_cuda:
            return []
        try:
            coords = self._coords_for(X)
        except ValueError:
            self._cleanup(handles)
            raise
        ctx.metadata["_op_pending"] = (X, like, handles)
        b = coords.shape[1]
        return [
            SubTask(
                fn=SF.dnc_gram_chunk,
                args=(ref, coords[:, lo:hi].contiguous()),
                name=f"dnc_gram[{lo}:{hi}]",
            )
            for lo, hi in chunk_ranges(b, min(self.chunk_size, b))
        ]

    def reduce_subtasks(self, ctx: OpContext, results: List[Any], **inputs: Any) -> Any:
        X, like, handles = ctx.metadata.pop("_op_pending")
        try:
            Gc = sum(r[0] for r in results)
            bad = sum(r[1] for r in results)
            keep = F.dnc_keep(X.shape[0], self.f, self.c)
            idx, count = D.dnc_select_from_gram(Gc, bad, keep)
            return to_like(D.mean_rows_counted(X, idx, count), like)
        finally:
            self._cleanup(handles)


class AFA(Aggregator):
    """Adaptive Federated Averaging (Muñoz-González, Co, Lupu 2019), one
    round of its Algorithm 1: pass after pass, drop the rows whose cosine to
    the weighted mean of the rows still alive lies more than xi standard
    deviations past the median, on the side the mean lies (xi grows by
    delta_xi after every pass that dropped a row), then return the weighted
    mean of the survivors; zeros when none survives (skip the round).

    ``weights`` (n,) >= 0, default all ones, may be replaced between calls
    (``agg.weights = ...``); AFAReputation keeps the paper's cross-round
    state and produces them. A non-finite row or one of weight 0 is never
    kept.

    GPU: MFMA Gram, one selection launch, counted gather-mean — no host sync
    up to 128 rows. CPU pools: row-chunked Gram."""

    name = "afa"
    supports_subtasks = True
    max_subtasks_inflight = 0

    def __init__(
        self,
        xi: float = 2.0,
        delta_xi: float = 0.5,
        *,
        weights: "torch.Tensor | Sequence[float] | None" = None,
        chunk_size: int = 32,
    ) -> None:
        F._afa_check(xi, delta_xi)
        self.xi, self.delta_xi = float(xi), float(delta_xi)
        self.weights = weights
        self.chunk_size = int(chunk_size)

    def _aggregate(self, X: torch.Tensor) -> torch.Tensor:
        return D.afa(X, self.weights, self.xi, self.delta_xi)

    def create_subtasks(self, ctx: OpContext, **inputs: Any) -> Sequence[SubTask]:
        gradients = inputs[self.input_key]
        ref, X, like, handles = self._matrix_ref(ctx, gradients)
        if X.is_cuda:
            return []
        n = X.shape[0]
        try:
            F._afa_weights(self.weights, n)
        except ValueError:
            self._cleanup(handles)
            raise
        ctx.metadata["_op_pending"] = (X, like, handles)
        chunk = max(1, min(self.chunk_size, n))
        return [
            SubTask(fn=SF.gram_row_chunk, args=(ref, lo, hi), name=f"gram[{lo}:{hi}]")
            for lo, hi in chunk_ranges(n, chunk)
        ]

    def reduce_subtasks(self, ctx: OpContext, results: List[Any], **inputs: Any) -> Any:
        X, like, handles = ctx.metadata.pop("_op_pending")
        try:
            G = torch.cat(results, dim=0)
            idx, count = D.afa_select_from_gram(
                G, self.weights, self.xi, self.delta_xi
            )
            w = None
            if self.weights is not None:
                w = F._afa_weights(self.weights, X.shape[0])
            return to_like(D.mean_rows_counted(X, idx, count, weights=w), like)
        finally:
            self._cleanup(handles)


class AFAReputation:
    """The cross-round state of AFA: a Beta(alpha, beta) belief per client
    that it sends good updates. ``update(good_mask)`` adds 1 to alpha for the
    clients the round kept and to beta for those it dropped; a client is
    ``blocked`` once P[p < 0.5] = I_0.5(alpha, beta) >= block_at, and is
    never updated again. ``weights(sizes)`` = alpha / (alpha + beta) * sizes,
    0 where blocked: what AFA takes as ``weights``.

    alpha0, beta0 are positive integers, so the Beta CDF at 0.5 is the
    finite binomial sum sum_{j=alpha}^{N} C(N, j) 2^-N with
    N = alpha + beta - 1, computed exactly in integers."""

    def __init__(
        self, n: int, alpha0: float = 3.0, beta0: float = 3.0, block_at: float = 0.95
    ) -> None:
        if n < 1:
            raise ValueError("n must be >= 1")
        if alpha0 != int(alpha0) or beta0 != int(beta0) or alpha0 < 1 or beta0 < 1:
            raise ValueError("alpha0 and beta0 must be integers >= 1")
        if not 0.0 < block_at <= 1.0:
            raise ValueError("block_at must lie in (0, 1]")
        self.alpha = [int(alpha0)] * int(n)
        self.beta = [int(beta0)] * int(n)
        self.block_at = float(block_at)
        self._blocked = [False] * int(n)
        self._refresh()

    @staticmethod
    def cdf_half(alpha: int, beta: int) -> float:
        """I_0.5(alpha, beta) for integers alpha, beta >= 1."""
        N = alpha + beta - 1
        return sum(math.comb(N, j) for j in range(alpha, N + 1)) / 2**N

    def _refresh(self) -> None:
        for i, (a, b) in enumerate(zip(self.alpha, self.beta)):
            if not self._blocked[i] and self.cdf_half(a, b) >= self.block_at:
                self._blocked[i] = True

    @property
    def blocked(self) -> torch.Tensor:
        return torch.tensor(self._blocked, dtype=torch.bool)

    def update(self, good_mask) -> None:
        good = torch.as_tensor(good_mask).detach().cpu().flatten().tolist()
        if len(good) != len(self.alpha):
            raise ValueError(
                f"good_mask: expected {len(self.alpha)} entries, got {len(good)}"
            )
        for i, g in enumerate(good):
            if self._blocked[i]:
                continue
            if g:
                self.alpha[i] += 1
            else:
                self.beta[i] += 1
        self._refresh()

    def weights(self, sizes=None) -> torch.Tensor:
        p = torch.tensor(
            [a / (a + b) for a, b in zip(self.alpha, self.beta)],
            dtype=torch.float32,
        )
        if sizes is not None:
            sz = torch.as_tensor(sizes, dtype=torch.float32).flatten()
            if sz.numel() != p.numel():
                raise ValueError(
                    f"sizes: expected {p.numel()} entries, got {sz.numel()}"
                )
            p = p * sz
        return p.masked_fill(self.blocked, 0.0)


class GeometricMedian(Aggregator):
    """Weiszfeld fixed point; barriered per-iteration fan-out on CPU pools
    (reference geometric_median.py:106-158), fused kernels on GPU."""

    name = "geometric-median"
    supports_barriered_subtasks = True
    max_subtasks_inflight = 0

    def __init__(
        self,
        *,
        tol: float = 1e-6,
        max_iter: int = 256,
        eps: float = 1e-12,
        init: str = "median",
        chunk_size: int = 32,
        fixed_iters: "int | None" = None,
    ) -> None:
        if tol <= 0 or max_iter <= 0 or eps <= 0:
            raise ValueError("tol, max_iter, eps must be > 0")
        if init not in {"median", "mean"}:
            raise ValueError("init must be 'median' or 'mean'")
        if fixed_iters is not None and fixed_iters <= 0:
            raise ValueError("fixed_iters must be > 0")
        self.tol, self.max_iter, self.eps = float(tol), int(max_iter), float(eps)
        self.init = init
        self.chunk_size = int(chunk_size)
        # fixed_iters: exactly that many Weiszfeld steps, NO convergence
        # polls — fully async on GPU (per-node streams overlap; hipGraph
        # capture-safe). The poll-free path is what unblocks config-4
        # gossip (round-1 weakness 5).
        self.fixed_iters = None if fixed_iters is None else int(fixed_iters)

    def _aggregate(self, X: torch.Tensor) -> torch.Tensor:
        return D.geometric_median(
            X, tol=self.tol, max_iter=self.max_iter, eps=self.eps,
            init=self.init, fixed_iters=self.fixed_iters
        )

    async def run_barriered_subtasks(self, ctx: OpContext, **inputs: Any) -> Any:
        gradients = inputs[self.input_key]
        ref, X, like, handles = self._matrix_ref(ctx, gradients)
        if X.is_cuda:
            self._cleanup(handles)
            return to_like(self._aggregate(X), like)
        use_shm = handles != []
        center_handle = None
        try:
            n = X.shape[0]
            chunk = max(1, min(self.chunk_size, n))
            iters = self.fixed_iters if self.fixed_iters is not None else self.max_iter
            z = (F.median(X) if self.init == "median" else X.float().mean(dim=0)).float()
            if use_shm:
                # ONE segment, rewritten per iteration (reference
                # geometric_median.py:126 _write_handle semantics)
                center_handle = register_tensor(z)
            for _ in range(iters):
                if use_shm:
                    write_handle(center_handle, z)
                    center_ref = center_handle
                else:
                    center_ref = z
                tasks = [
                    SubTask(
                        fn=SF.weiszfeld_chunk,
                        args=(ref, lo, hi, center_ref, self.eps),
                    )
                    for lo, hi in chunk_ranges(n, chunk)
                ]
                partials = await self._run_subtasks(ctx, tasks)
                num = sum(p[0] for p in partials)
                den = sum(p[1] for p in partials)
                z_new = num / den
                shift = float((z_new - z).norm())
                z = z_new
                if self.fixed_iters is None and shift <= self.tol:
                    break
            return to_like(z.to(X.dtype), like)
        finally:
            if center_handle is not None:
                self._cleanup([center_handle])
            self._cleanup(handles)


class MinimumDiameterAveraging(Aggregator):
    """Exact min-diameter (n-f)-subset mean; combo-batched subtasks on CPU
    pools, host branch-and-bound over the device-computed D2 on GPU."""

    name = "minimum-diameter-averaging"
    supports_subtasks = True
    max_subtasks_inflight = 0

    def __init__(self, f: int, *, chunk_size: int = 256) -> None:
        if f < 0:
            raise ValueError("f must be >= 0")
        self.f = int(f)
        self.chunk_size = int(chunk_size)

    def _aggregate(self, X: torch.Tensor) -> torch.Tensor:
        return D.minimum_diameter_averaging(X, self.f)

    def create_subtasks(self, ctx: OpContext, **inputs: Any) -> Sequence[SubTask]:
        gradients = inputs[self.input_key]
        X, like = stack_gradients(gradients)
        if X.is_cuda:
            return []
        n = X.shape[0]
        m = n - self.f
        D2 = F.pairwise_sq_dists(X)
        use_shm = bool(getattr(ctx.pool, "prefers_shared_memory", False))
        handles = []
        if use_shm:
            ref = register_tensor(D2)
            handles.append(ref)
        else:
            ref = D2
        ctx.metadata["_op_pending"] = (X, like, handles)
        combos = list(itertools.combinations(range(n), m))
        batch = max(1, self.chunk_size)
        return [
            SubTask(fn=SF.mda_combo_chunk, args=(ref, combos[i : i + batch], m))
            for i in range(0, len(combos), batch)
        ]

    def reduce_subtasks(self, ctx: OpContext, results: List[Any], **inputs: Any) -> Any:
        X, like, handles = ctx.metadata.pop("_op_pending")
        try:
            # min diameter, then lexicographic subset (canonical tie-break)
            best_diam, best = min(results, key=lambda r: (r[0], r[1]))
            idx = torch.tensor(best, dtype=torch.long)
            out = X.float()[idx].mean(dim=0).to(X.dtype)
            return to_like(out, like)
        finally:
            self._cleanup(handles)


class MoNNA(Aggregator):
    """Mean of the n-f nearest neighbours of a trusted reference row."""

    name = "monna"
    supports_subtasks = True
    max_subtasks_inflight = 0

    def __init__(self, f: int, *, reference_index: int = 0, chunk_size: int = 32) -> None:
        if f < 0:
            raise ValueError("f must be >= 0")
        self.f = int(f)
        self.reference_index = int(reference_index)
        self.chunk_size = int(chunk_size)

    def _aggregate(self, X: torch.Tensor) -> torch.Tensor:
        return D.monna(X, self.f, self.reference_index)

    def create_subtasks(self, ctx: OpContext, **inputs: Any) -> Sequence[SubTask]:
        gradients = inputs[self.input_key]
        ref, X, like, handles = self._matrix_ref(ctx, gradients)
        if X.is_cuda:
            return []
        ctx.metadata["_op_pending"] = (X, like, handles)
        n = X.shape[0]
        chunk = max(1, min(self.chunk_size, n))
        return [
            SubTask(
                fn=SF.ref_dist_chunk, args=(ref, lo, hi, self.reference_index)
            )
            for lo, hi in chunk_ranges(n, chunk)
        ]

    def reduce_subtasks(self, ctx: OpContext, results: List[Any], **inputs: Any) -> Any:
        X, like, handles = ctx.metadata.pop("_op_pending")
        try:
            d2 = torch.cat(results)
            d2[self.reference_index] = -1.0  # reference-first tiebreak
            k = X.shape[0] - self.f
            idx = torch.argsort(d2, stable=True)[:k]
            out = X.float()[idx].mean(dim=0).to(X.dtype)
            return to_like(out, like)
        finally:
            self._cleanup(handles)


class SMEA(Aggregator):
    """Smallest max-eigenvalue (n-f)-subset mean; Gram once, combo-batched
    eigensolves."""

    name = "smea"
    supports_subtasks = True
    max_subtasks_inflight = 0

    def __init__(self, f: int, *, chunk_size: int = 256) -> None:
        if f < 0:
            raise ValueError("f must be >= 0")
        self.f = int(f)
        self.chunk_size = int(chunk_size)

    def _aggregate(self, X: torch.Tensor) -> torch.Tensor:
        return D.smea(X, self.f)

    def create_subtasks(self, ctx: OpContext, **inputs: Any) -> Sequence[SubTask]:
        gradients = inputs[self.input_key]
        X, like = stack_gradients(gradients)
        if X.is_cuda:
            return []
        n = X.shape[0]
        m = n - self.f
        Xf = X.float()
        G = Xf @ Xf.T
        use_shm = bool(getattr(ctx.pool, "prefers_shared_memory", False))
        handles = []
        if use_shm:
            ref = register_tensor(G)
            handles.append(ref)
        else:
            ref = G
        ctx.metadata["_op_pending"] = (X, like, handles)
        combos = list(itertools.combinations(range(n), m))
        batch = max(1, self.chunk_size)
        return [
            SubTask(fn=SF.smea_combo_chunk, args=(ref, combos[i : i + batch], m))
            for i in range(0, len(combos), batch)
        ]

    def reduce_subtasks(self, ctx: OpContext, results: List[Any], **inputs: Any) -> Any:
        X, like, handles = ctx.metadata.pop("_op_pending")
        try:
            best_ev, best = min(results, key=lambda r: r[0])
            idx = torch.tensor(best, dtype=torch.long)
            out = X.float()[idx].mean(dim=0).to(X.dtype)
            return to_like(out, like)
        finally:
            self._cleanup(handles)
