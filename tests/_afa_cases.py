"""Inputs shared by test_afa.py and test_gpu_afa.py: four kinds of client
matrices on which AFA takes its lower branch, its upper branch, several
passes, or drops next to nothing, and the decision margin of a run.

A selection computed from an f32 Gram can only be compared with the f64
oracle where no decision is close: ``margin`` is the smallest distance, over
the passes of the oracle's run, between a cosine and the pass's threshold and
between the mean and the median (which picks the branch). The seeds below were
chosen on the CPU (the first seed from 0 at which every run of the case
clears 2e-3, with and without the test weights, for f32 and bf16 values);
the tests assert MIN_MARGIN = 1e-3; the worst-case f32
dot-product error at the largest d here is 2050 * 2^-24 = 1.2e-4, so a cosine
off the device Gram cannot move a decision that clears it."""
import functools

import torch

from byzpy_amd.ops import functional as F

MIN_MARGIN = 1e-3
# (n, f, d): odd d, more than one block, the last register-width boundary of
# the Gram kernel, the selection kernel's row cap
SHAPES = [(9, 1, 33), (23, 3, 2050), (64, 9, 1030), (128, 16, 257)]
VARIANTS = ["flip", "tiers", "collude", "clean"]
# seed per (variant, n), see the module docstring
SEEDS = {
    ("flip", 9): 2, ("flip", 23): 0, ("flip", 64): 0, ("flip", 128): 0,
    ("flip", 129): 0,
    ("tiers", 9): 0, ("tiers", 23): 0, ("tiers", 64): 1, ("tiers", 128): 0,
    ("tiers", 129): 0,
    ("collude", 9): 0, ("collude", 23): 0, ("collude", 64): 2,
    ("collude", 128): 0, ("collude", 129): 1,
    ("clean", 9): 0, ("clean", 23): 1, ("clean", 64): 0, ("clean", 128): 5,
    ("clean", 129): 2,
}
# one row past the selection kernel's cap: the torch path on the device
OVER_CAP = (129, 16, 300)


def case_weights(n):
    """1 + (i mod 3), and one row at weight 0."""
    w = 1.0 + (torch.arange(n) % 3).float()
    w[n // 2] = 0.0
    return w


def build(variant, n, f, d, seed):
    g = torch.Generator().manual_seed(seed)

    def honest(m):
        scale = 1.0 + 0.1 * torch.arange(m, dtype=torch.float32)
        return torch.randn(m, d, generator=g) * (scale / scale.mean())[:, None] + 0.6

    def flipped(m, H):
        return -2.0 * H.mean(dim=0)[None, :] + 0.05 * torch.randn(m, d, generator=g)

    if variant == "flip":
        H = honest(n - f)
        rows = [H, flipped(f, H)]
    elif variant == "tiers":
        a = max(1, f // 2)
        b = f + 1 - a
        H = honest(n - a - b)
        rows = [H, flipped(a, H), torch.randn(b, d, generator=g) - 0.15]
    elif variant == "collude":
        v = torch.randn(d, generator=g)
        H = honest(n - f) - 0.6
        rows = [H, 6.0 * v[None, :] + 0.05 * torch.randn(f, d, generator=g)]
    elif variant == "clean":
        rows = [honest(n)]
    else:
        raise ValueError(variant)
    X = torch.cat(rows, dim=0)
    return X[torch.randperm(n, generator=g)].contiguous()


def margin(trace):
    """Smallest |s_i - threshold| over the alive rows and |mean - med|, over
    the passes of one oracle run."""
    m = float("inf")
    for r in trace:
        s = r["s"][r["alive"]]
        m = min(m, float((s - r["threshold"]).abs().min()), abs(r["mean"] - r["med"]))
    return m


@functools.lru_cache(maxsize=None)
def case(variant, n, f, d, dtype, weighted=False, seed=None):
    """One input (already cast to ``dtype``, so the oracle sees the device's
    values) with the oracle's run on it, built once."""
    seed = SEEDS[(variant, n)] if seed is None else seed
    X = build(variant, n, f, d, seed).to(dtype)
    w = case_weights(n) if weighted else None
    good, trace = F.afa_trace(X.float(), w)
    return dict(
        X=X, w=w, good=good, trace=trace, rounds=len(trace),
        margin=margin(trace), out=F.afa(X, w),
        lower=[r["lower"] for r in trace],
    )
