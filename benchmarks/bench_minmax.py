"""Min-Max / Min-Sum on one MI355X: the fused statistics pass against the
same outputs from other kernels, with row_sqnorms on the same matrix as the
pure-stream yardstick, then the two attacks end to end.

Versions, alternated round by round in one process:
  fused     ext.little_fused(X, 0, 1): mu, p, a, b, c (one pass at n <= 64)
  unfused   the same outputs from kernels older than the attack:
            caf_colsum (mu), little_fused(X, 1) (mu + sigma, so p),
            row_center_sqdists (a), caf_matvec (-b), torch for c
  sqnorms   ext.row_sqnorms(X): one read of X, nothing else
  min_max   D.min_max(X): statistics pass + MFMA Gram + closed-form gamma
  min_sum   D.min_sum(X): statistics pass + closed-form gamma

Every version is warmed up, then timed with device events in batches sized
to >= 0.1 s, `--rounds` batches per version; the table gives the median
batch and the min..max spread, per call. GB/s counts n * d * sizeof(T), one
read of X, whatever the version actually reads.

Usage: python benchmarks/bench_minmax.py [--out FILE.md] [--rounds 5]
"""
from __future__ import annotations

import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from byzpy_amd.hip import dispatch as D
from byzpy_amd.hip import require

SHAPES = [
    (64, 1 << 24, torch.bfloat16),
    (16, 1 << 24, torch.bfloat16),
    (64, 1 << 22, torch.float32),
]


def _inputs(n, d, dtype, device):
    g = torch.Generator().manual_seed(1000 + n)
    scale = (1 + 0.1 * torch.arange(n))[torch.randperm(n, generator=g)]
    gd = torch.Generator(device=device).manual_seed(1000 + n)
    X = torch.empty(n, d, dtype=dtype, device=device)
    for i in range(n):  # row by row: no (n, d) f32 staging copy
        X[i] = (torch.randn(d, generator=gd, device=device) * scale[i] + 0.3).to(dtype)
    return X


def _time_batch(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps  # ms per call


def measure(versions, rounds):
    reps = {}
    for name, fn in versions.items():  # warm up, then size the batches
        fn()
        torch.cuda.synchronize()
        t = _time_batch(fn, 1)
        reps[name] = max(1, math.ceil(100.0 / max(t, 1e-3)))
    samples = {name: [] for name in versions}
    for _ in range(rounds):
        for name, fn in versions.items():
            samples[name].append(_time_batch(fn, reps[name]))
    return {
        k: (statistics.median(v), min(v), max(v), reps[k]) for k, v in samples.items()
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="tiny shapes (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_minmax needs a GPU: timings elsewhere mean nothing")
    ext = require()
    dev = torch.device("cuda:0")
    shapes = [(16, 4096, torch.bfloat16)] if args.small else SHAPES
    lines = [
        "| n x d | version | ms/call median | min..max | GB/s (one read of X) | calls/batch |",
        "|---|---|---|---|---|---|",
    ]
    notes = []
    for n, d, dtype in shapes:
        X = _inputs(n, d, dtype, dev)
        name = "bf16" if dtype == torch.bfloat16 else "f32"
        ones = torch.ones(n, device=dev)
        inv_n = torch.full((), 1.0 / n, device=dev)

        def fused():
            return ext.little_fused(X, 0.0, 1)

        def unfused():
            mu = ext.caf_colsum(X, ones, None, inv_n)
            p = mu - ext.little_fused(X, 1.0).float()
            a = ext.row_center_sqdists(X, mu)
            b = -ext.caf_matvec(X, mu, p)
            return mu, p, torch.cat([a, b, (p * p).sum()[None]])

        versions = {
            "fused": fused,
            "unfused": unfused,
            "sqnorms": lambda: ext.row_sqnorms(X),
            "min_max": lambda: D.min_max(X),
            "min_sum": lambda: D.min_sum(X),
        }
        out = {k: versions[k]() for k in ("fused", "unfused")}
        torch.cuda.synchronize()

        def rel(x, y):
            return ((x - y).norm() / y.norm().clamp_min(1e-30)).item()

        agree = (
            f"unfused vs fused: mu {rel(out['unfused'][0], out['fused'][0]):.1e}, "
            f"p {rel(out['unfused'][1], out['fused'][1]):.1e}, "
            f"stats {rel(out['unfused'][2], out['fused'][2]):.1e}"
        )
        del out
        res = measure(versions, args.rounds)
        nbytes = n * d * X.element_size()
        for k, (med, lo, hi, reps) in res.items():
            lines.append(
                f"| {n} x {d} {name} | {k} | {med:.3f} | {lo:.3f}..{hi:.3f} | "
                f"{nbytes / (med * 1e-3) / 1e9:.0f} | {reps} |"
            )
        f_med, f_lo, f_hi, _ = res["fused"]
        notes.append(
            f"- {n} x {d} {name}: fused/unfused = {f_med / res['unfused'][0]:.3f}, "
            f"fused/sqnorms = {f_med / res['sqnorms'][0]:.2f}; fused spread "
            f"{(f_hi - f_lo) / f_med:.1%}, unfused spread "
            f"{(res['unfused'][2] - res['unfused'][1]) / res['unfused'][0]:.1%}; "
            f"relative differences, {agree}"
        )
        del X
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n\n" + "\n".join(notes) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
