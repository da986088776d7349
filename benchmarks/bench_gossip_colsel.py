"""K24: a gossip round of a coordinate-wise rule, one pass against the loop.

Times, with device events and in one process, alternating the two routes:
  grouped  D.median / trimmed_mean / mean_of_medians(theta, groups=): every
           node's statistic in one pass over theta (colsel_groups.hip);
  loop     the per-node aggregate loop of gossip_round (its only route for
           these rules before K24, and still its fallback).
Each is set against the bytes its shape has to move, (rows read + M) x d x
sizeof(T): the grouped call reads each of the N rows once, the loop reads
every neighbourhood's rows again.

  python benchmarks/bench_gossip_colsel.py [--reps 7] [--quick]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from byzpy_amd.aggregators import (
    CoordinateWiseMedian,
    CoordinateWiseTrimmedMean,
    MeanOfMedians,
)
from byzpy_amd.hip import dispatch as D

MODES = ("median", "trimmed", "meamed")


def timed_pair(fa, fb, reps: int, warmup: int = 2):
    """(median, min, max) in ms of fa and of fb, the two alternating."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(reps):
        for k, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return tuple((statistics.median(t), min(t), max(t)) for t in ms)


def ring_rows(N: int, m: int):
    """node i listens to itself and the m - 1 rows around it on the ring"""
    return [[i] + [(i + s) % N for s in range(-((m - 1) // 2), m // 2 + 1) if s]
            for i in range(N)]


def case(theta: torch.Tensor, rows, mode: str, f: int, reps: int) -> None:
    N, d = theta.shape
    M, m = len(rows), max(len(r) for r in rows)
    groups = D.gossip_groups(rows, theta.device)
    if mode == "median":
        rule, grouped = CoordinateWiseMedian(), lambda: D.median(theta, groups=groups)
    elif mode == "trimmed":
        rule = CoordinateWiseTrimmedMean(f)
        grouped = lambda: D.trimmed_mean(theta, f, groups=groups)  # noqa: E731
    else:
        rule = MeanOfMedians(f)
        grouped = lambda: D.mean_of_medians(theta, f, groups=groups)  # noqa: E731

    def loop():
        return torch.stack([rule.aggregate([theta[j] for j in r]) for r in rows])

    tg, tl = timed_pair(grouped, loop, reps)
    size = theta.element_size()
    bg = (N + M) * d * size
    bl = (sum(len(r) for r in rows) + M) * d * size
    name = "bf16" if theta.dtype == torch.bfloat16 else "f32"
    # faster only past the run-to-run spread: the slowest grouped repetition
    # against the fastest of the loop
    verdict = "grouped" if tg[2] < tl[1] else ("loop" if tl[2] < tg[1] else "tie")
    print(f"| {name} | {N} x {d} | {m} | {mode} f={f} "
          f"| {tg[0]:.3f} ({tg[1]:.3f}-{tg[2]:.3f}) | {bg / 1e9:.2f} | {bg / tg[0] / 1e9:.2f} "
          f"| {tl[0]:.3f} ({tl[1]:.3f}-{tl[2]:.3f}) | {bl / 1e9:.2f} | {bl / tl[0] / 1e9:.2f} "
          f"| {tl[0] / tg[0]:.2f} | {verdict} |", flush=True)


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--quick", action="store_true", help="small shapes (a rehearsal)")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gossip_colsel.py measures device kernels: no GPU found")
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    print("| dtype | N x d | m | rule | grouped ms (min-max) | GB | TB/s "
          "| loop ms (min-max) | GB | TB/s | loop / grouped | faster |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")

    def theta(N, d, dtype):
        return torch.empty(N, d, dtype=dtype, device=dev).normal_(generator=g)

    # config 4: ring(8, 2), m = 5
    X = theta(8, 4096 * 5 + 3 if args.quick else 25_610_152, torch.bfloat16)
    for mode in MODES:
        case(X, ring_rows(8, 5), mode, 1, args.reps)
    del X
    for dtype in (torch.bfloat16, torch.float32):
        X = theta(64, 4096 * 9 + 5 if args.quick else 16 * 1024 * 1024, dtype)
        for m in (5, 17, 32):
            for mode in MODES:
                case(X, ring_rows(64, m), mode, m // 4, args.reps)
        del X
    X = theta(128, 4096 * 3 + 1 if args.quick else 4 * 1024 * 1024, torch.bfloat16)
    for mode in MODES:
        case(X, ring_rows(128, 5), mode, 1, args.reps)


if __name__ == "__main__":
    main()
