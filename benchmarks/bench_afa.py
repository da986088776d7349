"""AFA on one MI355X: the fused device path, its three launches one by one,
and the same selection loop as torch ops on the device Gram.

Versions, alternated round by round in one process:
  afa        D.afa(X): MFMA Gram, one selection launch, counted gather-mean
             (three binding calls, no host sync)
  afa_w      D.afa(X, w): the same with non-uniform weights, so the weighted
             counted gather-mean
  gram       D.gram(X) alone: the first pass over X
  select     ext.smea_select(G, weights=, xi=, delta_xi=) alone: the whole
             data-dependent loop in one launch
  mean       ext.mean_rows(X, idx, count=) alone: the second pass over X
  wmean      ext.mean_rows(X, idx, count=, weights=) alone
  torch_sel  D._afa_select_torch on the same device Gram: the loop as f64
             torch ops, one host sync per pass (the dispatch fallback past
             128 rows)

Every version is warmed up, then timed with device events in batches sized
to >= 0.1 s, `--rounds` batches per version; the table gives the median
batch and the min..max spread, per call.

Usage: python benchmarks/bench_afa.py [--out FILE.md] [--rounds 5]
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

# (n, d, flipped rows)
SHAPES = [(64, 1 << 24, 9), (64, 1 << 20, 9), (128, 1 << 20, 16)]


def _inputs(n, d, flipped, dtype, device):
    """Honest rows N(0.6, 1); the last `flipped` rows with the sign flipped."""
    gd = torch.Generator(device=device).manual_seed(3000 + n)
    X = torch.empty(n, d, dtype=dtype, device=device)
    for i in range(n):  # row by row: no (n, d) f32 staging copy
        row = torch.randn(d, generator=gd, device=device) + 0.6
        X[i] = (-row if i >= n - flipped else row).to(dtype)
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
        sys.exit("bench_afa needs a GPU: timings elsewhere mean nothing")
    ext = require()
    dev = torch.device("cuda:0")
    shapes = [(16, 4096, 3)] if args.small else SHAPES
    lines = [
        "| n x d, flipped | dtype | version | ms/call median | min..max | calls/batch |",
        "|---|---|---|---|---|---|",
    ]
    notes = []
    for n, d, flipped in shapes:
        for dtype, size, tag in ((torch.bfloat16, 2, "bf16"), (torch.float32, 4, "f32")):
            if tag == "f32" and d > (1 << 20):
                continue  # the issue's shape is bf16; f32 at the smaller d only
            X = _inputs(n, d, flipped, dtype, dev)
            ones = torch.ones(n, device=dev)
            w = (1.0 + (torch.arange(n, device=dev) % 3)).float()
            G = D.gram(X)
            idx, count, rounds = ext.smea_select(G, weights=ones, xi=2.0, delta_xi=0.5)
            versions = {
                "afa": lambda: D.afa(X),
                "afa_w": lambda: D.afa(X, w),
                "gram": lambda: D.gram(X),
                "select": lambda: ext.smea_select(G, weights=ones, xi=2.0, delta_xi=0.5),
                "mean": lambda: ext.mean_rows(X, idx, count=count),
                "wmean": lambda: ext.mean_rows(X, idx, count=count, weights=w),
                "torch_sel": lambda: D._afa_select_torch(G, ones, 2.0, 0.5),
            }
            i2, c2, r2 = D._afa_select_torch(G, ones, 2.0, 0.5)
            torch.cuda.synchronize()
            kept = int(count)
            same = (
                f"kept {kept} of {n} rows in {int(rounds)} passes (the {flipped} "
                f"flipped rows dropped: {idx[:kept].max().item() < n - flipped}); "
                f"fused selection == torch selection: "
                f"{torch.equal(idx, i2) and int(c2) == kept and r2 == int(rounds)}"
            )
            res = measure(versions, args.rounds)
            for k, (med, lo, hi, reps) in res.items():
                lines.append(
                    f"| {n} x {d}, {flipped} | {tag} | {k} | {med:.4f} | "
                    f"{lo:.4f}..{hi:.4f} | {reps} |"
                )
            passes = res["gram"][0] + res["mean"][0]
            notes.append(
                f"- {n} x {d} {tag}: select / (gram + mean) = "
                f"{res['select'][0] / passes:.4f}, select / torch_sel = "
                f"{res['select'][0] / res['torch_sel'][0]:.4f}, afa / (gram + select + "
                f"mean) = {res['afa'][0] / (passes + res['select'][0]):.3f}; gram reads "
                f"n*d*{size} B = {n * d * size / 1e6:.0f} MB at "
                f"{n * d * size / (res['gram'][0] * 1e-3) / 1e9:.0f} GB/s, mean reads "
                f"{kept}*d*{size} B at "
                f"{kept * d * size / (res['mean'][0] * 1e-3) / 1e9:.0f} GB/s; {same}"
            )
            del X, G
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n\n" + "\n".join(notes) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
