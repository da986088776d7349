"""Bulyan on one MI355X: the fused device path against its unfused
compositions, and the row-indexed mean-around-median kernel against the
un-indexed kernel on the gathered rows.

Versions, alternated round by round in one process:
  fused     D.bulyan: MFMA Gram, one selection launch, one indexed colsel
  unfused   the same Gram, the selection as torch ops on the Gram (about ten
            launches per pick), X[sel] gathered, un-indexed colsel
  oracle    F.bulyan on the device tensor (selection loop on the host)
  indexed   ext.colsel(X, 2, 2f, sel) alone
  gathered  ext.colsel(X[sel], 2, 2f) alone, gather not timed

Every version is warmed up, then timed with device events in batches sized
to >= 0.1 s, `--rounds` batches per version; the table gives the median
batch and the min..max spread, per call. Achieved bytes/s of the indexed
kernel counts theta * d * sizeof(T), the bytes it has to read.

Usage: python benchmarks/bench_bulyan.py [--out FILE.md] [--rounds 5]
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
from byzpy_amd.ops import functional as F

SHAPES = [(64, 1 << 20, 15), (64, 1 << 24, 15), (16, 1 << 24, 3)]


def _inputs(n, d, dtype, device):
    g = torch.Generator().manual_seed(1000 + n)
    scale = (1 + 0.1 * torch.arange(n))[torch.randperm(n, generator=g)]
    gd = torch.Generator(device=device).manual_seed(1000 + n)
    X = torch.empty(n, d, dtype=dtype, device=device)
    for i in range(n):  # row by row: no (n, d) f32 staging copy
        X[i] = (torch.randn(d, generator=gd, device=device) * scale[i]).to(dtype)
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
        sys.exit("bench_bulyan needs a GPU: timings elsewhere mean nothing")
    ext = require()
    dev = torch.device("cuda:0")
    dtype, size = torch.bfloat16, 2
    shapes = [(16, 4096, 3)] if args.small else SHAPES
    lines = [
        "| n x d (bf16), f | version | ms/call median | min..max | calls/batch |",
        "|---|---|---|---|---|",
    ]
    notes = []
    for n, d, f in shapes:
        X = _inputs(n, d, dtype, dev)
        theta = n - 2 * f
        sel = D.bulyan_select_from_gram(D.gram(X), f)
        Xg = X[sel.long()].contiguous()

        def unfused():
            s = D._bulyan_select_torch(D.gram(X), f)
            return D.mean_of_medians(X[s.long()].contiguous(), 2 * f)

        versions = {
            "fused": lambda: D.bulyan(X, f),
            "unfused": unfused,
            "oracle": lambda: F.bulyan(X, f),
            "indexed": lambda: ext.colsel(X, 2, 2 * f, sel),
            "gathered": lambda: ext.colsel(Xg, 2, 2 * f),
        }
        out = {k: fn() for k, fn in versions.items()}
        torch.cuda.synchronize()
        same = (
            f"fused == unfused bitwise: {torch.equal(out['fused'], out['unfused'])}, "
            f"indexed == gathered bitwise: {torch.equal(out['indexed'], out['gathered'])}"
        )
        err = (out["fused"].float() - out["oracle"].float()).abs().max().item()
        del out
        res = measure(versions, args.rounds)
        for k, (med, lo, hi, reps) in res.items():
            lines.append(
                f"| {n} x {d}, f={f} | {k} | {med:.3f} | {lo:.3f}..{hi:.3f} | {reps} |"
            )
        gbs = theta * d * size / (res["indexed"][0] * 1e-3) / 1e9
        notes.append(
            f"- {n} x {d}, f={f}: fused/unfused = "
            f"{res['fused'][0] / res['unfused'][0]:.3f}, fused/oracle = "
            f"{res['fused'][0] / res['oracle'][0]:.4f}, indexed/gathered = "
            f"{res['indexed'][0] / res['gathered'][0]:.3f}; indexed kernel reads "
            f"theta*d*{size} B = {theta * d * size / 1e6:.1f} MB at {gbs:.0f} GB/s; "
            f"max |fused - oracle| = {err:.3g} (bf16 output); {same}"
        )
        del X, Xg
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n\n" + "\n".join(notes) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
