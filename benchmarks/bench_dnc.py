"""DnC on one MI355X: the fused device path against the same steps as torch
ops on the device, and against the bandwidth floor of the rule.

Versions, alternated round by round in one process:
  fused     D.dnc: sampled centred Grams, spectral selection, counted
            gather-mean (three binding calls, no host sync)
  torch     the same steps as torch ops on the device: the (niters, n, b)
            sample gathered by index, centring, bmm, f64 eigh (host sync),
            scores, argsort, intersection, counted gather-mean
  oracle    F.dnc on the device tensor (per-iteration loop, eigh on the host)
  mean      ext.mean_rows over `keep` rows alone: the rule has to read the
            rows it averages, so this is the floor the whole rule approaches
  gram      ext.gram(X, cols=) alone
  select    ext.smea_select(Gc, bad, keep) alone

Every version is warmed up, then timed with device events in batches sized
to >= 0.1 s, `--rounds` batches per version; the table gives the median
batch and the min..max spread, per call. Achieved bytes/s of `mean` counts
keep * d * sizeof(T), the bytes it has to read.

Usage: python benchmarks/bench_dnc.py [--out FILE.md] [--rounds 5]
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

# (n, d, f): niters = 5, b = 10,000, c = 1
SHAPES = [(64, 1 << 24, 15), (64, 1 << 20, 15)]
NITERS, SUBSAMPLE = 5, 10_000


def _inputs(n, d, dtype, device):
    """Honest rows N(0, 1); the last f rows shifted along one direction."""
    gd = torch.Generator(device=device).manual_seed(2000 + n)
    X = torch.empty(n, d, dtype=dtype, device=device)
    w = torch.randn(d, generator=gd, device=device)
    for i in range(n):  # row by row: no (n, d) f32 staging copy
        X[i] = torch.randn(d, generator=gd, device=device).to(dtype)
    return X, w


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
        sys.exit("bench_dnc needs a GPU: timings elsewhere mean nothing")
    ext = require()
    dev = torch.device("cuda:0")
    shapes = [(16, 4096, 3)] if args.small else SHAPES
    lines = [
        "| n x d, f | dtype | version | ms/call median | min..max | calls/batch |",
        "|---|---|---|---|---|---|",
    ]
    notes = []
    for n, d, f in shapes:
        for dtype, size, tag in ((torch.bfloat16, 2, "bf16"), (torch.float32, 4, "f32")):
            X, w = _inputs(n, d, dtype, dev)
            for i in range(n - f, n):
                X[i] = (X[i].float() + 3.0 * w).to(dtype)
            del w
            b = min(SUBSAMPLE, d)
            g = torch.Generator().manual_seed(7)
            coords = torch.sort(
                torch.randint(0, d, (NITERS, b), generator=g), dim=1
            ).values
            cols = coords.to(dev, torch.int32)
            keep = F.dnc_keep(n, f, 1.0)
            Gc, bad = ext.gram(X, cols=cols)
            idx, count = ext.smea_select(Gc, bad, keep)
            rows = idx[:keep].contiguous()

            def torch_steps():
                G2, b2 = D._dnc_gram_torch(X, cols)
                i2, c2 = D._dnc_select_torch(G2, b2, keep)
                return D.mean_rows_counted(X, i2, c2)

            versions = {
                "fused": lambda: D.dnc(X, f, cols, 1.0),
                "torch": torch_steps,
                "oracle": lambda: F.dnc(X, f, coords, 1.0),
                "mean": lambda: ext.mean_rows(X, rows),
                "gram": lambda: ext.gram(X, cols=cols),
                "select": lambda: ext.smea_select(Gc, bad, keep),
            }
            out = {k: versions[k]() for k in ("fused", "torch", "oracle")}
            torch.cuda.synchronize()
            kept = int(count)
            same = (
                f"kept {kept} of {n} rows (the {f} shifted rows dropped: "
                f"{idx[:kept].max().item() < n - f}); fused == torch bitwise: "
                f"{torch.equal(out['fused'], out['torch'])}; max |fused - oracle| = "
                f"{(out['fused'].float() - out['oracle'].float()).abs().max().item():.3g}"
            )
            del out
            res = measure(versions, args.rounds)
            for k, (med, lo, hi, reps) in res.items():
                lines.append(
                    f"| {n} x {d}, f={f} | {tag} | {k} | {med:.3f} | "
                    f"{lo:.3f}..{hi:.3f} | {reps} |"
                )
            gbs = keep * d * size / (res["mean"][0] * 1e-3) / 1e9
            notes.append(
                f"- {n} x {d} {tag}, f={f}: fused/torch = "
                f"{res['fused'][0] / res['torch'][0]:.3f}, fused/oracle = "
                f"{res['fused'][0] / res['oracle'][0]:.4f}, fused/mean = "
                f"{res['fused'][0] / res['mean'][0]:.3f}; mean reads keep*d*{size} B = "
                f"{keep * d * size / 1e6:.1f} MB at {gbs:.0f} GB/s; {same}"
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
