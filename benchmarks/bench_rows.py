"""Lists of per-worker device tensors aggregated in place (K19) on one
MI355X: the row-pointer kernels against stacking the list first.

Versions per shape and operation, alternated round by round in one process:
  (i)   public stacked   aggregate(rows) with BYZPY_ROWS_IN_PLACE=stack:
                         torch.stack + the contiguous kernels (the route
                         before K19)
  (ii)  public in place  aggregate(rows): the row-pointer kernels
  (iii) kernel stacked   the contiguous kernels alone on a pre-stacked matrix
  (iv)  kernel in place  the row-pointer kernels alone on the list
Operations: median, trimmed mean (f = 15), Multi-Krum (f = 16, q = 12; Gram,
selection and mean of the winners). Rows are separately allocated (16 B
aligned: vector loads, packed bf16 median). `--element` times the element-
load fallbacks once, on rows at odd element offsets of one buffer.

Every version is warmed up, then timed with device events in batches sized
to >= 0.1 s, `--rounds` batches per version; the table gives the median
batch and the min..max spread, per call.

Usage: python benchmarks/bench_rows.py [--element] [--out FILE.md] [--rounds 5]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from bench_minmax import _inputs, measure
from byzpy_amd.aggregators import (
    CoordinateWiseMedian,
    CoordinateWiseTrimmedMean,
    MultiKrum,
)
from byzpy_amd.hip import dispatch as D
from byzpy_amd.hip import require

# (n, d)
SHAPES = [(64, 1 << 16), (64, 1 << 20), (64, 1 << 24), (33, 1 << 24)]
DTYPES = [(torch.bfloat16, "bf16"), (torch.float32, "f32")]
ENV = "BYZPY_ROWS_IN_PLACE"
TRIM_F, KRUM_F, KRUM_Q = 15, 16, 12


def _stacked(fn):
    def run():
        os.environ[ENV] = "stack"
        try:
            return fn()
        finally:
            os.environ.pop(ENV, None)

    return run


def _versions(X, rows):
    ops = {
        "median": (CoordinateWiseMedian(), lambda A: D.median(A)),
        "trimmed": (CoordinateWiseTrimmedMean(TRIM_F), lambda A: D.trimmed_mean(A, TRIM_F)),
        "multi-krum": (MultiKrum(KRUM_F, KRUM_Q), lambda A: D.multi_krum(A, KRUM_F, KRUM_Q)),
    }
    out = {}
    for name, (agg, kern) in ops.items():
        out[f"{name} (i) public stacked"] = _stacked(lambda agg=agg: agg.aggregate(rows))
        out[f"{name} (ii) public in place"] = lambda agg=agg: agg.aggregate(rows)
        out[f"{name} (iii) kernel stacked"] = lambda kern=kern: kern(X)
        out[f"{name} (iv) kernel in place"] = lambda kern=kern: kern(rows)
    return out


def _offset_rows(X):
    n, d = X.shape
    buf = torch.empty(n * (d + 1) + 1, dtype=X.dtype, device=X.device)
    rows = [buf[i * (d + 1) + 1 : i * (d + 1) + 1 + d] for i in range(n)]
    for r, x in zip(rows, X):
        r.copy_(x)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--element", action="store_true", help="element-load paths, 64 x 1M")
    ap.add_argument("--small", action="store_true", help="tiny shapes (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rows needs a GPU: timings elsewhere mean nothing")
    ext = require()
    dev = torch.device("cuda:0")
    lines = ["| n x d | version | ms/call median | min..max | calls/batch |", "|---|---|---|---|---|"]
    notes = []
    shapes = [(40, 4096)] if args.small else ([(64, 1 << 20)] if args.element else SHAPES)
    for n, d in shapes:
        for dtype, dname in DTYPES:
            X = _inputs(n, d, dtype, dev)
            tag = f"{n} x {d} {dname}"
            if args.element:
                rows = _offset_rows(X)
                idx = torch.arange(KRUM_Q, device=dev, dtype=torch.int32)
                versions = {
                    "median, element loads": lambda: ext.colsel(rows, 0, 0),
                    "median, contiguous": lambda: D.median(X),
                    "gram, element loads": lambda: ext.gram(rows),
                    "gram, contiguous": lambda: D.gram(X),
                    "mean_rows, element loads": lambda: ext.mean_rows(rows, idx),
                    "mean_rows, contiguous": lambda: D.mean_rows(X, idx),
                }
            else:
                rows = [X[i].clone() for i in range(n)]
                versions = _versions(X, rows)
            res = measure(versions, args.rounds)
            for k, (med, lo, hi, reps) in res.items():
                lines.append(f"| {tag} | {k} | {med:.4f} | {lo:.4f}..{hi:.4f} | {reps} |")
            if not args.element:
                for op in ("median", "trimmed", "multi-krum"):
                    t = {v: res[f"{op} ({v}) {w}"][0] for v, w in
                         [("i", "public stacked"), ("ii", "public in place"),
                          ("iii", "kernel stacked"), ("iv", "kernel in place")]}
                    a, b = versions[f"{op} (iii) kernel stacked"](), versions[f"{op} (iv) kernel in place"]()
                    diff = (a.float() - b.float()).abs().max().item()
                    notes.append(
                        f"- {tag}, {op}: (iv) / (iii) = {t['iv'] / t['iii']:.3f}, "
                        f"(ii) / (i) = {t['ii'] / t['i']:.3f} "
                        f"((i) - (ii) = {t['i'] - t['ii']:.4f} ms); largest |(iii) - (iv)| {diff:.3g}"
                    )
            del X, rows, versions
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n\n" + "\n".join(notes) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
