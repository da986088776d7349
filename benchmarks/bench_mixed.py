"""Mixing pre-aggregator + coordinate-wise rule on one MI355X: the fused
kernel ``colsel(X, mode, f, mix=)`` (K18, no mixed matrix) against the
composition that writes the (m, d) mixed matrix and reads it back.

Versions, alternated round by round in one process:
  step nnm->tm fused / split       the mix + select step alone, membership
                                   given: ext.colsel(X, 1, f, mix=) against
                                   trimmed_mean(group_mean_rows(X, idx), f)
  step bucket->median fused/split  ext.colsel(X, 0, 0, mix=) against
                                   median(bucket_mean(X, perm, s))
  nnm->tm fused / split            PreAggregated(NNM(f), TrimmedMean(f)) end
                                   to end (Gram and neighbour search included)
  bucket->median fused / split     PreAggregated(Bucketing(s), Median())

`--sweep` times the NNM step at d = 64K .. 16M and n in {33, 64} instead: the
table behind dispatch.MIXED_COLSEL_FUSED_MIN_D.

Every version is warmed up, then timed with device events in batches sized
to >= 0.1 s, `--rounds` batches per version; the table gives the median
batch and the min..max spread, per call.

Usage: python benchmarks/bench_mixed.py [--sweep] [--out FILE.md] [--rounds 5]
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
    PreAggregated,
)
from byzpy_amd.hip import dispatch as D
from byzpy_amd.hip import require
from byzpy_amd.pre_aggregators import Bucketing, NearestNeighborMixing

# (n, d, f, bucket size)
SHAPES = [(64, 1 << 24, 15, 2)]
SWEEP = [(n, 1 << e, n // 4) for n in (33, 64) for e in (16, 18, 20, 22, 24)]
ENV = "BYZPY_MIXED_COLSEL"


def _routed(route, fn):
    def run():
        os.environ[ENV] = route
        try:
            return fn()
        finally:
            os.environ.pop(ENV, None)

    return run


def _nnm_step(ext, X, f):
    nnm = NearestNeighborMixing(f)
    mix = nnm.membership(X)
    idx = D.nearest_rows_from_gram(D.gram(X), X.shape[0] - f).to(torch.int32)
    return {
        "step nnm->tm fused": lambda: ext.colsel(X, 1, f, mix=mix),
        "step nnm->tm split": lambda: D.trimmed_mean(D.group_mean_rows(X, idx), f),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="routing threshold sweep")
    ap.add_argument("--small", action="store_true", help="tiny shapes (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mixed needs a GPU: timings elsewhere mean nothing")
    ext = require()
    dev = torch.device("cuda:0")
    lines = [
        "| n x d bf16, f | version | ms/call median | min..max | calls/batch |",
        "|---|---|---|---|---|",
    ]
    notes = []
    if args.sweep:
        shapes = [(16, 4096, 3)] if args.small else SWEEP
        for n, d, f in shapes:
            X = _inputs(n, d, torch.bfloat16, dev)
            versions = _nnm_step(ext, X, f)
            res = measure(versions, args.rounds)
            for k, (med, lo, hi, reps) in res.items():
                lines.append(f"| {n} x {d}, f = {f} | {k} | {med:.4f} | {lo:.4f}..{hi:.4f} | {reps} |")
            fu, sp = res["step nnm->tm fused"], res["step nnm->tm split"]
            notes.append(
                f"- {n} x {d}: fused / split = {fu[0] / sp[0]:.2f} (medians), "
                f"worst fused {fu[2]:.4f} ms against best split {sp[1]:.4f} ms"
            )
            del X, versions
            torch.cuda.empty_cache()
    else:
        shapes = [(16, 4096, 3, 2)] if args.small else SHAPES
        for n, d, f, s in shapes:
            X = _inputs(n, d, torch.bfloat16, dev)
            versions = _nnm_step(ext, X, f)
            bucket = Bucketing(s, perm=torch.randperm(n).tolist())
            mixb = bucket.membership(X)
            perm = torch.as_tensor(bucket.perm, device=dev, dtype=torch.int32)
            versions["step bucket->median fused"] = lambda: ext.colsel(X, 0, 0, mix=mixb)
            versions["step bucket->median split"] = lambda: D.median(
                ext.bucket_mean(X, perm, s)
            )
            nnm_tm = PreAggregated(NearestNeighborMixing(f), CoordinateWiseTrimmedMean(f))
            buc_med = PreAggregated(bucket, CoordinateWiseMedian())
            for route in ("fused", "split"):
                versions[f"nnm->tm {route}"] = _routed(route, lambda: nnm_tm._aggregate(X))
                versions[f"bucket->median {route}"] = _routed(
                    route, lambda: buc_med._aggregate(X)
                )
            res = measure(versions, args.rounds)
            for k, (med, lo, hi, reps) in res.items():
                lines.append(f"| {n} x {d}, f = {f} | {k} | {med:.3f} | {lo:.3f}..{hi:.3f} | {reps} |")
            for pair in ("step nnm->tm", "step bucket->median", "nnm->tm", "bucket->median"):
                fu, sp = versions[f"{pair} fused"](), versions[f"{pair} split"]()
                diff = (fu.float() - sp.float()).abs().max().item()
                notes.append(
                    f"- {n} x {d}, {pair}: fused {res[f'{pair} fused'][0]:.3f} ms, split "
                    f"{res[f'{pair} split'][0]:.3f} ms "
                    f"({res[f'{pair} split'][0] / res[f'{pair} fused'][0]:.2f} x); largest "
                    f"|fused - split| {diff:.3g} (the split rounds the mixed rows to bf16)"
                )
            del X, versions
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n\n" + "\n".join(notes) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
