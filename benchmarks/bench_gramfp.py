"""GeometricMedian and CenteredClipping on one MI355X: the iterative kernels
(two passes over X per step) against ``solver="gram"`` (K20: Gram, one solver
launch, one combine pass, whatever the step count).

Versions, alternated round by round in one process, per shape and dtype:
  gm iterative / gram, k steps     GeometricMedian(init="mean", fixed_iters=k)
  cc iterative / gram, M steps     CenteredClipping(init="mean", M=M)
  gram pass, solver, combine       the three launches of the gram route alone
  gm gram from a list              the rows as n separate tensors, read in place
  nnm->gm iterative / gram         PreAggregated(NNM(f), GeometricMedian(...))
The last column is the time in units of the shape's Gram pass, the cheapest
full read of X measured here: the expectation under test is about 2 for the
gram route at any step count against about 2 k + 1 for the iterative one.

Every version is warmed up, then timed with device events in batches sized
to >= 0.1 s, `--rounds` batches per version; the table gives the median
batch and the min..max spread, per call.

Usage: python benchmarks/bench_gramfp.py [--out FILE.md] [--rounds 3]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from bench_minmax import _inputs, measure
from byzpy_amd.aggregators import CenteredClipping, GeometricMedian, PreAggregated
from byzpy_amd.hip import dispatch as D
from byzpy_amd.hip import require
from byzpy_amd.pre_aggregators import NearestNeighborMixing

SHAPES = [(64, 1 << 24), (33, 1 << 24)]
DTYPES = [torch.bfloat16, torch.float32]
STEPS = (8, 32)
CC_STEPS = 10


def _versions(ext, X, extras):
    n = X.shape[0]
    v = {}
    for k in STEPS:
        for solver in D.SOLVERS:
            gm = GeometricMedian(init="mean", fixed_iters=k, solver=solver)
            v[f"gm {solver}, {k} steps"] = lambda gm=gm: gm._aggregate(X)
    # distances are about sqrt(d): half of that clips every row
    c_tau = 0.5 * float(X.shape[1]) ** 0.5
    for solver in D.SOLVERS:
        cc = CenteredClipping(c_tau=c_tau, M=CC_STEPS, init="mean", solver=solver)
        v[f"cc {solver}, {CC_STEPS} steps"] = lambda cc=cc: cc._aggregate(X)
    G = D.gram(X)
    a0 = torch.full((n,), 1.0 / n, device=X.device)
    v["gram pass"] = lambda: D.gram(X)
    v[f"solver alone, {STEPS[-1]} steps"] = lambda: ext.weiszfeld_iter(
        G, a0, eps=1e-12, tol=0.0, iters=STEPS[-1]
    )
    v["combine alone"] = lambda: ext.mean_rows(X, coeffs=a0)
    if extras:
        rows = [r.clone() for r in X]
        gm = GeometricMedian(init="mean", fixed_iters=STEPS[-1], solver="gram")
        v[f"gm gram from a list, {STEPS[-1]} steps"] = lambda: gm._aggregate(rows)
        for solver in D.SOLVERS:
            agg = PreAggregated(
                NearestNeighborMixing(n // 4),
                GeometricMedian(init="mean", fixed_iters=STEPS[0], solver=solver),
            )
            v[f"nnm->gm {solver}, {STEPS[0]} steps"] = lambda agg=agg: agg._aggregate(X)
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="tiny shapes (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gramfp needs a GPU: timings elsewhere mean nothing")
    ext = require()
    dev = torch.device("cuda:0")
    lines = [
        "| n x d | version | ms/call median | min..max | / gram pass | calls/batch |",
        "|---|---|---|---|---|---|",
    ]
    shapes = [(16, 4096)] if args.small else SHAPES
    for n, d in shapes:
        for dtype in DTYPES:
            X = _inputs(n, d, dtype, dev)
            name = f"{n} x {d} {'bf16' if dtype == torch.bfloat16 else 'f32'}"
            # the list and NNM versions need a second copy of X: bf16 only
            versions = _versions(ext, X, extras=dtype == torch.bfloat16)
            res = measure(versions, args.rounds)
            unit = res["gram pass"][0]
            for k, (med, lo, hi, reps) in res.items():
                lines.append(
                    f"| {name} | {k} | {med:.3f} | {lo:.3f}..{hi:.3f} | "
                    f"{med / unit:.2f} | {reps} |"
                )
            del X, versions
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
