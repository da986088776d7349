"""CAF on one MI355X: the iterative K9 route (8 passes over X, a d-long host
draw and a host readback per round) against ``solver="gram"`` (K21: Gram, one
solver launch for every round, one combine pass).

Measured, per shape, dtype and f, in one process on the same inputs:
  caf iterative / gram             CAF(f, solver=...)._aggregate(X)
  caf gram from a list             the rows as n separate tensors, read in place
  gram pass, combine               the two passes over X of the gram route alone
and the solver launch alone at n = 64 and 128, on a typical Gram (rounds as
the input needs) and on the worst case (an input on which every one of the n
rounds runs).

Every version is warmed up, then timed with device events in batches sized
to >= 0.1 s, `--rounds` batches per version, versions alternating; the table
gives the median batch and the min..max spread, per call. The iterative route
at d = 2^24 takes seconds per call and is timed in single-call batches.

``--accuracy`` measures instead the error that the f32 MFMA Gram alone forces
on the end-to-end test inputs of tests/test_gpu_caf_gram.py: F.caf_gram in
f64 on the device Gram, combined in f64, against the d-space f64 loop. No
part of it runs the solver kernel.

Usage: python benchmarks/bench_caf_gram.py [--out FILE.md] [--rounds 3]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from bench_minmax import _inputs, measure
from byzpy_amd.aggregators import CAF
from byzpy_amd.hip import dispatch as D
from byzpy_amd.hip import require
from byzpy_amd.ops import functional as F

SHAPES = [(64, 1 << 16), (64, 1 << 24)]
DTYPES = [torch.bfloat16, torch.float32]
FS = (8, 15)


def _row(lines, shape, name, r, extra=""):
    med, lo, hi, reps = r
    lines.append(f"| {shape} | {name} | {med:.4f} | {lo:.4f}..{hi:.4f} | {reps} | {extra} |")


def _routes(lines, n, d, dtype, dev, rounds):
    X = _inputs(n, d, dtype, dev)
    shape = f"{n} x {d} {'bf16' if dtype == torch.bfloat16 else 'f32'}"
    fast, slow = {}, {}
    for f in FS:
        gram, it = CAF(f, solver="gram"), CAF(f)
        fast[f"caf gram, f={f}"] = lambda a=gram: a._aggregate(X)
        (slow if d >= 1 << 22 else fast)[f"caf iterative, f={f}"] = lambda a=it: a._aggregate(X)
    a0 = torch.full((n,), 1.0 / n, device=dev)
    fast["gram pass"] = lambda: D.gram(X)
    fast["combine alone"] = lambda: D.combine_rows(X, a0)
    if d >= 1 << 22:
        rows = [r.clone() for r in X]
        gram = CAF(FS[0], solver="gram")
        fast[f"caf gram from a list, f={FS[0]}"] = lambda: gram._aggregate(rows)
    res = measure(fast, rounds)
    res.update(measure(slow, 1) if slow else {})
    for f in FS:
        G = D.gram(X)
        rnd = int(D.caf_gram(G, f)[2])
        ratio = res[f"caf iterative, f={f}"][0] / res[f"caf gram, f={f}"][0]
        _row(lines, shape, f"caf iterative, f={f}", res[f"caf iterative, f={f}"], f"{rnd} rounds")
        _row(lines, shape, f"caf gram, f={f}", res[f"caf gram, f={f}"], f"{ratio:.1f}x faster")
    for name in res:
        if not name.startswith("caf iterative") and not name.startswith("caf gram, "):
            _row(lines, shape, name, res[name])


def _solver(lines, ext, n, dev, rounds):
    g = torch.Generator().manual_seed(n)
    X = torch.randn(n, 4096, generator=g)
    X[: n // 4] += 3.0
    typical = (X.double() @ X.double().T).float().to(dev)
    # two far outliers and n - 2f <= 2: the mass never gets there, n rounds run
    Y = torch.randn(n, 256, generator=g, dtype=torch.float64)
    Y[:2] *= 20.0
    worst = (Y @ Y.T).float().to(dev)
    seeds = F.caf_gram_seeds(n).to(dev)
    v = {}
    for name, G, f in (("typical", typical, n // 8), ("worst case", worst, (n - 1) // 2)):
        rnd = int(ext.caf_matvec(G, seeds, f=f, power_iters=3)[2])
        v[f"solver alone, {name}, {rnd} rounds"] = (
            lambda G=G, f=f: ext.caf_matvec(G, seeds, f=f, power_iters=3)
        )
    for name, r in measure(v, rounds).items():
        _row(lines, f"{n} x {n} Gram", name, r)


def _accuracy(lines):
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
    import test_gpu_caf_gram as T

    cases = [(17, 4, False), (64, 16, False), (128, 32, False), (33, 8, False), (17, 4, True)]
    for n, f, inf in cases:
        for dtype in (torch.float32, torch.bfloat16):
            X = T._inputs(n, dtype)
            if inf:
                X[9, 11] = float("inf")
            ref = T._ref(X, n, f, (n, dtype, inf))
            G = D.solver_gram(X.cuda()).cpu()
            a = F.caf_gram(G, f, F.caf_gram_seeds(n))[0]
            live = a != 0
            out = a[live] @ X[live].double()
            rel = float((out - ref).abs().max() / ref.abs().max())
            lines.append(f"| {n} | {f} | {dtype} | {'inf row' if inf else ''} | {rel:.3e} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--small", action="store_true", help="tiny shapes (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_caf_gram needs a GPU: timings elsewhere mean nothing")
    ext = require()
    dev = torch.device("cuda:0")
    if args.accuracy:
        lines = ["| n | f | dtype | | rel err of the f32 Gram alone |", "|---|---|---|---|---|"]
        _accuracy(lines)
    else:
        lines = [
            "| shape | version | ms/call median | min..max | calls/batch | |",
            "|---|---|---|---|---|---|",
        ]
        for n in (64, 128):
            _solver(lines, ext, n, dev, args.rounds)
        for n, d in [(16, 4096)] if args.small else SHAPES:
            for dtype in DTYPES:
                _routes(lines, n, d, dtype, dev, args.rounds)
                torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
