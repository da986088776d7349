"""The column-centred Gram on one MI355X (K22, csrc/gram_centered.hip).

Measured, per shape and dtype, in one process on the same input:
  gram(X)                 the uncentred MFMA Gram as it stands (what the
                          centring sweep costs on top of is read off here)
  gram(X, center=True)    the one-pass centred kernel
  mean, subtract, gram    the composition it replaces: f32 column mean,
                          X - mu into an (n, d) temporary cast back to X's
                          dtype, then gram of the temporary
Every version is warmed up, then timed with device events in batches sized
to >= 0.1 s, ``--rounds`` batches per version, versions alternating; the
table gives the median batch and the min..max spread, per call.

The accuracy table repeats the issue's comparison on the device at
64 x 65,536: rows = one N(0, 1) vector + rel x noise, max relative error of
the squared distances from the raw and from the centred Gram against f64 on
the stored values.

Usage: python benchmarks/bench_gram_centered.py [--out FILE.md] [--rounds 5]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from bench_minmax import _inputs, measure
from byzpy_amd.hip import dispatch as D
from byzpy_amd.hip import require

SHAPES = [
    (64, 1 << 16, torch.bfloat16),
    (64, 1 << 24, torch.bfloat16),
    (128, 1 << 24, torch.bfloat16),
    (64, 1 << 24, torch.float32),
    (128, 1 << 24, torch.float32),
]
ACCURACY = [(torch.float32, 2.0**-8), (torch.float32, 2.0**-12),
            (torch.bfloat16, 2.0**-8), (torch.bfloat16, 2.0**-12)]


def _name(dtype):
    return "bf16" if dtype == torch.bfloat16 else "f32"


def _composition(X):
    mu = torch.mean(X, dim=0, dtype=torch.float32)
    return D.gram((X - mu).to(X.dtype))


def _timings(lines, n, d, dtype, dev, rounds):
    X = _inputs(n, d, dtype, dev)
    res = measure(
        {
            "gram(X)": lambda: D.gram(X),
            "gram(X, center=True)": lambda: D.gram(X, center=True),
            "mean, subtract, gram": lambda: _composition(X),
        },
        rounds,
    )
    gb = n * d * X.element_size() / 1e9
    for name, (med, lo, hi, reps) in res.items():
        lines.append(
            f"| {n} x {d} {_name(dtype)} | {name} | {med:.4f} | {lo:.4f}..{hi:.4f} "
            f"| {gb / (med * 1e-3):.0f} | {reps} |"
        )
    return res["gram(X, center=True)"][0] < res["mean, subtract, gram"][0]


def _accuracy(lines, dtype, rel, dev):
    n, d = 64, 1 << 16
    g = torch.Generator().manual_seed(0)
    X = torch.randn(d, generator=g)[None, :] + rel * torch.randn(n, d, generator=g)
    X = X.to(dtype)
    Xd = X.double()
    ref = D.sq_dists_from_gram((Xd - Xd.mean(0)) @ (Xd - Xd.mean(0)).T)
    off = ~torch.eye(n, dtype=torch.bool)
    errs = []
    for center in (False, True):
        got = D.sq_dists_from_gram(D.gram(X.to(dev), center=center).double().cpu())
        errs.append(float(((got - ref).abs()[off] / ref[off]).max()))
    lines.append(f"| {_name(dtype)} | 2^{int(torch.log2(torch.tensor(rel)))} "
                 f"| {errs[0]:.2e} | {errs[1]:.2e} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="tiny shapes (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gram_centered needs a GPU: timings elsewhere mean nothing")
    require()
    dev = torch.device("cuda:0")
    shapes = [(17, 4099, torch.bfloat16)] if args.small else SHAPES
    lines = [
        "| n x d | version | ms/call median | min..max | GB/s (one read of X) | calls/batch |",
        "|---|---|---|---|---|---|",
    ]
    slower = []
    for n, d, dtype in shapes:
        if not _timings(lines, n, d, dtype, dev, args.rounds):
            slower.append(f"{n} x {d} {_name(dtype)}")
    lines += [
        "",
        "Kernel slower than the composition at: " + (", ".join(slower) or "no measured shape"),
        "",
        "| dtype | rel | max rel. error of D, raw gram | same, gram(center=True) |",
        "|---|---|---|---|",
    ]
    for dtype, rel in ACCURACY:
        _accuracy(lines, dtype, rel, dev)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
