"""Tailored attacks on the coordinate-wise rules on one MI355X: the one-pass
objective kernel (32 trial gammas per pass over X) against the plain median /
trimmed-mean kernels' pass over the same X, against the same arithmetic as
batched torch ops, and the attack end to end.

Versions, alternated round by round in one process:
  stats              ext.little_fused(X, 0, 1): mu, p, a, b, c
  colsel <rule>      D.median(X) / D.trimmed_mean(X, f): the aggregator's own
                     pass, the yardstick for bytes of X over time
  objective <rule>   ext.colsel(X, mode, f, mu=, p=, gammas=) with T = 32
  torch <rule>       D._agr_coord_objective_torch, same inputs, on the device
  attack <rule>      D.agr_coord(X, f, rule): stats + three objective passes
                     + the schedule's small device ops + addcmul

Every version is warmed up, then timed with device events in batches sized
to >= 0.1 s, `--rounds` batches per version; the table gives the median
batch and the min..max spread, per call, and the bytes of X over the time.
After the timings, one line per rule gives ||agg(X u m x f) - mu|| for the
tailored vector next to the Min-Max and Min-Sum vectors on the same input.

Usage: python benchmarks/bench_coord_tailored.py [--out FILE.md] [--rounds 5]
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

# (n, d, dtype, f)
SHAPES = [(64, 1 << 24, torch.bfloat16, 15)]
RULES = ["median", "trimmed-mean"]
MODES = {"median": 0, "trimmed-mean": 1}


def _aggregate(A, f, rule):
    return D.median(A) if rule == "median" else D.trimmed_mean(A, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="tiny shapes (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_coord_tailored needs a GPU: timings elsewhere mean nothing")
    ext = require()
    dev = torch.device("cuda:0")
    shapes = [(16, 4096, torch.bfloat16, 3)] if args.small else SHAPES
    lines = [
        "| n x d, f | version | ms/call median | min..max | GB/s (one read of X) | calls/batch |",
        "|---|---|---|---|---|---|",
    ]
    notes = []
    for n, d, dtype, f in shapes:
        X = _inputs(n, d, dtype, dev)
        name = "bf16" if dtype == torch.bfloat16 else "f32"
        xbytes = X.numel() * X.element_size()
        mu, p, stats = ext.little_fused(X, 0.0, 1)
        a, c = stats[:n], stats[2 * n]
        g0 = torch.sqrt(a.max() / c)
        gammas = torch.cat(
            [torch.zeros(1, device=dev), g0 * 2.0 ** torch.arange(-15, 16, device=dev)]
        ).float()

        versions = {"stats": lambda: ext.little_fused(X, 0.0, 1)}
        for rule in RULES:
            versions[f"colsel {rule}"] = lambda rule=rule: _aggregate(X, f, rule)
        for rule in RULES:
            versions[f"objective {rule}"] = lambda rule=rule: ext.colsel(
                X, MODES[rule], f, mu=mu, p=p, gammas=gammas
            )
        for rule in RULES:
            versions[f"torch {rule}"] = lambda rule=rule: D._agr_coord_objective_torch(
                X, mu, p, gammas, f, rule
            )
        for rule in RULES:
            versions[f"attack {rule}"] = lambda rule=rule: D.agr_coord(X, f, rule)

        res = measure(versions, args.rounds)
        for k, (med, lo, hi, reps) in res.items():
            lines.append(
                f"| {n} x {d} {name}, f = {f} | {k} | {med:.3f} | {lo:.3f}..{hi:.3f} | "
                f"{xbytes / med / 1e6:.0f} | {reps} |"
            )
        for rule in RULES:
            o, k, t = (res[f"{v} {rule}"][0] for v in ("objective", "colsel", "torch"))
            notes.append(
                f"- {n} x {d} {name}, f = {f}, {rule}: objective pass {o:.3f} ms "
                f"({xbytes / o / 1e6:.0f} GB/s of X) = {o / k:.2f} x the {rule} kernel's "
                f"pass ({k:.3f} ms, {xbytes / k / 1e6:.0f} GB/s); torch composition "
                f"{t:.1f} ms = {t / o:.0f} x the kernel; attack end to end "
                f"{res[f'attack {rule}'][0]:.3f} ms"
            )
            dk = versions[f"objective {rule}"]()
            dt = versions[f"torch {rule}"]()
            rel = ((dk - dt).abs() / dt.abs().clamp_min(1e-300)).max().item()
            notes.append(
                f"- {n} x {d} {name}, {rule}: kernel against torch composition (f64), "
                f"largest relative difference over the 32 trials {rel:.1e}"
            )
        m_other = {"Min-Max": D.min_max(X), "Min-Sum": D.min_sum(X)}
        for rule in RULES:
            m_t = D.agr_coord(X, f, rule)
            dist = {}
            for label, m in [("tailored", m_t)] + list(m_other.items()):
                A = torch.cat([X, m[None, :].expand(f, -1)])
                dist[label] = (_aggregate(A, f, rule).float() - mu).norm().item()
                del A
            clean = (_aggregate(X, f, rule).float() - mu).norm().item()
            notes.append(
                f"- {n} x {d} {name}, f = {f}, {rule}: ||agg - mu|| = "
                + ", ".join(f"{v:.4g} ({k})" for k, v in dist.items())
                + f", {clean:.4g} (no attack)"
            )
        del X, mu, p, stats, m_other, m_t
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n\n" + "\n".join(notes) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
