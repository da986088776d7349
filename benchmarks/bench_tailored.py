"""Aggregator-tailored attacks on one MI355X: the device grid search against
the same schedule as batched torch ops and against the two passes over X it
rides on, then the attack end to end with Min-Max beside it.

Versions, alternated round by round in one process:
  stats            ext.little_fused(X, 0, 1): mu, p, a, b, c
  gram             D.gram(X): the MFMA Gram
  search <rule>    ext.krum_select(G, f, q, stats=, rule=): three grid
                   launches and a finish on the O(n^2) numbers
  torch <rule>     D._agr_gamma_torch: the same grids as (B, n, n + f) sorts
                   (Krum / Multi-Krum; Bulyan has no torch composition)
  tailored <rule>  D.agr_tailored(X, f, rule): stats + gram + search + addcmul
  min_max          D.min_max(X): stats + gram + closed-form gamma

Every version is warmed up, then timed with device events in batches sized
to >= 0.1 s, `--rounds` batches per version; the table gives the median
batch and the min..max spread, per call. After the timings, one line per
rule gives ||agg(X u m x f) - mu|| for the tailored vector next to the
Min-Max vector on the same input.

Usage: python benchmarks/bench_tailored.py [--out FILE.md] [--rounds 5]
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
SHAPES = [
    (64, 1 << 24, torch.bfloat16, 15),
    (16, 1 << 24, torch.bfloat16, 3),
    (64, 1 << 22, torch.float32, 15),
]
RULES = ["krum", "multi-krum", "bulyan"]


def _aggregate(A, f, n, rule):
    if rule == "krum":
        return D.krum(A, f)
    if rule == "multi-krum":
        return D.multi_krum(A, f, n)
    return D.bulyan(A, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="tiny shapes (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_tailored needs a GPU: timings elsewhere mean nothing")
    ext = require()
    dev = torch.device("cuda:0")
    shapes = [(16, 4096, torch.bfloat16, 3)] if args.small else SHAPES
    lines = [
        "| n x d, f | version | ms/call median | min..max | calls/batch |",
        "|---|---|---|---|---|",
    ]
    notes = []
    for n, d, dtype, f in shapes:
        X = _inputs(n, d, dtype, dev)
        name = "bf16" if dtype == torch.bfloat16 else "f32"
        mu, p, stats = ext.little_fused(X, 0.0, 1)
        a, b, c = stats[:n], stats[n : 2 * n], stats[2 * n]
        G = D.gram(X)
        qs = {"krum": 1, "multi-krum": n, "bulyan": n - f}

        versions = {
            "stats": lambda: ext.little_fused(X, 0.0, 1),
            "gram": lambda: D.gram(X),
        }
        for rule in RULES:
            versions[f"search {rule}"] = lambda rule=rule: ext.krum_select(
                G, f, qs[rule], stats=stats, rule=int(rule == "bulyan")
            )
        for rule in RULES[:2]:
            versions[f"torch {rule}"] = lambda rule=rule: D._agr_gamma_torch(
                G, a, b, c, f, qs[rule]
            )
        for rule in RULES:
            versions[f"tailored {rule}"] = lambda rule=rule: D.agr_tailored(X, f, rule)
        versions["min_max"] = lambda: D.min_max(X)

        res = measure(versions, args.rounds)
        for k, (med, lo, hi, reps) in res.items():
            lines.append(
                f"| {n} x {d} {name}, f = {f} | {k} | {med:.3f} | {lo:.3f}..{hi:.3f} | {reps} |"
            )
        passes = res["stats"][0] + res["gram"][0]
        for rule in RULES:
            s = res[f"search {rule}"][0]
            t = res.get(f"torch {rule}")
            vs_torch = f"torch / search = {t[0] / s:.1f}, " if t else ""
            notes.append(
                f"- {n} x {d} {name}, f = {f}, {rule}: search {s:.3f} ms, {vs_torch}"
                f"search / (stats + gram) = {s / passes:.2f}, end to end "
                f"{res[f'tailored {rule}'][0]:.3f} ms against Min-Max {res['min_max'][0]:.3f} ms"
            )
        # the two searches agree, and what the attack does to each rule
        for rule in RULES[:2]:
            g_dev = float(versions[f"search {rule}"]())
            g_torch = float(versions[f"torch {rule}"]())
            notes.append(
                f"- {n} x {d} {name}, {rule}: gamma {g_dev:.6f} (device), "
                f"{g_torch:.6f} (torch), relative difference "
                f"{abs(g_dev - g_torch) / max(abs(g_torch), 1e-30):.1e}"
            )
        m_mm = D.min_max(X)
        for rule in RULES:
            m_t = D.agr_tailored(X, f, rule)
            dist = {}
            for label, m in (("tailored", m_t), ("min_max", m_mm)):
                A = torch.cat([X, m[None, :].expand(f, -1)])
                dist[label] = (_aggregate(A, f, n, rule).float() - mu).norm().item()
                del A
            clean = (_aggregate(X, f, n - f if rule == "multi-krum" else n, rule).float() - mu).norm().item()
            notes.append(
                f"- {n} x {d} {name}, f = {f}, {rule}: ||agg - mu|| = "
                f"{dist['tailored']:.4g} (tailored), {dist['min_max']:.4g} (Min-Max), "
                f"{clean:.4g} (no attack); ||m - mu|| = {(m_t.float() - mu).norm().item():.4g} "
                f"(tailored), {(m_mm.float() - mu).norm().item():.4g} (Min-Max)"
            )
        del X, G, mu, p, stats, m_mm, m_t
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n\n" + "\n".join(notes) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
