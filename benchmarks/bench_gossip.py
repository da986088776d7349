"""K23: the gossip round on one shared Gram, step by step.

Times, with device events around each step, the Gram of theta, the one-launch
solver for all nodes and the batched combine, at the config-4 shape (ring of
8, k = 2, d = 25,610,152) and the combine alone at larger node counts, and
sets each pass against the bytes it has to move (every read row once, every
output element once).

  python benchmarks/bench_gossip.py [--reps 20] [--quick]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from byzpy_amd import hip
from byzpy_amd.engine.peer_to_peer.topology import Topology
from byzpy_amd.hip import dispatch as D


def timed(fn, reps: int, warmup: int = 3):
    """Median and (min, max) of `reps` device-event timings of fn, in ms."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def ring_coeffs(N: int, m: int, dev) -> torch.Tensor:
    """(N, N) coefficients of a ring whose nodes listen to m rows each."""
    A = torch.zeros(N, N)
    for i in range(N):
        for s in range(m):
            A[i, (i + s - m // 2) % N] = 1.0 / m + 0.001 * s
    return A.to(dev)


def report(name: str, t, nbytes: float) -> None:
    med, lo, hi = t
    print(f"{name}: {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); "
          f"{nbytes / 1e9:.3f} GB -> {nbytes / med / 1e9:.2f} TB/s")


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--quick", action="store_true", help="small shapes (a rehearsal)")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gossip.py measures device kernels: no GPU found")
    dev = torch.device("cuda")
    ext = hip.require()
    g = torch.Generator(device=dev).manual_seed(0)

    # config 4: ring(8, 2), NNM(1) + geometric median, 4 fixed steps
    N, d = 8, 4096 * 5 + 3 if args.quick else 25_610_152
    topo = Topology.ring(N, 2)
    theta = torch.empty(N, d, dtype=torch.bfloat16, device=dev).normal_(generator=g)
    groups = D.gossip_groups([[i] + topo.in_neighbors(i) for i in range(N)], dev)
    G = D.gram(theta)
    A = ext.weiszfeld_iter(G, groups=groups, nnm_f=1, eps=1e-12, tol=0.0, iters=4)[0]
    row = 2.0 * d
    report(f"gram {N} x {d} bf16", timed(lambda: D.gram(theta), args.reps), N * row)
    t = timed(lambda: ext.weiszfeld_iter(
        G, groups=groups, nnm_f=1, eps=1e-12, tol=0.0, iters=4), args.reps)
    print(f"solver {N} nodes, m = 5, NNM, 4 steps: {t[0]:.4f} ms (min {t[1]:.4f}, max {t[2]:.4f})")
    report(f"combine {N} x {N} x {d} bf16",
           timed(lambda: ext.mean_rows(theta, coeffs=A), args.reps), 2 * N * row)
    report("whole round (gram + solver + combine)", timed(
        lambda: D.gossip_geometric_median(theta, groups, nnm_f=1, fixed_iters=4),
        args.reps), 3 * N * row)
    del theta

    # the solver at its caps
    Gb = torch.randn(128, 256, device=dev, generator=g)
    Gb = Gb @ Gb.T
    gb = torch.stack([torch.randperm(128, device=dev)[:32] for _ in range(128)]).int()
    for f in (-1, 8):
        t = timed(lambda: ext.weiszfeld_iter(
            Gb, groups=gb, nnm_f=f, eps=1e-12, tol=0.0, iters=16), args.reps)
        print(f"solver 128 nodes, m = 32, nnm_f = {f}, 16 steps: {t[0]:.4f} ms "
              f"(min {t[1]:.4f}, max {t[2]:.4f})")

    # the combine alone against its HBM bytes: all N rows read, N rows written
    d = 4096 * 9 + 5 if args.quick else 16 * 1024 * 1024
    for N in (64, 128):
        X = torch.empty(N, d, dtype=torch.bfloat16, device=dev).normal_(generator=g)
        for m in (5, 32):
            Ab = ring_coeffs(N, m, dev)
            report(f"combine {N} x {N} (m = {m}) x {d} bf16",
                   timed(lambda: ext.mean_rows(X, coeffs=Ab), args.reps), 2.0 * N * 2 * d)
        del X


if __name__ == "__main__":
    main()
