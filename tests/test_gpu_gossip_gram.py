"""K23 on the device: the one-launch gossip solver, the batched combine on
the matrix pipe, and the gossip round end to end, each against f64."""
import pytest
import torch

from byzpy_amd import hip
from byzpy_amd.aggregators import GeometricMedian
from byzpy_amd.engine.peer_to_peer import Topology, gossip_round
from byzpy_amd.hip import dispatch as D
from byzpy_amd.ops import functional as F
from byzpy_amd.pre_aggregators import NearestNeighborMixing

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-12
MANT = {torch.float32: 24, torch.bfloat16: 8}


def _ulp(r, dtype):
    """The spacing of dtype at the f64 values r (normal range)."""
    return torch.ldexp(torch.ones_like(r), torch.frexp(r)[1] - MANT[dtype])


# -- 1. solver alone ----------------------------------------------------------


def solver_inputs(M, m, n, case=""):
    """f32 Gram of random rows plus two far outliers, and M neighbourhoods of
    m distinct rows each. No row of a neighbourhood has two equal neighbour
    distances (asserted in f64), so the tie-break decides nothing."""
    g = torch.Generator().manual_seed(1000 * M + 10 * m + n)
    X = torch.randn(n, 256, generator=g, dtype=torch.float64)
    X[: min(2, n - 1)] *= 20.0
    G = (X @ X.T).float()
    groups = torch.stack([torch.randperm(n, generator=g)[:m] for _ in range(M)])
    groups = groups.to(torch.int32)
    if case == "pad":
        groups[::2, -1] = -1
        groups[1, -3:] = -1
    if case == "inf":
        G[1, :] = G[:, 1] = float("inf")
    Gd = G.double()
    for r in groups.tolist():
        r = [j for j in r if j >= 0 and bool(torch.isfinite(Gd[j, j]))]
        S = Gd[r][:, r]
        D2 = torch.diagonal(S)[:, None] + torch.diagonal(S)[None, :] - 2.0 * S
        assert all(len(set(row)) == len(row) for row in D2.tolist())
    return G, groups


def _check_solver(G, groups, f, iters, tol=0.0):
    A, steps = hip.require().weiszfeld_iter(
        G.to(DEV), groups=groups.to(DEV), nnm_f=-1 if f is None else f,
        eps=EPS, tol=tol, iters=iters,
    )
    ref, rsteps = F.gossip_coeffs(G, groups, f, iters=iters, eps=EPS, tol=tol)
    assert A.dtype == torch.float32 and A.shape == ref.shape
    # 1e-9 of f64 reordering, and the f32 rounding of the output itself
    err = (A.cpu().double() - ref).abs()
    print(f"solver {tuple(groups.shape)} n={G.shape[0]} f={f} iters={iters}: "
          f"max err {float(err.max()):.3e}")
    assert bool((err <= 1e-9 + 2.0**-24 * ref.abs()).all())
    assert torch.equal(steps.cpu().long(), rsteps)
    return A.cpu(), rsteps


@pytest.mark.parametrize("iters", [1, 3, 50])
@pytest.mark.parametrize("f", [None, 1])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 2, 2), (3, 5, 7), (8, 5, 8), (128, 32, 128)])
def test_solver_matches_f64_composition_on_the_same_gram(shape, f, iters):
    if f is not None and shape[1] - f < 1:
        pytest.skip("NNM needs m - f >= 1")
    _check_solver(*solver_inputs(*shape), f, iters)


@pytest.mark.parametrize("f", [None, 1])
@pytest.mark.parametrize("case", ["pad", "inf"])
def test_solver_padded_and_dead_rows(case, f):
    G, groups = solver_inputs(8, 5, 8, case)
    A, _ = _check_solver(G, groups, f, 3)
    assert bool(torch.isfinite(A).all())
    if case == "inf":
        assert bool((A[:, 1] == 0).all())


def test_solver_stops_each_node_at_the_reference_step():
    """tol lies a factor 3 below node 0's first shift: Weiszfeld converges
    linearly, so that node stops after its first step and before the last."""
    G, groups = solver_inputs(8, 5, 8)
    one = F.gossip_coeffs(G, groups[:1], None, iters=1, eps=EPS)[0][0]
    a0 = torch.zeros(8, dtype=torch.float64)
    a0[groups[0].long()] = 0.2
    shift = float((one - a0) @ G.double() @ (one - a0)) ** 0.5
    _, rsteps = _check_solver(G, groups, None, 50, tol=shift / 3.0)
    assert 1 < int(rsteps[0]) < 50


# -- 2. combine alone -----------------------------------------------------------


def _combine_bound(A, X, ref, dtype):
    """c 2^-24 sum_i |a_i x_i| + 0.5 ulp(out), c = 2 K, K the products summed
    per output: 3 per read row for bf16 (three exact parts), 1 for f32."""
    keep = (A != 0).any(dim=0)
    K = int(keep.sum()) * (3 if dtype == torch.bfloat16 else 1)
    mass = A[:, keep].double().abs() @ X[keep].double().abs()
    return 2 * K * 2.0**-24 * mass + 0.5 * _ulp(ref, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d", [1, 7, 4099])
@pytest.mark.parametrize("M", [1, 8, 17, 128])
@pytest.mark.parametrize("n", [1, 8, 17, 128])
def test_batched_combine_matches_f64(n, M, d, dtype):
    g = torch.Generator().manual_seed(1000 * n + 10 * M + d)
    X = torch.randn(n, d, generator=g).to(dtype)
    A = torch.randn(M, n, generator=g)
    A[torch.rand(M, n, generator=g) < 0.3] = 0.0
    if n > 1:
        A[:, n // 2] = 0.0
        X[n // 2] = float("inf")  # under an all-zero column: never read
    keep = (A != 0).any(dim=0)
    ref = A[:, keep].double() @ X[keep].double()
    ext = hip.require()
    out = ext.mean_rows(X.to(DEV), coeffs=A.to(DEV))
    again = ext.mean_rows(X.to(DEV), coeffs=A.to(DEV))
    assert out.dtype == dtype and out.shape == (M, d)
    assert torch.equal(out, again)
    assert bool(torch.isfinite(out).all())
    err = (out.cpu().double() - ref).abs()
    bound = _combine_bound(A, X, ref, dtype)
    print(f"combine n={n} M={M} d={d} {dtype}: max err/bound "
          f"{float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


# -- 3. end to end -------------------------------------------------------------


@pytest.mark.parametrize("f", [None, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gossip_round_end_to_end(dtype, f, monkeypatch):
    topo = Topology.ring(8, 2)
    g = torch.Generator().manual_seed(7)
    theta = torch.randn(8, 4099, generator=g).to(dtype)
    theta[3] = float("inf")  # a Byzantine state: coefficient 0 everywhere
    rows = [[i] + topo.in_neighbors(i) for i in range(8)]
    groups = D.gossip_groups(rows)
    td = theta.to(DEV)
    Gd = D.solver_gram(td)
    # the Gram kernel adds its partials with atomics: every route below gets
    # this one Gram, so that A is the matrix the rounds combine with
    monkeypatch.setattr(D, "solver_gram", lambda X, centered=False: Gd)
    A = D.gossip_coeffs(Gd, groups.to(DEV), f, iters=4, eps=EPS)[0].cpu()
    Aref = F.gossip_coeffs(Gd.cpu(), groups, f, iters=4, eps=EPS)[0]
    keep = torch.arange(8) != 3
    assert bool((A[:, 3] == 0).all()) and bool((Aref[:, 3] == 0).all())
    Xk = theta[keep].double()
    ref = Aref[:, keep] @ Xk
    bound = _combine_bound(A, theta, ref, dtype) + (A.double() - Aref)[:, keep].abs() @ Xk.abs()
    agg = GeometricMedian(solver="gram", init="mean", fixed_iters=4, eps=EPS)
    pre = None if f is None else NearestNeighborMixing(f)
    direct = D.gossip_geometric_median(td, groups.to(DEV), nnm_f=f, fixed_iters=4, eps=EPS)
    for out in (direct, gossip_round(td, topo, agg, pre)):
        assert out.dtype == dtype and out.shape == (8, 4099)
        err = (out.cpu().double() - ref).abs()
        print(f"round {dtype} f={f}: max err/bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
