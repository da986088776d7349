"""K20 on the device: the one-launch solver on the Gram, the coefficient
combine, and solver="gram" end to end, each against an f64 reference."""
import pytest
import torch

from byzpy_amd import hip
from byzpy_amd.aggregators import CenteredClipping, GeometricMedian
from byzpy_amd.aggregators.pre_aggregated import PreAggregated
from byzpy_amd.ops import functional as F
from byzpy_amd.pre_aggregators import NearestNeighborMixing

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-12
MANT = {torch.float32: 24, torch.bfloat16: 8}


def _ulp(r, dtype):
    """The spacing of dtype at the f64 values r (normal range)."""
    return torch.ldexp(torch.ones_like(r), torch.frexp(r)[1] - MANT[dtype])


def _gram32(n, case=""):
    """f64 Gram of random rows plus two far outliers, cast to f32."""
    g = torch.Generator().manual_seed(100 + n)
    X = torch.randn(n, 256, generator=g, dtype=torch.float64)
    X[: min(2, n - 1)] *= 20.0
    if case == "identical" and n > 3:
        X[3] = X[2]
    G = (X @ X.T).float()
    if case == "inf" and n > 1:
        G[1, :] = G[:, 1] = float("inf")
    return G


# -- 1. solver alone ----------------------------------------------------------


def _check_solver(G, rule, iters, tol=0.0):
    n = G.shape[0]
    a0 = torch.full((n,), 1.0 / n)
    ext = hip.require()
    Gd, a0d = G.to(DEV), a0.to(DEV)
    if rule == "weiszfeld":
        a, steps, shift2 = ext.weiszfeld_iter(Gd, a0d, eps=EPS, tol=tol, iters=iters)
    else:
        a = ext.cc_iter(Gd, a0d, c_tau=30.0, eps=EPS, iters=iters)
    ref, rsteps, rshift2 = F.gram_fixed_point(
        G, a0, rule=rule, iters=iters, eps=EPS, tol=tol, c_tau=30.0
    )
    assert a.dtype == torch.float32
    # 1e-9 of f64 reordering, and the f32 rounding of the output itself
    err = (a.cpu().double() - ref).abs()
    print(f"solver n={n} {rule} iters={iters}: max err {float(err.max()):.3e}")
    assert bool((err <= 1e-9 + 2.0**-24 * ref.abs()).all())
    if rule == "weiszfeld":
        assert int(steps) == rsteps
        if iters <= 3:  # past convergence shift2 is rounding noise
            assert abs(float(shift2) - float(rshift2)) <= 1e-6 * float(rshift2)
    return a.cpu(), ref


@pytest.mark.parametrize("iters", [1, 3, 50])
@pytest.mark.parametrize("rule", ["weiszfeld", "cc"])
@pytest.mark.parametrize("n", [1, 2, 16, 17, 64, 65, 128])
def test_solver_matches_f64_loop_on_the_same_gram(n, rule, iters):
    _check_solver(_gram32(n), rule, iters)


@pytest.mark.parametrize("rule", ["weiszfeld", "cc"])
@pytest.mark.parametrize("case", ["inf", "identical"])
def test_solver_dead_and_identical_rows(case, rule):
    a, _ = _check_solver(_gram32(17, case), rule, 3)
    if case == "inf":
        assert float(a[1]) == 0.0 and bool(torch.isfinite(a).all())
    else:
        assert float(a[2]) == float(a[3])


def test_solver_stops_on_tol_at_the_reference_step():
    """Weiszfeld converges linearly, so successive shifts lie a fixed factor
    apart; at n = 128 the first two lie a factor 120 apart, and tol is put a
    factor 10 below the first: the 2nd step is the one that stops."""
    G = _gram32(128)
    a0 = torch.full((128,), 1.0 / 128)
    shifts = [
        float(F.gram_fixed_point(G, a0, rule="weiszfeld", iters=k, eps=EPS)[2]) ** 0.5
        for k in (1, 2)
    ]
    assert shifts[1] * 100.0 <= shifts[0]
    _, steps, _ = hip.require().weiszfeld_iter(
        G.to(DEV), a0.to(DEV), eps=EPS, tol=shifts[0] / 10.0, iters=50
    )
    assert int(steps) == 2
    _check_solver(G, "weiszfeld", 50, tol=shifts[0] / 10.0)


# -- 2. combine alone -----------------------------------------------------------


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [1, 33, 128])
@pytest.mark.parametrize("d", [1, 7, 4099])
def test_combine_matches_f64(d, n, dtype):
    g = torch.Generator().manual_seed(d + n)
    X = torch.randn(n, d, generator=g).to(dtype)
    a = torch.randn(n, generator=g)
    a[2::5] = 0.0
    if n > 2:
        X[2] = float("inf")  # under a zero coefficient: never read
    out = hip.require().mean_rows(X.to(DEV), coeffs=a.to(DEV)).cpu()
    assert out.dtype == dtype and bool(torch.isfinite(out).all())
    keep = a != 0
    terms = a[keep].double()[:, None] * X[keep].double()
    ref = terms.sum(dim=0)
    bound = n * 2.0**-24 * terms.abs().sum(dim=0) + 0.5 * _ulp(ref, dtype)
    assert bool(((out.double() - ref).abs() <= bound).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_combine_list_equals_stacked_bitwise(dtype):
    n, d = 33, 4099
    g = torch.Generator().manual_seed(7)
    X = torch.randn(n, d, generator=g).to(dtype).to(DEV)
    a = torch.randn(n, generator=g).to(DEV)
    a[4] = 0.0
    rows = [X[i].clone() for i in range(n)]
    # row 5 starts one element past a 16-byte boundary
    buf = torch.empty(d + 8, dtype=dtype, device=DEV)
    buf[1 : d + 1] = X[5]
    rows[5] = buf[1 : d + 1]
    assert rows[5].data_ptr() % 16 == X.element_size()
    ext = hip.require()
    assert torch.equal(ext.mean_rows(rows, coeffs=a), ext.mean_rows(X, coeffs=a))


# -- 3. end to end --------------------------------------------------------------

D_E2E, C_TAU = 4099, 40.0
# Relative error max|out - ref| / max|ref| allowed on the f32 route: 4 x the
# largest error the ITERATIVE device route shows against the same f64
# references on the same inputs (benchmarks/RESULTS_MI355X_gramfp.md,
# "Accuracy"); the gram route's only extra error source is the cancellation
# in G_ii - 2 u_i + q.
E2E_F32_REL = 4 * 3.9e-7


def _inputs(n, dtype):
    """iid standard normal rows plus a few scaled outliers: every row lies at
    a distance comparable to its norm from the fixed point."""
    g = torch.Generator().manual_seed(n)
    X = torch.randn(n, D_E2E, generator=g)
    X[: max(1, n // 8)] *= 4.0
    return X.to(dtype)


def _ref64(Xd, rule, init, steps, tol=0.0):
    """The plain f64 loop on the exact input values."""
    live = torch.isfinite(Xd).all(dim=1)
    Xd = Xd[live]
    z = {"mean": Xd.mean(dim=0), "median": Xd.quantile(0.5, dim=0),
         "zero": torch.zeros_like(Xd[0])}[init]
    for _ in range(steps):
        dist = (Xd - z).norm(dim=1).clamp(min=EPS)
        if rule == "gm":
            w = 1.0 / dist
            z_new = (w[:, None] * Xd).sum(dim=0) / w.sum()
        else:
            c = (C_TAU / dist).clamp(max=1.0)
            z_new = z + (c[:, None] * (Xd - z)).sum(dim=0) / live.numel()
        shift = (z_new - z).norm()
        z = z_new
        if tol > 0.0 and shift <= tol:
            break
    return z


def _check_e2e(out, ref, dtype, what):
    assert out.dtype == dtype
    out = out.cpu().double()
    if dtype == torch.float32:
        rel = float((out - ref).abs().max() / ref.abs().max())
        print(f"e2e {what}: rel err {rel:.3e}")
        assert rel <= E2E_F32_REL
    else:  # one bf16 ulp of the rounded reference
        r = ref.to(dtype).double()
        ulps = float(((out - r).abs() / _ulp(r, dtype)).max())
        print(f"e2e {what}: {ulps:.2f} bf16 ulp")
        assert ulps <= 1.0


E2E_CASES = {
    "gm-mean": ("gm", dict(init="mean", tol=1e-6, max_iter=64), 64),
    "gm-median": ("gm", dict(init="median", fixed_iters=6), 6),
    "gm-fixed": ("gm", dict(init="mean", fixed_iters=3), 3),
    "cc-mean": ("cc", dict(init="mean", M=5), 5),
    "cc-zero": ("cc", dict(init="zero", M=5), 5),
}


def _make(rule, kw, solver="gram"):
    if rule == "gm":
        return GeometricMedian(eps=EPS, solver=solver, **kw)
    return CenteredClipping(c_tau=C_TAU, eps=EPS, solver=solver, **kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [17, 64, 128])
@pytest.mark.parametrize("case", sorted(E2E_CASES))
def test_public_classes_match_f64_loop(case, n, dtype):
    rule, kw, steps = E2E_CASES[case]
    X = _inputs(n, dtype)
    out = _make(rule, kw).aggregate(X.to(DEV))
    ref = _ref64(X.double(), rule, kw["init"], steps, kw.get("tol", 0.0))
    _check_e2e(out, ref, dtype, f"{case} n={n}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_list_input_is_read_in_place(dtype, monkeypatch):
    X = _inputs(33, dtype)
    rows = [r.clone() for r in X.to(DEV)]
    monkeypatch.setattr(torch, "stack", None)  # the route stacks nothing
    out = GeometricMedian(eps=EPS, solver="gram", init="mean", fixed_iters=4).aggregate(rows)
    _check_e2e(out, _ref64(X.double(), "gm", "mean", 4), dtype, "list n=33")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_nnm_in_front_runs_on_the_mixed_gram(dtype):
    n, f = 17, 4
    X = _inputs(n, dtype)
    Xd = X.double()
    near = torch.cdist(Xd, Xd).topk(n - f, dim=1, largest=False).indices
    Y = Xd[near].mean(dim=1)
    agg = PreAggregated(
        NearestNeighborMixing(f),
        GeometricMedian(eps=EPS, solver="gram", init="mean", fixed_iters=4),
    )
    _check_e2e(agg.aggregate(X.to(DEV)), _ref64(Y, "gm", "mean", 4), dtype, "nnm")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_inf_row_is_left_out(dtype):
    X = _inputs(17, dtype)
    # row 9: without it no coordinate of the fixed point lies within 1e-4 of
    # max |z| of zero (checked in f64). Closer than ~2^-16 the f32 accumulation
    # noise of any route exceeds a bf16 ulp of that coordinate.
    X[9, 11] = float("inf")
    out = GeometricMedian(eps=EPS, solver="gram", init="mean", fixed_iters=4).aggregate(X.to(DEV))
    _check_e2e(out, _ref64(X.double(), "gm", "mean", 4), dtype, "inf row")
