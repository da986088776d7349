"""K21 on the device: the one-launch CAF solver against F.caf_gram on the same
Gram and seeds, and CAF(solver="gram") end to end against the f64 d-space loop.
Every comparison first asserts ON THE REFERENCE that its input keeps the
filter's discrete decisions away from ties: a failure there blames the input."""
import pytest
import torch

from byzpy_amd import hip
from byzpy_amd.aggregators import CAF
from byzpy_amd.ops import functional as F
from test_caf_gram import dspace_caf

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _assert_separated(n, f, lams, wsums, wnexts):
    """Exempt, being no rounding ties: round 0's wsum (the exact live count, with
    f = 0 the target itself) and sum(w_next) of a round that stops on wsum."""
    lo = sorted(lams)
    assert len(lo) < 2 or lo[0] <= 0.999 * lo[1]  # the minimum is 0.1 % clear
    for r, (ws, wn) in enumerate(zip(wsums, wnexts)):
        assert r == 0 or abs(ws - (n - 2 * f)) > 1e-3
        assert ws <= n - 2 * f or wn > 1e-3


def _gram32(n, case=""):
    g = torch.Generator().manual_seed(100 + n)
    X = torch.randn(n, 256, generator=g, dtype=torch.float64)
    X[: min(2, n - 1)] *= 20.0
    if case == "identical":
        X[3] = X[2]
    if case == "all-identical":
        X[:] = X[0].clone()
    G = (X @ X.T).float()
    if case == "inf":
        G[1, :] = G[:, 1] = float("inf")
    return G


def _solve(G, f, power_iters):
    seeds = F.caf_gram_seeds(G.shape[0]).to(DEV)
    a, lam, rounds = hip.require().caf_matvec(G.to(DEV), seeds, f=f, power_iters=power_iters)
    assert a.dtype == lam.dtype == torch.float32
    return a.cpu(), float(lam), int(rounds)


def _check_solver(G, f, power_iters):
    seeds = F.caf_gram_seeds(G.shape[0])
    a, lam, rounds = _solve(G, f, power_iters)
    ref, rlam, rrounds, *trace = F.caf_gram(G, f, seeds, power_iters=power_iters, trace=True)
    _assert_separated(G.shape[0], f, *trace)
    assert rounds == rrounds
    # 1e-9 of f64 reordering, and the f32 rounding of the output itself
    assert bool(((a.double() - ref).abs() <= 1e-9 + 2.0**-24 * ref.abs()).all())
    assert abs(lam - rlam) <= 1e-6 * rlam
    return a


@pytest.mark.parametrize("power_iters", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 16, 17, 64, 65, 128])
@pytest.mark.parametrize("half", [False, True])
def test_solver_matches_f64_loop_on_the_same_gram(half, n, power_iters):
    _check_solver(_gram32(n), (n - 1) // 2 if half else 0, power_iters)


@pytest.mark.parametrize("case", ["inf", "identical"])
def test_solver_dead_and_identical_rows(case):
    a = _check_solver(_gram32(17, case), 8, 3)
    if case == "inf":
        assert float(a[1]) == 0.0 and bool(torch.isfinite(a).all())
    else:
        assert float(a[2]) == float(a[3])


@pytest.mark.parametrize("scale", [0.0, 1.0])
def test_solver_all_rows_identical(scale):
    """Zero rows: exact arithmetic, all n rounds run, round 0's uniform p wins.
    Identical rows of norm > 0 run on rounding noise that the rule's 1e-20
    clamps scale to order 1 (on MI355X the kernel stops after 1 round,
    F.caf_gram after 2): there a is a convex combination, a @ X is the row."""
    G = _gram32(17, "all-identical") * scale
    a, _, rounds = _solve(G, 8, 3)
    if scale == 0.0:
        assert rounds == 17 == F.caf_gram(G, 8, F.caf_gram_seeds(17))[2]
        assert torch.equal(a, torch.full((17,), 1.0 / 17))
    assert bool((a >= 0).all()) and abs(float(a.double().sum()) - 1.0) <= 17 * 2.0**-24


# -- end to end -----------------------------------------------------------------

D_E2E = 4099
# max|out - ref| / max|ref| allowed on the f32 route: 4 x the largest error the
# f32 MFMA Gram ALONE forces on these inputs, measured on MI355X without the new
# kernel: F.caf_gram in f64 on the device Gram, combined in f64, against the
# d-space f64 loop (benchmarks/RESULTS_MI355X_caf_gram.md, "Accuracy").
E2E_F32_REL = 4 * 7.1e-7
_REFS: dict = {}


def _inputs(n, dtype):
    # iid normal rows, n // 4 shifted along one direction: separated top eigenvalue
    g = torch.Generator().manual_seed(n)
    X = torch.randn(n, D_E2E, generator=g)
    e = torch.randn(D_E2E, generator=g)
    X[: n // 4] += 320.0 * e / e.norm()
    return X.to(dtype)


def _ref(X, n, f, key):
    if key not in _REFS:
        Xd = X.double()
        live = torch.isfinite(Xd).all(dim=1)
        G = torch.where(live[:, None] & live[None, :], Xd @ Xd.T, float("inf"))
        _assert_separated(n, f, *F.caf_gram(G, f, F.caf_gram_seeds(n), trace=True)[3:])
        _REFS[key] = dspace_caf(Xd, f, F.caf_gram_seeds(n), 3)[0]
    return _REFS[key]


def _check_e2e(out, ref, dtype, what):
    assert out.dtype == dtype
    out = out.cpu().double()
    if dtype == torch.float32:
        assert float((out - ref).abs().max() / ref.abs().max()) <= E2E_F32_REL, what
    else:  # one bf16 ulp of the rounded reference
        r = ref.to(dtype).double()
        ulp = torch.ldexp(torch.ones_like(r), torch.frexp(r)[1] - 8)
        assert float(((out - r).abs() / ulp).max()) <= 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n,inf", [(17, False), (64, False), (128, False), (17, True)])
def test_public_class_matches_f64_loop(n, inf, dtype):
    X = _inputs(n, dtype)
    if inf:  # the row is left out
        X[9, 11] = float("inf")
    out = CAF(n // 4, solver="gram").aggregate(X.to(DEV))
    _check_e2e(out, _ref(X, n, n // 4, (n, dtype, inf)), dtype, f"n={n} inf={inf}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_list_input_is_read_in_place(dtype, monkeypatch):
    X = _inputs(33, dtype)
    rows = [r.clone() for r in X.to(DEV)]
    ref = _ref(X, 33, 8, (33, dtype))
    monkeypatch.setattr(torch, "stack", None)  # the route stacks nothing
    _check_e2e(CAF(8, solver="gram").aggregate(rows), ref, dtype, "list n=33")
