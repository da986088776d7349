"""Tailored attacks on the coordinate-wise rules, on the GPU: the one-pass
objective kernel behind colsel(X, mode, f, mu=, p=, gammas=) against the
functional oracle (bitwise on an exact-arithmetic family, to a measured f32
tolerance on random and skewed data), the whole search, repeatability, the
binding's rejections, the dispatch past the kernel's row cap, the operator
class and hipGraph capture."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from byzpy_amd.attacks import CoordinateTailoredAttack
from byzpy_amd.hip import dispatch as D
from byzpy_amd.hip import require
from byzpy_amd.hip.graphs import CapturedAggregate
from byzpy_amd.ops import functional as F

DTYPES = [torch.float32, torch.bfloat16]
DTYPE_IDS = ["f32", "bf16"]
RULES = ["trimmed-mean", "median"]
MODES = {"median": 0, "trimmed-mean": 1}

SHAPE_N = [1, 2, 9, 23, 33, 47, 64]
SHAPE_D = [1, 33, 257, 2050]
TRIALS = [1, 7, 32]
EXACT_NF = [(9, 1), (20, 4), (23, 7), (47, 15), (64, 32)]
# the launcher caps its grid at 1024 blocks of 256 columns: past this d a
# block takes a second strip
STRIP_D = 1024 * 256 + 513


@pytest.fixture(scope="module")
def ext():
    return require()


def _tol(dtype):  # as in test_gpu_kernels.py
    return dict(atol=1e-4, rtol=1e-4) if dtype == torch.float32 else dict(atol=5e-2, rtol=5e-2)


@pytest.fixture(scope="module", autouse=True)
def _one_torch_thread():
    """The oracle is many small CPU ops in Python loops: intra-op threads only
    add wake-ups to them."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


def _fs(n, agr):
    fs = {1, n // 4, n // 2, n - 1}
    if agr == "median":
        fs.add(n + 3)
    return sorted(f for f in fs if f >= 1 and (agr == "median" or f < n))


def _bits(t):
    return t.contiguous().view(torch.int64)


@functools.lru_cache(maxsize=None)
def _exact_case(n, d):
    """As test_coord_tailored._exact_case: integers in [-4, 4], mu multiples
    of 1/16, p in {-1, 0, 1}, gammas k / 4. All of it is exact in bf16 too."""
    g = torch.Generator().manual_seed(7 * n + 1)
    X = torch.randint(-4, 5, (n, d), generator=g).float()
    mu = torch.randint(-64, 65, (d,), generator=g).float() / 16
    p = torch.randint(-1, 2, (d,), generator=g).float()
    gammas = torch.arange(32).float() / 4
    return X, mu, p, gammas


def _oracle(H, mu, p, gammas, f, agr, dtype=torch.float64):
    return torch.tensor(
        [F.agr_coord_objective(H, float(g), f, agr, mu=mu, p=p, dtype=dtype) for g in gammas],
        dtype=torch.float64,
    )


@pytest.mark.parametrize("agr", RULES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n,f", EXACT_NF)
def test_exact_family_is_bitwise(ext, n, f, dtype, agr):
    X, mu, p, gammas = _exact_case(n, 2050)
    ref = _oracle(X, mu, p, gammas, f, agr)
    got = ext.colsel(
        X.to("cuda", dtype), MODES[agr], f, mu=mu.cuda(), p=p.cuda(), gammas=gammas.cuda()
    )
    assert got.dtype == torch.float64 and got.shape == (32,) and got.is_cuda
    assert torch.equal(_bits(got.cpu()), _bits(ref))
    # and through the dispatch, with fewer trials than the kernel runs
    few = D.agr_coord_objective(X.to("cuda", dtype), mu.cuda(), p.cuda(), gammas[3:10].cuda(), f, agr)
    assert torch.equal(_bits(few.cpu()), _bits(ref[3:10]))


@pytest.mark.parametrize("agr", RULES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_exact_family_second_strip_is_bitwise(ext, dtype, agr):
    """d past the grid cap: every block walks a second strip of columns, the
    last one partly filled."""
    X, mu, p, gammas = _exact_case(9, STRIP_D)
    gammas = gammas[::5]  # 7 trials
    ref = _oracle(X, mu, p, gammas, 1, agr)
    got = ext.colsel(
        X.to("cuda", dtype), MODES[agr], 1, mu=mu.cuda(), p=p.cuda(), gammas=gammas.cuda()
    )
    assert torch.equal(_bits(got.cpu()), _bits(ref))


@functools.lru_cache(maxsize=None)
def _random_case(n, d, dtype, kind="randn"):
    """The device matrix, the f32 CPU view of exactly the values it holds, and
    the kernel's own statistics on the CPU."""
    g = torch.Generator().manual_seed(100 * n + d)
    if kind == "randn":
        X = torch.randn(n, d, generator=g) * (1 + 0.1 * torch.arange(n))[:, None] + 0.3
    else:  # skewed: lognormal
        X = torch.exp(torch.randn(n, d, generator=g))
    X = X.to("cuda", dtype).contiguous()
    mu, p, a, _, c = D.attack_stats(X, "std")
    return X, X.float().cpu(), mu, p, a, c


def _trial_gammas(a, c, T):
    """T points of the schedule's round 0 around the anchor."""
    g0 = float(torch.sqrt(a.max() / c)) if float(c) > 0 else 1.0
    pts = [0.0] + [g0 * 2.0**k for k in range(-15, 16)]
    pick = {1: [16], 7: [0, 10, 13, 15, 16, 18, 25], 32: list(range(32))}[T]
    return torch.tensor([pts[i] for i in pick], dtype=torch.float32)


def _check_against_oracle(ext, X, H, mu, p, gammas, f, agr, label):
    """The kernel's D against the oracle's f64 D on the kernel's own f32 mu
    and p. Tolerance per trial: 16 x the relative discrepancy between the
    oracle's own f32 and f64 evaluations, floored at (n + f) 2^-23."""
    n = H.shape[0]
    got = ext.colsel(X, MODES[agr], f, mu=mu, p=p, gammas=gammas.cuda()).cpu()
    mu_c, p_c = mu.cpu(), p.cpu()
    ref = _oracle(H, mu_c, p_c, gammas, f, agr)
    ref32 = _oracle(H, mu_c, p_c, gammas, f, agr, dtype=torch.float32)
    scale = ref.abs().clamp_min(1e-300)
    own = (ref32 - ref).abs() / scale
    tol = torch.maximum(16.0 * own, torch.full_like(own, (n + f) * 2.0**-23))
    err = (got - ref).abs() / scale
    exact_zero = (ref == 0) & (got == 0)
    err = torch.where(exact_zero, torch.zeros_like(err), err)
    print(
        f"{label}: kernel rel err max {err.max():.3e}, oracle f32-vs-f64 max "
        f"{own.max():.3e}, tol min {tol.min():.3e}"
    )
    assert bool((err <= tol).all()), (label, err, tol)
    return float(tol.max())


@pytest.mark.parametrize("agr", RULES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n", SHAPE_N)
def test_shapes_match_oracle(ext, n, dtype, agr):
    for d in SHAPE_D:
        X, H, mu, p, a, c = _random_case(n, d, dtype)
        for f in _fs(n, agr):
            for T in TRIALS:
                _check_against_oracle(
                    ext, X, H, mu, p, _trial_gammas(a, c, T), f, agr,
                    f"{agr} n={n} f={f} d={d} T={T} {dtype}",
                )


@pytest.mark.parametrize("agr", RULES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n,f,d", [(64, 15, 4099), (23, 7, 2050)])
def test_skewed_data_matches_oracle(ext, n, f, d, dtype, agr):
    X, H, mu, p, a, c = _random_case(n, d, dtype, "lognormal")
    _check_against_oracle(
        ext, X, H, mu, p, _trial_gammas(a, c, 32), f, agr,
        f"lognormal {agr} n={n} f={f} d={d} {dtype}",
    )


@pytest.mark.parametrize("agr", RULES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_second_strip_matches_oracle(ext, dtype, agr):
    X, H, mu, p, a, c = _random_case(9, STRIP_D, dtype)
    _check_against_oracle(
        ext, X, H, mu, p, _trial_gammas(a, c, 7), 2, agr, f"strip {agr} {dtype}"
    )


@pytest.mark.parametrize("agr", RULES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize(
    "n,f,d,kind,perturbation",
    [
        (23, 7, 2050, "randn", "std"),
        (9, 2, 257, "randn", "unit"),
        (33, 8, 300, "randn", "sign"),
        (23, 7, 2050, "lognormal", "std"),
    ],
)
def test_whole_attack(n, f, d, kind, perturbation, dtype, agr):
    """The device's gamma does as well as the oracle's on the oracle's own
    objective (both searches on the kernel's mu and p), and the vector is
    mu + gamma p in the input dtype."""
    X, H = _random_case(n, d, dtype, kind)[:2]
    mu, p, a, _, c = D.attack_stats(X, perturbation)
    gamma = D.agr_coord_gamma(X, mu, p, a, c, f, agr)
    assert gamma.dim() == 0 and gamma.is_cuda
    mu_c, p_c = mu.cpu(), p.cpu()
    # the oracle's search from the device's own anchor, so that both walk
    # the same grid and only the objective's arithmetic differs
    g0 = float(torch.sqrt(a.double().max() / c.double()).float())
    g_ref = F.agr_coord_gamma(H, f, agr, gamma0=g0, mu=mu_c, p=p_c)
    one = torch.tensor([g_ref])
    d_ref = float(_oracle(H, mu_c, p_c, one, f, agr))
    d_ref32 = float(_oracle(H, mu_c, p_c, one, f, agr, dtype=torch.float32))
    tol = max(16.0 * abs(d_ref32 - d_ref) / d_ref, (n + f) * 2.0**-23)
    d_dev = float(_oracle(H, mu_c, p_c, gamma.cpu().reshape(1), f, agr))
    print(
        f"{agr} {kind} {perturbation} n={n} f={f} d={d} {dtype}: gamma {float(gamma):.6f} "
        f"vs {g_ref:.6f}, D {d_dev:.9e} vs {d_ref:.9e}, tol {tol:.2e}"
    )
    assert d_ref > 0.0
    assert d_dev >= d_ref * (1.0 - 2.0 * tol)
    out = D.agr_coord(X, f, agr, perturbation)
    assert out.dtype == dtype and out.device == X.device and out.shape == (d,)
    want = torch.addcmul(mu, gamma.to(mu.dtype), p).to(dtype)
    # the statistics pass adds with float atomics: two calls agree to the
    # search resolution and the output rounding, not to the bit
    assert torch.allclose(out.float(), want.float(), **_tol(dtype))


@pytest.mark.parametrize("agr", RULES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n,f,d", [(23, 7, 2050), (64, 15, 4099), (9, 2, STRIP_D)])
def test_same_inputs_give_the_same_bits(ext, n, f, d, dtype, agr):
    X, _, mu, p, a, c = _random_case(n, d, dtype)
    gammas = _trial_gammas(a, c, 32).cuda()
    runs = [ext.colsel(X, MODES[agr], f, mu=mu, p=p, gammas=gammas) for _ in range(3)]
    assert bool(torch.isfinite(runs[0]).all()) and float(runs[0].max()) > 0.0
    assert torch.equal(_bits(runs[0]), _bits(runs[1]))
    assert torch.equal(_bits(runs[0]), _bits(runs[2]))


def test_non_finite_inputs_do_not_fault(ext):
    X, _, mu, p, a, c = _random_case(23, 2050, torch.float32)
    gammas = _trial_gammas(a, c, 7).cuda()
    Xb = X.clone()
    Xb[3, 17] = float("inf")
    Xb[5, 900] = float("nan")
    Xb[7, 2049] = -float("inf")
    mub = mu.clone()
    mub[40] = float("nan")
    pb = p.clone()
    pb[41] = float("inf")
    for agr in RULES:
        out = ext.colsel(Xb, MODES[agr], 7, mu=mu, p=p, gammas=gammas)
        torch.cuda.synchronize()
        assert out.shape == (7,)
        out = ext.colsel(X, MODES[agr], 7, mu=mub, p=p, gammas=gammas)
        assert not bool(torch.isfinite(out).any())
        # an infinite p only makes v infinite, which both rules survive
        out = ext.colsel(X, MODES[agr], 7, mu=mu, p=pb, gammas=gammas)
        torch.cuda.synchronize()
        assert out.shape == (7,)
        nan_gamma = torch.tensor([0.0, float("nan")], device="cuda")
        out = ext.colsel(X, MODES[agr], 7, mu=mu, p=p, gammas=nan_gamma).cpu()
        assert bool(torch.isfinite(out[0]))
    # statistics that are not finite: gamma = 0, on the device too
    bad = a.clone()
    bad[2] = float("nan")
    assert float(D.agr_coord_gamma(X, mu, p, bad, c, 7, "median")) == 0.0
    assert float(D.agr_coord_gamma(X, mu, p, a, c * 0.0, 7, "trimmed-mean")) == 0.0


def _nonfinite_columns(n, f):
    """One-column problems (so that one bad column cannot hide the others)
    around values that are not finite or leave the f32 range: (label, X
    (n, 1), mu (1,), p (1,)), f32, and the trial gammas."""
    g = torch.Generator().manual_seed(31 * n + f)
    base = torch.randn(n, generator=g) + 0.3
    inf, nan = float("inf"), float("nan")

    def col(label, edits=(), p=-0.7, mu=None):
        x = base.clone()
        for i, val in edits:
            x[i] = val
        m = float(base.double().mean()) if mu is None else mu
        return label, x[:, None].contiguous(), torch.tensor([m]), torch.tensor([p])

    cols = [
        col("clean"),
        col("x +inf", [(0, inf)]),
        col("x -inf", [(1, -inf)]),
        col("x nan", [(2, nan)]),
        col("x f+1 +inf", [(i, inf) for i in range(f + 1)]),
        col("x f+1 -inf", [(i, -inf) for i in range(f + 1)]),
        col("x nan and +inf", [(0, inf), (1, nan)]),
        col("p -inf", p=-inf),
        col("p +inf", p=inf),
        col("p 1e30", p=1e30),
        col("p -1e30", p=-1e30),
        col("x -inf, p -inf", [(3, -inf)], p=-inf),
        col("x nan, p +inf", [(3, nan)], p=inf),
        col("mu nan", mu=nan),
        col("mu inf", mu=inf),
    ]
    gammas = torch.tensor([0.0, 0.5, 2.0, 1e30, nan])
    return cols, gammas


@pytest.mark.parametrize("agr", RULES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n,f", [(23, 7), (23, 8), (10, 9), (47, 23)])
def test_non_finite_values_rank_as_in_the_oracle(ext, n, f, dtype, agr):
    """The kernel against the oracle column by column, with min(f, n - f)
    below the kernel's tail width (7 of 8, 1 of 4, 23 of 32) and equal to it
    (8): D is finite in exactly the oracle's trials (a NaN ranks above +inf,
    as torch.sort has it; a dropped extreme does no harm, a kept one does; an
    f64 v outside the f32 range is an extreme, not an infinity), and within
    the random-data tolerance of it where finite."""
    cols, gammas = _nonfinite_columns(n, f)
    seen = set()
    for label, X, mu, p in cols:
        Xd = X.to("cuda", dtype)
        H = Xd.float().cpu()
        got = ext.colsel(Xd, MODES[agr], f, mu=mu.cuda(), p=p.cuda(), gammas=gammas.cuda()).cpu()
        ref = _oracle(H, mu, p, gammas, f, agr)
        ref32 = _oracle(H, mu, p, gammas, f, agr, dtype=torch.float32)
        fin = torch.isfinite(ref)
        assert torch.equal(torch.isfinite(got), fin), (label, got, ref)
        both = fin & torch.isfinite(ref32)
        scale = ref.abs().clamp_min(1e-300)
        own = torch.where(both, (ref32 - ref).abs() / scale, torch.zeros_like(ref))
        tol = torch.maximum(16.0 * own, torch.full_like(own, (n + f) * 2.0**-23))
        err = (got - ref).abs() / scale
        assert bool((err[fin] <= tol[fin]).all()), (label, got, ref, tol)
        seen.update(fin.tolist())
    assert seen == {True, False}


def test_rejections(ext):
    X, _, mu, p, a, c = _random_case(23, 2050, torch.float32)
    g = torch.ones(4, device="cuda")
    X65 = torch.zeros(65, 2050, device="cuda")
    for bad in (
        lambda: ext.colsel(X.cpu(), 1, 7, mu=mu.cpu(), p=p.cpu(), gammas=g.cpu()),
        lambda: ext.colsel(X, 1, 7, mu=mu.cpu(), p=p, gammas=g),
        lambda: ext.colsel(X, 1, 7, mu=mu, p=p.cpu(), gammas=g),
        lambda: ext.colsel(X, 1, 7, mu=mu, p=p, gammas=g.cpu()),
        lambda: ext.colsel(X, 2, 7, mu=mu, p=p, gammas=g),            # mode 2
        lambda: ext.colsel(X, -1, 7, mu=mu, p=p, gammas=g),
        lambda: ext.colsel(X65, 0, 7, mu=mu, p=p, gammas=g),          # n > 64
        lambda: ext.colsel(X, 0, 7, mu=mu, p=p, gammas=torch.ones(33, device="cuda")),
        lambda: ext.colsel(X, 0, 7, mu=mu, p=p, gammas=g[:0]),
        lambda: ext.colsel(X, 0, 7, mu=mu[:-1], p=p, gammas=g),
        lambda: ext.colsel(X, 0, 7, mu=mu, p=p[:-1], gammas=g),
        lambda: ext.colsel(X, 0, 7, mu=mu.reshape(2, -1), p=p, gammas=g),
        lambda: ext.colsel(X, 0, 7, mu=mu, p=p, gammas=g.reshape(2, 2)),
        lambda: ext.colsel(X, 0, 7, mu=mu.double(), p=p, gammas=g),
        lambda: ext.colsel(X, 0, 7, mu=mu, p=p.double(), gammas=g),
        lambda: ext.colsel(X, 0, 7, mu=mu, p=p, gammas=g.double()),
        lambda: ext.colsel(X.double(), 0, 7, mu=mu, p=p, gammas=g),
        lambda: ext.colsel(X[0], 0, 7, mu=mu, p=p, gammas=g),
        lambda: ext.colsel(X, 0, 0, mu=mu, p=p, gammas=g),            # f >= 1
        lambda: ext.colsel(X, 1, 23, mu=mu, p=p, gammas=g),           # f < n
        lambda: ext.colsel(X, 1, 30, mu=mu, p=p, gammas=g),
    ):
        with pytest.raises((RuntimeError, TypeError)):
            bad()
    ext.colsel(X, 0, 23, mu=mu, p=p, gammas=g)  # the median takes any f >= 1
    with pytest.raises(ValueError):
        D.agr_coord(X, 0, "median")
    with pytest.raises(ValueError):
        D.agr_coord(X, 23, "trimmed-mean")
    with pytest.raises(ValueError):
        D.agr_coord(X, 5, "krum")
    with pytest.raises(ValueError):
        D.agr_coord(X, 5, "median", "variance")


@pytest.mark.parametrize("agr", RULES)
def test_dispatch_past_the_cap_takes_the_torch_composition(ext, agr):
    """65 rows run the composition on the device, 64 the kernel; each agrees
    with the oracle of its own rows, on the same mu, p and trials."""
    n, f, d = 65, 15, 515
    X, H, mu, p, a, c = _random_case(n, d, torch.float32)
    gammas = _trial_gammas(a, c, 32)
    mu_c, p_c = mu.cpu(), p.cpu()
    got = D.agr_coord_objective(X, mu, p, gammas.cuda(), f, agr)
    assert got.is_cuda and got.dtype == torch.float64
    assert torch.allclose(got.cpu(), _oracle(H, mu_c, p_c, gammas, f, agr), rtol=1e-11, atol=0.0)
    prefix = X[:64].contiguous()
    kern = D.agr_coord_objective(prefix, mu, p, gammas.cuda(), f, agr)
    assert torch.equal(_bits(kern), _bits(ext.colsel(prefix, MODES[agr], f, mu=mu, p=p, gammas=gammas.cuda())))
    _check_against_oracle(ext, prefix, H[:64], mu, p, gammas, f, agr, f"prefix {agr}")
    out = D.agr_coord(X, f, agr)
    assert out.is_cuda and out.shape == (d,)
    gamma = D.agr_coord_gamma(X, mu, p, a, c, f, agr)
    assert torch.allclose(out, torch.addcmul(mu, gamma.to(mu.dtype), p), **_tol(torch.float32))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("agr", RULES)
@pytest.mark.parametrize("perturbation", ["unit", "std", "sign"])
def test_identical_rows_return_the_mean(perturbation, agr, dtype):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(64, generator=g) + 0.3
    Xd = x[None, :].repeat(8, 1).to("cuda", dtype)
    out = D.agr_coord(Xd, 1, agr, perturbation)
    mu_dev = D.attack_stats(Xd, perturbation)[0]
    assert torch.equal(out, mu_dev.to(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_operator_class_on_device(dtype):
    X = _random_case(23, 2050, dtype)[0]
    for agr in RULES:
        direct = D.agr_coord(X, 7, agr, "sign")
        for grads in ([X[i] for i in range(len(X))], X):
            out = CoordinateTailoredAttack(7, agr, perturbation="sign").apply(honest_grads=grads)
            assert out.is_cuda and out.dtype == dtype and out.shape == (2050,)
            assert torch.allclose(out.float(), direct.float(), **_tol(dtype))


@pytest.mark.parametrize("agr", RULES)
def test_agr_coord_captures_into_a_graph(agr):
    """No host sync anywhere: the whole call replays from a hipGraph."""
    X0 = _random_case(23, 2050, torch.float32)[0]
    cap = CapturedAggregate(lambda X: D.agr_coord(X, 7, agr), X0)
    g = torch.Generator().manual_seed(99)
    X1 = (torch.randn(23, 2050, generator=g) * 2.0 - 0.7).cuda()
    replayed = cap.run(X1).clone()
    eager = D.agr_coord(X1, 7, agr)
    assert torch.allclose(replayed, eager, **_tol(torch.float32))
    # and the first capture's data no longer decides the output
    assert not torch.allclose(replayed, D.agr_coord(X0, 7, agr), **_tol(torch.float32))
