"""Aggregator-tailored attacks on the GPU: the device grid search behind
krum_select(G, f, q, stats=, rule=) against the functional oracle (run on
X.float().cpu(), so both sides see identical values), the binding's flags and
rejections, the dispatch past the kernel's row cap, degenerate inputs and
hipGraph capture."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from byzpy_amd.attacks import AGRTailoredAttack
from byzpy_amd.hip import dispatch as D
from byzpy_amd.hip import require
from byzpy_amd.hip.graphs import CapturedAggregate
from byzpy_amd.ops import functional as F

DTYPES = [torch.float32, torch.bfloat16]
DTYPE_IDS = ["f32", "bf16"]
PERTURBATIONS = ["unit", "std", "sign"]
RULES = ["krum", "multi-krum", "bulyan"]

# (n, f, d)
SMALL = [
    (9, 2, 33),      # Bulyan at its minimum N = 4f + 3, odd d
    (11, 2, 300),    # Bulyan just above its minimum
    (23, 5, 2050),   # P = 32 statistics, more than one block
]
LARGE = [
    (49, 15, 515),   # N = 64: one full lane chunk
    (64, 15, 1030),  # N = 79: past one chunk, last register-path n
    (113, 15, 257),  # N = 128: the cap, three-kernel statistics
]


@pytest.fixture(scope="module")
def ext():
    return require()


def _tol(dtype):  # as in test_gpu_kernels.py
    return dict(atol=1e-4, rtol=1e-4) if dtype == torch.float32 else dict(atol=5e-2, rtol=5e-2)


@pytest.fixture(scope="module", autouse=True)
def _one_torch_thread():
    """The oracle is thousands of tiny CPU ops in Python loops: intra-op
    threads only add wake-ups to them, and whatever ran earlier in the
    process may have left torch with more threads than there are CPUs."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


@functools.lru_cache(maxsize=None)
def _case(n, d, dtype):
    """As test_gpu_minmax_attacks._case: the device matrix and the f32 CPU
    view of exactly the values it holds."""
    g = torch.Generator().manual_seed(100 * n + d)
    X = torch.randn(n, d, generator=g) * (1 + 0.1 * torch.arange(n))[:, None] + 0.3
    X = X[torch.randperm(n, generator=g)].to("cuda", dtype).contiguous()
    return X, X.float().cpu()


@functools.lru_cache(maxsize=None)
def _oracle_gamma(n, f, d, dtype, agr, perturbation):
    return F.agr_tailored_gamma(_case(n, d, dtype)[1], f, agr, None, perturbation)


def _device_gamma(n, f, d, dtype, agr, perturbation):
    """The device's gamma, in the oracle's units: the device's "unit" p is
    the unnormalised -mu (m does not change), so gamma is compared as the
    step length gamma ||p|| over the oracle's ||p||."""
    X, H = _case(n, d, dtype)
    _, _, a, b, c = D.attack_stats(X, perturbation)
    gamma = D.agr_tailored_gamma(D.gram(X), a, b, c, f, agr)
    assert gamma.dim() == 0 and gamma.dtype == torch.float32 and gamma.is_cuda
    _, p = F.attack_perturbation(H, perturbation)
    return float(gamma) * math.sqrt(float(c)) / float(p.norm())


@pytest.mark.parametrize("n,f,d", SMALL)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("perturbation", PERTURBATIONS)
@pytest.mark.parametrize("agr", RULES)
def test_device_gamma_and_vector_match_oracle(n, f, d, dtype, perturbation, agr):
    """1e-3 relative: the 2^-16 search resolution plus the f32 Gram-identity
    error (about 1e-5 here, row norms being comparable to distances)."""
    X, H = _case(n, d, dtype)
    ref = _oracle_gamma(n, f, d, dtype, agr, perturbation)
    got = _device_gamma(n, f, d, dtype, agr, perturbation)
    rel = abs(got - ref) / ref
    print(f"{agr} n={n} f={f} d={d} {perturbation} {dtype}: gamma {got:.6f} vs {ref:.6f}, rel {rel:.2e}")
    assert rel <= 1e-3
    out = D.agr_tailored(X, f, agr, None, perturbation)
    assert out.dtype == dtype and out.device == X.device and out.shape == (d,)
    m_ref = F.agr_tailored(H, f, agr, None, perturbation)
    err = (out.float().cpu() - m_ref).abs().max().item()
    print(f"    max |device - oracle| = {err:.3e}")
    assert torch.allclose(out.float().cpu(), m_ref, **_tol(dtype))


@pytest.mark.parametrize("n,f,d", LARGE)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("perturbation", PERTURBATIONS)
@pytest.mark.parametrize("agr", RULES)
def test_device_gamma_brackets_the_boundary(n, f, d, dtype, perturbation, agr):
    """No oracle search at these sizes: two oracle evaluations around the
    device's gamma."""
    _, H = _case(n, d, dtype)
    g = _device_gamma(n, f, d, dtype, agr, perturbation)
    print(f"{agr} n={n} f={f} d={d} {perturbation} {dtype}: gamma {g:.6f}")
    assert g > 0.0
    assert F.agr_feasible(H, g * (1.0 - 2e-3), f, agr, None, perturbation)
    assert not F.agr_feasible(H, g * (1.0 + 2e-3), f, agr, None, perturbation)


def _binding_inputs(n, d, perturbation="std"):
    X, _ = _case(n, d, torch.float32)
    _, _, stats = require().little_fused(X, 0.0, PERTURBATIONS.index(perturbation))
    return D.gram(X), stats


@pytest.mark.parametrize("rule", [0, 1], ids=["krum", "bulyan"])
@pytest.mark.parametrize("n,f,d", [(23, 5, 2050), (64, 15, 1030), (113, 15, 257)])
def test_same_inputs_give_the_same_bits(ext, n, f, d, rule):
    G, stats = _binding_inputs(n, d)
    g1 = ext.krum_select(G, f, n, stats=stats, rule=rule)
    g2 = ext.krum_select(G, f, n, stats=stats, rule=rule)
    assert g1.dim() == 0 and g1.dtype == torch.float32 and float(g1) > 0.0
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    grid = float(g1) * torch.linspace(0.0, 2.0, 77, device="cuda")
    fl1 = ext.krum_select(G, f, n, stats=stats, rule=rule, gammas=grid)
    fl2 = ext.krum_select(G, f, n, stats=stats, rule=rule, gammas=grid)
    assert fl1.dtype == torch.int32 and fl1.shape == (77,)
    assert torch.equal(fl1, fl2)


@pytest.mark.parametrize("agr", RULES)
@pytest.mark.parametrize("n,f,d", [(9, 2, 33), (23, 5, 2050)])
def test_flags_match_the_oracle_point_for_point(ext, n, f, d, agr):
    """A hand-made grid that keeps 1 % clear of the boundary, where the f32
    Gram identity (1e-5) cannot change a flag."""
    _, H = _case(n, d, torch.float32)
    G, stats = _binding_inputs(n, d)
    gs = _oracle_gamma(n, f, d, torch.float32, agr, "std")
    mult = [0.0, 1e-3, 0.25, 0.5, 0.9, 0.99, 1.01, 1.1, 2.0, 10.0, 1e3]
    grid = torch.tensor([gs * k for k in mult], dtype=torch.float32, device="cuda")
    q = 1 if agr == "krum" else n
    flags = ext.krum_select(G, f, q, stats=stats, rule=int(agr == "bulyan"), gammas=grid)
    want = [int(F.agr_feasible(H, float(g), f, agr, None, "std")) for g in grid.cpu()]
    assert want == [1] * 6 + [0] * 5
    assert flags.cpu().tolist() == want
    # a non-finite trial value is infeasible, not an error
    odd = torch.tensor([float("nan"), float("inf"), 0.0], device="cuda")
    got = ext.krum_select(G, f, q, stats=stats, rule=int(agr == "bulyan"), gammas=odd)
    assert got.cpu().tolist() == [0, 0, 1]


def test_non_finite_statistics_give_zero(ext):
    G, stats = _binding_inputs(23, 2050)
    for pos, bad in ((3, float("nan")), (30, float("inf")), (46, float("nan")), (46, 0.0)):
        s = stats.clone()
        s[pos] = bad
        for rule in (0, 1):
            assert float(ext.krum_select(G, 5, 23, stats=s, rule=rule)) == 0.0


def test_rejections(ext):
    G, stats = _binding_inputs(23, 2050)
    grid = torch.ones(4, device="cuda")
    big = torch.eye(114, device="cuda")
    for bad in (
        lambda: ext.krum_select(G.cpu(), 5, 23, stats=stats.cpu(), rule=0),
        lambda: ext.krum_select(G, 5, 23, stats=stats.cpu(), rule=0),
        lambda: ext.krum_select(G, 5, 23, stats=stats, rule=0, gammas=grid.cpu()),
        lambda: ext.krum_select(G.double(), 5, 23, stats=stats, rule=0),
        lambda: ext.krum_select(G, 5, 23, stats=stats.double(), rule=0),
        lambda: ext.krum_select(G, 5, 23, stats=stats[:-1], rule=0),
        lambda: ext.krum_select(big, 15, 114, stats=torch.ones(229, device="cuda"), rule=0),  # N = 129
        lambda: ext.krum_select(G, 0, 23, stats=stats, rule=0),
        lambda: ext.krum_select(G, 24, 23, stats=stats, rule=0),
        lambda: ext.krum_select(G, 7, 23, stats=stats, rule=1),   # n = 23 < 3f + 3 = 24
        lambda: ext.krum_select(G, 5, 0, stats=stats, rule=0),
        lambda: ext.krum_select(G, 5, 29, stats=stats, rule=0),
        lambda: ext.krum_select(G, 5, 23, stats=stats, rule=2),
        lambda: ext.krum_select(G, 5, 23, stats=stats, rule=0, gammas=grid[:0]),
    ):
        with pytest.raises(RuntimeError):
            bad()
    X, _ = _case(23, 2050, torch.float32)
    with pytest.raises(ValueError):
        D.agr_tailored(X, 0, "krum")
    with pytest.raises(ValueError):
        D.agr_tailored(X, 7, "bulyan")
    with pytest.raises(ValueError):
        D.agr_tailored(X, 5, "krum", None, "variance")


@pytest.mark.parametrize("agr", ["krum", "multi-krum"])
def test_dispatch_past_the_cap_takes_the_torch_composition(agr):
    n, f, d = 120, 15, 64  # N = 135 > 128
    X, H = _case(n, d, torch.float32)
    ref = _oracle_gamma(n, f, d, torch.float32, agr, "std")
    got = _device_gamma(n, f, d, torch.float32, agr, "std")
    rel = abs(got - ref) / ref
    print(f"{agr} past the cap: gamma {got:.6f} vs {ref:.6f}, rel {rel:.2e}")
    assert rel <= 1e-3
    out = D.agr_tailored(X, f, agr)
    assert out.is_cuda and out.dtype == torch.float32
    assert torch.allclose(out.cpu(), F.agr_tailored(H, f, agr), **_tol(torch.float32))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("agr", RULES)
@pytest.mark.parametrize("perturbation", PERTURBATIONS)
def test_identical_rows_return_the_mean(perturbation, agr, dtype):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(64, generator=g) + 0.3
    Xd = x[None, :].repeat(8, 1).to("cuda", dtype)
    out = D.agr_tailored(Xd, 1, agr, None, perturbation)
    mu_dev = D.attack_stats(Xd, perturbation)[0]
    # a = 0 exactly, so gamma0 = 0 and every grid point is 0: m is the
    # kernel's own mean cast to the input dtype, bit for bit
    assert torch.equal(mu_dev.cpu().double(), Xd.float().cpu().double().mean(dim=0))
    assert torch.equal(out, mu_dev.to(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_operator_class_on_device(dtype):
    X, _ = _case(23, 2050, dtype)
    direct = D.agr_tailored(X, 5, "bulyan", None, "sign")
    for grads in ([X[i] for i in range(len(X))], X):
        out = AGRTailoredAttack(5, "bulyan", perturbation="sign").apply(honest_grads=grads)
        assert out.is_cuda and out.dtype == dtype and out.shape == (2050,)
        # the statistics pass adds with float atomics, so two calls agree
        # to the search resolution and the output rounding, not to the bit
        assert torch.allclose(out.float(), direct.float(), **_tol(dtype))


def test_agr_tailored_captures_into_a_graph():
    """No host sync anywhere: the whole call replays from a hipGraph."""
    X0, _ = _case(23, 2050, torch.float32)
    cap = CapturedAggregate(lambda X: D.agr_tailored(X, 5, "bulyan"), X0)
    g = torch.Generator().manual_seed(99)
    X1 = (torch.randn(23, 2050, generator=g) * 2.0 - 0.7).cuda()
    replayed = cap.run(X1).clone()
    eager = D.agr_tailored(X1, 5, "bulyan")
    assert torch.allclose(replayed, eager, **_tol(torch.float32))
    ref = F.agr_tailored(X1.cpu(), 5, "bulyan")
    assert torch.allclose(replayed.cpu(), ref, **_tol(torch.float32))
    # and the first capture's data no longer decides the output
    assert not torch.allclose(replayed, D.agr_tailored(X0, 5, "bulyan"), **_tol(torch.float32))
