"""Min-Max / Min-Sum attacks on the GPU: the statistics pass behind
little_fused(X, z, perturb) against explicit f64 differences, the device
dispatch against the functional oracle (run on X.float().cpu(), so both
sides see identical values), rejections, degenerate inputs and hipGraph
capture."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from byzpy_amd.attacks import MinMaxAttack, MinSumAttack
from byzpy_amd.hip import dispatch as D
from byzpy_amd.hip import require
from byzpy_amd.hip.graphs import CapturedAggregate
from byzpy_amd.ops import functional as F

DTYPES = [torch.float32, torch.bfloat16]
DTYPE_IDS = ["f32", "bf16"]
PERTURBATIONS = ["unit", "std", "sign"]

# (n, d): one case per register width / path
CASES = [
    (5, 33),      # P = 8, odd-d tail
    (8, 64),      # P = 8, full
    (12, 300),    # P = 16
    (23, 2050),   # P = 32, more than one block
    (40, 1030),   # P = 64 with pads: the masked walk at the widest kernel
    (64, 4097),   # full P = 64: the unmasked n == P walk
    (67, 512),    # first n past the register path: three-kernel composition
    (100, 777),
]


@pytest.fixture(scope="module")
def ext():
    return require()


def _tol(dtype):  # as in test_gpu_kernels.py
    return dict(atol=1e-4, rtol=1e-4) if dtype == torch.float32 else dict(atol=5e-2, rtol=5e-2)


@functools.lru_cache(maxsize=None)
def _case(n, d, dtype):
    """Device matrix and the f64 view of exactly the values it holds."""
    g = torch.Generator().manual_seed(100 * n + d)
    X = torch.randn(n, d, generator=g) * (1 + 0.1 * torch.arange(n))[:, None] + 0.3
    X = X[torch.randperm(n, generator=g)].to("cuda", dtype).contiguous()
    return X, X.float().cpu().double()


@functools.lru_cache(maxsize=None)
def _ref_stats(n, d, dtype, perturbation):
    """mu, p (the device's column-local form: "unit" is -mu), a, b, c from
    explicit f64 differences."""
    _, H = _case(n, d, dtype)
    mu = H.mean(dim=0)
    if perturbation == "unit":
        p = -mu
    elif perturbation == "std":
        p = -H.std(dim=0, unbiased=False)
    else:
        p = -torch.sign(mu)
    diff = mu[None, :] - H
    return mu, p, (diff * diff).sum(dim=1), (diff * p[None, :]).sum(dim=1), (p * p).sum()


@functools.lru_cache(maxsize=None)
def _oracle(n, d, dtype, attack, perturbation):
    X, _ = _case(n, d, dtype)
    fn = F.min_max if attack == "min_max" else F.min_sum
    return fn(X.float().cpu(), perturbation)


@pytest.mark.parametrize("n,d", CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("perturbation", PERTURBATIONS)
def test_statistics_pass(ext, n, d, dtype, perturbation):
    X, _ = _case(n, d, dtype)
    mu_r, p_r, a_r, b_r, c_r = _ref_stats(n, d, dtype, perturbation)
    code = PERTURBATIONS.index(perturbation)
    mu, p, stats = ext.little_fused(X, 0.0, code)
    for t, shape in ((mu, (d,)), (p, (d,)), (stats, (2 * n + 1,))):
        assert t.dtype == torch.float32 and t.device == X.device and t.shape == shape
    mu, p, stats = mu.cpu().double(), p.cpu().double(), stats.cpu().double()
    a, b, c = stats[:n], stats[n : 2 * n], stats[2 * n]
    assert torch.allclose(mu, mu_r, **_tol(dtype))
    assert torch.allclose(p, p_r, **_tol(dtype))
    rel_a = ((a - a_r).abs() / a_r).max().item()
    rel_c = (abs(c - c_r) / c_r).item()
    # b is a signed sum: scale by its Cauchy-Schwarz bound sqrt(a_i c)
    rel_b = ((b - b_r).abs() / (a_r * c_r).sqrt()).max().item()
    print(f"n={n} d={d} {perturbation}: rel a {rel_a:.2e}, b {rel_b:.2e}, c {rel_c:.2e}")
    # f32 sums of <= 4097 non-negative terms: worst case near d * 2^-24
    assert rel_a <= 1e-3 and rel_c <= 1e-3
    assert rel_b <= 1e-3
    # dispatch view of the same binding
    mu2, p2, a2, b2, c2 = D.attack_stats(X, perturbation)
    assert a2.shape == (n,) and b2.shape == (n,) and c2.dim() == 0
    assert torch.allclose(a2.cpu().double(), a_r, rtol=1e-3, atol=0.0)


@pytest.mark.parametrize("n,d", CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("perturbation", PERTURBATIONS)
@pytest.mark.parametrize("attack", ["min_max", "min_sum"])
def test_dispatch_matches_oracle(n, d, dtype, perturbation, attack):
    X, _ = _case(n, d, dtype)
    fn = D.min_max if attack == "min_max" else D.min_sum
    out = fn(X, perturbation)
    assert out.dtype == dtype and out.device == X.device and out.shape == (d,)
    ref = _oracle(n, d, dtype, attack, perturbation)
    err = (out.float().cpu() - ref).abs().max().item()
    print(f"{attack} n={n} d={d} {perturbation}: max |device - oracle| = {err:.3e}")
    assert torch.allclose(out.float().cpu(), ref, **_tol(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("cls,fn", [(MinMaxAttack, D.min_max), (MinSumAttack, D.min_sum)])
def test_operator_classes_on_device(cls, fn, dtype):
    X, _ = _case(23, 2050, dtype)
    direct = fn(X, "sign").float()
    # Same kernels on the same values: only the arrival order of the float
    # atomic adds can differ between two calls. That moves each f32 sum by
    # about an ulp, gamma (built from up to three such sums: a, b, tau) by
    # up to three, and the result by one more rounding to the output dtype:
    # four ulp of the output dtype at the largest coordinate.
    atol = 4 * torch.finfo(dtype).eps * direct.abs().max().item()
    for grads in ([X[i] for i in range(len(X))], X):
        out = cls("sign").apply(honest_grads=grads)
        assert out.is_cuda and out.dtype == dtype and out.shape == (2050,)
        err = (out.float() - direct).abs().max().item()
        print(f"{cls.__name__} {dtype}: max |operator - dispatch| = {err:.3e}, atol {atol:.3e}")
        assert err <= atol
    # and the bound is tight enough to tell the perturbations apart
    assert (fn(X, "std").float() - direct).abs().max().item() > atol


@pytest.mark.parametrize("n,d", [(12, 2048), (67, 512)])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_default_little_fused_is_unchanged(ext, n, d, dtype):
    X, H = _case(n, d, dtype)
    out = ext.little_fused(X, 1.5)
    assert isinstance(out, torch.Tensor) and out.dtype == dtype and out.shape == (d,)
    Xf = H.float()
    ref = Xf.mean(dim=0) + 1.5 * Xf.std(dim=0, unbiased=False)
    assert torch.allclose(out.float().cpu(), ref, **_tol(dtype))
    assert torch.equal(out, ext.little_fused(X, 1.5))


def test_rejections(ext):
    X = torch.randn(5, 8, device="cuda")
    for bad in (
        lambda: ext.little_fused(X.cpu(), 0.0, 1),
        lambda: ext.little_fused(X.to(torch.int32), 0.0, 1),
        lambda: ext.little_fused(X.half(), 0.0, 1),
        lambda: ext.little_fused(X, 0.0, 3),
        lambda: ext.little_fused(X, 0.0, -1),
        lambda: ext.little_fused(torch.zeros(1025, 8, device="cuda"), 0.0, 1),
        lambda: ext.little_fused(torch.zeros(0, 8, device="cuda"), 0.0, 1),
    ):
        with pytest.raises(RuntimeError):
            bad()
    with pytest.raises(ValueError):
        D.min_max(X, "variance")
    # past the binding's row cap the dispatch takes the functional path
    big = torch.randn(1025, 8, device="cuda")
    out = D.min_sum(big, "std")
    assert out.is_cuda and torch.allclose(out.cpu(), F.min_sum(big.cpu(), "std"), atol=1e-4)


def _degenerate_cases():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(64, generator=g) + 0.3
    const_cols = torch.arange(64, dtype=torch.float32)[None, :].repeat(8, 1) * 0.25
    return [
        ("identical_rows", x[None, :].repeat(8, 1), PERTURBATIONS),
        ("one_row", x[None, :].clone(), PERTURBATIONS),
        ("x_and_minus_x", torch.stack([x, -x]), ["unit", "sign"]),
        ("constant_columns", const_cols, ["std"]),
    ]


DEGENERATE = [(name, X, p) for name, X, perts in _degenerate_cases() for p in perts]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("attack", ["min_max", "min_sum"])
@pytest.mark.parametrize(
    "name,X,perturbation", DEGENERATE, ids=[f"{c[0]}-{c[2]}" for c in DEGENERATE]
)
def test_degenerate_inputs_return_the_mean(name, X, perturbation, attack, dtype):
    Xd = X.to("cuda", dtype)
    fn = D.min_max if attack == "min_max" else D.min_sum
    out = fn(Xd, perturbation)
    assert out.dtype == dtype and torch.isfinite(out).all()
    H = Xd.float().cpu().double()
    mu = H.mean(dim=0)
    mu_dev = D.attack_stats(Xd, perturbation)[0]
    # the kernel's own mean is exact here: equal values, or two that cancel
    assert torch.equal(mu_dev.cpu().double(), mu)
    if attack == "min_max" and name == "identical_rows" and perturbation != "std":
        # The one case with c != 0 and a Gram in it: tau comes off the f32
        # Gram as ||a||^2 + ||b||^2 - 2 a.b, good to a few ulp of the squared
        # row norm, so gamma may be as large as puts m sqrt(4 * 2^-23) ~ 7e-4
        # row norms from mu; a bf16 result adds its own rounding, 2^-9.
        scale = H.norm(dim=1).max().item()
        bound = (1e-3 if dtype == torch.float32 else 1e-3 + 2.0**-9) * scale
        dist = (out.float().cpu().double() - mu).norm().item()
        print(f"{name} {perturbation} {attack}: ||m - mu|| = {dist:.3e}, bound {bound:.3e}")
        assert dist <= bound
        return
    # Everywhere else gamma is exactly 0 (c = 0; or a = 0 with no Gram
    # involved; or a 1 x 1 Gram, whose tau is g + g - 2g = 0), so m is the
    # kernel's mean cast to the input dtype, bit for bit.
    assert torch.equal(out, mu_dev.to(dtype))


def test_min_max_captures_into_a_graph():
    """No host sync anywhere: the whole call replays from a hipGraph."""
    X0, _ = _case(23, 2050, torch.float32)
    cap = CapturedAggregate(lambda X: D.min_max(X), X0)
    g = torch.Generator().manual_seed(99)
    X1 = (torch.randn(23, 2050, generator=g) * 2.0 - 0.7).cuda()
    replayed = cap.run(X1).clone()
    eager = D.min_max(X1)
    assert torch.allclose(replayed, eager, **_tol(torch.float32))
    assert torch.allclose(replayed.cpu(), F.min_max(X1.cpu()), **_tol(torch.float32))
    # and the first capture's data no longer decides the output
    assert not torch.allclose(replayed, D.min_max(X0), **_tol(torch.float32))
