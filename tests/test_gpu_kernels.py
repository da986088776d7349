"""GPU parity tests: every HIP kernel against the plain-torch fp32 reference
(SURVEY.md §4 pattern 2, on-device). All marked gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from byzpy_amd.hip import dispatch as D
from byzpy_amd.ops import functional as F


def _rand(n, d, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, d, generator=g)
    return X.to("cuda", dtype)


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    from byzpy_amd.hip import require

    require()


SHAPES = [(8, 1000), (16, 4097), (64, 8192), (10, 33)]
DTYPES = [torch.float32, torch.bfloat16]


def _tol(dtype):
    return dict(atol=1e-4, rtol=1e-4) if dtype == torch.float32 else dict(atol=5e-2, rtol=5e-2)


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_median(n, d, dtype):
    X = _rand(n, d, dtype)
    out = D.median(X)
    ref = F.median(X.float().cpu())
    assert torch.allclose(out.float().cpu(), ref, **_tol(dtype))


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_trimmed_mean(n, d, dtype):
    X = _rand(n, d, dtype)
    out = D.trimmed_mean(X, 2)
    ref = F.trimmed_mean(X.float().cpu(), 2)
    assert torch.allclose(out.float().cpu(), ref, **_tol(dtype))


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_meamed(n, d, dtype):
    X = _rand(n, d, dtype)
    out = D.mean_of_medians(X, 2)
    ref = F.mean_of_medians(X.float().cpu(), 2)
    if dtype == torch.float32:
        assert torch.allclose(out.float().cpu(), ref, **_tol(dtype))
    else:
        # bf16 quantization produces exact deviation TIES at the window
        # boundary; GPU (sorted two-pointer) and CPU (topk index order) may
        # keep different-but-equally-close elements. Valid results differ by
        # at most 2*tau/(n-f) per boundary tie, tau = the largest kept
        # deviation — check against that bound instead of allclose.
        Xf = X.float().cpu()
        f = 2
        med = F.median(Xf)
        dev = (Xf - med[None, :]).abs()
        tau = torch.topk(dev, k=n - f, dim=0, largest=False).values[-1]
        bound = 2.0 * tau / (n - f) + 0.02
        diff = (out.float().cpu() - ref).abs()
        assert (diff <= bound).all(), f"max excess {(diff - bound).max()}"


@pytest.mark.parametrize("n", [72, 100, 128, 200, 256, 512])
def test_colsel_lds_large_n(n):
    X = _rand(n, 2049)
    assert torch.allclose(D.median(X).cpu(), F.median(X.cpu()), atol=1e-4)
    assert torch.allclose(
        D.trimmed_mean(X, 5).cpu(), F.trimmed_mean(X.cpu(), 5), atol=1e-4
    )
    assert torch.allclose(
        D.mean_of_medians(X, 5).cpu(), F.mean_of_medians(X.cpu(), 5), atol=1e-4
    )


@pytest.mark.parametrize("n,d", [(8, 512), (64, 8192), (100, 4096), (64, 8191)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gram_vs_matmul(n, d, dtype):
    X = _rand(n, d, dtype)
    G = D.gram(X)
    Xf = X.float()
    ref = Xf @ Xf.T
    tol = 1e-3 if dtype == torch.float32 else 0.3
    assert (G - ref).abs().max().item() < tol * max(1.0, ref.abs().max().item() / 100)


def test_gram_transpose_detecting():
    # asymmetric check (guide §3): X[i] = e_i * (i+1) + ramp — G must equal ref
    n, d = 32, 256
    X = torch.zeros(n, d)
    for i in range(n):
        X[i, i] = i + 1.0
        X[i, (i + 7) % d] = 0.5 * (i + 3)
    X = X.cuda()
    G = D.gram(X)
    ref = X.float() @ X.float().T
    assert torch.allclose(G, ref, atol=1e-3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_sqnorms_and_scale(dtype):
    X = _rand(33, 5000, dtype)
    norms = D.row_sqnorms(X)
    ref = (X.float() ** 2).sum(dim=1)
    assert torch.allclose(norms, ref, rtol=2e-2 if dtype == torch.bfloat16 else 1e-4)
    s = torch.rand(33, device="cuda")
    Y = D.row_scale(X, s)
    refY = (X.float() * s[:, None]).to(dtype)
    assert torch.allclose(Y.float(), refY.float(), **_tol(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_multi_krum_gpu(dtype):
    X = _rand(24, 4096, dtype, seed=3)
    out = D.multi_krum(X, 4, 6)
    ref = F.multi_krum(X.float().cpu(), 4, 6)
    assert torch.allclose(out.float().cpu(), ref, **_tol(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_geometric_median_gpu(dtype):
    X = _rand(16, 2048, dtype, seed=4)
    out = D.geometric_median(X, tol=1e-7, max_iter=200)
    ref = F.geometric_median(X.float().cpu(), tol=1e-7, max_iter=200)
    assert (out.float().cpu() - ref).norm() < 0.05 * max(1.0, ref.norm().item())


@pytest.mark.parametrize("dtype", DTYPES)
def test_centered_clipping_gpu(dtype):
    X = _rand(16, 2048, dtype, seed=5)
    out = D.centered_clipping(X, c_tau=0.7, M=6)
    ref = F.centered_clipping(X.float().cpu(), c_tau=0.7, M=6)
    assert torch.allclose(out.float().cpu(), ref, atol=5e-2 if dtype == torch.bfloat16 else 1e-3)


def test_cge_gpu():
    X = _rand(20, 3000, seed=6)
    out = D.cge(X, 4)
    ref = F.cge(X.cpu(), 4)
    assert torch.allclose(out.cpu(), ref, atol=1e-4)


def test_clip_and_arc_gpu():
    X = _rand(32, 3000, seed=7)
    assert torch.allclose(D.clip_rows(X, 1.0).cpu(), F.clip_rows(X.cpu(), 1.0), atol=1e-4)
    assert torch.allclose(D.arc_clip(X, 4).cpu(), F.arc_clip(X.cpu(), 4), atol=1e-4)


def test_bucketing_gpu():
    X = _rand(17, 1000, seed=8)
    perm = list(range(17))
    out = D.bucketing(X, 4, perm)
    ref = F.bucketing(X.cpu(), 4, perm)
    assert torch.allclose(out.cpu(), ref, atol=1e-4)


def test_nnm_gpu():
    X = _rand(24, 2000, seed=9)
    out = D.nnm(X, 5)
    ref = F.nnm(X.cpu(), 5)
    assert torch.allclose(out.cpu(), ref, atol=1e-3)


def test_mda_monna_gpu():
    X = _rand(16, 1024, seed=10)
    assert torch.allclose(
        D.minimum_diameter_averaging(X, 4).cpu(),
        F.minimum_diameter_averaging(X.cpu(), 4),
        atol=1e-4,
    )
    assert torch.allclose(D.monna(X, 4, 0).cpu(), F.monna(X.cpu(), 4, 0), atol=1e-4)


def test_aggregator_classes_on_gpu():
    from byzpy_amd.aggregators import CoordinateWiseMedian, MultiKrum

    X = _rand(10, 513, torch.bfloat16, seed=11)
    out = CoordinateWiseMedian().aggregate(list(X))
    assert out.is_cuda and out.dtype == torch.bfloat16
    out2 = MultiKrum(2, 3).aggregate(list(X))
    assert out2.is_cuda and out2.shape == (513,)


@pytest.mark.parametrize("n,f,q", [(16, 3, 4), (64, 16, 12), (100, 20, 8)])
def test_krum_select_kernel(n, f, q):
    from byzpy_amd.hip import require

    X = _rand(n, 2048, seed=21)
    G = D.gram(X)
    idx = require().krum_select(G, f, q)
    # reference: torch scores path on the same Gram
    norms = torch.diagonal(G)
    D2 = (norms[:, None] + norms[None, :] - 2.0 * G).clamp_(min=0.0)
    D2 = D2 + torch.diag(torch.full((n,), float("inf"), device=G.device))
    scores = torch.topk(D2, k=n - f - 1, dim=1, largest=False).values.sum(dim=1)
    ref = torch.topk(scores, k=q, largest=False).indices
    assert set(idx.cpu().tolist()) == set(ref.cpu().tolist())


class TestCafKernels:
    """K9 fused pair: caf_matvec (s = (X - mu) @ v) and caf_colsum
    (t = scale * sum_i a_i (x_i - mu)) vs plain torch f32."""

    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
    @pytest.mark.parametrize("n,d", [(8, 4096), (64, 8192), (33, 1000)])
    def test_matvec_parity(self, n, d, dtype):
        from byzpy_amd.hip import require

        X = _rand(n, d, dtype, seed=31)
        mu = _rand(1, d, torch.float32, seed=32)[0]
        v = _rand(1, d, torch.float32, seed=33)[0]
        out = require().caf_matvec(X, mu, v)
        ref = (X.float() - mu) @ v
        assert torch.allclose(out, ref, atol=1e-2 * d**0.5, rtol=1e-3)

    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
    @pytest.mark.parametrize("n,d", [(8, 4096), (64, 8192), (33, 1000)])
    def test_colsum_parity(self, n, d, dtype):
        from byzpy_amd.hip import require

        X = _rand(n, d, dtype, seed=41)
        mu = _rand(1, d, torch.float32, seed=42)[0]
        a = _rand(1, n, torch.float32, seed=43)[0]
        sc = torch.tensor(0.25, device="cuda")
        out = require().caf_colsum(X, a, mu, sc)
        ref = 0.25 * (a[:, None] * (X.float() - mu)).sum(dim=0)
        assert torch.allclose(out, ref, atol=2e-2, rtol=1e-3)
        # mu=None, scale=None: plain weighted column sum
        out2 = require().caf_colsum(X, a)
        ref2 = (a[:, None] * X.float()).sum(dim=0)
        assert torch.allclose(out2, ref2, atol=2e-2, rtol=1e-3)

    def test_caf_dispatch_matches_oracle(self):
        X = _rand(24, 4096, torch.float32, seed=51)
        honest = X.clone()
        honest[-4:] = 40.0  # 4 clear outlier rows
        got = D.caf(honest, 4)
        ref = F.caf(honest.cpu(), 4)
        # trajectories are float-order sensitive; demand the robust outcome
        assert (got.cpu() - ref).norm() < 0.5 * ref.norm() + 1e-3
        clean_mean = honest[:-4].mean(dim=0).cpu()
        assert (got.cpu() - clean_mean).norm() < (honest.mean(dim=0).cpu() - clean_mean).norm()


AGG_GPU_CASES = None


def _all_agg_instances():
    from byzpy_amd.aggregators import (
        CAF,
        CenteredClipping,
        ComparativeGradientElimination,
        CoordinateWiseMedian,
        CoordinateWiseTrimmedMean,
        GeometricMedian,
        Krum,
        MeanOfMedians,
        MinimumDiameterAveraging,
        MoNNA,
        MultiKrum,
        SMEA,
    )

    return [
        CoordinateWiseMedian(),
        CoordinateWiseTrimmedMean(3),
        MeanOfMedians(3),
        MultiKrum(3, 4),
        Krum(3),
        GeometricMedian(),
        MinimumDiameterAveraging(3),
        MoNNA(3),
        SMEA(3),
        CenteredClipping(c_tau=0.7),
        ComparativeGradientElimination(3),
        CAF(3),
    ]


@pytest.mark.parametrize(
    "agg", _all_agg_instances(), ids=[a.name for a in _all_agg_instances()]
)
def test_every_aggregator_on_device_matches_cpu_oracle(agg):
    """Every aggregator class, bf16 CUDA tensors in -> device result out,
    within bf16 tolerance of the fp32 CPU oracle on the same values."""
    X = _rand(16, 4097, torch.bfloat16, seed=77)  # odd d: vector fallback
    grads = list(X)
    out = agg.aggregate(grads)
    assert out.is_cuda and out.dtype == torch.bfloat16 and out.shape == (4097,)
    ref = agg.aggregate([g.cpu().float() for g in grads])
    tol = 0.05 if agg.name in ("caf",) else 0.02
    num = (out.cpu().float() - ref).norm()
    den = ref.norm().clamp_min(1e-6)
    assert num / den < tol, f"{agg.name}: rel err {num / den:.4f}"


@pytest.mark.parametrize("preagg_name", ["clipping", "bucketing", "nnm", "arc"])
def test_every_preagg_on_device(preagg_name):
    from byzpy_amd.pre_aggregators import ARC, Bucketing, Clipping, NearestNeighborMixing

    pre = {
        "clipping": Clipping(1.0),
        "bucketing": Bucketing(3, perm=list(range(16))),
        "nnm": NearestNeighborMixing(3),
        "arc": ARC(3),
    }[preagg_name]
    X = _rand(16, 2048, torch.bfloat16, seed=78)
    out = pre.pre_aggregate(list(X))
    assert all(v.is_cuda and v.dtype == torch.bfloat16 for v in out)
    ref = pre.pre_aggregate([g.cpu().float() for g in X])
    assert len(out) == len(ref)
    for a, b in zip(out, ref):
        assert (a.cpu().float() - b).norm() / b.norm().clamp_min(1e-6) < 0.02


class TestRadixMedianLargeN:
    """bf16 median for n > 64 vs the fp32 oracle, bit for bit: a median of
    bf16 inputs is one of them or the mean of two. The binding sends a
    shape to the radix engine (rsel.hip) only for n > 512, or n > 64 at
    d >= 32768, so at these d only n = 700 and 4096 of test_parity reach it;
    n = 65 ... 512 and the other three tests (n = 100, 300, 129) run the
    cooperative LDS sort. test_gpu_colsel_exact.py::test_radix covers the
    radix engine at 64 < n <= 512."""

    @pytest.mark.parametrize("n", [65, 100, 128, 257, 512, 700, 4096])
    def test_parity(self, n):
        X = _rand(n, 3001, torch.bfloat16, seed=n)
        out = D.median(X)
        ref = F.median(X.float().cpu()).bfloat16()
        assert torch.equal(out.cpu(), ref), f"n={n}"

    def test_with_inf_rows(self):
        X = _rand(100, 2048, torch.bfloat16, seed=3)
        X[7] = float("inf")
        X[13] = float("-inf")
        out = D.median(X)
        ref = F.median(X.float().cpu()).bfloat16()
        assert torch.equal(out.cpu(), ref)

    def test_ties_heavy(self):
        # constant-ish columns: every bucket collapses to one value
        X = torch.ones(300, 1024, dtype=torch.bfloat16, device="cuda")
        X[:150] = 2.0
        out = D.median(X)
        ref = F.median(X.float().cpu()).bfloat16()
        assert torch.equal(out.cpu(), ref)

    def test_odd_d_and_small_d(self):
        X = _rand(129, 77, torch.bfloat16, seed=5)
        out = D.median(X)
        ref = F.median(X.float().cpu()).bfloat16()
        assert torch.equal(out.cpu(), ref)


def _meamed_tie_avg_ref(Xf: torch.Tensor, f: int) -> torch.Tensor:
    """CPU f32 replica of the radix MEAMED closed form (rsel.hip): keep all
    dev < rho, distribute exact dev==rho ties left-side first at their mean."""
    n = Xf.shape[0]
    k = n - f
    med = F.median(Xf)
    dev = (Xf - med[None, :]).abs()
    rho = dev.sort(dim=0).values[k - 1]
    below = dev < rho[None, :]
    nb = below.sum(0)
    ties = dev == rho[None, :]
    left = ties & (Xf < med[None, :])
    right = ties & ~left
    tk = (k - nb).float()
    cL = left.sum(0).float()
    cR = right.sum(0).float()
    takeL = torch.minimum(tk, cL)
    takeR = tk - takeL
    sL = (Xf * left).sum(0)
    sR = (Xf * right).sum(0)
    S = (Xf * below).sum(0)
    S = S + torch.where(cL > 0, sL / cL.clamp(min=1), torch.zeros_like(sL)) * takeL
    S = S + torch.where(cR > 0, sR / cR.clamp(min=1), torch.zeros_like(sR)) * takeR
    return S / k


class TestRadixLargeNModes:
    """TRIMMED / MEAMED / f32 MEDIAN at n >= 200 vs the fp32 CPU oracle.
    Every d here is below 32768, so under the binding's routing rule
    (radix for n > 512, or n > 64 at d >= 32768) only n = 1024, 2048 and
    4096 run the rsel.hip radix engine; n = 200 ... 512, and the inf-rows
    and ties tests (n = 300, 256, 400), run the cooperative LDS sort.
    test_gpu_colsel_exact.py::test_radix covers the engine's modes at
    64 < n <= 512 and just above."""

    @pytest.mark.parametrize("n", [200, 300, 512, 1024, 4096])
    @pytest.mark.parametrize("dtype", DTYPES)
    def test_trimmed(self, n, dtype):
        f = n // 8
        X = _rand(n, 1537, dtype, seed=n)
        out = D.trimmed_mean(X, f)
        ref = F.trimmed_mean(X.float().cpu(), f)
        tol = dict(atol=1e-3, rtol=1e-3) if dtype == torch.float32 else dict(
            atol=2e-2, rtol=2e-2
        )
        assert torch.allclose(out.float().cpu(), ref, **tol)

    @pytest.mark.parametrize("n", [200, 512, 2048])
    def test_f32_median_exact(self, n):
        X = _rand(n, 2047, torch.float32, seed=n + 1)
        out = D.median(X)
        ref = F.median(X.cpu())
        assert torch.equal(out.cpu(), ref)

    def test_f32_median_inf_rows(self):
        X = _rand(300, 1024, torch.float32, seed=9)
        X[3] = float("inf")
        X[5] = float("-inf")
        out = D.median(X)
        ref = F.median(X.cpu())
        assert torch.equal(out.cpu(), ref)

    @pytest.mark.parametrize("n", [200, 512, 1024])
    @pytest.mark.parametrize("dtype", DTYPES)
    def test_meamed(self, n, dtype):
        f = n // 6
        X = _rand(n, 1023, dtype, seed=n + 2)
        out = D.mean_of_medians(X, f)
        ref = _meamed_tie_avg_ref(X.float().cpu(), f)
        tol = dict(atol=1e-3, rtol=1e-3) if dtype == torch.float32 else dict(
            atol=2e-2, rtol=2e-2
        )
        assert torch.allclose(out.float().cpu(), ref, **tol), (
            f"max diff {(out.float().cpu() - ref).abs().max()}"
        )
        # and loosely against the true oracle (tie-policy differences only)
        oracle = F.mean_of_medians(X.float().cpu(), f)
        assert (out.float().cpu() - oracle).abs().max() < 0.1

    def test_trimmed_inf_rows(self):
        # +-inf byzantine rows must be trimmed away exactly (f on each end)
        X = _rand(256, 1024, torch.bfloat16, seed=13)
        X[1] = float("inf")
        X[2] = float("inf")
        X[3] = float("-inf")
        out = D.trimmed_mean(X, 4)
        ref = F.trimmed_mean(X.float().cpu(), 4)
        assert torch.isfinite(out.float().cpu()).all()
        assert torch.allclose(out.float().cpu(), ref, atol=2e-2, rtol=2e-2)

    def test_trimmed_ties_heavy(self):
        X = torch.ones(400, 512, dtype=torch.bfloat16, device="cuda")
        X[:100] = 2.0
        X[300:] = -1.0
        out = D.trimmed_mean(X, 110)
        ref = F.trimmed_mean(X.float().cpu(), 110)
        assert torch.allclose(out.float().cpu(), ref, atol=1e-3)


class TestGramSmallN:
    """Wave-slab small-n Gram kernels (gram.hip): exactly-once HBM traffic
    at n <= 32 via A==B fragment reuse and slab packing."""

    @pytest.mark.parametrize("n", [2, 4, 5, 8, 12, 16, 17, 24, 32])
    @pytest.mark.parametrize("dtype", DTYPES)
    def test_parity(self, n, dtype):
        X = _rand(n, 8192, dtype, seed=n * 7)
        G = D.gram(X)
        Xf = X.float()
        ref = Xf @ Xf.T
        tol = 1e-3 if dtype == torch.float32 else 0.3
        assert (G - ref).abs().max().item() < tol * max(
            1.0, ref.abs().max().item() / 100
        )

    @pytest.mark.parametrize("d", [64, 72, 1000, 2048, 100000])
    def test_tail_handling(self, d):
        # d values that exercise the partial final wave / sub-slab tails
        for dtype in DTYPES:
            if dtype == torch.bfloat16 and d % 8 != 0:
                continue  # bf16 small path requires d % 8 == 0 (falls back)
            X = _rand(8, d, dtype, seed=d % 97)
            G = D.gram(X)
            Xf = X.float()
            ref = Xf @ Xf.T
            tol = 1e-3 if dtype == torch.float32 else 0.3
            assert (G - ref).abs().max().item() < tol * max(
                1.0, ref.abs().max().item() / 100
            ), f"d={d} {dtype}"

    def test_asymmetric(self):
        # transpose-detecting data (guide §3) through the small-n path
        n, d = 12, 4096
        X = torch.zeros(n, d)
        for i in range(n):
            X[i, i] = i + 1.0
            X[i, (i * 13 + 7) % d] = 0.5 * (i + 3)
        X = X.cuda()
        G = D.gram(X)
        ref = X.float() @ X.float().T
        assert torch.allclose(G, ref, atol=1e-3)

    def test_small_n_krum_end_to_end(self):
        X = _rand(8, 100000, torch.bfloat16, seed=3)
        out = D.multi_krum(X, 1, 3)
        ref = F.multi_krum(X.float().cpu(), 1, 3)
        assert torch.allclose(out.float().cpu(), ref, atol=5e-2, rtol=5e-2)


class TestCafGraphAndFixedIters:
    """Round-2 iterative-op unblocking: hipGraph CAF blocks and poll-free
    geometric median."""

    def test_caf_graph_matches_eager(self, monkeypatch):
        X = _rand(24, 4096, torch.float32, seed=51)
        X[-4:] = 40.0
        monkeypatch.setenv("BYZPY_CAF_GRAPH", "1")
        got_graph = D.caf(X, 4)
        monkeypatch.setenv("BYZPY_CAF_GRAPH", "0")
        got_eager = D.caf(X, 4)
        assert torch.allclose(got_graph, got_eager, atol=1e-3, rtol=1e-3)

    def test_caf_graph_matches_cpu_oracle(self, monkeypatch):
        monkeypatch.setenv("BYZPY_CAF_GRAPH", "1")
        X = _rand(16, 2048, torch.float32, seed=52)
        X[0] = 25.0
        X[1] = -25.0
        got = D.caf(X, 2)
        ref = F.caf(X.cpu(), 2)
        assert (got.cpu() - ref).norm() < 0.05 * max(1.0, float(ref.norm()))

    def test_caf_graph_replay_is_stateless(self, monkeypatch):
        # two different inputs through the SAME cached graph must not leak
        monkeypatch.setenv("BYZPY_CAF_GRAPH", "1")
        X1 = _rand(16, 1024, torch.float32, seed=53)
        X2 = _rand(16, 1024, torch.float32, seed=54)
        a1 = D.caf(X1, 3).clone()
        _ = D.caf(X2, 3)
        a1_again = D.caf(X1, 3)
        assert torch.allclose(a1, a1_again)

    @pytest.mark.parametrize("dtype", DTYPES)
    def test_geomed_fixed_iters_parity(self, dtype):
        X = _rand(16, 2048, dtype, seed=55)
        out = D.geometric_median(X, fixed_iters=64)
        ref = F.geometric_median(X.float().cpu(), tol=1e-30, max_iter=64)
        assert (out.float().cpu() - ref).norm() < 0.05 * max(1.0, float(ref.norm()))

    def test_geomed_fixed_iters_capture_safe(self):
        # the poll-free path must capture into a hipGraph without error
        X = _rand(8, 4096, torch.bfloat16, seed=56)
        from byzpy_amd.hip.graphs import CapturedAggregate

        cap = CapturedAggregate(
            lambda Y: D.geometric_median(Y, fixed_iters=16), X
        )
        out = cap.run(X).clone()
        ref = D.geometric_median(X, fixed_iters=16)
        assert torch.allclose(out.float(), ref.float(), atol=1e-2, rtol=1e-2)



class TestRadixLowCrossover:
    """The radix engine now takes over from n > 64 when d >= 32768."""

    @pytest.mark.parametrize("n", [65, 100, 150, 192])
    def test_median_exact_both_dtypes(self, n):
        for dtype in DTYPES:
            X = _rand(n, 40000, dtype, seed=n)
            out = D.median(X)
            ref = F.median(X.float().cpu()).to(dtype)
            assert torch.equal(out.cpu(), ref), f"n={n} {dtype}"

    def test_trimmed_and_meamed_crossover_shapes(self):
        X = _rand(100, 40000, torch.bfloat16, seed=9)
        assert torch.allclose(
            D.trimmed_mean(X, 10).float().cpu(),
            F.trimmed_mean(X.float().cpu(), 10),
            atol=2e-2, rtol=2e-2,
        )
        out = D.mean_of_medians(X, 10)
        ref = _meamed_tie_avg_ref(X.float().cpu(), 10)
        assert torch.allclose(out.float().cpu(), ref, atol=2e-2, rtol=2e-2)


class TestDeviceSubsetSearch:
    """K11 device-side MDA/SMEA (subsets.hip): no host D2 copy, parity
    with the CPU oracles including lex-smallest tie-breaks."""

    @pytest.mark.parametrize("n,f", [(10, 3), (16, 4), (20, 6), (30, 10)])
    def test_mda_parity(self, n, f):
        X = _rand(n, 2048, torch.float32, seed=n * 3 + f)
        out = D.minimum_diameter_averaging(X, f)
        ref = F.minimum_diameter_averaging(X.cpu(), f)
        assert torch.allclose(out.cpu(), ref, atol=1e-4), f"n={n} f={f}"

    def test_mda_ties_all_equal(self):
        # all-equal rows: every subset has diameter 0; lex-smallest wins
        X = torch.ones(12, 256, device="cuda")
        out = D.minimum_diameter_averaging(X, 4)
        assert torch.allclose(out, torch.ones(256, device="cuda"))

    def test_mda_clustered(self):
        # 4 outliers far away: the tight cluster must be selected exactly
        g = torch.Generator().manual_seed(5)
        X = torch.randn(16, 512, generator=g).cuda()
        X[3] += 100.0
        X[7] -= 100.0
        X[11] += 50.0
        X[12] -= 50.0
        out = D.minimum_diameter_averaging(X, 4)
        ref = X[[i for i in range(16) if i not in (3, 7, 11, 12)]].mean(0)
        assert torch.allclose(out, ref, atol=1e-4)

    def test_mda_bf16(self):
        X = _rand(14, 1024, torch.bfloat16, seed=77)
        out = D.minimum_diameter_averaging(X, 4)
        ref = F.minimum_diameter_averaging(X.float().cpu(), 4)
        assert torch.allclose(out.float().cpu(), ref, atol=5e-2, rtol=5e-2)

    @pytest.mark.parametrize("n,f", [(10, 2), (12, 3), (16, 3)])
    def test_smea_parity(self, n, f):
        X = _rand(n, 1024, torch.float32, seed=n + f)
        out = D.smea(X, f)
        ref = F.smea(X.cpu(), f)
        assert torch.allclose(out.cpu(), ref, atol=1e-3), f"n={n} f={f}"

    def test_smea_outlier_rejection(self):
        g = torch.Generator().manual_seed(6)
        X = torch.randn(12, 768, generator=g).cuda()
        X[2] *= 50.0
        X[9] *= 50.0
        out = D.smea(X, 2)
        ref = F.smea(X.cpu(), 2)
        assert torch.allclose(out.cpu(), ref, atol=1e-3)

    def test_smea_bf16_device_class(self):
        from byzpy_amd.aggregators import SMEA

        X = _rand(12, 2048, torch.bfloat16, seed=8)
        out = SMEA(3).aggregate(list(X))
        assert out.is_cuda and out.dtype == torch.bfloat16
        ref = SMEA(3).aggregate([g.cpu().float() for g in X])
        assert (out.float().cpu() - ref).norm() / ref.norm().clamp_min(1e-6) < 0.02


class TestAttackKernels:
    """K14 attack math: fused Little pass + philox Gaussian fill."""

    @pytest.mark.parametrize("dtype", DTYPES)
    @pytest.mark.parametrize("n,d", [(10, 4097), (33, 1000), (64, 65536)])
    def test_little_parity(self, n, d, dtype):
        X = _rand(n, d, dtype, seed=n + d)
        out = D.little(X, 3)
        ref = F.little(X.float().cpu(), 3)
        tol = dict(atol=1e-3, rtol=1e-3) if dtype == torch.float32 else dict(
            atol=5e-2, rtol=5e-2
        )
        assert torch.allclose(out.float().cpu(), ref, **tol)

    def test_little_attack_class_on_device(self):
        from byzpy_amd.attacks import LittleAttack

        grads = [torch.randn(2048).cuda() for _ in range(12)]
        out = LittleAttack(3).apply(honest_grads=grads)
        assert out.is_cuda
        ref = F.little(torch.stack([g.cpu() for g in grads]), 3)
        assert torch.allclose(out.cpu(), ref, atol=1e-3)

    def test_gaussian_fill_statistics(self):
        like = torch.empty(1, device="cuda")
        out = D.gaussian_attack(
            torch.empty(1, 1_000_000, device="cuda"), 2.0, 3.0, seed=7
        )
        assert out.shape == (1_000_000,)
        assert abs(float(out.mean()) - 2.0) < 0.02
        assert abs(float(out.std()) - 3.0) < 0.02
        assert torch.isfinite(out).all()

    def test_gaussian_fill_deterministic_per_seed(self):
        t = torch.empty(1, 100_000, device="cuda")
        a = D.gaussian_attack(t, 0.0, 1.0, seed=13)
        b = D.gaussian_attack(t, 0.0, 1.0, seed=13)
        c = D.gaussian_attack(t, 0.0, 1.0, seed=14)
        assert torch.equal(a, b)
        assert not torch.equal(a, c)

    def test_gaussian_fill_bf16(self):
        t = torch.empty(1, 65536, device="cuda", dtype=torch.bfloat16)
        out = D.gaussian_attack(t, 0.0, 1.0, seed=3)
        assert out.dtype == torch.bfloat16
        assert abs(float(out.float().mean())) < 0.05


def test_geomed_warm_start_init_z():
    """init_z warm start: starting at the converged center stays there."""
    X = _rand(12, 4096, torch.bfloat16, seed=91)
    z0 = D.geometric_median(X, tol=1e-8, max_iter=300)
    z1 = D.geometric_median(X, fixed_iters=3, init_z=z0.float())
    assert torch.allclose(z0.float(), z1.float(), atol=1e-2, rtol=1e-2)
    # and from an arbitrary center it still converges toward the oracle
    z2 = D.geometric_median(
        X, fixed_iters=100, init_z=torch.zeros(4096, device="cuda")
    )
    ref = F.geometric_median(X.float().cpu(), tol=1e-8, max_iter=300)
    assert (z2.float().cpu() - ref).norm() < 0.05 * max(1.0, float(ref.norm()))


class TestGramF32Sym64:
    """Symmetric 3-tile f32 Gram for 32 < n <= 64."""

    @pytest.mark.parametrize("n", [33, 40, 48, 63, 64])
    def test_parity(self, n):
        X = _rand(n, 8192, torch.float32, seed=n)
        G = D.gram(X)
        ref = X @ X.T
        assert torch.allclose(G, ref, atol=1e-2, rtol=1e-4), f"n={n}"

    def test_asymmetric_structure(self):
        n, d = 50, 2048
        X = torch.zeros(n, d)
        for i in range(n):
            X[i, (i * 17) % d] = i + 1.0
            X[i, (i * 5 + 3) % d] = -0.25 * i
        X = X.cuda()
        G = D.gram(X)
        ref = X @ X.T
        assert torch.allclose(G, ref, atol=1e-3)

    def test_tail_d(self):
        X = _rand(64, 100001, torch.float32, seed=3)
        G = D.gram(X)
        ref = X @ X.T
        assert torch.allclose(G, ref, atol=0.05, rtol=1e-4)


class TestRadixCapEdges:
    """Boundary shapes for the radix engine: just past the LDS cap and at
    the 65535-row ceiling."""

    def test_n_513(self):
        X = _rand(513, 2000, torch.bfloat16, seed=513)
        assert torch.equal(
            D.median(X).cpu(), F.median(X.float().cpu()).bfloat16()
        )
        assert torch.allclose(
            D.trimmed_mean(X, 100).float().cpu(),
            F.trimmed_mean(X.float().cpu(), 100),
            atol=2e-2, rtol=2e-2,
        )

    def test_n_cap_65535(self):
        X = _rand(65535, 257, torch.bfloat16, seed=1)
        assert torch.equal(
            D.median(X).cpu(), F.median(X.float().cpu()).bfloat16()
        )

    def test_extreme_f(self):
        n = 401
        X = _rand(n, 2048, torch.float32, seed=7)
        f = (n - 1) // 2  # keeps exactly one coordinate
        out = D.trimmed_mean(X, f)
        ref = F.trimmed_mean(X.cpu(), f)
        assert torch.allclose(out.cpu(), ref, atol=1e-4)

    def test_above_cap_falls_back_to_torch(self):
        X = _rand(65600, 64, torch.bfloat16, seed=2)
        out = D.median(X)  # dispatch cap -> F.median on device
        ref = F.median(X.float().cpu()).bfloat16()
        assert torch.equal(out.cpu(), ref)


class TestFusedGramMedian:
    """One-pass gram+median (the flagship bench fusion)."""

    @pytest.mark.parametrize("n", [8, 16, 33, 48, 64])
    @pytest.mark.parametrize("d", [2048, 4097, 100000])
    def test_parity(self, n, d):
        X = _rand(n, d, torch.bfloat16, seed=n + d)
        med, G = D.median_and_gram(X)
        ref_med = F.median(X.float().cpu())
        Xf = X.float()
        ref_G = Xf @ Xf.T
        assert torch.allclose(med.float().cpu(), ref_med, atol=5e-2, rtol=5e-2)
        assert (G - ref_G).abs().max().item() < 0.3 * max(
            1.0, float(ref_G.abs().max()) / 100
        )

    def test_median_exact_vs_separate_kernel(self):
        # same keys, same averaging -> fused median must EQUAL D.median
        X = _rand(64, 250000, torch.bfloat16, seed=9)
        med, _ = D.median_and_gram(X)
        assert torch.equal(med, D.median(X))

    def test_with_inf_rows(self):
        X = _rand(64, 8192, torch.bfloat16, seed=11)
        X[3] = float("inf")
        X[5] = float("-inf")
        med, G = D.median_and_gram(X)
        assert torch.equal(med, D.median(X))

    def test_sharded_fused_matches_separate(self):
        from byzpy_amd.parallel import sharded

        X = _rand(64, 100000, torch.bfloat16, seed=13)
        med, krum_out = sharded.median_and_multi_krum(X, 16, 12)
        assert torch.equal(med, sharded.median(X))
        assert torch.equal(krum_out, sharded.multi_krum(X, 16, 12))


class TestGroupedOps:
    """Grouped gossip kernels: all nodes' aggregates per launch."""

    @pytest.mark.parametrize("dtype", DTYPES)
    def test_grouped_weiszfeld_matches_per_group(self, dtype):
        g = torch.Generator().manual_seed(21)
        X3 = torch.randn(6, 5, 4096, generator=g).to("cuda", dtype)
        Z = D.geometric_median_grouped(X3, iters=12)
        for i in range(6):
            zi = D.geometric_median(X3[i], fixed_iters=12)
            assert torch.allclose(Z[i], zi.float(), atol=1e-2, rtol=1e-2), i

    def test_grouped_weiszfeld_warm_start(self):
        g = torch.Generator().manual_seed(22)
        X3 = torch.randn(4, 7, 2048, generator=g).cuda()
        Z0 = D.geometric_median_grouped(X3, iters=100)
        Z1 = D.geometric_median_grouped(X3, iters=2, init_z=Z0)
        assert torch.allclose(Z0, Z1, atol=1e-3)

    def test_nnm_grouped_matches_per_group(self):
        g = torch.Generator().manual_seed(23)
        X3 = torch.randn(5, 6, 1024, generator=g).to("cuda", torch.bfloat16)
        out = D.nnm_grouped(X3, 2)
        for i in range(5):
            ref = D.nnm(X3[i], 2)
            assert torch.allclose(
                out[i].float(), ref.float(), atol=5e-2, rtol=5e-2
            ), i

    def test_grouped_cpu_fallback(self):
        g = torch.Generator().manual_seed(24)
        X3 = torch.randn(3, 5, 257, generator=g)
        Z = D.geometric_median_grouped(X3, iters=30)
        for i in range(3):
            zi = D.geometric_median(X3[i], fixed_iters=30)
            assert torch.allclose(Z[i], zi.float(), atol=1e-4), i


@pytest.mark.gpu
class TestMedianSelectionAllN:
    """Exhaustive n sweep for the selection-network median (the pad-split
    epilogue maps every n <= P onto fixed ranks P/2-1 / P/2 — each n
    exercises a different pad count L, so cover them all)."""

    def test_every_n_to_64(self):
        g = torch.Generator().manual_seed(123)
        for dtype in (torch.bfloat16, torch.float32):
            for n in range(1, 65):
                X = torch.randn(n, 4096, generator=g).to("cuda", dtype)
                out = D.median(X)
                ref = F.median(X.float().cpu()).to(dtype)
                assert torch.equal(out.cpu(), ref), (dtype, n)

    def test_every_n_with_infs(self):
        g = torch.Generator().manual_seed(7)
        for n in range(2, 65, 5):
            X = torch.randn(n, 2048, generator=g).to("cuda", torch.bfloat16)
            X[0] = float("inf")
            X[n - 1] = float("-inf")
            out = D.median(X)
            ref = F.median(X.float().cpu()).to(torch.bfloat16)
            # n=2 averages +inf and -inf to NaN on both paths: NaN-aware
            assert torch.allclose(
                out.float().cpu(), ref.float(), atol=0, rtol=0, equal_nan=True
            ), n



@pytest.mark.gpu
class TestCafPipelineParity:
    """The CAF eager loop pipelines its break-condition readback one round
    deep and stages seeds through pinned memory; BYZPY_CAF_SYNC=1 recovers
    the fully synchronous loop. The two must be BITWISE equal — the
    pipeline only moves host waits, never changes a computed value.
    (Shapes stay at d <= 65536 where caf_matvec is single-owner per row;
    larger d splits k and is only ulp-stable — see TestDeterminism.)"""

    def test_sync_equals_pipelined(self, monkeypatch):
        g = torch.Generator().manual_seed(99)
        for (n, d, f) in [(64, 65536, 16), (33, 10000, 9), (128, 4096, 40)]:
            X = torch.randn(n, d, generator=g).to("cuda")
            monkeypatch.setenv("BYZPY_CAF_SYNC", "1")
            ref = D.caf(X, f)
            monkeypatch.delenv("BYZPY_CAF_SYNC")
            out = D.caf(X, f)
            assert torch.equal(out, ref), (n, d, f)


@pytest.mark.gpu
class TestDeterminism:
    """Every device op must be bitwise run-to-run deterministic on the
    same input (the engines' seeded-rng replay contract depends on it —
    e.g. split-K Gram must reduce in a fixed order, not via racing
    atomics)."""

    def test_ops_bitwise_stable(self):
        g = torch.Generator().manual_seed(41)
        X = torch.randn(64, 200_000, generator=g).to("cuda", torch.bfloat16)
        Xf = X.float()
        X512 = torch.randn(512, 40_000, generator=g).to("cuda", torch.bfloat16)
        ops = [
            ("median", lambda: D.median(X)),
            ("trimmed", lambda: D.trimmed_mean(X, 8)),
            ("meamed", lambda: D.mean_of_medians(X, 8)),
            ("multi_krum", lambda: D.multi_krum(X, 8, 4)),
            ("cge", lambda: D.cge(X, 8)),
            ("nnm", lambda: D.nnm(X, 8)),
            ("rsel_median", lambda: D.median(X512)),
            ("rsel_trimmed", lambda: D.trimmed_mean(X512, 64)),
            ("rsel_meamed", lambda: D.mean_of_medians(X512, 64)),
        ]
        for name, fn in ops:
            a, b = fn(), fn()
            assert torch.equal(a, b), f"{name} is not run-to-run deterministic"

    def test_atomic_reduction_ops_are_ulp_stable(self):
        """The TWO ops whose k-slab partials land via f32 atomicAdd in
        hardware order are allowed bounded run-to-run drift — that
        design is what reaches the HBM floor:
        - gram: split-K image, a few f32 ulp in G;
        - geometric_median / cc / caf: their distance/matvec passes
          split k above a d threshold and can flip the final output
          rounding (geomed measured max drift 2e-3 = one bf16 ulp,
          flat in iteration count; caf/cc measure bitwise-stable at
          d <= 65k but not structurally guaranteed at larger d).
        Everything downstream of gram SELECTS (Krum, cge), which only
        flips on exact ties the engines never rely on."""
        g = torch.Generator().manual_seed(42)
        X = torch.randn(64, 200_000, generator=g).to("cuda", torch.bfloat16)
        for name, fn, tol in [
            ("gram", lambda: D.gram(X), 1e-5),
            ("gram_f32", lambda: D.gram(X.float()), 1e-5),
            ("geomed", lambda: D.geometric_median(X, fixed_iters=8), 6e-3),
            ("cc", lambda: D.centered_clipping(X, c_tau=0.5, M=5), 1e-4),
            ("caf", lambda: D.caf(X.float(), 8), 1e-3),
        ]:
            a, b = fn(), fn()
            scale = max(1.0, float(a.abs().max()))
            assert torch.allclose(
                a.float(), b.float(), atol=tol * scale, rtol=1e-5
            ), f"{name} drifted beyond ulp scale"


# -- binding layer: dtype / vector-width selection and the LDS row cap -------
# Every _hip_ops binding that takes an (n, d) matrix, called directly at
# n = 5 in both dtypes: d = 33 is no multiple of either vector width (4 f32
# / 8 bf16 lanes -> scalar kernels, and odd d keeps bf16 colsel off the
# packed path); d = 64 takes the vector kernels. References run on the CPU
# copy of the (dtype-rounded) input.

_SMALL_N = 5
_SMALL_SEED = 22  # no exact |x - med| ties at the MEAMED window boundary


def _wz_step(Xf, z, eps=1e-12):
    w = 1.0 / (Xf - z[None, :]).norm(dim=1).clamp_(min=eps)
    return (w[:, None] * Xf).sum(dim=0) / w.sum()


def _cc_step(Xf, v, c_tau, eps=1e-12):
    diff = Xf - v[None, :]
    alpha = torch.clamp(c_tau / diff.norm(dim=1).clamp_(min=eps), max=1.0)
    return v + (alpha[:, None] * diff).sum(dim=0) / Xf.shape[0]


def _small_cases():
    """name -> (binding call on device inputs, reference on CPU inputs).
    Each takes (ext, X, aux) / (Xf, aux); aux holds the shared f32 vectors."""
    idx = [3, 0, 4]
    gidx = [[0, 1, 2], [4, 4, 1]]
    perm = [2, 0, 4, 1, 3]

    def dev_i32(v, like):
        return torch.tensor(v, dtype=torch.int32, device=like.device)

    def shift(like):
        return torch.zeros((), device=like.device)

    return {
        "colsel_median": (
            lambda e, X, a: e.colsel(X, 0, 0), lambda Xf, a: F.median(Xf)),
        "colsel_trimmed": (
            lambda e, X, a: e.colsel(X, 1, 1), lambda Xf, a: F.trimmed_mean(Xf, 1)),
        "colsel_meamed": (
            lambda e, X, a: e.colsel(X, 2, 1),
            lambda Xf, a: F.mean_of_medians(Xf, 1)),
        "row_sqnorms": (
            lambda e, X, a: e.row_sqnorms(X), lambda Xf, a: (Xf * Xf).sum(dim=1)),
        "row_center_sqdists": (
            lambda e, X, a: e.row_center_sqdists(X, a["z"]),
            lambda Xf, a: ((Xf - a["z"][None, :]) ** 2).sum(dim=1)),
        "row_scale": (
            lambda e, X, a: e.row_scale(X, a["s"]),
            lambda Xf, a: Xf * a["s"][:, None]),
        "mean_rows": (
            lambda e, X, a: e.mean_rows(X, dev_i32(idx, X)),
            lambda Xf, a: Xf[idx].mean(dim=0)),
        "group_mean_rows": (
            lambda e, X, a: e.group_mean_rows(X, dev_i32(gidx, X)),
            lambda Xf, a: Xf[torch.tensor(gidx)].mean(dim=1)),
        "bucket_mean": (
            lambda e, X, a: e.bucket_mean(X, dev_i32(perm, X), 2),
            lambda Xf, a: F.bucketing(Xf, 2, perm)),
        "gram": (lambda e, X, a: e.gram(X), lambda Xf, a: Xf @ Xf.T),
        "weiszfeld_iter": (
            lambda e, X, a: e.weiszfeld_iter(X, a["z"], 1e-12, shift(X)),
            lambda Xf, a: _wz_step(Xf, a["z"])),
        "weiszfeld_apply": (
            lambda e, X, a: e.weiszfeld_apply(
                X, a["z"], e.row_center_sqdists(X, a["z"]), 1e-12, shift(X)),
            lambda Xf, a: _wz_step(Xf, a["z"])),
        "cc_iter": (
            lambda e, X, a: e.cc_iter(X, a["z"], 0.7, 1e-12),
            lambda Xf, a: _cc_step(Xf, a["z"], 0.7)),
        "cc_apply": (
            lambda e, X, a: e.cc_apply(
                X, a["z"], e.row_center_sqdists(X, a["z"]), 0.7, 1e-12),
            lambda Xf, a: _cc_step(Xf, a["z"], 0.7)),
        "caf_matvec": (
            lambda e, X, a: e.caf_matvec(X, a["z"], a["v"]),
            lambda Xf, a: (Xf - a["z"][None, :]) @ a["v"]),
        "caf_colsum": (
            lambda e, X, a: e.caf_colsum(X, a["s"], a["z"], a["scale"]),
            lambda Xf, a: a["scale"]
            * (a["s"][:, None] * (Xf - a["z"][None, :])).sum(dim=0)),
        "caf_colsum_plain": (
            lambda e, X, a: e.caf_colsum(X, a["s"]),
            lambda Xf, a: (a["s"][:, None] * Xf).sum(dim=0)),
        "little_fused": (
            lambda e, X, a: e.little_fused(X, 1.5),
            lambda Xf, a: Xf.mean(dim=0) + 1.5 * Xf.std(dim=0, unbiased=False)),
    }


_SMALL_CASES = _small_cases()


@pytest.fixture(scope="module")
def small_inputs():
    """(d, dtype) -> (X on device, X.float() on CPU, aux on device, aux on
    CPU); built once, never modified."""
    out = {}
    for d in (33, 64):
        g = torch.Generator().manual_seed(_SMALL_SEED + d)
        aux = {
            "z": torch.randn(d, generator=g),
            "v": torch.randn(d, generator=g),
            "s": torch.rand(_SMALL_N, generator=g) + 0.5,
            "scale": torch.tensor(0.25),
        }
        aux_dev = {k: v.cuda() for k, v in aux.items()}
        for dtype in DTYPES:
            X = _rand(_SMALL_N, d, dtype, seed=_SMALL_SEED)
            out[d, dtype] = (X, X.float().cpu(), aux_dev, aux)
    return out


@pytest.mark.parametrize("d", [33, 64])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", sorted(_SMALL_CASES))
def test_binding_small_n_both_dtypes_both_widths(small_inputs, op, dtype, d):
    from byzpy_amd.hip import require

    X, Xf, aux_dev, aux = small_inputs[d, dtype]
    if op == "colsel_meamed":  # precondition: the kept window is unambiguous
        dev = (Xf - F.median(Xf)[None, :]).abs().sort(dim=0).values
        assert (dev[_SMALL_N - 1] > dev[_SMALL_N - 2]).all()
    run, ref = _SMALL_CASES[op]
    out = run(require(), X, aux_dev)
    expect = ref(Xf, aux)
    assert out.shape == expect.shape
    assert torch.allclose(out.float().cpu(), expect, **_tol(dtype)), (
        f"{op} d={d} {dtype}: max err "
        f"{(out.float().cpu() - expect).abs().max().item():.3e}"
    )


@pytest.mark.parametrize("d", [33, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_binding_grouped_weiszfeld_small(dtype, d):
    from byzpy_amd.hip import require

    g = torch.Generator().manual_seed(_SMALL_SEED)
    X3 = torch.randn(2, 3, d, generator=g).to("cuda", dtype)
    Z = torch.randn(2, d, generator=g)
    out = require().weiszfeld_iter_grouped(X3, Z.cuda(), 1e-12)
    X3f = X3.float().cpu()
    expect = torch.stack([_wz_step(X3f[i], Z[i]) for i in range(2)])
    assert torch.allclose(out.cpu(), expect, **_tol(dtype))


# -- rowops loop nests beyond the n = 5 cases ---------------------------------
# The cases above use n = 5 and 3-entry index lists, so the column-sum
# kernels only run their one-row tail loop there and the row-group kernels
# see a single group. These reach the 4-row unrolled block plus a tail
# through every row map, a second row group (37 = 32 + 4 + 1), every
# accumulator slot of the grouped path (m = 32), and a second column
# grid-stride step (more than 4096 blocks x 256 threads of work).

_IDX6 = [7, 0, 3, 8, 3, 5]  # 4 + 2, row 3 twice
_GIDX_3x5 = [[0, 1, 2, 3, 4], [8, 8, 2, 6, 1], [5, 7, 0, 4, 4]]
_GIDX_5x5 = _GIDX_3x5 + [[6, 3, 1, 8, 0], [2, 2, 2, 7, 5]]  # g > 4: other grid
_PERM9 = [4, 0, 8, 2, 6, 1, 7, 3, 5]  # bucket = 5 -> buckets of 5 and 4


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


_INDEX_MAP_CASES = {
    "mean_rows": (
        lambda e, X: e.mean_rows(X, _i32(_IDX6)),
        lambda Xf: Xf[_IDX6].mean(dim=0)),
    "group_mean_rows_3x5": (
        lambda e, X: e.group_mean_rows(X, _i32(_GIDX_3x5)),
        lambda Xf: Xf[torch.tensor(_GIDX_3x5)].mean(dim=1)),
    "group_mean_rows_5x5": (
        lambda e, X: e.group_mean_rows(X, _i32(_GIDX_5x5)),
        lambda Xf: Xf[torch.tensor(_GIDX_5x5)].mean(dim=1)),
    "bucket_mean": (
        lambda e, X: e.bucket_mean(X, _i32(_PERM9), 5),
        lambda Xf: F.bucketing(Xf, 5, _PERM9)),
}


@pytest.fixture(scope="module")
def rowops_inputs():
    """(n, d, dtype) -> (X on device, X.float() on CPU) for n = 9 and n = 37;
    built once, never modified."""
    out = {}
    for n in (9, 37):
        for d in (33, 64):
            for dtype in DTYPES:
                X = _rand(n, d, dtype, seed=_SMALL_SEED + n)
                out[n, d, dtype] = (X, X.float().cpu())
    return out


def _assert_close(out, expect, dtype, what):
    assert out.shape == expect.shape, what
    err = (out.float().cpu() - expect).abs().max().item()
    print(f"{what}: max err {err:.3e}")
    assert torch.allclose(out.float().cpu(), expect, **_tol(dtype)), (
        f"{what}: max err {err:.3e}")


@pytest.mark.parametrize("d", [33, 64])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", sorted(_INDEX_MAP_CASES))
def test_binding_index_maps_unrolled_block_plus_tail(rowops_inputs, op, dtype, d):
    from byzpy_amd.hip import require

    X, Xf = rowops_inputs[9, d, dtype]
    run, ref = _INDEX_MAP_CASES[op]
    _assert_close(run(require(), X), ref(Xf), dtype, f"{op} n=9 d={d} {dtype}")


@pytest.mark.parametrize("m,d", [(6, 33), (6, 64), (32, 33), (32, 64)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_binding_grouped_weiszfeld_unrolled_and_full_group(dtype, m, d):
    """G = 2 groups of m = 6 (4 + 2) rows, and of m = 32, the grouped
    path's cap, where every accumulator slot is live."""
    from byzpy_amd.hip import require

    g = torch.Generator().manual_seed(_SMALL_SEED + m)
    X3 = torch.randn(2, m, d, generator=g).to("cuda", dtype)
    Z = torch.randn(2, d, generator=g)
    out = require().weiszfeld_iter_grouped(X3, Z.cuda(), 1e-12)
    X3f = X3.float().cpu()
    expect = torch.stack([_wz_step(X3f[i], Z[i]) for i in range(2)])
    _assert_close(out, expect, dtype, f"weiszfeld_iter_grouped m={m} d={d} {dtype}")


@pytest.mark.parametrize("d", [33, 64])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", ["row_center_sqdists", "caf_matvec"])
def test_binding_row_group_boundary(rowops_inputs, op, dtype, d):
    """n = 37: two row groups, the second with 4 + 1 rows."""
    from byzpy_amd.hip import require

    X, Xf = rowops_inputs[37, d, dtype]
    g = torch.Generator().manual_seed(_SMALL_SEED + d)
    z = torch.randn(d, generator=g)
    v = torch.randn(d, generator=g)
    if op == "row_center_sqdists":
        out = require().row_center_sqdists(X, z.cuda())
        expect = ((Xf - z[None, :]) ** 2).sum(dim=1)
    else:
        out = require().caf_matvec(X, z.cuda(), v.cuda())
        expect = (Xf - z[None, :]) @ v
    _assert_close(out, expect, dtype, f"{op} n=37 d={d} {dtype}")


_COL_THREADS = 4096 * 256  # col_grid's cap: one column step covers this many


@pytest.mark.parametrize(
    "op,dtype,d",
    [
        ("mean_rows", torch.bfloat16, 8 * _COL_THREADS + 8 * 256),
        ("caf_colsum_plain", torch.float32, 4 * _COL_THREADS + 4 * 256),
        ("caf_colsum_plain", torch.float32, _COL_THREADS + 257),  # scalar path
    ],
)
def test_binding_column_grid_stride_wrap(op, dtype, d):
    """More work items than col_grid's 4096 x 256 threads: the first threads
    take a second column step."""
    from byzpy_amd.hip import require

    X = _rand(_SMALL_N, d, dtype, seed=_SMALL_SEED)
    Xf = X.float().cpu()
    if op == "mean_rows":
        idx = [3, 0, 4]
        out = require().mean_rows(X, _i32(idx))
        expect = Xf[idx].mean(dim=0)
    else:
        s = torch.rand(_SMALL_N, generator=torch.Generator().manual_seed(d)) + 0.5
        out = require().caf_colsum(X, s.cuda())
        expect = (s[:, None] * Xf).sum(dim=0)
    _assert_close(out, expect, dtype, f"{op} n={_SMALL_N} d={d} {dtype}")


def test_lds_row_cap_rejected_by_every_lds_staging_binding():
    """weiszfeld_update / cc_update / caf_colsum stage one weight per row in
    a 1024-float LDS array: all five bindings that launch them must refuse
    n = 1025 (by name) instead of writing past it."""
    from byzpy_amd.hip import require

    ext = require()
    n, d = 1025, 8
    X = _rand(n, d)
    z = torch.zeros(d, device="cuda")
    dist2 = torch.ones(n, device="cuda")
    a = torch.ones(n, device="cuda")
    shift = torch.zeros((), device="cuda")
    calls = {
        "weiszfeld_iter": lambda: ext.weiszfeld_iter(X, z, 1e-12, shift),
        "weiszfeld_apply": lambda: ext.weiszfeld_apply(X, z, dist2, 1e-12, shift),
        "cc_iter": lambda: ext.cc_iter(X, z, 0.7, 1e-12),
        "cc_apply": lambda: ext.cc_apply(X, z, dist2, 0.7, 1e-12),
        "caf_colsum": lambda: ext.caf_colsum(X, a),
    }
    for op, call in calls.items():
        with pytest.raises(RuntimeError, match=rf"\b{op} supports n <= 1024"):
            call()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sharded_iterative_ops_above_lds_row_cap(dtype):
    """One rank, n = 1025 > the fused kernels' row cap: the d-sharded
    geometric median and centered clipping must take their torch formulas
    on device and agree with the same functions on the CPU copy."""
    from byzpy_amd.parallel import sharded as S

    X = _rand(1025, 16, dtype, seed=12)
    Xc = X.cpu()
    out = S.geometric_median(X, fixed_iters=4)
    ref = S.geometric_median(Xc, fixed_iters=4)
    assert out.is_cuda and out.dtype == dtype
    assert (out.float().cpu() - ref.float()).norm() < 0.05 * max(
        1.0, ref.float().norm().item()
    )
    out = S.centered_clipping(X, c_tau=0.7, M=3)
    ref = S.centered_clipping(Xc, c_tau=0.7, M=3)
    assert out.is_cuda and out.dtype == dtype
    assert (out.float().cpu() - ref.float()).norm() < 0.05 * max(
        1.0, ref.float().norm().item()
    )
