"""AFA on the GPU: the one-launch selection on the MFMA Gram and the weighted
counted gather-mean, each against a reference on the same values, then the
end-to-end rule against the oracle in ops/functional.py.

A selection off an f32 Gram can only equal the f64 oracle's where no decision
is close, so every parametrised case first ASSERTS the oracle's own margin
(_afa_cases.margin, >= 1e-3) before it compares; a failure of that assertion
is a bad fixture, not a kernel failure."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _afa_cases as C
from byzpy_amd.aggregators import AFA
from byzpy_amd.hip import dispatch as D
from byzpy_amd.hip import require
from byzpy_amd.hip.graphs import CapturedAggregate
from byzpy_amd.ops import functional as F

DTYPES = [torch.float32, torch.bfloat16]
CASES = [(v, n, f, d) for v in C.VARIANTS for (n, f, d) in C.SHAPES]


@pytest.fixture(scope="module")
def ext():
    return require()


def _tol(dtype):  # as in test_gpu_kernels.py
    return dict(atol=1e-4, rtol=1e-4) if dtype == torch.float32 else dict(atol=5e-2, rtol=5e-2)


def _ones(n):
    return torch.ones(n, device="cuda")


@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
@pytest.mark.parametrize("variant,n,f,d", CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_selection_and_aggregate_against_the_oracle(ext, variant, n, f, d, dtype, weighted):
    k = C.case(variant, n, f, d, dtype, weighted)
    print(f"margin {k['margin']:.3e} rounds {k['rounds']} lower {k['lower']}")
    assert k["margin"] >= C.MIN_MARGIN, k["margin"]
    Xd = k["X"].cuda()
    w = None if k["w"] is None else k["w"].cuda()

    # the binding on the device Gram: set, order, padding, pass count
    G = D.gram(Xd)
    idx, count, rounds = ext.smea_select(
        G, weights=_ones(n) if w is None else w, xi=2.0, delta_xi=0.5
    )
    assert idx.shape == (n,) and idx.dtype == torch.int32
    assert count.dim() == 0 and count.dtype == torch.int32
    assert rounds.dim() == 0 and rounds.dtype == torch.int32
    cnt = int(count)
    assert idx[:cnt].tolist() == torch.nonzero(k["good"]).flatten().tolist()
    assert bool((idx[cnt:] == 0).all())
    assert int(rounds) == k["rounds"]

    # same bits on a second call
    idx2, count2, rounds2 = ext.smea_select(
        G, weights=_ones(n) if w is None else w, xi=2.0, delta_xi=0.5
    )
    assert torch.equal(idx, idx2) and torch.equal(count, count2)
    assert torch.equal(rounds, rounds2)

    # dispatch: mask exactly, aggregate within the project's tolerance
    assert torch.equal(D.afa_select(Xd, w).cpu(), k["good"])
    out = D.afa(Xd, w)
    assert out.dtype == dtype and out.is_cuda and out.shape == (d,)
    assert torch.allclose(out.float().cpu(), k["out"].float(), **_tol(dtype))
    assert torch.equal(D.afa(Xd, w), out)


@pytest.mark.parametrize("d", [33, 2050, 1024])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_weighted_counted_mean(ext, dtype, d):
    g = torch.Generator().manual_seed(d)
    n = 23
    X = torch.randn(n, d, generator=g).to(dtype)
    w = (0.5 + torch.rand(n, generator=g)).float()
    Xp = X.clone()
    Xp[7] = float("inf")  # a row the count leaves out must not reach the result
    Xd, Xpd, wd = X.cuda(), Xp.cuda(), w.cuda()
    idx = torch.tensor([3, 1, 22, 0, 5, 7, 7], dtype=torch.int32, device="cuda")
    for cnt in (0, 1, 5):
        count = torch.tensor(cnt, dtype=torch.int32, device="cuda")
        out = ext.mean_rows(Xpd, idx, count=count, weights=wd)
        assert out.dtype == dtype and out.shape == (d,)
        if cnt == 0:
            assert torch.equal(out, torch.zeros_like(out))
            continue
        rows = idx[:cnt].long().cpu()
        ref = (w[rows, None] * X.float()[rows]).sum(dim=0) / w[rows].sum()
        assert torch.allclose(out.float().cpu(), ref, **_tol(dtype))
        assert torch.equal(out, ext.mean_rows(Xpd, idx, count=count, weights=wd))
    # unit weights: the weighted mean is the plain one
    count = torch.tensor(5, dtype=torch.int32, device="cuda")
    plain = ext.mean_rows(Xd, idx, count=count)
    ones = ext.mean_rows(Xd, idx, count=count, weights=_ones(n))
    assert torch.allclose(ones.float(), plain.float(), **_tol(dtype))
    # the un-weighted counted form is bitwise what it was: mean_rows on idx[:count]
    assert torch.equal(plain, ext.mean_rows(Xd, idx[:5].contiguous()))
    # a zero weight sum writes zeros and reads no row
    zero = ext.mean_rows(Xpd, idx, count=torch.tensor(7, dtype=torch.int32, device="cuda"),
                         weights=torch.zeros(n, device="cuda"))
    assert torch.equal(zero, torch.zeros_like(zero))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_degenerate_inputs(ext, dtype):
    k = C.case("flip", 23, 3, 2050, dtype)
    X = k["X"]
    # identical rows return that row. (Which of them are kept is not fixed:
    # the entries of the device Gram differ in their last bits, the cosines
    # with them, and against an sd of that size some lie past the threshold.)
    same = X[:1].repeat(9, 1).cuda()
    assert torch.allclose(D.afa(same).float(), same[0].float(), **_tol(dtype))
    assert bool(D.afa_select(same).any())
    # an inf / NaN row is never kept, and does not reach the result
    for poison in (float("inf"), float("nan")):
        Xp = X.clone()
        victim = int(torch.nonzero(k["good"]).flatten()[2])
        Xp[victim, 5] = poison
        good, trace = F.afa_trace(Xp.float())
        assert C.margin(trace) >= C.MIN_MARGIN
        assert not bool(good[victim])
        assert torch.equal(D.afa_select(Xp.cuda()).cpu(), good)
        out = D.afa(Xp.cuda())
        assert bool(torch.isfinite(out).all())
        assert torch.allclose(out.float().cpu(), F.afa(Xp).float(), **_tol(dtype))
    # all weights zero: nothing alive, zeros, no pass
    Xd = X.cuda()
    zeros = torch.zeros(23, device="cuda")
    assert torch.equal(D.afa(Xd, zeros), torch.zeros(2050, dtype=dtype, device="cuda"))
    idx, count, rounds = ext.smea_select(D.gram(Xd), weights=zeros, xi=2.0, delta_xi=0.5)
    assert int(count) == 0 and int(rounds) == 0 and bool((idx == 0).all())
    # n = 1
    one = X[:1].cuda()
    assert torch.equal(D.afa(one), one[0])
    idx, count, rounds = ext.smea_select(D.gram(one), weights=_ones(1), xi=2.0, delta_xi=0.5)
    assert idx.tolist() == [0] and int(count) == 1 and int(rounds) == 1
    # a zero row has cosine 0 by definition and the kernel divides by nothing
    Xz = X.clone()
    Xz[4] = 0
    good, trace = F.afa_trace(Xz.float())
    assert C.margin(trace) >= C.MIN_MARGIN
    assert torch.equal(D.afa_select(Xz.cuda()).cpu(), good)


@pytest.mark.parametrize("variant", ["flip", "collude"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_n_129_takes_the_torch_path(ext, dtype, variant):
    n, f, d = C.OVER_CAP
    assert n > D.AFA_MAX_N
    k = C.case(variant, n, f, d, dtype)
    assert k["margin"] >= C.MIN_MARGIN, k["margin"]
    Xd = k["X"].cuda()
    with pytest.raises(RuntimeError):
        ext.smea_select(D.gram(Xd), weights=_ones(n), xi=2.0, delta_xi=0.5)
    assert torch.equal(D.afa_select(Xd).cpu(), k["good"])
    assert torch.allclose(D.afa(Xd).float().cpu(), k["out"].float(), **_tol(dtype))


def test_binding_rejects_bad_arguments(ext):
    G = D.gram(torch.randn(8, 100, device="cuda"))
    w = _ones(8)
    ok = dict(weights=w, xi=2.0, delta_xi=0.5)
    ext.smea_select(G, **ok)
    with pytest.raises(RuntimeError):  # host Gram
        ext.smea_select(G.cpu(), **ok)
    with pytest.raises(RuntimeError):  # host weights
        ext.smea_select(G, weights=w.cpu(), xi=2.0, delta_xi=0.5)
    with pytest.raises(RuntimeError):  # f64 Gram
        ext.smea_select(G.double(), **ok)
    with pytest.raises(RuntimeError):  # f64 weights
        ext.smea_select(G, weights=w.double(), xi=2.0, delta_xi=0.5)
    with pytest.raises(RuntimeError):  # not square
        ext.smea_select(G[:, :7].contiguous(), **ok)
    with pytest.raises(RuntimeError):  # three dimensions
        ext.smea_select(G[None].contiguous(), **ok)
    with pytest.raises(RuntimeError):  # weights of another length
        ext.smea_select(G, weights=_ones(7), xi=2.0, delta_xi=0.5)
    with pytest.raises(RuntimeError):  # weights of another shape
        ext.smea_select(G, weights=torch.ones(2, 4, device="cuda"), xi=2.0, delta_xi=0.5)
    with pytest.raises(RuntimeError):  # n = 0
        ext.smea_select(torch.zeros(0, 0, device="cuda"), weights=_ones(0), xi=2.0, delta_xi=0.5)
    with pytest.raises(RuntimeError):  # n = 129
        ext.smea_select(torch.zeros(129, 129, device="cuda"), weights=_ones(129), xi=2.0, delta_xi=0.5)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(RuntimeError):
            ext.smea_select(G, weights=w, xi=bad, delta_xi=0.5)
        with pytest.raises(RuntimeError):
            ext.smea_select(G, weights=w, xi=2.0, delta_xi=bad)
    if torch.cuda.device_count() > 1:  # a device mismatch
        with pytest.raises(RuntimeError):
            ext.smea_select(G, weights=w.to("cuda:1"), xi=2.0, delta_xi=0.5)
    # the weighted counted mean
    X = torch.randn(8, 100, device="cuda")
    idx = torch.arange(4, dtype=torch.int32, device="cuda")
    cnt = torch.tensor(2, dtype=torch.int32, device="cuda")
    ext.mean_rows(X, idx, count=cnt, weights=w)
    with pytest.raises(RuntimeError):  # one weight per row of X
        ext.mean_rows(X, idx, count=cnt, weights=_ones(4))
    with pytest.raises(RuntimeError):  # host weights
        ext.mean_rows(X, idx, count=cnt, weights=w.cpu())
    with pytest.raises(RuntimeError):  # f64 weights
        ext.mean_rows(X, idx, count=cnt, weights=w.double())
    with pytest.raises(RuntimeError):  # host count
        ext.mean_rows(X, idx, count=cnt.cpu(), weights=w)
    # the two older forms of smea_select still answer
    combos = torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32, device="cuda")
    assert ext.smea_select(G, combos).shape == (1,)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_graph_capture_replays_to_the_eager_result(dtype):
    # capture fails on any host sync, so a replay that matches is the proof
    # that the fused path has none
    k0 = C.case("flip", 64, 9, 1030, dtype)
    k1 = C.case("collude", 64, 9, 1030, dtype)
    X0, X1 = k0["X"].cuda(), k1["X"].cuda()
    cap = CapturedAggregate(lambda X: D.afa(X), X0)
    out1 = cap.run(X1)
    assert torch.equal(out1, D.afa(X1))
    assert torch.allclose(out1.float().cpu(), k1["out"].float(), **_tol(dtype))
    assert not torch.allclose(out1.float(), D.afa(X0).float(), **_tol(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_operator_on_device_list_and_matrix(dtype):
    k = C.case("tiers", 23, 3, 2050, dtype, True)
    Xd = k["X"].cuda()
    agg = AFA(weights=k["w"])
    for grads in (list(Xd), Xd):
        out = agg.aggregate(grads)
        assert out.dtype == dtype and out.is_cuda and out.shape == (2050,)
        assert torch.allclose(out.float().cpu(), k["out"].float(), **_tol(dtype))
    agg.weights = None
    ref = C.case("tiers", 23, 3, 2050, dtype)["out"]
    assert torch.allclose(agg.aggregate(Xd).float().cpu(), ref.float(), **_tol(dtype))
