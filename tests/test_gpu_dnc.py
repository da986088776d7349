"""DnC on the GPU: the sampled centred Gram, the spectral selection and the
counted gather-mean each against a reference on the same values, then the
end-to-end rule against the oracle in ops/functional.py.

The selection comparison only means something where the scores around the
keep boundary are separated, so the inputs spread the rows along one
direction (t_i = i^2 / n) and every case ASSERTS the oracle's relative gap
at the boundary (>= 1e-3 in every iteration) before it compares."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from byzpy_amd.aggregators import DnC
from byzpy_amd.hip import dispatch as D
from byzpy_amd.hip import require
from byzpy_amd.hip.graphs import CapturedAggregate
from byzpy_amd.ops import functional as F

DTYPES = [torch.float32, torch.bfloat16]
NS = [5, 33, 64, 65, 128]
# b below one 64-column tile, b no tile multiple, odd d everywhere
SHAPES = [(257, 64), (4099, 300), (70001, 1000)]
MIN_GAP = 1e-3


@pytest.fixture(scope="module")
def ext():
    return require()


def _tol(dtype):  # as in test_gpu_bulyan.py
    return dict(atol=1e-4, rtol=1e-4) if dtype == torch.float32 else dict(atol=5e-2, rtol=5e-2)


def _f(n):
    return max(1, n // 4)


def _scores_f64(S):
    """lambda u_i^2 of the centred (n, b) sample, f64, and the centred Gram."""
    Sd = S.double()
    C = Sd - Sd.mean(dim=0, keepdim=True)
    G = C @ C.T
    lam, U = torch.linalg.eigh(G)
    return lam[-1] * U[:, -1] ** 2, G


def _good_from_gram(Gc, bad, keep):
    """The rule on given Grams, f64, written out row by row."""
    niters, n = bad.shape
    good = torch.ones(n, dtype=torch.bool)
    for t in range(niters):
        lam, U = torch.linalg.eigh(Gc[t].double().cpu())
        s = (lam[-1] * U[:, -1] ** 2).tolist()
        b = bad[t].cpu().tolist()
        order = sorted(range(n), key=lambda i: (math.inf if b[i] else s[i], i))
        kept = set(i for i in order[:keep] if not b[i])
        good &= torch.tensor([i in kept for i in range(n)])
    return good


@functools.lru_cache(maxsize=None)
def _case(n, d, b, niters, dtype, c):
    """One input, its oracle results and device copies, built once."""
    g = torch.Generator().manual_seed(1000 * n + d + niters)
    w = torch.randn(d, generator=g)
    w /= w.norm()
    t = (torch.arange(n, dtype=torch.float32) ** 2 / n)[torch.randperm(n, generator=g)]
    X = 0.05 * torch.randn(n, d, generator=g) + t[:, None] * w[None, :] * (0.2 * d**0.5)
    X = X.to(dtype)  # cast first: the oracle sees the same values
    coords = torch.sort(torch.randint(0, d, (niters, b), generator=g), dim=1).values
    coords[:, 0], coords[:, -1] = 0, d - 1
    coords[:, 2] = coords[:, 1]  # a duplicate; still sorted
    f = _f(n)
    keep = F.dnc_keep(n, f, c)
    gaps, grams = [], []
    for row in coords:
        s, G = _scores_f64(X[:, row].float())
        grams.append(G)
        srt = torch.sort(s).values
        gaps.append(float((srt[keep] - srt[keep - 1]) / srt[keep]))
    return dict(
        X=X, Xd=X.cuda(), coords=coords, cols=coords.to("cuda", torch.int32),
        f=f, keep=keep, gap=min(gaps), gram=torch.stack(grams),
        good=F.dnc_select(X, f, coords, c), out=F.dnc(X, f, coords, c),
    )


CASES = [
    (n, d, b, niters, c)
    for n in NS
    for (d, b) in SHAPES
    for (niters, c) in [(1, 1.0), (3, 1.5)]
]


@pytest.mark.parametrize("n,d,b,niters,c", CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_three_launches_against_the_oracle(ext, n, d, b, niters, c, dtype):
    k = _case(n, d, b, niters, dtype, c)
    assert k["gap"] >= MIN_GAP, k["gap"]
    Xd, cols, keep = k["Xd"], k["cols"], k["keep"]

    # 1. sampled centred Gram, at the f32 Gram tolerance of test_gpu_kernels
    Gc, bad = ext.gram(Xd, cols=cols)
    assert Gc.shape == (niters, n, n) and Gc.dtype == torch.float32
    assert bad.shape == (niters, n) and bad.dtype == torch.int32
    ref = k["gram"]
    err = (Gc.double().cpu() - ref).abs().max().item()
    print(f"gram err {err:.3e} of max {ref.abs().max().item():.3e}")
    assert err < 1e-3 * max(1.0, ref.abs().max().item() / 100)
    assert not bool(bad.any())
    Gc2, bad2 = ext.gram(Xd, cols=cols)
    assert torch.equal(Gc, Gc2) and torch.equal(bad, bad2)

    # 2. spectral selection, against the rule on the SAME Gram
    idx, count = ext.smea_select(Gc, bad, keep)
    assert idx.shape == (n,) and idx.dtype == torch.int32 and count.dim() == 0
    cnt = int(count)
    good = _good_from_gram(Gc, bad, keep)
    assert idx[:cnt].tolist() == torch.nonzero(good).flatten().tolist()
    assert torch.equal(good, k["good"])  # and the oracle's own, from X
    assert bool((idx[cnt:] == 0).all())

    # 3. counted gather-mean: bitwise the un-counted kernel on idx[:count]
    out = ext.mean_rows(Xd, idx, count=count)
    assert cnt >= 1
    assert torch.equal(out, ext.mean_rows(Xd, idx[:cnt].contiguous()))

    # end to end, twice
    e2e = D.dnc(Xd, k["f"], cols, c)
    assert e2e.dtype == dtype and torch.equal(e2e, out)
    assert torch.equal(D.dnc(Xd, k["f"], cols, c), e2e)
    assert torch.allclose(e2e.float().cpu(), k["out"].float(), **_tol(dtype))
    assert torch.equal(D.dnc_select(Xd, k["f"], cols, c).cpu(), k["good"])
    agg = DnC(k["f"], c=c, coords=k["coords"])
    assert torch.equal(agg._aggregate(Xd), e2e)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_counted_mean_at_count_zero_and_partial(ext, dtype):
    k = _case(33, 4099, 300, 1, dtype, 1.0)
    Xd = k["Xd"]
    # +inf in a row the count leaves out must not reach the result
    Xp = Xd.clone()
    Xp[7] = float("inf")
    idx = torch.tensor([3, 1, 30, 7, 7], dtype=torch.int32, device="cuda")
    for cnt in range(4):
        count = torch.tensor(cnt, dtype=torch.int32, device="cuda")
        out = ext.mean_rows(Xp, idx, count=count)
        if cnt == 0:
            assert torch.equal(out, torch.zeros_like(out))
        else:
            assert torch.equal(out, ext.mean_rows(Xd, idx[:cnt].contiguous()))
    # an empty intersection end to end: keep = 1 and iterations that disagree
    X = torch.tensor([[0.0, 5.0, 1.0], [1.0, 0.0, 1.0], [4.0, 1.0, 1.0]]).to(dtype)
    coords = torch.tensor([[0], [1]])
    assert not bool(F.dnc_select(X, 2, coords).any())
    assert torch.equal(D.dnc(X.cuda(), 2, coords), torch.zeros(3, dtype=dtype, device="cuda"))


@pytest.mark.parametrize("poison", [float("inf"), float("nan"), 1e30])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [33, 128])
def test_non_finite_and_huge_rows(ext, n, dtype, poison):
    k = _case(n, 4099, 300, 3, dtype, 1.5)
    X = k["X"].clone()
    coords = k["coords"]
    victim = int(torch.nonzero(k["good"]).flatten()[1])  # a row DnC would keep
    col = int(coords[1, 5])
    X[victim, col] = poison
    other = int(torch.nonzero(k["good"]).flatten()[0])
    sampled = set(coords.flatten().tolist())
    unsampled = next(j for j in range(4099) if j not in sampled)
    X[other, unsampled] = float("inf")  # never sampled: `other` stays kept
    Xd = X.cuda()
    Gc, bad = ext.gram(Xd, cols=k["cols"])
    expect_bad = torch.zeros(3, n, dtype=torch.int32)
    expect_bad[:, victim] = (coords == col).any(dim=1).to(torch.int32)
    assert int(expect_bad[1, victim]) == 1
    assert torch.equal(bad.cpu(), expect_bad)
    assert bool(torch.isfinite(Gc).all())
    good = F.dnc_select(X, k["f"], coords, 1.5)
    assert not bool(good[victim])
    got = D.dnc_select(Xd, k["f"], k["cols"], 1.5).cpu()
    assert torch.equal(got, good)
    out = D.dnc(Xd, k["f"], k["cols"], 1.5)
    ref = F.dnc(X, k["f"], coords, 1.5)
    j = torch.arange(4099) != unsampled  # `other` is kept: its inf column is inf
    assert bool(torch.isfinite(out[j.cuda()]).all())
    assert torch.allclose(out.float().cpu()[j], ref.float()[j], **_tol(dtype))
    assert torch.equal(torch.isfinite(out.float().cpu()), torch.isfinite(ref.float()))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_duplicated_rows_tie_by_index(ext, dtype):
    # rows 3 and 9 identical: the Gram rows, hence the scores, are bitwise
    # equal, so wherever the boundary falls between them row 3 wins
    k = _case(33, 4099, 300, 1, dtype, 1.0)
    X = k["Xd"].clone()
    X[9] = X[3]
    Gc, bad = ext.gram(X, cols=k["cols"])
    assert torch.equal(Gc[0, 3], Gc[0, 9]) and torch.equal(Gc[0, :, 3], Gc[0, :, 9])
    seen_split = False
    for keep in range(1, 33):
        idx, count = ext.smea_select(Gc, bad, keep)
        kept = set(idx[: int(count)].tolist())
        assert not (9 in kept and 3 not in kept), keep
        seen_split |= 3 in kept and 9 not in kept
    assert seen_split


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_n_129_takes_the_torch_path(dtype):
    k = _case(129, 4099, 300, 3, dtype, 1.5)
    assert k["gap"] >= MIN_GAP, k["gap"]
    assert 129 > D.DNC_MAX_N
    out = D.dnc(k["Xd"], k["f"], k["cols"], 1.5)
    assert torch.equal(D.dnc_select(k["Xd"], k["f"], k["cols"], 1.5).cpu(), k["good"])
    assert torch.allclose(out.float().cpu(), k["out"].float(), **_tol(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_graph_capture_replays_to_the_eager_result(dtype):
    # capture fails on any host sync, so a replay that matches is the proof
    # that the fused path has none
    k = _case(64, 70001, 1000, 3, dtype, 1.5)
    cols, f = k["cols"], k["f"]
    cap = CapturedAggregate(lambda X: D.dnc(X, f, cols, 1.5), k["Xd"])
    assert torch.equal(cap.run(k["Xd"]), D.dnc(k["Xd"], f, cols, 1.5))
    k2 = _case(64, 70001, 1000, 1, dtype, 1.0)  # other data, same shape
    assert torch.equal(cap.run(k2["Xd"]), D.dnc(k2["Xd"], f, cols, 1.5))


def test_class_draws_the_same_coords_on_cpu_and_gpu():
    k = _case(33, 4099, 300, 1, torch.float32, 1.0)
    cpu = DnC(k["f"], niters=2, subsample=500, seed=9).aggregate(list(k["X"]))
    gpu = DnC(k["f"], niters=2, subsample=500, seed=9).aggregate(list(k["Xd"]))
    assert gpu.is_cuda
    assert torch.allclose(gpu.cpu(), cpu, **_tol(torch.float32))


def test_new_binding_forms_reject_bad_arguments(ext):
    X = torch.randn(8, 100, device="cuda")
    cols = torch.zeros(2, 10, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):  # int64 cols
        ext.gram(X, cols=cols.long())
    with pytest.raises(RuntimeError):  # 1-d cols
        ext.gram(X, cols=cols[0])
    with pytest.raises(RuntimeError):  # f64 X
        ext.gram(X.double(), cols=cols)
    with pytest.raises(RuntimeError):  # row cap
        ext.gram(torch.randn(129, 100, device="cuda"), cols=cols)
    with pytest.raises(RuntimeError):  # empty sample
        ext.gram(X, cols=cols[:, :0].contiguous())
    Gc, bad = ext.gram(X, cols=cols)
    with pytest.raises(RuntimeError):  # keep out of range
        ext.smea_select(Gc, bad, 0)
    with pytest.raises(RuntimeError):
        ext.smea_select(Gc, bad, 9)
    with pytest.raises(RuntimeError):  # bad of another shape
        ext.smea_select(Gc, bad[:1].contiguous(), 4)
    with pytest.raises(RuntimeError):  # f64 Gram
        ext.smea_select(Gc.double(), bad, 4)
    with pytest.raises(RuntimeError):  # row cap
        ext.smea_select(
            torch.zeros(1, 129, 129, device="cuda"),
            torch.zeros(1, 129, dtype=torch.int32, device="cuda"), 4,
        )
    idx = torch.arange(4, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):  # float count
        ext.mean_rows(X, idx, count=torch.tensor(2.0, device="cuda"))
    with pytest.raises(RuntimeError):  # host count
        ext.mean_rows(X, idx, count=torch.tensor(2, dtype=torch.int32))
    with pytest.raises(RuntimeError):  # count of two entries
        ext.mean_rows(X, idx, count=idx[:2].contiguous())
    # out-of-range coordinates are clamped, not read past the row
    wild = torch.tensor([[-5, 0, 99, 100, 2**31 - 1]], dtype=torch.int32, device="cuda")
    tame = torch.tensor([[0, 0, 99, 99, 99]], dtype=torch.int32, device="cuda")
    assert torch.equal(ext.gram(X, cols=wild)[0], ext.gram(X, cols=tame)[0])
