"""AFA (Adaptive Federated Averaging) on the CPU: the oracle in
ops/functional.py on inputs small enough to check by hand, the Gram-based
selection of the pooled / sharded / device paths against it, the public
class, and the reputation helper."""
import asyncio
import math

import pytest
import torch

import _afa_cases as C
import byzpy_amd.ops.functional as F
from byzpy_amd import run_operator
from byzpy_amd.aggregators import AFA, AFAReputation
from byzpy_amd.graph.pool import ActorPoolConfig
from byzpy_amd.hip import dispatch as D
from byzpy_amd.parallel import sharded


def _mask_from(idx, count, n):
    m = torch.zeros(n, dtype=torch.bool)
    m[idx[: int(count)].long()] = True
    return m


# -- the rule, by hand --------------------------------------------------------


def test_lower_branch_removes_the_flipped_row():
    """Rows (1,0) x3 and (-1,0). g = (0.5, 0); cosines 1, 1, 1, -1; mean 0.5
    < med 1, so the lower branch; sd = sqrt((3 * 0.25 + 2.25) / 4) =
    sqrt(0.75) = 0.8660; threshold 1 - 2 * 0.8660 = -0.7321 > -1: row 3
    goes. Pass 2 (xi = 2.5): all cosines 1, sd 0, nothing goes."""
    X = torch.tensor([[1.0, 0.0], [1.0, 0.0], [1.0, 0.0], [-1.0, 0.0]])
    good, trace = F.afa_trace(X)
    assert good.tolist() == [True, True, True, False]
    assert len(trace) == 2 and trace[0]["lower"]
    assert trace[0]["mean"] == pytest.approx(0.5)
    assert trace[0]["med"] == pytest.approx(1.0)
    assert trace[0]["sd"] == pytest.approx(math.sqrt(0.75))
    assert trace[0]["threshold"] == pytest.approx(1.0 - 2.0 * math.sqrt(0.75))
    assert trace[1]["sd"] == 0.0 and not bool(trace[1]["removed"].any())
    assert torch.equal(F.afa(X), torch.tensor([1.0, 0.0]))


def test_upper_branch_removes_the_colluder_and_keeps_a_zero_row():
    """Rows e1, -e1, e2, -e2, 0 and (0,0,4). g = (0, 0, 2/3); cosines
    0, 0, 0, 0, 0 (zero row: defined as 0), 1; mean 1/6 >= med 0, so the
    upper branch; sd = sqrt(1/6 - 1/36) = sqrt(5)/6 = 0.3727; threshold
    0.7454 < 1: row 5 goes. Pass 2: g = 0, every cosine 0 by definition,
    sd 0, nothing goes. The survivors average to the zero vector."""
    X = torch.tensor([
        [1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 0],
        [0, 0, 4.0],
    ])
    good, trace = F.afa_trace(X)
    assert good.tolist() == [True] * 5 + [False]
    assert len(trace) == 2 and not trace[0]["lower"]
    assert trace[0]["sd"] == pytest.approx(math.sqrt(5.0) / 6.0)
    assert trace[0]["threshold"] == pytest.approx(math.sqrt(5.0) / 3.0)
    assert trace[1]["s"].tolist() == [0.0] * 6
    assert torch.equal(F.afa(X), torch.zeros(3))


def test_sd_zero_removes_nothing():
    """Identical rows: every cosine is the same number c (1 up to rounding),
    the median is c exactly, sd is 0 up to rounding, and the strict
    inequality holds for no row whatever the rounding of the mean; one
    pass."""
    X = torch.tensor([[1.0, 2.0]] * 3)
    good, trace = F.afa_trace(X)
    assert good.all() and len(trace) == 1 and trace[0]["sd"] < 1e-15
    assert len(set(trace[0]["s"].tolist())) == 1
    assert torch.equal(F.afa(X), torch.tensor([1.0, 2.0]))


def test_one_row():
    X = torch.tensor([[3.0, 4.0]])
    assert F.afa_select(X).tolist() == [True]
    assert torch.equal(F.afa(X), X[0])


def test_inf_row_and_zero_weight_row_start_dead():
    X = torch.tensor([[1.0, 0.0], [1.0, 0.0], [float("inf"), 0.0]])
    assert F.afa_select(X).tolist() == [True, True, False]
    assert torch.equal(F.afa(X), torch.tensor([1.0, 0.0]))
    X = torch.tensor([[1.0, 0.0], [1.0, 0.0], [float("nan"), 0.0]])
    assert F.afa_select(X).tolist() == [True, True, False]
    X = torch.tensor([[1.0, 0.0], [1.0, 0.0], [-5.0, 0.0]])
    w = torch.tensor([1.0, 1.0, 0.0])
    assert F.afa_select(X, w).tolist() == [True, True, False]
    assert torch.equal(F.afa(X, w), torch.tensor([1.0, 0.0]))


def test_weighted_mean_of_two_rows():
    """Rows e1, e2 with weights 1, 3: g = (0.25, 0.75), cosines 0.3162 and
    0.9487; two values, so mean = med and the upper branch; sd 0.3162,
    threshold 0.6325 + 0.6325 > 0.9487: nothing goes."""
    X = torch.tensor([[1.0, 0.0], [0.0, 1.0]])
    w = [1.0, 3.0]
    good, trace = F.afa_trace(X, w)
    assert good.all() and len(trace) == 1 and not trace[0]["lower"]
    assert trace[0]["s"].tolist() == pytest.approx([0.1**0.5, 0.9**0.5])
    assert torch.allclose(F.afa(X, w), torch.tensor([0.25, 0.75]))


def test_nothing_alive_gives_zeros():
    X = torch.tensor([[float("inf"), 1.0], [float("nan"), 2.0]])
    good, trace = F.afa_trace(X)
    assert not good.any() and trace == []
    assert torch.equal(F.afa(X), torch.zeros(2))
    X = torch.tensor([[1.0, 1.0], [2.0, 2.0]])
    assert torch.equal(F.afa(X, [0.0, 0.0]), torch.zeros(2))
    assert torch.equal(D.afa(X, [0.0, 0.0]), torch.zeros(2))
    assert torch.equal(AFA(weights=[0.0, 0.0]).aggregate(list(X)), torch.zeros(2))


# -- the Gram-based selection against the oracle -------------------------------

CASES = [(v, n, f, d) for v in C.VARIANTS for (n, f, d) in C.SHAPES]


@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
@pytest.mark.parametrize("variant,n,f,d", CASES)
def test_selection_from_the_gram_is_the_oracles(variant, n, f, d, weighted):
    k = C.case(variant, n, f, d, torch.float32, weighted)
    assert k["margin"] >= C.MIN_MARGIN, k["margin"]
    Xd = k["X"].double()
    idx, count = D.afa_select_from_gram(Xd @ Xd.T, k["w"])
    assert idx.dtype == torch.int32 and idx.shape == (n,)
    assert torch.equal(_mask_from(idx, count, n), k["good"])
    assert bool((idx[int(count):] == 0).all())
    idx2, _, rounds = D._afa_select_torch(
        Xd @ Xd.T, torch.ones(n) if k["w"] is None else k["w"], 2.0, 0.5
    )
    assert torch.equal(idx2, idx) and rounds == k["rounds"]


def test_fixtures_cover_both_branches_and_several_passes():
    lowers, rounds = set(), set()
    for (v, n, f, d) in CASES:
        k = C.case(v, n, f, d, torch.float32)
        lowers.add(k["lower"][0])
        rounds.add(k["rounds"])
        if v == "flip":
            assert k["lower"][0] and int(k["good"].sum()) == n - f
        if v == "collude":
            assert not k["lower"][0]
    assert lowers == {True, False} and max(rounds) >= 3


@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
def test_dispatch_and_class_agree_for_list_and_matrix(weighted):
    k = C.case("tiers", 23, 3, 2050, torch.float32, weighted)
    X, w = k["X"], k["w"]
    ref = F.afa(X, w)
    assert torch.equal(D.afa(X, w), ref)
    assert torch.equal(D.afa_select(X, w), k["good"])
    agg = AFA(weights=w)
    assert agg.name == "afa"
    assert torch.equal(agg.aggregate(list(X)), ref)
    assert torch.equal(agg.aggregate(X), ref)
    # weights may be replaced between calls
    agg.weights = None
    assert torch.equal(agg.aggregate(X), F.afa(X))
    import byzpy_amd.aggregators as A

    assert "AFA" in A.__all__ and A.AFA is AFA


@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
@pytest.mark.parametrize("chunk_size", [1, 7, 4096])
def test_thread_pool_matches_direct(chunk_size, weighted):
    k = C.case("flip", 23, 3, 2050, torch.float32, weighted)
    grads = list(k["X"])
    direct = AFA(weights=k["w"]).aggregate(grads)

    async def pooled():
        return await run_operator(
            AFA(weights=k["w"], chunk_size=chunk_size),
            {"gradients": grads},
            pool_config=ActorPoolConfig(backend="thread", count=3),
        )

    out = asyncio.run(pooled())
    assert torch.allclose(out, direct, atol=1e-6, rtol=1e-6)
    # the pooled path selects on an f32 Gram, the direct one on the rows
    assert torch.allclose(out, k["out"], atol=1e-6, rtol=1e-6)


@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
def test_sharded_on_two_column_halves(monkeypatch, weighted):
    k = C.case("collude", 23, 3, 2050, torch.float32, weighted)
    X, w = k["X"], k["w"]
    halves = [X[:, :1025].contiguous(), X[:, 1025:].contiguous()]
    whole = D.afa(X, w)
    outs = []
    for r in (0, 1):
        other = D.gram(halves[1 - r])
        # the all-reduce, by hand: this rank's partial Gram plus the other's
        monkeypatch.setattr(sharded, "all_reduce_", lambda G, o=other: G + o)
        outs.append(sharded.afa(halves[r], w))
    assert torch.allclose(torch.cat(outs), whole, atol=1e-6, rtol=1e-6)
    monkeypatch.undo()
    # without a process group the all-reduce is the identity: one shard = whole
    assert torch.allclose(sharded.afa(X, w), whole, atol=1e-6, rtol=1e-6)


def test_bf16_inputs_keep_their_dtype():
    k = C.case("flip", 9, 1, 33, torch.bfloat16)
    out = AFA().aggregate(list(k["X"]))
    assert out.dtype == torch.bfloat16 and out.shape == (33,)
    assert torch.equal(out, k["out"])


# -- reputation ---------------------------------------------------------------


def test_beta_cdf_at_one_half_by_hand():
    """N = a + b - 1, sum_{j=a}^{N} C(N, j) / 2^N: (3,3) -> (10+5+1)/32,
    (3,4) -> (20+15+6+1)/64, (3,9) -> (2048 - 1 - 11 - 55)/2048,
    (4,3) -> (15+6+1)/64."""
    cdf = AFAReputation.cdf_half
    assert cdf(3, 3) == 0.5
    assert cdf(3, 4) == 42 / 64
    assert cdf(3, 8) == 968 / 1024
    assert cdf(3, 9) == 1981 / 2048
    assert cdf(4, 3) == 22 / 64
    assert cdf(1, 1) == 0.5


def test_reputation_blocks_after_six_bad_rounds():
    """Client 1 is dropped every round: beta 3 -> 9. The CDF passes 0.6563,
    0.7734, 0.8555, 0.9102, 0.9453 (< 0.95) and reaches 0.9673 at beta = 9,
    the sixth bad round."""
    rep = AFAReputation(3)
    assert rep.weights().tolist() == [0.5, 0.5, 0.5]
    assert not rep.blocked.any()
    for rnd in range(1, 7):
        rep.update(torch.tensor([True, False, True]))
        assert rep.blocked.tolist() == [False, rnd >= 6, False], rnd
    assert rep.alpha == [9, 3, 9] and rep.beta == [3, 9, 3]
    w = rep.weights()
    assert w.tolist() == pytest.approx([0.75, 0.0, 0.75])
    assert rep.weights([10, 20, 30]).tolist() == pytest.approx([7.5, 0.0, 22.5])
    # a blocked client is never updated again
    rep.update([True, True, False])
    assert rep.alpha == [10, 3, 9] and rep.beta == [3, 9, 4]
    assert rep.blocked.tolist() == [False, True, False]
    # and its weight drops the row out of AFA
    X = torch.tensor([[1.0, 0.0], [-9.0, 0.0], [1.0, 0.0]])
    assert F.afa_select(X, rep.weights()).tolist() == [True, False, True]


def test_reputation_arguments():
    with pytest.raises(ValueError):
        AFAReputation(0)
    with pytest.raises(ValueError):
        AFAReputation(3, alpha0=2.5)
    with pytest.raises(ValueError):
        AFAReputation(3, beta0=0)
    with pytest.raises(ValueError):
        AFAReputation(3, block_at=0.0)
    rep = AFAReputation(3)
    with pytest.raises(ValueError):
        rep.update([True, False])
    with pytest.raises(ValueError):
        rep.weights([1.0, 2.0])


# -- arguments ------------------------------------------------------------------

BAD_WEIGHTS = [
    [1.0, -1.0, 1.0, 1.0],
    [1.0, float("nan"), 1.0, 1.0],
    [1.0, float("inf"), 1.0, 1.0],
    [1.0, 1.0, 1.0],
]


@pytest.mark.parametrize("fn", [F.afa_select, F.afa, F.afa_trace, D.afa, D.afa_select])
def test_value_errors(fn):
    X = torch.randn(4, 6)
    with pytest.raises(ValueError):
        fn(X, None, -0.1)
    with pytest.raises(ValueError):
        fn(X, None, 2.0, -0.5)
    for w in BAD_WEIGHTS:
        with pytest.raises(ValueError):
            fn(X, w)
        with pytest.raises(ValueError):
            fn(X, torch.tensor(w))


def test_value_errors_of_the_gram_form_and_the_class():
    X = torch.randn(4, 6)
    G = X @ X.T
    with pytest.raises(ValueError):
        D.afa_select_from_gram(G, None, -1.0)
    with pytest.raises(ValueError):
        D.afa_select_from_gram(G, None, 2.0, -1.0)
    for w in BAD_WEIGHTS:
        with pytest.raises(ValueError):
            D.afa_select_from_gram(G, w)
        with pytest.raises(ValueError):
            AFA(weights=w).aggregate(list(X))
        with pytest.raises(ValueError):
            sharded.afa(X, w)
    with pytest.raises(ValueError):
        AFA(xi=-1.0)
    with pytest.raises(ValueError):
        AFA(delta_xi=-1.0)

    # the pooled path raises before it fans out
    async def pooled():
        return await run_operator(
            AFA(weights=BAD_WEIGHTS[0]),
            {"gradients": list(X)},
            pool_config=ActorPoolConfig(backend="thread", count=2),
        )

    with pytest.raises(ValueError):
        asyncio.run(pooled())
