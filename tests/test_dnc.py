"""DnC (Divide-and-Conquer spectral filter) on the CPU: the oracle in
ops/functional.py on fixtures small enough to check by hand, the public
class (direct, pooled, seeds, validation) and the CPU face of the new
binding forms."""
import asyncio

import pytest
import torch

import byzpy_amd.ops.functional as F
from byzpy_amd import hip, run_operator
from byzpy_amd.aggregators import DnC
from byzpy_amd.graph.pool import ActorPoolConfig
from byzpy_amd.hip import dispatch as D


def _all_cols(d, niters=1):
    return torch.arange(d).repeat(niters, 1)


# -- the rule ---------------------------------------------------------------


def test_hand_fixture():
    # one column: the centred values are (-2.5, -1.5, -0.5, 4.5), the top
    # singular direction is that column itself, the scores are their squares
    # 6.25, 2.25, 0.25, 20.25; keep = 4 - 1 drops row 3
    X = torch.tensor([[1.0, 7.0], [2.0, 7.0], [3.0, 7.0], [8.0, 7.0]])
    coords = torch.tensor([[0]])
    assert F.dnc_select(X, 1, coords).tolist() == [True, True, True, False]
    assert torch.equal(F.dnc(X, 1, coords), torch.tensor([2.0, 7.0]))
    # f = 2 drops the two largest scores, rows 3 and 0
    assert F.dnc_select(X, 2, coords).tolist() == [False, True, True, False]
    assert torch.equal(D.dnc(X, 2, coords), torch.tensor([2.5, 7.0]))


def _outlier_case():
    g = torch.Generator().manual_seed(3)
    n, d, f = 12, 40, 3
    X = 0.1 * torch.randn(n, d, generator=g)
    w = torch.randn(d, generator=g)
    bad = [2, 5, 9]
    for k, i in enumerate(bad):
        X[i] += (4.0 + k) * w
    return X, f, bad


def test_outliers_along_one_direction_are_excluded():
    X, f, bad = _outlier_case()
    coords = _all_cols(X.shape[1], 2)
    good = F.dnc_select(X, f, coords)
    assert sorted(torch.nonzero(~good).flatten().tolist()) == bad
    rest = [i for i in range(X.shape[0]) if i not in bad]
    assert torch.allclose(F.dnc(X, f, coords), X[rest].mean(dim=0), atol=1e-6)
    assert torch.equal(D.dnc_select(X, f, coords), good)


def test_intersection_across_iterations():
    # columns 0..3 carry the attacker (row 0); column 4 is quiet except for
    # honest row 3. Iteration 0 samples 0..3 and drops row 0, iteration 1
    # samples only column 4 and drops row 3: neither survives
    g = torch.Generator().manual_seed(0)
    X = 0.01 * torch.randn(6, 5, generator=g)
    X[0, :4] += 5.0
    X[3, 4] += 3.0
    c0 = torch.tensor([[0, 1, 2, 3]])
    c1 = torch.tensor([[4, 4, 4, 4]])
    assert F.dnc_select(X, 1, c0).tolist() == [False] + [True] * 5
    assert F.dnc_select(X, 1, c1).tolist() == [True] * 3 + [False] + [True] * 2
    both = torch.cat([c0, c1])
    assert F.dnc_select(X, 1, both).tolist() == [False, True, True, False, True, True]
    assert torch.allclose(F.dnc(X, 1, both), X[[1, 2, 4, 5]].mean(dim=0), atol=1e-7)


def test_filter_fraction_floors():
    X = torch.tensor([[0.0], [1.0], [2.0], [3.0], [4.0], [50.0], [60.0], [70.0]])
    coords = torch.tensor([[0]])
    # keep = 8 - floor(1.5 * 3) = 4: the four rows nearest the mean 23.75
    assert F.dnc_keep(8, 3, 1.5) == 4
    assert int(F.dnc_select(X, 3, coords, 1.5).sum()) == 4
    assert F.dnc_keep(8, 1, 1.5) == 7  # floor(1.5) = 1
    assert F.dnc_keep(8, 3, 0.0) == 8
    assert int(F.dnc_select(X, 3, coords, 0.0).sum()) == 8


def test_ties_go_to_the_smaller_index():
    # rows 1 and 4 are identical and tie for the last kept place: column 0,
    # (3.2, 9.2, 4.2, -0.8, 9.2), has mean 5 and centred squares
    # 0: 3.24, 1: 17.64, 2: 0.64, 3: 33.64, 4: 17.64 -> keep 3 = {2, 0, 1}
    X = torch.tensor([[3.0, 1.0], [9.0, 2.0], [4.0, 3.0], [-1.0, 4.0], [9.0, 2.0]])
    X[:, 0] += 0.2
    coords = torch.tensor([[0]])
    assert F.dnc_select(X, 2, coords).tolist() == [True, True, True, False, False]
    # the same through the Gram-based selection of the pooled / sharded paths
    Gc, bad = D.dnc_gram(X, coords)
    idx, count = D.dnc_select_from_gram(Gc, bad, 3)
    assert idx[: int(count)].tolist() == [0, 1, 2]
    # and on a wide sample, where eigh's u_1 and u_4 agree only to rounding
    g = torch.Generator().manual_seed(1)
    Y = torch.randn(7, 30, generator=g)
    Y[5] = Y[2]
    for keep_f in range(1, 6):
        sel = F.dnc_select(Y, keep_f, _all_cols(30))
        assert not (bool(sel[5]) and not bool(sel[2])), keep_f
        idx, count = D.dnc_select_from_gram(*D.dnc_gram(Y, _all_cols(30)), 7 - keep_f)
        assert idx[: int(count)].tolist() == torch.nonzero(sel).flatten().tolist()


@pytest.mark.parametrize("poison", [float("inf"), float("-inf"), float("nan"), 1e30])
def test_non_finite_sampled_row_is_never_kept(poison):
    g = torch.Generator().manual_seed(5)
    X = torch.randn(8, 12, generator=g)
    X[6, 3] = poison
    coords = torch.tensor([[1, 3, 5, 7], [0, 3, 4, 9]])
    for f in (0, 2):
        good = F.dnc_select(X, f, coords)
        assert not bool(good[6])
        out = F.dnc(X, f, coords)
        assert bool(torch.isfinite(out).all())
        assert torch.allclose(out, X[good].mean(dim=0))
        assert torch.equal(D.dnc(X, f, coords), out)
    # the entry is left out of its column's mean and centres to 0: the other
    # rows score as if it sat exactly at the mean of the finite entries
    Y = X.clone()
    Y[6, 3] = X[[0, 1, 2, 3, 4, 5, 7], 3].mean()
    Gx, bx = D.dnc_gram(X, coords)
    Gy, by = D.dnc_gram(Y, coords)
    assert torch.allclose(Gx, Gy, rtol=1e-6, atol=1e-6)
    assert bx.tolist() == [[0] * 6 + [1, 0]] * 2 and not bool(by.any())


def test_inf_in_an_unsampled_column_changes_nothing():
    g = torch.Generator().manual_seed(5)
    X = torch.randn(8, 12, generator=g)
    coords = torch.tensor([[1, 3, 5, 7], [0, 3, 4, 9]])
    ref = F.dnc_select(X, 2, coords)
    kept_row = int(torch.nonzero(ref).flatten()[0])
    X[kept_row, 11] = float("inf")
    assert torch.equal(F.dnc_select(X, 2, coords), ref)
    dropped = int(torch.nonzero(~ref).flatten()[0])
    X[kept_row, 11] = 0.0
    X[dropped, 11] = float("inf")
    out = F.dnc(X, 2, coords)
    assert bool(torch.isfinite(out).all())  # rows outside `good` are not read


def test_empty_intersection_gives_zeros():
    # keep = 3 - 2 = 1 and two iterations that keep different rows
    X = torch.tensor([[0.0, 5.0, 1.0], [1.0, 0.0, 1.0], [4.0, 1.0, 1.0]])
    coords = torch.tensor([[0], [1]])
    # column 0: centred (-5/3, -2/3, 7/3) -> keep 1 = row 1
    # column 1: centred (3, -2, -1)       -> keep 1 = row 2
    assert F.dnc_select(X, 2, coords).tolist() == [False, False, False]
    assert torch.equal(F.dnc(X, 2, coords), torch.zeros(3))
    assert torch.equal(D.dnc(X, 2, coords), torch.zeros(3))
    assert torch.equal(DnC(2, coords=coords).aggregate(list(X)), torch.zeros(3))


def test_duplicate_coords_are_accepted():
    X, f, bad = _outlier_case()
    coords = torch.tensor([[0, 0, 0, 7, 7, 39, 39]])
    good = F.dnc_select(X, f, coords)
    assert sorted(torch.nonzero(~good).flatten().tolist()) == bad
    out = DnC(f, coords=coords).aggregate(list(X))
    assert torch.allclose(out, X[good].mean(dim=0), atol=1e-6)


# -- the class --------------------------------------------------------------


def test_export_and_name():
    import byzpy_amd.aggregators as A

    assert "DnC" in A.__all__ and A.DnC is DnC
    assert DnC(1).name == "dnc"
    assert D.DNC_MAX_N == 128


def test_same_seed_same_output():
    X, f, _ = _outlier_case()
    grads = list(X)
    a = DnC(f, niters=3, subsample=10, seed=11).aggregate(grads)
    b = DnC(f, niters=3, subsample=10, seed=11).aggregate(grads)
    assert torch.equal(a, b)
    # the draw itself: sorted, in range, b = min(subsample, d)
    agg = DnC(f, niters=3, subsample=1000, seed=11)
    co = agg._coords_for(X)
    assert co.shape == (3, X.shape[1])
    assert bool((co[:, 1:] >= co[:, :-1]).all())
    assert int(co.min()) >= 0 and int(co.max()) < X.shape[1]
    ref = torch.sort(
        torch.randint(0, X.shape[1], (3, X.shape[1]),
                      generator=torch.Generator().manual_seed(11)),
        dim=1,
    ).values
    assert torch.equal(co, ref)


@pytest.mark.parametrize("chunk_size", [1, 7, 4096])
def test_thread_pool_matches_direct(chunk_size):
    X, f, _ = _outlier_case()
    grads = list(X)
    direct = DnC(f, niters=3, subsample=25, seed=4).aggregate(grads)

    async def pooled():
        return await run_operator(
            DnC(f, niters=3, subsample=25, seed=4, chunk_size=chunk_size),
            {"gradients": grads},
            pool_config=ActorPoolConfig(backend="thread", count=3),
        )

    out = asyncio.run(pooled())
    assert torch.equal(out, direct), "dnc pooled != direct"


def test_bf16_inputs():
    X, f, bad = _outlier_case()
    Xb = X.to(torch.bfloat16)
    out = DnC(f, coords=_all_cols(X.shape[1])).aggregate(list(Xb))
    assert out.dtype == torch.bfloat16
    rest = [i for i in range(X.shape[0]) if i not in bad]
    assert torch.equal(out, Xb[rest].float().mean(dim=0).to(torch.bfloat16))


def test_value_errors():
    X = torch.randn(6, 9)
    grads = list(X)
    with pytest.raises(ValueError):
        DnC(-1)
    with pytest.raises(ValueError):
        DnC(1, c=-0.5)
    with pytest.raises(ValueError):
        DnC(1, niters=0)
    with pytest.raises(ValueError):  # keep = 6 - 6 < 1
        DnC(6).aggregate(grads)
    with pytest.raises(ValueError):  # keep = 6 - floor(2.5 * 3) < 1
        DnC(3, c=2.5).aggregate(grads)
    with pytest.raises(ValueError):  # unsorted
        DnC(1, coords=torch.tensor([[3, 1, 2]]))
    with pytest.raises(ValueError):  # out of range: d = 9
        DnC(1, coords=torch.tensor([[0, 4, 9]])).aggregate(grads)
    with pytest.raises(ValueError):
        DnC(1, coords=torch.tensor([[-1, 4, 8]])).aggregate(grads)
    with pytest.raises(ValueError):
        F.dnc(X, -1, torch.tensor([[0]]))
    with pytest.raises(ValueError):
        D.dnc(X, 6, torch.tensor([[0]]))
    # the pooled path raises before it fans out, and leaves nothing behind
    async def pooled():
        return await run_operator(
            DnC(6), {"gradients": grads},
            pool_config=ActorPoolConfig(backend="thread", count=2),
        )

    with pytest.raises(ValueError):
        asyncio.run(pooled())


# -- binding forms, CPU face ------------------------------------------------


def test_new_binding_forms_refuse_cpu_tensors():
    ext = hip.require()
    X = torch.randn(5, 8)
    cols = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ext.gram(X, cols=cols)
    with pytest.raises(RuntimeError):
        ext.smea_select(torch.zeros(1, 5, 5), torch.zeros(1, 5, dtype=torch.int32), 3)
    with pytest.raises(RuntimeError):
        ext.mean_rows(
            X, torch.tensor([0, 1], dtype=torch.int32),
            count=torch.tensor(2, dtype=torch.int32),
        )
    with pytest.raises(TypeError):  # cols and count are keyword-only
        ext.gram(X, cols)
    with pytest.raises(TypeError):
        ext.mean_rows(X, cols[0], cols[0])
