"""Bulyan on the CPU: the functional oracle against a hand-worked fixture,
the dispatch selection against the oracle on exactly-representable inputs,
the public class (direct, pooled, dtype), the `rows=` argument of the
coordinate-wise ops, the d-sharded form over gloo, and the optional-argument
plumbing of the two extended bindings."""
import asyncio
import os

import pytest
import torch
import torch.multiprocessing as tmp

import byzpy_amd.ops.functional as F
from byzpy_amd import hip, run_operator
from byzpy_amd.aggregators import Bulyan
from byzpy_amd.graph.pool import ActorPoolConfig
from byzpy_amd.hip import dispatch as D

HAND_X = torch.tensor([[0.0], [1.0], [2.0], [3.0], [4.0], [5.0], [100.0]])


def test_hand_fixture():
    # first pick: rows 2 and 3 tie at score 19, index 2 wins
    assert F.bulyan_select(HAND_X, 1).tolist() == [2, 3, 1, 4, 0]
    assert F.bulyan(HAND_X, 1).tolist() == [2.0]
    assert D.bulyan(HAND_X, 1).tolist() == [2.0]


def _integer_matrix(n, d=48):
    g = torch.Generator().manual_seed(100 + n)
    X = torch.randint(-4, 5, (n, d), generator=g).float()
    X[1] = X[0]  # exact distance and score ties
    return X


@pytest.mark.parametrize(
    "n,f", [(7, 1), (11, 2), (15, 3), (33, 1), (64, 15), (67, 16)]
)
def test_selection_exact_on_integer_inputs(n, f):
    # every Gram entry and every score is an integer below 2^24: f32
    # (dispatch) and f64 (oracle) arithmetic are both exact
    X = _integer_matrix(n)
    got = D.bulyan_select_from_gram(X @ X.T, f)
    assert got.dtype == torch.int32 and got.shape == (n - 2 * f,)
    assert got.tolist() == F.bulyan_select(X, f).tolist()
    assert len(set(got.tolist())) == n - 2 * f


def test_validation():
    f = 2
    bad = torch.randn(4 * f + 2, 5)
    for call in (
        lambda: F.bulyan(bad, f),
        lambda: D.bulyan(bad, f),
        lambda: D.bulyan_select_from_gram(bad @ bad.T, f),
        lambda: Bulyan(f).aggregate(list(bad)),
    ):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        Bulyan(-1)
    ok = torch.randn(4 * f + 3, 5, generator=torch.Generator().manual_seed(3))
    assert torch.allclose(D.bulyan(ok, f), F.bulyan(ok, f), atol=1e-6)
    assert Bulyan(f).aggregate(list(ok)).shape == (5,)


def test_f_zero_is_the_mean():
    X = torch.randn(6, 33, generator=torch.Generator().manual_seed(4))
    assert F.bulyan_select(X, 0).tolist() == list(range(6))
    assert D.bulyan_select_from_gram(X @ X.T, 0).tolist() == list(range(6))
    for out in (F.bulyan(X, 0), D.bulyan(X, 0), Bulyan(0).aggregate(list(X))):
        assert torch.allclose(out, X.mean(dim=0), atol=1e-6)


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(42)
    return torch.randn(12, 257, generator=g)


def test_direct_matches_oracle(data):
    assert torch.allclose(
        Bulyan(2).aggregate(list(data)), F.bulyan(data, 2), atol=1e-6
    )


def test_thread_pool_matches_direct(data):
    agg = Bulyan(2, chunk_size=4)
    grads = list(data)
    direct = agg.aggregate(grads)

    async def pooled():
        return await run_operator(
            agg,
            {"gradients": grads},
            pool_config=ActorPoolConfig(backend="thread", count=3),
        )

    out = asyncio.run(pooled())
    assert torch.allclose(out, direct, atol=1e-4), "bulyan pooled != direct"


def test_bf16_roundtrip(data):
    out = Bulyan(2).aggregate([g.bfloat16() for g in data])
    assert out.dtype == torch.bfloat16 and out.shape == (257,)


def test_cli_lists_bulyan(capsys):
    from byzpy_amd.cli import main as cli_main

    assert cli_main(["list", "aggregators"]) == 0
    assert "Bulyan" in capsys.readouterr().out


def test_cpu_rows_argument(data):
    r = torch.tensor([7, 2, 9, 0, 11, 4, 5], dtype=torch.int32)
    sub = data[r.long()]
    assert torch.equal(D.median(data, rows=r), F.median(sub))
    assert torch.equal(D.trimmed_mean(data, 2, rows=r), F.trimmed_mean(sub, 2))
    assert torch.equal(
        D.mean_of_medians(data, 3, rows=r), F.mean_of_medians(sub, 3)
    )


# -- sharded.bulyan over gloo, world_size = 2 -------------------------------

WORLD = 2


def _entry(rank, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(WORLD)
    os.environ["LOCAL_RANK"] = str(rank)
    import torch.distributed as dist

    from byzpy_amd.parallel import dist as pdist
    from byzpy_amd.parallel import sharded
    from byzpy_amd.parallel.dist import column_shard

    pdist.init_from_env()
    try:
        g = torch.Generator().manual_seed(7)
        X = torch.randn(11, 64, generator=g)  # identical on both ranks
        out = sharded.bulyan(column_shard(X, rank), 2)
        both = pdist.all_gather_rows(out.reshape(1, -1)).reshape(-1)
        assert torch.allclose(both, F.bulyan(X, 2), atol=1e-5)
    finally:
        dist.destroy_process_group()


def test_sharded_bulyan_gloo():
    ctx = tmp.get_context("spawn")
    port = 29531 + 2000 + os.getpid() % 500
    procs = [ctx.Process(target=_entry, args=(r, port)) for r in range(WORLD)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
    for p in procs:
        assert p.exitcode == 0, f"worker failed with {p.exitcode}"


# -- optional-argument plumbing of the extended bindings --------------------


@pytest.fixture(scope="module")
def ext():
    return hip.require()


def test_extended_bindings_still_refuse_cpu_tensors(ext):
    X = torch.randn(5, 8)
    rows = torch.tensor([0, 2, 4], dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ext.colsel(X, 2, 1, rows)
    with pytest.raises(RuntimeError):
        ext.colsel(X, 2, 1, rows=rows)
    with pytest.raises(RuntimeError):
        ext.krum_select(torch.eye(5), 1, 2, True)
    with pytest.raises(RuntimeError):
        ext.krum_select(torch.eye(5), 1, 2, iterative=True)


def test_extended_bindings_have_no_fifth_argument(ext):
    X = torch.randn(5, 8)
    rows = torch.tensor([0, 2, 4], dtype=torch.int32)
    with pytest.raises(TypeError):
        ext.colsel(X, 2, 1, rows, None)
    with pytest.raises(TypeError):
        ext.krum_select(torch.eye(5), 1, 2, True, None)
