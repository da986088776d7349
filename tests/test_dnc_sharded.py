"""sharded.dnc over gloo, world_size = 2: column halves with their own
coordinates against D.dnc on the whole matrix with the union, and the
selection identical on both ranks."""
import os

import torch
import torch.multiprocessing as tmp

from byzpy_amd.hip import dispatch as D
from byzpy_amd.parallel.sharded import dnc as sharded_dnc

WORLD = 2
N, DLOC, NITERS, BLOC, F_, C_ = 12, 32, 3, 10, 3, 1.5


def _inputs():
    """Identical on every rank: X, and per-rank local coordinates."""
    g = torch.Generator().manual_seed(21)
    X = 0.1 * torch.randn(N, WORLD * DLOC, generator=g)
    w = torch.randn(WORLD * DLOC, generator=g)
    for k, i in enumerate((1, 6, 10)):
        X[i] += (3.0 + k) * w
    local = [
        torch.sort(torch.randint(0, DLOC, (NITERS, BLOC), generator=g), dim=1).values
        for _ in range(WORLD)
    ]
    return X, local


def _entry(rank, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(WORLD)
    os.environ["LOCAL_RANK"] = str(rank)
    import torch.distributed as dist

    from byzpy_amd.ops import functional as F
    from byzpy_amd.parallel import dist as pdist
    from byzpy_amd.parallel import sharded
    from byzpy_amd.parallel.dist import all_reduce_, column_shard

    pdist.init_from_env()
    try:
        X, local = _inputs()
        Xs = column_shard(X, rank)
        out = sharded.dnc(Xs, F_, local[rank], C_)
        both = pdist.all_gather_rows(out.reshape(1, -1)).reshape(-1)
        union = torch.cat([local[r] + r * DLOC for r in range(WORLD)], dim=1)
        whole = D.dnc(X, F_, union, C_)
        assert torch.allclose(both, whole, atol=1e-6)
        # the selection, rank by rank
        Gc, bad = D.dnc_gram(Xs, local[rank])
        idx, count = D.dnc_select_from_gram(
            all_reduce_(Gc), all_reduce_(bad), F.dnc_keep(N, F_, C_)
        )
        mask = torch.zeros(N)
        mask[idx[: int(count)].long()] = 1.0
        masks = pdist.all_gather_rows(mask.reshape(1, -1))
        assert torch.equal(masks[0], masks[1])
        assert torch.equal(masks[rank].bool(), F.dnc_select(X, F_, union, C_))
        assert 1 <= int(count) <= N - 3
    finally:
        dist.destroy_process_group()


def test_sharded_dnc_gloo():
    ctx = tmp.get_context("spawn")
    port = 29531 + 2500 + os.getpid() % 500
    procs = [ctx.Process(target=_entry, args=(r, port)) for r in range(WORLD)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
    for p in procs:
        assert p.exitcode == 0, f"worker failed with {p.exitcode}"


def test_sharded_dnc_single_process_equals_dispatch():
    # without a process group all_reduce_ is the identity: one shard = whole
    X, local = _inputs()
    union = torch.cat([local[r] + r * DLOC for r in range(WORLD)], dim=1)
    assert torch.allclose(sharded_dnc(X, F_, union, C_), D.dnc(X, F_, union, C_), atol=1e-6)
