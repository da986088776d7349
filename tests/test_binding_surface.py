"""CPU-side checks of the _hip_ops binding surface and of the Gram-derived
selection helpers in hip/dispatch.py. The extension loads without a GPU:
every device binding must refuse a CPU tensor before touching the device,
and the host MDA search runs here."""
import pytest
import torch

from byzpy_amd import hip
from byzpy_amd.hip import dispatch as D
from byzpy_amd.ops import functional as F

BINDINGS = (
    "bucket_mean caf_colsum caf_matvec cc_apply cc_iter colsel gaussian_fill "
    "gram group_mean_rows krum_select little_fused mda_search mda_select "
    "mean_rows row_center_sqdists row_scale row_sqnorms smea_select "
    "weiszfeld_apply weiszfeld_iter weiszfeld_iter_grouped"
).split()


@pytest.fixture(scope="module")
def ext():
    return hip.require()


def test_public_names(ext):
    assert sorted(n for n in dir(ext) if not n.startswith("_")) == BINDINGS


def test_mda_select_has_no_fourth_argument(ext):
    D2 = torch.zeros(4, 4)
    with pytest.raises(TypeError):
        ext.mda_select(D2, 1, None, None)
    with pytest.raises(TypeError):
        ext.mda_select(D2, 1, ub=None, D2perm=None)


def _cpu_calls(ext):
    X = torch.randn(5, 8)
    vd, vn = torch.zeros(8), torch.ones(5)
    s0 = torch.zeros(())
    i1 = torch.tensor([0, 1], dtype=torch.int32)
    i2 = torch.tensor([[0, 1], [2, 3]], dtype=torch.int32)
    perm = torch.arange(5, dtype=torch.int32)
    G = torch.eye(5)
    return {
        "bucket_mean": lambda: ext.bucket_mean(X, perm, 2),
        "caf_colsum": lambda: ext.caf_colsum(X, vn),
        "caf_matvec": lambda: ext.caf_matvec(X, vd, vd),
        "cc_apply": lambda: ext.cc_apply(X, vd, vn, 0.5, 1e-12),
        "cc_iter": lambda: ext.cc_iter(X, vd, 0.5, 1e-12),
        "colsel": lambda: ext.colsel(X, 0, 0),
        "gaussian_fill": lambda: ext.gaussian_fill(8, 1, 0.0, 1.0, vd),
        "gram": lambda: ext.gram(X),
        "group_mean_rows": lambda: ext.group_mean_rows(X, i2),
        "krum_select": lambda: ext.krum_select(G, 1, 2),
        "little_fused": lambda: ext.little_fused(X, 1.0),
        "mda_select": lambda: ext.mda_select(G, 1),
        "mean_rows": lambda: ext.mean_rows(X, i1),
        "row_center_sqdists": lambda: ext.row_center_sqdists(X, vd),
        "row_scale": lambda: ext.row_scale(X, vn),
        "row_sqnorms": lambda: ext.row_sqnorms(X),
        "smea_select": lambda: ext.smea_select(G, i2),
        "weiszfeld_apply": lambda: ext.weiszfeld_apply(X, vd, vn, 1e-12, s0),
        "weiszfeld_iter": lambda: ext.weiszfeld_iter(X, vd, 1e-12, s0),
        "weiszfeld_iter_grouped": lambda: ext.weiszfeld_iter_grouped(
            torch.randn(2, 3, 8), torch.zeros(2, 8), 1e-12
        ),
    }


def test_every_device_binding_rejects_cpu_tensors(ext):
    calls = _cpu_calls(ext)
    # mda_search is the one host op; everything else takes device tensors
    assert sorted(calls) == [b for b in BINDINGS if b != "mda_search"]
    for name, call in calls.items():
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"{name} accepted a CPU tensor")


def test_mda_search_matches_python_dfs(ext, monkeypatch):
    g = torch.Generator().manual_seed(5)
    P = torch.randn(8, 3, generator=g)
    D2 = ((P[:, None, :] - P[None, :, :]) ** 2).sum(dim=2)
    D2 = 0.5 * (D2 + D2.T)
    native = tuple(int(i) for i in ext.mda_search(D2, 2))
    monkeypatch.setattr(hip, "extension", lambda: None)
    fallback = F.mda_subset(D2, 2)
    assert len(native) == 6
    assert native == fallback


# -- Gram-derived helpers -----------------------------------------------------


def _gram_inputs():
    g = torch.Generator().manual_seed(0)
    X = torch.randn(7, 5, generator=g)
    dup = X.clone()
    dup[4] = dup[1]  # two identical rows: exact distance / score ties
    zero = X.clone()
    zero[2] = 0.0
    return {"random": X, "duplicated_rows": dup, "zero_row": zero}


GRAM_INPUTS = _gram_inputs()
_F, _Q = 2, 3


@pytest.mark.parametrize("case", sorted(GRAM_INPUTS))
def test_gram_helpers_equal_the_written_out_chain(case):
    X = GRAM_INPUTS[case]
    n = X.shape[0]
    G = X @ X.T
    norms = torch.diagonal(G)
    D2 = (norms[:, None] + norms[None, :] - 2.0 * G).clamp_(min=0.0)
    assert torch.equal(D.sq_dists_from_gram(G), D2)

    D2i = D2 + torch.diag(
        torch.full((n,), float("inf"), device=G.device, dtype=D2.dtype)
    )
    scores = torch.topk(D2i, k=n - _F - 1, dim=1, largest=False).values.sum(dim=1)
    assert torch.equal(D.krum_scores_from_gram(G, _F), scores)

    winners = torch.topk(scores, k=_Q, largest=False).indices.to(torch.int32)
    got = D.krum_winners_from_gram(G, _F, _Q)
    assert got.dtype == torch.int32 and torch.equal(got, winners)

    k = n - _F
    idx = torch.topk(D2, k=k, dim=1, largest=False).indices
    assert torch.equal(D.nearest_rows_from_gram(G, k), idx)

    # batched form, as nnm_grouped wrote it
    Gm = torch.stack([G, 2.0 * G])
    nb = torch.diagonal(Gm, dim1=1, dim2=2)
    D2b = (nb[:, :, None] + nb[:, None, :] - 2.0 * Gm).clamp_(min=0.0)
    assert torch.equal(D.sq_dists_from_gram(Gm), D2b)
    idxb = torch.topk(D2b, k=k, dim=2, largest=False).indices
    assert torch.equal(D.nearest_rows_from_gram(Gm, k), idxb)


def test_gram_helpers_keep_dtype_and_device():
    G = (GRAM_INPUTS["random"] @ GRAM_INPUTS["random"].T).double()
    assert D.sq_dists_from_gram(G).dtype == torch.float64
    assert D.krum_scores_from_gram(G, _F).dtype == torch.float64
    assert D.krum_scores_from_gram(G, _F).device == G.device


@pytest.mark.parametrize("case", sorted(GRAM_INPUTS))
def test_krum_winners_match_functional_multi_krum(case):
    X = GRAM_INPUTS[case]
    got = D.krum_winners_from_gram(X @ X.T, _F, _Q).long()
    ref = torch.topk(F.multi_krum_scores(X, _F), k=_Q, largest=False).indices
    # identical rows are the same winner: name each by its first occurrence
    first = torch.tensor(
        [min(j for j in range(len(X)) if torch.equal(X[j], X[i])) for i in range(len(X))]
    )
    assert sorted(first[got].tolist()) == sorted(first[ref].tolist())
    assert torch.allclose(X[got].mean(dim=0), F.multi_krum(X, _F, _Q), atol=1e-6)
