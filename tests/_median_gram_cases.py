"""Shared by the three test files of the one-pass median + Gram kernel
(test_gpu_median_gram.py, _wave.py, _rawbits.py): the extension and the
strip-split fixtures, the call through the binding, the float64 Gram and the
bound a Gram of random data is held to. Fixtures reach a test file by import."""
import pytest
import torch

from byzpy_amd import hip


@pytest.fixture(scope="module")
def ext():
    return hip.require()


@pytest.fixture(params=["even", "ticket"])
def split(request, monkeypatch):
    """how the strips reach the waves: one even share each (what the binding
    picks at these sizes) or chunks drawn from the work counter (what it
    picks from 2^25 columns up), forced here so that the drawn loop runs at
    test sizes"""
    monkeypatch.setenv("BYZPY_MEDIAN_GRAM_TICKET",
                       "1" if request.param == "ticket" else "0")
    return request.param


def fused(ext, X, G=None):
    """(median, Gram) of ``ext.colsel(X, 0, 0, gram=G)``"""
    n = X.shape[0]
    if G is None:
        # garbage, not zeros: the call has to overwrite all of it
        G = torch.full((n, n), 1.0e9, dtype=torch.float32, device=X.device)
    med = ext.colsel(X, 0, 0, gram=G)
    return med, G


def gram_ref(X):
    Xd = X.cpu().double()
    return Xd @ Xd.T


def gram_bound(G_ref):
    """TestFusedGramMedian.test_parity's bound on max|G - G_ref|"""
    return 0.3 * max(1.0, float(G_ref.abs().max()) / 100)
