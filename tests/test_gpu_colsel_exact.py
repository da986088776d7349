"""Every colsel engine against exact float64 expected values.

Inputs are integers chosen so that f32 summation is exact in any order
(tests/_colsel_exact.py), so a kernel may differ from the float64 value only
by its final divide and output rounding: the tolerance is 2^-21 relative for
f32 outputs and 2^-8 (the unit roundoff) for bf16 outputs, with no absolute
term, and mean-around-median ties are handled by the set of valid values and
by nothing else. No column is masked out.

Which engine a shape reaches (bind.cpp): n <= 64 the register kernels, and
for bf16 with even d the packed kernel; 64 < n <= 512 at d < 32768 the
cooperative LDS sort; n > 512, or n > 64 at d >= 32768, the radix engine."""
import pytest
import torch

import _colsel_exact as CE
from byzpy_amd.hip import dispatch as D

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
EVEN_D, ODD_D = 322, 323  # 161 pairs: not a multiple of 64, more than a wave
LDS_D, RADIX_D = 130, 32768


def _run(X, mode, f, rows=None):
    if mode == CE.MEDIAN:
        return D.median(X, rows=rows)
    if mode == CE.TRIMMED:
        return D.trimmed_mean(X, f, rows=rows)
    return D.mean_of_medians(X, f, rows=rows)


def _collect(fails, got, ex, mode, f, what):
    assert got.dtype == ex.dtype and got.shape == (ex.d,)
    try:
        CE.check(got, ex, mode, f, what=what)
    except AssertionError as e:
        fails.append(str(e))


def _sweep(n, d, dtype, f_values, seed):
    """all families x modes x f of one shape; every failure is reported"""
    fails = []
    for family in CE.FAMILIES:
        X = CE.make(family, n, d, dtype, seed=seed, device=DEV)
        ex = CE.Exact(X)
        for mode in CE.MODES:
            for f in f_values(n, mode):
                _collect(fails, _run(X, mode, f), ex, mode, f, family)
    assert not fails, "\n".join(fails[:12])


# -- register and packed kernels: every n, every pad count --------------------


@pytest.mark.parametrize("n", range(1, 65))
@pytest.mark.parametrize("d", [EVEN_D, ODD_D])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_register_and_packed(dtype, d, n):
    """f = n - 1 at n = 64, bf16, even d is the packed mean-around-median
    kernel's largest dynamic LDS request (256 * 129 words, 132 KB)."""
    _sweep(n, d, dtype, CE.f_values, seed=1000 * d + n)


@pytest.mark.parametrize("n", range(33, 65))
def test_fused_median_gram_median(n, monkeypatch):
    """the median of the one-pass median + Gram kernel (bf16, 32 < n <= 64,
    even d), which sorts raw words with packed f16 min/max. The dispatch
    layer sends d below MEDIAN_GRAM_FUSED_MIN_D to the two-kernel pair, so
    the threshold is lowered for the second call."""
    fails = []
    for family in CE.FAMILIES:
        X = CE.make(family, n, EVEN_D, torch.bfloat16, seed=n, device=DEV)
        ex = CE.Exact(X)
        med, _ = D.median_and_gram(X)
        _collect(fails, med, ex, CE.MEDIAN, 0, f"pair {family}")
        with monkeypatch.context() as m:
            m.setattr(D, "MEDIAN_GRAM_FUSED_MIN_D", 2)
            assert D._median_gram_fused_ok(X)
            med, _ = D.median_and_gram(X)
        _collect(fails, med, ex, CE.MEDIAN, 0, f"fused {family}")
    assert not fails, "\n".join(fails)


# -- LDS sort: P = 128, 256, 512, full and partial ----------------------------


@pytest.mark.parametrize("n", [65, 100, 128, 129, 257, 512])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_lds(dtype, n):
    _sweep(n, LDS_D, dtype, CE.f_values, seed=n)


# -- radix engine, reached for certain ----------------------------------------


def _radix_f(n, mode):
    if mode == CE.MEDIAN:
        return [0]
    fs = {0, 1, n // 8, (n - 1) // 2}
    if mode == CE.MEAMED:
        fs |= {n - n // 4, n - 1}
    return sorted(fs)


@pytest.mark.parametrize(
    "n,d", [(513, LDS_D), (777, LDS_D), (1000, LDS_D),
            (65, RADIX_D), (100, RADIX_D), (192, RADIX_D)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_radix(dtype, n, d):
    assert n > 512 or (n > 64 and d >= 32768)  # bind.cpp's routing rule
    _sweep(n, d, dtype, _radix_f, seed=n + d)


# -- rows=: against the checker, not against the gathered call ----------------


@pytest.mark.parametrize(
    "n_src,m,d,dtype",
    [(40, 23, ODD_D, torch.float32), (70, 64, ODD_D, torch.bfloat16),
     (90, 34, EVEN_D, torch.bfloat16), (600, 100, LDS_D, torch.float32),
     (300, 257, LDS_D, torch.bfloat16)],
    ids=["register-f32", "register-bf16", "packed-bf16", "lds-f32", "lds-bf16"])
def test_rows(n_src, m, d, dtype):
    X = CE.make("distinct", n_src, d, dtype, seed=n_src, device=DEV)
    g = torch.Generator().manual_seed(m)
    rows = torch.randperm(n_src, generator=g)[:m]
    assert rows.tolist() != sorted(rows.tolist())  # non-monotone
    rows = rows.to(DEV, torch.int32)
    ex = CE.Exact(X[rows.long()])
    fails = []
    for mode in CE.MODES:
        for f in CE.f_values(m, mode):
            _collect(fails, _run(X, mode, f, rows=rows), ex, mode, f, "rows")
    assert not fails, "\n".join(fails[:12])


# -- pure selection on arbitrary bit patterns ---------------------------------

_BITS = {torch.float32: (32, 23), torch.bfloat16: (16, 7)}


def _from_bits(bits, dtype):
    """int64 bit patterns -> tensor of ``dtype``"""
    width, _ = _BITS[dtype]
    signed = torch.where(bits >= 2 ** (width - 1), bits - 2 ** width, bits)
    if dtype == torch.float32:
        return signed.to(torch.int32).view(torch.float32)
    return signed.to(torch.int16).view(torch.bfloat16)


def _bit_data(kind, n, d, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    width, mant = _BITS[dtype]
    sign = 2 ** (width - 1)
    inf = sign - 2 ** mant  # the pattern of +inf: the largest non-NaN
    if kind == "allbits":
        # uniform over every non-NaN pattern: all exponents, both signs,
        # subnormals, +-0, and +-inf per element
        i = torch.randint(0, 2 * (inf + 1), (n, d), generator=g, device=DEV)
        bits = torch.where(i <= inf, i, sign + (i - inf - 1))
    elif kind == "ulps":
        # base + j ulps: a column's keys differ only in their last 6..12 bits
        s = torch.randint(0, 2, (d,), generator=g, device=DEV) * sign
        top = width - 1 - 12  # magnitude bits above the low 12
        hi = torch.randint(0, 2 ** top - 2 ** max(top - 3, 0), (d,), generator=g,
                           device=DEV)
        base = s + hi * 4096
        w = 6 + torch.arange(d, device=DEV) % 7
        off = (torch.rand(n, d, generator=g, device=DEV) * (2.0 ** w)[None]).long()
        bits = base[None] + off
    elif kind == "zeros":
        # columns that straddle zero: both zeros and the smallest subnormals
        s = torch.randint(0, 2, (n, d), generator=g, device=DEV) * sign
        bits = s + torch.randint(0, 8, (n, d), generator=g, device=DEV)
    else:
        raise ValueError(kind)
    X = _from_bits(bits, dtype).contiguous()
    assert not bool(torch.isnan(X).any())
    return X


@pytest.mark.parametrize("kind", ["allbits", "ulps", "zeros"])
@pytest.mark.parametrize(
    "n,d", [(7, EVEN_D), (33, EVEN_D), (63, EVEN_D), (33, ODD_D), (63, ODD_D),
            (129, LDS_D), (101, RADIX_D), (777, LDS_D)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_selection_bit_patterns(dtype, n, d, kind):
    """odd n: the median, and the trimmed mean with f = (n-1)//2, each return
    one input element, so any float compares exactly (NaN inputs stay out:
    their order statistics are documented as unspecified; -0 == +0)."""
    X = _bit_data(kind, n, d, dtype, seed=n + d)
    if kind == "ulps":
        assert bool((X.double().max(0).values > X.double().min(0).values).any())
    want = X.double().sort(dim=0).values[n // 2].to(dtype)
    assert torch.equal(D.median(X), want), "median"
    assert torch.equal(D.trimmed_mean(X, (n - 1) // 2), want), "trimmed"


# -- the 16-bit histogram ceiling ---------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_radix_histogram_ceiling(dtype):
    """n = 65535: a bin holds 0xFFFF in either half of its packed word.
    Columns are constant, 65534 copies of a and one b, or split half and
    half; |values| <= 255 keeps every sum below 2^24."""
    n, d = 65535, 64
    g = torch.Generator(device=DEV).manual_seed(65535)
    a = torch.randint(-255, 256, (d,), generator=g, device=DEV).double()
    b = torch.randint(-255, 256, (d,), generator=g, device=DEV).double()
    order = torch.rand(n, d, generator=g, device=DEV).argsort(dim=0)
    col = torch.arange(d, device=DEV)
    nb = torch.where(col % 3 == 0, 0, torch.where(col % 3 == 1, 1, n // 2))
    X = torch.where(order < nb[None], b[None], a[None]).to(dtype).contiguous()
    ex = CE.Exact(X)
    fails = []
    for mode in CE.MODES:
        for f in _radix_f(n, mode):
            _collect(fails, _run(X, mode, f), ex, mode, f, "ceiling")
    assert not fails, "\n".join(fails[:12])


# -- extreme rows: the breakdown contract, exactly ----------------------------

_EXTREME_SHAPES = [
    (7, EVEN_D), (24, EVEN_D), (64, EVEN_D), (24, ODD_D), (64, ODD_D),
    (129, LDS_D), (513, LDS_D), (100, RADIX_D)]


@pytest.mark.parametrize("kind", ["+big", "-big", "mixbig", "+inf", "-inf", "mixinf"])
@pytest.mark.parametrize("n,d", _EXTREME_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_extreme_rows(dtype, n, d, kind):
    """In every column an independently chosen set of n // 3 rows is +-1e30
    or +-inf. With f at least that many, the trimmed mean and the
    mean-around-median have to be the exact honest value: no accumulator may
    ever hold a dropped element."""
    b = n // 3
    H = CE.make("distinct", n, d, dtype, seed=n + d, device=DEV)
    X = CE.plant_extremes(H, b, kind, seed=n)
    ex = CE.Exact(X)
    half = (n - 1) // 2
    fails = []
    for mode, fs in ((CE.TRIMMED, {b, half}), (CE.MEAMED, {b, half + 1, n - 2})):
        for f in sorted(fs):
            assert f >= b
            valid = ex.valid_values(mode, f)[0]
            assert bool(torch.isfinite(valid).all())
            _collect(fails, _run(X, mode, f), ex, mode, f, kind)
    assert not fails, "\n".join(fails)
