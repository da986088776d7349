"""The raw-word selection network of the one-pass median + Gram kernel
(colsel.hip: median_gram_bf16_kernel) and its guarded fallback, through the
binding ``ext.colsel(X, 0, 0, gram=G)``.

The fused kernel orders the raw bf16 words with v_pk_min_f16 / v_pk_max_f16.
That is the order of the values for the 63,488 "legal" patterns whose
magnitude bits are below 0x7C00 (|x| < 2^121); any other word makes its row's
diagonal Gram entry non-finite, and a second kernel on the same stream then
recomputes the whole median with the u16-key kernel.

The reference for the median is always ``ext.colsel(X, 0, 0)``, the u16-key
kernel, and medians are compared BITWISE (as int16, so that -0 / +0 and NaN
payloads count). The Gram is compared as tests/test_gpu_median_gram_wave.py
does it.

Which kernel answers: f32 holds a row's sum of squares only while the words
stay below about 2^64 / sqrt(d), far under 2^121. The full-range cases below
(every legal pattern, pads of 0xFBFF / 0x7BFF) therefore overflow the Gram and
are answered by guard + fallback; they pin the whole call. The ``in_range``
cases hold the same patterns below 2^50 in magnitude (45,312 of them: all
f16-subnormal patterns, both zeros, everything up to 0x587F), assert that the
Gram's diagonal IS finite, and so pin the f16 network itself: -0 / +0 order,
subnormal pass-through, operand order.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from _median_gram_cases import (ext, fused, gram_bound, gram_ref,  # noqa: F401
                                 split)
from byzpy_amd.hip.graphs import CapturedAggregate

NS = [33, 48, 63, 64]
DS = [2, 126, 128, 130, 514, 1022]
D_MULTI_CHUNK = 2 * 512 * 512 + 514

LEGAL_MAG = 0x7C00      # magnitude bits of the legal patterns: [0, 0x7C00)
IN_RANGE_MAG = 0x5880   # 2^50: d * 2^100 stays finite in f32 for d < 2^28


def _i16(pattern):
    """a 16-bit pattern as the int16 value with those bits"""
    return pattern - 0x10000 if pattern >= 0x8000 else pattern


def _bf16(bits):
    """integer tensor of 16-bit patterns -> bf16 tensor on the device"""
    b = bits.to("cuda").to(torch.int32) & 0xFFFF
    b = torch.where(b >= 0x8000, b - 0x10000, b)
    return b.to(torch.int16).view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int16)


def _patterns(mag_end, device="cuda"):
    """every pattern with magnitude bits below mag_end, both signs"""
    m = torch.arange(mag_end, device=device, dtype=torch.int32)
    return torch.cat([m, m | 0x8000])


def _assert_median_bits(ext, X, med):
    ref = ext.colsel(X, 0, 0)
    wrong = (_bits(med) != _bits(ref)).nonzero()
    assert wrong.numel() == 0, (
        f"{wrong.shape[0]} of {med.numel()} medians differ, first at column "
        f"{wrong[0].item()}: got {_bits(med)[wrong[0]].item() & 0xFFFF:#06x}, "
        f"expected {_bits(ref)[wrong[0]].item() & 0xFFFF:#06x}"
    )


def _assert_gram_within_bound(G, X):
    G_ref = gram_ref(X)
    bound = gram_bound(G_ref)
    err = (G.cpu().double() - G_ref).abs().max().item()
    print(f"n={X.shape[0]} d={X.shape[1]} gram err {err:.4g} bound {bound:.4g}")
    assert err < bound


# --------------------------------------------------------------------------
# 1. compare-exchange semantics through the kernel
# --------------------------------------------------------------------------

def _specials(top):
    """the 16 special partners: +-0, smallest / largest f16-subnormal pattern
    of either sign, +-0x0400 (the smallest f16-normal), +-0x3F80 (one),
    +-top (the largest pattern of the span), and mid-range values (four: the
    named ones are 14)"""
    return torch.tensor(
        [0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x8400,
         0x3F80, 0xBF80, top, top | 0x8000, 0x4049, 0xC2F7, 0x1234, 0x9ABC],
        dtype=torch.int32, device="cuda")


def _pairs(mag_end, seed):
    """(a, b): every pattern against each of 16 special partners, then 2^20
    random pairs"""
    pats = _patterns(mag_end)
    sp = _specials(mag_end - 1)
    assert sp.numel() == 16 and int((sp & 0x7FFF).max()) < mag_end
    a = pats.repeat_interleave(16)
    b = sp.repeat(pats.numel())
    g = torch.Generator(device="cuda").manual_seed(seed)
    ra = pats[torch.randint(pats.numel(), (1 << 20,), generator=g, device="cuda")]
    rb = pats[torch.randint(pats.numel(), (1 << 20,), generator=g, device="cuda")]
    return torch.cat([a, ra]), torch.cat([b, rb]), g


def _semantics_matrix(a, b, lo_fill, hi_fill, n_lo, g):
    """63 x m: per column n_lo copies of lo_fill, then a, b, then copies of
    hi_fill, in a per-column shuffled row order"""
    m = a.numel()
    base = torch.empty((63, m), dtype=torch.int32, device="cuda")
    base[:n_lo] = lo_fill
    base[n_lo] = a
    base[n_lo + 1] = b
    base[n_lo + 2:] = hi_fill
    out = torch.empty_like(base)
    step = 1 << 19
    for c in range(0, m, step):
        perm = torch.rand((63, min(step, m - c)), generator=g,
                          device="cuda").argsort(dim=0)
        out[:, c:c + step] = base[:, c:c + step].gather(0, perm)
    return _bf16(out)


def _key(bits):
    """the value order of legal patterns as an integer (-0 below +0)"""
    bits = bits & 0xFFFF
    return torch.where(bits >= 0x8000, -(bits & 0x7FFF) - 1, bits)


@pytest.mark.parametrize("role", ["max", "min"])
@pytest.mark.parametrize("span", ["full_range", "in_range"])
def test_compare_exchange_semantics(ext, span, role):
    # n = 63 is odd: the output is the bits of ONE element. 30 low + a, b +
    # 31 high puts max(a, b) at the median's rank; 31 low + 30 high puts
    # min(a, b) there.
    mag_end = LEGAL_MAG if span == "full_range" else IN_RANGE_MAG
    a, b, g = _pairs(mag_end, seed=17 if role == "max" else 18)
    lo_fill, hi_fill = 0x8000 | (mag_end - 1), mag_end - 1
    X = _semantics_matrix(a, b, lo_fill, hi_fill, 30 if role == "max" else 31, g)
    assert X.shape[1] % 2 == 0
    med, G = fused(ext, X)
    finite = bool(torch.isfinite(G.diagonal()).all())
    print(f"{span} {role}: {X.shape[1]} columns, Gram diagonal finite: {finite}")
    if span == "in_range":
        assert finite  # the f16 network's own answer, not the fallback's
    # what the order of the values says, independent of either kernel
    ka, kb = _key(a), _key(b)
    pick_a = (ka >= kb) if role == "max" else (ka <= kb)
    want = torch.where(pick_a, a, b) & 0xFFFF
    got = _bits(med).to(torch.int32) & 0xFFFF
    wrong = (got != want).nonzero()
    assert wrong.numel() == 0, (
        f"{wrong.shape[0]} wrong, first: a={a[wrong[0]].item():#06x} "
        f"b={b[wrong[0]].item():#06x} got {got[wrong[0]].item():#06x}")
    _assert_median_bits(ext, X, med)


# --------------------------------------------------------------------------
# 2. random legal patterns, uniform over the patterns
# --------------------------------------------------------------------------

def _uniform_patterns(n, d, mag_end, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    bits = torch.randint(2 * mag_end, (n, d), generator=g, device="cuda",
                         dtype=torch.int32)
    # [0, mag_end) positive, [mag_end, 2 mag_end) the same magnitudes negative
    bits = torch.where(bits >= mag_end, (bits - mag_end) | 0x8000, bits)
    return _bf16(bits)


@pytest.mark.parametrize("span", ["full_range", "in_range"])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", DS)
def test_uniform_patterns(ext, split, span, n, d):
    mag_end = LEGAL_MAG if span == "full_range" else IN_RANGE_MAG
    X = _uniform_patterns(n, d, mag_end, seed=1000 * n + d)
    med, G = fused(ext, X)
    if span == "in_range":
        assert bool(torch.isfinite(G.diagonal()).all())
    _assert_median_bits(ext, X, med)


@pytest.mark.parametrize("span", ["full_range", "in_range"])
def test_uniform_patterns_multi_chunk(ext, split, span):
    mag_end = LEGAL_MAG if span == "full_range" else IN_RANGE_MAG
    X = _uniform_patterns(64, D_MULTI_CHUNK, mag_end, seed=5)
    med, G = fused(ext, X)
    if span == "in_range":
        assert bool(torch.isfinite(G.diagonal()).all())
    _assert_median_bits(ext, X, med)


# --------------------------------------------------------------------------
# 3. Gaussian rows with exact zeros of both signs
# --------------------------------------------------------------------------

def _gauss(n, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.randn(n, d, generator=g, device="cuda")
    X *= (1.0 + torch.arange(n, device="cuda", dtype=torch.float32) / n)[:, None]
    return X, g


def _gauss_with_zeros(n, d, seed):
    """half of each column is zero, +0 and -0 mixed"""
    X, g = _gauss(n, d, seed)
    X = X.to(torch.bfloat16)
    u = torch.rand((n, d), generator=g, device="cuda")
    rank = u.argsort(dim=0).argsort(dim=0)
    zero = rank < n // 2
    neg = torch.rand((n, d), generator=g, device="cuda") < 0.5
    z = torch.where(neg, torch.tensor(-0.0, device="cuda"),
                    torch.tensor(0.0, device="cuda")).to(torch.bfloat16)
    return torch.where(zero, z, X)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", DS)
def test_gaussian_with_signed_zeros(ext, split, n, d):
    X = _gauss_with_zeros(n, d, seed=7000 + 100 * n + d)
    assert bool((_bits(X) == _i16(0x8000)).any())  # -0 is there
    assert bool((_bits(X) == 0).any())
    med, G = fused(ext, X)
    assert bool(torch.isfinite(G.diagonal()).all())
    _assert_median_bits(ext, X, med)
    _assert_gram_within_bound(G, X)
    assert torch.equal(G, G.T)


def test_gaussian_with_signed_zeros_multi_chunk(ext, split):
    X = _gauss_with_zeros(64, D_MULTI_CHUNK, seed=71)
    med, G = fused(ext, X)
    assert bool(torch.isfinite(G.diagonal()).all())
    _assert_median_bits(ext, X, med)
    _assert_gram_within_bound(G, X)


def test_integer_data_gram_is_exact(ext, split):
    # the Gram side is untouched: integers in {-2..2} give exact sums
    g = torch.Generator().manual_seed(3)
    X = torch.randint(-2, 3, (48, 1022), generator=g).to("cuda", torch.bfloat16)
    med, G = fused(ext, X)
    assert torch.equal(G.cpu().double(), gram_ref(X))
    _assert_median_bits(ext, X, med)


# --------------------------------------------------------------------------
# 4. fallback
# --------------------------------------------------------------------------

D_FALLBACK = 1022  # 7 full strips of 128 columns and a partial one of 126
POSITIONS = {"first_strip": 5, "middle_strip": 3 * 128 + 77,
             "partial_last_strip": D_FALLBACK - 1}
ILLEGAL = {"pinf": 0x7F80, "ninf": 0xFF80, "nan": 0x7FC0,
           "2p121": 0x7C00, "m2p121": 0xFC00}


@pytest.mark.parametrize("n", [64, 33])
@pytest.mark.parametrize("where", list(POSITIONS))
@pytest.mark.parametrize("what", list(ILLEGAL))
def test_one_illegal_word_falls_back(ext, n, where, what):
    X, _ = _gauss(n, D_FALLBACK, seed=n + 13)
    X = X.to(torch.bfloat16)
    row, col = (2 * n) // 3, POSITIONS[where]
    _bits(X)[row, col] = _i16(ILLEGAL[what])
    med, G = fused(ext, X)
    assert not bool(torch.isfinite(G[row, row]))
    _assert_median_bits(ext, X, med)


def test_legal_words_whose_gram_overflows(ext):
    # +-2^63: every word is legal, every diagonal entry is 1022 * 2^126 = inf
    g = torch.Generator(device="cuda").manual_seed(9)
    sign = torch.randint(0, 2, (64, D_FALLBACK), generator=g, device="cuda",
                         dtype=torch.int32)
    X = _bf16(0x5F00 | (sign << 15))
    assert float(X.float().abs().min()) == 2.0**63
    med, G = fused(ext, X)
    assert bool(torch.isinf(G.diagonal()).all())
    _assert_median_bits(ext, X, med)


# --------------------------------------------------------------------------
# 5. graph capture
# --------------------------------------------------------------------------

def test_graph_capture_and_replay(ext, split):
    n, d = 64, 4 * 512 + 130
    Xa, _ = _gauss(n, d, seed=41)
    Xa = Xa.to(torch.bfloat16)
    Xb = Xa.flip(0).contiguous()
    _bits(Xb)[7, d - 3] = 0x7FC0  # a NaN: this replay must take the fallback
    G = torch.empty((n, n), dtype=torch.float32, device="cuda")
    cap = CapturedAggregate(lambda X: ext.colsel(X, 0, 0, gram=G), Xa)
    for X in (Xa, Xb, Xa):
        med = cap.run(X).clone()
        G_replay = G.clone()
        eager, G_eager = fused(ext, X)
        assert torch.equal(_bits(med), _bits(eager))
        assert torch.equal(torch.isfinite(G_replay), torch.isfinite(G_eager))
        assert bool(torch.isfinite(G_replay.diagonal()).all()) == (X is Xa)
        _assert_median_bits(ext, X, med)
