"""Exact-arithmetic checker for the column order statistics (colsel modes
0 median, 1 trimmed mean, 2 mean-around-median), shared by
test_colsel_exact_checker.py (CPU) and test_gpu_colsel_exact.py.

Inputs. Every value is an integer that the dtype under test holds exactly,
and small enough that every partial sum of a column is an exact f32 in any
order (n * max|x| <= 2^24 with integer terms): f32 data is |x| <= 1024 for
n <= 1024; bf16 data is |x| <= 255 for n <= 255 and bf16-exact integers
m * 2^e with |x| <= 2^14 for n <= 1024. A kernel that sums in f32 can then
differ from the float64 value only by its final divide and its output
rounding.

Three families, each drawn independently per column, so that one call checks
d rank patterns:
  distinct  n distinct values per column;
  balanced  a multiset symmetric about a per-column integer c, |c| <= 2
            (c = 0 where bf16 needs the m * 2^e integers), rows shuffled per
            column: the true result is tiny, so that an error of 1/k shows at
            full relative precision even in a bf16 output;
  ties      values from {-3..3}: every boundary is a tie.

Expected values come from a float64 sort. Median and trimmed mean have one
valid value. Mean-around-median has a SET, because the engines break
deviation ties differently (the packed and LDS kernels drop the right end
first, the f32 register kernel follows its key-value network, the radix
engine takes the left ties first, F.mean_of_medians follows topk). With
k = n - f, rho the k-th smallest |x - med|, S_below the sum of the values
with deviation below rho, t = k - #below, and cL / cR the number of ties at
med - rho / med + rho, the valid results are

    (S_below + j * (med - rho) + (t - j) * (med + rho)) / k
    for max(0, t - cR) <= j <= min(t, cL).

Sums are built with torch.where, never by multiplying with a mask: the
extreme-row inputs hold +-inf, and inf * 0 is NaN.

Tolerance: derived, relative to the valid value, no absolute term.
  f32 outputs   2^-21: three roundings of 2^-24 (a reciprocal, a product, a
                conversion) with a factor 2.67 of slack;
  bf16 outputs  2^-8: the unit roundoff of the output format.
A result is accepted if it is within tolerance of any valid value; every
column has to be accepted. No column is ever masked out."""
import torch

MEDIAN, TRIMMED, MEAMED = 0, 1, 2
MODES = (MEDIAN, TRIMMED, MEAMED)
FAMILIES = ("distinct", "balanced", "ties")
TOL = {torch.float32: 2.0 ** -21, torch.bfloat16: 2.0 ** -8}


# -- inputs -----------------------------------------------------------------


def magnitudes(n, dtype):
    """The positive magnitudes (ascending, float64) the families draw from."""
    if dtype == torch.float32:
        assert n <= 1024
        return torch.arange(1, 1025, dtype=torch.float64)
    assert dtype == torch.bfloat16 and n <= 1024
    if n <= 255:
        return torch.arange(1, 256, dtype=torch.float64)
    # bf16 has 8 significant bits: every integer to 256, then 128 per octave
    m = [torch.arange(1, 257, dtype=torch.float64)]
    for e in range(1, 7):
        m.append(torch.arange(129, 257, dtype=torch.float64) * 2.0 ** e)
    return torch.cat(m)  # 1024 values, the largest 2^14


def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def _shuffle_rows(X, g):
    """an independent row permutation in every column"""
    order = torch.rand(X.shape, generator=g, device=X.device).argsort(dim=0)
    return X.gather(0, order)


def make(family, n, d, dtype, seed=0, device="cpu"):
    """An (n, d) matrix of ``dtype`` from one of FAMILIES."""
    g = _gen(seed, device)
    if family == "ties":
        X = torch.randint(-3, 4, (n, d), generator=g, device=device).double()
        return X.to(dtype)
    mag = magnitudes(n, dtype).to(device)
    if family == "distinct":
        pool = torch.cat([-mag.flip(0), mag.new_zeros(1), mag])
        pick = torch.rand(pool.numel(), d, generator=g, device=device)
        X = pool[pick.argsort(dim=0)[:n]]
    elif family == "balanced":
        small = dtype == torch.float32 or n <= 255
        h = n // 2
        if small:
            c = torch.randint(-2, 3, (d,), generator=g, device=device).double()
            mag = mag[: mag.numel() - 2]  # |c +- a| stays inside the range
        else:
            c = torch.zeros(d, dtype=torch.float64, device=device)
        pick = torch.rand(mag.numel(), d, generator=g, device=device)
        a = mag[pick.argsort(dim=0)[:h]]
        parts = [c[None] - a, c[None] + a]
        if n % 2:
            parts.append(c[None])
        X = _shuffle_rows(torch.cat(parts, dim=0), g)
    else:
        raise ValueError(family)
    out = X.to(dtype)
    assert torch.equal(out.double(), X), "values must be exact in the dtype"
    return out.contiguous()


def plant_extremes(X, count, kind, seed=0):
    """A copy of X in which every column has ``count`` rows, chosen
    independently per column, replaced by extreme values: kind is '+big',
    '-big', 'mixbig' (+-1e30), '+inf', '-inf' or 'mixinf'."""
    n, d = X.shape
    g = _gen(seed, X.device)
    where = torch.rand(n, d, generator=g, device=X.device).argsort(dim=0)[:count]
    mag = float("inf") if kind.endswith("inf") else 1e30
    if kind.startswith("+"):
        sign = torch.ones(count, d, device=X.device)
    elif kind.startswith("-"):
        sign = -torch.ones(count, d, device=X.device)
    else:
        sign = torch.randint(0, 2, (count, d), generator=g, device=X.device) * 2.0 - 1.0
    Y = X.clone()
    Y.scatter_(0, where, (sign * mag).to(X.dtype))
    return Y


# -- expected values --------------------------------------------------------


class Exact:
    """The float64 order statistics of one matrix (any dtype, any device);
    the sort is done once and shared by every mode and f."""

    def __init__(self, X):
        self.X = X.double()
        self.n, self.d = X.shape
        self.dtype = X.dtype
        self.s = self.X.sort(dim=0).values
        n = self.n
        self.med = 0.5 * (self.s[(n - 1) // 2] + self.s[n // 2])
        self._dev = None

    def median(self):
        return self.med

    def trimmed(self, f):
        n = self.n
        assert 0 <= 2 * f < n
        return self.s[f:n - f].sum(dim=0) / (n - 2 * f)

    def meamed(self, f):
        """(base, step, jmin, jmax, k): the valid values are
        (base - j * step) / k for jmin <= j <= jmax (integers per column)."""
        n = self.n
        assert 0 <= f < n
        k = n - f
        if self._dev is None:
            dev = (self.X - self.med[None]).abs()
            self._dev = (dev, dev.sort(dim=0).values)
        dev, sdev = self._dev
        rho = sdev[k - 1]
        below = dev < rho[None]
        zero = torch.zeros((), dtype=torch.float64, device=self.X.device)
        s_below = torch.where(below, self.X, zero).sum(dim=0)
        t = k - below.sum(dim=0)
        tie = dev == rho[None]
        left = tie & (self.X < self.med[None])
        c_l = left.sum(dim=0)
        c_r = (tie & ~left).sum(dim=0)
        jmin = (t - c_r).clamp(min=0)
        jmax = torch.minimum(t, c_l)
        assert bool((jmin <= jmax).all())
        base = s_below + t * (self.med + rho)
        return base, 2.0 * rho, jmin, jmax, k

    def valid_values(self, mode, f=0):
        """Dense (J, d) table of the valid values, NaN where a column has
        fewer than J. For small cases and for checking the checker."""
        if mode == MEDIAN:
            return self.median()[None]
        if mode == TRIMMED:
            return self.trimmed(f)[None]
        base, step, jmin, jmax, k = self.meamed(f)
        J = int((jmax - jmin).max()) + 1
        j = jmin[None] + torch.arange(J, device=base.device)[:, None]
        vals = (base[None] - j * step[None]) / k
        nan = torch.full((), float("nan"), dtype=torch.float64, device=base.device)
        return torch.where(j <= jmax[None], vals, nan)

    def rejected(self, got, mode, f=0, tol=None):
        """Bool (d,): the columns of ``got`` within tolerance of no valid
        value. The tolerance is that of got's dtype."""
        tol = TOL[got.dtype] if tol is None else tol
        g = got.double().to(self.X.device)
        assert g.shape == (self.d,)
        if mode == MEDIAN:
            cands = [self.median()]
        elif mode == TRIMMED:
            cands = [self.trimmed(f)]
        else:
            base, step, jmin, jmax, k = self.meamed(f)
            # the valid values are evenly spaced: only the ones next to
            # ``got`` can accept it
            safe = torch.where(step > 0, step, torch.ones_like(step))
            j0 = torch.nan_to_num((base - g * k) / safe, nan=0.0, posinf=0.0, neginf=0.0)
            j0 = j0.round().clamp(-1e9, 1e9).long()
            cands = []
            for dj in (-1, 0, 1):
                j = torch.minimum(torch.maximum(j0 + dj, jmin), jmax)
                cands.append((base - j * step) / k)
        ok = torch.zeros(self.d, dtype=torch.bool, device=g.device)
        for v in cands:
            ok |= (g - v).abs() <= tol * v.abs()
        return ~ok


def check(got, ex, mode, f=0, what=""):
    """Assert that every column of ``got`` is accepted by ``ex`` (an Exact)."""
    bad = ex.rejected(got, mode, f)
    if bool(bad.any()):
        cols = bad.nonzero().flatten()[:4].tolist()
        vals = ex.valid_values(mode, f)[:3, cols].tolist()
        raise AssertionError(
            f"{what} mode={mode} n={ex.n} d={ex.d} f={f}: {int(bad.sum())} of "
            f"{ex.d} columns rejected; columns {cols} got "
            f"{got.double()[cols].tolist()}, valid (first 3) {vals}"
        )


def f_values(n, mode):
    """The f swept by the tests: every legal one to n = 16, then
    {0, 1, 2, (n-1)//4, (n-1)//2, (n-1)//2 + 1, n-2, n-1} cut to what the mode
    allows (2f < n trimmed, f < n mean-around-median)."""
    if mode == MEDIAN:
        return [0]
    legal = (lambda f: 0 <= 2 * f < n) if mode == TRIMMED else (lambda f: 0 <= f < n)
    if n <= 16:
        cand = range(n)
    else:
        cand = {0, 1, 2, (n - 1) // 4, (n - 1) // 2, (n - 1) // 2 + 1, n - 2, n - 1}
    return sorted(f for f in cand if legal(f))
