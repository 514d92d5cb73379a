"""Host model of the running observation normalisation (sacmi_set_obs_norm; csrc/obsnorm.hip,
DESIGN.md §20): the fp64 running moments merged chunk by chunk, the fp32 vectors derived from
them, and the fp32 normalise expression — plus the exact rational reference and the shared
fixture the CPU and GPU tests check against."""
import functools
from fractions import Fraction

import numpy as np

CHUNK = 1024        # rows per chunk that reaches the device (the push chunk)
ROW_LANES = 16      # k_obs_stats: row lanes whose partials are folded in lane order


class RunningMoments:
    """count, mean[S], M2[S] in fp64; chunks merged with Chan's formula (never E[x^2] - mean^2).
    form "chan": a chunk's own moments by two passes, then one merge; "welford": a per-row
    step; "device": as k_obs_stats — ROW_LANES Welford partials over rows l, l + 16, ...,
    folded in lane order, then merged."""

    def __init__(self, S, form="chan"):
        self.count = 0.0
        self.mean = np.zeros(S, np.float64)
        self.m2 = np.zeros(S, np.float64)
        self.form = form

    def _merge(self, n, mean, m2):
        if n == 0:
            return
        if self.count == 0:
            self.count, self.mean, self.m2 = float(n), mean.copy(), m2.copy()
            return
        tot = self.count + n
        d = mean - self.mean
        self.mean = self.mean + d * (n / tot)
        self.m2 = self.m2 + m2 + d * d * (self.count * n / tot)
        self.count = tot

    @staticmethod
    def _welford(x):
        n, mean, m2 = 0.0, np.zeros(x.shape[1]), np.zeros(x.shape[1])
        for row in x:
            n += 1.0
            d = row - mean
            mean = mean + d / n
            m2 = m2 + d * (row - mean)
        return n, mean, m2

    def update(self, rows):
        x = np.asarray(rows, np.float32).astype(np.float64).reshape(-1, self.mean.size)
        for i in range(0, len(x), CHUNK):
            c = x[i:i + CHUNK]
            if self.form == "welford":
                for row in c:
                    self._merge(1.0, row, np.zeros_like(row))
            elif self.form == "device":
                part = RunningMoments(self.mean.size)
                for lane in range(ROW_LANES):
                    part._merge(*self._welford(c[lane::ROW_LANES]))
                self._merge(part.count, part.mean, part.m2)
            else:
                mean = c.mean(axis=0)
                self._merge(float(len(c)), mean, ((c - mean) ** 2).sum(axis=0))
        return self


class NaiveMoments:
    """The form the feature must NOT use: running sums of x and x^2 in fp64, M2 = sum x^2 -
    count mean^2.  Kept as the control that misses the bound."""

    def __init__(self, S):
        self.count, self.sx, self.sxx = 0.0, np.zeros(S), np.zeros(S)

    def update(self, rows):
        x = np.asarray(rows, np.float32).astype(np.float64)
        self.count += len(x)
        self.sx += x.sum(axis=0)
        self.sxx += (x * x).sum(axis=0)
        return self

    @property
    def mean(self):
        return self.sx / self.count

    @property
    def m2(self):
        return self.sxx - self.count * self.mean ** 2


def vectors(count, mean, m2, eps):
    """(nmean, nrstd) float32: fp64 arithmetic, rounded once; count == 0 is the identity."""
    mean, m2 = np.asarray(mean, np.float64), np.asarray(m2, np.float64)
    if count == 0:
        return np.zeros(mean.size, np.float32), np.ones(mean.size, np.float32)
    with np.errstate(divide="ignore"):
        return mean.astype(np.float32), (1.0 / np.sqrt(m2 / count + eps)).astype(np.float32)


def normalize(x, nmean, nrstd, clip):
    """fp32: t = (x - nmean) * nrstd, then compares (a NaN stays a NaN; no fmin / fmax)."""
    x = np.asarray(x, np.float32)
    c = np.float32(clip)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (x - np.asarray(nmean, np.float32)) * np.asarray(nrstd, np.float32)
        return np.where(t < -c, -c, np.where(t > c, c, t)).astype(np.float32)


def exact_moments(rows):
    """(count, mean, M2) per column in exact rational arithmetic (lists of Fraction)."""
    x = np.asarray(rows, np.float32)
    n = len(x)
    mean, m2 = [], []
    for k in range(x.shape[1]):
        col = [Fraction(float(v)) for v in x[:, k]]
        mu = sum(col) / n
        mean.append(mu)
        m2.append(sum(v * v for v in col) - n * mu * mu)
    return n, mean, m2


def exact_vectors(n, mean, m2, eps):
    """The vectors from the exact moments: the square root in fp64 of a value that is itself
    the exact quotient rounded once (within 1 fp64 ulp of exact: far inside half an fp32 ulp
    unless the result sits on a rounding boundary)."""
    nmean = np.array([float(m) for m in mean], np.float64).astype(np.float32)
    var = np.array([float(v / n + Fraction(eps)) for v in m2], np.float64)
    return nmean, (1.0 / np.sqrt(var)).astype(np.float32)


N_ROWS, S_FIX = 5000, 11
CUTS = (0, 1, 17, 18, 1042, 4096, 5000)


@functools.lru_cache(maxsize=None)
def fixture_rows(S=S_FIX, n=N_ROWS, seed=20):
    """float32(0.5 N(0,1)) with column 3 = 4096 + 0.01 N, 5 = -2.5, 7 = 1e-3 + 1e-3 N,
    10 = 300 N: a large offset with a tiny spread, a constant, a tiny column, a huge one."""
    rng = np.random.default_rng(seed)
    x = (0.5 * rng.standard_normal((n, S))).astype(np.float32)
    x[:, 3] = (4096 + 0.01 * rng.standard_normal(n)).astype(np.float32)
    x[:, 5] = np.float32(-2.5)
    x[:, 7] = (1e-3 + 1e-3 * rng.standard_normal(n)).astype(np.float32)
    x[:, 10] = (300 * rng.standard_normal(n)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def fixture_exact(S=S_FIX, n=N_ROWS, seed=20):
    return exact_moments(fixture_rows(S, n, seed))


def ulp32(got, want):
    """|got - want| in fp32 ulps of want."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    sp = np.spacing(np.maximum(np.abs(want), np.float32(1e-38)))
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / sp.astype(np.float64)


def moment_errors(count, mean, m2, rows, exact=None):
    """(max relative M2 error, max mean error / max|x_k|) against exact arithmetic; a column
    whose exact M2 is 0 (a constant) counts its absolute M2 against max|x_k|^2 * count."""
    x = np.asarray(rows, np.float32).astype(np.float64)
    n, emean, em2 = exact if exact is not None else exact_moments(rows)
    assert count == n
    amax = np.abs(x).max(axis=0)
    e_m2 = 0.0
    for k in range(x.shape[1]):
        ref = float(em2[k])
        err = abs(float(Fraction(float(m2[k])) - em2[k]))
        e_m2 = max(e_m2, err / ref if ref > 0 else err / (amax[k] ** 2 * n))
    e_mean = max(abs(float(Fraction(float(mean[k])) - emean[k])) / amax[k] for k in range(x.shape[1]))
    return e_m2, e_mean
