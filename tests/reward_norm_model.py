"""Host model of the reward scaling and running return normalisation (sacmi_set_reward_norm;
csrc/retnorm.hip): the fp64 return recurrence, the running moments of the returns
merged chunk by chunk, the fp32 factor and the fp32 normalise expression — plus the exact rational
reference and the shared fixture the CPU and GPU tests check against."""
import functools
from fractions import Fraction

import numpy as np

CHUNK = 1024        # rows per chunk that reaches the device (the push chunk)
ROW_LANES = 16      # k_ret_stats: Welford lanes over rows l, l + 16, ..., folded in lane order


def _welford(xs):
    n, mean, m2 = 0.0, 0.0, 0.0
    for x in xs:
        n += 1.0
        d = x - mean
        mean = mean + d / n
        m2 = m2 + d * (x - mean)
    return n, mean, m2


class ReturnStats:
    """ret, count, mean, M2 in fp64.  Per stored row, in push order: ret = fl(fl(ret * gamma) +
    r) (two roundings), the moments take ret, ret = 0 behind a terminal or a flagged row.
    form "serial": one Welford step per row; "chan": a chunk's own moments by two passes, then
    one Chan merge; "device": as k_ret_stats — ROW_LANES Welford partials folded in lane order,
    then merged.  Never E[x^2] - mean^2."""

    def __init__(self, gamma, form="device", capacity=None):
        self.gamma = float(gamma)
        self.form = form
        self.capacity = capacity
        self.count = self.mean = self.m2 = self.ret = 0.0

    def state(self):
        return self.count, self.mean, self.m2, self.ret

    def _merge(self, n, mean, m2):
        if n == 0:
            return
        if self.count == 0:
            self.count, self.mean, self.m2 = float(n), float(mean), float(m2)
            return
        tot = self.count + n
        d = mean - self.mean
        self.mean = self.mean + d * (n / tot)
        self.m2 = self.m2 + m2 + d * d * (self.count * n / tot)
        self.count = tot

    def returns(self, r, d, end):
        """The chunk's ret_i (float64), advancing self.ret."""
        out = np.empty(len(r), np.float64)
        ret = self.ret
        for i in range(len(r)):
            ret = float(np.float64(ret) * np.float64(self.gamma)) + float(r[i])
            out[i] = ret
            if d[i] or end[i]:
                ret = 0.0
        self.ret = ret
        return out

    def push(self, r, d, end=None):
        r = np.asarray(r, np.float32).reshape(-1)
        d = np.asarray(d).astype(bool).reshape(-1)
        end = np.zeros(len(r), bool) if end is None else np.asarray(end).astype(bool).reshape(-1)
        if self.capacity is not None and len(r) > self.capacity:
            # only the stored rows count, and ret restarts before the first of them
            skip = len(r) - self.capacity
            r, d, end = r[skip:], d[skip:], end[skip:]
            self.ret = 0.0
        for i in range(0, len(r), CHUNK):
            with np.errstate(invalid="ignore", over="ignore"):
                x = self.returns(r[i:i + CHUNK], d[i:i + CHUNK], end[i:i + CHUNK])
                if self.form == "serial":
                    for v in x:
                        self._merge(1.0, float(v), 0.0)
                elif self.form == "device":
                    part = ReturnStats(self.gamma)
                    for lane in range(ROW_LANES):
                        part._merge(*_welford([float(v) for v in x[lane::ROW_LANES]]))
                    self._merge(part.count, part.mean, part.m2)
                else:
                    mean = float(x.mean())
                    self._merge(float(len(x)), mean, float(((x - mean) ** 2).sum()))
        return self

    def mark_episode_end(self):
        self.ret = 0.0


class NaiveReturnStats(ReturnStats):
    """The form the feature must NOT use: running sums of ret and ret^2 in fp64, M2 = sum x^2 -
    count mean^2.  Kept as the control that misses the bound."""

    def __init__(self, gamma):
        super().__init__(gamma)
        self.sx = self.sxx = 0.0

    def push(self, r, d, end=None):
        r = np.asarray(r, np.float32).reshape(-1)
        end = np.zeros(len(r), bool) if end is None else end
        x = self.returns(r, np.asarray(d).astype(bool), np.asarray(end).astype(bool))
        self.count += len(x)
        self.sx += float(x.sum())
        self.sxx += float((x * x).sum())
        self.mean = self.sx / self.count
        self.m2 = self.sxx - self.count * self.mean ** 2
        return self


def factor(count, m2, scale=1.0, eps=1e-8, mode=1):
    """k float32: fp64 arithmetic, rounded once; mode 3 or count == 0: the scale alone."""
    if mode == 3 or count == 0:
        return np.float32(scale)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(np.float64(scale) / np.sqrt(np.float64(m2) / np.float64(count) + np.float64(eps)))


def normalize(r, k, clip):
    """fp32: t = r * k (one rounding), then compares (a NaN stays a NaN; no fmin / fmax)."""
    r = np.asarray(r, np.float32)
    c = np.float32(clip)
    with np.errstate(invalid="ignore", over="ignore"):
        t = r * np.float32(k)
        return np.where(t < -c, -c, np.where(t > c, c, t)).astype(np.float32)


def exact_returns(r, d, end, gamma, ret0=Fraction(0)):
    """The ret_i as Fractions: the recurrence itself in exact arithmetic, from the float32
    rewards and the double gamma."""
    g = Fraction(float(gamma))
    ret, out = Fraction(ret0), []
    for i in range(len(r)):
        ret = ret * g + Fraction(float(r[i]))
        out.append(ret)
        if d[i] or end[i]:
            ret = Fraction(0)
    return out, ret


def exact_moments(xs):
    n = len(xs)
    mean = sum(xs) / n
    return n, mean, sum(v * v for v in xs) - n * mean * mean


def exact_factor(n, m2, scale=1.0, eps=1e-8):
    """The factor from the exact moments: the square root in fp64 of the exact quotient rounded
    once (within 1 fp64 ulp of exact: far inside half an fp32 ulp)."""
    return np.float32(np.float64(scale) / np.sqrt(np.float64(float(m2 / n + Fraction(float(eps))))))


GAMMA = 0.99
N_ROWS = 5000
CUTS = (0, 1, 18, 1043, 5000)          # pushes of 1 + 17 + 1025 + 3957 rows
STRETCH = (2000, 2400)                 # rewards at 4096 +- 0.01


@functools.lru_cache(maxsize=None)
def fixture(n=N_ROWS, seed=24, max_len=300):
    """(r float32, done bool, end bool): rewards 1 + 0.5 N(0,1) with a stretch at 4096 +- 0.01,
    random episode lengths in [1, max_len), 60 % of the ends terminals and the rest flag-only."""
    rng = np.random.default_rng(seed)
    r = (1.0 + 0.5 * rng.standard_normal(n)).astype(np.float32)
    lo, hi = STRETCH
    stretch = (4096.0 + 0.01 * rng.standard_normal(hi - lo)).astype(np.float32)
    r[lo:hi] = stretch[:len(r[lo:hi])]            # (a short fixture has none)
    done, end = np.zeros(n, bool), np.zeros(n, bool)
    pos = 0
    while True:
        pos += int(rng.integers(1, max_len))
        if pos > n:
            break
        (done if rng.random() < 0.6 else end)[pos - 1] = True
    for a in (r, done, end):
        a.setflags(write=False)
    return r, done, end


@functools.lru_cache(maxsize=None)
def fixture_exact(n=N_ROWS, seed=24, first=0):
    """(exact ret list, (count, mean, M2)) of fixture rows [first, n)."""
    r, d, e = fixture(n, seed)
    xs, _ = exact_returns(r[first:], d[first:], e[first:], GAMMA)
    return xs, exact_moments(xs)


def ulp32(got, want):
    """|got - want| in fp32 ulps of want."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    sp = np.spacing(np.maximum(np.abs(want), np.float32(1e-38)))
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / sp.astype(np.float64)


def state_errors(count, mean, m2, exact):
    """(relative M2 error, mean error / max|ret|) against exact arithmetic."""
    xs, (n, emean, em2) = exact
    assert count == n, (count, n)
    amax = float(max(abs(v) for v in xs))
    e_m2 = abs(float(Fraction(float(m2)) - em2)) / float(em2)
    e_mean = abs(float(Fraction(float(mean)) - emean)) / amax
    return e_m2, e_mean
