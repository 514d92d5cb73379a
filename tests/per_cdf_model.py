"""Host model of the prioritized sampler's cdf, and the boundary probes that pin it.

TEST INFRASTRUCTURE ONLY.  ``csrc/per.hip`` claims ``np.random.choice(p=probs)`` bit for bit:
numpy's float32 pairwise sum, an exact int64 fixed-point prefix and a two-level search.  A
random uniform does not see a wrong sum: a normaliser one float32 ulp off moves every float64
cdf entry, but by so little that a random draw almost never lands between the old and the new
boundary.  A uniform placed ON a boundary does: ``searchsorted(cdf, u, 'right')`` steps over
index ``i`` exactly when ``u >= cdf[i]``, so ``u = cdf[i]`` and ``u = nextafter(cdf[i], 0)``
answer differently as soon as ``cdf[i]`` moves by one float64 ulp.

* ``model(prio, n, alpha)``   (probs, cdf) as replay_buffer.py:58-67 and numpy's ``choice`` make
  them, with numpy's own ``sum`` and ``cumsum``;
* ``probes(cdf, positions)``  (u, want): the two uniforms per position and numpy's own answer;
* ``positions_for(n)``        where the kernels change path: around the multiples of the leaf's
  8 accumulators, the 128-row leaf, the 1024-row scan block, F2's 4096-row wave, the 8192-row
  chunk and the top table's stride, the four ends, and a fixed random set.
"""
from __future__ import annotations

import numpy as np

P_EXACT_MIN = np.float32(2.0 ** -29)   # below this (and nonzero) the sampler takes its
                                       # sequential float64 cumsum (per.hip's "bad" flag)
TOP_MAX = 2048                         # per.hip kTopMax
PER_KIND = 1000                        # positions kept per kind of multiple
N_RANDOM = 2000
WIDE_SEED = 200                        # wide_prio(n, WIDE_SEED + n): the order-sensitive inputs


def model(prio: np.ndarray, n: int, alpha: float):
    """replay_buffer.py:58-64 and RandomState.choice's cdf."""
    prio = np.asarray(prio, np.float32)
    p = prio[:n] ** np.float32(alpha)
    assert p.dtype == np.float32
    p /= p.sum()
    cdf = p.astype(np.float64).cumsum()
    cdf /= cdf[-1]
    return p, cdf


def takes_fallback(p: np.ndarray) -> bool:
    """A nonzero probability below 2^-29 (or one that is no number) leaves the exact fixed-point
    path: k_per_f2's ``p != 0 && !(p >= 2^-29)``."""
    return bool(np.any((p != 0) & ~(p >= P_EXACT_MIN)))


def top_stride(n: int) -> int:
    """The search's top table keeps every stride-th cdf entry, at most TOP_MAX of them."""
    s = 1024
    while (n + s - 1) // s > TOP_MAX:
        s *= 2
    return s


def _around_multiples(n: int, m: int, cap: int) -> np.ndarray:
    """k*m - 1, k*m, k*m + 1 for the multiples k*m in [0, n], clipped to [0, n); when that is
    more than ``cap`` positions, the multiples are thinned evenly (first and last kept)."""
    k = np.arange(0, n // m + 1, dtype=np.int64)
    keep = max(2, cap // 3)
    if k.size > keep:
        k = k[np.unique(np.linspace(0, k.size - 1, keep).round().astype(np.int64))]
    pos = (k[:, None] * m + np.array([-1, 0, 1], np.int64)[None, :]).ravel()
    return pos[(pos >= 0) & (pos < n)]


def positions_for(n: int, seed: int = 20240) -> np.ndarray:
    """Sorted unique probe positions for a fill of n rows (about 8000 at most)."""
    kinds = [8, 128, 1024, 4096, 8192, top_stride(n)]
    parts = [_around_multiples(n, m, PER_KIND) for m in dict.fromkeys(kinds)]
    parts.append(np.array([0, 1, n - 2, n - 1], np.int64))
    rng = np.random.default_rng(seed)
    parts.append(rng.integers(0, n, N_RANDOM) if n > N_RANDOM else np.arange(n, dtype=np.int64))
    pos = np.unique(np.concatenate(parts))
    return pos[(pos >= 0) & (pos < n)]


def probes(cdf: np.ndarray, positions):
    """(u, want).  Per position i: u = cdf[i] when that is < 1, and u = nextafter(cdf[i], 0);
    want = cdf.searchsorted(u, 'right').  Every u is in [0, 1)."""
    c = np.asarray(cdf, np.float64)[np.asarray(positions, np.int64)]
    u = np.concatenate([c[c < 1.0], np.nextafter(c, 0.0)])
    assert u.dtype == np.float64 and np.all((u >= 0.0) & (u < 1.0))
    want = np.asarray(cdf).searchsorted(u, side="right").astype(np.int64)
    return u, want


def weights64(p: np.ndarray, n: int, idx, beta: float) -> np.ndarray:
    """The importance weights in float64, from the float32 probabilities and the float32
    exponent the reference's ``(n * probs[idx]) ** (-beta)`` works with (replay_buffer.py:69-71):
    w = (n p)^-beta / max."""
    b = np.float64(np.float32(beta))
    w = (np.float64(n) * p[np.asarray(idx, np.int64)].astype(np.float64)) ** (-b)
    return w / w.max()


def default_prio(n: int, seed: int) -> np.ndarray:
    """uniform(0.5, 1) * 2^[-3, 3]: seven binades, so the float32 sum depends on its order and
    every probability stays >= 2^-29 up to 2^22 rows (the exact fixed-point path)."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 1.0, n) * 2.0 ** rng.integers(-3, 4, n)).astype(np.float32)


def wide_prio(n: int, seed: int) -> np.ndarray:
    """Exponents over 24 binades: nearly every addition of the float32 sum rounds."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 1.0, n) * 2.0 ** rng.integers(-23, 1, n)).astype(np.float32)


def pow2_prio(n: int, seed: int, lo: int, hi: int) -> np.ndarray:
    """Priorities 2^k, k uniform in [lo, hi] within [-33, 15].  The device's powf is not exact at
    y = 1 (4.9 % of random x come back one ulp off, measured), but for every
    power of two in that range it returned 2^k itself, so the host model of an alpha = 1 context
    stays exact.  Sums of powers of two over many binades still round, so they still depend on
    their order."""
    assert -33 <= lo <= hi <= 15
    rng = np.random.default_rng(seed)
    return (2.0 ** rng.integers(lo, hi + 1, n)).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# Emulated wrong sums: what the inputs of the sum-order cases are chosen against.
SUM_MUTANTS = {
    "A": "a leaf's 8 accumulators combined left to right instead of pairwise",
    "B": "the ragged tree split at n / 2 without rounding down to a multiple of 8",
    "C": "a leaf's tail (n % 8 rows) added into the accumulators instead of after their combine",
    "D": "the chunk sums combined pairwise from the right instead of in chunk order",
    "F": "leaves of 64 rows instead of 128",
}


def mutant_sum(a: np.ndarray, mutant: str = "") -> np.float32:
    """numpy's float32 ``sum`` of a contiguous array ("" — oracle.per.pairwise_sum_f32's
    arithmetic, eight lanes at a time), or one of SUM_MUTANTS."""
    f = np.float32
    leaf_max = 64 if mutant == "F" else 128

    def tree(x):
        n = x.shape[0]
        if n < 8:
            res = f(0.0)
            for v in x:
                res = f(res + v)
            return res
        if n <= leaf_max:
            body = n - n % 8
            r = x[:body].reshape(-1, 8).copy()
            acc = r[0]
            for row in r[1:]:
                acc = acc + row                       # float32, lane by lane
            tail = x[body:]
            if mutant == "C":
                acc = acc.copy()
                acc[:tail.size] = acc[:tail.size] + tail
                tail = tail[:0]
            if mutant == "A":
                res = acc[0]
                for v in acc[1:]:
                    res = f(res + v)
            else:
                res = f(f(f(acc[0] + acc[1]) + f(acc[2] + acc[3])) + f(f(acc[4] + acc[5]) + f(acc[6] + acc[7])))
            for v in tail:
                res = f(res + v)
            return res
        n2 = n // 2
        if mutant != "B":
            n2 -= n2 % 8
        return f(tree(x[:n2]) + tree(x[n2:]))

    a = np.ascontiguousarray(a, np.float32)
    sums = [tree(a[c:c + 8192]) for c in range(0, a.shape[0], 8192)]
    if mutant == "D" and len(sums) > 1:
        acc = sums[-1]
        for s in sums[-2::-1]:
            acc = f(s + acc)
        return acc
    acc = f(-0.0)
    for s in sums:
        acc = f(acc + s)
    return acc


# fill -> (seeds of pow2_prio(n, seed, -33, 15), the SUM_MUTANTS those inputs expose between
# them).  Found by searching seeds 0..399 against the emulated mutants above; a mutant missing
# from a fill's string either does not apply there (B at a fill whose halves are multiples of 8,
# D below three chunks) or was exposed by none of the 400.  tests/test_per_cdf_model.py asserts
# the table.  Every one of these is a fallback case (49 binades of priorities).
SUM_CASES = {
    9: ((6, 81), "AC"), 127: ((2, 4), "ACF"), 128: ((3, 4), "AF"), 129: ((1, 7, 111), "ACF"),
    136: ((2, 3), "ABF"), 255: ((0, 2, 5), "ABCF"), 257: ((4, 144), "ACF"),
    1023: ((3, 4, 69), "ABCF"), 1024: ((3, 4), "AF"), 1025: ((3, 4), "AF"),
    4095: ((4, 8, 44), "ABCF"), 4096: ((2, 22), "AF"), 4097: ((2, 22, 312), "ACF"),
    8191: ((4, 6), "ABF"), 8192: ((3, 17), "AF"), 8193: ((3, 17), "AF"), 8195: ((3, 17), "AF"),
    8199: ((3, 17), "AF"), 8200: ((3, 17), "AF"), 16384: ((1,), "AF"), 16385: ((1, 46), "ADF"),
    16513: ((1,), "ADF"), 24705: ((0, 3, 10), "ADF"),
}
