"""CPU checks of the prioritized sampler's cdf model and its boundary probes
(tests/per_cdf_model.py) — what tests/test_gpu_per_cdf.py holds the device to.

* numpy's own ``sum`` is the reduction oracle/per.py restates (and per.hip implements), on
  inputs on which a plain float64 sum gives another float32: the inputs are order-sensitive.
* The probes see a normaliser that is one float32 ulp off: at least a quarter of them change
  their answer (about half do; random uniforms essentially never do).
* Zero-probability rows make ties in the cdf; the probes return numpy's skipped-over indices.
"""
import numpy as np
import pytest

from oracle import per as P
from per_cdf_model import (SUM_CASES, SUM_MUTANTS, WIDE_SEED, default_prio, model, mutant_sum,
                           positions_for, pow2_prio, probes, takes_fallback, top_stride, weights64,
                           wide_prio)

SUM_FILLS = [1, 7, 8, 9, 127, 128, 129, 136, 255, 8191, 8192, 8193, 8199, 8200, 16385, 24705]


@pytest.mark.parametrize("n", SUM_FILLS)
def test_numpy_sum_is_the_restated_pairwise_sum(n):
    a = wide_prio(n, WIDE_SEED + n)
    assert n < 100 or np.log2(a.max() / a.min()) > 20
    assert a.sum() == P.pairwise_sum_f32(a)
    assert a.sum().dtype == np.float32


def test_sum_inputs_are_order_sensitive():
    """A kernel that summed in another order would not get these totals: a sequential float32
    sum differs from numpy's tree at every fill that has a tree (>= 127 here), and a float64 sum
    rounded once differs at several fills on both sides of the 8192-row chunk."""
    def seq(a):
        s = np.float32(0)
        for v in a:
            s = np.float32(s + v)
        return s
    data = {n: wide_prio(n, WIDE_SEED + n) for n in SUM_FILLS}
    assert all(seq(a) != a.sum() for n, a in data.items() if n >= 127)
    differ = [n for n, a in data.items() if np.float32(a.astype(np.float64).sum()) != a.sum()]
    assert len(differ) >= 4, differ
    assert any(n >= 8192 for n in differ) and any(n < 8192 for n in differ), differ


def test_model_is_the_oracles_and_alpha_one_is_exact():
    prio = default_prio(5000, 1)
    p, cdf = model(prio, 4000, 0.6)
    assert np.array_equal(p, P.probs_from(prio.copy(), 4000, 0.6))
    assert cdf[-1] == 1.0 and np.all(np.diff(cdf) > 0)
    p1, _ = model(prio, 4000, 1.0)
    assert np.array_equal(p1, prio[:4000] / prio[:4000].sum())     # x ** 1 is x
    assert not takes_fallback(p1)
    assert takes_fallback(np.array([1e-10, 1.0], np.float32)) and not takes_fallback(np.array([0, 1.0], np.float32))


@pytest.mark.parametrize("n", [1, 2, 5, 129, 8195, 300_001, 2_097_153 + 4999])
def test_positions(n):
    pos = positions_for(n)
    assert pos.dtype == np.int64 and np.all(np.diff(pos) > 0)
    assert pos[0] == 0 and pos[-1] == n - 1 and pos.size <= 8100
    s = set(pos.tolist())
    stride = top_stride(n)
    assert stride == (2048 if n > 2_097_152 else 1024)
    for m in (8, 128, 1024, 4096, 8192, stride):
        last = (n // m) * m                      # the last multiple: the ragged tail starts here
        for q in (0, 1, last - 1, last, last + 1):   # (thinned in between when there are many)
            assert q in s or not 0 <= q < n, (m, q)
    if n <= 2000:
        assert pos.size == n
    assert np.array_equal(pos, positions_for(n))                    # fixed seed


def test_probes_see_a_one_ulp_normaliser():
    """20 000 rows, the float32 total nudged by one ulp: the boundary probes change their answer
    at >= 25 % (about half); 16 000 random uniforms change essentially never."""
    n = 20000
    prio = default_prio(n, 7)
    p, cdf = model(prio, n, 1.0)
    u, want = probes(cdf, positions_for(n))
    assert u.size > 4000 and np.all((want >= 0) & (want < n))
    x = prio[:n].copy()
    for direction in (np.float32(np.inf), np.float32(0)):
        q = x / np.nextafter(x.sum(), direction)
        cdf2 = q.astype(np.float64).cumsum()
        cdf2 /= cdf2[-1]
        assert np.mean(cdf2 != cdf) > 0.9
        changed = np.mean(cdf2.searchsorted(u, side="right") != want)
        assert changed >= 0.25, changed
        ur = np.random.default_rng(3).random(16000)
        assert np.mean(cdf2.searchsorted(ur, side="right") != cdf.searchsorted(ur, side="right")) < 1e-3


def test_probes_one_wrong_leaf_is_seen():
    """The same for a total that is wrong the way a kernel gets it wrong: a plain sequential
    float32 sum instead of the pairwise tree."""
    n = 8199
    prio = wide_prio(n, WIDE_SEED + n)
    p, cdf = model(prio, n, 1.0)
    seq = np.float32(0)
    for v in prio:
        seq = np.float32(seq + v)
    assert seq != prio.sum()
    q = prio / seq
    cdf2 = q.astype(np.float64).cumsum()
    cdf2 /= cdf2[-1]
    u, want = probes(cdf, positions_for(n))
    assert np.mean(cdf2.searchsorted(u, side="right") != want) >= 0.25


def test_probes_over_zero_probability_runs():
    """Leading, interior and trailing zero-probability rows: equal cdf entries.  'right' steps
    over a whole run of ties, so no probe answers an index inside a run, a probe on the run's
    value answers the first index after it, and u = 0 answers the first nonzero row."""
    n = 20000
    prio = default_prio(n, 9)
    prio[:5] = 0
    prio[100:140] = 0
    prio[-9:] = 0
    p, cdf = model(prio, n, 1.0)
    assert not takes_fallback(p)
    assert np.all(cdf[:5] == 0) and np.all(cdf[100:140] == cdf[99]) and np.all(cdf[-10:] == 1.0)
    u, want = probes(cdf, np.arange(n))
    assert u.min() == 0.0 and u.max() < 1.0
    zero = np.zeros(n, bool)
    zero[:5] = zero[100:140] = zero[-9:] = True
    assert not zero[want].any()
    assert want.min() == 5 and want.max() == n - 10
    # on the tie's value: past the run; just below it: the row that owns the boundary
    assert np.all(cdf.searchsorted(cdf[100:140], "right") == 140)
    assert np.all(cdf.searchsorted(np.nextafter(cdf[100:140], 0), "right") == 99)
    assert cdf.searchsorted(0.0, "right") == 5
    assert cdf.searchsorted(np.nextafter(1.0, 0.0), "right") == n - 10
    # every nonzero row is some probe's answer except none is lost: rows 5 .. n-10
    assert np.array_equal(np.unique(want), np.flatnonzero(~zero))


def test_weights_model():
    prio = default_prio(3000, 4)
    p, _ = model(prio, 3000, 1.0)
    idx = np.array([0, 17, 2999, 17])
    w = weights64(p, 3000, idx, 0.4)
    assert w.max() == 1.0 and w[1] == w[3] and np.all((w > 0) & (w <= 1))
    ref = (3000 * p[idx]) ** (-0.4)                                 # the reference's float32 line
    ref /= ref.max()
    assert ref.dtype == np.float32
    assert np.all(np.abs(w - ref) <= 4 * np.spacing(ref))


def test_power_of_two_inputs_are_order_sensitive_too():
    """The GPU tests at alpha = 1 use priorities 2^k (exact under the device's powf).  Over 24
    binades a sequential float32 sum still differs from numpy's tree from 129 rows on; over 17
    binades (every probability >= 2^-29 up to 24 705 rows: the exact fixed-point path) from
    4095 rows on."""
    def seq(a):
        s = np.float32(0)
        for v in a:
            s = np.float32(s + v)
        return s
    for n in SUM_FILLS + [257, 1023, 1024, 1025, 4095, 4096, 4097, 8195, 16384, 2 * 8192 + 129]:
        a = pow2_prio(n, 300 + n, -23, 0)
        assert a.sum() == P.pairwise_sum_f32(a)
        assert n < 129 or seq(a) != a.sum(), n
        assert takes_fallback(model(a, n, 1.0)[0]) == (n >= 1023), n
        b = pow2_prio(n, 300 + n, -16, 0)
        assert b.sum() == P.pairwise_sum_f32(b)
        assert n < 4095 or seq(b) != b.sum(), n
        assert not takes_fallback(model(b, n, 1.0)[0]), n


@pytest.mark.parametrize("n", sorted(SUM_CASES))
def test_sum_order_cases_expose_the_emulated_mutants(n):
    """The inputs of the GPU sum-order cases: numpy's sum is the restated tree on them, and each
    wrong sum listed for the fill gives another total on at least one of them — which moves
    ~100 % of the cdf, as test_probes_see_a_one_ulp_normaliser shows."""
    seeds, exposed = SUM_CASES[n]
    data = [pow2_prio(n, s, -33, 15) for s in seeds]
    for a in data:
        assert a.sum() == mutant_sum(a) == P.pairwise_sum_f32(a)
    for m in exposed:
        assert m in SUM_MUTANTS and any(mutant_sum(a, m) != a.sum() for a in data), m
    assert "A" in exposed and (n < 127 or "F" in exposed)
    if n >= 2 * 8192 + 1:
        assert "D" in exposed
