"""CPU checks of the n-step gather's host model (tests/nstep_model.py; sacmi_set_nstep in
include/sacmi.h) — the model the GPU tests hold the device to bit for bit.

Bounds (u = 2^-24, the fp32 unit roundoff; r_j are fp32 inputs, exact):

* Return.  R = r_0 + sum_{j=1..m} fl(g_j r_j), summed left to right.  g_j = gamma^j (1 + d1),
  the product adds (1 + d2), and a term passes through at most m additions, each (1 + d): a term
  carries at most m + 2 factors (1 + d), |d| <= u, so
      |R - R64| <= ((1 + u)^(m+2) - 1) sum |g_j r_j| <= 1.001 (m + 2) u sum |g_j r_j|.
  With m <= n - 1 and n >= 2 that is below 2 n u sum = n 2^-23 sum |g_j r_j|, the asserted bound
  (n = 1: m = 0 and R = r_0 exactly).  The fp64 reference's own error is ~1e-16 relative.
* Coefficient.  c = fl(fl(1 - d') * gf), d' = fl(1 - g), g = g[m] = gamma^m (1 + d1) in (0, 1],
  gf = gamma (1 + d3).  d' = 1 - g + e with |e| <= 2^-25 (half the spacing of [0.5, 1)), and e = 0
  when g >= 0.5 (Sterbenz).  1 - d' is exact either way (d' >= 0.5: Sterbenz; d' < 0.5: it is g
  again), so fl(1 - d') = g - e.  Absolute errors against gamma^(m+1), every value below 1:
  gamma^(m+1) |d1| <= u, gamma |e| <= u / 2, gamma^(m+1) |d3| <= u, the product's rounding <= u:
  3.5 u <= 4 * 2^-24, the asserted bound.  For g >= 0.5, e = 0 and c = fl(g * gf) exactly.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from nstep_model import (CATEGORIES, NMAX, Ring, brute_force, categories, coefficient, collapsed_rows,
                         fixture_marks, g_table, nstep_rows)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "humanoid-walking-with-sac_amd", "sacmi", "libsacmi.so")
NEW = ("sacmi_set_nstep", "sacmi_nstep", "sacmi_push_ep", "sacmi_push_packed_ep", "sacmi_mark_episode_end",
       "sacmi_get_episode_ends", "sacmi_read_batch_rd", "sacmi_debug_set_done")
U = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_ring(capacity, pushed, seed, p_done=0.1, p_end=0.1, scale=1.0):
    rng = np.random.default_rng(seed)
    r = (rng.standard_normal(pushed) * scale).astype(np.float32)
    d = rng.random(pushed) < p_done
    e = rng.random(pushed) < p_end
    return Ring(capacity).push(r, d, e)


def check_against_brute_force(ring, n, gamma):
    idx = np.arange(ring.length)
    m, R, d, sl = ring.rows(n, gamma, idx)
    c = coefficient(d, gamma)
    g = g_table(gamma)
    worst_r = worst_c = 0.0
    for i in idx:
        m64, R64, A, c64 = brute_force(ring.rew, ring.done, ring.ep_end, ring.head, ring.length,
                                       ring.capacity, n, gamma, int(i))
        assert m[i] == m64, (i, m[i], m64)
        assert sl[i] == (ring.head + i + m64) % ring.capacity
        err = abs(float(R[i]) - R64)
        assert err <= n * 2.0 ** -23 * A, (i, err, A)
        worst_r = max(worst_r, err / max(A, 1e-300))
        ec = abs(float(c[i]) - c64)
        assert ec <= 4 * U, (i, ec)
        worst_c = max(worst_c, ec)
        if d[i] != 1 and g[m[i]] >= 0.5:
            assert bits(c[i]) == bits(np.float32(g[m[i]] * np.float32(gamma))), i
    return worst_r, worst_c


def test_table():
    g = g_table(0.99)
    assert g.dtype == np.float32 and len(g) == NMAX and g[0] == 1.0
    assert g[1] == np.float32(0.99) and g[31] == np.float32(0.99 ** 31)


@pytest.mark.parametrize("gamma", [0.99, 0.9, 0.5, 0.997])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 32])
def test_return_and_coefficient_against_fp64(n, gamma):
    ring = random_ring(257, 300, 11 * n, scale=3.0)
    wr, wc = check_against_brute_force(ring, n, gamma)
    print(f"n {n} gamma {gamma}: R {wr / U:.2f} u of sum|g r|, coefficient {wc / U:.2f} u")


def test_low_gamma_coefficient_stays_within_bound():
    """g[m] < 0.5 (the rounding of d' is no longer exact): still within 4 * 2^-24."""
    ring = Ring(80).push(np.ones(80, np.float32), np.zeros(80), np.zeros(80))
    for gamma in (0.5, 0.7, 0.9, 0.95):
        m, R, d, sl = ring.rows(32, gamma, np.arange(80))
        assert (g_table(gamma)[m] < 0.5).any()
        check_against_brute_force(ring, 32, gamma)


def test_m0_rows_are_the_raw_rows():
    ring = random_ring(64, 64, 5, p_done=0.3, p_end=0.3)
    idx = np.arange(64)
    m, R, d, sl = ring.rows(5, 0.99, idx)
    z = m == 0
    assert z.any() and not z.all()
    assert np.array_equal(bits(R[z]), bits(ring.rew[idx[z]]))
    assert np.array_equal(bits(d[z]), bits(ring.done[idx[z]]))
    assert np.array_equal(sl[z], idx[z])
    # n = 1: every row
    m1, R1, d1, sl1 = ring.rows(1, 0.99, idx)
    assert not m1.any() and np.array_equal(bits(R1), bits(ring.rew)) and np.array_equal(bits(d1), bits(ring.done))


def test_nan_reward_propagates():
    ring = Ring(8).push([1, np.nan, 1, 1], [0, 0, 0, 0])
    m, R, d, sl = ring.rows(3, 0.99, [0, 1, 2])
    assert np.isnan(R[0]) and np.isnan(R[1]) and R[2] == np.float32(1 + np.float32(np.float32(0.99) * 1))


def test_edge_len_one():
    ring = Ring(8).push([2.5], [0])
    m, R, d, sl = ring.rows(5, 0.99, [0])
    assert (m[0], R[0], d[0], sl[0]) == (0, 2.5, 0.0, 0)


def test_edge_capacity_below_n():
    ring = Ring(4).push(np.arange(1, 8, dtype=np.float32), np.zeros(7))      # holds rows 3..6, head 3
    assert ring.head == 3 and ring.length == 4
    m, R, d, sl = ring.rows(5, 0.5, np.arange(4))
    assert list(m) == [3, 2, 1, 0]                       # stopped by the newest row, never wraps
    assert list(sl) == [2, 2, 2, 2]
    assert R[0] == 4 + 0.5 * 5 + 0.25 * 6 + 0.125 * 7
    check_against_brute_force(ring, 5, 0.5)


def test_edge_full_ring_head_mid_array_chains_wrap():
    ring = Ring(16).push(np.arange(23, dtype=np.float32), np.zeros(23))     # head 7
    assert ring.head == 7
    m, R, d, sl = ring.rows(3, 0.99, np.arange(16))
    wrap = (ring.head + np.arange(16)) % 16 + m >= 16
    assert wrap.any()
    assert list(m[:14]) == [2] * 14 and list(m[14:]) == [1, 0]
    assert sl[8] == 1 and sl[7] == 0                     # slots 15 -> 1, 14 -> 0
    by_slot = ring.rows(3, 0.99, (ring.head + np.arange(16)) % 16, by_slot=True)
    for x, y in zip((m, R, d, sl), by_slot):
        assert np.array_equal(x, y)
    check_against_brute_force(ring, 3, 0.99)


def test_edge_stops():
    #          row: 0  1  2  3  4  5  6  7
    done = np.array([0, 0, 1, 0, 0, 0, 1, 0])
    end = np.array([0, 0, 0, 0, 1, 0, 1, 0])
    ring = Ring(8).push(np.ones(8, np.float32), done, end)
    m, R, d, sl = ring.rows(4, 0.9, np.arange(8))
    g = g_table(0.9)
    assert list(m) == [2, 1, 0, 1, 0, 1, 0, 0]
    # by a terminal: d' = 1; by a flag with done == 0: bootstraps (d' = 1 - g[m], or 0 at m == 0);
    # terminal and flag on the same row: the terminal wins; by the newest row
    assert d[0] == 1 and d[1] == 1 and d[2] == 1
    assert d[3] == np.float32(1 - g[1]) and d[4] == 0
    assert d[5] == 1 and d[6] == 1
    assert d[7] == 0 and sl[7] == 7
    assert coefficient(d[3:4], 0.9)[0] == np.float32(g[1] * np.float32(0.9))


def test_edge_eviction_overwrites_a_flagged_slot():
    ring = Ring(4).push(np.ones(4, np.float32), np.zeros(4), [0, 1, 0, 0])
    assert ring.ep_end[1] == 1
    assert list(ring.rows(3, 0.9, [0])[0]) == [1]
    ring.push(np.ones(2, np.float32), np.zeros(2))       # plain pushes write 0 over slots 0, 1
    assert not ring.ep_end.any()
    assert list(ring.rows(3, 0.9, np.arange(4))[0]) == [2, 2, 1, 0]
    ring.mark_episode_end()
    assert list(np.flatnonzero(ring.ep_end)) == [1]
    assert list(ring.rows(3, 0.9, np.arange(4))[0]) == [2, 2, 1, 0]


def test_fixture_has_every_category():
    for cap, n in ((64, 2), (64, 3), (64, 5), (64, 32), (4200, 5)):
        done, end = fixture_marks(cap + 23)
        ring = Ring(cap)
        rng = np.random.default_rng(1)
        ring.push(rng.standard_normal(cap + 23).astype(np.float32), done, end)
        assert ring.head == 23
        cat = categories(ring, n, 0.99, np.arange(cap))
        assert all(cat[k] > 0 for k in CATEGORIES), (cap, n, cat)
        check_against_brute_force(ring, n, 0.99)


def test_collapsed_rows_gather_to_the_same_batch():
    """The one-step ring the GPU equivalence test feeds context B: gathering row i of it with the
    feature off gives the n-step row i of the raw ring."""
    cap, n = 16, 4
    rng = np.random.default_rng(3)
    N = cap + 7
    s, a, s2 = rng.standard_normal((N, 2)), rng.standard_normal((N, 1)), rng.standard_normal((N, 2))
    done, end = rng.random(N) < 0.15, rng.random(N) < 0.15
    ring = Ring(cap).push(rng.standard_normal(N).astype(np.float32), done, end)
    (cs, ca, cR, cs2, cd), dprime = collapsed_rows(ring, n, 0.99, s, a, s2)
    m, R, d, sl = ring.rows(n, 0.99, np.arange(cap))
    assert np.array_equal(cs, s[7:]) and np.array_equal(ca, a[7:])
    assert np.array_equal(cs2, s2[7 + np.arange(cap) + m])
    b = Ring(cap).push(cR, cd)
    assert np.array_equal(b.done != 0, d != 0)
    b.done[:] = dprime                                    # (debug_set_done: the fractional d')
    # a context that never enabled the feature gathers r and done as stored
    assert np.array_equal(bits(b.rew), bits(R)) and np.array_equal(bits(b.done), bits(d))


def test_exports_carry_the_new_symbols():
    from sacmi import _lib as L
    missing = [f for f in NEW if f not in L.EXPORTS]
    assert not missing, missing
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (sacmi_\w+)", out))
    assert not [f for f in NEW if f not in exported]
