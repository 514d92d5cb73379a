"""CPU checks of the reward-normalisation contract (include/sacmi.h): the six
functions are declared, exported and bridged; and the host model (tests/reward_norm_model.py) of
the fp64 return recurrence, the chunked running moments, the fp32 factor and the fp32 normalise
expression agrees with exact rational arithmetic on a fixture of 5000 rows with random episode
lengths, terminals and flag-only ends, and a stretch of rewards at 4096 +- 0.01.

Bounds, the project's own for running moments (tests/test_obs_norm_model.py): M2 within 1e-9
relative, the mean within 1e-12 of max|ret|, the factor within 1 ulp; the fp64 recurrence itself
within 1e-12 of max|ret| as well.  The E[x^2] - mean^2 form in fp64 is kept as the control that
must miss the M2 bound: on the fixture's stretch pushed as one-row episodes (returns at 4096 with
a spread of 0.01 — on the whole fixture the returns' own spread is as large as their mean, and no
form cancels)."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from reward_norm_model import (CUTS, GAMMA, STRETCH, NaiveReturnStats, ReturnStats, exact_factor,
                               exact_moments, exact_returns, factor, fixture, fixture_exact,
                               normalize, state_errors, ulp32)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sacmi.h")
LIB = os.path.join(ROOT, "humanoid-walking-with-sac_amd", "sacmi", "libsacmi.so")
FUNCS = ("sacmi_set_reward_norm", "sacmi_reward_norm", "sacmi_reward_norm_get_state",
         "sacmi_reward_norm_set_state", "sacmi_reward_norm_get_factor", "sacmi_read_batch_rn")
M2_RTOL, MEAN_RTOL, EPS = 1e-9, 1e-12, 1e-8
ONE_ROW = tuple(range(21)) + (5000,)      # twenty one-row pushes, then the rest


def test_abi_declares_exports_and_bridges_the_six_functions():
    text = open(HEADER).read()
    declared = set(re.findall(r"^\s*int\s+(sacmi_\w+)\s*\(", text, re.M))
    assert not [f for f in FUNCS if f not in declared]
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (sacmi_\w+)", out))
    assert not [f for f in FUNCS if f not in exported]
    from sacmi import _lib as L
    assert not [f for f in FUNCS if f not in L.EXPORTS]


def run_model(form, cuts):
    r, d, e = fixture()
    m = ReturnStats(GAMMA, form)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        m.push(r[lo:hi], d[lo:hi], e[lo:hi])
    return m


@pytest.mark.parametrize("cuts", [CUTS, ONE_ROW], ids=["1_17_1025_3957", "twenty_one_row"])
@pytest.mark.parametrize("form", ["serial", "chan", "device"])
def test_state_matches_exact_arithmetic(form, cuts):
    m = run_model(form, cuts)
    exact = fixture_exact()
    e_m2, e_mean = state_errors(m.count, m.mean, m.m2, exact)
    print(f"{form}: M2 {e_m2:.2e} relative, mean {e_mean:.2e} of max|ret|")
    assert e_m2 <= M2_RTOL and e_mean <= MEAN_RTOL
    n, _, em2 = exact[1]
    u = float(ulp32(factor(m.count, m.m2, 1.0, EPS), exact_factor(n, em2, 1.0, EPS)))
    print(f"{form}: factor {u:.1f} ulp")
    assert u <= 1.0
    # the running return behind the last row, against the exact one
    r, d, e = fixture()
    _, ret = exact_returns(r, d, e, GAMMA)
    amax = float(max(abs(v) for v in exact[0]))
    assert abs(float(Fraction(m.ret) - ret)) <= MEAN_RTOL * amax


def test_recurrence_matches_exact_arithmetic():
    r, d, e = fixture()
    got = ReturnStats(GAMMA).returns(r, d, e)
    xs = fixture_exact()[0]
    amax = float(max(abs(v) for v in xs))
    err = max(abs(float(Fraction(float(a)) - b)) for a, b in zip(got, xs)) / amax
    print(f"recurrence: {err:.2e} of max|ret| = {amax:.6g}")
    assert err <= MEAN_RTOL
    # ret restarts behind every terminal and every flag-only end
    for i in np.flatnonzero(d | e)[:-1]:
        assert got[i + 1] == float(r[i + 1])
    assert d.sum() > 5 and e.sum() > 5 and not (d & e).any()


def test_sum_of_squares_form_misses_the_bound():
    """The control: returns at 4096 +- 0.01 (the stretch, one-row episodes); fp64 sums of ret and
    ret^2 lose M2 to cancellation, the model's forms do not."""
    r = fixture()[0][STRETCH[0]:STRETCH[1]]
    d = np.ones(len(r), bool)
    xs, _ = exact_returns(r, d, ~d, GAMMA)
    exact = (xs, exact_moments(xs))
    naive = NaiveReturnStats(GAMMA).push(r, d)
    rel = abs(naive.m2 - float(exact[1][2])) / float(exact[1][2])
    print(f"naive: M2 off by {rel:.2e} relative")
    assert rel > 1e3 * M2_RTOL
    for form in ("serial", "chan", "device"):
        m = ReturnStats(GAMMA, form)
        for lo in range(0, len(r), 17):
            m.push(r[lo:lo + 17], d[lo:lo + 17])
        e_m2, e_mean = state_errors(m.count, m.mean, m.m2, exact)
        print(f"{form}: M2 {e_m2:.2e} relative, mean {e_mean:.2e}")
        assert e_m2 <= M2_RTOL and e_mean <= MEAN_RTOL


def test_count_zero_and_mode_3_are_the_scale_alone():
    m = ReturnStats(GAMMA)
    assert factor(m.count, m.m2, 1.0, EPS) == np.float32(1.0)
    assert factor(m.count, m.m2, 0.3, EPS) == np.float32(0.3)
    x = np.array([1.5, -2.0, 0.0, 3e30, -7.25], np.float32)
    assert np.array_equal(normalize(x, factor(0.0, 0.0), np.inf), x)            # the identity
    m.push(*[a[:100] for a in fixture()])
    assert factor(m.count, m.m2, 0.25, EPS, mode=3) == np.float32(0.25)
    assert factor(m.count, m.m2, 0.25, EPS, mode=1) != np.float32(0.25)
    assert np.array_equal(normalize(x, np.float32(0.25), np.inf), x * np.float32(0.25))
    m.push(np.zeros(0, np.float32), np.zeros(0, bool))      # an empty push changes nothing
    assert m.count == 100


def test_normalize_expression_clip_nan_inf():
    r = np.array([3.0, np.nan, 100.0, 0.5, -9.0, np.inf, -np.inf, 0.0], np.float32)
    y = normalize(r, 2.0, 1.5)
    want = np.array([1.5, np.nan, 1.5, 1.0, -1.5, 1.5, -1.5, 0.0], np.float32)
    assert np.array_equal(y, want, equal_nan=True)
    assert np.isnan(y[1])                                   # a NaN is not clamped away
    y = normalize(r, 2.0, np.inf)                           # clip = inf: none
    want = np.array([6.0, np.nan, 200.0, 1.0, -18.0, np.inf, -np.inf, 0.0], np.float32)
    assert np.array_equal(y, want, equal_nan=True)
    # one fp32 rounding: the product
    a, k = np.float32(1.0000001), np.float32(3.0000002)
    assert normalize(a, k, np.inf) == np.float32(a * k)


def test_nan_and_inf_rewards_poison_the_state():
    for bad in (np.nan, np.inf, -np.inf):
        r, d, e = (a[:40].copy() for a in fixture())
        d[:] = False
        e[:] = False
        r[7] = bad
        m = ReturnStats(GAMMA).push(r, d, e)
        assert m.count == 40 and not np.isfinite(m.m2) and not np.isfinite(m.ret)
        assert np.isnan(factor(m.count, m.m2, 1.0, EPS)) or factor(m.count, m.m2, 1.0, EPS) == 0.0
        # the row's own normalised reward keeps its kind under any finite factor
        y = normalize(np.float32(bad), 0.5, 10.0)
        assert np.isnan(y) if np.isnan(bad) else y == np.float32(np.sign(bad) * 10.0)


def test_ret_restarts_at_done_at_a_flag_and_at_mark_episode_end():
    g = GAMMA
    m = ReturnStats(g, "serial")
    m.push([1.0, 2.0], [False, False])
    assert m.ret == 1.0 * g + 2.0
    m.push([3.0], [True])                                   # a terminal
    assert m.ret == 0.0
    m.push([4.0, 5.0], [False, False], [False, True])       # a flag-only end
    assert m.ret == 0.0
    m.push([6.0], [False])
    assert m.ret == 6.0
    m.mark_episode_end()                                    # learnt of after the push
    assert m.ret == 0.0 and m.count == 6
    m.push([7.0], [False])
    assert m.ret == 7.0
    xs, _ = exact_returns([1, 2, 3, 4, 5, 6, 7], [0, 0, 1, 0, 0, 0, 0], [0, 0, 0, 0, 1, 1, 0], g)
    n, mean, m2 = exact_moments(xs)
    assert m.count == n and abs(m.mean - float(mean)) < 1e-14 and abs(m.m2 - float(m2)) < 1e-12


def test_a_push_of_more_than_capacity_counts_the_stored_rows_only():
    r, d, e = fixture()
    cap = 64
    m = ReturnStats(GAMMA, "device", capacity=cap).push(r[:10], d[:10], e[:10])
    before = m.state()
    m.push(r[10:10 + cap + 5], d[10:10 + cap + 5], e[10:10 + cap + 5])
    want = ReturnStats(GAMMA, "device")
    want.count, want.mean, want.m2, want.ret = before[0], before[1], before[2], 0.0
    want.push(r[15:15 + cap], d[15:15 + cap], e[15:15 + cap])
    assert m.state() == want.state() and m.count == 10 + cap


def test_recorded_resource_reports_leave_every_existing_kernel_as_it_was():
    """profiles/reward_norm/: tools/resources.py on every .hip file of the parent commit and of
    this one.  Every kernel of the parent has the same line (registers, spills, LDS) — k_obs_stats
    among them, whose moment helpers moved into a shared header — and the new kernels are the
    two of csrc/retnorm.hip, without spills."""
    d = os.path.join(ROOT, "profiles", "reward_norm")
    parent = [l for l in open(os.path.join(d, "resources_parent.txt")).read().splitlines()
              if l and not l.startswith("==")]
    this = [l for l in open(os.path.join(d, "resources_this.txt")).read().splitlines()
            if l and not l.startswith("==")]
    assert len(parent) > 200 and any("k_obs_stats" in l for l in parent)
    assert [l for l in this if l in set(parent)] == parent
    new = [l for l in this if l not in set(parent)]
    assert len(new) == 2 and "k_ret_stats" in new[0] and "k_reward_norm" in new[1], new
    assert all("spill   0" in l for l in new)
