"""Reward scaling and running return normalisation on the GPU (sacmi_set_reward_norm;
csrc/retnorm.hip).

The state is checked against exact rational arithmetic with the CPU bounds of
tests/test_reward_norm_model.py.  Everything downstream is checked by EQUIVALENCE, bit for bit:
context A has the feature on (frozen after the pushes) and holds raw rewards; context B never
enabled it and holds y = clamp(fl(r k), -clip, clip) computed in numpy
(tests/reward_norm_model.py normalize) with A's factor read back.  Same parameters, same indices
and noise (or the same generator key): losses, parameters, targets, Adam moments and the alpha
state must be identical after the updates, because the only difference is WHERE the fp32
expression ran.  The clip is chosen so that some but not all rewards are clipped.
"""
import functools
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle.sac_step import SacConfig, init_params

from nstep_model import collapsed_rows
from reward_norm_model import (GAMMA, ReturnStats, exact_factor, exact_moments, exact_returns, factor,
                               fixture, fixture_exact, normalize, state_errors, ulp32)
import test_gpu_nstep as tn
import test_gpu_obs_norm as ton
from test_gpu_obs_norm import CASES, assert_same, bits, bits64, differs, new_ctx, snapshot
from test_gpu_parity import ctx_state, load_params, make_ctx

pytestmark = pytest.mark.gpu

M2_RTOL, MEAN_RTOL = 1e-9, 1e-12      # the CPU bounds (tests/test_reward_norm_model.py)
EPS, CLIP = 1e-8, 0.2
SMALL = "S11-H96-B40"


@functools.lru_cache(maxsize=None)
def case_rows(name):
    """The case's rows with rewards of a scale nobody chose (3 r + 1, two outliers) and a flag on
    some non-terminal rows; the model's state after pushing them."""
    cfg, _, (s, a, r, s2, d) = ton.case_inputs(name)[:3]
    rng = np.random.default_rng(CASES[name][6] + 3000)
    r = (3.0 * r + 1.0).astype(np.float32)
    r[rng.integers(0, len(r), 2)] = np.float32(40.0)
    end = (rng.random(len(r)) < 0.1) & (np.asarray(d) == 0)
    model = ReturnStats(cfg.gamma, "device").push(r, d, end)
    return (s, a, r, s2, d), end, model


def ctx_a(name, mode=2, clip=CLIP, scale=1.0):
    """Feature on, raw rewards, the rows pushed in mode 1 (counted), then `mode`."""
    rows, end, _ = case_rows(name)
    ctx = new_ctx(name)
    ctx.set_reward_norm(1, scale, EPS, clip)
    ctx.push(*rows, episode_end=end)
    if mode != 1:
        ctx.set_reward_norm(mode, scale, EPS, clip)
    return ctx


def ctx_b(name, k, clip=CLIP):
    """Never enabled; the rewards normalised in numpy with A's factor."""
    s, a, r, s2, d = case_rows(name)[0]
    ctx = new_ctx(name)
    ctx.push(s, a, normalize(r, k, clip), s2, d)
    return ctx


def two_updates(ctx, name):
    return ton.two_updates(ctx, name)


@functools.lru_cache(maxsize=None)
def equivalence(name):
    a = ctx_a(name)
    try:
        k = a.reward_norm_factor()
        st = a.reward_norm_state()
        ra = two_updates(a, name)
    finally:
        a.close()
    b = ctx_b(name, k)
    try:
        rb = two_updates(b, name)
    finally:
        b.close()
    return ra, rb, k, st


@functools.lru_cache(maxsize=None)
def raw_off(name):
    ctx = new_ctx(name)
    try:
        ctx.push(*case_rows(name)[0])
        return two_updates(ctx, name)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# 1. the state against exact arithmetic
def stats_ctx(capacity=8192, mode=1, S=5):
    cfg = SacConfig(S, 3, 32)
    ctx = make_ctx(cfg, max_batch=8, capacity=capacity, seed=5)
    load_params(ctx, init_params(cfg, 77, bias_scale=0.05))
    if mode:
        ctx.set_reward_norm(mode, 1.0, EPS, 10.0)
    return ctx, cfg


def push_rewards(ctx, r, d, end=None, S=5):
    n = len(r)
    z = np.zeros((n, S), np.float32)
    ctx.push(z, np.zeros((n, 3), np.float32), r, z, d, episode_end=end)


def check_state(ctx, exact, ret_exact, what):
    count, mean, m2, ret = ctx.reward_norm_state()
    e_m2, e_mean = state_errors(count, mean, m2, exact)
    amax = float(max(abs(v) for v in exact[0]))
    e_ret = abs(float(Fraction(ret) - ret_exact)) / amax
    print(f"{what}: count {count:.0f}, M2 {e_m2:.2e} relative, mean {e_mean:.2e}, ret {e_ret:.2e} of max|ret|")
    assert e_m2 <= M2_RTOL and e_mean <= MEAN_RTOL and e_ret <= MEAN_RTOL, (what, e_m2, e_mean, e_ret)
    k = np.float32(ctx.reward_norm_factor())
    u = float(ulp32(k, exact_factor(exact[1][0], exact[1][2], 1.0, EPS)))
    print(f"{what}: factor {u:.1f} ulp of the exact one")
    assert u <= 1.0, (what, u)
    # ... and exactly float32 of the expression in numpy fp64 from the state read back
    assert bits(k) == bits(factor(count, m2, 1.0, EPS)), what
    return count, mean, m2, ret


SPLIT = (1, 17, 1025, 3957)     # mapped staging, staged copy, across the 1024-row chunk, the rest


def test_state_fixture_against_exact_arithmetic_and_repeatable():
    r, d, e = fixture()
    _, ret_exact = exact_returns(r, d, e, GAMMA)
    got = []
    for _ in range(2):
        ctx, cfg = stats_ctx()
        try:
            assert cfg.gamma == GAMMA
            assert ctx.reward_norm() == (1, 1.0, EPS, 10.0)
            assert ctx.reward_norm_factor() == 1.0         # count == 0: the scale alone
            lo = 0
            for m in SPLIT:
                push_rewards(ctx, r[lo:lo + m], d[lo:lo + m], e[lo:lo + m])
                lo += m
            assert lo == len(r) == len(ctx)
            got.append(check_state(ctx, fixture_exact(), ret_exact, "fixture 1+17+1025+3957"))
        finally:
            ctx.close()
    assert got[0][0] == 5000.0
    assert np.array_equal(bits64(got[0]), bits64(got[1]))   # the same pushes: the same bits


def test_one_row_pushes_between_synchronous_updates_are_all_counted():
    """The trainer's loop: a row per env step, a synchronous update behind it.  Off, such rows
    wait in the push mailbox for the update's sampler; in mode 1 they bypass it."""
    r, d, e = (x[140:168] for x in fixture(400, 25, 12))
    assert (d | e)[8:].any()
    ctx, _ = stats_ctx(capacity=64)
    try:
        push_rewards(ctx, r[:8], d[:8], e[:8])
        for i in range(8, 28):
            push_rewards(ctx, r[i:i + 1], d[i:i + 1], e[i:i + 1])
            ctx.step(4)
            xs, ret = exact_returns(r[:i + 1], d[:i + 1], e[:i + 1], GAMMA)
            check_state(ctx, (xs, exact_moments(xs)), ret, f"after row {i}")
            assert len(ctx) == i + 1
    finally:
        ctx.close()


def test_push_past_capacity_counts_what_is_stored_and_clear_keeps_the_state():
    r, d, e = (x[:79] for x in fixture(400, 26, 12))
    ctx, _ = stats_ctx(capacity=64)
    try:
        push_rewards(ctx, r[:10], d[:10], e[:10])
        push_rewards(ctx, r[10:], d[10:], e[10:])          # capacity + 5 rows: the first 5 are skipped
        x0, _ = exact_returns(r[:10], d[:10], e[:10], GAMMA)
        x1, ret = exact_returns(r[15:], d[15:], e[15:], GAMMA)      # ret restarts at 0
        before = check_state(ctx, (x0 + x1, exact_moments(x0 + x1)), ret, "capacity + 5")
        ctx.replay_clear()
        assert np.array_equal(bits64(before), bits64(ctx.reward_norm_state()))
    finally:
        ctx.close()


def test_frozen_pushes_leave_every_word_and_mark_episode_end_zeroes_ret():
    r, d, e = (x[:60].copy() for x in fixture(400, 27, 12))
    d[40:], e[40:] = False, False
    ctx, _ = stats_ctx(capacity=256)
    try:
        push_rewards(ctx, r[:50], d[:50], e[:50])
        st0, k0 = ctx.reward_norm_state(), ctx.reward_norm_factor()
        assert st0[3] != 0.0
        ctx.set_reward_norm(2, 1.0, EPS, 10.0)
        push_rewards(ctx, r[50:], d[50:], np.ones(10, bool))         # frozen: stored, not counted
        assert len(ctx) == 60
        assert np.array_equal(bits64(st0), bits64(ctx.reward_norm_state()))
        assert ctx.reward_norm_factor() == k0
        ctx.set_reward_norm(3, 0.5, EPS, 10.0)              # switching modes leaves the state alone
        assert ctx.reward_norm_factor() == 0.5
        push_rewards(ctx, r[:3], d[:3])
        ctx.set_reward_norm(1, 1.0, EPS, 10.0)
        assert np.array_equal(bits64(st0), bits64(ctx.reward_norm_state()))
        assert ctx.reward_norm_factor() == k0
        ctx.mark_episode_end()                              # n-step off: accepted, feeds the reset only
        st1 = ctx.reward_norm_state()
        assert st1[3] == 0.0 and np.array_equal(bits64(st0[:3]), bits64(st1[:3]))
        assert not ctx.get_episode_ends(np.arange(len(ctx))).any()
        push_rewards(ctx, r[:1], [False])
        assert ctx.reward_norm_state()[3] == float(r[0]) and ctx.reward_norm_state()[0] == 51.0
        ctx.set_reward_norm_state(7.0, 0.5, 3.5, -2.0)
        assert ctx.reward_norm_state() == (7.0, 0.5, 3.5, -2.0)
        assert bits(ctx.reward_norm_factor()) == bits(factor(7.0, 3.5, 1.0, EPS))
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# 2. equivalence, frozen
@pytest.mark.parametrize("name", list(CASES))
def test_equivalence_frozen(name):
    rows, end, model = case_rows(name)
    ra, rb, k, st = equivalence(name)
    assert st[0] == len(rows[2])
    xs, _ = exact_returns(rows[2], rows[4], end, GAMMA)
    e_m2, e_mean = state_errors(*st[:3], (xs, exact_moments(xs)))
    print(f"{name}: M2 {e_m2:.2e} relative, mean {e_mean:.2e} of max|ret|, k {k:.6g}")
    assert e_m2 <= M2_RTOL and e_mean <= MEAN_RTOL
    assert bits(k) == bits(factor(st[0], st[2], 1.0, EPS))
    clipped = np.abs(rows[2] * np.float32(k)) > CLIP
    assert clipped.any() and not clipped.all(), clipped.mean()
    print(f"{name}: {clipped.mean():.1%} of the rewards clipped")
    assert all(np.all(np.isfinite(l)) for l in ra["losses"])
    assert_same(ra, rb, name)
    assert differs(ra, raw_off(name)), "the control: an off context on the raw rewards must differ"


def test_update_right_behind_a_push_sees_all_its_rows():
    name = SMALL
    S, H, B, dt, n, kind, seed = CASES[name]
    cfg = ton.case_inputs(name)[0]
    rows, end, _ = case_rows(name)
    a = new_ctx(name)
    try:
        a.set_reward_norm(1, 1.0, EPS, CLIP)
        a.push(*rows, episode_end=end)                  # 64 rows
        a.step_async(B)                                 # no synchronisation in between
        ra = snapshot(a, cfg)
        ra["losses"] = [a.fetch_losses(1)[0]]
        k = a.reward_norm_factor()
        st = a.reward_norm_state()
        assert st[0] == n and bits(k) == bits(factor(st[0], st[2], 1.0, EPS)) and k != 1.0
    finally:
        a.close()
    b = ctx_b(name, k)
    try:
        b.step_async(B)
        rb = snapshot(b, cfg)
        rb["losses"] = [b.fetch_losses(1)[0]]
    finally:
        b.close()
    assert_same(ra, rb, "update behind the push")


# ---------------------------------------------------------------------------------------------
# 3. the rides and the draw-ahead survive
def many(ctx, cfg, B, how):
    if how == "many":
        ctx.step_many_async(B, 5)
    else:
        for _ in range(5):
            ctx.step_async(B)
    ctx.step_many_async(B, 2)          # behind a multi-update launch: consumes the batch drawn ahead
    out = snapshot(ctx, cfg)
    out["losses"] = list(ctx.fetch_losses(7))
    assert len(out["losses"]) == 7
    return out


def test_multi_update_launch_equals_single_updates_and_b_and_still_rides():
    name = SMALL
    B = CASES[name][2]
    cfg = ton.case_inputs(name)[0]
    res = {}
    for how in ("many", "single"):
        a = ctx_a(name)
        try:
            k = a.reward_norm_factor()
            ride_a = a.ride_possible(B)
            res[how] = many(a, cfg, B, how)
        finally:
            a.close()
    b = ctx_b(name, k)
    try:
        assert ride_a == b.ride_possible(B) and ride_a           # what a never-enabled context reports
        res["b"] = many(b, cfg, B, "many")
    finally:
        b.close()
    assert_same(res["many"], res["single"], "step_many_async vs five single updates")
    assert_same(res["many"], res["b"], "step_many_async vs B")


def test_launch_timeline_keeps_the_rides_and_names_the_new_launch():
    """One 3-update launch: the feature adds one k_reward_norm launch per update and removes no
    ride (the later updates still have no sampler / gather launch of their own)."""
    name = SMALL
    B = CASES[name][2]
    names = {}
    for on in (True, False):
        ctx = ctx_a(name) if on else ctx_b(name, 1.0)
        try:
            tl, _ = ctx.profile_timeline(B, 3, launch=True)
            names[on] = [t["site"] for t in tl]
        finally:
            ctx.close()
    mine = [n for n in names[True] if n.startswith("reward_norm")]
    assert len(mine) == 3, names[True]
    assert [n for n in names[True] if not n.startswith("reward_norm")] == names[False]


def test_mode_3_constant_scale():
    name = SMALL
    rows, end, _ = case_rows(name)
    a = new_ctx(name)
    try:
        a.set_reward_norm(3, 0.25, EPS, math.inf)
        a.push(*rows)
        assert a.reward_norm_factor() == 0.25 and a.reward_norm_state() == (0.0, 0.0, 0.0, 0.0)
        ra = two_updates(a, name)
    finally:
        a.close()
    b = new_ctx(name)
    try:
        s, a_, r, s2, d = rows
        b.push(s, a_, (r * np.float32(0.25)).astype(np.float32), s2, d)   # a power of two: exact
        rb = two_updates(b, name)
    finally:
        b.close()
    assert_same(ra, rb, "mode 3")
    assert differs(ra, raw_off(name))


def test_with_nstep_the_collapsed_return_is_scaled_and_clipped():
    name = tn.NORM_CASE
    cfg, _, rows, end, ring = tn.case_inputs(name)[:5]
    n = tn.CASES[name][7]
    k, clip = 0.37, 0.5
    a = tn.new_ctx(name)
    try:
        a.set_nstep(n)
        a.set_reward_norm(2, 1.0, EPS, clip)
        a.set_reward_norm_state(10.0, 0.0, 10.0 / (k * k), 0.0)
        kf = a.reward_norm_factor()
        tn.push_chunks(a, rows, end)
        ra = tn.two_updates(a, name)
        B = tn.CASES[name][2]
        raw, _ = a.read_batch_rd(B)
        rn = a.read_batch_rn(B)
    finally:
        a.close()
    s, a_, r, s2, d = rows
    (cs, ca, cR, cs2, cd), dprime = collapsed_rows(ring, n, cfg.gamma, s, a_, s2)
    y = normalize(cR, kf, clip)
    hit = np.abs(cR * np.float32(kf)) > clip
    assert hit.any() and not hit.all()
    assert np.array_equal(bits(rn), bits(normalize(raw, kf, clip)))   # the clip bounds R k
    b = tn.new_ctx(name)
    try:
        b.push(*[x[:tn.EXTRA] for x in rows])
        b.push(cs, ca, y, cs2, cd)
        b.debug_set_done((ring.head + np.arange(ring.length)) % ring.capacity, dprime)
        rb = tn.two_updates(b, name)
    finally:
        b.close()
    tn.assert_same(ra, rb, "n-step + reward normalisation")


def test_with_obs_norm_diagnostics_clipping_and_prioritized_feedback():
    name = "S11-H96-B40-per"
    B = CASES[name][2]
    cfg, mom = ton.case_inputs(name)[0], ton.case_inputs(name)[5]

    def run(ctx):
        ctx.per_set_feedback(True)
        ctx.set_stats(True)
        ctx.set_grad_clip(0.5, 0.5)
        losses = [np.asarray(ctx.step(B), np.float32) for _ in range(2)]
        ctx.step_many_async(B, 2)                      # (prioritized: the side-stream form)
        losses += list(ctx.fetch_losses(2))
        out = snapshot(ctx, cfg)
        out.update(losses=losses, stats=ctx.fetch_stats()[0], gn=ctx.fetch_grad_norms()[0],
                   prio=ctx.per_priorities())
        return out

    def obs_on(ctx):
        ctx.set_obs_norm(2, ton.EPS, ton.CLIP)
        ctx.set_obs_norm_moments(mom.count, mom.mean, mom.m2)

    rows, end, _ = case_rows(name)
    a = new_ctx(name)
    try:
        obs_on(a)
        a.set_reward_norm(1, 1.0, EPS, CLIP)
        a.push(*rows, episode_end=end)
        a.set_reward_norm(2, 1.0, EPS, CLIP)
        k = a.reward_norm_factor()
        ra = run(a)
    finally:
        a.close()
    b = new_ctx(name)
    try:
        obs_on(b)
        s, a_, r, s2, d = rows
        b.push(s, a_, normalize(r, k, CLIP), s2, d)
        rb = run(b)
    finally:
        b.close()
    assert_same(ra, rb, "all five features")
    assert len(ra["losses"]) == 4 and ra["stats"].shape[0] == 4 and ra["gn"].shape[0] == 4
    for key in ("stats", "gn", "prio"):
        assert np.array_equal(bits(ra[key]), bits(rb[key])), key


@pytest.mark.parametrize("name", [SMALL, "S11-H96-B40-per"])
def test_read_batch_rn_is_the_model_and_rd_stays_raw(name):
    S, H, B, dt, n, kind, seed = CASES[name]
    rows = case_rows(name)[0]
    a = ctx_a(name)
    try:
        k = a.reward_norm_factor()
        two_updates(a, name)
        raw, _ = a.read_batch_rd(B)
        rn = a.read_batch_rn(B)
    finally:
        a.close()
    assert np.isin(bits(raw), bits(rows[2])).all()                    # raw rewards of the ring
    assert np.array_equal(bits(rn), bits(normalize(raw, k, CLIP)))
    assert (np.abs(rn) == CLIP).any() and not (np.abs(rn) == CLIP).all()


# ---------------------------------------------------------------------------------------------
# 4. off is off; the settings are not in the graph key
def test_on_then_off_is_never_enabled_and_settings_add_no_graph():
    from sacmi import _lib as L
    name = SMALL
    B = CASES[name][2]
    rows, end, _ = case_rows(name)
    ctx = new_ctx(name)
    try:
        ctx.set_reward_norm(1, 1.0, EPS, CLIP)
        ctx.push(*rows, episode_end=end)
        ctx.set_reward_norm(0, 1.0, EPS, CLIP)
        assert ctx.reward_norm()[0] == 0
        res = two_updates(ctx, name)
        ctx.step_async(B)                               # (the off form of the launches below)
        g_off = int(ctx.get_scalar(L.S_GRAPH_COUNT))
        ctx.set_reward_norm(1, 1.0, EPS, CLIP)
        ctx.step_async(B)
        g_on = int(ctx.get_scalar(L.S_GRAPH_COUNT))
        assert g_on > g_off                             # on and off are distinct captured graphs
        for mode, scale, clip in ((2, 1.0, 3.0), (3, 0.5, math.inf), (1, 2.0, 0.5), (2, 2.0, 0.5)):
            ctx.set_reward_norm(mode, scale, EPS, clip)
            ctx.step_async(B)
        ctx.set_reward_norm_state(5.0, 1.0, 2.0, 0.0)
        ctx.step_async(B)
        ctx.synchronize()
        assert int(ctx.get_scalar(L.S_GRAPH_COUNT)) == g_on
    finally:
        ctx.close()
    assert_same(res, raw_off(name), "enabled then disabled")


# ---------------------------------------------------------------------------------------------
# 5. NaN, refusals
def test_nan_reward_behaves_as_without_the_feature():
    """A NaN reward in the minibatch stays a NaN through the scaling and the clip; frozen
    statistics stay usable, and a normal reward pushed behind it is normalised as before."""
    name = SMALL
    S, H, B, dt, n, kind, seed = CASES[name]
    cfg, _, _, idx, eps, _ = ton.case_inputs(name)
    (s, a_, r, s2, d), end, _ = case_rows(name)
    r = r.copy()
    bad = int(idx[0][3])
    r[bad] = np.nan

    def run(ctx):
        out = []
        for u in range(2):
            try:
                out.append(np.asarray(ctx.step(B, idx[u], eps[2 * u], eps[2 * u + 1]), np.float32))
            except Exception as e:           # whatever a context without the feature does
                out.append(type(e).__name__)
        return out

    a = new_ctx(name)
    try:
        a.set_reward_norm(2, 1.0, EPS, CLIP)
        a.set_reward_norm_state(10.0, 0.0, 40.0, 0.0)
        k = a.reward_norm_factor()
        a.push(s, a_, r, s2, d)
        ra = run(a)
        rn = a.read_batch_rn(B)
        raw, _ = a.read_batch_rd(B)
    finally:
        a.close()
    b = new_ctx(name)
    try:
        b.push(s, a_, normalize(r, k, CLIP), s2, d)
        rb = run(b)
    finally:
        b.close()
    assert len(ra) == len(rb) == 2
    for x, y in zip(ra, rb):
        assert type(x) is type(y)
        assert x == y if isinstance(x, str) else np.array_equal(bits(x), bits(y))
    assert np.array_equal(bits(rn), bits(normalize(raw, k, CLIP)))
    # mode 1: the NaN enters the statistics (documented), and set_state repairs them
    ctx, _ = stats_ctx(capacity=64)
    try:
        push_rewards(ctx, np.array([1.0, np.nan, 2.0], np.float32), [False, True, False])
        st = ctx.reward_norm_state()
        assert st[0] == 3.0 and math.isnan(st[2]) and st[3] == 2.0     # ret restarted behind the terminal
        assert math.isnan(ctx.reward_norm_factor())
        ctx.set_reward_norm_state(2.0, 1.5, 0.5, 2.0)
        assert bits(ctx.reward_norm_factor()) == bits(factor(2.0, 0.5, 1.0, EPS))
    finally:
        ctx.close()


def test_refusals():
    from sacmi import _lib as L
    name = SMALL
    S, H, B, dt, n, kind, seed = CASES[name]
    cfg = ton.case_inputs(name)[0]
    rows, end, _ = case_rows(name)
    estate = f"sacmi error {L.SACMI_ESTATE}"
    a = ctx_a(name, mode=1)
    try:
        before = ctx_state(a, cfg)
        for mode in (1, 2, 3):
            a.set_reward_norm(mode, 1.0, EPS, CLIP)
            for f in (lambda: a.step_phase(B, 0), lambda: a.step_phase(B, 1, 1.0, 1, False, False)):
                with pytest.raises(L.SacmiError, match=estate):
                    f()
        a.set_reward_norm(0, 1.0, EPS, CLIP)
        a.dp_loopback_init(2)
        a.set_reward_norm(3, 0.5, EPS, CLIP)
        with pytest.raises(L.SacmiError, match=estate):
            a.step_dp(B, 1)
        after = ctx_state(a, cfg)
        for key in before:
            assert np.array_equal(bits(before[key]), bits(after[key])), key
        # episode-end flags with n-step off: modes 0 and 3 refuse as before, 1 and 2 accept
        one = [x[:1] for x in rows]
        for mode in (0, 3):
            a.set_reward_norm(mode, 0.5, EPS, CLIP)
            with pytest.raises(L.SacmiError, match=estate):
                a.push(*one, episode_end=[True])
            with pytest.raises(L.SacmiError, match=estate):
                a.mark_episode_end()
        for mode in (1, 2):
            a.set_reward_norm(mode, 0.5, EPS, CLIP)
            a.push(*one, episode_end=[True])
            a.mark_episode_end()
        a.set_reward_norm(1, 1.0, EPS, CLIP)
        for bad in (lambda: a.set_reward_norm(4, 1.0, EPS, 10.0), lambda: a.set_reward_norm(-1, 1.0, EPS, 10.0),
                    lambda: a.set_reward_norm(1, 0.0, EPS, 10.0), lambda: a.set_reward_norm(1, -1.0, EPS, 10.0),
                    lambda: a.set_reward_norm(1, math.inf, EPS, 10.0),
                    lambda: a.set_reward_norm(1, math.nan, EPS, 10.0),
                    lambda: a.set_reward_norm(1, 1.0, -1e-8, 10.0), lambda: a.set_reward_norm(1, 1.0, math.nan, 10.0),
                    lambda: a.set_reward_norm(1, 1.0, math.inf, 10.0),
                    lambda: a.set_reward_norm(1, 1.0, EPS, 0.0), lambda: a.set_reward_norm(1, 1.0, EPS, -1.0),
                    lambda: a.set_reward_norm(1, 1.0, EPS, math.nan),
                    lambda: a.set_reward_norm_state(-1.0, 0.0, 1.0, 0.0),
                    lambda: a.set_reward_norm_state(5.0, 0.0, -1.0, 0.0),
                    lambda: a.set_reward_norm_state(5.0, math.nan, 1.0, 0.0),
                    lambda: a.set_reward_norm_state(5.0, 0.0, 1.0, math.inf)):
            with pytest.raises(ValueError):
                bad()
        assert a.reward_norm() == (1, 1.0, EPS, CLIP)
        a.set_reward_norm(1, 1.0, EPS, math.inf)           # +inf: no clipping, accepted
        assert a.reward_norm() == (1, 1.0, EPS, math.inf)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------
# 6. drop-in
def test_drop_in_agent_and_checkpoints(tmp_path):
    from sacmi import SAC
    S, A, n = 11, 3, 80
    r, d, e = (x[100:100 + n] for x in fixture(400, 28, 12))
    rng = np.random.default_rng(9)
    x = rng.standard_normal((n + 1, S)).astype(np.float32)

    def fill(agent, flags=True):
        for i in range(n):
            kw = {"episode_end": bool(e[i])} if flags else {}
            agent.replay_buffer.push(x[i], rng.uniform(-0.4, 0.4, A).astype(np.float32), float(r[i]),
                                     x[i + 1], bool(d[i]), **kw)

    agent = SAC(S, A, 64, capacity=256, max_batch=32, seed=3, normalize_reward=True, reward_clip=5.0)
    assert agent._ctx.reward_norm() == (1, 1.0, 1e-8, 5.0)
    fill(agent)
    out = agent.update_parameters(32)
    assert all(math.isfinite(v) for v in out.values())
    st = agent.reward_norm_state()
    xs, ret = exact_returns(r, d, e, agent.gamma)
    e_m2, e_mean = state_errors(st["count"], st["mean"], st["var"] * n, (xs, exact_moments(xs)))
    assert st["count"] == n and e_m2 <= M2_RTOL and e_mean <= MEAN_RTOL
    agent.freeze_reward_norm(True)
    agent.replay_buffer.push(x[0], np.zeros(A, np.float32), 3.0, x[1], False)
    agent.update_parameters(32)
    assert agent.reward_norm_state()["count"] == n
    agent.freeze_reward_norm(False)
    agent.replay_buffer.push(x[0], np.zeros(A, np.float32), 3.0, x[1], False)
    agent.replay_buffer.mark_episode_end()
    agent.update_parameters(32)
    state = agent._ctx.reward_norm_state()
    assert state[0] == n + 1 and state[3] == 0.0

    full, nets = str(tmp_path / "full.pt"), str(tmp_path / "nets.pt")
    agent.save_checkpoint(full, 1, 2)
    agent.save(nets)
    assert "reward_norm" in torch.load(nets, weights_only=True)

    fresh = SAC(S, A, 64, capacity=256, max_batch=32, seed=4, normalize_reward=True, reward_clip=7.0)
    fresh.load_checkpoint(full)                        # (reloads the 82 replay rows: not counted)
    assert len(fresh.replay_buffer) == n + 2
    assert np.array_equal(bits64(fresh._ctx.reward_norm_state()), bits64(state))
    assert fresh._ctx.reward_norm() == (1, 1.0, 1e-8, 5.0)
    assert fresh._ctx.reward_norm_factor() == agent._ctx.reward_norm_factor()

    other = SAC(S, A, 64, capacity=256, max_batch=32, seed=5)
    assert other._ctx.reward_norm()[0] == 0
    other.load(nets)
    assert other._ctx.reward_norm() == (1, 1.0, 1e-8, 5.0)
    assert np.array_equal(bits64(other._ctx.reward_norm_state()), bits64(state))

    # a checkpoint without the entry loads and leaves the statistics as they are
    plain = SAC(S, A, 64, capacity=256, max_batch=32, seed=6)
    fill(plain, flags=False)
    with pytest.raises(ValueError):                    # flags need n-step or return statistics
        plain.replay_buffer.push(x[0], np.zeros(A, np.float32), 0.0, x[1], False, episode_end=True)
        plain.replay_buffer._flush()
    plain.replay_buffer._ends[-1] = False
    old = str(tmp_path / "plain.pt")
    plain.save_checkpoint(old, 0, 0)
    assert "reward_norm" not in torch.load(old, weights_only=True)
    other.load_checkpoint(old, load_replay_buffer=False)
    assert np.array_equal(bits64(other._ctx.reward_norm_state()), bits64(state))

    # reward_scale alone: the constant-scale mode, no clipping unless asked for
    scaled = SAC(S, A, 64, capacity=256, max_batch=32, seed=7, reward_scale=0.1)
    assert scaled._ctx.reward_norm() == (3, 0.1, 1e-8, math.inf)
    clipped = SAC(S, A, 64, capacity=256, max_batch=32, seed=7, reward_scale=0.1, reward_clip=2.0)
    assert clipped._ctx.reward_norm() == (3, 0.1, 1e-8, 2.0)
    with pytest.raises(RuntimeError):
        scaled.freeze_reward_norm()


def test_env_switches_at_creation():
    """SACMI_REWARD_NORM=1 at creation: mode 1, scale 1, eps 1e-8, clip 10 (how the unchanged
    benchmark runs with the feature on); SACMI_REWARD_SCALE=<x>: the scale, alone mode 3."""
    name = SMALL
    want = {("1", None): (1, 1.0, 1e-8, 10.0), ("1", "0.5"): (1, 0.5, 1e-8, 10.0),
            (None, "0.25"): (3, 0.25, 1e-8, math.inf), (None, None): (0, 1.0, 1e-8, 10.0)}
    for (norm, scale), expect in want.items():
        if norm:
            os.environ["SACMI_REWARD_NORM"] = norm
        if scale:
            os.environ["SACMI_REWARD_SCALE"] = scale
        try:
            ctx = new_ctx(name)
        finally:
            os.environ.pop("SACMI_REWARD_NORM", None)
            os.environ.pop("SACMI_REWARD_SCALE", None)
        try:
            assert ctx.reward_norm() == expect
            ctx.push(*case_rows(name)[0])
            ctx.step(CASES[name][2])
            assert ctx.reward_norm_state()[0] == (CASES[name][4] if expect[0] == 1 else 0.0)
        finally:
            ctx.close()
