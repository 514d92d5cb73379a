"""Running observation normalisation on the GPU (sacmi_set_obs_norm; csrc/obsnorm.hip, the NORM
gather of csrc/replay_dev.h).

The moments are checked against exact rational arithmetic with the CPU bounds of
tests/test_obs_norm_model.py.  Everything downstream is checked by EQUIVALENCE, bit for bit:
context A has the feature on and holds raw rows; context B never enabled it and holds the rows
normalised in numpy (tests/obs_norm_model.py normalize) with A's vectors read back.  Same
parameters, same indices and noise (or the same generator key): losses, parameters, targets,
Adam moments and the alpha state must be identical after the updates, because the only
difference is WHERE the fp32 expression ran.  Raw columns carry different scales and offsets and
the clip is 1.5, so some but not all elements are clipped.
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle.sac_step import SacConfig, init_params, param_shapes, synthetic_rows

from obs_norm_model import (RunningMoments, exact_moments, exact_vectors, fixture_exact, fixture_rows,
                            moment_errors, normalize, ulp32, vectors)
from test_gpu_parity import ctx_alpha_state, ctx_state, load_params, make_ctx

pytestmark = pytest.mark.gpu

M2_RTOL, MEAN_RTOL = 1e-9, 1e-12      # the CPU bounds (tests/test_obs_norm_model.py)
EPS, CLIP = 1e-8, 1.5
KEY = (np.arange(624, dtype=np.uint64) * 1812433 % (2 ** 32)).astype(np.uint32)
GROUPS = ("policy", "q1", "q2")

# name -> S, H, B, compute dtype, replay rows, replay kind, seed
CASES = {
    "S11-H96-B40": (11, 96, 40, "fp32", 64, "uniform", 2001),
    "S12-H96-B40": (12, 96, 40, "fp32", 64, "uniform", 2002),
    "S11-H96-B40-per": (11, 96, 40, "fp32", 64, "per", 2003),
    "S11-H512-B4096-bf16": (11, 512, 4096, "bf16", 4200, "uniform", 2004),
    "S11-H96-B4100": (11, 96, 4100, "fp32", 4200, "uniform", 2005),
}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    S, H, B, dt, n, kind, seed = CASES[name]
    cfg = SacConfig(S, 3, H)
    params = init_params(cfg, seed, bias_scale=0.05)
    s, a, r, s2, d = synthetic_rows(cfg, n, seed + 1000, state_scale=0.5)
    rng = np.random.default_rng(seed + 2000)
    # columns of different scale and offset, as real observations have
    scale = (10.0 ** rng.uniform(-2, 2, S)).astype(np.float32)
    off = (rng.standard_normal(S) * 5).astype(np.float32)
    s, s2 = s * scale + off, s2 * scale + off
    idx = [rng.permutation(n)[:B] for _ in range(2)]
    eps = [rng.standard_normal((B, 3)).astype(np.float32) for _ in range(4)]
    mom = RunningMoments(S, "device").update(s)
    return cfg, params, (s, a, r, s2, d), idx, eps, mom


def new_ctx(name, **kw):
    S, H, B, dt, n, kind, seed = CASES[name]
    cfg, params = case_inputs(name)[:2]
    ctx = make_ctx(cfg, max_batch=max(B, 128), capacity=n, seed=5, compute_dtype=dt, replay=kind, **kw)
    load_params(ctx, params)
    ctx.set_mt(0, KEY, 624)
    if kind == "per":
        ctx.set_mt(1, KEY, 624)
    return ctx


def ctx_a(name, mode=2, clip=CLIP):
    """Feature on, raw rows, the moments set from the model."""
    rows, mom = case_inputs(name)[2], case_inputs(name)[5]
    ctx = new_ctx(name)
    ctx.set_obs_norm(2, EPS, clip)
    ctx.set_obs_norm_moments(mom.count, mom.mean, mom.m2)
    ctx.push(*rows)                      # (frozen: not counted)
    if mode != 2:
        ctx.set_obs_norm(mode, EPS, clip)
    return ctx


def normalised_rows(rows, nmean, nrstd, clip=CLIP):
    s, a, r, s2, d = rows
    return normalize(s, nmean, nrstd, clip), a, r, normalize(s2, nmean, nrstd, clip), d


def ctx_b(name, vec, clip=CLIP):
    """Never enabled; the rows normalised in numpy with A's vectors."""
    ctx = new_ctx(name)
    ctx.push(*normalised_rows(case_inputs(name)[2], *vec, clip))
    return ctx


def snapshot(ctx, cfg):
    shapes = param_shapes(cfg)
    out = {"state": ctx_state(ctx, cfg), "alpha": ctx_alpha_state(ctx)}
    for slot in ("m", "v"):
        out[slot] = {f"{n}.{k}": v for n in GROUPS for k, v in ctx.get_net(n, slot, shapes[n]).items()}
    return out


def assert_same(a, b, what):
    for la, lb in zip(a["losses"], b["losses"]):
        assert np.array_equal(bits(la), bits(lb)), (what, "losses", la, lb)
    for part in ("state", "m", "v"):
        for k in a[part]:
            assert np.array_equal(bits(a[part][k]), bits(b[part][k])), (what, part, k)
    assert a["alpha"] == b["alpha"], (what, a["alpha"], b["alpha"])


def differs(a, b):
    return any(not np.array_equal(bits(a["state"][k]), bits(b["state"][k])) for k in a["state"])


def two_updates(ctx, name):
    """Two updates from the case's fixed state: staged indices and noise, or (prioritized) the
    device's own draw and noise; everything they leave."""
    S, H, B, dt, n, kind, seed = CASES[name]
    cfg, _, _, idx, eps, _ = case_inputs(name)
    losses = []
    for u in range(2):
        if kind == "per":
            losses.append(np.asarray(ctx.step(B), np.float32))
        else:
            losses.append(np.asarray(ctx.step(B, idx[u], eps[2 * u], eps[2 * u + 1]), np.float32))
    out = snapshot(ctx, cfg)
    out["losses"] = losses
    return out


@functools.lru_cache(maxsize=None)
def equivalence(name):
    """(A, B, vectors): the two-update results of A (on, frozen, raw rows) and of B."""
    a = ctx_a(name)
    try:
        vec = a.obs_norm_vectors()
        ra = two_updates(a, name)
    finally:
        a.close()
    b = ctx_b(name, vec)
    try:
        rb = two_updates(b, name)
    finally:
        b.close()
    return ra, rb, vec


@functools.lru_cache(maxsize=None)
def raw_off(name):
    """An off context holding the raw rows: the control."""
    ctx = new_ctx(name)
    try:
        ctx.push(*case_inputs(name)[2])
        return two_updates(ctx, name)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# 1. moments
def stats_ctx(S, capacity=8192, mode=1, eps=EPS, clip=10.0):
    cfg = SacConfig(S, 3, 32)
    ctx = make_ctx(cfg, max_batch=8, capacity=capacity, seed=5)
    load_params(ctx, init_params(cfg, 77, bias_scale=0.05))
    if mode:
        ctx.set_obs_norm(mode, eps, clip)
    return ctx, cfg


def push_states(ctx, s, s2=None):
    """Transitions whose state is s and whose next state is something else entirely."""
    n = len(s)
    rng = np.random.default_rng(5)
    s2 = (1e3 + rng.standard_normal(s.shape)).astype(np.float32) if s2 is None else s2
    ctx.push(s, np.zeros((n, 3), np.float32), np.zeros(n, np.float32), s2, np.zeros(n, np.uint8))


def check_moments(ctx, rows, exact=None, what=""):
    count, mean, m2 = ctx.obs_norm_moments()
    assert count == len(rows), (what, count)
    e_m2, e_mean = moment_errors(count, mean, m2, rows, exact)
    print(f"{what}: count {count:.0f}, M2 {e_m2:.2e} relative, mean {e_mean:.2e} of max|x|")
    assert e_m2 <= M2_RTOL and e_mean <= MEAN_RTOL, (what, e_m2, e_mean)
    ex = exact if exact is not None else exact_moments(rows)
    nmean, nrstd = ctx.obs_norm_vectors()
    want_mean, want_rstd = exact_vectors(*ex, EPS)
    u = max(ulp32(nmean, want_mean).max(), ulp32(nrstd, want_rstd).max())
    print(f"{what}: vectors {u:.1f} ulp of the exact ones")
    assert u <= 1.0, (what, u)
    # ... and exactly float32 of the expression in numpy fp64 from the moments read back
    mine = vectors(count, mean, m2, EPS)
    assert np.array_equal(bits(nmean), bits(mine[0])), what
    assert np.array_equal(bits(nrstd), bits(mine[1])), what
    return count, mean, m2


SPLIT = (1, 17, 1025, 3957)     # mapped staging, staged copy, across the 1024-row chunk, the rest


def push_fixture(ctx, x):
    lo = 0
    for m in SPLIT:
        push_states(ctx, x[lo:lo + m])
        lo += m
    assert lo == len(x)


def test_moments_fixture_against_exact_arithmetic_and_repeatable():
    x = fixture_rows()
    got = []
    for _ in range(2):
        ctx, _ = stats_ctx(x.shape[1])
        try:
            assert ctx.obs_norm() == (1, EPS, 10.0)
            nm, nr = ctx.obs_norm_vectors()           # count == 0: the identity
            assert np.array_equal(nm, np.zeros_like(nm)) and np.array_equal(nr, np.ones_like(nr))
            push_fixture(ctx, x)
            got.append(check_moments(ctx, x, fixture_exact(), "fixture 1+17+1025+3957"))
            assert len(ctx) == len(x)
        finally:
            ctx.close()
    assert got[0][0] == got[1][0] == 5000.0
    for a, b in zip(got[0][1:], got[1][1:]):            # the same pushes: the same bits
        assert np.array_equal(bits64(a), bits64(b))
    assert got[0][2][5] == 0.0 and got[0][1][5] == -2.5  # the constant column, exactly


@pytest.mark.parametrize("S,n", [(12, 300), (661, 40)])
def test_moments_other_widths(S, n):
    """S = 12: no S % 4 tail; S = 661: 42 workgroups of columns, the last one partly empty."""
    x = fixture_rows(S, n, 21 + S)
    ctx, _ = stats_ctx(S, capacity=512)
    try:
        push_states(ctx, x[:3])
        push_states(ctx, x[3:])
        check_moments(ctx, x, None, f"S{S}")
    finally:
        ctx.close()


def test_one_row_pushes_between_synchronous_updates_are_all_counted():
    """The trainer's loop: a row per env step, a synchronous update behind it.  Off, such rows
    wait in the push mailbox for the update's sampler; in mode 1 they bypass it."""
    x = fixture_rows(11, 28, 31)
    ctx, _ = stats_ctx(11, capacity=64)
    try:
        push_states(ctx, x[:8])
        for i in range(8, 28):
            push_states(ctx, x[i:i + 1])
            ctx.step(4)
            check_moments(ctx, x[:i + 1], None, f"after row {i}")
            assert len(ctx) == i + 1
    finally:
        ctx.close()


def test_push_past_capacity_counts_what_is_stored_and_clear_keeps_the_moments():
    x = fixture_rows(11, 69, 32)
    ctx, _ = stats_ctx(11, capacity=64)
    try:
        push_states(ctx, x)                            # capacity + 5 rows: the first 5 are skipped
        before = check_moments(ctx, x[5:], None, "capacity + 5")
        ctx.replay_clear()
        after = ctx.obs_norm_moments()
        assert after[0] == 64.0
        assert np.array_equal(bits64(before[1]), bits64(after[1]))
        assert np.array_equal(bits64(before[2]), bits64(after[2]))
    finally:
        ctx.close()


def test_frozen_pushes_leave_the_moments_and_explicit_update_counts():
    x = fixture_rows(11, 2100, 33)
    ctx, _ = stats_ctx(11, capacity=4096)
    try:
        push_states(ctx, x[:50])
        ctx.set_obs_norm(2, EPS, 10.0)
        c0 = ctx.obs_norm_moments()
        push_states(ctx, x[50:60])                     # frozen: stored, not counted
        c1 = ctx.obs_norm_moments()
        assert c1[0] == 50.0 and np.array_equal(bits64(c0[2]), bits64(c1[2]))
        ctx.obs_norm_update(x[60:])                    # 2040 rows: two chunks; counts though frozen
        check_moments(ctx, np.concatenate([x[:50], x[60:]]), None, "explicit update, frozen")
        ctx.set_obs_norm(0, EPS, 10.0)
        with pytest.raises(Exception, match="off"):
            ctx.obs_norm_update(x[:4])
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# 2. gather equivalence, frozen
@pytest.mark.parametrize("name", list(CASES))
def test_gather_equivalence_frozen(name):
    S, H, B, dt, n, kind, seed = CASES[name]
    rows = case_inputs(name)[2]
    ra, rb, vec = equivalence(name)
    t = (np.concatenate([rows[0], rows[3]]) - vec[0]) * vec[1]
    clipped = np.abs(t) > CLIP
    assert clipped.any() and not clipped.all(), clipped.mean()
    print(f"{name}: {clipped.mean():.1%} of the elements clipped")
    assert all(np.all(np.isfinite(l)) for l in ra["losses"])
    assert_same(ra, rb, name)
    assert differs(ra, raw_off(name)), "the control: an off context on the raw rows must differ"


# ---------------------------------------------------------------------------------------------
# 3. ordering: the gather behind a push sees the statistics of every pushed row
def test_update_right_behind_a_push_sees_all_its_rows():
    name = "S11-H96-B40"
    S, H, B, dt, n, kind, seed = CASES[name]
    cfg, _, rows, _, _, _ = case_inputs(name)
    a = new_ctx(name)
    try:
        a.set_obs_norm(1, EPS, CLIP)
        a.push(*rows)                                  # 64 rows
        a.step_async(B)                                # no synchronisation in between
        ra = snapshot(a, cfg)
        ra["losses"] = [a.fetch_losses(1)[0]]
        vec = a.obs_norm_vectors()
        count, mean, m2 = a.obs_norm_moments()
        assert count == n
        assert np.array_equal(bits(vec[1]), bits(vectors(count, mean, m2, EPS)[1]))
    finally:
        a.close()
    b = ctx_b(name, vec)
    try:
        b.step_async(B)
        rb = snapshot(b, cfg)
        rb["losses"] = [b.fetch_losses(1)[0]]
    finally:
        b.close()
    assert_same(ra, rb, "update behind the push")


# ---------------------------------------------------------------------------------------------
# 4. multi-update launches, 5. off is off
def many(ctx, cfg, B, how):
    if how == "many":
        ctx.step_many_async(B, 3)
    else:
        for _ in range(3):
            ctx.step_async(B)
    out = snapshot(ctx, cfg)
    out["losses"] = list(ctx.fetch_losses(3))
    assert len(out["losses"]) == 3
    return out


def test_multi_update_launch_equals_single_updates_and_b():
    from sacmi import _lib as L
    name = "S11-H96-B40"
    B = CASES[name][2]
    cfg = case_inputs(name)[0]
    res = {}
    for how in ("many", "single"):
        a = ctx_a(name)
        try:
            assert not a.ride_possible(B)
            vec = a.obs_norm_vectors()
            res[how] = many(a, cfg, B, how)
            if how == "single":                       # on and off are distinct captured graphs
                g_on = int(a.get_scalar(L.S_GRAPH_COUNT))
                a.step_async(B)
                assert int(a.get_scalar(L.S_GRAPH_COUNT)) == g_on
                a.set_obs_norm(0, EPS, CLIP)
                assert a.ride_possible(B)
                a.step_async(B)
                assert int(a.get_scalar(L.S_GRAPH_COUNT)) == g_on + 1
                a.set_obs_norm(2, EPS, 3.0)           # another clip, frozen <-> on: no new graph
                a.step_async(B)
                a.set_obs_norm(1, EPS, 2.0)
                a.step_async(B)
                a.synchronize()
                assert int(a.get_scalar(L.S_GRAPH_COUNT)) == g_on + 1
        finally:
            a.close()
    b = ctx_b(name, vec)
    try:
        res["b"] = many(b, cfg, B, "many")
    finally:
        b.close()
    assert_same(res["many"], res["single"], "step_many_async vs three single updates")
    assert_same(res["many"], res["b"], "step_many_async vs B")


def test_enabled_then_disabled_is_bit_identical_to_never_enabled():
    name = "S11-H96-B40"
    ctx = new_ctx(name)
    try:
        ctx.set_obs_norm(1, EPS, CLIP)
        ctx.push(*case_inputs(name)[2])
        ctx.set_obs_norm(0, EPS, CLIP)
        assert ctx.obs_norm()[0] == 0
        res = two_updates(ctx, name)
    finally:
        ctx.close()
    assert_same(res, raw_off(name), "enabled then disabled")


# ---------------------------------------------------------------------------------------------
# 6. select_action
@pytest.mark.parametrize("n", [1, 7, 200])
def test_act_equals_act_on_normalised_states(n):
    """n = 1: the one-state GEMV path (its own operand buffer), 7: mapped staging, 200: copied."""
    name = "S11-H96-B4100"                              # (max_batch 4100: n = 200 fits)
    rows = case_inputs(name)[2]
    rng = np.random.default_rng(n)
    eps = rng.standard_normal((n, 3)).astype(np.float32)
    a = ctx_a(name)
    try:
        vec = a.obs_norm_vectors()
        # rows of which some but not all elements are clipped (n = 1 must show both, too)
        hit = np.abs(normalize(rows[0], *vec, CLIP)) == CLIP
        states = rows[0][np.flatnonzero(hit.any(axis=1) & ~hit.all(axis=1))[:n]]
        assert len(states) == n
        got = [a.act(states, True), a.act(states, False, eps), a.act(states, True)]
    finally:
        a.close()
    y = normalize(states, *vec, CLIP)
    assert (np.abs(y) == CLIP).any() and not (np.abs(y) == CLIP).all()
    b = ctx_b(name, vec)
    try:
        want = [b.act(y, True), b.act(y, False, eps), b.act(y, True)]
        raw = b.act(states, True)
    finally:
        b.close()
    for g, w in zip(got, want):
        assert np.array_equal(bits(g), bits(w))
    assert not np.array_equal(bits(got[0]), bits(raw))


# ---------------------------------------------------------------------------------------------
# 7. NaN, 8. refusals
def test_nan_observation_still_raises():
    name = "S11-H96-B40"
    S, H, B, dt, n, kind, seed = CASES[name]
    cfg, _, rows, idx, eps, mom = case_inputs(name)
    s = rows[0].copy()
    s[idx[0][3], 4] = np.nan
    ctx = new_ctx(name)
    try:
        ctx.set_obs_norm(2, EPS, CLIP)
        ctx.set_obs_norm_moments(mom.count, mom.mean, mom.m2)
        ctx.push(s, *rows[1:])
        with pytest.raises(ValueError):
            ctx.step(B, idx[0], eps[0], eps[1])
    finally:
        ctx.close()


def test_refusals():
    from sacmi import _lib as L
    name = "S11-H96-B40"
    S, H, B, dt, n, kind, seed = CASES[name]
    cfg = case_inputs(name)[0]
    a = ctx_a(name, mode=1)
    try:
        before = ctx_state(a, cfg)
        calls = [lambda: a.step_phase(B, 0), lambda: a.step_phase(B, 1, 1.0, 1, False, False)]
        for f in calls:
            with pytest.raises(L.SacmiError, match=f"sacmi error {L.SACMI_ESTATE}"):
                f()
        a.set_obs_norm(0, EPS, CLIP)
        a.dp_loopback_init(2)
        a.set_obs_norm(1, EPS, CLIP)
        with pytest.raises(L.SacmiError, match=f"sacmi error {L.SACMI_ESTATE}"):
            a.step_dp(B, 1)
        with pytest.raises(L.SacmiError, match="observation normalisation is on"):
            a.profile_timeline(B, 1, data_parallel=True)   # (the sequence step_dp would replay)
        after = ctx_state(a, cfg)
        for k in before:
            assert np.array_equal(bits(before[k]), bits(after[k])), k
        ok = np.ones(S)
        for bad in (lambda: a.set_obs_norm(1, -1e-8, 10.0), lambda: a.set_obs_norm(1, math.nan, 10.0),
                    lambda: a.set_obs_norm(1, math.inf, 10.0),
                    lambda: a.set_obs_norm(1, EPS, 0.0), lambda: a.set_obs_norm(1, EPS, -1.0),
                    lambda: a.set_obs_norm(1, EPS, math.nan), lambda: a.set_obs_norm(3, EPS, 10.0),
                    lambda: a.set_obs_norm_moments(-1.0, ok, ok),
                    lambda: a.set_obs_norm_moments(5.0, ok, -ok),
                    lambda: a.set_obs_norm_moments(5.0, ok * math.nan, ok),
                    lambda: a.set_obs_norm_moments(5.0, np.ones(S + 1), np.ones(S + 1))):
            with pytest.raises(ValueError):
                bad()
        assert a.obs_norm() == (1, EPS, CLIP)
        a.set_obs_norm(1, EPS, math.inf)               # +inf: no clipping, accepted
        assert a.obs_norm() == (1, EPS, math.inf)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------
# 9. coexistence
def test_with_diagnostics_clipping_and_prioritized_feedback():
    name = "S11-H96-B40-per"
    B = CASES[name][2]
    cfg = case_inputs(name)[0]

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

    a = ctx_a(name)
    try:
        vec = a.obs_norm_vectors()
        ra = run(a)
    finally:
        a.close()
    b = ctx_b(name, vec)
    try:
        rb = run(b)
    finally:
        b.close()
    assert_same(ra, rb, "all four features")
    assert len(ra["losses"]) == 4 and ra["stats"].shape[0] == 4 and ra["gn"].shape[0] == 4
    for k in ("stats", "gn", "prio"):
        assert np.array_equal(bits(ra[k]), bits(rb[k])), k


# ---------------------------------------------------------------------------------------------
# 10. drop-in
def test_drop_in_agent_and_checkpoints(tmp_path):
    from sacmi import SAC
    S, A, n = 11, 3, 80
    x = fixture_rows(S, n + 1, 41)
    rng = np.random.default_rng(9)

    def fill(agent):
        for i in range(n):
            agent.replay_buffer.push(x[i], rng.uniform(-0.4, 0.4, A).astype(np.float32), float(i % 3),
                                     x[i + 1], i % 17 == 0)

    agent = SAC(S, A, 64, capacity=256, max_batch=32, seed=3, normalize_obs=True, obs_clip=5.0)
    fill(agent)
    out = agent.update_parameters(32)
    assert all(math.isfinite(v) for v in out.values())
    st = agent.obs_norm_state()
    assert st["count"] == n
    e_m2, e_mean = moment_errors(st["count"], st["mean"], st["var"] * n, x[:n])
    assert e_m2 <= M2_RTOL and e_mean <= MEAN_RTOL
    act = agent.select_action(x[5], evaluate=True)
    assert act.shape == (A,) and np.all(np.isfinite(act))
    agent.update_obs_norm(x[n:])                       # the terminal observation, by hand
    assert agent.obs_norm_state()["count"] == n + 1
    agent.freeze_obs_norm(True)
    agent.replay_buffer.push(x[0], np.zeros(A, np.float32), 0.0, x[1], False)
    agent.update_parameters(32)
    assert agent.obs_norm_state()["count"] == n + 1
    agent.freeze_obs_norm(False)
    count, mean, m2 = agent._ctx.obs_norm_moments()

    full, nets = str(tmp_path / "full.pt"), str(tmp_path / "nets.pt")
    agent.save_checkpoint(full, 1, 2)
    agent.save(nets)
    assert "obs_norm" in torch.load(nets, weights_only=True)
    want = agent.select_action(x[7], evaluate=True)

    fresh = SAC(S, A, 64, capacity=256, max_batch=32, seed=4, normalize_obs=True, obs_clip=7.0)
    fresh.load_checkpoint(full)                        # (reloads the 81 replay rows: not counted)
    c2, mean2, m22 = fresh._ctx.obs_norm_moments()
    assert c2 == count == n + 1 and len(fresh.replay_buffer) == n + 1
    assert np.array_equal(bits64(mean), bits64(mean2)) and np.array_equal(bits64(m2), bits64(m22))
    assert fresh._ctx.obs_norm() == (1, 1e-8, 5.0)
    assert np.array_equal(bits(fresh.select_action(x[7], evaluate=True)), bits(want))

    other = SAC(S, A, 64, capacity=256, max_batch=32, seed=5, normalize_obs=True)
    other.load(nets)
    c3, mean3, m23 = other._ctx.obs_norm_moments()
    assert c3 == count and np.array_equal(bits64(m2), bits64(m23))

    # a checkpoint without the entry loads and leaves the statistics as they are
    plain = SAC(S, A, 64, capacity=256, max_batch=32, seed=6)
    fill(plain)
    old = str(tmp_path / "plain.pt")
    plain.save_checkpoint(old, 0, 0)
    assert "obs_norm" not in torch.load(old, weights_only=True)
    other.load_checkpoint(old, load_replay_buffer=False)
    c4, _, m24 = other._ctx.obs_norm_moments()
    assert c4 == count and np.array_equal(bits64(m2), bits64(m24))


def test_env_switch_at_creation():
    """SACMI_OBS_NORM=1 at creation: mode 1, eps 1e-8, clip 10 from the first push (how the
    unchanged benchmark runs with the feature on)."""
    name = "S11-H96-B40"
    os.environ["SACMI_OBS_NORM"] = "1"
    try:
        ctx = new_ctx(name)
    finally:
        os.environ.pop("SACMI_OBS_NORM", None)
    try:
        assert ctx.obs_norm() == (1, 1e-8, 10.0)
        ctx.push(*case_inputs(name)[2])
        ctx.step(CASES[name][2])
        assert ctx.obs_norm_moments()[0] == CASES[name][4]
    finally:
        ctx.close()
    ctx = new_ctx(name)
    try:
        assert ctx.obs_norm() == (0, 1e-8, 10.0)
    finally:
        ctx.close()
