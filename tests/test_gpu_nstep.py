"""N-step returns in the replay gather on the GPU (sacmi_set_nstep; csrc/nstep.hip).

Everything is checked by EQUIVALENCE, bit for bit, against the host model (tests/nstep_model.py):
context A has the feature on and holds the raw rows; context B never enabled it and holds, slot
for slot, the rows the model collapses them to — (s_p, a_p, R_p, s2 of p_m, d'_p), the fractional
d' written raw into its done array.  Same parameters, same indices and noise (or the same
generator key and the device's own draw): losses, parameters, targets, Adam moments and the alpha
state must be identical, because the only difference is WHERE the row was made.

The fixture ring (nstep_model.fixture_marks): capacity + 23 rows pushed in chunks of 1 + 17 + rest,
so the ring is full with its head mid-array; episodes of lengths 1..9 ending in a terminal, a
flag-only end, both, or no mark, a stretch of 33 unmarked rows and 5 more up to the newest.  Every
case first asserts that its batch holds a row of each category (nstep_model.CATEGORIES).
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle.sac_step import OracleSAC, SacConfig, init_params, param_shapes, synthetic_rows

from nstep_model import CATEGORIES, Ring, categories, collapsed_rows, fixture_marks
from obs_norm_model import RunningMoments, normalize
from test_gpu_parity import (GRAD_TOL, LOSS_TOL, check_step, ctx_alpha_state, ctx_grads, ctx_state,
                             flat_params, load_params, make_ctx)

pytestmark = pytest.mark.gpu

KEY = (np.arange(624, dtype=np.uint64) * 1812433 % (2 ** 32)).astype(np.uint32)
# the prioritized sampler's stream: chosen on the CPU (oracle.per.sample_from_probs on equal
# priorities) so that the first draw of 40 slots holds a row of every category
KEY_PER = (np.arange(624, dtype=np.uint64) * 1812435 % (2 ** 32)).astype(np.uint32)
GROUPS = ("policy", "q1", "q2")
EXTRA = 23                      # rows pushed beyond the capacity: the ring's head
EPS, CLIP = 1e-8, 1.5           # the observation-normalisation case

# name -> S, H, B, compute dtype, capacity, replay kind, seed, n
CASES = {f"S{S}-H96-B40-n{n}": (S, 96, 40, "fp32", 64, "uniform", 3000 + 10 * S + n, n)
         for S in (11, 12) for n in (2, 3, 5, 32)}
CASES.update({
    "S11-H96-B40-per-n5": (11, 96, 40, "fp32", 64, "per", 3201, 5),
    "S11-H512-B4096-bf16-n3": (11, 512, 4096, "bf16", 4200, "uniform", 3202, 3),
    "S11-H96-B4100-n3": (11, 96, 4100, "fp32", 4200, "uniform", 3203, 3),
})
NORM_CASE = "S11-H96-B40-n3"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def staged_indices(ring, n, gamma, B, rng):
    """B distinct deque positions in random order, one row of every category among them."""
    perm = rng.permutation(ring.length)
    reps = []
    for c in CATEGORIES:
        for p in perm:
            if categories(ring, n, gamma, [p])[c]:
                reps.append(int(p))
                break
    reps = list(dict.fromkeys(reps))
    rest = [int(p) for p in perm if int(p) not in reps]
    idx = np.array(reps + rest[:B - len(reps)], np.int64)
    return idx[rng.permutation(B)]


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    S, H, B, dt, cap, kind, seed, n = CASES[name]
    cfg = SacConfig(S, 3, H)
    params = init_params(cfg, seed, bias_scale=0.05)
    N = cap + EXTRA
    s, a, r, s2, _ = synthetic_rows(cfg, N, seed + 1000, state_scale=0.5)
    d, end = fixture_marks(N)
    ring = Ring(cap).push(r, d, end)
    assert ring.head == EXTRA
    rng = np.random.default_rng(seed + 2000)
    idx = [staged_indices(ring, n, cfg.gamma, B, rng) for _ in range(2)]
    eps = [rng.standard_normal((B, 3)).astype(np.float32) for _ in range(4)]
    return cfg, params, (s, a, r, s2, d), end, ring, idx, eps


def assert_categories(ring, n, gamma, idx, by_slot, what):
    cat = categories(ring, n, gamma, idx, by_slot)
    print(f"{what}: {cat}")
    assert all(cat[c] > 0 for c in CATEGORIES), (what, cat)


def new_ctx(name, **kw):
    S, H, B, dt, cap, kind, seed, n = CASES[name]
    cfg, params = case_inputs(name)[:2]
    ctx = make_ctx(cfg, max_batch=max(B, 128), capacity=cap, seed=5, compute_dtype=dt, replay=kind, **kw)
    load_params(ctx, params)
    ctx.set_mt(0, KEY, 624)
    if kind == "per":
        ctx.set_mt(1, KEY_PER, 624)
    return ctx


def push_chunks(ctx, rows, end=None):
    """1 + 17 + rest: mapped staging, more than its 16 rows, and the 1024-row chunks."""
    N = len(rows[2])
    for lo, hi in ((0, 1), (1, 18), (18, N)):
        part = [x[lo:hi] for x in rows]
        if end is None:
            ctx.push(*part)
        else:
            ctx.push(*part, episode_end=end[lo:hi])


def ctx_a(name, norm=None):
    """Feature on, the raw rows with their flags.  norm: the moments (observation
    normalisation on as well, frozen)."""
    rows, end = case_inputs(name)[2:4]
    ctx = new_ctx(name)
    if norm is not None:
        ctx.set_obs_norm(2, EPS, CLIP)
        ctx.set_obs_norm_moments(norm.count, norm.mean, norm.m2)
    ctx.set_nstep(CASES[name][7])
    push_chunks(ctx, rows, end)
    return ctx


def ctx_b(name, n=None, vec=None):
    """Never enabled: the same slots hold the model's collapsed rows (EXTRA rows that the ring
    evicts first, so head and write position are A's), normalised with `vec` if given."""
    cfg, _, rows, end, ring = case_inputs(name)[:5]
    n = CASES[name][7] if n is None else n
    s, a, r, s2, d = rows
    (cs, ca, cR, cs2, cd), dprime = collapsed_rows(ring, n, cfg.gamma, s, a, s2)
    if vec is not None:
        cs, cs2 = normalize(cs, *vec, CLIP), normalize(cs2, *vec, CLIP)
    ctx = new_ctx(name)
    ctx.push(*[x[:EXTRA] for x in rows])
    ctx.push(cs, ca, cR, cs2, cd)
    slots = (ring.head + np.arange(ring.length)) % ring.capacity
    ctx.debug_set_done(slots, dprime)
    return ctx


def snapshot(ctx, cfg):
    shapes = param_shapes(cfg)
    out = {"state": ctx_state(ctx, cfg), "alpha": ctx_alpha_state(ctx)}
    for slot in ("m", "v"):
        out[slot] = {f"{n}.{k}": v for n in GROUPS for k, v in ctx.get_net(n, slot, shapes[n]).items()}
    return out


def assert_same(a, b, what):
    assert len(a["losses"]) == len(b["losses"])
    for la, lb in zip(a["losses"], b["losses"]):
        assert np.array_equal(bits(la), bits(lb)), (what, "losses", la, lb)
    for part in ("state", "m", "v"):
        for k in a[part]:
            assert np.array_equal(bits(a[part][k]), bits(b[part][k])), (what, part, k)
    assert a["alpha"] == b["alpha"], (what, a["alpha"], b["alpha"])


def differs(a, b):
    return any(not np.array_equal(bits(a["state"][k]), bits(b["state"][k])) for k in a["state"])


def two_updates(ctx, name):
    """Two updates: staged indices and noise, or (prioritized) the device's own draw and noise."""
    S, H, B, dt, cap, kind, seed, n = CASES[name]
    cfg, idx, eps = case_inputs(name)[0], case_inputs(name)[5], case_inputs(name)[6]
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
def raw_off(name):
    """A context that never enabled the feature, on the raw rows: the control."""
    ctx = new_ctx(name)
    try:
        push_chunks(ctx, case_inputs(name)[2])
        return two_updates(ctx, name)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# 1. equivalence
@pytest.mark.parametrize("name", list(CASES))
def test_equivalence(name):
    S, H, B, dt, cap, kind, seed, n = CASES[name]
    cfg, _, rows, end, ring, idx, eps = case_inputs(name)
    a = ctx_a(name)
    try:
        assert a.nstep() == n and not a.ride_possible(B)
        if kind == "per":                               # the device's draw: ring slots
            first = np.asarray(a.step(B), np.float32)
            assert_categories(ring, n, cfg.gamma, a.read_batch(B)[0], True, name)
            second = np.asarray(a.step(B), np.float32)
            ra = snapshot(a, cfg)
            ra["losses"] = [first, second]
        else:
            for u in range(2):
                assert_categories(ring, n, cfg.gamma, idx[u], False, f"{name} update {u}")
            ra = two_updates(a, name)
    finally:
        a.close()
    b = ctx_b(name)
    try:
        rb = two_updates(b, name)
    finally:
        b.close()
    assert all(np.all(np.isfinite(l)) for l in ra["losses"])
    assert_same(ra, rb, name)
    assert differs(ra, raw_off(name)), "the control: a context with the feature off must differ"


def test_equivalence_with_observation_normalisation():
    name = NORM_CASE
    cfg, _, rows, end, ring, idx, eps = case_inputs(name)
    mom = RunningMoments(CASES[name][0], "device").update(rows[0])
    a = ctx_a(name, norm=mom)
    try:
        vec = a.obs_norm_vectors()
        ra = two_updates(a, name)
    finally:
        a.close()
    t = np.abs((rows[0] - vec[0]) * vec[1]) > CLIP
    assert t.any() and not t.all()
    b = ctx_b(name, vec=vec)
    try:
        rb = two_updates(b, name)
    finally:
        b.close()
    assert_same(ra, rb, "n-step + observation normalisation")
    b = ctx_b(name)                                     # collapsed but not normalised: differs
    try:
        assert differs(ra, two_updates(b, name))
    finally:
        b.close()


def test_with_diagnostics_clipping_and_prioritized_feedback():
    name = "S11-H96-B40-per-n5"
    B = CASES[name][2]
    cfg = case_inputs(name)[0]

    def run(ctx):
        ctx.per_set_feedback(True)
        ctx.set_stats(True)
        ctx.set_grad_clip(0.5, 0.5)
        losses = [np.asarray(ctx.step(B), np.float32) for _ in range(2)]
        ctx.step_many_async(B, 2)
        losses += list(ctx.fetch_losses(2))
        out = snapshot(ctx, cfg)
        n = len(ctx)
        out.update(losses=losses, stats=ctx.fetch_stats()[0], gn=ctx.fetch_grad_norms()[0],
                   prio=ctx.per_priorities(), ring=ctx.get_rows(np.arange(n)))
        return out

    a = ctx_a(name)
    try:
        ra = run(a)
    finally:
        a.close()
    b = ctx_b(name)
    try:
        rb = run(b)
    finally:
        b.close()
    assert_same(ra, rb, "n-step + diagnostics + clipping + feedback")
    assert len(ra["losses"]) == 4 and ra["stats"].shape[0] == 4 and ra["gn"].shape[0] == 4
    for k in ("stats", "gn", "prio"):
        assert np.array_equal(bits(ra[k]), bits(rb[k])), k
    # the rings themselves: A still holds the raw rows, B the collapsed ones (s, a agree)
    rows = case_inputs(name)[2]
    for got, want in zip(ra["ring"][:4], [x[EXTRA:] for x in rows[:4]]):
        assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(ra["ring"][0]), bits(rb["ring"][0]))
    assert np.array_equal(bits(ra["ring"][1]), bits(rb["ring"][1]))


# ---------------------------------------------------------------------------------------------
# 2. what the gather left in r[b], d[b]
@pytest.mark.parametrize("name", ["S11-H96-B40-n5", "S11-H96-B40-per-n5"])
def test_read_batch_rd_equals_the_model(name):
    S, H, B, dt, cap, kind, seed, n = CASES[name]
    cfg, ring = case_inputs(name)[0], case_inputs(name)[4]
    a = ctx_a(name)
    try:
        a.step(B)                                       # device-sampled
        idx, _ = a.read_batch(B)
        r, d = a.read_batch_rd(B)
    finally:
        a.close()
    assert_categories(ring, n, cfg.gamma, idx, kind == "per", name)
    m, R, dp, sl = ring.rows(n, cfg.gamma, idx, by_slot=kind == "per")
    assert np.array_equal(bits(r), bits(R)) and np.array_equal(bits(d), bits(dp))
    assert ((dp > 0) & (dp < 1)).any()


# ---------------------------------------------------------------------------------------------
# 3. degenerate
def test_every_row_flagged_is_the_one_step_update():
    name = "S11-H96-B40-n5"
    rows = case_inputs(name)[2]
    ctx = new_ctx(name)
    try:
        ctx.set_nstep(5)
        push_chunks(ctx, rows, np.ones(len(rows[2]), np.uint8))
        res = two_updates(ctx, name)
    finally:
        ctx.close()
    assert_same(res, raw_off(name), "every row flagged")


def test_on_then_off_is_never_enabled_and_n_is_not_in_the_graph_key():
    from sacmi import _lib as L
    name = "S11-H96-B40-n3"
    S, H, B, dt, cap, kind, seed, n = CASES[name]
    cfg, _, rows, end, ring, idx, eps = case_inputs(name)
    counts = {}
    for how in ("never", "on-off"):
        ctx = new_ctx(name)
        try:
            if how == "on-off":
                ctx.set_nstep(3)
                ctx.set_nstep(1)
                assert ctx.nstep() == 1 and ctx.ride_possible(B)
            push_chunks(ctx, rows)
            res = two_updates(ctx, name)
            counts[how] = int(ctx.get_scalar(L.S_GRAPH_COUNT))
        finally:
            ctx.close()
        assert_same(res, raw_off(name), how)
    assert counts["on-off"] == counts["never"], counts
    a = ctx_a(name)
    try:
        a.step(B, idx[0], eps[0], eps[1])
        g = int(a.get_scalar(L.S_GRAPH_COUNT))
        a.set_nstep(5)
        assert a.nstep() == 5
        l5 = np.asarray(a.step(B, idx[1], eps[2], eps[3]), np.float32)
        assert int(a.get_scalar(L.S_GRAPH_COUNT)) == g
        ra = snapshot(a, cfg)
    finally:
        a.close()
    # ... and the second update did run with n = 5: B's ring collapsed with 3, then with 5
    b = ctx_b(name, n=3)
    try:
        b.step(B, idx[0], eps[0], eps[1])
        s, a_, r, s2, d = rows
        (cs, ca, cR, cs2, cd), dprime = collapsed_rows(ring, 5, cfg.gamma, s, a_, s2)
        b.replay_clear()
        b.push(cs, ca, cR, cs2, cd)
        b.debug_set_done(np.arange(ring.length), dprime)
        lb = np.asarray(b.step(B, idx[1], eps[2], eps[3]), np.float32)
        rb = snapshot(b, cfg)
    finally:
        b.close()
    ra["losses"], rb["losses"] = [l5], [lb]
    assert_same(ra, rb, "n changed from 3 to 5")


# ---------------------------------------------------------------------------------------------
# 4. fp64 oracle
def test_update_vs_fp64_oracle_on_the_collapsed_batch():
    """The update on n-step rows against OracleSAC.step on the model's collapsed batch, d' as the
    float done, held to test_gpu_parity's bars for this shape (LOSS_TOL, GRAD_TOL)."""
    name = "S11-H96-B40-n3"
    S, H, B, dt, cap, kind, seed, n = CASES[name]
    cfg, params, rows, end, ring, idx, eps = case_inputs(name)
    s, a_, r, s2, d = rows
    (cs, ca, cR, cs2, cd), dprime = collapsed_rows(ring, n, cfg.gamma, s, a_, s2)
    batch = [cs[idx[0]], ca[idx[0]], cR[idx[0]], cs2[idx[0]], dprime[idx[0]]]
    assert ((dprime[idx[0]] > 0) & (dprime[idx[0]] < 1)).any()
    a = ctx_a(name)
    try:
        lg = a.step(B, idx[0], eps[0], eps[1])
        res = {"gpu": (lg, ctx_state(a, cfg), ctx_grads(a, cfg)), "alpha": ctx_alpha_state(a)}
    finally:
        a.close()
    for tag, dtype in (("o32", torch.float32), ("o64", torch.float64)):
        o = OracleSAC(cfg, params, dtype)
        l = o.step(*batch, eps[0], eps[1])
        res[tag] = (l, o.state(), o.grads_flat())
    assert LOSS_TOL == 1e-5 and GRAD_TOL == 1e-5        # the bars check_step applies
    check_step(res, flat_params(params), "n-step S11-H96-B40 n=3")


# ---------------------------------------------------------------------------------------------
# 5. forms
def many(ctx, cfg, B, how, k=4):
    if how == "many":
        ctx.step_many_async(B, k)
    else:
        for _ in range(k):
            ctx.step_async(B)
    out = snapshot(ctx, cfg)
    out["losses"] = list(ctx.fetch_losses(k))
    assert len(out["losses"]) == k
    return out


def test_multi_update_launch_equals_single_updates_and_b():
    name = "S11-H96-B40-n3"
    B = CASES[name][2]
    cfg = case_inputs(name)[0]
    res = {}
    for how in ("many", "single"):
        a = ctx_a(name)
        try:
            res[how] = many(a, cfg, B, how)
        finally:
            a.close()
    b = ctx_b(name)
    try:
        res["b"] = many(b, cfg, B, "many")
    finally:
        b.close()
    assert_same(res["many"], res["single"], "step_many_async vs four single updates")
    assert_same(res["many"], res["b"], "step_many_async vs B")


def test_update_right_behind_a_one_row_push_twenty_times():
    """The trainer's rhythm: one row, one update.  On, every row takes the chunked path (the push
    mailbox is bypassed) with its flag behind it; the oldest row is evicted each time and the
    rows near the newest grow longer chains, so B's ring is rebuilt from the model every time."""
    name = "S11-H96-B40-n3"
    S, H, B, dt, cap, kind, seed, n = CASES[name]
    cfg, params, rows, end, ring0, _, _ = case_inputs(name)
    s, a_, r, s2, d = rows
    extra = synthetic_rows(cfg, 20, 77, state_scale=0.5)
    xd, xe = fixture_marks(20 + 40)
    xd, xe = xd[:20], xe[:20]
    S_all, A_all, S2_all = (np.concatenate([x, y]) for x, y in ((s, extra[0]), (a_, extra[1]), (s2, extra[3])))
    ring = Ring(cap).push(r, d, end)
    a = ctx_a(name)
    b = new_ctx(name)
    try:
        for k in range(20):
            row = [x[k:k + 1] for x in extra[:4]] + [xd[k:k + 1]]
            a.push(*row, episode_end=xe[k:k + 1])
            a.step_async(B)
            ring.push(extra[2][k:k + 1], xd[k:k + 1], xe[k:k + 1])
            (cs, ca, cR, cs2, cd), dprime = collapsed_rows(ring, n, cfg.gamma, S_all, A_all, S2_all)
            b.replay_clear()
            b.push(cs, ca, cR, cs2, cd)
            b.debug_set_done(np.arange(cap), dprime)
            b.step_async(B)
        ra, rb = snapshot(a, cfg), snapshot(b, cfg)
        ra["losses"], rb["losses"] = list(a.fetch_losses(20)), list(b.fetch_losses(20))
        flags = a.get_episode_ends(np.arange(cap))
    finally:
        a.close()
        b.close()
    assert len(ra["losses"]) == 20
    assert_same(ra, rb, "twenty one-row pushes")
    assert np.array_equal(flags, ring.ep_end[(ring.head + np.arange(cap)) % cap] != 0)


def test_data_parallel_loopback_equals_fused_updates():
    name = "S11-H96-B40-n3"
    B = CASES[name][2]
    cfg = case_inputs(name)[0]
    a = ctx_a(name)
    try:
        a.dp_loopback_init(2)
        a.step_dp(B, 2)
        a.synchronize()
        ra = snapshot(a, cfg)
        ra["losses"] = list(a.fetch_losses(2))
    finally:
        a.close()
    f = ctx_a(name)
    try:
        losses = [np.asarray(f.step(B), np.float32) for _ in range(2)]
        rf = snapshot(f, cfg)
        rf["losses"] = losses
    finally:
        f.close()
    assert_same(ra, rf, "step_dp (loopback, world 2) vs fused updates")
    b = ctx_b(name)
    try:
        losses = [np.asarray(b.step(B), np.float32) for _ in range(2)]
        rb = snapshot(b, cfg)
        rb["losses"] = losses
    finally:
        b.close()
    assert_same(rf, rb, "fused updates vs B")


def test_refusals():
    from sacmi import _lib as L
    name = "S11-H96-B40-n3"
    S, H, B, dt, cap, kind, seed, n = CASES[name]
    rows = case_inputs(name)[2]
    one = [x[:1] for x in rows]
    estate = f"sacmi error {L.SACMI_ESTATE}"
    ctx = new_ctx(name)
    try:
        with pytest.raises(L.SacmiError, match=estate):                 # off: no flags are kept
            ctx.push(*one, episode_end=[1])
        ctx.push(*one)
        with pytest.raises(L.SacmiError, match=estate):
            ctx.mark_episode_end()
        packed = np.zeros((1, 2 * S + 3 + 2), np.float32)
        with pytest.raises(L.SacmiError, match=estate):
            ctx.push_packed(packed, 1, episode_end=[0])
        assert len(ctx) == 1 and not ctx.get_episode_ends([0]).any()
        for bad in (0, 33, -1):
            with pytest.raises(ValueError):
                ctx.set_nstep(bad)
        assert ctx.nstep() == 1
        ctx.set_nstep(3)
        ctx.replay_clear()
        with pytest.raises(L.SacmiError, match=estate):                 # empty replay
            ctx.mark_episode_end()
        push_chunks(ctx, rows)
        with pytest.raises(L.SacmiError, match=estate):                 # no ride while on
            ctx.step_phase(B, 1, 1.0, 1, False, True)
        ctx.set_nstep(32)
        assert ctx.nstep() == 32
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# 6. the flags under pushes past the capacity
def test_flags_after_pushes_over_capacity_and_mark():
    name = "S11-H96-B40-n3"
    cap = CASES[name][4]
    cfg = case_inputs(name)[0]
    N = cap + 5
    rows = synthetic_rows(cfg, N, 91, state_scale=0.5)[:4]
    rng = np.random.default_rng(92)
    d, end = rng.random(N) < 0.1, rng.random(N) < 0.3
    end[-1] = False
    ring = Ring(cap)
    ctx = new_ctx(name)
    try:
        ctx.set_nstep(3)
        for lo, hi in ((0, 1), (1, 18), (18, 40), (40, N)):            # the last chunk wraps
            part = [x[lo:hi] for x in rows] + [d[lo:hi]]
            if lo == 18:
                ctx.push(*part)                                          # a plain push writes 0
                ring.push(rows[2][lo:hi], d[lo:hi])
            else:
                ctx.push(*part, episode_end=end[lo:hi])
                ring.push(rows[2][lo:hi], d[lo:hi], end[lo:hi])
        pos = np.arange(cap)
        want = ring.ep_end[(ring.head + pos) % cap] != 0
        assert want.any() and ring.head == 5
        assert np.array_equal(ctx.get_episode_ends(pos), want)
        assert np.array_equal(ctx.get_episode_ends(pos, by_slot=True), ring.ep_end != 0)
        ctx.mark_episode_end()
        ring.mark_episode_end()
        got = ctx.get_episode_ends(pos, by_slot=True)
        assert np.array_equal(got, ring.ep_end != 0) and got[(ring.wpos - 1) % cap]
        assert got.sum() == want.sum() + 1
        # packed rows carry their flags the same way
        S = cfg.state_dim
        packed = np.concatenate([rows[0][:3], rows[1][:3], rows[2][:3, None], rows[3][:3],
                                 np.zeros((3, 1), np.float32)], axis=1).astype(np.float32)
        ctx.push_packed(np.ascontiguousarray(packed), 3, episode_end=[1, 0, 1])
        ring.push(rows[2][:3], np.zeros(3), [1, 0, 1])
        assert np.array_equal(ctx.get_episode_ends(pos, by_slot=True), ring.ep_end != 0)
        # off and on again: every flag cleared
        ctx.set_nstep(1)
        assert not ctx.get_episode_ends(pos).any()
        ctx.set_nstep(2)
        assert not ctx.get_episode_ends(pos).any()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# 7. drop-in agent, checkpoints, environment switch
def test_drop_in_agent_flags_and_checkpoints(tmp_path):
    from sacmi import SAC
    from sacmi import _lib as L
    import ckpt_fixture as cf
    S, A, N = 11, 3, 90
    cfg = SacConfig(S, A, 64)
    s, a_, r, s2, _ = synthetic_rows(cfg, N, 55, state_scale=0.5)
    d, end = fixture_marks(N)
    first_end = int(np.flatnonzero(end)[0])

    def agent(**kw):
        torch.manual_seed(7)
        return SAC(S, A, 64, capacity=256, max_batch=32, seed=3, **kw)

    def fill(ag, how):
        for i in range(N):
            if how == "push":
                ag.replay_buffer.push(s[i], a_[i], float(r[i]), s2[i], bool(d[i]), bool(end[i]))
            else:
                ag.replay_buffer.push(s[i], a_[i], float(r[i]), s2[i], bool(d[i]))
                if end[i]:
                    if i == first_end:
                        ag.replay_buffer._flush()        # nothing staged: the context's own mark
                    ag.replay_buffer.mark_episode_end()

    with pytest.raises(ValueError):
        agent(n_step=0)
    with pytest.raises(ValueError):
        agent(n_step=33)
    a1, a2 = agent(n_step=3), agent(n_step=3)
    assert a1.n_step == 3
    fill(a1, "push")
    fill(a2, "mark")
    f1, f2 = a1.replay_buffer.episode_ends(), a2.replay_buffer.episode_ends()
    assert np.array_equal(f1, end != 0) and np.array_equal(f2, end != 0) and f1.any()
    assert len(a1.replay_buffer.buffer[0]) == 5          # still the reference's 5-tuples
    out = a1.update_parameters(32)
    assert all(np.isfinite(v) for v in out.values())

    path = str(tmp_path / "ck.pt")
    a1.save_checkpoint(path, 4, 90)
    ck = torch.load(path, weights_only=True)
    assert ck["n_step"] == 3 and "episode_end" in ck["replay_buffer"]
    other = agent()                                      # n_step 1 until the checkpoint says 3
    assert other.n_step == 1
    assert other.load_checkpoint(path) == (4, 90)
    assert other.n_step == 3 and np.array_equal(other.replay_buffer.episode_ends(), f1)
    key, pos = a1._ctx.get_mt(0)
    other._ctx.set_mt(0, key, pos)
    other._ctx.set_scalar(L.S_NOISE_COUNTER, a1._ctx.get_scalar(L.S_NOISE_COUNTER))
    assert a1.update_parameters(32) == other.update_parameters(32)

    # a checkpoint written before this change (no n_step, no flags) still loads: the agent's own
    # n_step stays, the flags are zeros
    del ck["n_step"], ck["replay_buffer"]["episode_end"]
    old = str(tmp_path / "old.pt")
    torch.save(ck, old)
    third = agent(n_step=5)
    third.load_checkpoint(old)
    assert third.n_step == 5 and len(third.replay_buffer) == N
    assert not third.replay_buffer.episode_ends().any()
    # ... and so does the reference's own checkpoint layout
    dims = cf.load_fixture()[1]["bipedal"]["dims"]
    ref = str(tmp_path / "best_model.pt")
    torch.save(cf.rebuild("bipedal"), ref)
    fourth = SAC(dims["S"], dims["A"], hidden_dim=dims["H"], capacity=1000, max_batch=64, n_step=3)
    fourth.load(ref)
    assert fourth.n_step == 3


def test_env_switch_at_creation():
    name = "S11-H96-B40-n3"
    os.environ["SACMI_NSTEP"] = "3"
    try:
        ctx = new_ctx(name)
    finally:
        os.environ.pop("SACMI_NSTEP", None)
    try:
        assert ctx.nstep() == 3
        res = None
        push_chunks(ctx, case_inputs(name)[2], case_inputs(name)[3])
        res = two_updates(ctx, name)
    finally:
        ctx.close()
    a = ctx_a(name)
    try:
        assert_same(res, two_updates(a, name), "SACMI_NSTEP=3 vs set_nstep(3)")
    finally:
        a.close()
    ctx = new_ctx(name)
    try:
        assert ctx.nstep() == 1
    finally:
        ctx.close()
