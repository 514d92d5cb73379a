"""Per-update training diagnostics on the GPU (sacmi_set_stats, csrc/stats.hip): every update
appends one row of twelve statistics, reduced on the device from what its forward passes left
in HBM.  Checked against the model of tests/update_stats_model.py, against the update's own
buffers (dot partials, stored TD errors, losses), and across the update's forms.

Cases: the smallest shapes that reach every path of the reduction and of the head partials —
  S11-A3-H96-B40            k_gemm levels, nparts 3, a batch that is no multiple of 64
  S11-A3-H100-B40-model2    a partial last 32-column block (nparts 4); three hidden layers
  S11-A3-H512-B1056         more than one row per thread in the one-workgroup form
  S11-A3-H256-B4096-fp32    the x6 kernels; four rows per thread
  S11-A3-H512-B4096-bf16    the act16 class
  S11-A3-H96-B4100          staged indices past 4096: the partial + finish pair, five
                            workgroups, the last holding 4 rows
The reduction reads a row's partials 16 bytes wide where nparts is a multiple of 4 (H100, H256,
H512) and by the word elsewhere (H96), eight partials a slot per round.  Two more cases:
  S11-A3-H384-B72           nparts 12: a second round that is half past the row's end
  S11-A3-H128-B4100         the 16-byte form in the partial + finish pair
"""
import functools

import numpy as np
import pytest
import torch

from oracle.sac_step import SacConfig, init_params, synthetic_rows

from test_gpu_parity import BF16_EMU_LOSS_TOL, LOSS_TOL, ctx_state, load_params, make_ctx
from update_stats_model import STAT_NAMES, StatsSAC, stat_scales, stats_row

pytestmark = pytest.mark.gpu

# name -> (S, A, H, B, compute dtype, n_hidden, replay rows, seed)
CASES = {
    "S11-A3-H96-B40": (11, 3, 96, 40, "fp32", 2, 64, 911),
    "S11-A3-H100-B40-model2": (11, 3, 100, 40, "fp32", 3, 64, 912),
    "S11-A3-H512-B1056": (11, 3, 512, 1056, "fp32", 2, 1100, 913),
    "S11-A3-H256-B4096-fp32": (11, 3, 256, 4096, "fp32", 2, 4200, 914),
    "S11-A3-H512-B4096-bf16": (11, 3, 512, 4096, "bf16", 2, 4200, 915),
    "S11-A3-H96-B4100": (11, 3, 96, 4100, "fp32", 2, 4200, 916),
    "S11-A3-H384-B72": (11, 3, 384, 72, "fp32", 2, 96, 917),
    "S11-A3-H128-B4100": (11, 3, 128, 4100, "fp32", 2, 4200, 918),
}
NAMES = list(CASES)
I = {k: i for i, k in enumerate(STAT_NAMES)}
MODELLED = [I[k] for k in ("q1_mean", "q2_mean", "q_target_mean", "td_mean", "td_max", "q_pi_mean",
                           "entropy", "alpha_loss")]
KEY = (np.arange(624, dtype=np.uint64) * 1812433 % (2 ** 32)).astype(np.uint32)


def f32(x):
    return np.float32(x)


def ulp(x):
    return float(np.spacing(np.float32(max(abs(float(x)), 1e-30))))


def case_inputs(name):
    S, A, H, B, dt, nh, n, seed = CASES[name]
    cfg = SacConfig(S, A, H, n_hidden=nh)
    params = init_params(cfg, seed, bias_scale=0.05)
    rows = synthetic_rows(cfg, n, seed + 1000, state_scale=0.5)
    rng = np.random.default_rng(seed + 2000)
    idx = [rng.permutation(n)[:B] for _ in range(2)]
    eps = [rng.standard_normal((B, A)).astype(np.float32) for _ in range(4)]
    return cfg, params, rows, idx, eps


def fresh_ctx(name, stats=True, **kw):
    S, A, H, B, dt, nh, n, seed = CASES[name]
    cfg, params, rows, _, _ = case_inputs(name)
    ctx = make_ctx(cfg, max_batch=B, capacity=n, seed=5, compute_dtype=dt, **kw)
    load_params(ctx, params)
    ctx.push(*rows)
    ctx.set_mt(0, KEY, 624)
    if stats:
        ctx.set_stats(True)
    return ctx


def heads_from_dotp(dotp):
    """[6, B] head values: the fp32 sum of a row's partials in block order."""
    acc = dotp[:, :, 0].astype(np.float32)
    for i in range(1, dotp.shape[2]):
        acc = (acc + dotp[:, :, i]).astype(np.float32)
    return acc


@functools.lru_cache(maxsize=None)
def two_updates(name):
    """Two staged updates of the case with stats on — alpha and log_alpha read before each,
    the first update's dot partials read back — and the model (fp64, fp32) on the first."""
    from sacmi import _lib as L
    S, A, H, B, dt, nh, n, seed = CASES[name]
    cfg, params, rows, idx, eps = case_inputs(name)
    ctx = fresh_ctx(name)
    try:
        assert ctx.stats()
        pre, losses = [], []
        for u in range(2):
            pre.append((f32(ctx.get_scalar(L.S_ALPHA)), f32(ctx.get_scalar(L.S_LOG_ALPHA))))
            losses.append(np.asarray(ctx.step(B, idx[u], eps[2 * u], eps[2 * u + 1]), np.float32))
            if u == 0:
                dotp = ctx.read_backward("dotp", B)
                act16 = ctx.act16(B)
                got1, total1 = ctx.fetch_stats()
        got, total = ctx.fetch_stats()
    finally:
        ctx.close()
    batch = [x[idx[0]] for x in rows]
    kw = dict(bf16_operands=True, bf16_act=act16) if dt == "bf16" else {}
    o64 = StatsSAC(cfg, params, torch.float64).step(*batch, eps[0], eps[1], **kw)
    o32 = StatsSAC(cfg, params, torch.float32).step(*batch, eps[0], eps[1], **kw)
    return dict(cfg=cfg, B=B, dt=dt, pre=pre, losses=losses, dotp=dotp, got1=got1, total1=total1,
                got=got, total=total, batch=batch, o64=o64, o32=o32)


@pytest.mark.parametrize("name", NAMES)
def test_parity_with_fp64(name):
    """Check 1.  BATCH exact; ALPHA / LOG_ALPHA bit-equal to the scalars read before each of
    two updates (alpha has moved off 0.2 by the second); REWARD_MEAN within 1 ulp of the fp64
    mean; the other eight within max(1e-5, 4 e_ref) x scale of the model in fp64 (bf16: floor
    1e-4, against the model with the bf16 roundings), e_ref the fp32 model's own error.
    Measured worst ratio |gpu - fp64| / scale (MI355X), statistic, and its bar:
      S11-A3-H96-B40 5.6e-8 (entropy, 1.0e-5); S11-A3-H100-B40-model2 1.2e-7 (td_max, 1.0e-5);
      S11-A3-H512-B1056 5.7e-8 (entropy, 1.0e-5); S11-A3-H256-B4096-fp32 6.8e-8 (td_max,
      1.0e-5); S11-A3-H512-B4096-bf16 1.9e-6 (q_pi_mean, 1.0e-4); S11-A3-H96-B4100 8.5e-8
      (td_max, 1.0e-5); S11-A3-H384-B72 5.3e-8 (entropy, 1.0e-5); S11-A3-H128-B4100 5.1e-8
      (entropy, 1.0e-5)   (DESIGN.md §18).
    The B 4100 case also pins k_gemm's dot partials at hidden 96 on 64-column tiles: a block
    past N used to be stored into the next row's block 0 (q means off by up to 6e-4 x scale)."""
    r = two_updates(name)
    B, got = r["B"], r["got"]
    assert r["total1"] == 1 and r["got1"].shape == (1, 12)
    assert r["total"] == 2 and got.shape == (2, 12) and got.dtype == np.float32
    assert np.array_equal(got[0].view(np.uint32), r["got1"][0].view(np.uint32))
    assert got[0, I["batch"]] == B and got[1, I["batch"]] == B
    for u in range(2):
        a, la = r["pre"][u]
        assert got[u, I["alpha"]].view(np.uint32) == a.view(np.uint32), (u, got[u, I["alpha"]], a)
        assert got[u, I["log_alpha"]].view(np.uint32) == la.view(np.uint32), (u, got[u, I["log_alpha"]], la)
    assert r["pre"][0][0] == f32(0.2) and r["pre"][0][1] == 0.0
    assert r["pre"][1][0] != f32(0.2) and r["pre"][1][1] != 0.0
    rmean = float(np.mean(r["batch"][2].astype(np.float64)))
    assert abs(float(got[0, I["reward_mean"]]) - rmean) <= ulp(rmean), (got[0, I["reward_mean"]], rmean)
    m64, m32, scale = stats_row(r["o64"]), stats_row(r["o32"]), stat_scales(r["o64"])
    floor = BF16_EMU_LOSS_TOL if r["dt"] == "bf16" else 1e-5
    worst = (0.0, None, 0.0)
    bad = {}
    for k in MODELLED:
        e_ref = abs(m32[k] - m64[k]) / scale[k]
        bar = max(floor, 4 * e_ref)
        err = abs(float(got[0, k]) - m64[k]) / scale[k]
        print(f"[stats {name}] {STAT_NAMES[k]:14s} gpu {got[0, k]: .8e} fp64 {m64[k]: .8e} "
              f"err/scale {err:.2e} e_ref {e_ref:.2e} bar {bar:.1e}")
        if err >= worst[0]:
            worst = (err, STAT_NAMES[k], bar)
        if not err <= bar:
            bad[STAT_NAMES[k]] = (err, bar)
    print(f"[stats {name}] worst {worst[0]:.2e} ({worst[1]}, bar {worst[2]:.1e})")
    assert np.all(np.isfinite(got))
    assert not bad, (name, bad)
    assert got[0, I["td_max"]] >= got[0, I["td_mean"]] >= 0


@pytest.mark.parametrize("name", NAMES)
def test_head_means_from_the_dot_partials(name):
    """Check 2a, no oracle: Q1_MEAN, Q2_MEAN and Q_PI_MEAN within 1 fp32 ulp of the values
    recomputed from the update's dot partials (fp32 sums in block order, fp64 mean) — slots
    0 / 1 and min(4, 5), row-major [B][nparts]."""
    r = two_updates(name)
    q = heads_from_dotp(r["dotp"]).astype(np.float64)
    want = {"q1_mean": q[0].mean(), "q2_mean": q[1].mean(), "q_pi_mean": np.minimum(q[4], q[5]).mean()}
    for k, w in want.items():
        g = float(r["got1"][0, I[k]])
        print(f"[stats {name}] {k} gpu {g:.9e} numpy {w:.9e} diff/ulp {abs(g - w) / ulp(w):.2f}")
        assert abs(g - w) <= ulp(w), (name, k, g, w)
    # (the slots are distinguishable: a swapped slot would not pass)
    assert abs(want["q1_mean"] - want["q2_mean"]) > 4 * ulp(want["q1_mean"])
    assert abs(want["q_pi_mean"] - np.minimum(q[0], q[1]).mean()) > 4 * ulp(want["q_pi_mean"])


@pytest.mark.parametrize("name", NAMES)
def test_policy_loss_from_the_row(name):
    """Check 3: the policy loss the update returned against -ALPHA ENTROPY - Q_PI_MEAN of its
    row, to the loss tolerance 1e-5 (floor 1e-3) — both updates."""
    r = two_updates(name)
    for u in range(2):
        row = r["got"][u].astype(np.float64)
        want = -row[I["alpha"]] * row[I["entropy"]] - row[I["q_pi_mean"]]
        pl = float(r["losses"][u][2])
        err = abs(pl - want) / max(abs(pl), 1e-3)
        print(f"[stats {name}] update {u} policy_loss {pl:.8e} from the row {want:.8e} err {err:.2e}")
        assert err <= LOSS_TOL, (name, u, pl, want, err)


@pytest.mark.parametrize("B,H,n,dt", [(40, 96, 40, "fp32"), (1056, 512, 1056, "fp32")])
def test_td_against_the_stored_td_in_feedback_mode(B, H, n, dt):
    """Check 2b: prioritized replay with feedback — TD_MEAN / TD_MAX (unweighted) against the
    mean / max of the TD errors the critic row prologue stored for the write-back, within
    1e-5 x scale (the floor of check 1's bar), scale = mean (max) over rows of |q1| + |q2| +
    |q^| from the dot partials."""
    cfg = SacConfig(11, 3, H)
    params = init_params(cfg, 921, bias_scale=0.05)
    rows = synthetic_rows(cfg, n, 922, state_scale=0.5)
    rng = np.random.default_rng(923)
    ctx = make_ctx(cfg, max_batch=B, capacity=n, replay="per", compute_dtype=dt, seed=5)
    try:
        load_params(ctx, params)
        ctx.push(*rows)
        ctx.per_set_priorities((10.0 ** rng.uniform(-1, 1, n)).astype(np.float32))
        ctx.per_set_feedback(True)
        ctx.set_stats(True)
        ctx.step(B)
        w, td, _ = ctx.read_per_feedback(B)
        q = heads_from_dotp(ctx.read_backward("dotp", B)).astype(np.float64)
        got, total = ctx.fetch_stats()
    finally:
        ctx.close()
    assert total == 1 and w.min() < 0.9          # the weights are not all one
    # (|q1| + |q2| alone: no larger than the model's |q1| + |q2| + |q^|, so the bar is no wider)
    rows_scale = np.abs(q[0]) + np.abs(q[1])
    tdm, tdx = float(td.astype(np.float64).mean()), float(td.max())
    e_mean = abs(float(got[0, I["td_mean"]]) - tdm) / rows_scale.mean()
    e_max = abs(float(got[0, I["td_max"]]) - tdx) / rows_scale.max()
    print(f"[stats feedback B{B}] td_mean err/scale {e_mean:.2e} td_max err/scale {e_max:.2e}")
    assert e_mean <= 1e-5 and e_max <= 1e-5, (e_mean, e_max)


def _per_ctx(B, H, n, stats=True):
    cfg = SacConfig(11, 3, H)
    params = init_params(cfg, 931, bias_scale=0.05)
    rows = synthetic_rows(cfg, n, 932, state_scale=0.5)
    ctx = make_ctx(cfg, max_batch=B, capacity=n, replay="per", seed=5)
    load_params(ctx, params)
    ctx.push(*rows)
    ctx.per_set_priorities((10.0 ** np.random.default_rng(933).uniform(-1, 1, n)).astype(np.float32))
    np.random.seed(934)
    st = np.random.get_state()
    ctx.set_mt(1, st[1], st[2])
    ctx.per_set_feedback(True)
    if stats:
        ctx.set_stats(True)
    return ctx


@pytest.mark.parametrize("kind", ["uniform-B40", "per-feedback-B4096"])
def test_one_launch_equals_n_launches(kind):
    """Check 4: step_many_async(B, 3) appends three rows, bit-equal to three step_async on a
    twin (uniform B 40: parity sets and ride-along sampling; prioritized feedback B 4096: the
    side stream) — and a repeat of the launch from the same state gives the same bits."""
    if kind == "uniform-B40":
        B, make = 40, lambda: fresh_ctx("S11-A3-H96-B40")
    else:
        B, make = 4096, lambda: _per_ctx(4096, 256, 4096)
    a, b, c = make(), make(), make()
    try:
        a.step_many_async(B, 3)
        c.step_many_async(B, 3)
        for _ in range(3):
            b.step_async(B)
        ra, ta = a.fetch_stats()
        rb, tb = b.fetch_stats()
        rc, tc = c.fetch_stats()
        la, lb = a.fetch_losses(8), b.fetch_losses(8)
    finally:
        for x in (a, b, c):
            x.close()
    assert ta == tb == tc == 3 and ra.shape == rb.shape == rc.shape == (3, 12)
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32))
    assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32)), (ra, rb)
    assert np.array_equal(ra.view(np.uint32), rc.view(np.uint32))
    assert np.all(np.isfinite(ra)) and np.all(ra[:, I["batch"]] == B)
    # three different minibatches, alpha moving
    assert len({float(x) for x in ra[:, I["reward_mean"]]}) == 3
    assert len({float(x) for x in ra[:, I["alpha"]]}) == 3


@pytest.mark.parametrize("sharded", [False, True])
def test_data_parallel_rows(sharded):
    """Check 5: step_dp(B, 2) on the two-rank loopback appends the rank's own minibatch's
    rows, bit-equal to the fused updates' on a twin, in the all-reduce and the sharded form."""
    name = "S11-A3-H96-B40"
    B = CASES[name][3]
    a, b = fresh_ctx(name), fresh_ctx(name)
    try:
        a.dp_loopback_init(2)
        a.dp_set_sharded(sharded)
        assert a.dp_sharded() == sharded
        a.step_dp(B, 2)
        fused = np.stack([b.step(B) for _ in range(2)])
        ra, ta = a.fetch_stats()
        rb, tb = b.fetch_stats()
        assert np.array_equal(a.fetch_losses(2), fused)
    finally:
        a.close()
        b.close()
    assert ta == tb == 2
    assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32)), (ra, rb)
    assert ra[1, I["alpha"]] != ra[0, I["alpha"]]


def test_off_means_off():
    """Check 6: stats off — the launch timeline of a context that had them on and off again is
    that of one that never heard of them, and nothing is appended; on, the timeline has
    exactly two more kernels (one per update), k_update_stats at site update_stats, one
    workgroup each, behind the update's last L8 level and before its L13; losses and every
    parameter after three updates are bit-equal on and off; toggling captures one more graph,
    toggling back none."""
    from sacmi import _lib as L
    name = "S11-A3-H96-B40"
    B = CASES[name][3]
    cfg, _, _, idx, eps = case_inputs(name)
    never, onoff, on = fresh_ctx(name, stats=False), fresh_ctx(name), fresh_ctx(name)
    try:
        onoff.set_stats(False)
        assert not never.stats() and not onoff.stats() and on.stats()
        lists = []
        for c in (never, onoff, on):
            ks, _ = c.profile_timeline(B, 2)
            lists.append(ks)
        sig = lambda ks: [(k["site"], k["kernel"], k["grid"]) for k in ks]
        assert sig(lists[0]) == sig(lists[1])
        assert not [k for k in lists[0] if k["site"] == "update_stats" or k["kernel"] == "k_update_stats"]
        extra = [k for k in lists[2] if k["site"] == "update_stats"]
        assert [(k["kernel"], k["grid"]) for k in extra] == [("k_update_stats", 1)] * 2
        assert sorted(sig(lists[0])) == sorted(x for x in sig(lists[2]) if x[0] != "update_stats")
        assert len(lists[2]) == len(lists[0]) + 2
        l8 = [k for k in lists[2] if k["site"] == "gemm_L8_act_fc2"]
        l13 = [k for k in lists[2] if k["site"] == "gemm_L13_pi_dW_adam"]
        for u in range(2):
            assert l8[u]["end_us"] <= extra[u]["start_us"] <= extra[u]["end_us"] <= l13[u]["start_us"], u
        assert "update_stats" in [s[0] for s in on.profile_step(B, 1)]
        assert "update_stats" not in [s[0] for s in never.profile_step(B, 1)]
        assert never.fetch_stats()[1] == 0 and onoff.fetch_stats()[0].shape == (0, 12)
        assert onoff.fetch_stats()[1] == 0
    finally:
        for c in (never, onoff, on):
            c.close()
    off, on = fresh_ctx(name, stats=False), fresh_ctx(name)
    try:
        for c in (off, on):
            for _ in range(3):
                c.step_async(B)
        lo, ln = off.fetch_losses(8), on.fetch_losses(8)
        assert lo.shape == (3, 3) and np.array_equal(lo.view(np.uint32), ln.view(np.uint32))
        so, sn = ctx_state(off, cfg), ctx_state(on, cfg)
        for k in so:
            assert np.array_equal(so[k].view(np.uint32), sn[k].view(np.uint32)), k
        assert off.fetch_stats()[1] == 0 and on.fetch_stats()[1] == 3
        # staged updates (no batch drawn ahead: one graph per form)
        g0 = int(off.get_scalar(L.S_GRAPH_COUNT))
        off.step(B, idx[0], eps[0], eps[1])
        g1 = int(off.get_scalar(L.S_GRAPH_COUNT))
        off.set_stats(True)
        off.step(B, idx[0], eps[0], eps[1])
        g2 = int(off.get_scalar(L.S_GRAPH_COUNT))
        off.set_stats(False)
        off.step(B, idx[0], eps[0], eps[1])
        off.set_stats(True)
        off.step(B, idx[0], eps[0], eps[1])
        g3 = int(off.get_scalar(L.S_GRAPH_COUNT))
        assert g1 == g0 + 1 and g2 == g1 + 1 and g3 == g2, (g0, g1, g2, g3)
        assert off.fetch_stats()[1] == 2
    finally:
        off.close()
        on.close()


def test_voided_update_appends_nothing():
    """Check 7: a NaN policy head weight (finite inputs) — the update raises ValueError and the
    row count stays; the weight restored, the next update appends one row."""
    name = "S11-A3-H96-B40"
    B = CASES[name][3]
    _, _, _, idx, eps = case_inputs(name)
    ctx = fresh_ctx(name)
    try:
        ctx.step(B, idx[0], eps[0], eps[1])
        rows0, total0 = ctx.fetch_stats()
        assert total0 == 1
        good = ctx.get_net("policy")
        bad = {k: v.copy() for k, v in good.items()}
        bad["mean.weight"].reshape(-1)[0] = np.nan
        ctx.set_net("policy", bad)
        with pytest.raises(ValueError):
            ctx.step(B, idx[1], eps[2], eps[3])
        rows1, total1 = ctx.fetch_stats()
        assert total1 == 1 and np.array_equal(rows1.view(np.uint32), rows0.view(np.uint32))
        ctx.step_many_async(B, 3)                  # (device-sampled: voided all the same)
        with pytest.raises(ValueError):
            ctx.fetch_losses(8)
        assert ctx.fetch_stats()[1] == 1
        ctx.set_net("policy", good)
        ctx.step(B, idx[1], eps[2], eps[3])
        rows2, total2 = ctx.fetch_stats()
        assert total2 == 2 and rows2.shape == (2, 12) and np.all(np.isfinite(rows2))
        assert np.array_equal(rows2[0].view(np.uint32), rows0[0].view(np.uint32))
    finally:
        ctx.close()


def test_ring_wrap():
    """Check 8: 4100 async updates in launches of 256 (and one of 4): total 4100, the 4096
    most recent rows come back oldest first — the rows fetched before the last four updates,
    shifted by four — and the last row is the row max_rows = 1 fetches."""
    name = "S11-A3-H96-B40"
    B = CASES[name][3]
    ctx = fresh_ctx(name)
    try:
        for _ in range(16):
            ctx.step_many_async(B, 256)
        before, t0 = ctx.fetch_stats()
        ctx.step_many_async(B, 4)
        rows, total = ctx.fetch_stats()
        last, t1 = ctx.fetch_stats(1)
        few, _ = ctx.fetch_stats(7)
        ctx.fetch_losses(1)
    finally:
        ctx.close()
    assert t0 == 4096 and before.shape == (4096, 12)
    assert total == t1 == 4100 and rows.shape == (4096, 12) and last.shape == (1, 12)
    assert np.all(np.isfinite(rows)) and np.all(rows[:, I["batch"]] == B)
    assert np.array_equal(rows[:-4].view(np.uint32), before[4:].view(np.uint32))
    assert np.array_equal(rows[-1].view(np.uint32), last[0].view(np.uint32))
    assert np.array_equal(rows[-7:].view(np.uint32), few.view(np.uint32))
    assert not np.array_equal(rows[-1], rows[-2])


def test_env_switch_at_creation():
    """SACMI_STATS=1 at context creation: stats on from the first update (how the cost of
    stats on is measured under the unchanged benchmark); unset, off."""
    import os
    name = "S11-A3-H96-B40"
    B = CASES[name][3]
    os.environ["SACMI_STATS"] = "1"
    try:
        ctx = fresh_ctx(name, stats=False)
    finally:
        os.environ.pop("SACMI_STATS", None)
    try:
        assert ctx.stats()
        ctx.step(B)
        assert ctx.fetch_stats()[1] == 1
    finally:
        ctx.close()
    ctx = fresh_ctx(name, stats=False)
    try:
        assert not ctx.stats()
    finally:
        ctx.close()


def test_agent_surface():
    """Check 9: SAC(..., diagnostics=True).fetch_diagnostics() returns dicts keyed by
    STAT_NAMES, oldest first; a default agent returns [] and update_parameters' keys are the
    reference's three."""
    from sacmi import SAC, STAT_NAMES as NAMES_PUBLIC
    assert NAMES_PUBLIC == STAT_NAMES
    cfg = SacConfig(11, 3, 96)
    rows = synthetic_rows(cfg, 48, 9, state_scale=0.5)
    for diag in (True, False):
        agent = SAC(11, 3, hidden_dim=96, capacity=64, max_batch=40, seed=5,
                    **(dict(diagnostics=True) if diag else {}))
        try:
            for i in range(48):
                agent.replay_buffer.push(rows[0][i], rows[1][i], float(rows[2][i]), rows[3][i], bool(rows[4][i]))
            out = agent.update_parameters(40)
            assert set(out) == {"q1_loss", "q2_loss", "policy_loss"}
            agent.update_parameters_many(40, 2)
            d = agent.fetch_diagnostics()
            if not diag:
                assert d == [] and not agent._ctx.stats()
                continue
            assert len(d) == 3 and all(tuple(x) == STAT_NAMES for x in d)
            assert all(x["batch"] == 40.0 and np.isfinite(list(x.values())).all() for x in d)
            assert d[0]["alpha"] == float(np.float32(0.2)) and d[2]["alpha"] != d[0]["alpha"]
            err = abs(out["policy_loss"] - (-d[0]["alpha"] * d[0]["entropy"] - d[0]["q_pi_mean"]))
            assert err <= LOSS_TOL * max(abs(out["policy_loss"]), 1e-3)
            assert len(agent.fetch_diagnostics(max_rows=2)) == 2
            assert agent.fetch_diagnostics(max_rows=1)[0] == d[-1]
        finally:
            agent._ctx.close()
