"""Prioritized replay with feedback on the GPU (sacmi_per_set_feedback): the critic row prologue
carries the draw's importance-sampling weights, leaves the rows' TD errors, and
k_per_feedback writes them back as priorities inside the update.  Checked against the host
loop of tests/per_feedback_model.py.

Cases: the smallest shapes that reach each consumer of the row prologue's arithmetic
(rows_coef) on the critic level L5 —
  S11-A3-H96-B40            k_gemm, the spread form (32x32 one-wave-group tiles)
  S11-A3-H512-B1056         k_gemm, the 64-row rows_load / rows_finish form (its weighted
                            instantiation)
  S11-A3-H256-B4096 fp32    k_axk_x6 (512 64x64 tiles over the two critics)
  S11-A3-H512-B4096 bf16    k_axk16 (the act16 class)
Every case fills the replay with exactly B rows — the library's population check (and the
reference's sample(), which draws min(B, len)) allows no replay shorter than the batch — whose
priorities are a seeded spread over two decades: B draws with replacement from B rows then
repeat rows (asserted on the draw), and the weights are far from 1 (asserted on the model:
the weighted and unweighted q losses differ by more than 1e-2 relative).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import per as P
from oracle.pyrandom import MT19937
from oracle.sac_step import NETS, SacConfig, init_params, synthetic_rows

from per_feedback_model import FeedbackSAC, stored_priorities
from test_gpu_parity import (BF16_EMU_GRAD_TOL, BF16_EMU_LOSS_TOL, FLIP_Z_TOL, GRAD_TOL, LOSS_TOL,
                             MASKED_GRAD_TOL, ctx_grads, ctx_state, gpu_relu_masks, load_params,
                             make_ctx, rel)

pytestmark = pytest.mark.gpu

# name -> (S, A, H, B, compute dtype, L5's kernel, L5's grid, seed)
#   grids: 2 descs x 6 32x32 tiles, each padded to 8 workgroups; 2 x 136 64x64 tiles;
#   2 x 64 x 4 64x64 tiles; 2 x 256 tiles (64 row blocks x 4 column blocks of 128)
CASES = {
    "S11-A3-H96-B40": (11, 3, 96, 40, "fp32", "k_gemm", 16, 811),
    "S11-A3-H512-B1056": (11, 3, 512, 1056, "fp32", "k_gemm", 272, 812),
    "S11-A3-H256-B4096-fp32": (11, 3, 256, 4096, "fp32", "k_axk_x6", 512, 813),
    "S11-A3-H512-B4096-bf16": (11, 3, 512, 4096, "bf16", "k_axk16", 512, 814),
}
NAMES = sorted(CASES)
LOSS_KEYS = ("q1_loss", "q2_loss", "policy_loss")


def case_inputs(name):
    S, A, H, B, dt, _, _, seed = CASES[name]
    cfg = SacConfig(S, A, H)
    params = init_params(cfg, seed, bias_scale=0.05)
    rows = synthetic_rows(cfg, B, seed + 1000, state_scale=0.5)
    rng = np.random.default_rng(seed + 2000)
    prios = (10.0 ** rng.uniform(-1.0, 1.0, B)).astype(np.float32)
    e1 = rng.standard_normal((B, A)).astype(np.float32)
    e2 = rng.standard_normal((B, A)).astype(np.float32)
    np.random.seed(seed)
    return cfg, params, rows, prios, np.random.get_state(), e1, e2


def fresh_ctx(name, feedback=True):
    """A prioritized context of the case: B rows, the spread priorities, the seeded numpy-MT
    stream, feedback on or off."""
    S, A, H, B, dt, *_ = CASES[name]
    cfg, params, rows, prios, st, _, _ = case_inputs(name)
    ctx = make_ctx(cfg, max_batch=B, capacity=B, replay="per", compute_dtype=dt)
    load_params(ctx, params)
    ctx.push(*rows)
    ctx.per_set_priorities(prios)
    ctx.set_mt(1, st[1], st[2])
    if feedback:
        ctx.per_set_feedback(True)
    return ctx


def frame_of(ctx):
    from sacmi import _lib as L
    return int(ctx.get_scalar(L.S_PER_FRAME))


def step_with_flip_evidence(model, batch, e1, e2, w, kw):
    """model.step_weighted under kw, and (forced masks: test_gpu_parity.flip_evidence's measure,
    here on the weighted update — the actor pass runs on the critics the weighted step left)
    the largest |pre-activation| of a ReLU decision the masks take differently from the model,
    relative to its layer's largest |pre-activation|."""
    import oracle.sac_step as osm
    masks = kw.get("masks") or {}
    orig, zrel, flips = osm._relu, [0.0], {}
    def spy(x, tag, i):
        if tag and (tag, i) in masks:
            z = x.detach().numpy()
            f = (z > 0) != (masks[(tag, i)] > 0)
            flips[f"{tag}.{i}"] = int(f.sum())
            if f.any():
                zrel[0] = max(zrel[0], float(np.abs(z[f]).max() / max(np.abs(z).max(), 1e-30)))
        return orig(x, tag, i)
    osm._relu = spy
    try:
        out = model.step_weighted(*batch, e1, e2, w, **kw)
    finally:
        osm._relu = orig
    if masks:
        print("ReLU decisions the GPU took differently from fp64:", {k: n for k, n in flips.items() if n},
              f"largest |z| of a flip / layer max: {zrel[0]:.2e}")
    return out, zrel[0]


@functools.lru_cache(maxsize=None)
def one_update(name):
    """One feedback update of the case with injected eps, everything it left read back through
    the hooks, then its launch timeline; and the model on the same batch and weights."""
    S, A, H, B, dt, *_ = CASES[name]
    cfg, params, rows, prios, st, e1, e2 = case_inputs(name)
    ctx = fresh_ctx(name)
    try:
        assert ctx.per_feedback()
        frame0 = frame_of(ctx)
        lg = np.asarray(ctx.step(B, eps1=e1, eps2=e2), np.float32)
        gg = ctx_grads(ctx, cfg)
        idx, _ = ctx.read_batch(B)
        w, td, pv = ctx.read_per_feedback(B)
        after = ctx.per_priorities()
        masks = gpu_relu_masks(ctx, cfg, B) if B >= 4096 and dt == "fp32" else None
        act16 = ctx.act16(B)
        key, pos = ctx.get_mt(1)
        frame1 = frame_of(ctx)
        ks, _ = ctx.profile_timeline(B, 1)
    finally:
        ctx.close()
    batch = [x[idx] for x in rows]
    kw = dict(bf16_operands=True, bf16_act=act16) if dt == "bf16" else dict(masks=masks)
    m64 = FeedbackSAC(cfg, params, torch.float64)
    o64, zmax = step_with_flip_evidence(m64, batch, e1, e2, w, kw)
    m32 = FeedbackSAC(cfg, params, torch.float32)
    o32 = m32.step_weighted(*batch, e1, e2, w, **kw)
    return dict(cfg=cfg, params=params, rows=rows, prios=prios, st=st, e1=e1, e2=e2, lg=lg, gg=gg,
                idx=idx, w=w, td=td, pv=pv, after=after, masks=masks, act16=act16, mt=(key, pos),
                frames=(frame0, frame1), ks=ks, o64=o64, zmax=zmax, g64=m64.grads_flat(), o32=o32, batch=batch)


@pytest.mark.parametrize("name", NAMES)
def test_l5_kernel_and_grid(name):
    """The case reaches the consumer of rows_coef it is there for (the launch timeline's kernel
    and grid of L5), and the write-back is one launch of one workgroup, the update's last."""
    r = one_update(name)
    *_, kern, grid, _ = CASES[name]
    l5 = {(k["kernel"], k["grid"]) for k in r["ks"] if k["site"] == "gemm_L5_critic_dh1"}
    print(f"\n[feedback {name}] L5 {l5}")
    assert l5 == {(kern, grid)}, (name, l5)
    fb = [(k["kernel"], k["grid"]) for k in r["ks"] if k["site"] == "per_feedback"]
    assert fb == [("k_per_feedback", 1)], fb
    start = [k["start_us"] for k in r["ks"] if k["site"] == "per_feedback"][0]
    assert start == max(k["start_us"] for k in r["ks"])


@pytest.mark.parametrize("name", NAMES)
def test_weighted_update_vs_fp64(name):
    """Check 4: one weighted update against the model in fp64 on the batch and weights the
    update used.  Batch <= 1056: losses within LOSS_TOL, every gradient tensor within GRAD_TOL
    normwise.  Batch 4096 fp32: fp64 under the GPU's own ReLU masks (every flipped decision
    within FLIP_Z_TOL of zero), gradients within MASKED_GRAD_TOL; bf16: against the model with
    the bf16 operand roundings, at BF16_EMU_LOSS_TOL / BF16_EMU_GRAD_TOL."""
    r = one_update(name)
    B, dt = CASES[name][3], CASES[name][4]
    o64 = r["o64"]
    # the inputs cannot hide a missing weight: weighted and unweighted q losses far apart
    for k in ("q1_loss", "q2_loss"):
        gap = abs(o64[k] - o64[k + "_unweighted"]) / abs(o64[k + "_unweighted"])
        assert gap > 1e-2, (name, k, gap)
    assert len(np.unique(r["idx"])) < B
    if dt == "bf16":
        ltol, lfloor, gtol = BF16_EMU_LOSS_TOL, 1e-2, BF16_EMU_GRAD_TOL
    else:
        ltol, lfloor, gtol = LOSS_TOL, 1e-3, (GRAD_TOL if B <= 1056 else MASKED_GRAD_TOL)
    if r["masks"] is not None:
        assert r["zmax"] <= FLIP_Z_TOL, ("a flipped ReLU decision away from zero", r["zmax"])
    lerr = {k: abs(r["lg"][i] - o64[k]) / max(abs(o64[k]), lfloor) for i, k in enumerate(LOSS_KEYS)}
    errs = {k: rel(r["gg"][k], v) for k, v in r["g64"].items() if dt != "bf16" or k != "log_alpha"}
    unw = {k: abs(r["lg"][i] - o64[k + "_unweighted"]) / abs(o64[k + "_unweighted"])
           for i, k in enumerate(LOSS_KEYS[:2])}
    print(f"\n[feedback {name}] loss err {lerr} (vs the unweighted loss: {unw}) "
          f"worst grad {max(errs.items(), key=lambda kv: kv[1])}")
    assert all(e <= ltol for e in lerr.values()), (name, lerr)
    over = {k: e for k, e in errs.items() if e > gtol}
    assert not over, (name, over)


@pytest.mark.parametrize("name", NAMES)
def test_td_vs_fp64(name):
    """Check 5: the rows' TD errors against fp64, per row on the row's own scale
    |q1| + |q2| + |q^|, at max(1e-5, 4 e_ref) with e_ref the fp32 model's own worst error
    against fp64 on the same inputs.  Measured worst (MI355X): 4.0e-6 at B 40 (bar 1.0e-5), 1.8e-6
    at B 1056 (8.1e-5), 1.7e-6 at B 4096 fp32 (6.7e-5), 5.0e-5 at B 4096 bf16 against the bf16
    emulation (e_ref 5.0e-5, bar 2.0e-4)
    (DESIGN.md §0, §17)."""
    r = one_update(name)
    scale = np.maximum(r["o64"]["td_scale"], 1e-30)
    t64 = r["o64"]["td"]
    e_ref = float(np.max(np.abs(r["o32"]["td"].astype(np.float64) - t64) / scale))
    err = np.abs(r["td"].astype(np.float64) - t64) / scale
    bar = max(1e-5, 4 * e_ref)
    print(f"\n[feedback {name}] td worst {err.max():.3e} (row {int(err.argmax())}), e_ref {e_ref:.3e}, bar {bar:.3e}")
    assert np.all(np.isfinite(r["td"]))
    assert err.max() <= bar, (name, float(err.max()), bar)


@pytest.mark.parametrize("name", NAMES)
def test_write_back_exact(name):
    """Check 6: the whole priority array after the update is, bit for bit, oracle.per's
    update_priorities on the GPU's own td (last duplicate wins, unsampled rows untouched);
    the stored values are float32(float64(td) + 1e-6)."""
    r = one_update(name)
    B = CASES[name][3]
    assert len(np.unique(r["idx"])) < B                      # duplicates are in the draw
    assert len(np.unique(r["idx"])) > B // 4
    want = P.update_priorities(r["prios"], r["idx"], r["td"])
    assert np.array_equal(r["after"].view(np.uint32), want.view(np.uint32)), \
        np.flatnonzero(r["after"] != want)[:8]
    assert np.array_equal(r["pv"].view(np.uint32), stored_priorities(r["td"]).view(np.uint32))
    untouched = np.setdiff1d(np.arange(B), r["idx"])
    assert untouched.size and np.array_equal(r["after"][untouched], r["prios"][untouched])
    assert not np.array_equal(r["after"], r["prios"])


@pytest.mark.parametrize("name", NAMES)
def test_weights_the_update_used(name):
    """Check 7: the weights (and indices) the update used are bit-identical to sacmi_per_sample's
    on a twin context in the same state, and within 4 ulp of oracle.per's; frame and numpy-MT
    stream moved by exactly one draw."""
    r = one_update(name)
    B = CASES[name][3]
    twin = fresh_ctx(name, feedback=False)
    try:
        tidx, tw = twin.per_sample(B)
        tmt = twin.get_mt(1)
    finally:
        twin.close()
    assert np.array_equal(r["idx"], tidx)
    assert np.array_equal(r["w"].view(np.uint32), tw.view(np.uint32))
    mt = MT19937.from_npstate(r["st"])
    oidx, ow = P.sample_from_probs(P.probs_from(r["prios"], B), B, mt, P.beta_at(r["frames"][0]))
    assert np.array_equal(r["idx"], oidx)
    ulp = np.spacing(np.maximum(np.abs(ow), np.float32(1e-30)))
    assert np.all(np.abs(r["w"] - ow) <= 4 * ulp), float(np.max(np.abs(r["w"] - ow) / ulp))
    assert r["w"].max() == 1.0 and r["w"].min() < 0.5
    assert r["frames"][1] == r["frames"][0] + 1
    assert r["mt"][1] == tmt[1] == mt.pos and np.array_equal(r["mt"][0], tmt[0])
    assert np.array_equal(r["mt"][0], mt.key)


@pytest.mark.parametrize("name", NAMES)
def test_closed_loop_three_updates(name):
    """Check 8: three updates on one context — each draws, exactly, what oracle.per draws from
    the priority array the previous update's write-back (check 6, on the GPU's own td) leaves,
    with the numpy-MT state carried along; frame and MT state at the end are exact."""
    B = CASES[name][3]
    cfg, params, rows, prios, st, _, _ = case_inputs(name)
    mt = MT19937.from_npstate(st)
    ctx = fresh_ctx(name)
    try:
        frame = frame_of(ctx)
        for t in range(3):
            ctx.step(B)
            idx, _ = ctx.read_batch(B)
            _, td, _ = ctx.read_per_feedback(B)
            oidx, _ = P.sample_from_probs(P.probs_from(prios, B), B, mt, P.beta_at(frame))
            frame += 1
            assert np.array_equal(idx, oidx), (name, t)
            prios = P.update_priorities(prios, idx, td)
            assert np.array_equal(ctx.per_priorities().view(np.uint32), prios.view(np.uint32)), (name, t)
        key, pos = ctx.get_mt(1)
        assert frame_of(ctx) == frame
        assert pos == mt.pos and np.array_equal(key, mt.key)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["S11-A3-H96-B40", "S11-A3-H256-B4096-fp32"])
def test_one_launch_equals_n_launches(name):
    """Check 9: step_many_async(B, 5) against five single updates on a twin: losses, every
    parameter, the priority array, the numpy-MT state and the frame, bit for bit — and the
    graph's write-backs sit on the side stream behind L5, not in front of L6.  (Finite td: a
    non-finite one makes the next draw raise, and where that lands inside a graph depends on
    timing — DESIGN.md §17.)"""
    B = CASES[name][3]
    cfg = case_inputs(name)[0]
    a, b = fresh_ctx(name), fresh_ctx(name)
    try:
        a.step_many_async(B, 5)
        for _ in range(5):
            b.step_async(B)
        la, lb = a.fetch_losses(8), b.fetch_losses(8)
        assert la.shape == lb.shape == (5, 3) and np.array_equal(la.view(np.uint32), lb.view(np.uint32))
        sa, sb = ctx_state(a, cfg), ctx_state(b, cfg)
        for k in sa:
            assert np.array_equal(sa[k].view(np.uint32), sb[k].view(np.uint32)), k
        assert np.array_equal(a.per_priorities().view(np.uint32), b.per_priorities().view(np.uint32))
        (ka, pa), (kb, pb) = a.get_mt(1), b.get_mt(1)
        assert pa == pb and np.array_equal(ka, kb)
        assert frame_of(a) == frame_of(b) == 6
        ks, _ = a.profile_timeline(B, 3)
    finally:
        a.close()
        b.close()
    sites = [k["site"] for k in ks]
    assert sites.count("per_feedback") == 3 and sites.count("per_sample_next") == 5 * 2
    # every write-back but the last starts after its update's L5 and before the next update's
    # draw; the next update's L1 starts after that draw's gather
    l5 = [k for k in ks if k["site"] == "gemm_L5_critic_dh1"]
    fb = [k for k in ks if k["site"] == "per_feedback"]
    nxt = [k for k in ks if k["site"] == "per_sample_next" and k["kernel"] == "k_per_f1"]
    gat = [k for k in ks if k["site"] == "gather_next"]
    l1 = [k for k in ks if k["site"] == "gemm_L1_fc1"]
    for u in range(2):
        assert l5[u]["end_us"] <= fb[u]["start_us"] <= fb[u]["end_us"] <= nxt[u]["start_us"], u
        assert gat[u]["end_us"] <= l1[u + 1]["start_us"], u


def test_off_means_off():
    """Check 1: a prioritized context that never enabled feedback — six updates leave every
    priority bit where it was, one captured graph, and a launch timeline without a write-back:
    the feedback-on timeline minus its k_per_feedback launches, kernel for kernel."""
    from sacmi import _lib as L
    name = "S11-A3-H96-B40"
    B = CASES[name][3]
    prios = case_inputs(name)[3]
    off, on = fresh_ctx(name, feedback=False), fresh_ctx(name)
    try:
        assert not off.per_feedback()
        for _ in range(6):
            off.step_async(B)
        off.fetch_losses(8)
        assert np.array_equal(off.per_priorities().view(np.uint32), prios.view(np.uint32))
        assert int(off.get_scalar(L.S_GRAPH_COUNT)) == 1
        lists = []
        for c in (off, on):
            ks, _ = c.profile_timeline(B, 2)
            lists.append([(k["site"], k["kernel"], k["grid"]) for k in ks])
        assert int(off.get_scalar(L.S_GRAPH_COUNT)) == 1       # (the timeline's graph is its own)
        assert not [x for x in lists[0] if x[1] == "k_per_feedback"]
        assert sorted(lists[0]) == sorted(x for x in lists[1] if x[1] != "k_per_feedback")
        assert len(lists[1]) == len(lists[0]) + 2
        # switching it on later is a second graph; the first stays
        off.per_set_feedback(True)
        off.step_async(B)
        off.fetch_losses(8)
        assert int(off.get_scalar(L.S_GRAPH_COUNT)) == 2
        assert not np.array_equal(off.per_priorities(), prios)
    finally:
        off.close()
        on.close()


def _agent(B=40, n=48):
    from sacmi import SAC
    cfg, params, rows, *_ = case_inputs("S11-A3-H96-B40")
    np.random.seed(21)
    st = np.random.get_state()
    agent = SAC(11, 3, hidden_dim=96, capacity=64, max_batch=B, seed=5, prioritized_replay=True)
    key, pos = agent._ctx.get_mt(1)
    assert pos == st[2] and np.array_equal(key, st[1])      # np.random's stream, adopted
    rows = synthetic_rows(cfg, n, 9, state_scale=0.5)
    for i in range(n):
        agent.replay_buffer.push(rows[0][i], rows[1][i], float(rows[2][i]), rows[3][i], bool(rows[4][i]))
    assert len(agent.replay_buffer) == n
    assert np.all(agent.replay_buffer.priorities[:n] == 1.0)     # (staged rows flushed: push's 1.0)
    pr = np.zeros(64, np.float32)
    pr[:n] = (10.0 ** np.random.default_rng(3).uniform(-1, 1, n)).astype(np.float32)
    agent._ctx.per_set_priorities(pr)
    return agent, pr


def test_voided_update_writes_nothing():
    """Check 10: a NaN in policy.fc2.weight — update_parameters raises ValueError and the
    priorities are bit for bit as before."""
    agent, pr = _agent()
    try:
        p = agent._ctx.get_net("policy")
        p["fc2.weight"][0] = np.nan
        agent._ctx.set_net("policy", p)
        before = agent.replay_buffer.priorities
        assert np.array_equal(before.view(np.uint32), pr.view(np.uint32))
        with pytest.raises(ValueError):
            agent.update_parameters(40)
        assert np.array_equal(agent.replay_buffer.priorities.view(np.uint32), before.view(np.uint32))
        with pytest.raises(ValueError):
            agent.update_parameters_many(40, 3)
        assert np.array_equal(agent.replay_buffer.priorities.view(np.uint32), before.view(np.uint32))
    finally:
        agent._ctx.close()


def test_refusals_and_surface():
    """Check 11: the data-parallel calls refuse a context in feedback mode (SACMI_ESTATE), as
    does an update with staged indices; per_set_feedback on a uniform context raises; the
    drop-in agent's replay_buffer is the bound prioritized buffer and an update moves its
    priorities."""
    from sacmi import Config, Context, PrioritizedReplayBuffer
    from sacmi._lib import SacmiError
    name = "S11-A3-H96-B40"
    B = CASES[name][3]
    ctx = fresh_ctx(name)
    try:
        # (the loopback communicator first: without one step_dp returns SACMI_ESTATE anyway)
        ctx.dp_loopback_init(2)
        mt0, frame0, prio0 = ctx.get_mt(1), frame_of(ctx), ctx.per_priorities()
        for call in (lambda: ctx.step_phase(B, 0), lambda: ctx.step_phase(B, 1, parity=1),
                     lambda: ctx.step_dp(B, 1), lambda: ctx.step_dp(B, 3),
                     lambda: ctx.profile_timeline(B, 1, data_parallel=True),
                     lambda: ctx.step(B, idx=np.arange(B))):
            with pytest.raises(SacmiError, match="sacmi error 2.*prioritized feedback is on"):
                call()
        # a refused call leaves no trace
        assert frame_of(ctx) == frame0 and ctx.get_mt(1)[1] == mt0[1]
        assert np.array_equal(ctx.get_mt(1)[0], mt0[0]) and np.array_equal(ctx.per_priorities(), prio0)
        ctx.per_set_feedback(False)
        assert not ctx.per_feedback()
    finally:
        ctx.close()
    uni = Context(Config(11, 3, 96, max_batch=B, capacity=64), 0)
    try:
        with pytest.raises(SacmiError, match="sacmi error 2"):
            uni.per_set_feedback(True)
    finally:
        uni.close()
    agent, pr = _agent()
    try:
        rb = agent.replay_buffer
        assert isinstance(rb, PrioritizedReplayBuffer) and rb.context is agent._ctx
        assert agent._ctx.per_feedback() and rb.frame == 1
        before = rb.priorities
        out = agent.update_parameters(40)
        assert set(out) == {"q1_loss", "q2_loss", "policy_loss"} and all(np.isfinite(list(out.values())))
        after = rb.priorities
        assert not np.array_equal(after, before) and rb.frame == 2
        assert np.array_equal(after[48:], before[48:])
        agent.update_parameters_many(40, 3)
        agent.update_parameters_async(40)
        agent.fetch_losses()
        assert rb.frame == 6
        s, a, r, s2, d, idx, w = rb.sample(16)             # the host API on the same buffer
        rb.update_priorities(idx, np.ones(16, np.float32))
        assert np.all(rb.priorities[idx] == np.float32(1.0 + 1e-6))
    finally:
        agent._ctx.close()
