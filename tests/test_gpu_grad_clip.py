"""Global-norm gradient clipping on the GPU (sacmi_set_grad_clip; csrc/clip.hip and k_adam's
clipped form): per update the three group norms (q1, q2, policy) reduced on the device from the
gradient arena, the coefficients min(1, max / (norm + 1e-6)) in fp32, and Adam stepped from
(g * grad_scale) * coef.  Checked against the GPU's own gradient, against numpy's fp32
expression, against a measure-only run of the same update, against ClipSAC in fp64
(tests/grad_clip_model.py), and across the update's forms.

Cases (all S11-A3), chosen for the reduction's and the layout's edges:
  H96-B40            pad columns in every row, the one-row head, one workgroup per group
  H100-B40-model2    three hidden layers: more segments per group
  H512-B40           groups large enough for several workgroups per group (partials order)
  H256-B4096         the x6 class, ride placement B, 128-byte row pitch
  H512-B4096-bf16    act16 class: k_adam also refreshes the bf16 shadows
  H96-B4100          staged indices; 128-byte pitch with the widest pads
Thresholds come from a measure-only update (inf, inf) of the same state: 0.5 x the smallest
norm (every group clipped), and the geometric mean of the two critic norms on the critic range
with inf on the actor range (one critic clipped, the other not).
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle.sac_step import NETS, OracleSAC, SacConfig, init_params, param_shapes, synthetic_rows

from grad_clip_model import GROUPS, ClipProxy, clip_coef
from test_gpu_parity import (GRAD_TOL, check_step, ctx_alpha_state, ctx_grads, ctx_state, flat_params,
                             load_params, make_ctx, oracle_from_ctx)

pytestmark = pytest.mark.gpu

# name -> (H, B, compute dtype, n_hidden, replay rows, seed)
CASES = {
    "H96-B40": (96, 40, "fp32", 2, 64, 931),
    "H100-B40-model2": (100, 40, "fp32", 3, 64, 932),
    "H512-B40": (512, 40, "fp32", 2, 64, 933),
    "H256-B4096": (256, 4096, "fp32", 2, 4200, 934),
    "H512-B4096-bf16": (512, 4096, "bf16", 2, 4200, 935),
    "H96-B4100": (96, 4100, "fp32", 2, 4200, 936),
}
NAMES = list(CASES)
DEVICE_SAMPLED = [n for n in NAMES if CASES[n][1] <= 4096]
KEY = (np.arange(624, dtype=np.uint64) * 1812433 % (2 ** 32)).astype(np.uint32)
INF = math.inf
GN = ("norm_q1", "norm_q2", "norm_pi", "coef_q1", "coef_q2", "coef_pi")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ulps(got, want):
    """|got - want| in fp32 ulps of want (elementwise; want in fp64)."""
    want = np.asarray(want, np.float64)
    sp = np.spacing(np.maximum(np.abs(want), 1e-38).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - want) / sp


def case_inputs(name):
    H, B, dt, nh, n, seed = CASES[name]
    cfg = SacConfig(11, 3, H, n_hidden=nh)
    params = init_params(cfg, seed, bias_scale=0.05)
    rows = synthetic_rows(cfg, n, seed + 1000, state_scale=0.5)
    rng = np.random.default_rng(seed + 2000)
    idx = [rng.permutation(n)[:B] for _ in range(2)]
    eps = [rng.standard_normal((B, 3)).astype(np.float32) for _ in range(4)]
    return cfg, params, rows, idx, eps


def fresh_ctx(name, clip=None, stats=False, **kw):
    H, B, dt, nh, n, seed = CASES[name]
    cfg, params, rows, _, _ = case_inputs(name)
    ctx = make_ctx(cfg, max_batch=B, capacity=n, seed=5, compute_dtype=dt, **kw)
    load_params(ctx, params)
    ctx.push(*rows)
    ctx.set_mt(0, KEY, 624)
    if stats:
        ctx.set_stats(True)
    if clip is not None:
        ctx.set_grad_clip(*clip)
    return ctx


def snapshot(ctx, cfg):
    """Everything an update leaves: parameters and targets, moments, log_alpha's state."""
    shapes = param_shapes(cfg)
    out = {"state": ctx_state(ctx, cfg), "alpha": ctx_alpha_state(ctx)}
    for slot in ("m", "v"):
        out[slot] = {f"{n}.{k}": v for n in GROUPS for k, v in ctx.get_net(n, slot, shapes[n]).items()}
    return out


def assert_same(a, b, what):
    for part in ("state", "m", "v"):
        for k in a[part]:
            assert np.array_equal(bits(a[part][k]), bits(b[part][k])), (what, part, k)
    assert a["alpha"] == b["alpha"], (what, a["alpha"], b["alpha"])


@functools.lru_cache(maxsize=None)
def staged(name, clip, n_updates=1, poison=False, stats=False):
    """n staged updates of the case from its fixed state.  clip: None (the feature never
    enabled) or (critic, actor).  poison: the gradient arena is a torch tensor filled with 1e3
    before the update (attach_grad_arena): whatever the update does not write stays poisoned."""
    H, B, dt, nh, n, seed = CASES[name]
    cfg, params, rows, idx, eps = case_inputs(name)
    ctx = fresh_ctx(name, clip, stats)
    arena = None
    try:
        if poison:
            numel = ctx.grad_arena_numel()
            arena = torch.zeros(numel, dtype=torch.float32, device="cuda")
            ctx.attach_grad_arena(arena.data_ptr(), numel)
            arena.fill_(1e3)
            torch.cuda.synchronize()
        losses, grads = [], []
        for u in range(n_updates):
            losses.append(np.asarray(ctx.step(B, idx[u], eps[2 * u], eps[2 * u + 1]), np.float32))
            grads.append(ctx_grads(ctx, cfg))
        rows_, total = ctx.fetch_grad_norms()
        out = snapshot(ctx, cfg)
        out.update(losses=losses, grads=grads, rows=rows_, total=total,
                   stats=ctx.fetch_stats()[0] if stats else None)
        return out
    finally:
        ctx.close()
        del arena


def measured(name):
    return staged(name, (INF, INF))["rows"][0][:3].astype(np.float64)


def thresholds(name):
    """(all-clipped, mixed) thresholds from the measure-only norms; asserts that the mixed one
    separates the critics."""
    nq1, nq2, npi = measured(name)
    allc = 0.5 * min(nq1, nq2, npi)
    mixed = math.sqrt(nq1 * nq2)
    lo, hi = min(nq1, nq2), max(nq1, nq2)
    # one critic's coefficient below 1, the other's exactly 1 (fp32: norm + 1e-6 <= max)
    assert clip_coef(hi, mixed) < 1 and clip_coef(lo, mixed) == 1, (name, nq1, nq2, mixed)
    return (allc, allc), (mixed, INF)


def group_norm_from_grads(grads, n):
    s = 0.0
    for k, v in grads.items():
        if k.startswith(n + "."):
            s += float(np.sum(np.square(v.astype(np.float64))))
    return float(np.float32(math.sqrt(s)))


# ---------------------------------------------------------------------------- check 1
@pytest.mark.parametrize("name", NAMES)
def test_measure_only_is_free_of_side_effects(name):
    """Check 1: two updates with (inf, inf) — staged, and device-sampled with a fixed MT key
    where the batch allows — leave parameters, targets, moments, log_alpha's state, losses and
    diagnostics rows bit-identical to a context that never enabled the feature; every coef is
    exactly 1.0 and `total` counts the updates."""
    off, on = staged(name, None, 2, stats=True), staged(name, (INF, INF), 2, stats=True)
    assert_same(off, on, name)
    assert np.array_equal(bits(np.stack(off["losses"])), bits(np.stack(on["losses"])))
    assert np.array_equal(bits(off["stats"]), bits(on["stats"])) and on["stats"].shape[0] == 2
    assert off["total"] == 0 and off["rows"].shape == (0, 6)
    assert on["total"] == 2 and on["rows"].shape == (2, 6) and on["rows"].dtype == np.float32
    assert np.all(on["rows"][:, 3:] == 1.0) and np.all(on["rows"][:, :3] > 0) and np.all(np.isfinite(on["rows"]))
    if name not in DEVICE_SAMPLED:
        return
    H, B, dt, nh, n, seed = CASES[name]
    cfg = case_inputs(name)[0]
    res = []
    for clip in (None, (INF, INF)):
        ctx = fresh_ctx(name, clip)
        try:
            ls = [np.asarray(ctx.step(B), np.float32) for _ in range(2)]
            res.append((snapshot(ctx, cfg), np.stack(ls), ctx.get_mt(0), ctx.fetch_grad_norms()))
        finally:
            ctx.close()
    assert_same(res[0][0], res[1][0], name + " device-sampled")
    assert np.array_equal(bits(res[0][1]), bits(res[1][1]))
    assert np.array_equal(res[0][2][0], res[1][2][0]) and res[0][2][1] == res[1][2][1]
    assert res[1][3][1] == 2 and np.all(res[1][3][0][:, 3:] == 1.0)


# ---------------------------------------------------------------------------- check 2
@pytest.mark.parametrize("name", NAMES)
def test_norm_against_the_gpus_own_gradient(name):
    """Check 2: norm_n == float32(sqrt(fp64 sum of squares of the REAL elements of
    SACMI_SLOT_GRAD)) within 1 fp32 ulp (the fp64 order differences are far below half an ulp;
    1 ulp allows the final rounding) — for the measure-only run and, SLOT_GRAD being the raw
    pre-clip gradient, for the clipped one.  Poisoning: with the arena filled with 1e3 before
    the update, everything the update does not write (the pad columns) stays 1e3, and the norms
    must not move by a bit: this fails if pads are counted."""
    for clip in ((INF, INF), thresholds(name)[0]):
        r = staged(name, clip)
        for i, n in enumerate(GROUPS):
            want = group_norm_from_grads(r["grads"][0], n)
            got = float(r["rows"][0][i])
            print(f"[clip {name}] {n} norm gpu {got:.9e} from SLOT_GRAD {want:.9e} ulps {ulps(got, want):.2f}")
            assert ulps(got, want) <= 1.0, (name, clip, n, got, want)
    clean, dirty = staged(name, (INF, INF)), staged(name, (INF, INF), 1, True)
    assert np.array_equal(bits(clean["rows"]), bits(dirty["rows"])), (name, clean["rows"], dirty["rows"])
    # (the groups are distinguishable: swapped slots would not pass)
    assert len({float(x) for x in clean["rows"][0][:3]}) == 3


# ---------------------------------------------------------------------------- check 3
@pytest.mark.parametrize("name", NAMES)
def test_coefficient_is_the_fp32_expression(name):
    """Check 3: coef == numpy's fp32 min(1, max / (norm + 1e-6)) of the row's own norm within
    1 ulp, all-clipped and mixed.  Measured on MI355X: bit-equal in every case (the kernel
    forms it with one fp32 add and one IEEE fp32 division)."""
    allc, mixed = thresholds(name)
    for clip in (allc, mixed):
        row = staged(name, clip)["rows"][0]
        mx = (clip[0], clip[0], clip[1])
        for i in range(3):
            want = clip_coef(row[i], mx[i])
            eq = bits(row[3 + i]) == bits(want)
            print(f"[clip {name}] {GN[3 + i]} gpu {row[3 + i]:.9e} numpy {want:.9e} bit-equal {bool(eq)}")
            assert ulps(row[3 + i], want) <= 1.0, (name, clip, i, row[3 + i], want)
    row = staged(name, allc)["rows"][0]
    assert np.all(row[3:] < 1.0) and np.all(row[3:] > 0.0)
    row = staged(name, mixed)["rows"][0]
    assert (row[3] < 1.0) != (row[4] < 1.0) and row[5] == 1.0


# ---------------------------------------------------------------------------- check 4
@pytest.mark.parametrize("name", NAMES)
def test_the_step_used_the_coefficient(name):
    """Check 4.  Adam at step 1 is almost scale-invariant (p -= lr g / (|g| + eps')), so the
    parameters alone cannot show a wrong coefficient; the moments can.  One clipped update from
    zero moments against the same update unclipped, with u = 2^-24 (half an ulp):
      m0 = fl((1-b1) g)                      m1 = fl((1-b1) fl(g c))
         -> three roundings between m1 and c m0: relative 3u, which is 1.5 ulp of a value with
            mantissa 1 and 3 ulp of one with mantissa near 2; + the fp32 coef read back  <= 4 ulp
      v0 = fl(fl((1-b2) g) g)                v1 = fl(fl((1-b2) g') g'),  g' = fl(g c)
         -> g' enters twice (2u), two more products (2u), v0's own two (2u): relative 6u, 3 to
            6 ulp  <= 8 ulp
    (the moment's old value is 0, so m + (1-b1)(g - m) and v b2 + ... add nothing).  Measured
    worst over the six cases (MI355X): m 2.17 ulp, v 3.86 ulp; coef-1 groups 0.  The
    unclipped reference is the measure-only run for q1 and q2; for the policy, whose gradient
    is taken through the critics the same update has just stepped, it is the run with the
    same critic threshold and inf on the actor range.  Groups with coef 1 are bit-equal;
    log_alpha, its moments and alpha never see a coefficient and are bit-equal to the
    measure-only run."""
    allc, mixed = thresholds(name)
    base = staged(name, (INF, INF))
    for clip in (allc, mixed):
        r = staged(name, clip)
        ref_pi = staged(name, (clip[0], INF))
        assert np.array_equal(bits(ref_pi["rows"][0][:5]), bits(r["rows"][0][:5]))
        for i, n in enumerate(GROUPS):
            c = np.float64(r["rows"][0][3 + i])
            ref = ref_pi if n == "policy" else base
            worst = [0.0, 0.0]
            for k in r["m"]:
                if not k.startswith(n + "."):
                    continue
                if c == 1.0:
                    assert np.array_equal(bits(r["m"][k]), bits(ref["m"][k])), (name, clip, k)
                    assert np.array_equal(bits(r["v"][k]), bits(ref["v"][k])), (name, clip, k)
                    assert np.array_equal(bits(r["state"][k]), bits(ref["state"][k])), (name, clip, k)
                    continue
                em = ulps(r["m"][k], c * ref["m"][k].astype(np.float64)).max()
                ev = ulps(r["v"][k], c * c * ref["v"][k].astype(np.float64)).max()
                worst = [max(worst[0], em), max(worst[1], ev)]
                assert em <= 4.0, (name, clip, k, "m", em)
                assert ev <= 8.0, (name, clip, k, "v", ev)
                assert np.any(r["m"][k] != ref["m"][k])
            print(f"[clip {name}] {n} coef {c:.6f} worst ulps m {worst[0]:.2f} v {worst[1]:.2f}")
        assert r["alpha"] == base["alpha"], (name, clip)
        assert np.array_equal(bits(r["state"]["log_alpha"]), bits(base["state"]["log_alpha"]))


# ---------------------------------------------------------------------------- check 5
@pytest.mark.parametrize("name", ["H96-B40", "H100-B40-model2"])
def test_parity_with_fp64(name):
    """Check 5: two clipped updates (every group clipped) against ClipSAC in fp64 (and fp32,
    the reference's own arithmetic, for check_step's bars), re-anchored on the GPU's state
    before the second.  Norms within GRAD_TOL relative — | ||g|| - ||g_ref|| | <= ||g - g_ref||,
    the per-tensor gradient bar — and so the coefs; parameters, gradients, losses and
    log_alpha's state pass check_step as an unclipped update's do; the moments are held to the
    gradient bar scaled the same way."""
    H, B, dt, nh, n, seed = CASES[name]
    cfg, params, rows, idx, eps = case_inputs(name)
    thr = thresholds(name)[0][0]
    mx = {g: thr for g in GROUPS}
    ctx = fresh_ctx(name, (thr, thr))
    try:
        o32, o64 = OracleSAC(cfg, params, torch.float32), OracleSAC(cfg, params, torch.float64)
        prev = flat_params(params)
        for u in range(2):
            if u:
                prev = {k: v.astype(np.float64) for k, v in ctx_state(ctx, cfg).items()}
                o32, o64 = oracle_from_ctx(ctx, cfg, torch.float32), oracle_from_ctx(ctx, cfg, torch.float64)
            for o in (o32, o64):
                for g in GROUPS:
                    o.opt[g] = ClipProxy(o.opt[g], mx[g], "fp64")
            lg = ctx.step(B, idx[u], eps[2 * u], eps[2 * u + 1])
            batch = [x[idx[u]] for x in rows]
            l32 = o32.step(*batch, eps[2 * u], eps[2 * u + 1])
            l64 = o64.step(*batch, eps[2 * u], eps[2 * u + 1])
            res = dict(gpu=(lg, ctx_state(ctx, cfg), ctx_grads(ctx, cfg)), alpha=ctx_alpha_state(ctx),
                       o32=(l32, o32.state(), o32.grads_flat()), o64=(l64, o64.state(), o64.grads_flat()))
            check_step(res, prev, f"clip-{name}-u{u}")
            row = ctx.fetch_grad_norms(1)[0][0].astype(np.float64)
            for i, g in enumerate(GROUPS):
                wn, wc = o64.opt[g].norms[-1], o64.opt[g].coefs[-1]
                print(f"[clip {name}] u{u} {g} norm gpu {row[i]:.9e} fp64 {wn:.9e} rel {abs(row[i] - wn) / wn:.2e}; "
                      f"coef gpu {row[3 + i]:.9e} fp64 {wc:.9e}")
                assert abs(row[i] - wn) <= GRAD_TOL * wn, (name, u, g, row[i], wn)
                assert abs(row[3 + i] - wc) <= GRAD_TOL * wc, (name, u, g, row[3 + i], wc)
                assert wc < 1.0
            if u == 0:      # from zero moments: m = (1-b1) c g, v = (1-b2) (c g)^2, per tensor
                shapes = param_shapes(cfg)
                s64 = res["o64"][1]
                for g in GROUPS:
                    m = ctx.get_net(g, "m", shapes[g])
                    v = ctx.get_net(g, "v", shapes[g])
                    for k in m:
                        em = np.linalg.norm(m[k] - s64[f"adam.{g}.{k}.m"]) / np.linalg.norm(s64[f"adam.{g}.{k}.m"])
                        ev = np.linalg.norm(v[k] - s64[f"adam.{g}.{k}.v"]) / np.linalg.norm(s64[f"adam.{g}.{k}.v"])
                        e32 = np.linalg.norm(res["o32"][1][f"adam.{g}.{k}.m"] - s64[f"adam.{g}.{k}.m"]) / \
                            np.linalg.norm(s64[f"adam.{g}.{k}.m"])
                        assert em <= max(2 * GRAD_TOL, 4 * e32), (name, g, k, "m", em, e32)
                        assert ev <= max(4 * GRAD_TOL, 8 * e32), (name, g, k, "v", ev, e32)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------- check 6
def _form_ctx(shape, clip, **kw):
    replay = "uniform"
    if shape == "small":
        cfg, B, nrows, dt = SacConfig(24, 4, 64), 64, 500, "fp32"
    elif shape == "per_small":
        cfg, B, nrows, dt, replay = SacConfig(24, 4, 64), 64, 500, "fp32", "per"
    else:
        cfg, B, nrows, dt = SacConfig(661, 23, 512), 4096, 6000, "bf16"
    params = init_params(cfg, 61, bias_scale=0.05)
    rows = synthetic_rows(cfg, nrows, 62, state_scale=0.5)
    ctx = make_ctx(cfg, max_batch=B, capacity=nrows, compute_dtype=dt, replay=replay, seed=7, **kw)
    load_params(ctx, params)
    ctx.push(*rows)
    if replay == "per":
        ctx.per_set_priorities(np.random.default_rng(64).uniform(0.1, 2.0, nrows).astype(np.float32))
        ctx.set_mt(1, (np.arange(624, dtype=np.uint64) * 69069 % (2 ** 32)).astype(np.uint32), 624)
        ctx.per_set_feedback(True)
    ctx.set_mt(0, (np.arange(624, dtype=np.uint64) * 40503 % (2 ** 32)).astype(np.uint32), 624)
    if clip is not None:
        ctx.set_grad_clip(*clip)
    return ctx, cfg, B


def _form_result(ctx, n):
    out = (ctx.fetch_losses(n), {k: ctx.get_net(k) for k in NETS},
           {(k, s): ctx.get_net(k, s) for k in GROUPS for s in ("m", "v")}, ctx.get_mt(0),
           ctx.fetch_grad_norms())
    return out


def _assert_forms_equal(a, b, what, n):
    assert np.array_equal(bits(a[0]), bits(b[0])) and a[0].shape == (n, 3), what
    for part in (1, 2):
        for k in a[part]:
            for t in a[part][k]:
                assert np.array_equal(bits(a[part][k][t]), bits(b[part][k][t])), (what, k, t)
    assert np.array_equal(a[3][0], b[3][0]) and a[3][1] == b[3][1], what
    assert a[4][1] == b[4][1] == n and np.array_equal(bits(a[4][0]), bits(b[4][0])), what
    # thresholds far below the norms: every update of the sequence was clipped
    assert np.all(a[4][0][:, 3:] < 1.0) and np.all(a[4][0][:, 3:] > 0.0), what


# (1e-3, 2e-3): far below any of these gradients' norms — asserted on the rows
FORM_CLIP = (1e-3, 2e-3)


@pytest.mark.parametrize("shape", ["small", "nao_b4096_bf16", "per_small"])
def test_many_updates_per_launch_identical_clipped(shape):
    """Check 6a: with clipping on, n single updates == sacmi_step_many_async launches bit for
    bit — losses, parameters, moments, the sampling stream and the norm rows: the small class
    (rides in L12 / L13), the batch-4096 bf16 class (placement B), and a prioritized context
    with feedback on (the side stream's write-back and draw)."""
    res = []
    for many in (True, False):
        ctx, cfg, B = _form_ctx(shape, FORM_CLIP)
        try:
            if many:
                ctx.step_many_async(B, 3)
                ctx.step_many_async(B, 2)
            else:
                for _ in range(5):
                    ctx.step_async(B)
            res.append(_form_result(ctx, 5))
        finally:
            ctx.close()
    _assert_forms_equal(res[0], res[1], shape, 5)


def test_graph_eager_launch_wait_and_stats_agree_clipped():
    """Check 6b: with clipping on, graph == eager, sacmi_step_launch / _wait == sacmi_step
    (losses read from the host-mapped words the actor Adam's scalar tail stores), and
    diagnostics on / off give the same parameters."""
    res = []
    for form in ("step", "eager", "launch_wait", "stats"):
        if form == "eager":
            os.environ["SACMI_NO_GRAPH"] = "1"
        try:
            ctx, cfg, B = _form_ctx("small", FORM_CLIP)
        finally:
            os.environ.pop("SACMI_NO_GRAPH", None)
        try:
            if form == "stats":
                ctx.set_stats(True)
            ls = []
            for _ in range(3):
                if form == "launch_wait":
                    ctx.step_launch(B)
                    ls.append(ctx.step_wait())
                else:
                    ls.append(ctx.step(B))
            r = _form_result(ctx, 0)
            res.append((np.asarray(ls, np.float32),) + r[1:])
            if form == "stats":
                assert ctx.fetch_stats()[1] == 3
        finally:
            ctx.close()
    for r, form in zip(res[1:], ("eager", "launch_wait", "stats")):
        assert np.array_equal(bits(res[0][0]), bits(r[0])), form
        for part in (1, 2):
            for k in r[part]:
                for t in r[part][k]:
                    assert np.array_equal(bits(res[0][part][k][t]), bits(r[part][k][t])), (form, k, t)
        assert res[0][4][1] == r[4][1] == 3 and np.array_equal(bits(res[0][4][0]), bits(r[4][0])), form
    assert np.all(res[0][4][0][:, 3:] < 1.0) and np.all(np.isfinite(res[0][0]))


# ---------------------------------------------------------------------------- check 7
@pytest.mark.parametrize("world", [2, 4])
def test_dp_loopback_allreduce_clipped(world):
    """Check 7a: sacmi_step_dp in the all-reduce form at world 2 and 4 (loopback: x world in
    place of the collective, 1/world in grad_scale — both exact for a power of two) with
    clipping on == the single context's clipped updates bit for bit, norm rows included: the
    reduction runs behind the collective on the scaled gradient, and the critic range's
    trailing flag floats are not gradient."""
    n = 3
    a, cfg, B = _form_ctx("small", FORM_CLIP)
    b, _, _ = _form_ctx("small", FORM_CLIP)
    try:
        a.dp_loopback_init(world)
        a.dp_set_sharded(False)
        a.step_dp(B, n)
        for _ in range(n):
            b.step_async(B)
        _assert_forms_equal(_form_result(a, n), _form_result(b, n), f"world {world}", n)
    finally:
        a.close()
        b.close()


def test_sharded_form_is_refused():
    """Check 7b: the sharded optimizer step and clipping exclude each other, both ways round,
    with SACMI_ESTATE and nothing touched."""
    from sacmi._lib import SacmiError
    ctx, cfg, B = _form_ctx("small", FORM_CLIP)
    try:
        ctx.dp_loopback_init(2)
        before = {k: ctx.get_net(k) for k in NETS}
        with pytest.raises(SacmiError, match="sharded"):
            ctx.dp_set_sharded(True)
        assert not ctx.dp_sharded() and ctx.grad_clip() == FORM_CLIP
        ctx.step_dp(B, 1)                                 # (the all-reduce form goes on working)
        assert ctx.fetch_grad_norms()[1] == 1
        after = {k: ctx.get_net(k) for k in NETS}
        assert any(not np.array_equal(before[k][t], after[k][t]) for k in before for t in before[k])
    finally:
        ctx.close()
    ctx, cfg, B = _form_ctx("small", None)
    try:
        ctx.dp_loopback_init(2)
        ctx.dp_set_sharded(True)
        before = {k: ctx.get_net(k) for k in NETS}
        with pytest.raises(SacmiError, match="sharded"):
            ctx.set_grad_clip(1.0, 1.0)
        assert ctx.grad_clip() == (0.0, 0.0) and ctx.dp_sharded()
        ctx.step_dp(B, 1)                                 # (unclipped, sharded: as before)
        assert ctx.fetch_grad_norms()[1] == 0
        ctx.dp_sync_state()
        after = {k: ctx.get_net(k) for k in NETS}
        assert any(not np.array_equal(before[k][t], after[k][t]) for k in before for t in before[k])
    finally:
        ctx.close()


# ---------------------------------------------------------------------------- check 8
def test_off_means_off():
    """Check 8: after set_grad_clip(0, 0) the update's launch sites are those of a context that
    never enabled the feature (no grad_sumsq site); on, each update has exactly the four new or
    changed sites and no fused *_dW_adam level.  Negative or NaN thresholds: SACMI_EVALUE."""
    def sites(ctx, B):
        return [k["site"] for k in ctx.profile_timeline(B, 2)[0]]
    fresh, cfg, B = _form_ctx("small", None)
    ctx, _, _ = _form_ctx("small", None)
    try:
        want = sites(fresh, B)
        assert not any("grad_sumsq" in s for s in want) and sum(s.endswith("_dW_adam") for s in want) == 4
        ctx.set_grad_clip(1.0, INF)
        assert ctx.grad_clip() == (1.0, INF)
        on = sites(ctx, B)
        for s in ("grad_sumsq_critic", "grad_sumsq_actor", "adam_actor_alpha"):
            assert on.count(s) == 2, (s, on)
        assert on.count("adam_critic") + on.count("adam_critic_polyak") == 2
        assert not any(s.endswith("_dW_adam") for s in on)
        assert on.count("gemm_L6_critic_dW1") == 2 and on.count("gemm_L13_pi_dW1") == 2
        assert on.index("gemm_L6_critic_dW1") < on.index("grad_sumsq_critic") < on.index("gemm_L7_act_fc1")
        assert on.index("gemm_L13_pi_dW1") < on.index("grad_sumsq_actor") < on.index("adam_actor_alpha")
        kernels = {k["site"]: k["kernel"] for k in ctx.profile_timeline(B, 1)[0]}
        assert kernels["grad_sumsq_critic"] == "k_grad_sumsq" and kernels["adam_actor_alpha"] == "k_adam"
        ctx.set_grad_clip(0, 0)
        assert ctx.grad_clip() == (0.0, 0.0)
        assert sites(ctx, B) == want
        ctx.set_grad_clip(0, 2.0)                       # critic range measured only
        assert ctx.grad_clip() == (INF, 2.0)
        for bad in ((-1.0, 1.0), (1.0, -1.0), (math.nan, 1.0), (1.0, math.nan), (-INF, 0.0)):
            with pytest.raises(ValueError):
                ctx.set_grad_clip(*bad)
            assert ctx.grad_clip() == (INF, 2.0)
    finally:
        fresh.close()
        ctx.close()


def test_env_switch_at_creation():
    """SACMI_GRAD_CLIP=<critic>[,<actor>] at creation: on from the first update (how the
    unchanged benchmark runs with the feature on); one value serves both ranges; inf accepted."""
    for env, want in (("inf", (INF, INF)), ("0.5,inf", (0.5, INF)), ("2", (2.0, 2.0))):
        os.environ["SACMI_GRAD_CLIP"] = env
        try:
            ctx, cfg, B = _form_ctx("small", None)
        finally:
            os.environ.pop("SACMI_GRAD_CLIP", None)
        try:
            assert ctx.grad_clip() == want
            ctx.step(B)
            assert ctx.fetch_grad_norms()[1] == 1
        finally:
            ctx.close()
    ctx, cfg, B = _form_ctx("small", None)
    try:
        assert ctx.grad_clip() == (0.0, 0.0)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------- check 9
def test_agent_surface():
    """Check 9: SAC(..., max_grad_norm=x).fetch_grad_norms() returns one dict per update keyed
    by sacmi.GNORM_NAMES; a float serves all three groups, a pair is (critic, actor);
    max_grad_norm=None returns [] and update_parameters' keys are the reference's three."""
    from sacmi import GNORM_NAMES, SAC
    assert tuple(GNORM_NAMES) == GN
    cfg = SacConfig(11, 3, 96)
    rows = synthetic_rows(cfg, 48, 9, state_scale=0.5)
    for mgn in (1e-3, (1e-3, math.inf), None):
        agent = SAC(11, 3, hidden_dim=96, capacity=64, max_batch=40, seed=5, max_grad_norm=mgn)
        try:
            for i in range(48):
                agent.replay_buffer.push(rows[0][i], rows[1][i], float(rows[2][i]), rows[3][i], bool(rows[4][i]))
            out = agent.update_parameters(40)
            assert set(out) == {"q1_loss", "q2_loss", "policy_loss"}
            agent.update_parameters_many(40, 2)
            d = agent.fetch_grad_norms()
            if mgn is None:
                assert d == [] and agent._ctx.grad_clip() == (0.0, 0.0)
                continue
            assert len(d) == 3 and all(tuple(x) == GN for x in d)
            assert all(np.isfinite(list(x.values())).all() for x in d)
            assert all(x["coef_q1"] < 1 and x["coef_q2"] < 1 for x in d)
            assert all((x["coef_pi"] < 1) == (mgn == 1e-3) for x in d)
            assert agent.fetch_grad_norms(max_rows=1)[0] == d[-1]
        finally:
            agent._ctx.close()
