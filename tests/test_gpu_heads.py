"""The policy sample head (k_heads_sample, k_act_heads, k_gemm_sample_bwd, k_sample_bwd_tail
and the rows_finish log-prob consumers) at its clamp, saturation and bound edges, through the
C ABI, on the doctored head columns of tests/heads_cases.py with action bounds (-0.3, 0.9).

The other parity tests draw small states against xavier heads: log_std stays near 0, tanh is
rarely saturated and the action bias is 0.  Here columns 0 / 1 are clamped on every row (their
log_std gradients must be EXACTLY zero), columns 2 / 3 sit exactly on a bound (the gradient
passes: torch.clamp is inclusive), columns 4 / 5 straddle one (the mask is a per-row decision,
taken from the raw head sum), columns 6 / 7 saturate tanh (|x| ~ 6 and 12), and the nonzero
bias reaches the critics through both policy samples.

Yardstick: the float64 oracle, with bars max(GRAD_TOL, 4 e_ref) where e_ref is the float32
noise floor of the well-conditioned head formula (oracle/heads_model.py in float32 against
float64 on the case's own inputs).  The reference's own fp32 step is NOT a yardstick here: on
these columns it is 1e-3 .. 1 from fp64 (its quadratic log-prob term and its 1 - y^2 cancel;
tests/test_heads_model.py prints both); it is printed next to the bars for the record.
Per column j the error of mean.weight[j, :], log_std.weight[j, :] and the two bias entries is
taken over the column's own scale sum_rows |dhead_ij| (x ||h_i|| for the weight rows), so a
cancelling batch sum neither hides an error nor inflates one.

Every update case asserts from the launch timeline which head kernels ran (site, kernel and
grid; the template instantiation follows from the launchers' rules, restated in
`instantiations` and asserted against the table of cases) and prints them.

Measured on the MI355X (worst column of the case; e_ref and the torch fp32 step on the same
scale; losses relative to fp64):
  case               head kernels (timeline: site grid)        gpu vs fp64, worst column            e_ref    torch fp32 step    losses gpu (q1 q2 pi)     torch fp32 losses
                                                               mean.w  mean.b  ls.w    ls.b         worst    mean.* / ls.*
  A6-H64-B64         heads<32,16> 8, tail<NPA 16> 8            1.2e-7  1.6e-7  4.6e-8  1.0e-7       1.1e-7   5.7e-1 / 4.6e-3    7.0e-8 1.4e-7 1.3e-7      3.6e-5 3.6e-5 1.5e-5
  A6-H64-B64-m2      heads<32,16> 8, L10<NST 10> 4             1.5e-7  2.0e-7  6.9e-8  2.4e-8       6.5e-8   4.0e-1 / 8.1e-3    6.9e-8 2.1e-7 6.5e-8      3.1e-5 3.1e-5 1.6e-5
  A17-H512-B100      heads<48,16> 13, tail<NPA 32> 13          1.7e-7  7.8e-8  5.7e-8  1.8e-7       1.7e-7   1.0    / 3.7e-3    1.8e-7 1.8e-7 1.0e-7      5.3e-5 5.3e-5 2.1e-5
  A23-H64-B64-m2     heads<48,16> 8, L10<NST 16> 4             1.7e-7  2.5e-7  6.1e-8  6.9e-8       1.9e-7   1.0    / 2.4e-3    2.7e-7 1.8e-7 1.0e-7      1.9e-5 1.9e-5 1.5e-5
  A32-H768-B64       heads<64,16> 8, tail<NPA 64> 8            6.2e-7  8.7e-7  6.6e-8  5.7e-8       2.1e-7   1.0    / 5.0e-3    1.9e-7 1.8e-7 1.1e-7      1.1e-4 1.1e-4 1.3e-5
  A32-H64-B72-m2     heads<64,16> 9, L10<NST 16> 5             1.6e-7  1.6e-7  7.3e-8  6.8e-8       1.7e-7   1.0    / 8.3e-3    2.9e-7 2.9e-7 <1e-8       9.5e-5 9.6e-5 2.0e-5
  A6-H64-B64-pm0.4   heads<32,16> 8, tail<NPA 16> 8            7.2e-8  9.7e-8  5.5e-8  4.0e-8       9.6e-8   5.8e-1 / 3.1e-3    1.3e-7 6.8e-8 1.9e-7      2.6e-5 2.5e-5 9.5e-6
  A6-H64-B4096       heads<32,32> 256, L10<NST 10> 256         1.3e-7  1.7e-7  7.2e-8  1.6e-7       4.2e-8   5.0e-1 / 2.7e-3    (masked-truth helper: within LOSS_TOL)
  A23-H512-B4096-bf16 heads<48,32,H16> 256, L10<NST 16,H16> 256   exact zeros hold; vs the bf16 emulation: policy heads 8.4e-6 .. 6.6e-5, worst tensor 1.7e-3 (q1.fc1.weight)
(the fold engages at hidden 768 / batch 64: 48 column-block partials, the tail's NPA 64 form.)
Every remaining policy tensor, log_alpha's gradient and the q1 / q2 gradients sit at 1e-8 .. 3e-7;
column 3's log_std.bias gradient is -alpha (1 + r) with r = 1.5e-8 .. 1.6e-7.  select_action:
max |gpu - fp64| 3.5e-8 .. 1.1e-7 over A in {6, 17, 32} x n in {1, 7, 200}, up to 164 elements
at |x| >= 12 a call.  The torch fp32 step's loss deviation is its `1 - y.pow(2)` rounding to 0 at
|x| > 9 (log(1e-6) where the truth is log(scale omy2 + 1e-6)): a kernel with that form in place of
one_minus_tanh2 reproduces those figures to two digits and misses LOSS_TOL in every fp32 case.
"""
import numpy as np
import pytest
import torch

from heads_cases import (ALL_CLAMPED, HEAD_KEYS, assert_straddle_precondition, doctor_heads, head_truth_tables,
                         make_case, policy_heads_fp64)
from oracle import heads_model as HM
from oracle.sac_step import NETS, OracleSAC, SacConfig, _policy_sample, init_params
from test_gpu_parity import GRAD_TOL, LOSS_TOL, ctx_grads, load_params, make_ctx, rel

pytestmark = pytest.mark.gpu

TAIL, L10, HEADS = "sample_bwd_tail_dhp2", "gemm_L10_dlda_sample_bwd_dhp2", "heads_sample"


def instantiations(A, H, B):
    """The launchers' own rules (kernels.hip launch_heads_sample, launch_gemm_sample_bwd,
    launch_sample_bwd_tail; sacmi_internal.h heads_rows_per_wg)."""
    n = 2 * A
    n_pa = 2 * ((H + 31) // 32)
    return dict(heads_TN=32 if n <= 32 else 48 if n <= 48 else 64, heads_TM=32 if 2 * B >= 8192 else 16,
                NST=10 if (n + 3) // 4 <= 10 else 16, NPA=16 if n_pa <= 16 else 32 if n_pa <= 32 else 64)


# name -> (make_case arguments, compute dtype, the backward site it must run, the instantiations
# the case is there for)
UPDATE_CASES = {
    "A6-H64-B64": (dict(S=20, A=6, H=64, B=64, n_hidden=2, seed=1), "fp32", TAIL, dict(NPA=16, heads_TN=32, heads_TM=16)),
    "A6-H64-B64-m2": (dict(S=20, A=6, H=64, B=64, n_hidden=3, seed=3), "fp32", L10, dict(NST=10)),
    "A17-H512-B100": (dict(S=24, A=17, H=512, B=100, seed=1), "fp32", TAIL, dict(NPA=32, heads_TN=48)),
    "A23-H64-B64-m2": (dict(S=24, A=23, H=64, B=64, n_hidden=3, seed=1), "fp32", L10, dict(NST=16, heads_TN=48)),
    "A32-H768-B64": (dict(S=24, A=32, H=768, B=64, seed=2), "fp32", TAIL, dict(NPA=64, heads_TN=64)),
    "A32-H64-B72-m2": (dict(S=24, A=32, H=64, B=72, n_hidden=3, seed=1), "fp32", L10, dict(NST=16, heads_TN=64)),
    "A6-H64-B64-pm0.4": (dict(S=20, A=6, H=64, B=64, n_hidden=2, seed=1, bounds=(-0.4, 0.4)), "fp32", TAIL,
                         dict(NPA=16, heads_TN=32)),
}
B4096_FP32 = (dict(S=20, A=6, H=64, B=4096, seed=1), "fp32", L10, dict(heads_TM=32, heads_TN=32, NST=10))
# bf16 activations (the H16 variants) need hidden >= 512, a multiple of 128, at batch >= 4096
# (sacmi_step_act16): (24, 23, 64) does not take them, (24, 23, 512) is the smallest that does
B4096_BF16 = (dict(S=24, A=23, H=512, B=4096, seed=2, bf16_act=True), "bf16", L10,
              dict(heads_TM=32, heads_TN=48, NST=16))


def head_kernels(ctx, case, site, want_inst, what):
    """Assert, from the launch timeline, the head kernels of an update (call it once everything
    of the checked update is read back: the timeline replays whole updates)."""
    cfg = case.cfg
    A, H, B = cfg.action_dim, cfg.hidden_dim, len(case.idx)
    inst = instantiations(A, H, B)
    for k, v in want_inst.items():
        assert inst[k] == v, (what, k, inst[k], "the case is there for", v)
    ks, _ = ctx.profile_timeline(B, 1)
    by_site = {}
    for k in ks:
        by_site.setdefault(k["site"], []).append((k["kernel"], k["grid"]))
    want = {HEADS: [("k_heads_sample", -(-2 * B // inst["heads_TM"]))],
            TAIL: [("k_sample_bwd_tail", -(-B // 8))] if site == TAIL else None,
            L10: [("k_gemm_sample_bwd", -(-B // 16))] if site == L10 else None}
    got = {s: by_site.get(s) for s in want}
    bwd = f"NPA {inst['NPA']}" if site == TAIL else f"NST {inst['NST']}"
    print(f"\n[heads kernels] {what}: " + ", ".join(f"{s} {v}" for s, v in got.items() if v)
          + f"  (k_heads_sample<TN {inst['heads_TN']}, TM {inst['heads_TM']}>, backward {bwd})")
    assert got == want, (what, got, "wanted", want)


def check_exact_zeros(name, gg):
    """Clamped on every row: the log_std gradients are exactly zero; everything else is not."""
    lb, lw = gg["policy.log_std.bias"], gg["policy.log_std.weight"]
    for j in range(len(lb)):
        if j in ALL_CLAMPED:
            assert lb[j] == 0.0 and np.all(lw[j] == 0.0), (name, "clamped column", j, lb[j], np.abs(lw[j]).max())
        else:
            assert lb[j] != 0.0 and np.any(lw[j] != 0.0), (name, "column", j)
    assert np.all(gg["policy.mean.bias"] != 0.0) and np.all(np.any(gg["policy.mean.weight"] != 0.0, axis=1)), name


def check_columns(name, case, gg, g_truth, tb):
    """The per-column bars of the module docstring; returns the worst column error / e_ref /
    torch fp32 deviation per head tensor (for the record)."""
    cfg = case.cfg
    got = {k: gg[f"policy.{k}"] for k in HEAD_KEYS}
    want = {k: g_truth[f"policy.{k}"] for k in HEAD_KEYS}
    err = HM.column_errors(got, want, tb["scales"])
    print(f"\n[heads columns] {name}: per column, gpu vs fp64 | e_ref | torch fp32 step vs fp64")
    print("  col  " + "  ".join(f"{k:>32s}" for k in HEAD_KEYS))
    over = []
    for j in range(cfg.action_dim):
        cells = []
        for k in HEAD_KEYS:
            bar = max(GRAD_TOL, 4 * tb["e_ref"][k][j])
            ok = err[k][j] <= bar
            cells.append(f"{err[k][j]:9.2e} | {tb['e_ref'][k][j]:8.2e} | {tb['torch32'][k][j]:8.2e}{' ' if ok else '!'}")
            if not ok:
                over.append((j, k, float(err[k][j]), float(bar)))
        print(f"  {j:3d}  " + "  ".join(cells))
    worst = {k: (float(err[k].max()), float(tb["e_ref"][k].max()), float(tb["torch32"][k].max())) for k in HEAD_KEYS}
    print("  [heads summary] " + name + ": " + "; ".join(f"{k} {a:.1e} / {b:.1e} / {c:.1e}" for k, (a, b, c) in worst.items()))
    check_exact_zeros(name, gg)
    # column 3 sits exactly on -20 with a zero mean head: dls = -alpha / B on every row
    r = float(gg["policy.log_std.bias"][3]) / -cfg.alpha - 1.0
    print(f"  column 3 log_std.bias gradient / -alpha - 1 = {r:.2e}")
    assert abs(r) <= GRAD_TOL, (name, "column 3", r)
    assert not over, (name, "columns over their bar (col, tensor, error, bar)", over)
    # the remaining policy tensors and log_alpha, normwise
    bad = {}
    for k, e_ref in tb["e_ref_tensor"].items():
        if k.split(".", 1)[-1] in HEAD_KEYS:
            continue
        e = rel(gg[k], g_truth[k])
        print(f"  {k:24s} gpu {e:9.2e}  e_ref {e_ref:9.2e}  torch fp32 {rel(tb['g32'][k], tb['g64'][k]):9.2e}")
        if e > max(GRAD_TOL, 4 * e_ref):
            bad[k] = (e, e_ref)
    assert not bad, (name, bad)
    return worst


def check_losses(name, case, lg, tb):
    l64, t, cfg = tb["l64"], tb["truth"], case.cfg
    # the float32 model's own policy loss, to tell "clamp or bias wrong" from fp32 conditioning
    pl32 = float(np.mean(cfg.alpha * tb["model32"]["logp"].astype(np.float64) - t["q_new"]))
    print(f"  losses gpu vs fp64 (relative): "
          + ", ".join(f"{k} {abs(lg[i] - l64[k]) / max(abs(l64[k]), 1e-3):.2e}" for i, k in enumerate(l64))
          + f"; torch fp32 step: " + ", ".join(f"{abs(tb['l32'][k] - v) / max(abs(v), 1e-3):.2e}" for k, v in l64.items())
          + f"; float32 model policy_loss {abs(pl32 - l64['policy_loss']) / max(abs(l64['policy_loss']), 1e-3):.2e}")
    for i, k in enumerate(("q1_loss", "q2_loss", "policy_loss")):
        assert abs(lg[i] - l64[k]) <= LOSS_TOL * max(abs(l64[k]), 1e-3), (name, k, lg[i], l64[k])


@pytest.mark.parametrize("name", sorted(UPDATE_CASES))
def test_update_at_the_head_edges(name):
    """One update each (injected idx, eps1, eps2; state_scale 0.5), fp32: exact zeros, column 3,
    the per-column and per-tensor bars against fp64, q1 / q2 gradients at GRAD_TOL, the three
    losses at LOSS_TOL (both policy samples pass the doctored heads), and the head kernels the
    case is there for."""
    kw, dtype, site, want_inst = UPDATE_CASES[name]
    case = make_case(**kw)
    frac = assert_straddle_precondition(case)
    cfg, B = case.cfg, len(case.idx)
    ctx = make_ctx(cfg, max_batch=B, capacity=len(case.rows[2]), compute_dtype=dtype)
    load_params(ctx, case.params)
    ctx.push(*case.rows)
    lg = ctx.step(B, idx=case.idx, eps1=case.e1, eps2=case.e2)
    gg = ctx_grads(ctx, cfg)
    head_kernels(ctx, case, site, want_inst, name)
    ctx.close()
    tb = head_truth_tables(case)
    print(f"  bounds ({cfg.action_low}, {cfg.action_high}), straddle columns' inside fraction {frac}")
    check_losses(name, case, lg, tb)
    check_columns(name, case, gg, tb["g64"], tb)
    bad = {k: rel(gg[k], v) for k, v in tb["g64"].items() if k[:2] in ("q1", "q2") and rel(gg[k], v) > GRAD_TOL}
    print("  q1 / q2 gradients, worst tensor vs fp64: "
          f"{max(rel(gg[k], v) for k, v in tb['g64'].items() if k[:2] in ('q1', 'q2')):.2e}")
    assert not bad, (name, bad)


def test_update_at_the_head_edges_b4096():
    """Batch 4096 (k_heads_sample with 32 rows a workgroup, the standalone L10 at 256
    workgroups): the masked-truth helper of test_gpu_parity takes the losses and every gradient
    tensor (fp64 under the GPU's own ReLU masks, for the ReLU flips only); the exact zeros,
    column 3 and the per-column bars are then taken against that same masked truth."""
    from test_gpu_parity import check_update_under_gpu_masks, gpu_relu_masks
    kw, _, site, want_inst = B4096_FP32
    name = "A6-H64-B4096"
    case = make_case(**kw)
    frac = assert_straddle_precondition(case)
    cfg, B = case.cfg, len(case.idx)
    seen = {}

    def after_readback(ctx):
        seen["grads"] = ctx_grads(ctx, cfg)
        seen["masks"] = gpu_relu_masks(ctx, cfg, B)
        head_kernels(ctx, case, site, want_inst, name)
    # (the helper draws idx, eps1, eps2 from default_rng(103) as make_case does: the same minibatch)
    check_update_under_gpu_masks(cfg, case.params, case.rows, B, name, after_readback=after_readback)
    om = OracleSAC(cfg, case.params, torch.float64)
    om.step(*case.batch, case.e1, case.e2, masks=seen["masks"])
    tb = head_truth_tables(case)
    print(f"  straddle columns' inside fraction {frac}")
    check_columns(name, case, seen["grads"], om.grads_flat(), tb)


def test_update_at_the_head_edges_bf16_act16():
    """The H16 variants (bf16 activations: k_heads_sample<.., true, 32>, k_gemm_sample_bwd<..,
    true>) at (24, 23, 512), batch 4096: the exact zeros unchanged; losses and gradients against
    the bf16 emulation oracle at the bars of test_bf16_compute_vs_emulation.  The straddle
    precondition is taken on the emulation's head sums (h rounded to bf16, as the kernels read
    it)."""
    from test_gpu_parity import _check_bf16_update
    kw, dtype, site, want_inst = B4096_BF16
    name = "A23-H512-B4096-bf16"
    case = make_case(**kw)
    assert_straddle_precondition(case)
    cfg, B = case.cfg, len(case.idx)
    ctx = make_ctx(cfg, max_batch=B, capacity=len(case.rows[2]), compute_dtype=dtype)
    assert ctx.act16(B)
    load_params(ctx, case.params)
    ctx.push(*case.rows)
    lb = ctx.step(B, idx=case.idx, eps1=case.e1, eps2=case.e2)
    gb = ctx_grads(ctx, cfg)
    head_kernels(ctx, case, site, want_inst, name)
    ctx.close()
    check_exact_zeros(name, gb)
    emu = OracleSAC(cfg, case.params, torch.float64)
    l_emu = emu.step(*case.batch, case.e1, case.e2, bf16_operands=True, bf16_act=True)
    exact = OracleSAC(cfg, case.params, torch.float64)
    exact.step(*case.batch, case.e1, case.e2)
    _check_bf16_update(cfg, lb, gb, emu, exact, l_emu)


@pytest.mark.parametrize("A", [6, 17, 32])
def test_act_at_the_head_edges(A):
    """select_action on the doctored heads, bounds (-0.3, 0.9), n = 1 (k_act_heads) and n = 7,
    200 (k_heads_sample), stochastic with injected eps and deterministic: every action against
    fp64 _policy_sample at rtol 1e-5 / atol 1e-6 (test_select_action_stochastic_vs_oracle's);
    within one fp32 ulp of the bound where |x| >= 12; and inside the bounds as fp32 arithmetic
    has them, [fl(-scale + bias), fl(scale + bias)] (|tanh| <= 1 and rounding is monotone: no
    slack.  fl(0.6f + 0.3f) is one ulp above 0.9f, in the reference's fp32 too)."""
    from sacmi import Config, Context
    S, H, low, high = 24, 64, -0.3, 0.9
    cfg = SacConfig(S, A, H, action_low=low, action_high=high)
    params = init_params(cfg, 5, bias_scale=0.02)
    doctor_heads(params, A)
    ctx = Context(Config(S, A, H, max_batch=128, capacity=256, action_low=low, action_high=high), 0)
    for n in NETS:
        ctx.set_net(n, params[n])
    pol = {k: torch.tensor(v, dtype=torch.float64) for k, v in params["policy"].items()}
    sc32, bi32 = np.float32(cfg.action_scale), np.float32(cfg.action_bias)
    lo32, hi32 = np.float32(-sc32 + bi32), np.float32(sc32 + bi32)
    rng = np.random.default_rng(6)
    inst = instantiations(A, H, 64)
    for n in (1, 7, 200):
        st = (rng.standard_normal((n, S)) * 0.5).astype(np.float32)
        eps = rng.standard_normal((n, A)).astype(np.float32)
        if n == 1:
            eps[0, 0] = 3.0          # the one-state kernel saturated too: x = mean + 3 e^2 in column 0
        _, mean, ls_raw = policy_heads_fp64(params["policy"], st)
        for deterministic in (False, True):
            e = np.zeros_like(eps) if deterministic else eps
            got = ctx.act(st, deterministic=deterministic, eps=None if deterministic else eps)
            with torch.no_grad():
                want, _ = _policy_sample(pol, torch.from_numpy(st).double(), torch.from_numpy(e).double(),
                                         cfg.action_scale, cfg.action_bias)
            x = HM.forward(mean, ls_raw, e, cfg.action_scale, cfg.action_bias)["x"]
            what = f"A={A} n={n} {'deterministic' if deterministic else 'stochastic'}"
            print(f"[heads act] {what}: {'k_act_heads' if n == 1 else 'k_heads_sample<TN %d>' % inst['heads_TN']}, "
                  f"max |gpu - fp64| {np.abs(got - want.numpy()).max():.2e}, max |x| {np.abs(x).max():.1f}, "
                  f"{int((np.abs(x) >= 12).sum())} elements at |x| >= 12")
            assert got.shape == (n, A) and got.dtype == np.float32
            np.testing.assert_allclose(got, want.numpy(), rtol=1e-5, atol=1e-6, err_msg=what)
            assert np.all(got >= lo32) and np.all(got <= hi32), (what, got.min(), got.max())
            sat = np.abs(x) >= 12
            assert sat.any() or deterministic or n > 1, what
            bound = np.where(x > 0, np.float32(high), np.float32(low)).astype(np.float32)
            assert np.all(np.abs(got[sat] - bound[sat]) <= np.spacing(np.abs(bound[sat]))), what
    ctx.close()


def test_action_dim_33_is_rejected_at_create():
    """action_dim is capped at 32 (lp[TM][33], TM * 32 <= 64 * KSPLIT, kTailRows * A <= 256):
    sacmi_create refuses 33 with SACMI_EVALUE before any kernel that indexes by A can run, and
    a context at the limit itself, A = 32, then works."""
    from sacmi import Config, Context
    with pytest.raises(ValueError, match="action_dim"):
        Context(Config(24, 33, 64, max_batch=16, capacity=64), 0)
    ctx = Context(Config(24, 32, 64, max_batch=16, capacity=64), 0)
    params = init_params(SacConfig(24, 32, 64), 7, bias_scale=0.02)
    for n in NETS:
        ctx.set_net(n, params[n])
    a = ctx.act(np.zeros((1, 24), np.float32), deterministic=True)
    assert a.shape == (1, 32) and np.all(np.isfinite(a)) and np.all(np.abs(a) <= np.float32(0.4))
    ctx.close()
