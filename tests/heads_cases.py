"""Doctored policy heads for the sample-head edge tests (test_heads_model.py on the CPU,
test_gpu_heads.py on the GPU): columns that sit beyond, exactly on and across the log_std
clamp bounds, saturated tanh columns, and asymmetric action bounds.

  col  log_std head                mean head           exercises
  0    bias 5                      as drawn            every row clamped high, sd = e^2
  1    bias -30                    weights, bias 0     every row clamped low; mean = 0: x - mean exact
  2    weights 0, bias 2.0         as drawn            exactly on the upper bound: gradient passes
  3    weights 0, bias -20.0       weights, bias 0     exactly on the lower bound: gradient passes
  4    bias 2.0, weights drawn     as drawn            rows straddle the upper bound
  5    bias -20.0, weights drawn   weights, bias 0     rows straddle the lower bound
  6,7  as drawn                    bias 6 / -12        tanh saturated (|x| ~ 6, 12) at ordinary sd
  rest as drawn                    as drawn            control
(columns beyond action_dim are dropped; action_dim >= 6.)

The straddle columns carry a precondition: no row's fp64 log_std sum may lie within
MARGIN * (sum_k |h_k||w_k| + |b|) of its bound, so that an fp32 evaluation can never
legitimately take another clamp decision than fp64 and no element needs leaving out.  The
replay rows of a case are the candidates that satisfy it (for s and s', both policy passes);
the tests assert it again on the minibatch they run."""
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

import oracle.sac_step as osm
from oracle import heads_model as HM
from oracle.sac_step import OracleSAC, SacConfig, init_params, synthetic_rows

STRADDLE = {4: 2.0, 5: -20.0}        # column -> the bound its rows straddle
ALL_CLAMPED = (0, 1)                 # columns whose log_std gradients are exactly zero
MARGIN = 1e-4
HEAD_KEYS = ("mean.weight", "mean.bias", "log_std.weight", "log_std.bias")


def doctor_heads(params: dict, A: int) -> None:
    assert A >= 6
    pol = params["policy"]
    mw, mb, lw, lb = (pol[k] for k in HEAD_KEYS)

    def zero_mean(j):
        mw[j] = 0.0
        mb[j] = 0.0
    lb[0] = 5.0
    lb[1] = -30.0; zero_mean(1)
    lw[2] = 0.0; lb[2] = 2.0
    lw[3] = 0.0; lb[3] = -20.0; zero_mean(3)
    lb[4] = 2.0
    lb[5] = -20.0; zero_mean(5)
    if A > 6:
        mb[6] = 6.0
    if A > 7:
        mb[7] = -12.0


def policy_heads_fp64(pol: dict, states, bf16_operands=False, bf16_act=False):
    """(h, mean, ls_raw) of the policy in float64 (numpy): the last hidden activations and the
    two head sums before the clamp.  bf16_*: under the oracle's bf16 operand emulation."""
    p = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in pol.items()}
    x = torch.as_tensor(np.asarray(states, np.float32)).double()
    osm._ROUND["on"], osm._ROUND["act"] = bool(bf16_operands), bool(bf16_act)
    try:
        with torch.no_grad():
            for i in range(1, osm._n_hidden(p) + 1):
                x = F.relu(osm._lin(x, p[f"fc{i}.weight"], p[f"fc{i}.bias"], "in" if i == 1 else "hid"))
            if bf16_operands and bf16_act:
                x = osm._bf(x)
            mean = osm._lin(x, p["mean.weight"], p["mean.bias"], "head")
            ls_raw = osm._lin(x, p["log_std.weight"], p["log_std.bias"], "head")
    finally:
        osm._ROUND["on"] = osm._ROUND["act"] = False
    return x.numpy(), mean.numpy(), ls_raw.numpy()


def straddle_clearance(pol: dict, h, ls_raw) -> np.ndarray:
    """[rows, 2]: |ls_raw - bound| / (sum_k |h_k||w_k| + |b|) of the two straddle columns."""
    out = []
    for j, bound in STRADDLE.items():
        w = np.abs(np.asarray(pol["log_std.weight"][j], np.float64))
        scale = np.abs(h) @ w + abs(float(pol["log_std.bias"][j]))
        out.append(np.abs(ls_raw[:, j] - bound) / scale)
    return np.stack(out, 1)


@dataclass
class HeadCase:
    cfg: SacConfig
    params: dict
    rows: tuple
    idx: np.ndarray
    e1: np.ndarray
    e2: np.ndarray
    bf16_act: object = None          # None: exact operands; else the bf16 emulation's bf16_act

    @property
    def batch(self):
        return [x[self.idx] for x in self.rows]


def make_case(S, A, H, B, n_hidden=2, bounds=(-0.3, 0.9), seed=0, state_scale=0.5, bf16_act=None,
              draw_seed=103) -> HeadCase:
    """Doctored heads on init_params(seed, bias_scale 0.02); replay rows: the synthetic
    candidates that keep the straddle precondition; minibatch and noise drawn as
    test_gpu_parity.check_update_under_gpu_masks draws them (idx, eps1, eps2 from
    default_rng(draw_seed))."""
    cfg = SacConfig(S, A, H, n_hidden=n_hidden, action_low=bounds[0], action_high=bounds[1])
    params = init_params(cfg, seed, bias_scale=0.02)
    doctor_heads(params, A)
    cand = synthetic_rows(cfg, 2 * B + 600, seed + 1, state_scale=state_scale)
    emu = dict(bf16_operands=bf16_act is not None, bf16_act=bool(bf16_act))
    ok = np.ones(len(cand[2]), bool)
    for st in (cand[0], cand[3]):
        h, _, ls_raw = policy_heads_fp64(params["policy"], st, **emu)
        ok &= (straddle_clearance(params["policy"], h, ls_raw) > 2 * MARGIN).all(1)
    keep = np.flatnonzero(ok)[:B + B // 4 + 16]
    assert len(keep) >= B, (len(keep), B)
    rows = tuple(x[keep] for x in cand)
    rng = np.random.default_rng(draw_seed)
    idx = rng.choice(len(keep), B, replace=False)
    e1 = rng.standard_normal((B, A)).astype(np.float32)
    e2 = rng.standard_normal((B, A)).astype(np.float32)
    return HeadCase(cfg, params, rows, idx, e1, e2, bf16_act)


def assert_straddle_precondition(case: HeadCase) -> dict:
    """On the minibatch's actor rows (the backward's mask decisions) and next-state rows:
    clearance > MARGIN everywhere, and at least 10 % of the actor rows on either side of each
    straddled bound.  Returns the inside-fraction per straddle column."""
    s, _, _, s2, _ = case.batch
    emu = dict(bf16_operands=case.bf16_act is not None, bf16_act=bool(case.bf16_act))
    pol = case.params["policy"]
    frac = {}
    for st, actor in ((s, True), (s2, False)):
        h, _, ls_raw = policy_heads_fp64(pol, st, **emu)
        c = straddle_clearance(pol, h, ls_raw)
        assert c.min() > MARGIN, ("a row within the margin of a clamp bound", c.min())
        if actor:
            for j in STRADDLE:
                inside = float(HM.clamp_mask(ls_raw[:, j]).mean())
                assert 0.1 <= inside <= 0.9, (j, inside)
                frac[j] = inside
    return frac


def actor_truth(case: HeadCase, critics: dict, alpha: float) -> dict:
    """The actor pass's head-level quantities in float64 on the case's minibatch: h, mean,
    ls_raw, the model's forward, ga = dL/da of L = mean(alpha * logp - min Q) through
    ``critics`` ({"q1", "q2"}: the critics AFTER their update, as the step uses them),
    glogp = alpha / B, and the model's dhead."""
    cfg = case.cfg
    s = case.batch[0]
    B = len(s)
    h, mean, ls_raw = policy_heads_fp64(case.params["policy"], s)
    fwd = HM.forward(mean, ls_raw, case.e2, cfg.action_scale, cfg.action_bias)
    a = torch.tensor(fwd["action"], dtype=torch.float64, requires_grad=True)
    st = torch.as_tensor(s).double()
    q = {n: {k: torch.as_tensor(np.asarray(v.detach() if torch.is_tensor(v) else v)).double()
             for k, v in critics[n].items()} for n in ("q1", "q2")}
    q_new = torch.min(osm._q_forward(q["q1"], st, a), osm._q_forward(q["q2"], st, a))
    (-q_new.mean()).backward()
    ga = a.grad.numpy()
    glogp = float(alpha) / B
    dmean, dls = HM.backward(fwd, ga, glogp, cfg.action_scale)
    return dict(h=h, mean=mean, ls_raw=ls_raw, fwd=fwd, ga=ga, glogp=glogp, dmean=dmean, dls=dls,
                q_new=q_new.detach().numpy().reshape(-1))


def policy_grads_from_dhead(case: HeadCase, dmean, dls) -> dict:
    """Every policy gradient tensor of a given dhead, the layers in float64 (autograd of
    sum(dhead * [mean | ls_raw]) through the policy on the actor rows)."""
    p = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True)
         for k, v in case.params["policy"].items()}
    x = torch.as_tensor(case.batch[0]).double()
    for i in range(1, osm._n_hidden(p) + 1):
        x = F.relu(F.linear(x, p[f"fc{i}.weight"], p[f"fc{i}.bias"]))
    mean = F.linear(x, p["mean.weight"], p["mean.bias"])
    ls_raw = F.linear(x, p["log_std.weight"], p["log_std.bias"])
    ((mean * torch.as_tensor(np.asarray(dmean, np.float64))).sum()
     + (ls_raw * torch.as_tensor(np.asarray(dls, np.float64))).sum()).backward()
    return {k: v.grad.numpy() for k, v in p.items()}


def head_truth_tables(case: HeadCase, alpha=None) -> dict:
    """One fp64 oracle update of the case plus everything the per-column bars need: the
    oracle (after its step) and its losses and gradients, the actor pass's head quantities,
    the columns' scales, e_ref per column (the model in float32 against float64) and per
    remaining policy tensor (the float32 model's dhead pushed through float64 layers), and
    the torch fp32 step's own deviation on the same scales, for the record."""
    cfg = case.cfg
    alpha = cfg.alpha if alpha is None else alpha
    o64 = OracleSAC(cfg, case.params, torch.float64)
    l64 = o64.step(*case.batch, case.e1, case.e2)
    g64 = o64.grads_flat()
    t = actor_truth(case, {n: o64.nets[n] for n in ("q1", "q2")}, alpha)
    scales = HM.column_scales(t["dmean"], t["dls"], t["h"])
    args = (t["mean"], t["ls_raw"], case.e2, t["ga"], t["glogp"], cfg.action_scale, cfg.action_bias)
    e_ref = HM.e_ref_columns(*args, t["h"])
    f32 = HM.forward(*args[:3], cfg.action_scale, cfg.action_bias, np.float32)
    d32 = HM.backward(f32, t["ga"], t["glogp"], cfg.action_scale)
    gp64 = policy_grads_from_dhead(case, t["dmean"], t["dls"])
    gp32 = policy_grads_from_dhead(case, *d32)
    e_ref_tensor = {f"policy.{k}": np.linalg.norm(gp32[k] - gp64[k]) / max(np.linalg.norm(gp64[k]), 1e-300)
                    for k in gp64}
    # dL/dlog_alpha = -mean(logp + target_entropy) (sac_imp.py:128-131)
    ga64 = -(t["fwd"]["logp"].mean() - cfg.action_dim)
    ga32 = -(f32["logp"].astype(np.float64).mean() - cfg.action_dim)
    e_ref_tensor["log_alpha"] = abs(ga32 - ga64) / abs(ga64)
    o32 = OracleSAC(cfg, case.params, torch.float32)
    l32 = o32.step(*case.batch, case.e1, case.e2)
    g32 = o32.grads_flat()
    heads64 = {k: g64[f"policy.{k}"] for k in HEAD_KEYS}
    torch32 = HM.column_errors({k: g32[f"policy.{k}"] for k in HEAD_KEYS}, heads64, scales)
    # the plumbing of this table itself: the model's dhead through fp64 layers IS the oracle's step
    for k in gp64:
        d = np.linalg.norm(gp64[k] - g64[f"policy.{k}"]) / max(np.linalg.norm(g64[f"policy.{k}"]), 1e-300)
        assert d <= 1e-6, ("model dhead through fp64 layers vs the fp64 oracle", k, d)
    return dict(o64=o64, l64=l64, g64=g64, l32=l32, g32=g32, truth=t, scales=scales, e_ref=e_ref,
                e_ref_tensor=e_ref_tensor, torch32=torch32, model32=f32)
