"""oracle/heads_model.py (the analytic sample-head model the GPU head tests are graded with)
against torch float64 autograd of oracle.sac_step._policy_sample, on the doctored head
columns of tests/heads_cases.py: log_std beyond, exactly on and across both clamp bounds, tanh
saturated at |x| ~ 6 and 12, action bounds (-0.3, 0.9).

The tie is elementwise, float64 against float64, at 1e-12 relative.  Two of the REFERENCE's
own float64 forms are ill-conditioned on these columns, and their rounding is added to the bar
as explicit terms (they vanish, well below 1e-12, everywhere else):
  * 1 - y^2 carries an absolute error of up to ~2^-51 (y rounded at ulp(1)/2, squared,
    rounded again; beyond |x| = 19 it is exactly 0); it multiplies G in dmean = G (1 - y^2)
    (relative 2^-51 / omy2: 1.8e-11 at |x| = 6, 2.8e-6 at |x| = 12) and enters
    u = scale (1 - y^2) + 1e-6 inside the log and the 1 / u;
  * autograd forms dmean as (G + T) - T with T = glogp eps / sd, the quadratic term's gradient
    (5e8 glogp at sd = e^-20): an absolute error of up to ~ulp(T).
The model's own forms have neither problem: evaluated in extended precision (x86 long double)
it moves by less than 1e-12 on every element, which test_model_is_well_conditioned asserts, so
on those columns the model is the better truth of the two and the bar is the reference's noise.
The log_std gradient — the clamp mask's subject — needs no such term beyond the 1 - y^2 one.
"""
import numpy as np
import pytest
import torch

from heads_cases import ALL_CLAMPED, STRADDLE, assert_straddle_precondition, head_truth_tables, make_case
from oracle import heads_model as HM
from oracle.sac_step import _policy_sample

TIE = 1e-12
DELTA = 2.0 ** -51        # |fl(1 - fl(y)^2) - (1 - y^2)| in float64, y = tanh(x) in (-1, 1)
ULP = 2.0 ** -52

CASES = {"A6": dict(S=20, A=6, H=64, B=64, seed=1),
         "A17": dict(S=24, A=17, H=512, B=100, seed=1)}


@pytest.fixture(scope="module", params=sorted(CASES))
def tables(request):
    case = make_case(**CASES[request.param])
    frac = assert_straddle_precondition(case)
    return request.param, case, head_truth_tables(case), frac


def torch_dhead(case, t, dtype=torch.float64):
    """(action, logp, dmean, dls) of _policy_sample by torch autograd, per element: the policy
    is the identity 'network' state = I, mean.weight = mean^T, log_std.weight = ls_raw^T (the
    head sums come out exactly, products by 0 and 1), so the weights' gradients are dhead^T.
    L = glogp sum(logp) + sum(ga * action)."""
    B, A = t["mean"].shape
    T = lambda v: torch.tensor(np.asarray(v), dtype=dtype)
    p = {"mean.weight": T(t["mean"].T).requires_grad_(True), "mean.bias": torch.zeros(A, dtype=dtype),
         "log_std.weight": T(t["ls_raw"].T).requires_grad_(True), "log_std.bias": torch.zeros(A, dtype=dtype)}
    action, logp = _policy_sample(p, torch.eye(B, dtype=dtype), T(case.e2), case.cfg.action_scale,
                                  case.cfg.action_bias)
    (t["glogp"] * logp.sum() + (T(t["ga"]) * action).sum()).backward()
    return (action.detach().numpy(), logp.detach().numpy().reshape(-1),
            p["mean.weight"].grad.numpy().T, p["log_std.weight"].grad.numpy().T)


def tie_excess(case, t, mask=None):
    """max over the elements of |model - torch fp64| / bar, per quantity (<= 1: tied)."""
    cfg = case.cfg
    fwd = t["fwd"]
    dmean, dls = HM.backward(fwd, t["ga"], t["glogp"], cfg.action_scale, mask=mask)
    action, logp, dmean_t, dls_t = torch_dhead(case, t)
    sc = cfg.action_scale
    u = sc * fwd["omy2"] + 1e-6
    # |G| term by term: the reference's error in 1 - y^2 is absolute, so it scales with G, not
    # with dmean = G omy2 (at |x| > 19 its 1 - y^2 is exactly 0 and so is its dmean)
    G_abs = np.abs(sc * t["ga"]) + abs(t["glogp"]) * 2 * sc * np.abs(fwd["y"]) / u
    T_quad = abs(t["glogp"]) * np.abs(fwd["eps"]) / fwd["sd"]
    bars = {"action": TIE * np.abs(action),
            "logp": TIE * np.abs(logp) + (sc * DELTA / u).sum(1),
            "dmean": TIE * np.abs(dmean_t) + 2 * DELTA * G_abs + 4 * ULP * T_quad,
            "dls": TIE * np.abs(dls_t) + 2 * DELTA * G_abs * np.abs(fwd["eps"]) * fwd["sd"]}
    got = {"action": fwd["action"], "logp": fwd["logp"], "dmean": dmean, "dls": dls}
    want = {"action": action, "logp": logp, "dmean": dmean_t, "dls": dls_t}
    out = {}
    for k in bars:
        d = np.abs(got[k] - want[k])
        out[k] = float(np.max(np.where(d == 0, 0.0, d / np.maximum(bars[k], 1e-300))))
    return out, (dmean_t, dls_t)


def test_model_matches_torch_fp64_autograd(tables):
    """Measured: the worst element sits at 0.21 of its bar (logp), 0.13 (dmean, dls)."""
    name, case, tb, frac = tables
    t = tb["truth"]
    excess, (dmean_t, dls_t) = tie_excess(case, t)
    print(f"\n[heads model] {name}: |model - torch fp64| / bar, worst element: "
          + ", ".join(f"{k} {v:.2f}" for k, v in excess.items())
          + f"; inside fraction of the straddle columns {frac}")
    assert max(excess.values()) <= 1.0, excess
    # where neither ill-conditioned reference form is in play the tie is the plain 1e-12:
    # every column's log_std gradient at ordinary |x|, and dmean at ordinary sd
    plain = (np.abs(t["fwd"]["x"]) < 3.0)
    rel = np.abs(t["dls"] - dls_t) / np.maximum(np.abs(dls_t), 1e-300)
    assert np.all(rel[plain & (dls_t != 0)] <= TIE), rel[plain].max()
    # the clamp's edges, in both evaluations: beyond a bound exactly zero, on it not
    for j in ALL_CLAMPED:
        assert np.all(t["dls"][:, j] == 0.0) and np.all(dls_t[:, j] == 0.0), j
    for j, bound in ((2, 2.0), (3, -20.0)):
        assert np.all(t["ls_raw"][:, j] == bound), j
        assert np.all(t["dls"][:, j] != 0.0) and np.all(dls_t[:, j] != 0.0), j
    for j in STRADDLE:
        m = HM.clamp_mask(t["ls_raw"][:, j]) > 0
        assert np.all(t["dls"][~m, j] == 0.0) and np.all(dls_t[~m, j] == 0.0), j
        assert np.all(t["dls"][m, j] != 0.0), j
    # column 3: the log_std.bias gradient is -alpha (the sd term is 2e-9 of it)
    assert abs(t["dls"][:, 3].sum() / -case.cfg.alpha - 1) <= 1e-8


def test_mask_is_inclusive_and_from_the_raw_value():
    lo, hi = np.float64(HM.LS_MIN), np.float64(HM.LS_MAX)
    ls = np.array([lo, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf), 5.0, -30.0, 0.0])
    assert HM.clamp_mask(ls).tolist() == [1, 1, 0, 0, 0, 0, 1]
    lo, hi = np.float32(HM.LS_MIN), np.float32(HM.LS_MAX)
    ls = np.array([lo, hi, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))], np.float32)
    assert HM.clamp_mask(ls).tolist() == [1, 1, 0, 0] and HM.clamp_mask(ls).dtype == np.float32
    # a value beyond the bound has a clamped value inside: the mask must not be taken from that
    f = HM.forward(np.zeros(2), np.array([5.0, -30.0]), np.ones(2), 0.6, 0.3)
    assert f["ls"].tolist() == [2.0, -20.0]
    _, dls = HM.backward(f, np.ones(2), 0.01, 0.6)
    assert dls.tolist() == [0.0, 0.0]


BROKEN = {"strict inequality": lambda ls_raw, ls: (ls_raw > HM.LS_MIN) & (ls_raw < HM.LS_MAX),
          "mask from the clamped value": lambda ls_raw, ls: (ls >= HM.LS_MIN) & (ls <= HM.LS_MAX),
          "no mask": lambda ls_raw, ls: np.ones_like(ls_raw, bool)}


@pytest.mark.parametrize("how", sorted(BROKEN))
def test_a_broken_mask_breaks_the_tie(tables, how):
    """The tie is sharp enough to catch each wrong mask: by a factor of 1e6 at the least."""
    name, case, tb, _ = tables
    t = tb["truth"]
    mask = BROKEN[how](t["ls_raw"], t["fwd"]["ls"]).astype(np.float64)
    excess, _ = tie_excess(case, t, mask=mask)
    print(f"\n[heads model] {name}, {how}: dls excess {excess['dls']:.3g}")
    assert excess["dls"] > 1e6, (how, excess)


def test_model_is_well_conditioned(tables):
    """float64 against x86 extended precision, every element at 1e-12 relative with no extra
    term: the model's forms do not cancel where the reference's do."""
    if np.finfo(np.longdouble).eps > 2.0 ** -60:
        return   # no extended-precision long double on this platform: nothing to compare with
    name, case, tb, _ = tables
    t, cfg = tb["truth"], case.cfg
    args = (t["mean"], t["ls_raw"], case.e2, cfg.action_scale, cfg.action_bias)
    fx = HM.forward(*args, np.longdouble)
    dx = HM.backward(fx, t["ga"], t["glogp"], cfg.action_scale)
    worst = {}
    for k, a, b in (("action", t["fwd"]["action"], fx["action"]), ("logp_elem", t["fwd"]["logp_elem"], fx["logp_elem"]),
                    ("omy2", t["fwd"]["omy2"], fx["omy2"]), ("dmean", t["dmean"], dx[0]), ("dls", t["dls"], dx[1])):
        b = np.asarray(b, np.longdouble)
        d = np.abs(np.asarray(a, np.longdouble) - b)
        worst[k] = float(np.max(np.where(d == 0, 0, d / np.maximum(np.abs(b), np.longdouble(1e-300)))))
    print(f"\n[heads model] {name}: float64 vs long double, worst relative element: "
          + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) <= TIE, worst


def test_e_ref_table(tables):
    """e_ref per column (the model in float32 against float64, on the column's own scale): the
    yardstick of the GPU head tests — next to the torch fp32 step's deviation from the fp64
    step on the same scale, which is why the latter is not used there.  e_ref is rounding
    noise: each of the model's ~10 operations rounds at 2^-24, and exp(-2|x|) turns the
    rounding of x into 2|x| 2^-24, so it is held to (16 + 4 max|x|) 2^-24 per column.
    Measured (S 20 / A 6 / H 64 / B 64 and S 24 / A 17 / H 512 / B 100, bounds (-0.3, 0.9)):
    e_ref 1e-9 .. 1.7e-7 on every column; the torch fp32 step 0.14 .. 1.0 on the mean head of
    the low-clamp columns 1, 3, 5 and of column 7 (|x| ~ 12), 1e-4 .. 1e-3 on columns 0, 2, 4,
    6, 1e-3 .. 5e-3 on the log_std head of columns 2, 4, 6, 7, and 3e-7 .. 3e-5 on the control
    columns; its losses 3.6e-5 / 5.3e-5 (q1, q2) and 1.5e-5 / 2.1e-5 (policy) from fp64."""
    name, case, tb, _ = tables
    t = tb["truth"]
    A = case.cfg.action_dim
    xmax = np.abs(t["fwd"]["x"]).max(0)
    print(f"\n[heads e_ref] {name}: per column, e_ref (model fp32 vs fp64) | torch fp32 step vs fp64 step")
    print("  col  max|x|   " + "   ".join(f"{k:>21s}" for k in tb["e_ref"]))
    for j in range(A):
        print(f"  {j:3d}  {xmax[j]:6.2f}   "
              + "   ".join(f"{tb['e_ref'][k][j]:9.2e} | {tb['torch32'][k][j]:9.2e}" for k in tb["e_ref"]))
    print("  remaining tensors, normwise: "
          + ", ".join(f"{k} {v:.2e}" for k, v in tb["e_ref_tensor"].items()))
    print(f"  losses, torch fp32 vs fp64 (relative): "
          + ", ".join(f"{k} {abs(tb['l32'][k] - v) / abs(v):.2e}" for k, v in tb["l64"].items()))
    for k, e in tb["e_ref"].items():
        assert np.all(np.isfinite(e)), (k, e)
        assert np.all(e <= (16 + 4 * xmax) * 2.0 ** -24), (k, e, xmax)
        for j in ALL_CLAMPED:
            if k.startswith("log_std"):
                assert e[j] == 0.0, (k, j)
