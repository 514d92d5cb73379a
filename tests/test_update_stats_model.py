"""The diagnostics model (tests/update_stats_model.py) against the update's own losses, and the
ABI surface of the feature.  No GPU.

The statistics are tied to the three losses the reference returns by identities that hold in
exact arithmetic; in fp64 they hold to 1e-12 relative:
    policy_loss = -alpha entropy - q_pi_mean                       (sac_imp.py:119)
    q1_loss     = mean((q1 - q^)^2) with weights all one            (sac_imp.py:101)
    alpha_loss  = -log_alpha (-entropy - action_dim)                (sac_imp.py:130)
    td_max >= td_mean >= 0
"""
import os
import re

import numpy as np
import pytest
import torch

from oracle.sac_step import OracleSAC, SacConfig, init_params, synthetic_rows

from update_stats_model import STAT_NAMES, StatsSAC, stat_scales, stats_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, A, H, B = 11, 3, 96, 40


def _inputs(n_hidden, auto):
    cfg = SacConfig(S, A, H, n_hidden=n_hidden, automatic_entropy_tuning=auto)
    params = init_params(cfg, 31 + n_hidden, bias_scale=0.05)
    rows = synthetic_rows(cfg, B, 77, state_scale=0.5)
    rng = np.random.default_rng(5)
    eps = [rng.standard_normal((B, A)).astype(np.float32) for _ in range(4)]
    return cfg, params, rows, eps


def _close(a, b, what):
    assert abs(a - b) <= 1e-12 * max(abs(a), abs(b), 1e-300), (what, a, b)


@pytest.mark.parametrize("auto", [True, False])
@pytest.mark.parametrize("n_hidden", [2, 3])
def test_identities_fp64(n_hidden, auto):
    """Two updates (the second with log_alpha off 0 when entropy tuning is on): the statistics
    reproduce the update's losses, and the model's losses and parameters are OracleSAC's."""
    cfg, params, rows, eps = _inputs(n_hidden, auto)
    m = StatsSAC(cfg, params, torch.float64)
    ref = OracleSAC(cfg, params, torch.float64)
    for u in range(2):
        e1, e2 = eps[2 * u], eps[2 * u + 1]
        alpha0, la0 = m.state()["alpha"].item(), m.log_alpha.item()
        out = m.step(*rows, e1, e2)
        want = ref.step(*rows, e1, e2)
        for k in ("q1_loss", "q2_loss", "policy_loss"):
            assert out[k] == want[k], (u, k)
        st = out["stats"]
        assert tuple(st) == STAT_NAMES
        assert st["alpha"] == alpha0 and st["log_alpha"] == la0
        _close(out["policy_loss"], -st["alpha"] * st["entropy"] - st["q_pi_mean"], "policy_loss")
        _close(st["alpha_loss"], -st["log_alpha"] * (-st["entropy"] - A) if auto else 0.0, "alpha_loss")
        assert st["td_max"] >= st["td_mean"] >= 0.0
        assert st["batch"] == B
        _close(st["reward_mean"], float(np.mean(rows[2].astype(np.float64))), "reward_mean")
        _close(st["td_mean"], float(out["td"].mean()), "td_mean")
        assert st["td_max"] == out["td"].max()
        if auto and u == 1:
            assert la0 != 0.0 and st["alpha_loss"] != 0.0 and alpha0 != cfg.alpha
        if not auto:
            assert st["alpha"] == cfg.alpha and st["log_alpha"] == 0.0
        sc = stat_scales(out)
        assert np.all(np.isnan(sc[[7, 8, 10, 11]])) and np.all(sc[[0, 1, 2, 3, 4, 5, 6, 9]] > 0)
        assert out["scales"]["q_max"] >= out["scales"]["q"]
        assert np.all(np.isfinite(stats_row(out)))
    sa, sb = m.state(), ref.state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k


@pytest.mark.parametrize("n_hidden", [2, 3])
def test_q_loss_is_the_mean_square_of_the_rows(n_hidden):
    """With weights all one q_i_loss = mean((q_i - q^)^2): recomputed from the model's own rows
    (a second model instance evaluates q1, q2, q^ without stepping)."""
    from oracle.sac_step import _policy_sample, _q_forward
    cfg, params, rows, eps = _inputs(n_hidden, True)
    m = StatsSAC(cfg, params, torch.float64)
    out = m.step(*rows, eps[0], eps[1])
    w1 = StatsSAC(cfg, params, torch.float64)
    w1.weights = np.ones(B, np.float32)
    out1 = w1.step(*rows, eps[0], eps[1])
    assert out1["q1_loss"] == out["q1_loss"] and out1["q2_loss"] == out["q2_loss"]
    f = StatsSAC(cfg, params, torch.float64)            # fresh: the parameters before the step
    T = lambda x: torch.as_tensor(np.asarray(x, np.float32)).to(torch.float64)
    s, a, r, s2, d = rows
    with torch.no_grad():
        na, nlp = _policy_sample(f.nets["policy"], T(s2), T(eps[0]), cfg.action_scale, cfg.action_bias)
        qt = torch.min(_q_forward(f.nets["q1_target"], T(s2), na), _q_forward(f.nets["q2_target"], T(s2), na))
        qhat = T(r).reshape(-1, 1) + (1 - T(d).reshape(-1, 1)) * cfg.gamma * (qt - cfg.alpha * nlp)
        q1 = _q_forward(f.nets["q1"], T(s), T(a))
        q2 = _q_forward(f.nets["q2"], T(s), T(a))
    _close(out["q1_loss"], ((q1 - qhat) ** 2).mean().item(), "q1_loss")
    _close(out["q2_loss"], ((q2 - qhat) ** 2).mean().item(), "q2_loss")
    _close(out["stats"]["q1_mean"], q1.mean().item(), "q1_mean")
    _close(out["stats"]["q_target_mean"], qhat.mean().item(), "q_target_mean")
    # the weights reach the losses and never the statistics
    w2 = StatsSAC(cfg, params, torch.float64)
    w2.weights = np.linspace(0.1, 1.0, B).astype(np.float32)
    out2 = w2.step(*rows, eps[0], eps[1])
    assert abs(out2["q1_loss"] - out["q1_loss"]) > 1e-2 * abs(out["q1_loss"])
    for k in ("q1_mean", "q2_mean", "q_target_mean", "td_mean", "td_max", "reward_mean"):
        assert out2["stats"][k] == out["stats"][k], k


def test_abi_surface():
    """The three functions are exported, the names tuple has the header's twelve columns in id
    order, and the ABI version stays 3 (the feature is additive)."""
    from sacmi import _lib as L
    for fn in ("sacmi_set_stats", "sacmi_stats", "sacmi_fetch_stats"):
        assert fn in L.EXPORTS, fn
    assert len(L.STAT_NAMES) == 12 and L.STAT_NAMES == STAT_NAMES
    hdr = open(os.path.join(ROOT, "include", "sacmi.h")).read()
    ids = dict(re.findall(r"SACMI_STAT_([A-Z0-9_]+) = (\d+)", hdr))
    assert int(ids.pop("COUNT")) == 12
    assert [k.lower() for k, v in sorted(ids.items(), key=lambda kv: int(kv[1]))] == list(L.STAT_NAMES)
    assert sorted(int(v) for v in ids.values()) == list(range(12))
    assert re.search(r"#define\s+SACMI_ABI_VERSION\s+3\b", hdr)
    assert L.ABI_VERSION == 3
    assert L.TL_KINDS[max(L.TL_KINDS)] == "k_update_stats"
