"""Model of the per-update training diagnostics (include/sacmi.h enum sacmi_stat): the twelve
statistics of one SAC update (sac_imp.py:74-144), in the oracle's arithmetic.

    q^          = r + (1 - d) gamma (min(q1t, q2t)(s', a') - alpha log pi(a'|s'))   sac_imp.py:87-98
    td          = 0.5 (|q1 - q^| + |q2 - q^|)                 per row, unweighted
    q_pi        = min(q1, q2)(s, a~) on the critics AFTER their step            sac_imp.py:117-119
    entropy     = -mean log pi(a~|s)
    alpha_loss  = -log_alpha mean(log pi(a~|s) + target_entropy)                 sac_imp.py:128-131
    alpha, log_alpha: as the update's losses used them (before its alpha step)

TEST INFRASTRUCTURE ONLY: ``StatsSAC`` is ``oracle.sac_step.OracleSAC`` whose ``step`` also
returns the statistics under "stats" (name -> float, computed in the model's dtype) and the
scales the GPU tests measure errors on under "scales".  It reuses ``_policy_sample`` /
``_q_forward`` with their tags, so ``bf16_operands``, ``bf16_act`` and ``masks`` work as on the
oracle.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle.sac_step import OracleSAC, _policy_sample, _q_forward, q_keys

STAT_NAMES = ("q1_mean", "q2_mean", "q_target_mean", "td_mean", "td_max", "q_pi_mean", "entropy",
              "alpha", "log_alpha", "alpha_loss", "reward_mean", "batch")
# which scale a statistic's error is measured on (None: compared exactly / to the ulp)
STAT_SCALE = {"q1_mean": "q", "q2_mean": "q", "q_target_mean": "q", "td_mean": "q", "td_max": "q_max",
              "q_pi_mean": "q", "entropy": "logp", "alpha_loss": "logp"}


def _scalar(x) -> float:
    return float(x.detach()) if torch.is_tensor(x) else float(x)


class StatsSAC(OracleSAC):
    """OracleSAC whose ``step`` returns, next to the losses, "stats" (STAT_NAMES -> float),
    "scales" ({"q": mean over rows of |q1| + |q2| + |q^|, "q_max": its maximum, "logp": mean
    |log pi(a~|s)| + action_dim}) and the per-row "td".  ``weights`` ([B], default all ones)
    weight the critic losses as FeedbackSAC's do; the statistics never carry them."""
    weights = None

    def _step(self, s, a, r, s2, d, eps1, eps2) -> dict:
        cfg, dt = self.cfg, self.dtype
        T = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float32)).to(dt)
        state, action, next_state = T(s), T(a), T(s2)
        reward = T(r).reshape(-1, 1)
        done = T(d).reshape(-1, 1)
        e1, e2 = T(eps1), T(eps2)
        w = torch.ones_like(reward) if self.weights is None else T(self.weights).reshape(-1, 1)
        P, Q1, Q2 = self.nets["policy"], self.nets["q1"], self.nets["q2"]
        sc, bi = cfg.action_scale, cfg.action_bias
        st = {"alpha": _scalar(self.alpha), "log_alpha": self.log_alpha.item()}
        with torch.no_grad():
            na, nlp = _policy_sample(P, next_state, e1, sc, bi, "pi_s2")
            q1n = _q_forward(self.nets["q1_target"], next_state, na, "q1t")
            q2n = _q_forward(self.nets["q2_target"], next_state, na, "q2t")
            value_target = torch.min(q1n, q2n) - self.alpha * nlp
            q_target = reward + (1 - done) * cfg.gamma * value_target
        q1 = _q_forward(Q1, state, action, "q1")
        q2 = _q_forward(Q2, state, action, "q2")
        q1_loss = (w * (q1 - q_target).pow(2)).mean()
        q2_loss = (w * (q2 - q_target).pow(2)).mean()
        with torch.no_grad():
            td = 0.5 * ((q1 - q_target).abs() + (q2 - q_target).abs())
            rows = q1.abs() + q2.abs() + q_target.abs()
            st.update(q1_mean=q1.mean().item(), q2_mean=q2.mean().item(),
                      q_target_mean=q_target.mean().item(), td_mean=td.mean().item(),
                      td_max=td.max().item(), reward_mean=reward.mean().item(),
                      batch=float(reward.shape[0]))
            scales = {"q": rows.mean().item(), "q_max": rows.max().item()}
        grads = {}
        self.opt["q1"].zero_grad(); q1_loss.backward()
        grads["q1"] = {k: v.grad.detach().clone() for k, v in Q1.items()}
        self.opt["q1"].step()
        self.opt["q2"].zero_grad(); q2_loss.backward()
        grads["q2"] = {k: v.grad.detach().clone() for k, v in Q2.items()}
        self.opt["q2"].step()

        self._actor_stats = {}
        policy_loss = self._actor(state, e2, grads)
        st.update(self._actor_stats.pop("stats"))
        scales["logp"] = self._actor_stats.pop("logp_scale")
        with torch.no_grad():
            tau = cfg.tau
            for src, dst in (("q1", "q1_target"), ("q2", "q2_target")):
                for k in q_keys(cfg.n_hidden):
                    t = self.nets[dst][k]
                    t.copy_(t * (1.0 - tau) + self.nets[src][k] * tau)
        self.last_grads = grads
        return {"q1_loss": q1_loss.item(), "q2_loss": q2_loss.item(),
                "policy_loss": policy_loss.item(), "stats": {k: st[k] for k in STAT_NAMES},
                "scales": scales, "td": td.reshape(-1).numpy().copy()}

    def _actor(self, state, e2, grads):
        """OracleSAC._actor, which also leaves q_pi_mean, entropy and alpha_loss (0 without
        automatic entropy tuning) in ``self._actor_stats``."""
        cfg = self.cfg
        P, Q1, Q2 = self.nets["policy"], self.nets["q1"], self.nets["q2"]
        new_a, logp = _policy_sample(P, state, e2, cfg.action_scale, cfg.action_bias, "pi_s")
        q_new = torch.min(_q_forward(Q1, state, new_a, "q1a"), _q_forward(Q2, state, new_a, "q2a"))
        policy_loss = (self.alpha * logp - q_new).mean()
        self.opt["policy"].zero_grad(); policy_loss.backward()
        grads["policy"] = {k: v.grad.detach().clone() for k, v in P.items()}
        self.opt["policy"].step()
        alpha_loss = 0.0
        if cfg.automatic_entropy_tuning:
            target_entropy = -cfg.action_dim
            al = -(self.log_alpha * (logp + target_entropy).detach()).mean()
            alpha_loss = al.item()
            self.opt["alpha"].zero_grad(); al.backward()
            grads["log_alpha"] = self.log_alpha.grad.detach().clone()
            self.opt["alpha"].step()
            self.alpha = self.log_alpha.exp()
        stats = getattr(self, "_actor_stats", None)
        if stats is not None:
            with torch.no_grad():
                stats["stats"] = dict(q_pi_mean=q_new.mean().item(), entropy=(-logp.mean()).item(),
                                      alpha_loss=alpha_loss)
                stats["logp_scale"] = logp.abs().mean().item() + cfg.action_dim
        return policy_loss


def stats_row(out) -> np.ndarray:
    """The model's statistics as a float64 row in id order."""
    return np.array([out["stats"][k] for k in STAT_NAMES], np.float64)


def stat_scales(out) -> np.ndarray:
    """Per statistic, the scale its error is measured on (nan where it is compared exactly)."""
    return np.array([out["scales"][STAT_SCALE[k]] if k in STAT_SCALE else np.nan
                     for k in STAT_NAMES], np.float64)
