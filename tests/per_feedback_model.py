"""Model of prioritized replay with feedback: the host loop a user would write against the
reference's PrioritizedReplayBuffer (replay_buffer.py:48-87) around the SAC update
(sac_imp.py:74-144), in the oracle's arithmetic.

    s, a, r, s2, d, idx, w = buffer.sample(B)
    q_i_loss = mean(w * (q_i(s, a) - q^) ** 2)          i = 1, 2; q^ as sac_imp.py:87-98
    td       = 0.5 * (|q1 - q^| + |q2 - q^|)            per row
    buffer.update_priorities(idx, td)                   stored: float32(float64(td) + 1e-6)

The actor and alpha blocks are not weighted; the q losses returned are the weighted ones.

TEST INFRASTRUCTURE ONLY: ``FeedbackSAC`` is ``oracle.sac_step.OracleSAC`` with the weighted
critic losses; ``closed_loop_update`` composes it with ``oracle.per`` into the loop above.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import per as P
from oracle.sac_step import OracleSAC, _policy_sample, _q_forward, q_keys


class FeedbackSAC(OracleSAC):
    """OracleSAC whose critic losses carry per-row weights (``weights``: [B], default all
    ones); ``step`` also returns the rows' TD errors under "td" (numpy, the model's dtype)
    and keeps the unweighted q losses under "q1_loss_unweighted" / "q2_loss_unweighted"."""
    weights = None

    def step_weighted(self, s, a, r, s2, d, eps1, eps2, weights, **kw) -> dict:
        self.weights = weights
        try:
            return self.step(s, a, r, s2, d, eps1, eps2, **kw)
        finally:
            self.weights = None

    def _step(self, s, a, r, s2, d, eps1, eps2) -> dict:
        cfg, dt = self.cfg, self.dtype
        T = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float32)).to(dt)
        state, action, next_state = T(s), T(a), T(s2)
        reward = T(r).reshape(-1, 1)
        done = T(d).reshape(-1, 1)
        e1, e2 = T(eps1), T(eps2)
        w = torch.ones_like(reward) if self.weights is None else T(self.weights).reshape(-1, 1)
        P_, Q1, Q2 = self.nets["policy"], self.nets["q1"], self.nets["q2"]
        sc, bi = cfg.action_scale, cfg.action_bias
        with torch.no_grad():
            na, nlp = _policy_sample(P_, next_state, e1, sc, bi, "pi_s2")
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
            unweighted = ((q1 - q_target).pow(2).mean().item(), (q2 - q_target).pow(2).mean().item())
            scale = (q1.abs() + q2.abs() + q_target.abs()).reshape(-1).numpy().copy()
        grads = {}
        self.opt["q1"].zero_grad(); q1_loss.backward()
        grads["q1"] = {k: v.grad.detach().clone() for k, v in Q1.items()}
        self.opt["q1"].step()
        self.opt["q2"].zero_grad(); q2_loss.backward()
        grads["q2"] = {k: v.grad.detach().clone() for k, v in Q2.items()}
        self.opt["q2"].step()

        policy_loss = self._actor(state, e2, grads)
        with torch.no_grad():
            tau = cfg.tau
            for src, dst in (("q1", "q1_target"), ("q2", "q2_target")):
                for k in q_keys(cfg.n_hidden):
                    t = self.nets[dst][k]
                    t.copy_(t * (1.0 - tau) + self.nets[src][k] * tau)
        self.last_grads = grads
        return {"q1_loss": q1_loss.item(), "q2_loss": q2_loss.item(),
                "policy_loss": policy_loss.item(), "td": td.reshape(-1).numpy().copy(),
                "td_scale": scale,
                "q1_loss_unweighted": unweighted[0], "q2_loss_unweighted": unweighted[1]}


def stored_priorities(td) -> np.ndarray:
    """What update_priorities stores for fp32 TD errors: float32(float64(td) + 1e-6)."""
    return (np.asarray(td, np.float32).astype(np.float64) + 1e-6).astype(np.float32)


def sample(prios, n, mt, frame, batch, alpha=0.6, beta_start=0.4, beta_frames=100000):
    """buffer.sample's indices and weights from the priority array, the fill, the numpy-MT
    stream (advanced in place) and the frame counter (the caller adds 1)."""
    probs = P.probs_from(np.asarray(prios, np.float32), n, alpha)
    return P.sample_from_probs(probs, batch, mt, P.beta_at(frame, beta_start, beta_frames))


def closed_loop_update(model: FeedbackSAC, prios, rows, mt, frame, batch, eps1, eps2,
                       alpha=0.6, beta_start=0.4, beta_frames=100000):
    """One update of the host loop on `rows` (s, a, r, s2, d stacked, slot order):
    returns (losses dict, idx, w, the priority array after update_priorities)."""
    n = len(rows[2])
    idx, w = sample(prios, n, mt, frame, batch, alpha, beta_start, beta_frames)
    out = model.step_weighted(*[x[idx] for x in rows], eps1, eps2, w)
    after = P.update_priorities(np.asarray(prios, np.float32), idx,
                                np.asarray(out["td"], np.float32))
    return out, idx, w, after
