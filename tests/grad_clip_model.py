"""Model of global-norm gradient clipping (include/sacmi.h sacmi_set_grad_clip):
``torch.nn.utils.clip_grad_norm_`` between ``backward()`` and ``optimizer.step()`` of the
reference's three network optimizers (q1, q2, policy: sac_imp.py:101-125; never log_alpha).

    sumsq = sum over the group's gradient elements of g^2          fp64
    norm  = sqrt(sumsq)
    coef  = min(1, max_norm / (norm + 1e-6))
    the optimizer steps from g * coef

TEST INFRASTRUCTURE ONLY: ``ClipSAC`` is ``oracle.sac_step.OracleSAC`` whose three network
optimizers are wrapped, from outside, by ``ClipProxy``: its ``step()`` first applies the formula
to its parameters' ``.grad`` in place (as torch does), then steps; it records ``norm`` and
``coef`` per update.  Two variants of the coefficient: "fp64" (norm and coef in fp64: the
truth the parity test compares with) and "fp32" (norm rounded to fp32, coef formed in fp32
with ``clip_coef``: the GPU's expression).
"""
from __future__ import annotations

import numpy as np
import torch

from oracle.sac_step import OracleSAC

GROUPS = ("q1", "q2", "policy")


def clip_coef(norm, max_norm) -> np.float32:
    """min(1, max_norm / (norm + 1e-6)) with every operation rounded to fp32."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        c = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    return np.float32(1.0) if c > np.float32(1.0) else np.float32(c)


def grad_norm64(grads) -> float:
    """sqrt of the fp64 sum of squares over an iterable of arrays / tensors."""
    s = 0.0
    for g in grads:
        g = g.detach().numpy() if torch.is_tensor(g) else np.asarray(g)
        s += float(np.sum(np.square(g.astype(np.float64))))
    return float(np.sqrt(s))


class ClipProxy:
    """An optimizer whose ``step()`` clips its parameters' gradients to ``max_norm`` first."""

    def __init__(self, opt, max_norm: float, variant: str = "fp64"):
        assert variant in ("fp64", "fp32")
        self.opt, self.max_norm, self.variant = opt, float(max_norm), variant
        self.norms, self.coefs = [], []

    @property
    def state(self):
        return self.opt.state

    @property
    def param_groups(self):
        return self.opt.param_groups

    def zero_grad(self, *a, **kw):
        return self.opt.zero_grad(*a, **kw)

    def _params(self):
        return [p for g in self.opt.param_groups for p in g["params"] if p.grad is not None]

    def step(self):
        ps = self._params()
        norm = grad_norm64(p.grad for p in ps)
        if self.variant == "fp32":
            norm = float(np.float32(norm))
            coef = float(clip_coef(norm, self.max_norm))
        else:
            coef = min(1.0, self.max_norm / (norm + 1e-6))
        with torch.no_grad():
            for p in ps:
                p.grad.mul_(coef)
        self.norms.append(norm)
        self.coefs.append(coef)
        return self.opt.step()


class ClipSAC(OracleSAC):
    """OracleSAC with clipped network optimizers.  ``max_norm``: {"q1", "q2", "policy"} -> float
    (``inf``: measured only).  ``norms()`` / ``coefs()``: [updates][3] in GROUPS order."""

    def install(self, max_norm: dict, variant: str = "fp64"):
        for n in GROUPS:
            self.opt[n] = ClipProxy(self.opt[n], max_norm[n], variant)
        return self

    def norms(self):
        return np.array([self.opt[n].norms for n in GROUPS], np.float64).T

    def coefs(self):
        return np.array([self.opt[n].coefs for n in GROUPS], np.float64).T
