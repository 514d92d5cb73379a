"""Analytic model of the policy sample head, forward and backward, in float32 or float64.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

Restates, element by element, the algebra the HIP head kernels state in their comments
(kernels.hip heads_elem / k_act_heads forward; k_gemm_sample_bwd / tail_unit backward) for
GaussianPolicy.sample (networks_model1.py:65-99):

forward, from the head sums ``mean`` and ``ls_raw`` (bias added) and the noise ``eps``:
    ls   = clamp(ls_raw, -20, 2)          sd = exp(ls)
    x    = mean + eps * sd                y  = tanh(x)
    omy2 = 1 - y^2 = 4t / (1 + t)^2,  t = exp(-2|x|)        (no cancellation at large |x|)
    logp_elem = -(x - mean)^2 / (2 sd^2) - log(sd) - log(sqrt(2 pi)) - log(scale * omy2 + 1e-6)
    action    = y * scale + bias

backward, given ga = dL/da and glogp = dL/dlogp (alpha / B for the policy loss):
    u     = scale * omy2 + 1e-6
    G     = scale * ga + glogp * 2 * scale * y / u
    dmean = G * omy2
    dls   = [-20 <= ls_raw <= 2] * (dmean * eps * sd - glogp)
(the Normal.log_prob quadratic term's gradients w.r.t. mean and std cancel exactly, since
x - mean = eps * sd; the clamp passes its gradient at both bounds, as torch.clamp does, and
the mask is taken from the RAW head sum: the clamped value always lies inside.)

In float64 this is the truth of the same operation as torch autograd of
oracle.sac_step._policy_sample (tests/test_heads_model.py ties the two).  In float32 it is the
well-conditioned formula's own rounding noise: ``e_ref`` of the GPU head tests.  The
reference's fp32 step cannot serve there: with log_std clamped at -20 its quadratic term's
two +-eps/sd ~ 5e8 gradient terms swallow the rest, and 1 - y^2 cancels at |x| >= 4.
"""
from __future__ import annotations

import numpy as np

LS_MIN, LS_MAX = -20.0, 2.0
LOG_SQRT_2PI = 0.91893853320467274178


def clamp_mask(ls_raw) -> np.ndarray:
    """1 where the clamp passes the gradient: inclusive at both bounds, on the raw value."""
    ls_raw = np.asarray(ls_raw)
    return ((ls_raw >= LS_MIN) & (ls_raw <= LS_MAX)).astype(ls_raw.dtype)


def forward(mean, ls_raw, eps, scale, bias, dtype=np.float64, deterministic=False) -> dict:
    """Every intermediate of the sample, all arithmetic in ``dtype`` (the inputs are rounded
    to it first).  deterministic: x = mean (select_action(evaluate=True))."""
    f = np.dtype(dtype).type
    mean, ls_raw, eps = (np.asarray(v, dtype=dtype) for v in (mean, ls_raw, eps))
    scale, bias = f(scale), f(bias)
    ls = np.minimum(np.maximum(ls_raw, f(LS_MIN)), f(LS_MAX))
    sd = np.exp(ls)
    x = mean if deterministic else mean + eps * sd
    y = np.tanh(x)
    t = np.exp(f(-2) * np.abs(x))
    omy2 = f(4) * t / ((f(1) + t) * (f(1) + t))
    dx = x - mean
    logp_elem = -(dx * dx) / (f(2) * (sd * sd)) - np.log(sd) - f(LOG_SQRT_2PI)
    logp_elem = logp_elem - np.log(scale * omy2 + f(1e-6))
    return dict(mean=mean, ls_raw=ls_raw, eps=eps, ls=ls, sd=sd, x=x, y=y, omy2=omy2,
                logp_elem=logp_elem, logp=logp_elem.sum(axis=-1), action=y * scale + bias)


def backward(fwd: dict, ga, glogp, scale, mask=None) -> tuple:
    """(dmean, dls) of a forward() result, in its dtype.  ``mask``: the clamp's gradient mask,
    clamp_mask(ls_raw) unless given (the tests pass wrong ones to show that they are caught)."""
    dtype = fwd["x"].dtype
    f = dtype.type
    ga = np.asarray(ga, dtype=dtype)
    glogp, scale = f(glogp), f(scale)
    u = scale * fwd["omy2"] + f(1e-6)
    G = scale * ga + glogp * (f(2) * scale * fwd["y"] / u)
    dmean = G * fwd["omy2"]
    if mask is None:
        mask = clamp_mask(fwd["ls_raw"])
    dls = np.asarray(mask, dtype=dtype) * (dmean * fwd["eps"] * fwd["sd"] - glogp)
    return dmean, dls


def column_scales(dmean, dls, h) -> dict:
    """The scale a head column's gradients are measured on: sum over the rows of |dhead_ij| for
    the bias entry, of |dhead_ij| ||h_i|| for the weight row (the bound of ||sum_i dhead_ij h_i||):
    a cancelling sum over the batch neither hides an error nor inflates one."""
    hn = np.linalg.norm(np.asarray(h, np.float64), axis=1)
    out = {}
    for name, d in (("mean", dmean), ("log_std", dls)):
        d = np.abs(np.asarray(d, np.float64))
        out[f"{name}.bias"] = d.sum(0)
        out[f"{name}.weight"] = (d * hn[:, None]).sum(0)
    return out


def head_grads(dmean, dls, h) -> dict:
    """The four head gradients of a dhead, in float64: weight = dhead^T h, bias = column sums."""
    h = np.asarray(h, np.float64)
    out = {}
    for name, d in (("mean", dmean), ("log_std", dls)):
        d = np.asarray(d, np.float64)
        out[f"{name}.weight"] = d.T @ h
        out[f"{name}.bias"] = d.sum(0)
    return out


def column_errors(got: dict, want: dict, scales: dict) -> dict:
    """Per column j and head tensor: |got_j - want_j| (2-norm over a weight row) over the
    column's scale; 0 where the scale is 0 and the two agree exactly (inf where they do not)."""
    out = {}
    for k, sc in scales.items():
        d = np.asarray(got[k], np.float64) - np.asarray(want[k], np.float64)
        e = np.abs(d) if d.ndim == 1 else np.linalg.norm(d, axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[k] = np.where(sc > 0, e / np.where(sc > 0, sc, 1.0), np.where(e == 0, 0.0, np.inf))
    return out


def e_ref_columns(mean, ls_raw, eps, ga, glogp, scale, bias, h) -> dict:
    """e_ref: the model's own float32-vs-float64 error per column and head tensor, on the
    columns' scales — the fp32 noise floor of the well-conditioned formula on these inputs."""
    f64 = forward(mean, ls_raw, eps, scale, bias, np.float64)
    f32 = forward(mean, ls_raw, eps, scale, bias, np.float32)
    d64 = backward(f64, ga, glogp, scale)
    d32 = backward(f32, ga, glogp, scale)
    return column_errors(head_grads(*d32, h), head_grads(*d64, h), column_scales(*d64, h))
