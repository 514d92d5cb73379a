"""The gradient-clipping yardstick (tests/grad_clip_model.py) pinned on the CPU: the proxy
against torch.nn.utils.clip_grad_norm_, measure-only against the plain oracle, and the fp32
coefficient helper at its edges.  These pass without the feature: they pin the model the GPU
tests (tests/test_gpu_grad_clip.py) compare with."""
import math

import numpy as np
import pytest
import torch

from oracle.sac_step import OracleSAC, SacConfig, init_params, synthetic_rows

from grad_clip_model import GROUPS, ClipProxy, ClipSAC, clip_coef, grad_norm64


def _inputs(B=24, seed=71):
    cfg = SacConfig(11, 3, 32)
    params = init_params(cfg, seed, bias_scale=0.05)
    rows = synthetic_rows(cfg, 64, seed + 1, state_scale=0.5)
    rng = np.random.default_rng(seed + 2)
    idx = [rng.permutation(64)[:B] for _ in range(2)]
    eps = [rng.standard_normal((B, 3)).astype(np.float32) for _ in range(4)]
    return cfg, params, rows, idx, eps


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("scale", [0.5, 2.0, math.inf])
def test_proxy_equals_torch_clip_grad_norm(dtype, scale):
    """The proxy's in-place scaling against torch.nn.utils.clip_grad_norm_ on the same
    gradients: clipped (0.5 x norm), not clipped (2 x norm) and inf."""
    g = torch.Generator().manual_seed(5)
    shapes = [(7, 5), (7,), (1, 7), (1,)]
    ps = [torch.randn(s, generator=g, dtype=dtype).requires_grad_() for s in shapes]
    grads = [torch.randn(s, generator=g, dtype=dtype) * 3 for s in shapes]
    qs = [p.detach().clone().requires_grad_() for p in ps]
    for p, q, gr in zip(ps, qs, grads):
        p.grad, q.grad = gr.clone(), gr.clone()
    norm = grad_norm64(grads)
    max_norm = scale * norm
    total = torch.nn.utils.clip_grad_norm_(qs, max_norm)
    proxy = ClipProxy(torch.optim.SGD(ps, lr=0.0), max_norm, "fp64")
    proxy.step()
    assert abs(float(total) - proxy.norms[0]) <= 4 * np.spacing(np.float32(norm) if dtype == torch.float32 else norm)
    want = min(1.0, max_norm / (norm + 1e-6))
    assert abs(proxy.coefs[0] - want) <= 1e-15
    assert (proxy.coefs[0] < 1.0) == (scale < 1.0)
    tol = 1e-6 if dtype == torch.float32 else 1e-14
    for p, q in zip(ps, qs):
        assert torch.allclose(p.grad, q.grad, rtol=tol, atol=0.0)


def test_inf_is_bit_identical_to_plain_oracle():
    """max_norm = inf: coef exactly 1, and x * 1.0 is exact — two updates leave parameters,
    moments, targets, log_alpha and losses bit-identical to OracleSAC (fp32 and fp64)."""
    cfg, params, rows, idx, eps = _inputs()
    for dtype in (torch.float32, torch.float64):
        for variant in ("fp64", "fp32"):
            a = OracleSAC(cfg, params, dtype)
            b = ClipSAC(cfg, params, dtype).install({n: math.inf for n in GROUPS}, variant)
            for u in range(2):
                batch = [x[idx[u]] for x in rows]
                la = a.step(*batch, eps[2 * u], eps[2 * u + 1])
                lb = b.step(*batch, eps[2 * u], eps[2 * u + 1])
                assert la == lb
            sa, sb = a.state(), b.state()
            assert sa.keys() == sb.keys()
            for k in sa:
                assert np.array_equal(sa[k], sb[k]), k
            assert np.all(b.coefs() == 1.0) and b.norms().shape == (2, 3) and np.all(b.norms() > 0)


def test_clipped_update_differs_and_records():
    """A finite threshold below the norm changes the moments by the coefficient, and the
    recorded norm is that of the pre-clip gradient the oracle exports."""
    cfg, params, rows, idx, eps = _inputs()
    batch = [x[idx[0]] for x in rows]
    m = ClipSAC(cfg, params, torch.float64).install({n: math.inf for n in GROUPS})
    m.step(*batch, eps[0], eps[1])
    norms = m.norms()[0]
    g = m.grads_flat()
    for i, n in enumerate(GROUPS):
        assert abs(grad_norm64(v for k, v in g.items() if k.startswith(n + ".")) - norms[i]) <= 1e-12 * norms[i]
    c = ClipSAC(cfg, params, torch.float64).install({n: 0.5 * norms[i] for i, n in enumerate(GROUPS)})
    c.step(*batch, eps[0], eps[1])
    assert np.all(np.abs(c.coefs()[0] - 0.5) < 1e-5)
    # q1's norm is the critic step's own; the policy's gradient is taken through the clipped
    # critics, so only q1 / q2 norms repeat exactly
    assert np.array_equal(c.norms()[0][:2], norms[:2])
    sm, sc = m.state(), c.state()
    k = "adam.q1.fc1.weight.m"
    assert np.allclose(sc[k], sm[k] * c.coefs()[0][0], rtol=1e-12, atol=0.0)


def test_clip_coef_edges():
    """The fp32 helper at its edges: norm 0 (max / 1e-6: far above 1, or exactly 1 for
    inf), a norm just below and just above max_norm - 1e-6, and inf."""
    f = np.float32
    assert clip_coef(0.0, 1.0) == f(1.0)
    assert clip_coef(0.0, 1e-7) == f(1e-7) / f(1e-6) and clip_coef(0.0, 1e-7) < 1
    assert clip_coef(0.0, math.inf) == f(1.0)
    assert clip_coef(3.0, math.inf) == f(1.0)
    assert np.isnan(clip_coef(math.inf, math.inf))          # inf / inf: the formula as written
    assert clip_coef(math.inf, 5.0) == f(0.0)
    assert np.isnan(clip_coef(math.nan, 5.0))
    mx = f(2.0)
    edge = f(mx - f(1e-6))                                   # norm + 1e-6 rounds to max_norm
    below, above = np.nextafter(edge, f(0)), np.nextafter(edge, f(4))
    for norm in (below, edge, above):
        den = f(norm) + f(1e-6)
        want = f(1.0) if mx / den > 1 else f(mx / den)
        assert clip_coef(norm, mx) == want
    assert clip_coef(below, mx) == f(1.0)
    assert clip_coef(f(2.0), mx) < f(1.0)
    assert clip_coef(f(4.0), mx) == f(2.0) / (f(4.0) + f(1e-6))
    assert clip_coef(1.0, 0.5).dtype == np.float32
