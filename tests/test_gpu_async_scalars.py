"""Updates whose losses leave through the device ring (step_async, step_many_async) store
nothing into the host-mapped loss / error / done words, and where a gather rides in a fused-Adam
level the level's scalar chain (losses, alpha step, ring row, done word) runs on the first ride
workgroup instead of block 0.  Every result keeps its bits.

Shapes: S11-A3-H96-B40 (the 16-way dW form; fp32, bf16, and fp32 with set_grad_clip(inf): the
k_adam scalar tail) and S376-A17-H512-B256 (fp32: the 64x64 fused-Adam form of L6, more than
256 32x64 tiles).

The host words are read through the debug entry sacmi_debug_host_words (Context.
debug_host_words): out[0..2] the loss bits, out[3] the error bits, out[4] the done counter.

Two places where this file reads the issue's text by its sense:
* the mixed sequence as listed (sync step, 3-update launch, sync step, async step, launch /
  wait, 2-update launch) is nine updates, so the twin context runs nine synchronous steps;
* a synchronous step writes no ring row (its losses come back through the host words), so "the
  next synchronous step returns losses equal to the ring's newest row" cannot hold of the ring;
  the step's losses are compared, bit for bit, with the twin context's step at the same
  position instead, and the ring is checked not to have moved.
"""
import numpy as np
import pytest

from oracle.sac_step import NETS, SacConfig, init_params, synthetic_rows

pytestmark = pytest.mark.gpu

# name -> (config, batch, rows in the replay, compute dtype, clip)
VARIANTS = {
    "small-fp32": (SacConfig(11, 3, 96), 40, 160, "fp32", False),
    "small-bf16": (SacConfig(11, 3, 96), 40, 160, "bf16", False),
    "small-clip": (SacConfig(11, 3, 96), 40, 160, "fp32", True),
    "large-fp32": (SacConfig(376, 17, 512), 256, 512, "fp32", False),
}
_inputs = {}


def inputs_of(cfg, nrows):
    key = (cfg.state_dim, cfg.hidden_dim)
    if key not in _inputs:
        params = init_params(cfg, 911, bias_scale=0.05)
        rows = synthetic_rows(cfg, nrows, 912, state_scale=0.5)
        mt = (np.arange(624, dtype=np.uint64) * 2654435761 % (2**32)).astype(np.uint32)
        _inputs[key] = (params, rows, mt)
    return _inputs[key]


def new_ctx(variant):
    from sacmi import Config, Context
    cfg, B, nrows, dtype, clip = VARIANTS[variant]
    params, rows, mt = inputs_of(cfg, nrows)
    ctx = Context(Config(cfg.state_dim, cfg.action_dim, cfg.hidden_dim, max_batch=B, capacity=nrows,
                         seed=7, compute_dtype=dtype), 0)
    for n in NETS:
        ctx.set_net(n, params[n])
    ctx.push(*rows)
    ctx.set_mt(0, mt, 624)
    if clip:
        ctx.set_grad_clip(float("inf"), float("inf"))
    return ctx, B


def state_of(ctx):
    """Parameters, targets, Adam moments and the log_alpha state."""
    from sacmi import _lib as L
    out = {}
    for n in NETS:
        for k, v in ctx.get_net(n).items():
            out[f"{n}.{k}"] = v
        if n in ("policy", "q1", "q2"):
            for slot in ("m", "v"):
                for k, v in ctx.get_net(n, slot).items():
                    out[f"{n}.{k}.{slot}"] = v
    for name, sid in (("log_alpha", L.S_LOG_ALPHA), ("log_alpha.m", L.S_ADAM_M_LOG_ALPHA),
                      ("log_alpha.v", L.S_ADAM_V_LOG_ALPHA), ("alpha", L.S_ALPHA)):
        out[name] = np.array([ctx.get_scalar(sid)])
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# the mixed sequence: (call, updates)
MIXED = (("sync", 1), ("many", 3), ("sync", 1), ("async", 1), ("launch_wait", 1), ("many", 2))
N_MIXED = sum(n for _, n in MIXED)


@pytest.fixture(scope="module")
def twins():
    """Per variant, once: the nine updates as nine synchronous steps -> (losses [9, 3], state)."""
    cache = {}

    def get(variant):
        if variant not in cache:
            ctx, B = new_ctx(variant)
            try:
                losses = np.stack([ctx.step(B) for _ in range(N_MIXED)])
                cache[variant] = (losses, state_of(ctx))
            finally:
                ctx.close()
        return cache[variant]
    return get


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_mixed_sequence_identical_to_synchronous_steps(variant, twins):
    want_losses, want_state = twins(variant)
    ctx, B = new_ctx(variant)
    try:
        sync_rows, ring_rows, pos = {}, [], 0
        for kind, n in MIXED:
            if kind == "sync":
                sync_rows[pos] = ctx.step(B)
            elif kind == "launch_wait":
                ctx.step_launch(B)
                sync_rows[pos] = ctx.step_wait()
            else:
                if kind == "many":
                    ctx.step_many_async(B, n)
                else:
                    ctx.step_async(B)
                ring_rows += list(range(pos, pos + n))
            pos += n
        ring = ctx.fetch_losses(N_MIXED)
        got_state = state_of(ctx)
    finally:
        ctx.close()
    assert np.all(np.isfinite(want_losses))
    # the ring holds the async updates' rows alone, oldest first
    assert ring.shape == (len(ring_rows), 3)
    assert np.array_equal(bits(ring), bits(want_losses[ring_rows])), (ring, want_losses[ring_rows])
    for p, row in sync_rows.items():
        assert np.array_equal(bits(row), bits(want_losses[p])), (p, row, want_losses[p])
    assert sorted(got_state) == sorted(want_state)
    for k in want_state:
        assert np.array_equal(got_state[k], want_state[k]), k


@pytest.mark.parametrize("polling", [True, False], ids=["polling", "inflight"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_host_words_across_async_launches(variant, polling, twins):
    want_losses, _ = twins(variant)
    ctx, B = new_ctx(variant)
    try:
        l0 = ctx.step(B)
        w0 = ctx.debug_host_words()
        assert np.array_equal(w0[:3], bits(l0)) and w0[3] == 0
        ctx.step_many_async(B, 3)
        ctx.step_async(B)
        if polling:
            ctx.synchronize()   # nothing in flight: the next step polls the done word
        w1 = ctx.debug_host_words()      # (waits for the stream; the context still counts the
        assert w1.tobytes() == w0.tobytes(), (w0, w1)   # launches as in flight without the sync)
        l5 = ctx.step(B)
        w2 = ctx.debug_host_words()
        ring = ctx.fetch_losses(16)
    finally:
        ctx.close()
    assert int(w2[4]) == int(w0[4]) + 1
    assert np.array_equal(w2[:3], bits(l5)) and w2[3] == 0
    assert np.array_equal(bits(l5), bits(want_losses[5])), (l5, want_losses[5])
    # the ring: the four async updates' rows, not moved by the synchronous step
    assert np.array_equal(bits(ring), bits(want_losses[1:5])), (ring, want_losses[1:5])


# kernels per update of a launch: the parent's, by site prefix.  Sampling (k_mt_sample,
# k_gather) belongs to the launch, not the update, and is left out
PER_UPDATE = {"small-fp32": 13, "large-fp32": 13}


@pytest.mark.parametrize("variant", list(PER_UPDATE))
def test_launch_timeline_has_no_new_launch(variant):
    ctx, B = new_ctx(variant)
    try:
        ks, _ = ctx.profile_timeline(B, 3, launch=True)
    finally:
        ctx.close()
    ks = [k for k in ks if k["kernel"] not in ("k_mt_sample", "k_gather")]
    sites = [k["site"] for k in ks]
    assert sum(s.startswith("gemm_L6_critic_dW") for s in sites) == 3, sites
    assert sum(s.startswith("gemm_L13_pi_dW") for s in sites) == 3, sites
    assert len(ks) == 3 * PER_UPDATE[variant], sites


@pytest.mark.parametrize("variant", ["small-fp32", "small-bf16", "small-clip"])
def test_voided_update_inside_an_async_launch(variant):
    cfg, B = VARIANTS[variant][0], VARIANTS[variant][1]
    A, H = cfg.action_dim, cfg.hidden_dim
    ctx, _ = new_ctx(variant)
    try:
        ctx.step(B)
        w0 = ctx.debug_host_words()
        ctx.step_many_async(B, 2)
        good = ctx.fetch_losses(8)
        assert good.shape == (2, 3)
        w = ctx.get_tensor("param", "policy", 2, 0, (A, H))      # policy.mean.weight
        keep = w[1, 5]
        w[1, 5] = np.nan
        ctx.set_tensor("param", "policy", 2, 0, w)
        ctx.step_many_async(B, 3)
        with pytest.raises(ValueError, match=r"Normal.*at update #2 "):
            ctx.fetch_losses(8)
        assert ctx.debug_host_words().tobytes() == w0.tobytes()
        # the voided updates took no ring slot: one more update is row 2
        w[1, 5] = keep
        ctx.set_tensor("param", "policy", 2, 0, w)
        ctx.step_async(B)
        ring = ctx.fetch_losses(8)
        assert ctx.debug_host_words().tobytes() == w0.tobytes()
    finally:
        ctx.close()
    assert ring.shape == (3, 3) and np.all(np.isfinite(ring))
    assert np.array_equal(bits(ring[:2]), bits(good))
