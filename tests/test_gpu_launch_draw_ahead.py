"""A multi-update launch leaves the next launch's first batch behind: the last update of an
n-update graph runs the next launch's random.sample + gather as its L12 / L13 rides, the
sampler saving the MT state it starts from, and a launch that finds a drawn batch of its own
batch size has no sampler / gather launch of its own.  Anything but a read in between restores
the save point first.

Shape S11-A3-H96-B40, uniform replay.  The sequence — a 3-update launch, a 3-update launch, a
single async update, a 2-update launch — runs with one kind of call in every gap (nothing; a
fetch of the losses and a synchronize; a push; a host random.sample; a launch of another batch
size) and must agree bit for bit with the same sequence in a context created with the
draw-ahead off (SACMI_NO_PREFETCH): losses, parameters, Adam moments, the MT state, the host
sample's indices.

The launch timeline of ONE real launch (profile_timeline(..., launch=True):
sacmi_profile_launch_timeline, the launch step_many_async would make now) shows the form: a
launch behind one that drew ahead has no k_mt_sample / k_gather of its own; the first launch
after any other call (the context's set-up, a push) has one each and draws nothing ahead, the
launch behind it has one each and draws ahead.
"""
import os

import numpy as np
import pytest

from oracle.sac_step import NETS, SacConfig, init_params, synthetic_rows

pytestmark = pytest.mark.gpu

CFG, B, NROWS, EXTRA = SacConfig(11, 3, 96), 40, 160, 8
GAPS = ("nothing", "fetch_sync", "push", "host_sample", "batch_change")


@pytest.fixture(scope="module")
def inputs():
    params = init_params(CFG, 811, bias_scale=0.05)
    rows = synthetic_rows(CFG, NROWS + EXTRA, 812, state_scale=0.5)
    key = (np.arange(624, dtype=np.uint64) * 2654435761 % (2**32)).astype(np.uint32)
    return params, rows, key


def new_ctx(inputs, ahead):
    from sacmi import Config, Context
    params, rows, key = inputs
    if not ahead:
        os.environ["SACMI_NO_PREFETCH"] = "1"
    try:
        ctx = Context(Config(CFG.state_dim, CFG.action_dim, CFG.hidden_dim, max_batch=B,
                             capacity=NROWS + EXTRA, seed=5), 0)
    finally:
        os.environ.pop("SACMI_NO_PREFETCH", None)
    for n in NETS:
        ctx.set_net(n, params[n])
    ctx.push(*[x[:NROWS] for x in rows])
    ctx.set_mt(0, key, 624)
    return ctx


def state_of(ctx):
    """Everything the sequence leaves: parameters, Adam moments, the log_alpha state, MT."""
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
                      ("log_alpha.v", L.S_ADAM_V_LOG_ALPHA)):
        out[name] = np.array([ctx.get_scalar(sid)])
    mt_key, mt_pos = ctx.get_mt(0)
    out["mt.key"], out["mt.pos"] = np.asarray(mt_key), np.array([mt_pos])
    return out


def assert_same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def run_sequence(ctx, rows, gap):
    """The four launches with `gap` in every gap.  Returns {name: array} of everything
    observed."""
    seen, pushed, done = {}, 0, 0
    steps = (("many", 3), ("many", 3), ("single", 1), ("many", 2))
    for i, (kind, n) in enumerate(steps):
        if kind == "single":
            ctx.step_async(B)
        else:
            ctx.step_many_async(B, n)
        done += n
        if i + 1 == len(steps):
            break
        if gap == "fetch_sync":
            seen[f"losses_after_{i}"] = ctx.fetch_losses(n)
            ctx.synchronize()
        elif gap == "push":
            ctx.push(*[x[NROWS + pushed:NROWS + pushed + 1] for x in rows])
            pushed += 1
        elif gap == "host_sample":
            seen[f"indices_after_{i}"] = ctx.sample_indices(B)
        elif gap == "batch_change":
            ctx.step_many_async(B // 2, 2)
            done += 2
    seen["losses"] = ctx.fetch_losses(done)
    assert seen["losses"].shape == (done, 3) and np.all(np.isfinite(seen["losses"]))
    seen.update(state_of(ctx))
    return seen


@pytest.mark.parametrize("gap", GAPS)
def test_launch_sequence_identical_to_no_prefetch(gap, inputs):
    """Bit for bit what the same sequence computes with nothing drawn ahead."""
    res = []
    for ahead in (True, False):
        ctx = new_ctx(inputs, ahead)
        try:
            res.append(run_sequence(ctx, inputs[1], gap))
        finally:
            ctx.close()
    assert_same(res[0], res[1], gap)


def own_sampling(kernels):
    """(k_mt_sample launches, k_gather launches) of a timeline."""
    kinds = [k["kernel"] for k in kernels]
    return kinds.count("k_mt_sample"), kinds.count("k_gather")


# the timeline test's calls, and per launch the (k_mt_sample, k_gather) launches of its own:
# the first launch after any other call samples for itself and draws nothing ahead (the rule
# that keeps a trainer with a push per env step from paying a restore per step), the next one
# samples for itself and draws ahead, and from there on no launch samples for itself
SCRIPT = (("many", 3, (1, 1)), ("many", 3, (1, 1)), ("many", 3, (0, 0)), ("single", 1, None),
          ("many", 2, (0, 0)), ("push", 0, None), ("many", 3, (1, 1)), ("many", 3, (1, 1)),
          ("many", 2, (0, 0)))


def run_script(ctx, rows, launch):
    forms, done = [], 0
    for kind, n, _ in SCRIPT:
        if kind == "many":
            forms.append(launch(ctx, n))
        elif kind == "single":
            ctx.step_async(B)
        else:
            ctx.push(*[x[NROWS:NROWS + 1] for x in rows])
        done += n
    seen = {"losses": ctx.fetch_losses(done)}
    assert seen["losses"].shape == (done, 3) and np.all(np.isfinite(seen["losses"]))
    seen.update(state_of(ctx))
    return forms, seen


def test_back_to_back_launches_do_not_sample_for_themselves(inputs):
    """The timeline of the real launches (SCRIPT): once a launch has drawn ahead, the launches
    behind it, back to back, have no k_mt_sample / k_gather of their own; after a push they do
    again.  The timed launches are the sequence's own: its results are bit for bit those of
    plain step_many_async launches with the draw-ahead off."""
    def timed(ctx, n):
        ks, _ = ctx.profile_timeline(B, n, launch=True)
        sites = [k["site"] for k in ks]
        assert sum(s.startswith("gemm_L13_pi_dW") for s in sites) == n, sites
        return own_sampling(ks)

    def plain(ctx, n):
        ctx.step_many_async(B, n)

    res = []
    for ahead, launch in ((True, timed), (False, plain)):
        ctx = new_ctx(inputs, ahead)
        try:
            res.append(run_script(ctx, inputs[1], launch))
        finally:
            ctx.close()
    assert res[0][0] == [f for kind, _, f in SCRIPT if kind == "many"], res[0][0]
    assert_same(res[0][1], res[1][1], "timed launches")
