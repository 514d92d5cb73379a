#!/usr/bin/env python3
"""Pin of the update's launch plan: what the host planner in csrc/sacmi.hip enqueues.

Runs the cases below on the GPU, one fresh context and one Context.profile_timeline call
each (the `launch` cases: two consecutive calls), and records for every launch its site name,
kernel, grid, and the site's algorithmic FLOPs and bytes: the five fields of the timeline that
do not depend on the clock.  They are host values (the grid is the one the launcher computed),
in the order the planner marked the sites, so a case is the same list on every run, the
side-stream (prioritized replay) cases included.  tests/test_gpu_launch_plan.py recomputes
the same record and compares it with tests/golden/launch_plan.json for exact equality.

usage: python tools/gen_launch_plan.py [OUT.json]    (default: tests/golden/launch_plan.json)

The file is generated on the commit whose plan is to be kept (here: the commit before the
planner was split into opt_step / range_segments / the twin-critic builders / the three
phase functions).  A change that means to move a launch regenerates it and says why.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "humanoid-walking-with-sac_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FIELDS = ("site", "kernel", "grid", "flops", "bytes")
BASE = dict(S=24, A=4, H=64, B=64, rows=2000, nh=2, dtype="fp32", replay="uniform", n=1,
            launch=False, dp=None, setup=())


def _case(**kw):
    unknown = set(kw) - set(BASE)
    assert not unknown, unknown
    return dict(BASE, **kw)


# name -> settings (BASE where not given).  setup: Context methods called before the rows are
# pushed; dp: "allreduce" | "sharded" over a loopback communicator of world 2
CASES = {}
for _nh in (2, 3):
    for _dt in ("fp32", "bf16"):
        for _n in (1, 3):      # n = 3: the next update's sampler and gather ride in L12 / L13
            CASES[f"fused-nh{_nh}-{_dt}-n{_n}"] = _case(nh=_nh, dtype=_dt, n=_n)
CASES["launch-n2-twice"] = _case(n=2, launch=True)      # draw-ahead made, then taken and made
# 32 x 8 = 256 row x column tiles, more than 192: Polyak stays in L6 (L12's grid carries no
# Polyak workgroups); the dL/da fold still applies at this hidden size
CASES["B1024-H256-no-polyak-ride"] = _case(B=1024, H=256)
CASES["B256-H64-fold"] = _case(B=256)
# bf16 activations, the sampler riding in L6 and the gather in L12, the standalone L10
CASES["B4096-H512-bf16-act16-placement-b"] = _case(B=4096, H=512, rows=6000, dtype="bf16", n=2)
for _n in (1, 3):              # n = 3: the next draw on the side stream
    CASES[f"per-n{_n}"] = _case(replay="per", n=_n)
    CASES[f"per-feedback-n{_n}"] = _case(replay="per", n=_n, setup=(("per_set_feedback", True),))
CASES["stats"] = _case(setup=(("set_stats", True),))
CASES["clip-n2"] = _case(n=2, setup=(("set_grad_clip", 0.05, 0.05),))
CASES["obs-norm"] = _case(setup=(("set_obs_norm", 1),))
CASES["nstep3"] = _case(setup=(("set_nstep", 3),))
CASES["reward-norm-running"] = _case(setup=(("set_reward_norm", 1),))
CASES["nstep3-obs-norm"] = _case(setup=(("set_nstep", 3), ("set_obs_norm", 1)))
for _nh in (2, 3):
    for _form in ("allreduce", "sharded"):
        CASES[f"dp-{_form}-nh{_nh}-n2"] = _case(nh=_nh, n=2, dp=_form)
CASES["dp-sharded-B1024-H256-polyak-pass"] = _case(B=1024, H=256, n=2, dp="sharded")


def make_ctx(case):
    from oracle.sac_step import NETS, SacConfig, init_params, synthetic_rows
    from sacmi import Config, Context
    k = CASES[case]
    cfg = SacConfig(k["S"], k["A"], k["H"], n_hidden=k["nh"])
    params = init_params(cfg, 5, bias_scale=0.05)
    ctx = Context(Config(k["S"], k["A"], k["H"], max_batch=k["B"], capacity=k["rows"], seed=7,
                         n_hidden=k["nh"], compute_dtype=k["dtype"], replay=k["replay"]), 0)
    for net in NETS:
        ctx.set_net(net, params[net])
    for name, *args in k["setup"]:
        getattr(ctx, name)(*args)
    ctx.push(*synthetic_rows(cfg, k["rows"], 6, state_scale=0.5))
    if k["dp"]:
        ctx.dp_loopback_init(2)
        ctx.dp_set_sharded(k["dp"] == "sharded")
    return ctx


def run_plan(case):
    """[[site, kernel, grid, flops, bytes] per launch] of one case."""
    k = CASES[case]
    ctx = make_ctx(case)
    try:
        out = []
        for _ in range(2 if k["launch"] else 1):
            ks, _us = ctx.profile_timeline(k["B"], k["n"], data_parallel=bool(k["dp"]),
                                           launch=k["launch"])
            out += [[r[f] for f in FIELDS] for r in ks]
    finally:
        ctx.close()
    return out


def dump(rec, path):
    """Compact: one launch per line."""
    with open(path, "w") as f:
        f.write("{\n")
        for i, (case, rows) in enumerate(sorted(rec.items())):
            body = ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rows)
            f.write(f" {json.dumps(case)}: [\n{body}\n ]{',' if i + 1 < len(rec) else ''}\n")
        f.write("}\n")


def main(argv):
    out = argv[1] if len(argv) > 1 else os.path.join(ROOT, "tests", "golden", "launch_plan.json")
    dump({case: run_plan(case) for case in CASES}, out)
    print("wrote", out)


if __name__ == "__main__":
    main(sys.argv)
