#!/usr/bin/env python3
"""Bit pin of the row-prologue dh levels (L5 critic dh1, L9 actor dh1).

Runs 6 updates at each of the shapes below on the GPU and records every loss as a hex
float and a sha256 of every parameter tensor (all five networks) and of log_alpha after
the last update.  tests/test_gpu_dh_rows.py recomputes the same record and compares it
with tests/golden/dh_rows_bits.json bit for bit.

usage: python tools/gen_dh_rows_bits.py [OUT.json]     (default: tests/golden/dh_rows_bits.json)

The file is generated on the commit whose bits are to be kept.  A change that means to
move them regenerates it and says why.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "humanoid-walking-with-sac_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# (name, state dim, action dim, hidden, batch, replay rows, state scale, seed)
#  * S11-A3-H96-B40: 3 dot partials per row, a second row tile with 8 live rows, the
#    column-tile-0 store of the coefficient-free rows, critic and actor prologue
#  * S376-A17-H512-B64: 16 partials per row (every lane of a (row, slot) group holds two),
#    L9's dL/da partials at Humanoid's action width
#  * S11-A3-H544-B40: 17 partials per row, the tail of the column-order sum
#  * S11-A3-H512-B1056: the smallest batch at hidden 512 whose dh1 levels take the 64-row
#    two-wave-group k_gemm tiles (528 32x64 tiles over the two critics), i.e. the
#    rows_load / rows_finish form of the prologue
CASES = (
    ("S11-A3-H96-B40", 11, 3, 96, 40, 160, 0.5, 701),
    ("S376-A17-H512-B64", 376, 17, 512, 64, 200, 0.1, 702),
    ("S11-A3-H544-B40", 11, 3, 544, 40, 160, 0.5, 703),
    ("S11-A3-H512-B1056", 11, 3, 512, 1056, 1200, 0.5, 704),
)
UPDATES = 6


def case_inputs(case):
    """(cfg, params, rows, per-update (idx, eps1, eps2)) of one case: fixed seeds."""
    from oracle.sac_step import SacConfig, init_params, synthetic_rows
    _, S, A, H, B, n_rows, scale, seed = case
    cfg = SacConfig(S, A, H)
    params = init_params(cfg, seed, bias_scale=0.05)
    rows = synthetic_rows(cfg, n_rows, seed + 1000, state_scale=scale)
    rng = np.random.default_rng(seed + 2000)
    draws = []
    for _ in range(UPDATES):
        idx = rng.choice(n_rows, B, replace=False)
        e1 = rng.standard_normal((B, A)).astype(np.float32)
        e2 = rng.standard_normal((B, A)).astype(np.float32)
        draws.append((idx, e1, e2))
    return cfg, params, rows, draws


def run_bits(case):
    """The record of one case: {"losses": [[hex, hex, hex] per update], "sha256": {tensor: hex}}."""
    from oracle.sac_step import NETS, param_shapes
    from sacmi import Config, Context
    from sacmi import _lib as L
    cfg, params, rows, draws = case_inputs(case)
    B = case[4]
    ctx = Context(Config(cfg.state_dim, cfg.action_dim, cfg.hidden_dim, max_batch=B, capacity=len(rows[2])), 0)
    try:
        for n in NETS:
            ctx.set_net(n, params[n])
        ctx.push(*rows)
        losses = []
        for idx, e1, e2 in draws:
            lg = np.asarray(ctx.step(B, idx=idx, eps1=e1, eps2=e2), np.float32)
            losses.append([float(v).hex() for v in lg])
        shapes = param_shapes(cfg)
        sha = {}
        for n in NETS:
            for k, v in ctx.get_net(n, "param", shapes[n]).items():
                sha[f"{n}.{k}"] = hashlib.sha256(np.ascontiguousarray(v, np.float32).tobytes()).hexdigest()
        la = np.array([ctx.get_scalar(L.S_LOG_ALPHA)], np.float64)
        sha["log_alpha"] = hashlib.sha256(la.tobytes()).hexdigest()
    finally:
        ctx.close()
    return {"losses": losses, "sha256": sha}


def main(argv):
    out = argv[1] if len(argv) > 1 else os.path.join(ROOT, "tests", "golden", "dh_rows_bits.json")
    rec = {case[0]: run_bits(case) for case in CASES}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main(sys.argv)
