#!/usr/bin/env python3
"""Bit pin of the weight-gradient levels (L6 critic dW, L13 policy dW) and of the dh
levels' u side store.

Runs the cases below on the GPU and records every loss as a hex float and a sha256 of every
parameter tensor, every Adam moment, log_alpha and its Adam state after the last update; the
side-store cases also record the two critics' fc2 weight gradient (the only reader of the
rows L5 stores through ax_out) after every update.  tests/test_gpu_dw_level_form.py
recomputes the same record and compares it with tests/golden/dw_level_bits.json bit for bit.

usage: python tools/gen_dw_level_bits.py [OUT.json]    (default: tests/golden/dw_level_bits.json)

The file is generated on the commit whose bits are to be kept (here: the commit before the
weight-gradient levels compiled the row-contiguous cores alone and the spread dh level chose
its storing core per workgroup).  A change that means to move them regenerates it and says why.
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

# shape name -> (state dim, action dim, hidden, batch, replay rows, state scale, seed)
#  * S11-A3-H96-B40: both dW levels on the 16-way K split of the 32x64 tiles (at most 256
#    tiles), L5 / L9 on the spread 32x32 tiles with the tile-0 u store
#  * S376-A17-H512-B256: the critics' dW level has 496 32x64 tiles (more than 256), so it takes
#    the 64x64 two-wave-group form: the smallest natural shape that does
#  * S11-A3-H512-B64: 16 column tiles per dh row block, one of them storing u
SHAPES = {
    "S11-A3-H96-B40": (11, 3, 96, 40, 160, 0.5, 801),
    "S376-A17-H512-B256": (376, 17, 512, 256, 400, 0.1, 802),
    "S11-A3-H512-B64": (11, 3, 512, 64, 200, 0.5, 803),
}
# (case, shape, dtype, mode, updates)
#   staged  synchronous updates on staged indices and noise (no ride-along workgroups)
#   launch  one multi-update launch, device-sampled: the sampler and the gather ride in
#           L12 / L13 (the fused-Adam kernel with ride-along workgroups)
#   clip    staged, with gradient clipping on: the plain dW form plus k_adam
#   ustore  staged, gradients kept: the fc2 critic weight gradients after every update
CASES = tuple(
    (f"{shape}-{dtype}-{mode}", shape, dtype, mode, n)
    for shape, mode, n in (("S11-A3-H96-B40", "staged", 6), ("S11-A3-H96-B40", "launch", 6),
                           ("S376-A17-H512-B256", "staged", 6), ("S376-A17-H512-B256", "launch", 6),
                           ("S11-A3-H96-B40", "clip", 6),
                           ("S11-A3-H96-B40", "ustore", 4), ("S11-A3-H512-B64", "ustore", 4))
    for dtype in ("fp32", "bf16"))
CLIP = (0.05, 0.05)      # below the first updates' norms at this shape: the coefficients engage


def sha(a, dtype=np.float32):
    return hashlib.sha256(np.ascontiguousarray(a, dtype).tobytes()).hexdigest()


def make_ctx(case):
    """(ctx, cfg, per-update (idx, eps1, eps2)) of one case, parameters and rows loaded."""
    from oracle.sac_step import NETS, SacConfig, init_params, synthetic_rows
    from sacmi import Config, Context
    _, shape, dtype, mode, n = case
    S, A, H, B, n_rows, scale, seed = SHAPES[shape]
    cfg = SacConfig(S, A, H)
    params = init_params(cfg, seed, bias_scale=0.05)
    rows = synthetic_rows(cfg, n_rows, seed + 1000, state_scale=scale)
    rng = np.random.default_rng(seed + 2000)
    draws = [(rng.choice(n_rows, B, replace=False), rng.standard_normal((B, A)).astype(np.float32),
              rng.standard_normal((B, A)).astype(np.float32)) for _ in range(n)]
    ctx = Context(Config(S, A, H, max_batch=B, capacity=n_rows, seed=seed, compute_dtype=dtype), 0)
    for net in NETS:
        ctx.set_net(net, params[net])
    ctx.push(*rows)
    return ctx, cfg, draws


def run_bits(case):
    """The record of one case: {"losses": [[hex, hex, hex] per update], "sha256": {name: hex}}
    (clip cases: and "grad_norms", [[hex] * 6 per update])."""
    from oracle.sac_step import NETS
    from sacmi import _lib as L
    _, shape, dtype, mode, n = case
    B = SHAPES[shape][3]
    ctx, cfg, draws = make_ctx(case)
    try:
        out = {}
        if mode == "clip":
            ctx.set_grad_clip(*CLIP)
        if mode == "ustore":
            ctx.set_scalar(L.S_KEEP_GRADS, 1)
        if mode == "launch":
            key = (np.arange(624, dtype=np.uint64) * 69069 % (2**32)).astype(np.uint32)
            ctx.set_mt(0, key, 624)
            ctx.step_many_async(B, n)
            losses = np.asarray(ctx.fetch_losses(n), np.float32).reshape(n, 3)
        else:
            losses = []
            for u, (idx, e1, e2) in enumerate(draws):
                losses.append(np.asarray(ctx.step(B, idx=idx, eps1=e1, eps2=e2), np.float32))
                if mode == "ustore":
                    for net in ("q1", "q2"):
                        out[f"update{u}.{net}.fc2.weight.grad"] = sha(ctx.get_net(net, "grad")["fc2.weight"])
        for net in NETS:
            for k, v in ctx.get_net(net).items():
                out[f"{net}.{k}"] = sha(v)
            if net in ("policy", "q1", "q2"):
                for slot in ("m", "v"):
                    for k, v in ctx.get_net(net, slot).items():
                        out[f"{net}.{k}.{slot}"] = sha(v)
        for name, sid in (("log_alpha", L.S_LOG_ALPHA), ("log_alpha.m", L.S_ADAM_M_LOG_ALPHA),
                          ("log_alpha.v", L.S_ADAM_V_LOG_ALPHA)):
            out[name] = sha(np.array([ctx.get_scalar(sid)]), np.float64)
        rec = {"losses": [[float(v).hex() for v in row] for row in losses], "sha256": out}
        if mode == "clip":     # per update: the three pre-clip norms, the three coefficients
            norms = np.asarray(ctx.fetch_grad_norms(n)[0], np.float32)
            rec["grad_norms"] = [[float(v).hex() for v in row] for row in norms]
    finally:
        ctx.close()
    return rec


def main(argv):
    out = argv[1] if len(argv) > 1 else os.path.join(ROOT, "tests", "golden", "dw_level_bits.json")
    rec = {case[0]: run_bits(case) for case in CASES}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main(sys.argv)
