"""The row-prologue dh levels (L5 critic dh1, L9 actor dh1) on k_gemm, in both forms of the
prologue: the spread form of the 32x32 one-wave-group tiles (the dot partials two per thread
and summed by lane shuffles, the row coefficients formed per epilogue thread behind one
barrier) and the rows_load / rows_finish form of the 64-row two-wave-group tiles.

Shapes (tools/gen_dh_rows_bits.py CASES), the smallest that reach every branch of the prologue:
  S11-A3-H96-B40      3 partials per row, a row tile with 8 live rows, the tile-0 ax_out
                      store, the critic and the actor kind
  S376-A17-H512-B64   16 partials per row (kRowsPv), L9's dL/da partials
  S11-A3-H544-B40     17 partials per row: hidden 544 at batch 40 is 36 32x64 tiles, so the
                      level still lands on the 32x32 axk k_gemm tiles and the sum runs its
                      tail loop past kRowsPv
  S11-A3-H512-B1056   the smallest batch at hidden 512 on the 64-row tiles: 528 32x64 tiles
                      (> 512), 272 64x64 and 136 64x128 tiles (< 512: not k_axk_x6)

Bit pin: tests/golden/dh_rows_bits.json was written by tools/gen_dh_rows_bits.py on the commit
BEFORE the level moved to the spread form (the B 1056 record: before the prologue became a
property of the level); the prologue's sums keep their order, so every loss and every
parameter must come out bit for bit.  A later change which means to move these
bits regenerates the file with that tool and says why.
"""
import importlib.util
import json
import os

import pytest

from test_gpu_parity import GRAD_TOL, LOSS_TOL, check_step, flat_params, rel, run_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_dh_rows_bits", os.path.join(ROOT, "tools", "gen_dh_rows_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

CASE_IDS = [c[0] for c in gen.CASES]


@pytest.fixture(scope="module")
def golden_bits(golden_dir):
    with open(os.path.join(golden_dir, "dh_rows_bits.json")) as f:
        return json.load(f)


def test_cases_land_on_the_axk_k_gemm_tiles():
    """Every case's dh1 levels run on k_gemm (not k_axk16 / k_axk_x6).  The first three on the
    one-wave-group 32x32 tiles: at most 512 32x64 tiles over the two critics, which is also
    what makes the H 544 case reach the tail of the partial sum (17 partials > kRowsPv = 16).
    The B 1056 case on the 64-row two-wave-group tiles: more than 512 32x64 tiles, and fewer
    than 512 64x64 / 64x128 tiles (k_axk_x6 wants 512 of either)."""
    def tiles(B, H, tm, tn):
        return 2 * ((B + tm - 1) // tm) * ((H + tn - 1) // tn)
    for name, S, A, H, B, *_ in gen.CASES[:3]:
        assert tiles(B, H, 32, 64) <= 512, name
    name, S, A, H, B, *_ = gen.CASES[3]
    assert (tiles(B, H, 32, 64), tiles(B, H, 64, 64), tiles(B, H, 64, 128)) == (528, 272, 136), name
    assert [(c[3] + 31) // 32 for c in gen.CASES] == [3, 16, 17, 16]


# case -> gridDim.x of its dh1 levels: 2 descs x 6 32x32 tiles, each desc padded to 8
# workgroups; 2 descs x 136 64x64 tiles
DH1_GRIDS = {"S11-A3-H96-B40": 16, "S11-A3-H512-B1056": 272}


@pytest.mark.parametrize("name", sorted(DH1_GRIDS))
def test_dh1_levels_run_k_gemm(name):
    """The launch timeline's kernel and grid of L5 / L9: k_gemm in the 32x32 form at batch 40,
    in the 64-row form at batch 1056."""
    from oracle.sac_step import NETS
    from sacmi import Config, Context
    case = next(c for c in gen.CASES if c[0] == name)
    cfg, params, rows, _ = gen.case_inputs(case)
    B = case[4]
    ctx = Context(Config(cfg.state_dim, cfg.action_dim, cfg.hidden_dim, max_batch=B, capacity=len(rows[2])), 0)
    try:
        for n in NETS:
            ctx.set_net(n, params[n])
        ctx.push(*rows)
        ks, _ = ctx.profile_timeline(B, 1)
    finally:
        ctx.close()
    by_site = {}
    for k in ks:
        by_site.setdefault(k["site"], set()).add((k["kernel"], k["grid"]))
    for site in ("gemm_L5_critic_dh1", "gemm_L9_act_dh1"):
        assert by_site.get(site) == {("k_gemm", DH1_GRIDS[name])}, (name, site, by_site.get(site))


@pytest.mark.parametrize("case", gen.CASES, ids=CASE_IDS)
def test_dh_rows_bit_pin(case, golden_bits):
    """6 updates: every loss (hex float) and the sha256 of every parameter tensor and of
    log_alpha equal the record taken before the change, bit for bit."""
    got = gen.run_bits(case)
    want = golden_bits[case[0]]
    assert got["losses"] == want["losses"], (case[0], got["losses"], want["losses"])
    diff = sorted(k for k in want["sha256"] if got["sha256"].get(k) != want["sha256"][k])
    assert not diff and set(got["sha256"]) == set(want["sha256"]), (case[0], diff)


@pytest.mark.parametrize("case", gen.CASES, ids=CASE_IDS)
def test_dh_rows_vs_oracle(case):
    """One update against OracleSAC in fp64 at the parity tests' bar for batch <= 1024:
    losses within 1e-5, every gradient tensor within 1e-5 normwise (and check_step's
    parameter-delta and alpha-state checks)."""
    cfg, params, rows, _ = gen.case_inputs(case)
    _, out = run_case(cfg, params, rows, B=case[4], steps=1, seed=case[7] + 3000)
    lg, _, gg = out[0]["gpu"]
    l64, _, g64 = out[0]["o64"]
    errs = {k: rel(gg[k], v) for k, v in g64.items()}
    lerr = {k: abs(lg[i] - l64[k]) / max(abs(l64[k]), 1e-3) for i, k in enumerate(("q1_loss", "q2_loss", "policy_loss"))}
    print(f"\n[dh rows vs fp64] {case[0]} losses {lerr} worst grad {max(errs.items(), key=lambda kv: kv[1])}")
    check_step(out[0], flat_params(params), f"dh rows {case[0]}")
    assert all(e <= LOSS_TOL for e in lerr.values()), (case[0], lerr)
    over = {k: e for k, e in errs.items() if e > GRAD_TOL}
    assert not over, (case[0], over)
