"""The weight-gradient levels (L6 critic dW, L13 policy dW) on the k_gemm kernels that compile
the two row-contiguous cores alone (kRowsDw), and the u side store of the spread dh level,
which picks its storing core once per workgroup.

Neither change may move a bit: tests/golden/dw_level_bits.json was written by
tools/gen_dw_level_bits.py on the commit BEFORE both (the dispatching dW kernels, the
range-dropped side stores in every dh workgroup), and every loss, parameter, Adam moment
and the log_alpha state must reproduce it.

Cases (tools/gen_dw_level_bits.py CASES), fp32 and bf16 each:
  S11-A3-H96-B40       both dW levels on the 16-way K split of the 32x64 tiles; staged
                       updates, one 6-update launch (the sampler and gather riding in
                       L12 / L13), and with clipping on (the plain dW form plus k_adam)
  S376-A17-H512-B256   the critic dW level on the 64x64 two-wave-group tiles (496 32x64 tiles
                       are more than 256: the smallest natural shape that gets there)
  S11-A3-H96-B40 and S11-A3-H512-B64 with the gradients kept: the critics' fc2 weight
                       gradient, the only reader of the rows L5 stores through ax_out, after
                       each of 4 updates — the storing core still stores
"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_dw_level_bits", os.path.join(ROOT, "tools", "gen_dw_level_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

CASE_IDS = [c[0] for c in gen.CASES]


@pytest.fixture(scope="module")
def golden_bits(golden_dir):
    with open(os.path.join(golden_dir, "dw_level_bits.json")) as f:
        return json.load(f)


def test_shapes_reach_both_dw_forms():
    """Tile counts of the critic dW level (two critics, fc1 + fc2 + fc3 each; the bias
    gradients are the row sums): at most 256 32x64 tiles at the small shape (the 16-way
    form), more at the Humanoid shape (the 64x64 form)."""
    def tiles(S, A, H):
        t = lambda m, n: ((m + 31) // 32) * ((n + 63) // 64)
        return 2 * (t(H, S + A) + t(H, H) + t(1, H))
    S, A, H = gen.SHAPES["S11-A3-H96-B40"][:3]
    assert tiles(S, A, H) <= 256
    S, A, H = gen.SHAPES["S376-A17-H512-B256"][:3]
    assert tiles(S, A, H) == 496


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_dw_levels_run_k_gemm(dtype):
    """The launch timeline's kernel and grid of L6 / L13: k_gemm at both shapes; L6's grid at
    the Humanoid shape is that of 64x64 tiles (256 of them and the workgroups riding along:
    fewer than the 496 32x64 tiles), at the small shape and for L13 that of one 32x64 tile per
    workgroup (at most 256, and the workgroups riding along)."""
    for shape in ("S11-A3-H96-B40", "S376-A17-H512-B256"):
        case = (f"{shape}-{dtype}-timeline", shape, dtype, "staged", 1)
        ctx, _, _ = gen.make_ctx(case)
        try:
            ks, _ = ctx.profile_timeline(gen.SHAPES[shape][3], 1)
        finally:
            ctx.close()
        by_site = {}
        for k in ks:
            by_site.setdefault(k["site"], []).append((k["kernel"], k["grid"]))
        (k6, g6), = by_site["gemm_L6_critic_dW_adam"]
        (k13, g13), = by_site["gemm_L13_pi_dW_adam"]
        assert k6 == k13 == "k_gemm", (shape, dtype, k6, k13)
        if shape == "S376-A17-H512-B256":
            assert 256 <= g6 < 496 and g13 <= 256 + 64, (shape, dtype, g6, g13)
        else:
            assert g6 <= 256 and g13 <= 256 + 64, (shape, dtype, g6, g13)


@pytest.mark.parametrize("case", gen.CASES, ids=CASE_IDS)
def test_dw_level_bit_pin(case, golden_bits):
    """Every loss (hex float) and the sha256 of every parameter tensor, Adam moment and of the
    log_alpha state equal the record taken before the change, bit for bit; the clipped cases'
    norms and coefficients too (and their clipping engages), the side-store cases' fc2 critic
    weight gradients after every update too."""
    got = gen.run_bits(case)
    want = golden_bits[case[0]]
    assert got["losses"] == want["losses"], (case[0], got["losses"], want["losses"])
    diff = sorted(k for k in want["sha256"] if got["sha256"].get(k) != want["sha256"][k])
    assert not diff and set(got["sha256"]) == set(want["sha256"]), (case[0], diff)
    if case[3] == "clip":
        assert got["grad_norms"] == want["grad_norms"], (case[0], got["grad_norms"])
        coef = [[float.fromhex(v) for v in row[3:]] for row in got["grad_norms"]]
        assert len(coef) == case[4] and all(min(col) < 1.0 for col in zip(*coef)), (case[0], coef)
    if case[3] == "ustore":
        grads = [k for k in want["sha256"] if k.endswith("fc2.weight.grad")]
        assert len(grads) == 2 * case[4], (case[0], grads)
