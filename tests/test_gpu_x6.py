"""The batch-4096 fp32 GEMM kernels (k_fwd_x6, k_axk_x6, k_dw_part_x6) on adversarial data,
through the C ABI.

The other batch-4096 tests run N(0, 0.1^2) states against xavier weights: random mantissas,
mixed signs, normwise bars.  There the x6 approximation looks like rounding noise and a
missing kept plane (about 2^-15 |ab| per product) averages down to the bars.  Here:

(a) every forward level of one update is compared ELEMENTWISE with the bit-faithful model
    oracle/x6_model.py (relu(dot6(x, W) + b), each level from its own operands: the batch for
    layer 0, the GPU's own layer l-1 activations for layer l, so errors do not compound), on
    the worst mantissa the split allows (`adv`, 0x00ffff), on all-ones mantissas, and on
    all-positive data where the one-signed truncation bias and a missing plane are coherent.
    error = |gpu - value| / (sum_k |x_k||W_k| + |b|).  Bars, per level:
      gpu vs model <= min(4 x the fp32 reference's own max error on these operands, 2^-17)
      gpu vs fp64  <= 2^-21 + that                   (the design bound, kernels.hip "x6")
    The reference's own error is torch's CPU fp32 F.linear against fp64 on the same operands
    (the project's standing 4x margin); the 2^-17 cap keeps a dropped plane on the `adv` and
    `ones` mantissas (>= 1.5e-5 = 2^-16, tests/test_x6_model.py) from ever fitting.  ReLU is
    1-Lipschitz, so |relu(gpu_pre) - relu(model_pre)| <= |gpu_pre - model_pre|: no element is
    skipped, whatever its pre-activation's distance from zero.
    Layer 0 carries its bias inside K (x = [s | 1 | a] against [W | b]: 1 splits to h alone, so
    b enters through the kept products bh, bm, bl, exactly); later layers add it in fp32 in the
    epilogue (FwdEpi::store).  Both are dot6(x, W) + b to within one rounding of the result.
(b) the masked-truth gradient check of test_step_humanoid_b4096_under_gpu_masks (k_axk_x6,
    k_dw_part_x6 and the forward levels together) on the `adv` and `ones` mantissas, mixed
    signs, at the project's own bars.  Same-sign data is not used for gradients: the reference's
    own fp32 step is 4.5e-2 from fp64 there.
(c) (a) at batch 4000: row counts that are no multiple of the 128-row tile, still on k_fwd_x6.

Every case asserts from the launch timeline that the levels it checks ran on the x6 kernels,
and prints them."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import x6_model as X
from oracle.sac_step import NETS, SacConfig, init_params, param_shapes, synthetic_rows

pytestmark = pytest.mark.gpu

H = 512                 # with batch >= 4000 the smallest shape the x6 selectors take: 512 tiles
MAIN = (376, 17)        # K = 394 / 377 at layer 0 (10- and 25-column tails of the 32-deep slab)
SHORT_K = (20, 4)       # K = 25 / 21: less than one slab
CAP = 2.0 ** -17
TILE = 128              # k_fwd_x6's row tile


@functools.lru_cache(maxsize=None)
def base_data(S, A, n_hidden):
    """The draw of test_step_humanoid_b4096_under_gpu_masks (same seeds), before recasting."""
    cfg = SacConfig(S, A, H, n_hidden=n_hidden)
    return cfg, init_params(cfg, 101, bias_scale=0.02), synthetic_rows(cfg, 6000, 102, state_scale=0.1)


def class_data(S, A, n_hidden, cls, positive):
    """Hidden layers' weights and s, a, s' recast to the class; heads, the critics' last layer
    and every bias as drawn."""
    cfg, params, rows = base_data(S, A, n_hidden)
    hidden = {f"fc{i}.weight" for i in range(1, n_hidden + 1)}
    params = {n: {k: (X.recast(v, cls, positive) if k in hidden else v.copy()) for k, v in params[n].items()}
              for n in NETS}
    s, a, r, s2, d = rows
    rows = (X.recast(s, cls, positive), X.recast(a, cls, positive), r, X.recast(s2, cls, positive), d)
    return cfg, params, rows


def fwd_sites(n_hidden):
    """timeline site -> the (pass, layer) activations it writes, for the levels checked here."""
    sites = {"gemm_L1_fc1": [(0, 0), (3, 0)], "gemm_L2_fc2": [(0, 1), (3, 1)],
             "gemm_L4_tgt_fc2": [(1, 1)], "gemm_L8_act_fc2": [(2, 1)]}
    if n_hidden == 3:
        sites.update({"gemm_L2b_fc3": [(0, 2), (3, 2)], "gemm_L4b_tgt_fc3": [(1, 2)], "gemm_L8b_act_fc3": [(2, 2)]})
    return sites


def assert_kernels(ctx, B, want, what):
    """The launch timeline's kernels per site (it replays whole updates: call it once
    everything of the checked update is read back)."""
    ks, _ = ctx.profile_timeline(B, 1)
    by_site = {}
    for k in ks:
        by_site.setdefault(k["site"], []).append(k["kernel"])
    got = {site: by_site.get(site) for site in want}
    print(f"\n[x6 kernels] {what}: " + ", ".join(f"{s} {'+'.join(k or ['-'])}" for s, k in got.items()))
    for site, kernels in want.items():
        assert got[site] == kernels, (what, site, got[site], "wanted", kernels)


def tile_rows(M, seed):
    """Row sample of an M-row operand: of every 128-row tile its first and last row plus 6
    others (all columns are checked)."""
    rng = np.random.default_rng(seed)
    out = []
    for r0 in range(0, M, TILE):
        r1 = min(r0 + TILE, M)
        inner = rng.choice(np.arange(r0 + 1, r1 - 1), 6, replace=False)
        out += [r0, r1 - 1, *sorted(inner)]
    return np.array(out)


def level_errors(x, w, b, got):
    """One level on sampled rows: x [R, K], w [N, K], b [N] (fp32), got [R, N] the GPU's
    post-ReLU output.  Returns (max error vs model, vs fp64, the fp32 reference's own vs
    fp64, min |z| / max |z| of the model's pre-activations, mean signed error vs model)."""
    scale = X.abs_dot(x, w) + np.abs(b.astype(np.float64))
    z6 = X.dot6(x, w) + b.astype(np.float64)
    z64 = X.dot64(x, w) + b.astype(np.float64)
    ref = F.linear(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b)).numpy().astype(np.float64)
    g = got.astype(np.float64)
    e_model = np.abs(g - np.maximum(z6, 0)) / scale
    e_64 = np.abs(g - np.maximum(z64, 0)) / scale
    e_ref = np.abs(ref - z64) / scale
    signed = ((g - np.maximum(z6, 0)) / scale).mean()
    return e_model.max(), e_64.max(), e_ref.max(), np.abs(z6).min() / np.abs(z6).max(), signed


def run_forward_case(S, A, n_hidden, cls, positive, B):
    from sacmi import Config, Context
    cfg, params, rows = class_data(S, A, n_hidden, cls, positive)
    name = f"(S, A) = ({S}, {A}) B {B} n_hidden {n_hidden} {cls} {'all positive' if positive else 'mixed sign'}"
    ctx = Context(Config(S, A, H, max_batch=B, capacity=len(rows[2]), n_hidden=n_hidden), 0)
    for n in NETS:
        ctx.set_net(n, params[n])
    ctx.push(*rows)
    rng = np.random.default_rng(103)
    idx = rng.choice(len(rows[2]), B, replace=False)
    e1 = rng.standard_normal((B, A)).astype(np.float32)
    e2 = rng.standard_normal((B, A)).astype(np.float32)
    losses = ctx.step(B, idx=idx, eps1=e1, eps2=e2)
    assert np.all(np.isfinite(losses)), losses
    rq, rp = tile_rows(B, 1), tile_rows(2 * B, 2)          # critic passes: B rows a net; policy: 2B
    # sampled rows of every activation (the full readbacks are 16 MB each: not kept)
    act = {}
    for p in range(4):
        for l in range(n_hidden):
            h = ctx.read_activation(p, l, B)
            act[(p, l)] = h[rp].copy() if p == 3 else h[:, rq].copy()
    q_after = {n: ctx.get_net(n, "param", param_shapes(cfg)[n]) for n in ("q1", "q2")}   # pass 2's weights
    assert_kernels(ctx, B, {site: ["k_fwd_x6"] for site in fwd_sites(n_hidden)}, name)
    ctx.close()

    s, a, _, s2, _ = (v[idx] for v in rows)
    table = []
    def check(label, x, w, b, got):
        e_model, e_64, e_ref, zr, signed = level_errors(np.ascontiguousarray(x), w, b, got)
        bar = min(4 * e_ref, CAP)
        table.append((label, x.shape[1], e_model, e_64, e_ref, bar, zr, signed))
    for i, n in enumerate(("q1", "q2")):
        check(f"pass 0 {n} layer 0", np.concatenate([s, a], 1)[rq], params[n]["fc1.weight"], params[n]["fc1.bias"],
              act[(0, 0)][i])
        for p, wsrc in ((0, params[n]), (1, params[f"{n}_target"]), (2, q_after[n])):
            for l in range(1, n_hidden):
                check(f"pass {p} {n} layer {l}", act[(p, l - 1)][i], wsrc[f"fc{l + 1}.weight"], wsrc[f"fc{l + 1}.bias"],
                      act[(p, l)][i])
    pol = params["policy"]
    check("pass 3 policy layer 0", np.concatenate([s2, s], 0)[rp], pol["fc1.weight"], pol["fc1.bias"], act[(3, 0)])
    for l in range(1, n_hidden):
        check(f"pass 3 policy layer {l}", act[(3, l - 1)], pol[f"fc{l + 1}.weight"], pol[f"fc{l + 1}.bias"], act[(3, l)])

    print(f"[x6 forward] {name}: max |gpu - value| / (sum|x||W| + |b|) on {len(rq)} of {B} / {len(rp)} of {2 * B} rows")
    for label, K, e_model, e_64, e_ref, bar, zr, signed in table:
        ok = e_model <= bar and e_64 <= X.DROP_BOUND + bar
        print(f"  {label:24s} K {K:3d}  vs model {e_model:.2e} (mean {signed:+.1e}, bar {bar:.2e})  vs fp64 {e_64:.2e} "
              f"(bar {X.DROP_BOUND + bar:.2e})  fp32 ref vs fp64 {e_ref:.2e}  min|z|/max|z| {zr:.1e}  {'ok' if ok else 'OVER'}")
    print(f"  [x6 summary] {name}: vs model {max(t[2] for t in table):.2e}  vs fp64 {max(t[3] for t in table):.2e}  "
          f"fp32 ref {max(t[4] for t in table):.2e}")
    over = [(t[0], t[2], t[3], t[5]) for t in table if t[2] > t[5] or t[3] > X.DROP_BOUND + t[5]]
    assert not over, (name, over)


FWD_CLASSES = [("adv", False), ("adv", True), ("rand", True), ("ones", False)]
FWD_IDS = ["adv-mixed", "adv-positive", "rand-positive", "ones-mixed"]


@pytest.mark.parametrize("n_hidden", [2, 3])
@pytest.mark.parametrize("cls,positive", FWD_CLASSES, ids=FWD_IDS)
def test_forward_levels_match_model(cls, positive, n_hidden):
    """Measured on the MI355X (max over the levels of a case, K = 377 .. 512; n_hidden 2 / 3):
      class          gpu vs model         gpu vs fp64          fp32 reference vs fp64
      adv mixed      7.5e-8 / 8.7e-8      1.9e-7 / 2.0e-7      1.3e-7 / 1.5e-7
      adv positive   3.3e-7 / 3.3e-7      7.0e-7 / 7.1e-7      7.8e-7 / 8.3e-7
      rand positive  3.4e-7 / 3.0e-7      3.5e-7 / 3.5e-7      7.2e-7 / 6.8e-7
      ones mixed     8.0e-8 / 7.8e-8      9.7e-8 / 1.0e-7      1.4e-7 / 1.5e-7
    gpu vs model is k_fwd_x6's fp32 accumulation error with each slab's six products summed
    on their own (x6_mfma<true>).  With every product chained through the running accumulator
    (the kernel's first form) it was 2.9e-7 / 3.4e-7, 1.4e-6 / 1.5e-6, 1.5e-6 / 1.5e-6 and
    3.8e-7 / 4.8e-7, and layer 0 of `ones` mixed missed its bar (3.2e-7 .. 4.8e-7 against
    1.5e-7 .. 1.8e-7: on all-ones operands the fp32 reference is nearly exact, 4e-8, see
    tests/test_x6_model.py test_slab_sum_chain_fits_the_fp32_reference_bar)."""
    run_forward_case(*MAIN, n_hidden, cls, positive, 4096)


@pytest.mark.parametrize("cls,positive", FWD_CLASSES, ids=FWD_IDS)
def test_forward_levels_match_model_short_k(cls, positive):
    """K = 25 / 21 at layer 0: a single, partly filled 32-deep slab."""
    run_forward_case(*SHORT_K, 2, cls, positive, 4096)


def test_forward_levels_match_model_ragged_batch():
    """Batch 4000: 31.25 row tiles a critic, 62.5 for the policy's 2B rows (the last tile's
    clamped rows), the levels 64 columns wide to reach 512 tiles."""
    run_forward_case(*MAIN, 2, "adv", True, 4000)


@pytest.mark.parametrize("n_hidden", [2, 3])
@pytest.mark.parametrize("cls", ["adv", "ones"])
def test_update_under_gpu_masks_worst_mantissas(cls, n_hidden):
    """The dh and weight-gradient kernels (with the forward levels) on the worst mantissas,
    mixed signs: fp64 under the GPU's own ReLU masks, at the project's LOSS_TOL, FLIP_Z_TOL and
    MASKED_GRAD_TOL."""
    from test_gpu_parity import check_update_under_gpu_masks
    cfg, params, rows = class_data(*MAIN, n_hidden, cls, False)
    want = {site: ["k_fwd_x6"] for site in fwd_sites(n_hidden)}
    want.update({"gemm_L3_tgt_fc1": ["k_fwd_x6"], "gemm_L7_act_fc1": ["k_fwd_x6"],
                 "gemm_L5_critic_dh1": ["k_axk_x6"], "gemm_L9_act_dh1": ["k_axk_x6"], "gemm_L12_pi_dhp1": ["k_axk_x6"],
                 "gemm_L6_critic_dW_adam": ["k_dw_part_x6", "k_dw_fin"],
                 "gemm_L13_pi_dW_adam": ["k_dw_part_x6", "k_dw_fin"]})
    name = f"humanoid B4096 n_hidden {n_hidden} {cls} mantissas"
    check_update_under_gpu_masks(cfg, params, rows, 4096, name,
                                 after_readback=lambda ctx: assert_kernels(ctx, 4096, want, name))
