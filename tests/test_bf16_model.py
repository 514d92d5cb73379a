"""The bf16 level model pinned on the host (no GPU): oracle/bf16_model.py is what
tests/test_gpu_bf16_levels.py holds k_fwd16 / k_fwd16p, k_axk16 and k_dw_part16 + k_dw_fin to.

* rne is torch's fp32 -> bf16 conversion bit for bit (ties to even and to odd, the largest
  finite values rounding to inf, subnormals, +-0, values already bf16), and the kernels still
  round at staging with the conversion it models;
* a product of two bf16 values is exact in fp32: the property the GPU bars rest on;
* rowsum_order32 repeats the split-K row sums thread for thread;
* a broken model breaks the bar: on operands drawn as the GPU cases draw them (K = 394, 512,
  4096; ReLU'd activations, half-masked gradients, xavier weights) a product dropped at
  k = 0, 31, 32, 63, 64, K - 2, K - 1 (for the weight gradient, K = the batch: a batch row
  dropped), or truncation for rne on either operand, exceeds the level's bar on >= 99 % of the
  outputs it touches.  fp32-stored outputs: every output whose dropped product is nonzero
  (truncation: every output).  bf16-stored outputs (the act16 forward levels) are compared
  through the monotone bounds; a bf16 store cannot show a move of the fp32 value below its own
  spacing on a single element, so an output counts as touched where the ReLU passes it and the
  mutation moves the pre-activation by at least one bf16 ulp of it - and, whatever the moves,
  every sampled row (the GPU test checks all columns of a row) must hold a violation."""
import math
import pathlib
import re

import numpy as np
import pytest
import torch

from oracle import bf16_model as M

KERNELS = pathlib.Path(__file__).resolve().parents[1] / "humanoid-walking-with-sac_amd" / "csrc" / "kernels.hip"
SHARE = 0.99


def from_bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


def torch_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def test_rne_is_torch_bf16_bit_for_bit():
    rng = np.random.default_rng(1)
    u = rng.integers(0, 1 << 32, 400000, dtype=np.uint64).astype(np.uint32)
    u = u[(u & 0x7FFFFFFF) <= 0x7F800000]                       # every finite pattern class, +-inf
    assert same_bits(M.rne(from_bits(u)), torch_bf16(from_bits(u)))
    x = (rng.standard_normal(100000) * 0.1).astype(np.float32)
    assert same_bits(M.rne(x), torch_bf16(x))
    edges = {0x3F808000: 0x3F800000,    # tie, even below: down
             0x3F818000: 0x3F820000,    # tie, odd below: up
             0x3F808001: 0x3F810000,    # just past the tie: up
             0x3F807FFF: 0x3F800000,    # just under it: down
             0x7F7FFFFF: 0x7F800000,    # the largest finite fp32 -> inf
             0x7F7F8000: 0x7F800000,    # tie above the largest bf16 (odd): up, to inf
             0x7F7F7FFF: 0x7F7F0000,    # the largest value that stays finite
             0x00000001: 0x00000000, 0x00008000: 0x00000000, 0x00018000: 0x00020000,   # subnormals
             0x00008001: 0x00010000, 0x007FFFFF: 0x00800000,                           # ... up to normal
             0x00000000: 0x00000000, 0x80000000: 0x80000000,                           # +-0
             0x3F810000: 0x3F810000, 0x42FF0000: 0x42FF0000, 0x7F800000: 0x7F800000}   # already bf16
    src = np.array(list(edges), np.uint32)
    for s in (src, src | np.uint32(0x80000000)):
        want = np.array([edges[int(k) & 0x7FFFFFFF] for k in s], np.uint32) | (s & np.uint32(0x80000000))
        assert np.array_equal(M.rne(from_bits(s)).view(np.uint32), want)
        assert same_bits(M.rne(from_bits(s)), torch_bf16(from_bits(s)))
    assert np.all(np.isnan(M.rne(from_bits([0x7FC00000, 0x7F800001, 0xFFFFFFFF]))))
    assert M.rne(np.ones((3, 5), np.float32)).shape == (3, 5)
    assert M.is_bf16(M.rne(x)) and not M.is_bf16(x) and same_bits(M.rne(M.rne(x)), M.rne(x))
    t = M.trunc(x)
    assert M.is_bf16(t) and np.all(np.abs(t) <= np.abs(x)) and np.all(np.abs(x - t) < np.abs(x) * 2.0 ** -7)
    assert same_bits(M.widen(np.array([0x3F80, 0xC2FF], np.uint16)), from_bits([0x3F800000, 0xC2FF0000]))


def test_kernels_round_at_staging_with_the_conversion_modelled():
    """pack_bf16x4 (every fp32 operand's way into LDS) and bf16_bits (the bf16 stores) are the
    compiler's float -> __bf16 conversion: round to nearest even."""
    text = KERNELS.read_text()
    body = re.search(r"u2v pack_bf16x4\(float4 v\) \{(.*?)\n\}", text, re.S).group(1)
    assert body.count("(__bf16)v.") == 4, body
    assert re.search(r"pack_bf16x2\(float lo, float hi\) \{\s*return \(uint32_t\)bf16_bits\(lo\)", text)


def test_bf16_products_are_exact_in_fp32():
    rng = np.random.default_rng(2)
    n = 1 << 20
    def draw():
        mant = rng.integers(0, 1 << 7, n, dtype=np.uint32) << np.uint32(16)
        expo = (rng.integers(-60, 61, n) + 127).astype(np.uint32) << np.uint32(23)
        sign = rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31)
        return from_bits(sign | expo | mant)
    a, b = draw(), draw()
    assert M.is_bf16(a) and M.is_bf16(b)
    p32 = a * b
    assert p32.dtype == np.float32
    assert np.array_equal(p32.astype(np.float64), a.astype(np.float64) * b.astype(np.float64))
    # ... and so dot16 of bf16 operands is the exact sum, to fp64 rounding
    x, w = M.rne(rng.standard_normal((4, 512)).astype(np.float32)), M.rne(rng.standard_normal((3, 512)).astype(np.float32))
    exact = np.array([[math.fsum(float(p) * float(q) for p, q in zip(r, c)) for c in w] for r in x])
    assert np.max(np.abs(M.dot16(x, w) - exact) / M.abs_dot16(x, w)) < 2.0 ** -48


def rowsum_by_thread(dy, ns):
    """k_dw_part16's row sums thread for thread (gload / swrite / dw_store_rowsum) + k_dw_fin."""
    B, N = dy.shape
    kc = ((B + ns - 1) // ns + 63) // 64 * 64
    out = np.zeros(N, np.float32)
    for n in range(N):
        total = None
        for sp in range(ns):
            kb, ke = sp * kc, min(B, sp * kc + kc)
            rs = [np.float32(0)] * 16
            for k0 in range(kb, max(ke, kb), 64):
                for kr0 in range(16):
                    for i in range(4):
                        k = k0 + kr0 + 16 * i
                        rs[kr0] = np.float32(rs[kr0] + (dy[k, n] if k < ke else np.float32(0)))
            v = rs[0]
            for g in range(1, 16):
                v = np.float32(v + rs[g])
            total = v if total is None else np.float32(total + v)
        out[n] = total
    return out


@pytest.mark.parametrize("B,ns", [(200, 3), (4096, 7), (4100, 7), (2048, 16), (130, 16), (64, 1)])
def test_rowsum_order32_is_the_kernels_order(B, ns):
    rng = np.random.default_rng(B + ns)
    dy = (rng.standard_normal((B, 3)) * 1e-4).astype(np.float32)
    got = M.rowsum_order32(dy, ns)
    assert got.dtype == np.float32 and same_bits(got, rowsum_by_thread(dy, ns))
    ints = rng.integers(-1000, 1000, (B, 5)).astype(np.float32)      # every order sums these exactly
    assert np.array_equal(M.rowsum_order32(ints, ns), ints.astype(np.float64).sum(0))
    z, sc = M.bias_grad(dy, False)
    depth = -(-B // ns // 16) + 16 + ns                              # adds behind one output
    assert np.max(np.abs(got - z) / sc) <= depth * 2.0 ** -24


def test_dw_split_plan():
    # config 5's critic level: 2 x (fc1 4 x 4, fc2 4 x 4, fc3 1 x 4) = 72 tiles -> 7 splits
    assert M.dw_tiles(512, 394) == 16 and M.dw_tiles(1, 512) == 4 and M.dw_tiles(34, 512) == 4
    assert M.dw_splits(72) == 7 and M.dw_splits(1) == 16 and M.dw_splits(600) == 1


# ---------------------------------------------------------------------------
# a broken model breaks the bar


def xavier(rng, n, k):
    b = math.sqrt(6.0 / (n + k))
    return rng.uniform(-b, b, (n, k)).astype(np.float32)


def relu16(rng, m, k):
    """stored act16 activations: ReLU'd, about half zeros, bf16."""
    return M.rne(np.maximum(rng.standard_normal((m, k)) * 0.3, 0).astype(np.float32))


def half_masked(rng, m, k, scale=1e-4):
    """a ReLU-backward gradient: fp32, about half its elements masked to zero."""
    return (rng.standard_normal((m, k)) * scale * (rng.random((m, k)) < 0.5)).astype(np.float32)


def level_operands(kind):
    """(x [R, K], w [N, K], bf16-stored output?) drawn as the GPU cases' levels are."""
    rng = np.random.default_rng({"fwd0": 11, "fwdh": 12, "dh": 13, "dw": 14}[kind])
    if kind == "fwd0":      # L1: [s | a | 1] against [W | b], K = 394
        x = np.concatenate([rng.standard_normal((256, 376)) * 0.1, rng.uniform(-0.4, 0.4, (256, 17)), np.ones((256, 1))], 1)
        w = np.concatenate([xavier(rng, 512, 393), rng.uniform(-0.02, 0.02, (512, 1))], 1)
        return x.astype(np.float32), w.astype(np.float32), True
    if kind == "fwdh":      # L2 ..: the GPU's own activations against W, K = 512
        return relu16(rng, 256, 512), xavier(rng, 512, 512), True
    if kind == "dh":        # L12 ..: a gradient against W, K = 512
        return half_masked(rng, 256, 512), xavier(rng, 512, 512), False
    return np.ascontiguousarray(half_masked(rng, 4096, 64).T), np.ascontiguousarray(relu16(rng, 4096, 512).T), False   # dW: K = B


def fp32_reference_error(x, w, z, scale):
    ref = (torch.from_numpy(M.rne(x)) @ torch.from_numpy(M.rne(w)).T).numpy().astype(np.float64)
    return (np.abs(ref - z) / scale).max()


def mutations(x, w):
    """name -> (mutant value, the outputs it touches at all)."""
    K = x.shape[1]
    out = {}
    for k in (0, 31, 32, 63, 64, K - 2, K - 1):
        xm = x.copy()
        xm[:, k] = 0
        out[f"product k = {k} dropped"] = (M.dot16(xm, w), np.outer(M.rne(x)[:, k], M.rne(w)[:, k]) != 0)
    everywhere = np.ones((len(x), len(w)), bool)
    if not M.is_bf16(x):
        out["truncation of x"] = (M.dot16(x, w, rx=M.trunc), everywhere)
    if not M.is_bf16(w):
        out["truncation of w"] = (M.dot16(x, w, rw=M.trunc), everywhere)
    return out


@pytest.mark.parametrize("kind", ["fwd0", "fwdh", "dh", "dw"])
def test_a_broken_model_breaks_the_bar(kind):
    x, w, stored16 = level_operands(kind)
    z, scale = M.dot16(x, w), M.abs_dot16(x, w)
    e_ref = fp32_reference_error(x, w, z, scale)
    bar = M.bar(e_ref)
    assert 0 < e_ref and bar == 4 * e_ref < M.CAP, e_ref      # (the cap is not what decides here)
    muts = mutations(x, w)
    assert len(muts) >= 8
    print(f"\n[bf16 mutations] {kind} K {x.shape[1]}: fp32 reference error {e_ref:.2e}, bar {bar:.2e}")
    for name, (zm, touched) in muts.items():
        if not stored16:
            seen = np.abs(zm - z) / scale > bar
            share = seen[touched].mean()
            print(f"  {name:26s} over the bar on {100 * share:.2f} % of {touched.sum()} outputs")
        else:
            lo, hi = M.stored_bounds(z, bar * scale)
            stored = M.rne(np.maximum(zm.astype(np.float32), 0))
            seen = (stored < lo) | (stored > hi)
            passed = touched & ((z > 0) | (zm > 0))
            ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.maximum(z, zm), 1e-300))) - 7)    # bf16 spacing at the value
            moved = passed & (np.abs(zm - z) >= ulp)
            share = seen[moved].mean()
            print(f"  {name:26s} outside the bounds on {100 * share:.2f} % of the {moved.sum()} outputs moved by >= 1 bf16 ulp "
                  f"({100 * seen[passed].mean():.1f} % of the {passed.sum()} the ReLU passes)")
            assert moved.sum() >= 1000, name                   # (the share is over something)
            rows = touched.any(1)
            assert np.all(seen[rows].any(1)), (name, "a sampled row without a violation")
        assert share >= SHARE, (kind, name, share)


# ---------------------------------------------------------------------------
# the MI355X's own outputs (tests/golden/bf16_levels_gpu.npz, written by
# tests/test_gpu_bf16_levels.py under SACMI_RECORD_BF16_LEVELS: slices of L2 (q1, pass 0), L12 and
# L6 (q1.fc2) of the (376, 17, 512) batch-4096 case) against the model and against broken models

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "bf16_levels_gpu.npz"


def within_fp32_bar(got, x, w, z, scale):
    live = scale > 0
    bar = M.bar(fp32_reference_error(x, w, np.where(live, z, 0), np.where(live, scale, 1)))
    return np.all(got[~live] == 0) and np.all(np.abs(got - z)[live] <= bar * scale[live])


def drop_k(x, k):
    y = x.copy()
    y[:, k] = 0
    return y


def test_recorded_gpu_outputs_go_red_under_a_broken_model():
    g = np.load(GOLDEN)
    # forward (bf16-stored): inside the bounds; red with W truncated or the slab's last k dropped
    x, w, b, got = M.widen(g["fwd_x"]), g["fwd_w"], g["fwd_b"], M.widen(g["fwd_got"])
    def fwd_ok(xm, rw):
        z = M.dot16(xm, w, rw=rw) + b.astype(np.float64)
        scale = M.abs_dot16(x, w) + np.abs(b.astype(np.float64))
        lo, hi = M.stored_bounds(z, M.bar(fp32_reference_error(x, w, M.dot16(x, w), M.abs_dot16(x, w))) * scale)
        return np.all((lo <= got) & (got <= hi))
    assert fwd_ok(x, M.rne)
    assert not fwd_ok(x, M.trunc) and not fwd_ok(drop_k(x, 63), M.rne) and not fwd_ok(drop_k(x, 511), M.rne)
    # dh (fp32-stored, masked)
    dy, w, below, got = g["dh_dy"], g["dh_w"], M.widen(g["dh_below"]), g["dh_got"]
    wt = np.ascontiguousarray(w.T)
    def dh_ok(dym, rx, rw):
        m = below > 0
        return within_fp32_bar(got, dy, wt, M.dot16(dym, wt, rx, rw) * m, M.abs_dot16(dy, wt) * m)
    assert dh_ok(dy, M.rne, M.rne)
    assert not dh_ok(dy, M.trunc, M.rne) and not dh_ok(dy, M.rne, M.trunc)
    assert not dh_ok(drop_k(dy, 63), M.rne, M.rne) and not dh_ok(drop_k(dy, 510), M.rne, M.rne)
    # dW (fp32-stored, K = the batch) and its row-sum bias gradient
    dyt, xt, got = np.ascontiguousarray(g["dw_dy"].T), np.ascontiguousarray(M.widen(g["dw_x"]).T), g["dw_got"]
    def dw_ok(dym, rx):
        return within_fp32_bar(got, dyt, xt, M.dot16(dym, xt, rx=rx), M.abs_dot16(dyt, xt))
    assert dw_ok(dyt, M.rne)
    assert not dw_ok(dyt, M.trunc)
    touched = [b for b in (63, 4095, 2047) if np.any(np.outer(M.rne(dyt)[:, b], xt[:, b]) != 0)]
    assert touched and all(not dw_ok(drop_k(dyt, b), M.rne) for b in touched)      # a batch row lost
    ns = int(g["dw_splits"])
    assert same_bits(M.rowsum_order32(g["dw_dy"], ns), g["dw_bias_got"])
    assert not same_bits(M.rowsum_order32(g["dw_dy"][:-1], ns), g["dw_bias_got"])
