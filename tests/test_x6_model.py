"""The x6 numerics pinned to a model (no GPU): oracle/x6_model.py repeats the three-way bf16
split (x6_split4) and the six kept products (x6_mfma) of the batch-4096 fp32 GEMM kernels.
Checked here, on mantissas chosen to be the worst the design allows and on same-sign dots
where its one-signed truncation bias cannot average out:

* the split's algebra (exact sum, bf16 parts, signs, nothing left after the third part) on
  its domain |x| >= 2^-110 or x == 0, and that the domain ends there;
* the dropped products per scalar product: 0 <= (ab - kept) / |ab| <= 2^-21, reached to
  within 2.3 % on the `adv` mantissa 0x00ffff;
* dots of K = 24 / 393 / 512: |dot6 - fp64| <= 2^-21 sum|a||b| everywhere, negative on
  same-sign data, and on random same-sign data below what an fp32 reference loses to rounding
  on the same operands (why a truncating split is acceptable);
* the kernel source still performs the operations the model repeats.

tests/test_gpu_x6.py holds the kernels to this model elementwise."""
import pathlib
import re

import numpy as np
import pytest
import torch

from oracle import x6_model as X

KERNELS = pathlib.Path(__file__).resolve().parents[1] / "humanoid-walking-with-sac_amd" / "csrc" / "kernels.hip"


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def from_bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


def drawn(n, seed, e_lo, e_hi):
    """n fp32 values of either sign, random mantissas, binary exponents uniform in [e_lo, e_hi]."""
    rng = np.random.default_rng(seed)
    mant = rng.integers(0, 1 << 23, n, dtype=np.uint32)
    expo = (rng.integers(e_lo, e_hi + 1, n) + 127).astype(np.uint32)
    sign = rng.integers(0, 2, n, dtype=np.uint32)
    return from_bits((sign << np.uint32(31)) | (expo << np.uint32(23)) | mant)


def domain_classes():
    """{name: fp32 values inside the split's exact domain}."""
    base = drawn(20000, 1, -110, 127)
    pow2 = from_bits(np.arange(1, 255, dtype=np.uint32) << np.uint32(23))        # 2^-126 .. 2^127
    pow2 = pow2[np.abs(pow2) >= X.EXACT_MIN]
    edge = drawn(4000, 2, -110, -110)                                            # 2^-110 (1 .. 2)
    out = {"adv": X.recast(base, "adv"), "ones": X.recast(base, "ones"), "rand": base,
           "adv+": X.recast(base, "adv", True), "ones+": X.recast(base, "ones", True),
           "rand+": X.recast(base, "rand", True),
           "pow2": np.concatenate([pow2, -pow2]), "zero": np.array([0.0, -0.0], np.float32),
           "edge_adv": X.recast(edge, "adv"), "edge_ones": X.recast(edge, "ones"), "edge_rand": edge,
           "edge_lo": np.array([2.0 ** -110, -(2.0 ** -110)], np.float32)}
    for k, v in out.items():
        assert np.all((np.abs(v) >= X.EXACT_MIN) | (v == 0)), k
    return out


@pytest.mark.parametrize("name", sorted(domain_classes()))
def test_split_is_exact_on_its_domain(name):
    x = domain_classes()[name]
    h, m, l, s = X.split_steps(x)
    f64 = np.float64
    assert np.array_equal(h.astype(f64) + m.astype(f64) + l.astype(f64), x.astype(f64))
    assert np.array_equal(bits(l), bits(s))                     # the third truncation drops nothing
    for part in (h, m, l):
        assert not np.any(bits(part) & np.uint32(0xFFFF)), "a part that is not a bf16"
        nz = part != 0
        assert np.array_equal(np.signbit(part[nz]), np.signbit(x[nz])), "a part against x's sign"
    # |m| < 2^-7 |x| and |l| < 2^-15 |x|: what the 2^-21 bound on the dropped products rests on
    ax = np.abs(x.astype(f64))
    assert np.all(np.abs(m.astype(f64)) <= ax * 2.0 ** -7) and np.all(np.abs(l.astype(f64)) <= ax * 2.0 ** -15)
    if name != "zero":
        assert np.all(np.abs(m.astype(f64))[ax > 0] < ax[ax > 0] * 2.0 ** -7)


def test_split_loses_bits_below_its_domain():
    """The documented end of the domain: under 2^-110 the remainders are fp32 subnormals with
    bits below 2^-133, the bf16 truncation drops them, and h + m + l falls short of x by less
    than 2^-133 (at most 16 bits) — always toward zero.  The workload never produces such
    operands; no GPU test runs them."""
    f64 = np.float64
    tiny = X.recast(drawn(4000, 3, -126, -111), "ones")                 # normal, below 2^-110
    sub = from_bits(np.concatenate([np.arange(1, 1 << 12, dtype=np.uint32),
                                    np.uint32(0x7FFFFF) - np.arange(0, 1 << 12, dtype=np.uint32)]))
    sub = np.concatenate([sub, -sub])                                   # fp32 subnormals
    for name, x in (("tiny", tiny), ("subnormal", sub)):
        assert np.all(np.abs(x) < X.EXACT_MIN)
        h, m, l, s = X.split_steps(x)
        got = h.astype(f64) + m.astype(f64) + l.astype(f64)
        lost = x.astype(f64) - got
        assert np.all(np.abs(lost) < 2.0 ** -133), name
        assert np.all(lost * np.sign(x) >= 0), name                     # short toward zero
        for part in (h, m, l):
            assert not np.any(bits(part) & np.uint32(0xFFFF))
        # every value with a bit below 2^-133 loses it; the others are still exact
        low = (np.abs(x.astype(f64)) % 2.0 ** -133) != 0
        assert np.array_equal(lost != 0, low), name
        assert low.mean() > 0.9, (name, low.mean())
    assert np.all((tiny.astype(f64) - sum(p.astype(f64) for p in X.split(tiny))) != 0)
    # one ulp above the edge nothing is lost; one binade below it something is
    x = from_bits(np.array([0x08FFFFFF, 0x087FFFFF], np.uint32))        # 2^-110 (2 - 2^-23), 2^-111 (..)
    h, m, l = (p.astype(f64) for p in X.split(x))
    assert (h + m + l)[0] == f64(x[0]) and (h + m + l)[1] != f64(x[1])


def kept_and_exact(a, b, pairs=X.PAIRS):
    """Per scalar product, in float64 (every term and both sums exact: 48-bit products)."""
    pa = dict(zip("hml", (p.astype(np.float64) for p in X.split(a))))
    pb = dict(zip("hml", (p.astype(np.float64) for p in X.split(b))))
    kept = sum(pa[i] * pb[j] for i, j in pairs)
    return kept, a.astype(np.float64) * b.astype(np.float64)


@pytest.mark.parametrize("name", ["adv", "ones", "rand", "adv+", "ones+", "rand+", "pow2", "edge_ones"])
def test_dropped_products_bound_per_product(name):
    """0 <= (ab - kept) / |ab| <= 2^-21: one-signed (each product short toward zero) and bounded;
    on `adv` it sits in [2^-22, 2^-21] (by hand: (2 m l + l^2) / x^2 with m = 2^-7 - 2^-15,
    l = 2^-15 - 2^-23, x = 1 + 2^-7 - 2^-23, about 0.977 * 2^-21), so the bound is tight."""
    cls = domain_classes()
    a = cls[name]
    rng = np.random.default_rng(5)
    b = rng.permutation(a)          # (every product and part product is a normal float64)
    kept, exact = kept_and_exact(a, b)
    ratio = (exact - kept) / exact                  # sign of ab divided out
    print(f"\n[x6 per product] {name:9s} dropped/|ab|: min {ratio.min():.3e} mean {ratio.mean():.3e} "
          f"max {ratio.max():.3e} (2^-21 = {X.DROP_BOUND:.3e})")
    assert np.all(ratio >= 0) and np.all(ratio <= X.DROP_BOUND)
    if name in ("adv", "adv+"):
        assert np.all(ratio >= 2.0 ** -22)
        assert abs(ratio.max() / X.DROP_BOUND - 0.977) < 0.01 and ratio.min() / X.DROP_BOUND > 0.97
    if name == "pow2":
        assert np.all(ratio == 0)


def dot_operands(cls, positive, K, seed, M=96, N=80):
    """Workload-like magnitudes (rows ~ N(0, 0.1^2), weights ~ U(-b, b)) recast to a class."""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((M, K)) * 0.1).astype(np.float32)
    w = rng.uniform(-0.08, 0.08, (N, K)).astype(np.float32)
    return X.recast(a, cls, positive), X.recast(w, cls, positive)


def fp32_reference_errors(a, w):
    """Scaled errors against float64 of two fp32 evaluations of a @ w.T: torch's CPU matmul
    (what the reference implementation runs) and a plain sequential fp32 sum over k."""
    scale, exact = X.abs_dot(a, w), X.dot64(a, w)
    mm = (torch.from_numpy(a) @ torch.from_numpy(w).T).numpy().astype(np.float64)
    acc = np.zeros((a.shape[0], w.shape[0]), np.float32)
    for k in range(a.shape[1]):
        acc = acc + a[:, k, None] * w[None, :, k]              # fp32 product, fp32 add
    return (mm - exact) / scale, (acc.astype(np.float64) - exact) / scale


DOT_CLASSES = [("adv", False), ("adv", True), ("ones", False), ("ones", True), ("rand", False), ("rand", True)]


@pytest.mark.parametrize("K", [24, 393, 512])
def test_dot6_bias_against_fp64_and_fp32_reference(K):
    print(f"\n[x6 dot, K = {K}] scaled error (value - fp64) / sum|a||b|")
    stats = {}
    for cls, positive in DOT_CLASSES:
        a, w = dot_operands(cls, positive, K, 100 + K)
        e = (X.dot6(a, w) - X.dot64(a, w)) / X.abs_dot(a, w)
        e_mm, e_seq = fp32_reference_errors(a, w)
        stats[(cls, positive)] = (e, e_mm, e_seq)
        print(f"  {cls:4s} {'same-sign ' if positive else 'mixed-sign'}  x6 model: mean {e.mean():+.2e} max| {np.abs(e).max():.2e}"
              f"   fp32 matmul: mean {e_mm.mean():+.2e} max| {np.abs(e_mm).max():.2e}"
              f"   fp32 sequential: max| {np.abs(e_seq).max():.2e}")
        assert np.abs(e).max() <= X.DROP_BOUND, (cls, positive)
        if positive:        # every product short toward zero: no element can come out high
            assert e.max() <= 0 and e.mean() < 0, (cls, positive)
    # the worst mantissa on same-sign data sits right under the bound: the check is not vacuous
    assert -stats[("adv", True)][0].mean() >= 0.97 * 0.977 * X.DROP_BOUND
    # why the truncating split stays: its mean bias on random same-sign operands is below what
    # the fp32 reference itself loses on them
    e, e_mm, e_seq = stats[("rand", True)]
    assert abs(e.mean()) < np.abs(e_mm).max(), (e.mean(), np.abs(e_mm).max())
    assert abs(e.mean()) < np.abs(e_seq).max(), (e.mean(), np.abs(e_seq).max())


def test_a_missing_plane_cannot_hide_on_same_sign_data():
    """The control for the GPU bars: with any one of the small kept products (al.bh, ah.bl,
    am.bm) dropped from the model, every element of a same-sign dot on the `adv` and `ones`
    mantissas moves by more than the 2^-17 cap that tests/test_gpu_x6.py puts on
    |gpu - model| (adv: 3.0e-5 / 6.0e-5, ones: 1.5e-5), for every K it runs.  Random same-sign
    mantissas move by 6e-6 to 8e-6 at K >= 377 (2e-6 to 8e-6 at K <= 24) — around the cap, not
    above it: on that class a missing plane is caught by the 4x-fp32-reference part of the
    bar (about 1e-6 to 3e-6 there), not by the cap."""
    cap = 2.0 ** -17
    for K in (20, 24, 377, 394, 512):
        for cls in ("adv", "ones", "rand"):
            a, w = dot_operands(cls, True, K, 7 * K)
            full, scale = X.dot6(a, w), X.abs_dot(a, w)
            for drop in X.PAIRS[:3]:
                e = np.abs(X.dot6(a, w, tuple(p for p in X.PAIRS if p != drop)) - full) / scale
                if cls == "rand":
                    assert np.median(e) > cap / 2 and e.min() > cap / 8, (K, cls, drop, e.min(), np.median(e))
                else:
                    assert e.min() > 1.9 * cap, (K, cls, drop, e.min())


@pytest.mark.parametrize("K", [377, 394, 512])
def test_slab_sum_chain_fits_the_fp32_reference_bar(K):
    """The GPU test allows |gpu - model| 4x the fp32 reference's own error on the level's
    operands.  Why k_fwd_x6 sums each slab on its own (x6_mfma<true>): with every product chained
    through the running accumulator, even one rounding per MFMA (X.chain32(slab_sum=False)) is
    over that bar where the reference is unusually exact — mantissa 0x7fffff on BOTH operands
    puts every value one ulp under a power of two, the reference's products and partial sums
    are few-bit numbers that add almost without rounding (mixed signs: 3e-8 to 4e-8, under one
    ulp of the scale), and 4x that is below the chained form's 1.8e-7 to 2.0e-7 (measured on
    the MI355X, with the MFMA's own internal roundings: 3.2e-7 to 4.8e-7).  The slab-sum form
    fits under the bar on every class, with a margin of 2 or more."""
    print(f"\n[x6 fp32 chains, K = {K}] max |chain32 - dot6| / sum|a||b| against 4x the fp32 references")
    for cls, positive in DOT_CLASSES:
        a, w = dot_operands(cls, positive, K, 100 + K, M=128, N=256)
        scale, z6 = X.abs_dot(a, w), X.dot6(a, w)
        e_slab = (np.abs(X.chain32(a, w) - z6) / scale).max()
        e_chained = (np.abs(X.chain32(a, w, slab_sum=False) - z6) / scale).max()
        e_mm, e_seq = (np.abs(v).max() for v in fp32_reference_errors(a, w))
        print(f"  {cls:4s} {'same-sign ' if positive else 'mixed-sign'}  slab sum {e_slab:.2e}   chained {e_chained:.2e}   "
              f"4x matmul {4 * e_mm:.2e}   4x sequential {4 * e_seq:.2e}")
        assert 2 * e_slab < 4 * min(e_mm, e_seq), (cls, positive, e_slab, e_mm, e_seq)
        if cls == "ones":
            assert e_chained > 4 * max(e_mm, e_seq), (cls, positive, e_chained, e_mm, e_seq)


# ---------------------------------------------------------------------------
# the tie to the kernel source: the model fails loudly when the kernels' split changes
def device_fn(name):
    src = KERNELS.read_text()
    heads = re.findall(rf"__device__ __forceinline__ void {name}\(", src)
    assert len(heads) == 1, f"one definition of {name}"
    body = src[src.index(heads[0]):]
    return body[:body.index("\n}\n")]


def v_perm_b32(s0, s1, sel):
    """__builtin_amdgcn_perm(s0, s1, sel): result byte i is byte sel[i] of the 8 bytes {s1, s0}
    (s1 the low four); selectors 0-7 only."""
    src = (int(s0) << 32) | int(s1)
    return sum((((src >> (8 * ((sel >> (8 * i)) & 0xFF))) & 0xFF) << (8 * i)) for i in range(4))


def test_model_matches_kernel_source():
    split = device_fn("x6_split4")
    # per value: two remainders x - trunc(x), r - trunc(r), each truncation a 0xffff0000 mask
    # (the function handles two values per loop pass: x0, x1)
    assert len(re.findall(r"& 0xffff0000u", split)) == 4
    for rem in (r"r0 = x0 - __uint_as_float\(u0 & 0xffff0000u\)", r"r1 = x1 - __uint_as_float\(u1 & 0xffff0000u\)",
                r"s0 = r0 - __uint_as_float\(v0 & 0xffff0000u\)", r"s1 = r1 - __uint_as_float\(v1 & 0xffff0000u\)"):
        assert len(re.findall(rem, split)) == 1, rem
    assert "u0 = __float_as_uint(x0), u1 = __float_as_uint(x1)" in split
    assert "v0 = __float_as_uint(r0), v1 = __float_as_uint(r1)" in split
    # the three parts are the top halves of x, r and s, packed by one byte permute each
    perms = re.findall(r"p([hml])\[d\] = __builtin_amdgcn_perm\((.+?), (.+?), (0x[0-9a-f]+)u\);", split)
    assert perms == [("h", "u1", "u0", "0x07060302"), ("m", "v1", "v0", "0x07060302"),
                     ("l", "__float_as_uint(s1)", "__float_as_uint(s0)", "0x07060302")], perms
    assert v_perm_b32(0xAABBCCDD, 0x11223344, 0x07060302) == 0xAABB1122      # (hi1 << 16) | hi0
    assert "rint" not in split and "0x7fff" not in split                      # truncation, no rounding
    mfma = device_fn("x6_mfma")
    calls = re.findall(r"__builtin_amdgcn_mfma_f32_16x16x32_bf16\(a([hml]), b([hml]), c, 0, 0, 0\)", mfma)
    assert tuple(calls) == X.PAIRS, calls
    assert mfma.count("__builtin_amdgcn_mfma") == 6 and "f4 c = acc;" in mfma
    # the slab-sum form (X.chain32's default): from zero, one add into the accumulator
    assert "if constexpr (SLAB) c = f4{0.f, 0.f, 0.f, 0.f};" in mfma and "if constexpr (SLAB) acc += c;" in mfma
    src = KERNELS.read_text()
    # every x6 kernel goes through the one split and the one chain: the forward kernel in the
    # slab-sum form, the dh and weight-gradient kernels chained through the accumulator
    assert len(re.findall(r"\bx6_split4\(", src)) == 2
    assert len(re.findall(r"\bx6_mfma<true>\(", src)) == 1 and len(re.findall(r"\bx6_mfma\(", src)) == 3
    fwd = src[src.index("void k_fwd_x6(GemmBatch batch)"):]
    assert "x6_mfma<true>(" in fwd[:fwd.index("\n}\n")]
