"""Bit-faithful numpy model of the x6 kernels' operand split and six-product dot.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

The batch-4096-class fp32 GEMM kernels (k_fwd_x6, k_axk_x6, k_dw_part_x6 in kernels.hip)
cut every fp32 operand into three bf16 parts (x6_split4) and sum six of the nine cross
products in an fp32 accumulator (x6_mfma).  ``split`` repeats x6_split4 operation for
operation; ``dot6`` sums the same six products in float64.  A product of two 8-bit parts is
exact, so ``dot6`` is the kernels' result with the fp32 accumulation rounding removed and the
truncation bias (the three dropped products) left in.  tests/test_x6_model.py ties both to
the kernel source and pins the split's domain and the bias bound.
"""
from __future__ import annotations

import numpy as np

# the six kept products, (A part, B part), in x6_mfma's accumulation order (small terms first)
PAIRS = (("l", "h"), ("h", "l"), ("m", "m"), ("m", "h"), ("h", "m"), ("h", "h"))
# the split is exact (h + m + l == x) for x == 0 and |x| >= 2^-110: below that the remainders
# go subnormal with significant bits under 2^-133, which a bf16 cannot hold
EXACT_MIN = 2.0 ** -110
# |dropped products| / |a b| per product (ml + lm + ll with |m| < 2^-7 |x|, |l| < 2^-15 |x|)
DROP_BOUND = 2.0 ** -21


def trunc_bf16(x: np.ndarray) -> np.ndarray:
    """fp32 -> the bf16 below it in magnitude (bits & 0xffff0000), as fp32."""
    x = np.ascontiguousarray(x, np.float32)
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def split_steps(x: np.ndarray):
    """x6_split4 on an fp32 array: (h, m, l, s) with s the second remainder before its
    truncation (l == s wherever the split is exact)."""
    x = np.ascontiguousarray(x, np.float32)
    h = trunc_bf16(x)
    r = x - h                       # fp32 subtraction, exact
    m = trunc_bf16(r)
    s = r - m                       # fp32 subtraction, exact
    return h, m, trunc_bf16(s), s


def split(x: np.ndarray):
    """(h, m, l): the three bf16 parts of fp32 x, each as fp32."""
    return split_steps(x)[:3]


def dot6(a: np.ndarray, b: np.ndarray, pairs=PAIRS) -> np.ndarray:
    """a [M, K] (rows), b [N, K] (weights, F.linear layout), fp32 -> float64 [M, N]: the sum
    over k of the kept part products."""
    pa = dict(zip("hml", (p.astype(np.float64) for p in split(a))))
    pb = dict(zip("hml", (p.astype(np.float64).T.copy() for p in split(b))))
    out = np.zeros((a.shape[0], b.shape[0]), np.float64)
    for i, j in pairs:
        out += pa[i] @ pb[j]
    return out


def chain32(a: np.ndarray, b: np.ndarray, slab_sum: bool = True, slab: int = 32) -> np.ndarray:
    """dot6 with an fp32 accumulator, ONE round-to-nearest rounding per MFMA (each 32-deep part
    product summed exactly): the least rounding the kernels' chain can have.  Not bit-faithful
    to the MFMA, whose internal summation is not documented (the measured errors match about
    four roundings per MFMA): a floor for the accumulation error of a form.
    slab_sum True: x6_mfma<true> (k_fwd_x6) — a slab's six products summed from zero, then
    added to the accumulator once.  False: x6_mfma<false> — every product chained through the
    running accumulator."""
    pa = dict(zip("hml", (p.astype(np.float64) for p in split(a))))
    pb = dict(zip("hml", (p.astype(np.float64) for p in split(b))))
    acc = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for k0 in range(0, a.shape[1], slab):
        c = np.zeros_like(acc) if slab_sum else acc
        for i, j in PAIRS:
            c = (c.astype(np.float64) + pa[i][:, k0:k0 + slab] @ pb[j][:, k0:k0 + slab].T).astype(np.float32)
        acc = acc + c if slab_sum else c
    return acc


def abs_dot(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """sum_k |a_k| |b_k| in float64, [M, N]: the scale of every elementwise x6 error bar."""
    return np.abs(np.asarray(a, np.float64)) @ np.abs(np.asarray(b, np.float64)).T


def dot64(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The exact-operand dot in float64, [M, N]."""
    return np.asarray(a, np.float64) @ np.asarray(b, np.float64).T


# ---------------------------------------------------------------------------
# input classes: fp32 values with their mantissa bits overwritten
MANTISSA = {"adv": 0x00FFFF,     # h = 1, m and l as large as truncation allows: the worst case
            "ones": 0x7FFFFF,    # every mantissa bit set
            "rand": None}        # mantissas left as drawn


def recast(x: np.ndarray, cls: str, positive: bool = False) -> np.ndarray:
    """x with every element's 23 mantissa bits replaced by the class pattern (exponent kept;
    sign kept, or forced positive).  Zeros stay zero."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).copy()
    mant = MANTISSA[cls]
    if mant is not None:
        u = np.where(x != 0, (u & np.uint32(0xFF800000)) | np.uint32(mant), u)
    if positive:
        u = u & np.uint32(0x7FFFFFFF)
    return u.astype(np.uint32).view(np.float32).reshape(x.shape)
