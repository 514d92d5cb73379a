"""Numpy model of the bf16 batch-4096-class GEMM levels, level by level.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

compute_dtype bf16 at the batch-4096 class runs its forward levels on k_fwd16 / k_fwd16p, its dh
levels on k_axk16 and its weight gradients on k_dw_part16 + k_dw_fin (kernels.hip).  Every one
of them rounds its fp32 operands to bf16 once at staging (pack_bf16x4: round to nearest even),
or reads them as stored bf16 (act16 updates, the weight shadows), and sums the products in fp32
(v_mfma_f32_16x16x32_bf16).  A product of two bf16 values has 16 significant bits: it is exact
in fp32, so once a level's operands are known exactly the only freedom the kernel has is the
order of its fp32 sums.  ``dot16`` is that level with the fp32 accumulation rounding removed (a
float64 sum of the exact products); tests/test_bf16_model.py pins ``rne`` to torch and the
exact-product property, tests/test_gpu_bf16_levels.py holds every level of an update to it.

Shapes follow F.linear: x [M, K] rows, w [N, K].
"""
from __future__ import annotations

import numpy as np

CAP = 2.0 ** -17        # no bar above this: one product of K <= 4096 like ones is >= 2^-12 of the scale


def _bits(x: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def rne(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 -> fp32, round to nearest even on the bit pattern (f2bf / pack_bf16x4 in the
    kernels, torch.Tensor.to(torch.bfloat16)): finite values past the largest bf16 go to inf,
    subnormals round like any other pattern, NaN stays NaN (quiet, payload not modelled)."""
    u = _bits(x).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)).astype(np.uint32)
    nan = (u & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    r = np.where(nan, np.uint32(0x7FC00000) | (u.astype(np.uint32) & np.uint32(0x80000000)), r).astype(np.uint32)
    return r.view(np.float32).reshape(np.shape(x))


def trunc(x: np.ndarray) -> np.ndarray:
    """fp32 -> the bf16 below it in magnitude (bits & 0xffff0000): what a staging that drops the
    low half instead of rounding would feed the MFMA (the mutation tests use it)."""
    return (_bits(x) & np.uint32(0xFFFF0000)).view(np.float32).reshape(np.shape(x))


def widen(bits16: np.ndarray) -> np.ndarray:
    """stored bf16 bit patterns (uint16) -> fp32 (bits << 16), exact."""
    return (np.ascontiguousarray(bits16, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def is_bf16(x: np.ndarray) -> bool:
    """every element representable in bf16 (low 16 bits clear)."""
    return not np.any(_bits(x) & np.uint32(0xFFFF))


def dot16(x: np.ndarray, w: np.ndarray, rx=rne, rw=rne) -> np.ndarray:
    """float64 [M, N]: sum_k rx(x)[m, k] rw(w)[n, k], every product exact.  rx / rw: the staging
    rounding of each operand (rne in the kernels; the mutation tests pass trunc)."""
    return rx(x).astype(np.float64) @ rw(w).astype(np.float64).T


def abs_dot16(x: np.ndarray, w: np.ndarray) -> np.ndarray:
    """sum_k |rne(x)| |rne(w)| in float64, [M, N]: the scale of every elementwise bar."""
    return np.abs(rne(x).astype(np.float64)) @ np.abs(rne(w).astype(np.float64)).T


def bar(e_ref: float) -> float:
    """The level bar from the fp32 reference's own max error on the same operands: the
    project's 4x margin, capped so that a missing product never fits."""
    return min(4.0 * float(e_ref), CAP)


# ---------------------------------------------------------------------------
# the levels' forms: each returns (value float64, scale float64); the fp32 torch reference of
# the same rounded operands is built by the tests from `operands`


def forward_folded(x: np.ndarray, w: np.ndarray, b: np.ndarray):
    """Layer 0 (k_fwd16 / k_fwd16p on the gathered rows): x = [input | 1] against [W | b], the
    bias a K column like any other, so it is rounded.  Pre-activation, scale."""
    x1 = np.concatenate([x, np.ones((x.shape[0], 1), np.float32)], 1)
    wb = np.concatenate([w, b[:, None]], 1).astype(np.float32)
    return dot16(x1, wb), abs_dot16(x1, wb)


def forward_hidden(x: np.ndarray, w: np.ndarray, b: np.ndarray):
    """Layers >= 1: rounded operands, the bias added in fp32 in the epilogue (FwdEpi::store).
    Pre-activation, scale (sum |x||w| + |b|)."""
    b64 = b.astype(np.float64)
    return dot16(x, w) + b64, abs_dot16(x, w) + np.abs(b64)


def stored_bounds(z: np.ndarray, delta: np.ndarray):
    """bf16-stored forward outputs: [rne(relu(z - delta)), rne(relu(z + delta))].  The kernel's
    fp32 value v lies within delta of z; fp64 -> fp32 rounding, ReLU and rne are monotone and
    v is an fp32 already, so rne(relu(v)) lies between the two: exact equality except where z
    sits within delta of a rounding boundary or of zero."""
    lo = rne(np.maximum((z - delta).astype(np.float32), 0))
    hi = rne(np.maximum((z + delta).astype(np.float32), 0))
    return lo, hi


def dh_plain(dy: np.ndarray, w: np.ndarray, h_below: np.ndarray):
    """k_axk16<false>: dh[l-1] = (rne(dh[l]) . rne(W[l])) * [h[l-1] > 0].  dy [M, K], w = W[l]
    as stored ([out = K, in = N]), h_below [M, N] the masked layer's activations."""
    m = (h_below > 0).astype(np.float64)
    wt = np.ascontiguousarray(w.T)
    return dot16(dy, wt) * m, abs_dot16(dy, wt) * m


def head_rows(h: np.ndarray, w_head: np.ndarray) -> np.ndarray:
    """The coefficient-free rows of the row-prologue levels (dh_u4): u = h > 0 ? w_head : 0,
    exact fp32 values."""
    return np.where(h > 0, w_head.astype(np.float32)[None, :], np.float32(0)).astype(np.float32)


def dh_rows(h: np.ndarray, w_head: np.ndarray, w: np.ndarray, coef: np.ndarray, h_below: np.ndarray):
    """k_axk16<true> (L5 / L9): dh[L-1][b][n] = coef[b] * sum_k [h[L][b][k] > 0] rne(w_head[k])
    rne(W[L][k][n]) * [h[L-1][b][n] > 0]; the coefficient multiplies the fp32 sum once in the
    epilogue (dh_epilogue)."""
    u = head_rows(h, w_head)
    z, s = dh_plain(u, w, h_below)
    c = coef.astype(np.float64)[:, None]
    return c * z, np.abs(c) * s


def actor_coef(qa1: np.ndarray, qa2: np.ndarray, batch: int):
    """rows_coef, actor kind: coef_i = -[q_i is the min] / B (ties 1/2 : 1/2), in fp32."""
    g = np.float32(-1.0) / np.float32(batch)
    w1 = np.where(qa1 < qa2, np.float32(1), np.where(qa1 == qa2, np.float32(0.5), np.float32(0))).astype(np.float32)
    return g * w1, g * (np.float32(1) - w1)


def head_sums(parts: np.ndarray) -> np.ndarray:
    """rows_finish: a row's head value = its dot partials summed in block order, fp32.
    parts [..., nparts] -> [...]."""
    acc = parts[..., 0].astype(np.float32).copy()
    for i in range(1, parts.shape[-1]):
        acc = acc + parts[..., i].astype(np.float32)
    return acc


def scaled_rows(u: np.ndarray, f: np.ndarray) -> np.ndarray:
    """The K-scaled dY of layer L's weight gradient as k_dw_part16's gload forms it: the fp32
    product u[b][n] * f[b] (rounded to bf16 afterwards, at staging)."""
    return (u.astype(np.float32) * f.astype(np.float32)[:, None]).astype(np.float32)


def dw(dy: np.ndarray, x: np.ndarray):
    """k_dw_part16 + k_dw_fin: dW[n][k] = sum_b rne(dY[b][n]) rne(X[b][k]).  dy [B, N], x [B, K]
    -> value, scale [N, K]."""
    dyt, xt = np.ascontiguousarray(dy.T), np.ascontiguousarray(x.T)
    return dot16(dyt, xt), abs_dot16(dyt, xt)


def dw_tiles(m: int, n: int) -> int:
    """128 x 128 output tiles of one weight-gradient tensor [m][n] (kDBM, kDBN)."""
    return -(-m // 128) * -(-n // 128)


def dw_splits(level_tiles: int) -> int:
    """dw_split_plan: the K splits of a split-K weight-gradient level from the tiles of all its
    tensors (as many as fit one pass over 512 workgroup slots, at most 16)."""
    return max(1, min(16, 512 // level_tiles))


def rowsum_order32(dy: np.ndarray, ns: int) -> np.ndarray:
    """The bias-gradient row sums of k_dw_part16 + k_dw_fin in the kernels' own order of fp32
    adds (plain adds, contraction off, so this is the kernels' arithmetic itself):
      split sp of ns takes the batch rows [sp kc, min(B, sp kc + kc)), kc = ceil(B / ns) rounded
        up to whole 64-row slabs (dw_tile; a split may be empty);
      staging thread row kr0 < 16 adds, slab after slab, its rows kr0, kr0 + 16, kr0 + 32,
        kr0 + 48 of the slab to a running sum that starts at 0 (rows past the range count 0);
      the 16 sums are added in order kr0 = 0 .. 15 (dw_store_rowsum);
      k_dw_fin adds the ns partials in split order.
    dy [B, N] fp32 (unrounded, the K-scale already applied) -> fp32 [N]."""
    dy = np.ascontiguousarray(dy, np.float32)
    B, N = dy.shape
    kc = -(-(-(-B // ns)) // 64) * 64
    total = None
    for sp in range(ns):
        rows = dy[min(B, sp * kc):min(B, sp * kc + kc)]
        nslab = -(-len(rows) // 64)
        pad = np.zeros((nslab * 64, N), np.float32)
        pad[:len(rows)] = rows
        steps = pad.reshape(nslab * 4, 16, N)          # k = 64 slab + 16 i + kr0
        acc = np.zeros((16, N), np.float32)
        for st in steps:
            acc = acc + st
        v = acc[0]
        for g in range(1, 16):
            v = v + acc[g]
        total = v if total is None else total + v
    return total


def bias_grad(dy: np.ndarray, rounded: bool):
    """Bias gradients: fp32 sums of the UNROUNDED dY for layers >= 1 and the heads (the row-sum
    column of k_dw_part16), the rounded bias column of dW for layer 0 (dY against the constant-1
    column).  dy [B, N] -> value, scale [N]."""
    d = (rne(dy) if rounded else np.ascontiguousarray(dy, np.float32)).astype(np.float64)
    return d.sum(0), np.abs(d).sum(0)
