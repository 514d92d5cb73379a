"""The prioritized sampler's cdf on the GPU, pinned bit for bit with boundary draws.

tests/test_gpu_per.py draws random uniforms; those do not see a normaliser that is one float32
ulp off (tests/test_per_cdf_model.py measures it).  Here the uniforms are placed ON the cdf's
boundaries (tests/per_cdf_model.py: ``u = cdf[i]`` and ``u = nextafter(cdf[i], 0)``) and fed
through ``Context.per_sample(k, u=...)``, 4096 at a time: a wrong summation order at a ragged
chunk, a wrong leaf split, a wrong chunk-sum order, a wrong scan offset or a wrong top-table
stride changes the answer of about half of them, and ``idx`` must equal numpy's own
``searchsorted`` for EVERY probe.

That needs probabilities the host knows exactly, so ``prio ** alpha`` must be exact:

* ``powf(x, 1) == x`` does NOT hold on the device.  Measured on the MI355X over 2^20 values
  uniform(0.5, 1) * 2^[-3, 3]: 4.9 % come back one ulp off (three in four of those low).  With
  such priorities fills 1, 7, 8 and 9 passed by having few rows; 127, 128 and 257 each had one
  or two rows one ulp low, and with them ~100 % of their boundaries moved.  numpy's
  ``x ** 1.0`` is x.  DESIGN section 26.
* ``per_alpha = 0``: every probability is 1/n (powf(x, 0) is 1, measured for all 2^20).  This
  pins the scan, the block offsets, the top-table stride and the search at every fill; the
  sum's order is NOT pinned by it (n ones add up to n in any order).
* ``per_alpha = 1`` with priorities 2^k, -33 <= k <= 15: measured, powf(2^k, 1) is 2^k for
  every k in that range (not for every k: 41 of the 254 normal powers of two come back one ulp
  low, the nearest at k = -34 and k = 16).  Over 17 to 24 binades the float32 sum of such
  priorities still depends on its order (test_per_cdf_model.py asserts it).  These cases pin the
  pairwise tree, the ragged chunk and the chunk order, under that measured property of powf.
  The one priority outside the range, 2^100 in the subnormal case, was measured exact too.

Fills -> the branch of csrc/per.hip they reach (F1..F4: the fused kernels):
  1, 7                  pw_leaf's n < 8 loop alone
  8, 9, 127, 128        one leaf: 8 accumulators, tail n % 8 of 0, 1, 7, 0
  129, 136, 255, 257    the ragged chunk's leaf enumeration and post-order combine (2..4 leaves)
  1023..1025            F2's 1024-row scan block: last row, exact end, one row into block 2
  4095..4097            a thread's four rows in F2 straddling the fill; 4 and 5 scan blocks
  8191                  the ragged path at its largest
  8192, 16384           exactly full chunks (the LDS tree) followed by nothing
  8193, 8195, 8199      a full chunk, then the n < 8 leaf as the last chunk's whole sum
  8200, 16385, 16513    a full chunk (two), then one leaf of 8 / of 1 / two leaves (129)
  262 145               F3's second 256-wide pass over the block totals (257 blocks)
  524 294               F2's second 64-wide readlane pass over the chunk sums (65 chunks)
  2 102 152             the top table's stride doubles to 2048 (2053 scan blocks)
  cap 24 676, len 8193  fill far below the capacity, NaN (then 3e38) past the fill
  "fallback" cases      a probability below 2^-29: F2b's sequential float64 cumsum
  capacity 16 778 240   the unfused nine-kernel sequence (k_per_pow .. k_per_wnorm)

Asserted per call: idx == want exactly; the MT19937 stream untouched by a ``u=`` call; the
frame advanced by one; weights finite, in (0, 1], max exactly 1.0, and within the 4 ulp of
tests/test_gpu_per.py of the float64 (len p[idx])^-beta / max at that call's frame.
"""
import time

import numpy as np
import pytest

from oracle import per as P
from per_cdf_model import (SUM_CASES, default_prio, model, positions_for, pow2_prio, probes, takes_fallback,
                           top_stride, weights64)

pytestmark = pytest.mark.gpu

BATCH = 4096
UNFUSED_CAP = 16_777_216 + 1024          # > kPerFusedMaxRows: the unfused sequence


def _ctx(cap, alpha=1.0, **kw):
    from sacmi import Config, Context
    return Context(Config(1, 1, 4, max_batch=BATCH, capacity=cap, replay="per", per_alpha=alpha,
                          **kw), 0)


def _push(ctx, n):
    ctx.push(np.arange(n, dtype=np.float32).reshape(n, 1), np.zeros((n, 1), np.float32),
             np.zeros(n, np.float32), np.zeros((n, 1), np.float32), np.zeros(n, np.uint8))


def _check_weights(w, p, n, idx, beta):
    assert np.all(np.isfinite(w)) and np.all((w > 0) & (w <= 1)) and w.max() == np.float32(1.0)
    ref = weights64(p, n, idx, beta)
    ulp = np.spacing(np.maximum(np.abs(ref.astype(np.float32)), np.float32(1e-30)))
    err = np.abs(w.astype(np.float64) - ref) / ulp
    assert np.all(err <= 4), (float(err.max()), int(idx[err.argmax()]))


def _feed(ctx, n, p, u, want, beta_start=0.4, beta_frames=100000):
    """All of u through per_sample(u=...), at most min(4096, n) per call."""
    from sacmi import _lib as L
    assert len(ctx) == n
    key0, pos0 = ctx.get_mt(1)
    chunk = min(BATCH, n)
    for lo in range(0, u.size, chunk):
        uc, wc = u[lo:lo + chunk], want[lo:lo + chunk]
        frame = int(ctx.get_scalar(L.S_PER_FRAME))
        idx, w = ctx.per_sample(uc.size, u=uc)
        assert idx.shape == wc.shape
        wrong = np.flatnonzero(idx != wc)
        assert wrong.size == 0, (
            f"fill {n}: {wrong.size} of {wc.size} probes wrong; first: probe {lo + wrong[0]} "
            f"u={uc[wrong[0]]!r} got {idx[wrong[0]]} want {wc[wrong[0]]}")
        assert int(ctx.get_scalar(L.S_PER_FRAME)) == frame + 1
        _check_weights(w, p, n, idx, P.beta_at(frame, beta_start, beta_frames))
    key1, pos1 = ctx.get_mt(1)
    assert pos1 == pos0 and np.array_equal(key1, key0)
    return u.size


def _probe(ctx, prio, n, alpha=1.0, positions=None, fallback=False, extra_u=()):
    """Set the priorities, build the model and the probes of fill n, feed them."""
    ctx.per_set_priorities(prio)
    p, cdf = model(prio, n, alpha)
    # every probability >= 2^-29 (the exact fixed-point path), or the case is a fallback case
    assert takes_fallback(p) == fallback
    u, want = probes(cdf, positions_for(n) if positions is None else positions)
    if len(extra_u):
        e = np.asarray(extra_u, np.float64)
        u = np.concatenate([u, e])
        want = np.concatenate([want, cdf.searchsorted(e, side="right")])
    return _feed(ctx, n, p, u, want)


LEAF_AND_TREE = [1, 7, 8, 9, 127, 128, 129, 136, 255, 257]
SCAN_BLOCK = [1023, 1024, 1025, 4095, 4096, 4097]
CHUNK_EDGES = [8191, 8192, 8193, 8195, 8199, 8200, 16384, 16385, 2 * 8192 + 129]
LARGE = [262_145, 524_289 + 5, 2_097_153 + 4999]
TO_24705 = LEAF_AND_TREE + SCAN_BLOCK + CHUNK_EDGES + [24705]


@pytest.mark.parametrize("n", LEAF_AND_TREE + SCAN_BLOCK + CHUNK_EDGES + LARGE)
def test_cdf_boundaries_equal_probabilities(n):
    """cap == len, alpha = 0: p = 1/n.  Scan, block offsets, top-table stride and search at
    every fill of the table (not the sum's order)."""
    if n == LARGE[2]:
        assert top_stride(n) == 2048
    ctx = _ctx(n, 0.0)
    _push(ctx, n)
    _probe(ctx, default_prio(n, n), n, alpha=0.0)
    ctx.close()


@pytest.mark.parametrize("n", TO_24705 + LARGE)
def test_cdf_boundaries_exact_path(n):
    """alpha = 1, priorities 2^k: 17 binades up to 24 705 rows (the sum depends on its order
    from 4095 rows on), 7 binades above; every probability >= 2^-29: the fixed-point prefix."""
    ctx = _ctx(n)
    _push(ctx, n)
    _probe(ctx, pow2_prio(n, 300 + n, *((-16, 0) if n <= 24705 else (-3, 3))), n)
    ctx.close()


@pytest.mark.parametrize("n", TO_24705, ids=[f"{n}{'-fallback' if n >= 1023 else ''}" for n in TO_24705])
def test_cdf_boundaries_wide_exponents(n):
    """alpha = 1, priorities 2^k over 24 binades: the sum depends on its order from 129 rows
    on.  From 1023 rows on the smallest probability is below 2^-29, so those are fallback cases
    (the normaliser still divides every probability, and numpy's sequential float64 cumsum is
    the model's own)."""
    ctx = _ctx(n)
    _push(ctx, n)
    _probe(ctx, pow2_prio(n, 300 + n, -23, 0), n, fallback=n >= 1023)
    ctx.close()


@pytest.mark.parametrize("n", sorted(SUM_CASES))
def test_cdf_boundaries_sum_order(n):
    """alpha = 1, priorities 2^k over 49 binades (fallback cases all), the seeds chosen so that
    each emulated wrong sum of per_cdf_model.SUM_MUTANTS that applies at the fill — the leaf's
    pairwise combine, the split's multiple of 8, the tail's place, the chunk order, the leaf
    size — gives another total on at least one of them."""
    ctx = _ctx(n)
    _push(ctx, n)
    for seed in SUM_CASES[n][0]:
        _probe(ctx, pow2_prio(n, seed, -33, 15), n, fallback=True)
    ctx.close()


def test_fill_below_capacity_garbage_past_the_fill():
    """The fused kernels' grids cover the capacity and read the fill on the device: rows past
    the fill must not be touched.  NaN there for the first probe, 3e38 after pushing on (set
    after the push: a push takes the max over the whole array)."""
    cap = 3 * 8192 + 100
    ctx = _ctx(cap)
    for n, junk, seed in ((8193, np.nan, 1), (2 * 8192 + 5, 3e38, 2)):
        _push(ctx, n - len(ctx))
        prio = pow2_prio(cap, seed, -16, 0)
        prio[n:] = np.float32(junk)
        _probe(ctx, prio, n)
    ctx.close()


def test_zero_probability_rows():
    """Leading, interior and trailing zero-probability rows make ties in the cdf: 'right' steps
    over each run.  Every position is probed, and both ends of [0, 1)."""
    n = 20000
    prio = pow2_prio(n, 9, -16, 0)
    prio[:5] = 0
    prio[100:140] = 0
    prio[-9:] = 0
    ctx = _ctx(n)
    _push(ctx, n)
    _probe(ctx, prio, n, positions=np.arange(n), extra_u=(0.0, np.nextafter(1.0, 0.0)))
    ctx.close()


def test_fallback_every_position():
    """Every 7th priority 2^-30 of its size (2^-33 .. 2^-27): probabilities below 2^-29, so the
    sequential float64 cumsum (F2b) makes the cdf."""
    n = 3000
    prio = pow2_prio(n, 3000, -3, 3)
    prio[::7] *= np.float32(2.0 ** -30)
    ctx = _ctx(n)
    _push(ctx, n)
    _probe(ctx, prio, n, positions=np.arange(n), fallback=True)
    ctx.close()


def test_subnormal_probabilities():
    """2999 priorities of 2^-33 and one of 2^100: probabilities of 2^-133, subnormal in
    float32.  numpy keeps them; a kernel that flushed them to zero would collapse 2999
    boundaries."""
    n = 3000
    prio = np.full(n, 2.0 ** -33, np.float32)
    prio[-1] = np.float32(2.0 ** 100)
    p, cdf = model(prio, n, 1.0)
    assert np.all((p[:-1] > 0) & (p[:-1] < np.finfo(np.float32).tiny)) and np.unique(cdf).size == n
    ctx = _ctx(n)
    _push(ctx, n)
    _probe(ctx, prio, n, positions=np.arange(n), fallback=True)
    ctx.close()


def test_batch_larger_than_fill():
    """replay_buffer.py:50: k = min(batch, len)."""
    from sacmi import _lib as L
    n = 5
    prio = np.array([4, 0.5, 1, 0.125, 2], np.float32)
    ctx = _ctx(n)
    _push(ctx, n)
    ctx.per_set_priorities(prio)
    p, cdf = model(prio, n, 1.0)
    u = cdf - np.array([0, 1e-3, 0, 1e-3, 1e-3])       # on and inside the boundaries, all < 1
    idx, w = ctx.per_sample(64, u=u)
    assert idx.shape == (5,) and w.shape == (5,)
    assert np.array_equal(idx, cdf.searchsorted(u, side="right"))
    _check_weights(w, p, n, idx, P.beta_at(int(ctx.get_scalar(L.S_PER_FRAME)) - 1))
    ctx.close()


def test_beta_schedule():
    """beta = min(1, beta_start + frame (1 - beta_start) / beta_frames) at that call's frame
    (replay_buffer.py:54), away from the defaults; at beta clamped to 1 rows of equal
    probability get exactly equal weights."""
    from sacmi import _lib as L
    n = 3000
    prio = pow2_prio(n, 31, -3, 3)
    p, cdf = model(prio, n, 1.0)
    u, want = probes(cdf, np.arange(n))
    u, want = u[:n], want[:n]
    for start, frames, at in ((0.4, 1000, (0, 999, 1000, 5000)), (1.0, 1000, (0,))):
        ctx = _ctx(n, per_beta_start=start, per_beta_frames=frames)
        _push(ctx, n)
        ctx.per_set_priorities(prio)
        for frame in at:
            ctx.set_scalar(L.S_PER_FRAME, frame)
            beta = P.beta_at(frame, start, frames)
            assert (beta == 1.0) == (frame >= 1000 or start == 1.0)
            idx, w = ctx.per_sample(u.size, u=u)
            assert np.array_equal(idx, want)
            assert int(ctx.get_scalar(L.S_PER_FRAME)) == frame + 1
            _check_weights(w, p, n, idx, beta)
            if beta == 1.0:
                for v in np.unique(p):
                    assert np.unique(w[p[idx] == v]).size == 1
        ctx.close()


# --------------------------------------------------------------------------------------------
# The unfused sequence: capacity > kPerFusedMaxRows (16 777 216).  One context lifetime per
# test, the fills walked upward inside it.
UNFUSED_FILLS = [7, 129, 8193, 16385, 70_000]


def _big_ctx(alpha):
    t0 = time.perf_counter()
    ctx = _ctx(UNFUSED_CAP, alpha)
    print(f"unfused context (capacity {UNFUSED_CAP}) created in {time.perf_counter() - t0:.2f} s")
    return ctx


def test_unfused_cdf_boundaries():
    """k_per_pow .. k_per_wnorm under the probe assertions of the fused path (alpha = 1,
    priorities 2^k: 16 binades, every probability >= 2^-29 up to 70 000 rows; then 24 binades,
    the fallback from 8193 rows on)."""
    ctx = _big_ctx(1.0)
    for n in UNFUSED_FILLS:
        _push(ctx, n - len(ctx))
        _probe(ctx, pow2_prio(n, 300 + n, -15, 0), n)
        _probe(ctx, pow2_prio(n, 300 + n, -23, 0), n, fallback=n >= 1023)
        for seed in SUM_CASES.get(n, ((), ""))[0]:
            _probe(ctx, pow2_prio(n, seed, -33, 15), n, fallback=True)
    ctx.close()


def test_unfused_equals_fused_at_default_alpha():
    """alpha = 0.6: both sequences run the device's powf, so on the same priorities and the
    same uniforms their indices and weights are equal bit for bit; so is one MT19937-driven
    draw, and the stream's state after it."""
    from sacmi import _lib as L
    big, small = _big_ctx(0.6), _ctx(UNFUSED_FILLS[-1], 0.6)
    for n in UNFUSED_FILLS:
        prio = default_prio(n, 1000 + n)
        _, cdf = model(prio, n, 0.6)                     # only to place the uniforms
        u, _ = probes(cdf, positions_for(n))
        chunk = min(BATCH, n)
        out = []
        for ctx in (big, small):
            _push(ctx, n - len(ctx))
            ctx.per_set_priorities(prio)
            ctx.set_scalar(L.S_PER_FRAME, 7)
            key0, pos0 = ctx.get_mt(1)
            got = [ctx.per_sample(u[lo:lo + chunk].size, u=u[lo:lo + chunk])
                   for lo in range(0, u.size, chunk)]
            key1, pos1 = ctx.get_mt(1)
            assert pos1 == pos0 and np.array_equal(key1, key0)
            assert int(ctx.get_scalar(L.S_PER_FRAME)) == 7 + len(got)
            out.append(got)
        for (bi, bw), (si, sw) in zip(*out):
            assert np.array_equal(bi, si), n
            assert np.array_equal(bw.view(np.uint32), sw.view(np.uint32)), n
            assert bw.max() == np.float32(1.0) and np.all((bw > 0) & (bw <= 1))
    # one draw from the numpy stream, no u
    np.random.seed(12)
    st = np.random.get_state()
    out = []
    for ctx in (big, small):
        ctx.set_scalar(L.S_PER_FRAME, 3)
        ctx.set_mt(1, st[1], st[2])
        idx, w = ctx.per_sample(BATCH)
        out.append((idx, w, ctx.get_mt(1), int(ctx.get_scalar(L.S_PER_FRAME))))
    (bi, bw, (bk, bp), bf), (si, sw, (sk, sp), sf) = out
    assert np.array_equal(bi, si) and np.array_equal(bw.view(np.uint32), sw.view(np.uint32))
    assert bp == sp and np.array_equal(bk, sk) and not np.array_equal(bk, st[1]) and bf == sf == 4
    big.close()
    small.close()
