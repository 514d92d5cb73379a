"""The prioritized-feedback model (tests/per_feedback_model.py) on the CPU: with every weight 1
it IS OracleSAC, bit for bit in fp32; the weights scale the critic losses and gradients and
leave the actor alone; the closed loop's write-back is oracle.per.update_priorities."""
import os

import numpy as np
import pytest
import torch

from oracle import per as P
from oracle.pyrandom import MT19937
from oracle.sac_step import NETS, OracleSAC, SacConfig, param_shapes

from per_feedback_model import FeedbackSAC, closed_loop_update, stored_priorities


@pytest.fixture(scope="module")
def small(golden_dir):
    z = np.load(os.path.join(golden_dir, "step_small.npz"))
    S, A, H, B, N = (int(x) for x in z["cfg"][:5])
    cfg = SacConfig(S, A, H)
    params = {n: {k: z[f"in.{n}.{k}"] for k in param_shapes(cfg)[n]} for n in NETS}
    rows = [z[f"rows.{k}"] for k in ("s", "a", "r", "s2", "d")]
    return z, cfg, params, rows, B, N


def test_unit_weights_equal_oracle_bitwise_fp32(small):
    """Two updates on tests/golden/step_small.npz in fp32: losses, every parameter, every Adam
    moment and every gradient equal OracleSAC.step's, bit for bit, with w = 1 given explicitly
    and with no weights given."""
    z, cfg, params, rows, B, N = small
    for explicit in (True, False):
        ref = OracleSAC(cfg, params, dtype=torch.float32)
        mod = FeedbackSAC(cfg, params, dtype=torch.float32)
        for t in range(2):
            idx = z[f"step{t}.idx"]
            batch = [x[idx] for x in rows]
            e1, e2 = z[f"step{t}.eps1"], z[f"step{t}.eps2"]
            want = ref.step(*batch, e1, e2)
            got = (mod.step_weighted(*batch, e1, e2, np.ones(B, np.float32)) if explicit
                   else mod.step(*batch, e1, e2))
            for k in ("q1_loss", "q2_loss", "policy_loss"):
                assert got[k] == want[k], (explicit, t, k)
            assert np.array_equal([got["q1_loss"], got["q2_loss"], got["policy_loss"]], z[f"step{t}.losses"])
            sr, sm = ref.state(), mod.state()
            assert sr.keys() == sm.keys()
            for k in sr:
                assert np.array_equal(sr[k], sm[k]), (explicit, t, k)
            gr, gm = ref.grads_flat(), mod.grads_flat()
            for k in gr:
                assert np.array_equal(gr[k], gm[k]), (explicit, t, k)
            assert got["q1_loss_unweighted"] == got["q1_loss"]
            assert got["td"].shape == (B,) and got["td"].dtype == np.float32


def test_weights_scale_the_critic_and_leave_the_actor(small):
    """fp64: a constant weight c scales both q losses and every critic gradient by c and
    leaves td alone; on a single row loss_i = w e_i^2 and td = 0.5 (|e_1| + |e_2|); row weights
    spread over two decades move the q losses by far more than 1e-2 and leave td alone."""
    z, cfg, params, rows, B, N = small
    idx = z["step0.idx"]
    batch = [x[idx] for x in rows]
    e1, e2 = z["step0.eps1"], z["step0.eps2"]
    one = FeedbackSAC(cfg, params, dtype=torch.float64)
    l1 = one.step(*batch, e1, e2)
    half = FeedbackSAC(cfg, params, dtype=torch.float64)
    lh = half.step_weighted(*batch, e1, e2, np.full(B, 0.5, np.float32))
    assert np.array_equal(l1["td"], lh["td"])
    for k in ("q1_loss", "q2_loss"):
        assert lh[k] == pytest.approx(0.5 * l1[k], rel=1e-14)
    g1, gh = one.grads_flat(), half.grads_flat()
    for k in g1:
        if k.startswith(("q1.", "q2.")):
            np.testing.assert_allclose(gh[k], 0.5 * g1[k], rtol=1e-12, atol=1e-300)
    # a single row: loss_i = w e_i^2 and td = (|e_1| + |e_2|) / 2
    row = [x[:1] for x in batch]
    m = FeedbackSAC(cfg, params, dtype=torch.float64)
    o = m.step_weighted(*row, e1[:1], e2[:1], np.array([0.25], np.float32))
    ea, eb = np.sqrt(o["q1_loss_unweighted"]), np.sqrt(o["q2_loss_unweighted"])
    assert o["td"][0] == pytest.approx(0.5 * (ea + eb), rel=1e-12)
    assert o["q1_loss"] == pytest.approx(0.25 * o["q1_loss_unweighted"], rel=1e-14)
    # row weights over two decades
    rng = np.random.default_rng(5)
    w = (10.0 ** rng.uniform(-2, 0, B)).astype(np.float32)
    mw = FeedbackSAC(cfg, params, dtype=torch.float64)
    lw = mw.step_weighted(*batch, e1, e2, w)
    assert np.array_equal(lw["td"], l1["td"])
    assert lw["q1_loss"] != pytest.approx(l1["q1_loss"], rel=1e-2)


def test_closed_loop_composes_with_oracle_per(small):
    """closed_loop_update = oracle.per sampling + the weighted step + update_priorities:
    duplicates resolve to the last one, unsampled rows keep their priority, the stored value
    is float32(float64(td) + 1e-6), the numpy-MT stream advances by the draw."""
    z, cfg, params, rows, B, N = small
    n = B          # (sample() draws min(B, len): as many rows as draws, with replacement)
    sub = [x[:n] for x in rows]
    rng = np.random.default_rng(11)
    prios = (10.0 ** rng.uniform(-1, 1, n)).astype(np.float32)
    np.random.seed(4)
    st = np.random.get_state()
    mt = MT19937.from_npstate(st)
    model = FeedbackSAC(cfg, params, dtype=torch.float32)
    out, idx, w, after = closed_loop_update(model, prios, sub, mt, 1, B, z["step0.eps1"], z["step0.eps2"])
    assert len(idx) == B and len(np.unique(idx)) < B
    ridx, rw = P.sample_from_probs(P.probs_from(prios, n), B, MT19937.from_npstate(st), P.beta_at(1))
    assert np.array_equal(idx, ridx) and np.array_equal(w, rw)
    assert w.max() == 1.0 and w.min() < 0.5
    val = stored_priorities(out["td"])
    last = {int(i): v for i, v in zip(idx, val)}
    for i in range(n):
        assert after[i] == (last[i] if i in last else prios[i]), i
    assert np.array_equal(after, P.update_priorities(prios, idx, out["td"]))
    ref = MT19937.from_npstate(st)
    for _ in range(B):
        ref.random_sample()
    assert mt.random_sample() == ref.random_sample()
