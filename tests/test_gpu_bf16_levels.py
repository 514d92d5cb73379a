"""The bf16 batch-4096-class GEMM kernels (k_fwd16 / k_fwd16p, k_axk16, k_dw_part16 + k_dw_fin)
elementwise, level by level, through the C ABI.

test_bf16_compute_vs_emulation compares a whole bf16 update with the emulation at 2e-2 per
tensor: any fp32-order-dependent value that is later rounded to bf16 may flip a rounding, and
the flips compound through the backward pass.  Here every level of ONE update is evaluated on
the host from its OWN operands as the GPU left them in HBM (sacmi_read_activation,
sacmi_read_backward, the host rows rounded as the gather rounds them), so nothing compounds:
bf16 x bf16 products are exact in fp32 and the only freedom a kernel has is the order of its
fp32 sums (oracle/bf16_model.py).

  error = |gpu - model| / (sum |x||w| + |b|), elementwise
  e_ref = the max error of torch's CPU fp32 product of the same rounded operands against fp64
  fp32-stored outputs (dh, dW, bias gradients; the forward levels of the fp32-activation case):
      error <= min(4 e_ref, 2^-17)
  bf16-stored outputs (the forward levels of act16 updates): with delta = bar * scale the stored
      value lies in [rne(relu(z - delta)), rne(relu(z + delta))] (bf16_model.stored_bounds): exact
      equality except within delta of a rounding boundary or of zero.  No element is skipped.
  the coefficient-free rows u of L5: bit for bit [h > 0] w_head.
  a masked-out dh element (scale 0) must be exactly zero.

Levels (tests/test_bf16_model.py shows that a dropped product, a dropped batch row or truncation
for rne in the model breaks these bars on >= 99 % of the outputs it touches):
  forward   layer 0 of passes 0 and 3 (L1: bias folded into K, so rounded) and layers >= 1 of all
            four passes (L2, L2b, L4, L4b, L8, L8b: bias added in fp32), x the GPU's own previous
            activations, W the tensor the pass reads (params, targets, post-Adam critics)
  dh        the row-prologue levels L5 / L9 (coefficients: dq read back; the actor's from the
            head dot partials as rows_coef forms them) and the plain levels L12, L5b, L9b, L11
  dW        every tensor of L6 and L13, bias gradients included, all B terms of each sampled row
Rows: of every row tile of the kernel under test (128 forward and dW, 64 dh) the first, the last
and 4 inner rows, all columns.  Each case asserts from the launch timeline which kernel ran
every level it checks, and prints it."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import bf16_model as M
from oracle.sac_step import NETS, SacConfig, init_params, param_shapes, synthetic_rows

pytestmark = pytest.mark.gpu

FWD = ({"k_fwd16"}, {"k_fwd16p"})
AXK = ({"k_axk16"},)
DW = (("k_dw_part16", "k_dw_fin"),)


def tile_rows(n, tile, seed, inner=4):
    """Row sample of an n-row operand: of every `tile`-row tile its first and last row plus
    `inner` others."""
    rng = np.random.default_rng(seed)
    out = []
    for r0 in range(0, n, tile):
        r1 = min(r0 + tile, n)
        mid = np.arange(r0 + 1, r1 - 1)
        out += sorted({r0, r1 - 1, *rng.choice(mid, min(inner, len(mid)), replace=False)})
    return np.array(out)


def t32(x):
    return torch.from_numpy(np.ascontiguousarray(M.rne(x)))


def ref_mm(x, w):
    """torch's CPU fp32 product of the rounded operands, x [R, K] against w [N, K]."""
    return (t32(x) @ t32(w).T).numpy()


class Table:
    def __init__(self, name):
        self.name, self.rows, self.over = name, [], []

    def fp32(self, label, K, got, z, scale, ref, order=None):
        """An fp32-stored output against its bar; scale == 0 (masked out) must be exactly 0.
        order: the host's fp32 emulation of the kernels' own order of sums, for the levels whose
        bar is 4 x ITS error (the row-sum bias gradients, see test_levels_match_model)."""
        live = scale > 0
        assert live.any(), label
        assert np.all(got[~live] == 0), (label, "nonzero where every term is masked out")
        s = np.where(live, scale, 1.0)
        e_ref = (np.abs(ref.astype(np.float64) - z) / s)[live].max()
        err = np.where(live, np.abs(got.astype(np.float64) - z) / s, 0)
        where = np.unravel_index(np.argmax(err), got.shape)
        if order is None:
            return self._row(label, K, err.max(), e_ref, where)
        e_ord = (np.abs(order.astype(np.float64) - z) / s)[live].max()
        same = int(np.sum(order.view(np.uint32) == np.ascontiguousarray(got).view(np.uint32)))
        self._row(label, K, err.max(), e_ref, where, e_bar=e_ord,
                  note=f"bar from the order emulation (its error {e_ord:.2e}; {same} of {got.size} outputs bit-equal to it)")

    def bf16(self, label, K, got, z, scale, ref):
        """A bf16-stored post-ReLU output against the monotone bounds; the error column is the
        distance outside them (0 = inside), on the level's scale."""
        e_ref = (np.abs(ref.astype(np.float64) - z) / scale).max()
        lo, hi = M.stored_bounds(z, M.bar(e_ref) * scale)
        out = np.maximum(np.maximum(lo.astype(np.float64) - got, got - hi.astype(np.float64)), 0) / scale
        exact = float(np.mean(lo == hi))
        self._row(label, K, out.max(), e_ref, np.unravel_index(np.argmax(out), got.shape), outside=True,
                  note=f"bounds pin {100 * exact:.2f} % of {got.size} outputs to one value")

    def _row(self, label, K, err, e_ref, where, outside=False, note="", e_bar=None):
        b = M.bar(e_ref if e_bar is None else e_bar)
        ok = err == 0 if outside else err <= b
        self.rows.append((label, K, err, e_ref, b, ok, note))
        if not ok:
            self.over.append((label, f"element {tuple(int(i) for i in where)}", err, b))

    def report(self):
        print(f"\n[bf16 levels] {self.name}: max |gpu - model| / (sum|x||w| + |b|)")
        for label, K, err, e_ref, b, ok, note in self.rows:
            print(f"  {label:34s} K {K:4d}  err {err:.2e}  e_ref {e_ref:.2e}  bar {b:.2e}  {'ok' if ok else 'OVER'}  {note}")
        fp = [r for r in self.rows if not r[6].startswith("bounds")]
        print(f"  [bf16 summary] {self.name}: fp32-stored max err {max(r[2] for r in fp):.2e}  "
              f"e_ref {min(r[3] for r in self.rows):.2e} .. {max(r[3] for r in self.rows):.2e}")


def kernels_by_site(ctx, B):
    ks, _ = ctx.profile_timeline(B, 1)
    by_site = {}
    for k in ks:
        by_site.setdefault(k["site"], []).append(k["kernel"])
    return by_site


@functools.lru_cache(maxsize=None)
def case_data(S, A, H, n_hidden, n_rows):
    cfg = SacConfig(S, A, H, n_hidden=n_hidden)
    return cfg, init_params(cfg, 71, bias_scale=0.02), synthetic_rows(cfg, n_rows, 72, state_scale=0.1)


def bf16_bits(x):
    assert M.is_bf16(x)
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def record_slices(path, act, params, dhp, hpa, dhc, dq, grads, ns6, rq, rd):
    """tests/golden/bf16_levels_gpu.npz: small slices of one forward, one dh and one weight-gradient
    level of the n_hidden 2 batch-4096 case with the outputs the MI355X gave, for
    tests/test_bf16_model.py test_recorded_gpu_outputs_go_red_under_a_broken_model (written when
    SACMI_RECORD_BF16_LEVELS names a file)."""
    r, c, n = rq[:8], slice(0, 32), np.array([0, 1, 127, 128])
    q1, pol = params["q1"], params["policy"]
    np.savez_compressed(
        path,
        fwd_x=bf16_bits(act[(0, 0)][0][r]), fwd_w=q1["fc2.weight"][c], fwd_b=q1["fc2.bias"][c],
        fwd_got=bf16_bits(act[(0, 1)][0][r][:, c]),
        dh_dy=dhp[1][rd[:8]], dh_w=pol["fc2.weight"][:, c], dh_below=bf16_bits(hpa[0][rd[:8]][:, c]),
        dh_got=dhp[0][rd[:8]][:, c],
        dw_dy=M.scaled_rows(dhc[1][:, 0], dq[0])[:, n], dw_x=bf16_bits(act[(0, 0)][0][:, :16]),
        dw_got=grads["q1"]["fc2.weight"][n][:, :16], dw_bias_got=grads["q1"]["fc2.bias"][n], dw_splits=np.int32(ns6))


def run_case(S, A, H, B, n_hidden, act16, want, record_to=None):
    """One bf16 update, every level read back and checked.  want: site -> the kernel tuples it may
    run on (checked once everything is read: the timeline replays whole updates); None where the
    timeline cannot be taken (it samples on the device: batch <= 4096) and the update is act16,
    whose levels launch_gemm runs on the batch-4096-class kernels or not at all (plan_gemm_level
    throws "bf16 activation operands on a level outside the batch-4096-class kernels")."""
    from sacmi import Config, Context, _lib as L
    cfg, params, rows = case_data(S, A, H, n_hidden, B + 1000)
    name = f"(S, A, H) = ({S}, {A}, {H}) B {B} n_hidden {n_hidden} {'act16' if act16 else 'fp32 activations'}"
    ctx = Context(Config(S, A, H, max_batch=B, capacity=len(rows[2]), n_hidden=n_hidden, compute_dtype="bf16"), 0)
    for n in NETS:
        ctx.set_net(n, params[n])
    ctx.set_scalar(L.S_KEEP_GRADS, 1)
    ctx.push(*rows)
    assert ctx.act16(B) == act16
    rng = np.random.default_rng(73)
    idx = rng.choice(len(rows[2]), B, replace=False)
    e1 = rng.standard_normal((B, A)).astype(np.float32)
    e2 = rng.standard_normal((B, A)).astype(np.float32)
    losses = ctx.step(B, idx=idx, eps1=e1, eps2=e2)
    assert np.all(np.isfinite(losses)), losses
    nh, Lh = n_hidden, n_hidden - 1
    shapes = param_shapes(cfg)
    act = {(p, l): ctx.read_activation(p, l, B) for p in range(4) for l in range(nh)}
    if act16:
        assert all(M.is_bf16(h) for h in act.values())
    dhc = [ctx.read_backward("dhc", B, l) for l in range(nh)]
    dha = [ctx.read_backward("dha", B, l) for l in range(Lh)]
    dhp = [ctx.read_backward("dhp", B, l) for l in range(nh)]
    dq, dq4, dhead = (ctx.read_backward(w, B) for w in ("dq", "dq4", "dhead"))
    dotp = ctx.read_backward("dotp", B)
    grads = {n: ctx.get_net(n, "grad", shapes[n]) for n in ("policy", "q1", "q2")}
    q_after = {n: ctx.get_net(n, "param", shapes[n]) for n in ("q1", "q2")}     # pass 2 and L9 read these
    assert want is not None or act16
    got_k = kernels_by_site(ctx, B) if want is not None else {}
    ctx.close()
    print(f"\n[bf16 kernels] {name}: " + (", ".join(f"{s} {'+'.join(got_k.get(s) or ['-'])}" for s in want) if want is not None
                                          else "act16: the batch-4096-class kernels by construction (no timeline past batch 4096)"))

    s, a, _, s2, _ = (v[idx] for v in rows)
    tab = Table(name)
    store = tab.bf16 if act16 else (lambda label, K, got, z, sc, ref:
                                    tab.fp32(label, K, got, np.maximum(z, 0), sc, np.maximum(ref, 0)))
    rq, rp = tile_rows(B, 128, 1), tile_rows(2 * B, 128, 2)
    rd = tile_rows(B, 64, 3)
    one = lambda x: np.concatenate([x, np.ones((len(x), 1), np.float32)], 1)
    fold = lambda w, b: np.concatenate([w, b[:, None]], 1)

    # ---- forward levels ----
    def fwd0(label, x, p, got):
        z, sc = M.forward_folded(x, p["fc1.weight"], p["fc1.bias"])
        store(label, x.shape[1] + 1, got, z, sc, ref_mm(one(x), fold(p["fc1.weight"], p["fc1.bias"])))

    def fwdh(label, x, p, l, got):
        w, b = p[f"fc{l + 1}.weight"], p[f"fc{l + 1}.bias"]
        z, sc = M.forward_hidden(x, w, b)
        store(label, x.shape[1], got, z, sc, ref_mm(x, w) + b)

    for i, n in enumerate(("q1", "q2")):
        fwd0(f"L1 pass 0 {n} layer 0", np.concatenate([s, a], 1)[rq], params[n], act[(0, 0)][i][rq])
        for p, wsrc, lv in ((0, params[n], "L2"), (1, params[f"{n}_target"], "L4"), (2, q_after[n], "L8")):
            for l in range(1, nh):
                fwdh(f"{lv}{'b' if l == 2 else ''} pass {p} {n} layer {l}", act[(p, l - 1)][i][rq], wsrc, l, act[(p, l)][i][rq])
    pol = params["policy"]
    fwd0("L1 pass 3 policy layer 0", np.concatenate([s2, s], 0)[rp], pol, act[(3, 0)][rp])
    for l in range(1, nh):
        fwdh(f"L2{'b' if l == 2 else ''} pass 3 policy layer {l}", act[(3, l - 1)][rp], pol, l, act[(3, l)][rp])

    # ---- dh levels ----
    def plain(label, dy, w, h_below, got):
        z, sc = M.dh_plain(dy, w, h_below)
        tab.fp32(label, dy.shape[1], got, z, sc, ref_mm(dy, w.T) * (h_below > 0))

    def rowsl(label, h, w_head, w, coef, h_below, got):
        z, sc = M.dh_rows(h, w_head, w, coef, h_below)
        ref = ref_mm(M.head_rows(h, w_head), w.T) * coef.astype(np.float32)[:, None] * (h_below > 0)
        tab.fp32(label, h.shape[1], got, z, sc, ref)

    qa = M.head_sums(dotp[4:6])
    ca = M.actor_coef(qa[0], qa[1], B)
    assert set(np.unique(ca[0] + ca[1])) == {np.float32(-1.0) / np.float32(B)}
    for i, n in enumerate(("q1", "q2")):
        wl, wh = f"fc{Lh + 1}.weight", f"fc{nh + 1}.weight"
        u = M.head_rows(act[(0, Lh)][i], params[n][wh][0])
        assert np.array_equal(dhc[Lh][:, i].view(np.uint32), u.view(np.uint32)), f"L5 {n}: the rows u are not [h > 0] w_head bit for bit"
        assert np.array_equal(dq4[i * B:(i + 1) * B, 0], dq[i]) and not dq4[:, 1:].any()
        rowsl(f"L5 {n} dh{Lh - 1}", act[(0, Lh)][i][rd], params[n][wh][0], params[n][wl], dq[i][rd],
              act[(0, Lh - 1)][i][rd], dhc[Lh - 1][rd, i])
        rowsl(f"L9 {n} dha{Lh - 1}", act[(2, Lh)][i][rd], q_after[n][wh][0], q_after[n][wl], ca[i][rd],
              act[(2, Lh - 1)][i][rd], dha[Lh - 1][rd, i])
        for l in range(Lh - 1, 0, -1):
            plain(f"L5b {n} dh{l - 1}", dhc[l][rd, i], params[n][f"fc{l + 1}.weight"], act[(0, l - 1)][i][rd], dhc[l - 1][rd, i])
            plain(f"L9b {n} dha{l - 1}", dha[l][rd, i], q_after[n][f"fc{l + 1}.weight"], act[(2, l - 1)][i][rd], dha[l - 1][rd, i])
    hpa = [act[(3, l)][B:] for l in range(nh)]          # the actor rows
    for l in range(Lh, 0, -1):
        plain(f"{'L12' if l == 1 else 'L11'} policy dhp{l - 1}", dhp[l][rd], pol[f"fc{l + 1}.weight"], hpa[l - 1][rd], dhp[l - 1][rd])

    # ---- weight gradients ----
    def dwl(label, dy, x, gw, gb, splits):
        """dy [B, N], x [B, K]; gw [N, K] / gb [N] the GPU's gradients.  splits 0: layer 0, the
        bias a K column of dW (rounded dY against the constant 1); else the level's split-K count
        (None: not on the split-K kernels): the bias is the fp32 row sum of the unrounded dY, held
        to the emulation of its order."""
        ns = tile_rows(dy.shape[1], 128, 4) if dy.shape[1] >= 128 else np.arange(dy.shape[1])
        z, sc = M.dw(dy[:, ns], x)
        tab.fp32(f"{label}.weight", len(dy), gw[ns], z, sc, ref_mm(dy[:, ns].T, x.T))
        zb, sb = M.bias_grad(dy, splits == 0)
        d32 = t32(dy) if splits == 0 else torch.from_numpy(np.ascontiguousarray(dy))
        tab.fp32(f"{label}.bias", len(dy), gb, zb, sb, d32.sum(0).numpy(),
                 order=M.rowsum_order32(dy, splits) if splits else None)

    # the split-K counts of L6 and L13, from the tiles of all their tensors (dw_split_plan); a
    # level that runs elsewhere (k_gemm) keeps the fp32 reference's bar for its row sums
    def splits(site, tiles):
        return M.dw_splits(tiles) if want is None or tuple(got_k.get(site) or []) == DW[0] else None
    ns6 = splits("gemm_L6_critic_dW_adam", 2 * (M.dw_tiles(H, S + A + 1) + Lh * M.dw_tiles(H, H) + M.dw_tiles(1, H)))
    ns13 = splits("gemm_L13_pi_dW_adam", M.dw_tiles(2 * A, H) + Lh * M.dw_tiles(H, H) + M.dw_tiles(H, S + 1))
    for i, n in enumerate(("q1", "q2")):
        g = grads[n]
        dwl(f"L6 {n}.fc1", dhc[0][:, i], np.concatenate([s, a], 1), g["fc1.weight"], g["fc1.bias"], 0)
        for l in range(1, Lh):
            dwl(f"L6 {n}.fc{l + 1}", dhc[l][:, i], act[(0, l - 1)][i], g[f"fc{l + 1}.weight"], g[f"fc{l + 1}.bias"], ns6)
        dwl(f"L6 {n}.fc{Lh + 1}", M.scaled_rows(dhc[Lh][:, i], dq[i]), act[(0, Lh - 1)][i], g[f"fc{Lh + 1}.weight"],
            g[f"fc{Lh + 1}.bias"], ns6)
        dwl(f"L6 {n}.fc{nh + 1}", dq[i][:, None], act[(0, Lh)][i], g[f"fc{nh + 1}.weight"], g[f"fc{nh + 1}.bias"], ns6)
    g = grads["policy"]
    dwl("L13 policy.heads", dhead, hpa[Lh], np.concatenate([g["mean.weight"], g["log_std.weight"]]),
        np.concatenate([g["mean.bias"], g["log_std.bias"]]), ns13)
    for l in range(Lh, 0, -1):
        dwl(f"L13 policy.fc{l + 1}", dhp[l], hpa[l - 1], g[f"fc{l + 1}.weight"], g[f"fc{l + 1}.bias"], ns13)
    dwl("L13 policy.fc1", dhp[0], s, g["fc1.weight"], g["fc1.bias"], 0)

    if record_to:
        record_slices(record_to, act, params, dhp, hpa, dhc, dq, grads, ns6, rq, rd)
    tab.report()
    wrong ={site: got_k.get(site) for site, allowed in (want or {}).items()
             if not any((set(got_k.get(site) or []) == k) if isinstance(k, set) else (tuple(got_k.get(site) or []) == k)
                        for k in allowed)}
    assert not wrong, (name, "levels on other kernels than expected", wrong)
    assert not tab.over, (name, tab.over)


def sites(n_hidden, fwd=FWD, axk=AXK, dw=DW, over=None):
    w = {"gemm_L1_fc1": fwd, "gemm_L2_fc2": fwd, "gemm_L4_tgt_fc2": fwd, "gemm_L8_act_fc2": fwd,
         "gemm_L5_critic_dh1": axk, "gemm_L9_act_dh1": axk, "gemm_L12_pi_dhp1": axk,
         "gemm_L6_critic_dW_adam": dw, "gemm_L13_pi_dW_adam": dw}
    if n_hidden == 3:
        w.update({"gemm_L2b_fc3": fwd, "gemm_L4b_tgt_fc3": fwd, "gemm_L8b_act_fc3": fwd,
                  "gemm_L5b_critic_dh": axk, "gemm_L9b_act_dh": axk, "gemm_L11_pi_dhp": axk})
    w.update(over or {})
    return w


@pytest.mark.parametrize("n_hidden", [2, 3])
def test_levels_match_model(n_hidden):
    """(376, 17, 512) at batch 4096: K = 394 / 377 at layer 0 (slab tails), 512 in the hidden
    levels, 4096 in the weight gradients; n_hidden 3 adds the plain critic and actor dh levels.
    Measured on the MI355X (max over the levels of a class, n_hidden 2 / 3; e_ref 2.3e-8 .. 4.3e-7
    over the levels, bars 4 x that):
      forward (bf16-stored)     outside the bounds: none; the bounds pin 99.5 .. 99.8 % of a
                                level's outputs to a single value
      dh, row prologue (L5/L9)  9.8e-8 / 8.2e-8      (e_ref 3.7e-8 .. 5.4e-8)
      dh, plain                 9.0e-8 / 1.3e-7      (e_ref 4.0e-8 .. 5.8e-8)
      dW weights                2.0e-7 / 2.6e-7      (e_ref 2.3e-8 .. 4.3e-7; the largest on the
                                layers whose dY and X are both masked or ReLU'd)
      bias, layer 0             1.2e-7 / 1.0e-7      (e_ref 3.1e-8 .. 1.5e-7)
      bias, row sums            1.2e-7 / 1.3e-7      bit-equal to rowsum_order32 on every output
    (20, 4): 9.3e-8, 9.8e-8, 8.3e-8, 3.6e-8, 5.6e-8; batch 4100: 1.0e-7, 1.1e-7, 2.2e-7, 1.1e-7,
    1.5e-7; batch 4095 with fp32 activations: forward 8.9e-8 (fp32-stored: bar 1.7e-7 .. 2.8e-7),
    8.8e-8, 9.7e-8, 2.0e-7, 1.3e-7, 1.4e-7.  The closest any level comes to its bar is 0.58 (L9).

    The row-sum bias gradients (layers >= 1, heads) are held to 4 x the error of the host's fp32
    emulation of the kernels' order of adds (bf16_model.rowsum_order32), not to 4 x e_ref: the
    critic head's bias gradient is a single output, torch's sum of that one column landed 7.6e-9
    from fp64 here (a bar of 3.0e-8, less than one fp32 rounding of a value of the scale's size)
    while k_dw_part16's per-thread / 16-thread / split order gives 4.7e-8 (q1.fc3.bias, n_hidden
    2).  Order alone explains it: the emulation matches every row-sum output of every case bit
    for bit (tests/test_bf16_model.py test_rowsum_order32_is_the_kernels_order)."""
    run_case(376, 17, 512, 4096, n_hidden, True, sites(n_hidden),
             record_to=os.environ.get("SACMI_RECORD_BF16_LEVELS") if n_hidden == 2 else None)


def test_levels_match_model_short_k():
    """K = 25 / 21 at layer 0: less than one slab."""
    run_case(20, 4, 512, 4096, 2, True, sites(2))


def test_levels_match_model_ragged_batch():
    """Batch 4100: row counts that are no multiple of 64 or 128 (the policy runs 8200 rows), and a
    weight-gradient K that is no multiple of the 64-deep slabs or of the split count.  The launch
    timeline samples on the device, which stops at batch 4096: the kernels are those of run_case's
    act16 argument (asserted: ctx.act16)."""
    run_case(376, 17, 512, 4100, 2, True, None)


def test_levels_match_model_fp32_activations():
    """bf16 operands with fp32-stored activations (k_fwd16 with fp32 A and C, k_axk16<...,
    ACT16 = false>, k_dw_part16<false>): batch 4095 at hidden 512, the one class of shapes below
    act16's batch 4096 that still reaches every selector (L12's 64 x 4 = 256 dh tiles need
    batch > 4032; hidden 1024 at batch 2048 is refused by the library: hidden_dim <= 1020) - and a
    second ragged batch.  The forward outputs are fp32, so they take the fp32-stored bar (ReLU is
    1-Lipschitz)."""
    run_case(376, 17, 512, 4095, 2, False, sites(2, fwd=({"k_fwd16"},)))
