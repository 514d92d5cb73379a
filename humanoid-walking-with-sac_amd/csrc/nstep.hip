// N-step returns in the replay gather (sacmi_set_nstep).
//
// The ring is SoA and consecutive slots are consecutive env steps, so the n-step row of a
// sampled slot p0 is made where the row is gathered, from the ring as it is then: the chain
// p_j = (p0 + j) % capacity stops at the first row m that is terminal, carries an episode-end
// flag, is the newest row, or has j = n - 1, and the gathered row is
//     s, a from p0 | r[b] = R = r_0 + g[1] r_1 + ... + g[m] r_m | s2 from p_m | d[b] = d'
// with d' = 1 for a terminal p_m, 0 for m = 0, else 1 - g[m]: the unchanged row algebra's
// fl(fl(1 - d') * gamma) is then the bootstrap coefficient gamma^(m + 1).  Nothing downstream
// of the gather knows (heads, critic rows, diagnostics, prioritized feedback).
//
// k_gather_nstep: a workgroup of 128 threads per row, as k_gather.  The chain is not walked:
// lane j of the first wave loads rew / done / ep_end of p_j and g[j] in one round trip, m is the
// first set bit of the ballot over the stop predicate, and R is accumulated in the fixed order
// from cross-lane reads.  s and a (from p0) do not depend on m: both waves copy them before
// the workgroup meets at the barrier behind which m is known; only the s2 loads from p_m form
// a second round trip.  The copies are gather_row's (write-through stores, float4 groups and
// the S % 4 tail, fp32 or bf16 rows, obs_normalize when NORM), split in two halves — which is
// why they are bodies of their own here and gather_row (every riding kernel's) is untouched.
//
// k_ep_scatter: the episode-end flags of a pushed chunk, behind k_push_rows.
#include "replay_dev.h"

namespace sacmi {

namespace {

// One state row `src` (ring) into minibatch row `row` of `base`, and with TWO also into row
// `row2` of `base2`; X16: bf16 rows, rounded once after normalising.
template <bool NORM, bool X16, bool TWO>
__device__ __forceinline__ void nstep_state(const GatherArgs& a, const float* src, float* base, int row,
                                            float* base2, int row2, int t, const ObsNormArgs& on,
                                            float clip) {
  constexpr uint32_t es = X16 ? 2u : 4u;
  const uint32_t o1 = (uint32_t)((size_t)row * a.ldx) * es;
  const uint32_t o2 = (uint32_t)((size_t)row2 * a.ldx) * es;
  const int s4 = a.S >> 2;
  for (int q = t; q < s4; q += 128) {
    float4 v = reinterpret_cast<const float4*>(src)[q];
    if constexpr (NORM) {
      const float4 mu = reinterpret_cast<const float4*>(on.nmean)[q];
      const float4 rs = reinterpret_cast<const float4*>(on.nrstd)[q];
      v.x = obs_normalize(v.x, mu.x, rs.x, clip); v.y = obs_normalize(v.y, mu.y, rs.y, clip);
      v.z = obs_normalize(v.z, mu.z, rs.z, clip); v.w = obs_normalize(v.w, mu.w, rs.w, clip);
    }
    if constexpr (X16) {
      const uint32_t vl = f2bf2(v.x, v.y), vh = f2bf2(v.z, v.w);
      st_wt8(base, o1 + 8u * q, vl, vh);
      if constexpr (TWO) st_wt8(base2, o2 + 8u * q, vl, vh);
    } else {
      st_wt4(base, o1 + 16u * q, v);
      if constexpr (TWO) st_wt4(base2, o2 + 16u * q, v);
    }
  }
  for (int q = 4 * s4 + t; q < a.S; q += 128) {
    float v = src[q];
    if constexpr (NORM) v = obs_normalize(v, on.nmean[q], on.nrstd[q], clip);
    if constexpr (X16) {
      st_wt2(base, o1 + 2u * q, f2bf(v));
      if constexpr (TWO) st_wt2(base2, o2 + 2u * q, f2bf(v));
    } else {
      st_wt(base + (size_t)row * a.ldx + q, v);
      if constexpr (TWO) st_wt(base2 + (size_t)row2 * a.ldx + q, v);
    }
  }
}

// the actions of slot p0 and the three ones columns of minibatch row b
template <bool X16>
__device__ __forceinline__ void nstep_act_ones(const GatherArgs& a, int64_t p0, int b, int t) {
  const float* ac = a.act + p0 * a.lda_;
  if constexpr (X16) {
    const uint32_t oq = (uint32_t)((size_t)b * a.ldx) * 2u;
    const uint32_t oa = (uint32_t)((size_t)(a.B + b) * a.ldx) * 2u;
    for (int j = t; j < a.A; j += 128) st_wt2(a.xq, oq + 2u * (a.S + 1 + j), f2bf(ac[j]));
    if (t == 127) {
      st_wt2(a.xq, oq + 2u * a.S, kBf16One); st_wt2(a.x2, oa + 2u * a.S, kBf16One);
      st_wt2(a.x2, oq + 2u * a.S, kBf16One);
    }
  } else {
    float* xq = a.xq + (size_t)b * a.ldx;
    float* xt = a.x2 + (size_t)b * a.ldx;
    float* xa = a.x2 + (size_t)(a.B + b) * a.ldx;
    for (int j = t; j < a.A; j += 128) st_wt(xq + a.S + 1 + j, ac[j]);
    if (t == 127) { st_wt(xq + a.S, 1.f); st_wt(xa + a.S, 1.f); st_wt(xt + a.S, 1.f); }
  }
}

__device__ __forceinline__ float lane_read(float v, int j) {   // j wave-uniform
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
}

template <bool NORM, bool X16>
__device__ __forceinline__ void nstep_row(const GatherArgs& a, const NStepArgs& ns, const ObsNormArgs& on,
                                          int* s_m) {
  const int b = blockIdx.x, t = threadIdx.x;
  const int64_t cap = a.capacity, head = a.sc->head, len = a.sc->len;
  const int64_t ix = a.idx[b];
  const int64_t p0 = a.by_slot ? ix : (head + ix) % cap;
  float clip = 0.f;
  if constexpr (NORM) clip = *on.clip;
  // ---- the chain, one lane per step (first wave): lanes 0..jmax load their row's reward,
  // terminal and flag (the others the row p0 again: in bounds, discarded)
  const bool chain = t < kWave;
  float rj = 0.f, dj = 0.f, gj = 0.f;
  uint8_t ej = 0;
  int jmax = 0;
  if (chain) {
    const int64_t i = a.by_slot ? (ix - head + cap) % cap : ix;    // deque position
    int n = *ns.n;
    n = n < 1 ? 1 : (n > kNStepMax ? kNStepMax : n);
    int64_t room = len - 1 - i;                 // rows behind this one, up to the newest
    room = room < 0 ? 0 : room;
    jmax = room < n - 1 ? (int)room : n - 1;                       // 0..31, < capacity
    int64_t pj = p0 + (t <= jmax ? t : 0);
    pj = pj >= cap ? pj - cap : pj;
    rj = a.rew[pj];
    dj = a.done[pj];
    ej = ns.ep_end[pj];
    gj = ns.g[t & (kNStepMax - 1)];
  }
  // s and a of p0 do not depend on m: their loads ride the same round trip
  nstep_state<NORM, X16, true>(a, a.obs + p0 * a.ldo, a.xq, b, a.x2, a.B + b, t, on, clip);
  nstep_act_ones<X16>(a, p0, b, t);
  if (chain) {
    const unsigned long long stop = __ballot(t <= jmax && (dj != 0.f || ej != 0 || t == jmax));
    const int m = __ffsll((long long)stop) - 1;                    // lane jmax always stops
    const float term = __fmul_rn(gj, rj);
    float R = lane_read(rj, 0);
    for (int j = 1; j <= m; ++j) R = __fadd_rn(R, lane_read(term, j));
    const float dm = lane_read(dj, m), gm = lane_read(gj, m);
    if (t == 0) {
      *s_m = m;
      st_wt(a.r + b, R);
      st_wt(a.d + b, dm != 0.f ? 1.f : (m == 0 ? 0.f : __fsub_rn(1.f, gm)));
    }
  }
  __syncthreads();
  // ---- the second round trip: s2 of p_m
  int64_t pm = p0 + *s_m;
  pm = pm >= cap ? pm - cap : pm;
  nstep_state<NORM, X16, false>(a, a.obs2 + pm * a.ldo, a.x2, b, nullptr, 0, t, on, clip);
}

template <bool NORM, class... On>
__global__ __launch_bounds__(128) void k_gather_nstep(GatherArgs a, NStepArgs ns, On... on) {
  const TlMark tl_mark(a.tl, TL_GATHER);
  __shared__ int s_m;
  if constexpr (NORM) {
    if (a.x16) nstep_row<true, true>(a, ns, on..., &s_m);
    else nstep_row<true, false>(a, ns, on..., &s_m);
  } else {
    if (a.x16) nstep_row<false, true>(a, ns, ObsNormArgs{}, &s_m);
    else nstep_row<false, false>(a, ns, ObsNormArgs{}, &s_m);
  }
}

// the chunk's flags into the slots k_push_rows just stored its rows in
__global__ __launch_bounds__(256) void k_ep_scatter(const uint8_t* stage, uint8_t* ep_end, int64_t n,
                                                    int64_t pos0, int64_t cap) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    ep_end[(pos0 + i) % cap] = stage[i] ? 1 : 0;
}

__global__ void k_nstep_table(NStepTable tab, float* g, int32_t* n) {
  const int t = threadIdx.x;
  if (t < kNStepMax) g[t] = tab.g[t];
  if (t == 0) *n = tab.n;
}

}  // namespace

void launch_gather_nstep(const GatherArgs& a, const NStepArgs& ns, const ObsNormArgs* on, hipStream_t s) {
  if (!ns.n || !ns.g || !ns.ep_end) throw Error{SACMI_ESTATE, "k_gather_nstep: no n-step state"};
  if (on) hipLaunchKernelGGL((k_gather_nstep<true, ObsNormArgs>), dim3(a.B), dim3(128), 0, s, a, ns, *on);
  else hipLaunchKernelGGL((k_gather_nstep<false>), dim3(a.B), dim3(128), 0, s, a, ns);
  launch_check("k_gather_nstep");
}

void launch_ep_scatter(const uint8_t* stage, uint8_t* ep_end, int64_t n, int64_t pos0, int64_t cap,
                       hipStream_t s) {
  if (n <= 0 || n > cap || pos0 < 0 || pos0 >= cap) throw Error{SACMI_ESTATE, "k_ep_scatter: bad chunk"};
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_ep_scatter, dim3((unsigned)(blocks < 64 ? blocks : 64)), dim3(256), 0, s, stage,
                     ep_end, n, pos0, cap);
  launch_check("k_ep_scatter");
}

void launch_nstep_table(const NStepTable& tab, float* g, int32_t* n, hipStream_t s) {
  hipLaunchKernelGGL(k_nstep_table, dim3(1), dim3(64), 0, s, tab, g, n);
  launch_check("k_nstep_table");
}

}  // namespace sacmi
