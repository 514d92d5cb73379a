// Reward scaling and running return normalisation (sacmi_set_reward_norm).
//
// State: st [4] fp64 = count | mean | M2 of the discounted returns seen | ret, the running
// discounted return of the episode being pushed.  For every stored transition, in push order,
//     ret = fl64(fl64(ret * gamma) + r)        (__dmul_rn / __dadd_rn: never contracted)
//     (count, mean, M2) take ret; ret = 0 behind a terminal row or an episode-end flag
// The factor kc[0] = (float)(scale / sqrt(M2 / count + eps)) (count == 0 or the constant-scale
// mode: (float)scale) and kc[1] = clip are what the per-update kernel reads.
//
// k_ret_stats, one workgroup per pushed chunk of at most kRetMaxRows rows, behind the chunk's
// k_push_rows on the same stream: all threads load r, d and the flags into LDS (every value
// loaded once: chunks of a few rows sit in host-mapped staging); thread 0 runs the recurrence,
// serial by nature, writing ret_i to LDS; lane l < kRetRowLanes takes ret_l, ret_(l + 16), ...
// with a Welford step each; thread 0 folds the lanes in lane order with Chan's merge, merges the
// chunk into the running moments and refreshes the factor (the scheme and the helpers of
// k_obs_stats).  Fixed order, no atomics, one writer per word: the same pushes from the same
// state give the same bits.
//
// k_reward_norm, one small launch per update behind whatever produced the minibatch: out of
// place (a replayed or profiled launch never scales twice), k and clip through pointers.
#include "moments_dev.h"
#include "sacmi_internal.h"

namespace sacmi {

namespace {

constexpr int kRetThreads = 256;
static_assert(kRetRowLanes <= kWave, "the Welford lanes are lanes of the first wave");

__device__ __forceinline__ float ret_factor(double n, double m2, double scale, double eps, int use_state) {
  return use_state && n > 0.0 ? (float)(scale / sqrt(m2 / n + eps)) : (float)scale;
}

__global__ __launch_bounds__(kRetThreads) void k_ret_stats(RetStatsArgs a) {
  __shared__ float s_r[kRetMaxRows];
  __shared__ uint8_t s_stop[kRetMaxRows];
  __shared__ double s_ret[kRetMaxRows];
  __shared__ double s_part[3][kRetRowLanes];
  const int t = threadIdx.x;
  for (int i = t; i < a.m; i += kRetThreads) {
    const float r = a.r[i], d = a.d[i];
    const uint8_t e = a.end ? a.end[i] : (uint8_t)0;
    s_r[i] = r;
    s_stop[i] = d != 0.f || e != 0 ? 1 : 0;
  }
  __syncthreads();
  if (t == 0) {
    double ret = a.reset ? 0.0 : a.st[3];
    for (int i = 0; i < a.m; ++i) {
      ret = __dadd_rn(__dmul_rn(ret, a.gamma), (double)s_r[i]);
      s_ret[i] = ret;
      if (s_stop[i]) ret = 0.0;
    }
    a.st[3] = ret;
  }
  __syncthreads();
  if (t < kRetRowLanes) {
    Moments p{0.0, 0.0, 0.0};
    for (int i = t; i < a.m; i += kRetRowLanes) welford_step(p, s_ret[i]);
    s_part[0][t] = p.n; s_part[1][t] = p.mean; s_part[2][t] = p.m2;
  }
  __syncthreads();
  if (t != 0) return;
  Moments run{a.st[0], a.st[1], a.st[2]};
  if (a.m > 0) {
    Moments b{0.0, 0.0, 0.0};
    for (int q = 0; q < kRetRowLanes; ++q) chan_merge(b, Moments{s_part[0][q], s_part[1][q], s_part[2][q]});
    chan_merge(run, b);
    a.st[0] = run.n; a.st[1] = run.mean; a.st[2] = run.m2;
  }
  a.kc[0] = ret_factor(run.n, run.m2, a.scale, a.eps, a.use_state);
  a.kc[1] = a.clip;
}

__global__ __launch_bounds__(256) void k_reward_norm(const float* r, float* rn, int B, const float* kc,
                                                     tl_word* tl) {
  const TlMark tl_mark(tl, TL_GATHER);
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) rn[b] = reward_normalize(r[b], kc[0], kc[1]);
}

}  // namespace

void launch_ret_stats(const RetStatsArgs& a, hipStream_t s) {
  if (a.m < 0 || a.m > kRetMaxRows || !a.st || !a.kc || (a.m > 0 && (!a.r || !a.d)))
    throw Error{SACMI_ESTATE, "k_ret_stats: bad chunk"};
  hipLaunchKernelGGL(k_ret_stats, dim3(1), dim3(kRetThreads), 0, s, a);
  launch_check("k_ret_stats");
}

void launch_reward_norm(const float* r, float* rn, int B, const float* kc, tl_word* tl, hipStream_t s) {
  if (B <= 0 || !r || !rn || !kc || r == rn) throw Error{SACMI_ESTATE, "k_reward_norm: bad batch"};
  hipLaunchKernelGGL(k_reward_norm, dim3((B + 255) / 256), dim3(256), 0, s, r, rn, B, kc, tl);
  launch_check("k_reward_norm");
}

}  // namespace sacmi
