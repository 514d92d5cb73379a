// Running observation normalisation (sacmi_set_obs_norm): the running moments
// of the stored states, the fp32 vectors derived from them, and the two consumers that are
// launches of their own — the update's normalising gather and select_action's states.
//
// Moments: per column k the rows counted, the mean and M2 = sum (x - mean)^2, all fp64
// (ObsStatsArgs::mom).  A chunk s[m][S] is merged in one pass: a workgroup owns kObsCols
// columns, thread (rl, col) takes rows rl, rl + kObsRowLanes, ... of its column with a Welford
// step per row (every value loaded once: chunks of a few rows sit in host-mapped staging), the
// kObsRowLanes partials of a column are folded in lane order with Chan's merge by the column's
// owner thread, and the chunk's moments are merged into the running ones the same way.  Never
// E[x^2] - mean^2.  Fixed order, no atomics; every word of the state has one writer (the count
// is kept per column for that): the same chunks from the same state give the same bits.
//
// Vectors: nmean[k] = (float)mean, nrstd[k] = (float)(1 / sqrt(M2 / count + eps)) in fp64,
// rounded once; count == 0: mean 0, rstd 1 (identity), as the pad columns up to Sp.
#include "moments_dev.h"
#include "replay_dev.h"

namespace sacmi {

namespace {

constexpr int kObsThreads = kObsCols * kObsRowLanes;
static_assert(kObsThreads % kWave == 0, "whole waves");

__device__ __forceinline__ void obs_vectors(double n, double mean, double m2, double eps,
                                            float* nmean, float* nrstd) {
  const bool any = n > 0.0;
  *nmean = any ? (float)mean : 0.f;
  *nrstd = any ? (float)(1.0 / sqrt(m2 / n + eps)) : 1.f;
}

__global__ __launch_bounds__(kObsThreads) void k_obs_stats(ObsStatsArgs a) {
  __shared__ double s_part[3][kObsRowLanes][kObsCols];
  const int col = threadIdx.x % kObsCols, rl = threadIdx.x / kObsCols;
  const int k = blockIdx.x * kObsCols + col;
  const bool live = k < a.S;
  Moments p{0.0, 0.0, 0.0};
  // four rows in flight per thread: the loads of a round are issued before its steps
  constexpr int kR = 4;
  for (int i0 = rl; i0 < a.m; i0 += kR * kObsRowLanes) {
    float x[kR];
#pragma unroll
    for (int j = 0; j < kR; ++j) {
      const int i = i0 + j * kObsRowLanes;
      x[j] = live && i < a.m ? a.s[(size_t)i * a.S + k] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < kR; ++j)
      if (live && i0 + j * kObsRowLanes < a.m) welford_step(p, x[j]);
  }
  s_part[0][rl][col] = p.n; s_part[1][rl][col] = p.mean; s_part[2][rl][col] = p.m2;
  __syncthreads();
  if (rl != 0 || !live) return;
  Moments b{0.0, 0.0, 0.0};
  for (int q = 0; q < kObsRowLanes; ++q)
    chan_merge(b, Moments{s_part[0][q][col], s_part[1][q][col], s_part[2][q][col]});
  Moments run{a.mom[k], a.mom[a.Sp + k], a.mom[2 * a.Sp + k]};
  chan_merge(run, b);
  a.mom[k] = run.n; a.mom[a.Sp + k] = run.mean; a.mom[2 * a.Sp + k] = run.m2;
  obs_vectors(run.n, run.mean, run.m2, a.eps, a.vec + k, a.vec + a.Sp + k);
}

__global__ __launch_bounds__(256) void k_obs_refresh(const double* mom, float* vec, int S, int Sp,
                                                     double eps, float clip) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k == 0) vec[2 * Sp] = clip;
  if (k >= Sp) return;
  if (k < S) {
    obs_vectors(mom[k], mom[Sp + k], mom[2 * Sp + k], eps, vec + k, vec + Sp + k);
  } else {
    vec[k] = 0.f; vec[Sp + k] = 1.f;
  }
}

// a workgroup per row (grid-stride), threads over the row's ldd columns
__global__ __launch_bounds__(128) void k_obs_normalize(const float* src, int lds, float* dst, int ldd,
                                                       int n, int S, ObsNormArgs on) {
  const float clip = *on.clip;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const float* x = src + (size_t)i * lds;
    float* y = dst + (size_t)i * ldd;
    for (int k = threadIdx.x; k < ldd; k += blockDim.x)
      y[k] = k < S ? obs_normalize(x[k], on.nmean[k], on.nrstd[k], clip) : (k == S ? 1.f : 0.f);
  }
}

}  // namespace

void launch_obs_stats(const ObsStatsArgs& a, hipStream_t s) {
  if (a.m <= 0 || a.m > kObsMaxRows || a.S <= 0 || a.Sp < a.S)
    throw Error{SACMI_ESTATE, "k_obs_stats: bad chunk"};
  hipLaunchKernelGGL(k_obs_stats, dim3((a.S + kObsCols - 1) / kObsCols), dim3(kObsThreads), 0, s, a);
  launch_check("k_obs_stats");
}

void launch_obs_refresh(const double* mom, float* vec, int S, int Sp, double eps, float clip,
                        hipStream_t s) {
  hipLaunchKernelGGL(k_obs_refresh, dim3((Sp + 255) / 256), dim3(256), 0, s, mom, vec, S, Sp, eps, clip);
  launch_check("k_obs_refresh");
}

void launch_obs_normalize(const float* src, int lds, float* dst, int ldd, int n, int S,
                          const ObsNormArgs& on, hipStream_t s) {
  if (n <= 0 || S >= ldd || S > lds) throw Error{SACMI_ESTATE, "k_obs_normalize: bad rows"};
  hipLaunchKernelGGL(k_obs_normalize, dim3(n < 1024 ? n : 1024), dim3(128), 0, s, src, lds, dst, ldd,
                     n, S, on);
  launch_check("k_obs_normalize");
}

void launch_gather_norm(const GatherArgs& a, const ObsNormArgs& on, hipStream_t s) {
  hipLaunchKernelGGL((k_gather<true, ObsNormArgs>), dim3(a.B), dim3(128), 0, s, a, on);
  launch_check("k_gather<true>");
}

}  // namespace sacmi
