// Running moments in fp64 (count, mean, M2 = sum (x - mean)^2): the per-value Welford step and
// Chan's merge, shared by k_obs_stats (obsnorm.hip) and k_ret_stats (retnorm.hip).  Never
// E[x^2] - mean^2.
#pragma once
#include <hip/hip_runtime.h>

namespace sacmi {

struct Moments { double n, mean, m2; };

// a <- a merged with b (Chan et al.): exact hand-over when either side is empty
__device__ __forceinline__ void chan_merge(Moments& a, const Moments& b) {
  if (b.n == 0.0) return;
  if (a.n == 0.0) { a = b; return; }
  const double n = a.n + b.n, d = b.mean - a.mean;
  a.mean = a.mean + d * (b.n / n);
  a.m2 = a.m2 + b.m2 + d * d * (a.n * b.n / n);
  a.n = n;
}

__device__ __forceinline__ void welford_step(Moments& a, double x) {
  a.n += 1.0;
  const double d = x - a.mean;
  a.mean += d / a.n;
  a.m2 += d * (x - a.mean);
}

__device__ __forceinline__ void welford_step(Moments& a, float xf) { welford_step(a, (double)xf); }

}  // namespace sacmi
