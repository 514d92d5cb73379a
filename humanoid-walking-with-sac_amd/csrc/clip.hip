// Global-norm gradient clipping (sacmi_set_grad_clip; include/sacmi.h enum sacmi_gnorm): the
// device reduction of the gradient arena to per-group sums of squares.  Three groups, as the
// reference's three network optimizers: q1, q2 (one launch over the critic range) and policy
// (one over the actor range); log_alpha is never clipped.
//
// What counts: a Linear is stored W~[n_out][ld] with the bias in a column and ld - kdim() pad
// columns; only the columns < kdim() of each row are torch's weight and bias elements.  The
// pad columns are masked, whatever they hold.
//
// Arithmetic: each element is (g * grad_scale)^2 with the product rounded to fp32 first (the
// value Adam steps from), squared and accumulated in fp64.  Fixed order, as stats.hip: a wave
// takes whole rows (wave v of the group's W * kClipWaves: rows v, v + W * kClipWaves, ... of the
// group's segments in segment order), lane l the row's 16-byte quads l, l + 64, ...; then a
// 64-wide shuffle tree, the workgroup's waves through LDS in wave order, one fp64 partial per
// workgroup.  k_adam's prologue folds a group's partials in index order (kernels.hip).  No
// atomics, no last-arriver hand-off: two runs from the same state give the same bits.
#include "sacmi_internal.h"

namespace sacmi {

namespace {

constexpr int kClipWaves = kClipThreads / kWave;
static_assert(kClipThreads % kWave == 0, "whole waves");
constexpr int kClipRows = 4;   // rows a wave has in flight

__device__ __forceinline__ double quad_sq(float4 f, int col, int kdim, float gs) {
  const float x = f.x * gs, y = f.y * gs, z = f.z * gs, w = f.w * gs;
  double s = 0.0;
  if (col < kdim) s += (double)x * (double)x;
  if (col + 1 < kdim) s += (double)y * (double)y;
  if (col + 2 < kdim) s += (double)z * (double)z;
  if (col + 3 < kdim) s += (double)w * (double)w;
  return s;
}

__global__ __launch_bounds__(kClipThreads) void k_grad_sumsq(GradSumsqArgs a) {
  const TlMark tl_mark(a.tl, TL_GRAD_SUMSQ);
  __shared__ double s_wave[kClipWaves];
  int grp = 0;
  for (int k = 1; k < a.ngroups; ++k)
    if ((int)blockIdx.x >= a.wg_begin[k]) grp = k;
  const int wg = blockIdx.x - a.wg_begin[grp], nwg = a.wg_begin[grp + 1] - a.wg_begin[grp];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int v = wg * kClipWaves + wave, nv = nwg * kClipWaves;
  double acc = 0.0;
  int row0 = 0;                 // the group's rows before this segment
  for (int sg = 0; sg < a.nseg; ++sg) {
    const ClipSeg seg = a.seg[sg];
    if (seg.group != grp) continue;
    const int ld4 = seg.ld / 4;
    // this wave's first row inside the segment: the smallest r >= 0 with (row0 + r) % nv == v
    int r = (v - row0 % nv + nv) % nv;
    for (; r < seg.rows; r += kClipRows * nv) {
      for (int q = lane; q < ld4; q += kWave) {
        // kClipRows rows' quads loaded before the first is used (rows past the segment:
        // the last row again, never added)
        float4 f[kClipRows];
#pragma unroll
        for (int j = 0; j < kClipRows; ++j) {
          const int rr = min(r + j * nv, seg.rows - 1);
          f[j] = *reinterpret_cast<const float4*>(a.g + seg.off + (int64_t)rr * seg.ld + 4 * q);
        }
#pragma unroll
        for (int j = 0; j < kClipRows; ++j)
          if (r + j * nv < seg.rows) acc += quad_sq(f[j], 4 * q, seg.kdim, a.grad_scale);
      }
    }
    row0 += seg.rows;
  }
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) acc += __shfl_down(acc, off, kWave);
  if (lane == 0) s_wave[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = s_wave[0];
    for (int w = 1; w < kClipWaves; ++w) t += s_wave[w];
    a.part[blockIdx.x] = t;
  }
}

#ifdef SACMI_CLIP_SEPARATE_FINISH
// the A/B of DESIGN §19: the partials folded once, by one wave, in a launch of its own
__global__ __launch_bounds__(kWave) void k_clip_finish(GradSumsqArgs a) {
  const TlMark tl_mark(a.tl, TL_GRAD_SUMSQ);
  const int k = threadIdx.x;
  if (k < a.ngroups) {
    double sum = a.part[a.wg_begin[k]];
    for (int w = a.wg_begin[k] + 1; w < a.wg_begin[k + 1]; ++w) sum += a.part[w];
    const float norm = (float)sqrt(sum);
    a.clip->fin[a.group0 + k][0] = norm;
    a.clip->fin[a.group0 + k][1] = clip_coef(norm, a.clip->max_norm[a.group0 + k]);
  }
}
#endif

__global__ void k_set_clip(ClipState* cs, float q1, float q2, float pi) {
  if (threadIdx.x == 0) { cs->max_norm[0] = q1; cs->max_norm[1] = q2; cs->max_norm[2] = pi; }
}

}  // namespace

void launch_grad_sumsq(const GradSumsqArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_grad_sumsq, dim3((unsigned)a.wg_begin[a.ngroups]), dim3(kClipThreads), 0, s, a);
#ifdef SACMI_CLIP_SEPARATE_FINISH
  GradSumsqArgs f = a;
  if (f.tl) f.tl += kTlWords;
  hipLaunchKernelGGL(k_clip_finish, dim3(1), dim3(kWave), 0, s, f);
#endif
  launch_check("grad sumsq");
}

void launch_set_clip(ClipState* cs, float q1, float q2, float pi, hipStream_t s) {
  hipLaunchKernelGGL(k_set_clip, dim3(1), dim3(kWave), 0, s, cs, q1, q2, pi);
  launch_check("set clip thresholds");
}

}  // namespace sacmi
