// Per-update training diagnostics (sacmi_set_stats; include/sacmi.h enum sacmi_stat): one
// row of SACMI_STAT_COUNT fp32 values per update, reduced from what the update's forward
// passes left in HBM — the critic head dot partials (slots 0-5), both log-prob halves, the
// batch's r and d, alpha and log_alpha before the alpha step — and appended to a ring.
//
// Arithmetic: a row's head value is the fp32 sum of its nparts dot partials in block order
// (block 0 carries the bias), exactly as the L5 / L9 row prologues finish them; the per-row
// quantities are fp32 in rows_coef's own expressions.  The sums accumulate in fp64 in a fixed
// order — each thread its rows in increasing order, a 64-wide shuffle tree inside the wave,
// the workgroup's waves through LDS in wave order, workgroup partials in index order — and
// each mean is divided in fp64 and rounded once.  No atomics: two runs from the same state
// give the same bits.
//
// Geometry: up to kStatOneWgRows rows (every device-sampled update) ONE launch of ONE
// workgroup, as k_per_feedback; past that (staged indices, up to max_batch 65536) one
// workgroup per kStatThreads rows stores its kStatAcc fp64 partials and a one-workgroup finish
// launch folds them — two stream-ordered launches, no last-arriver hand-off (what
// device-scope fences cost here).
//
// An update the error bits void appends nothing (any bit: the reference raised before it
// returned anything); the word is read once, before any barrier, and the appending thread's
// own reading decides.
#include "sacmi_internal.h"

namespace sacmi {

namespace {

constexpr int kStatWaves = kStatThreads / kWave;
static_assert(kStatThreads % kWave == 0, "whole waves");
static_assert(kStatOneWgRows % kStatThreads == 0, "the one-workgroup form takes whole passes");
// accumulators: sums of q1, q2, q^, td, min(qa1, qa2), log pi(a~|s), log pi(a~|s) +
// target_entropy, r; then the maximum of td
enum StatAcc { ACC_Q1 = 0, ACC_Q2, ACC_QT, ACC_TD, ACC_QPI, ACC_LP, ACC_LPT, ACC_R, ACC_TDMAX };
static_assert(ACC_TDMAX + 1 == kStatAcc, "accumulator count");

__device__ __forceinline__ double acc_join(int k, double a, double b) {
  return k == ACC_TDMAX ? fmax(a, b) : a + b;
}

// A row's six head values: each slot's partials summed in block order.  The row's partials
// are 4 nparts bytes per slot, a row per lane: every load instruction of a wave touches 64
// rows, so the loads go out kStatRound partials per slot at a time, all six slots at once,
// before the first is waited for (one load per partial, each waited for by its add, measured
// 14 us at batch 256 and 171 us at batch 4096 against 6.9 and 45 us), and 16 bytes wide where
// the rows are 16-byte aligned (V4: nparts % 4 == 0).  Indices past the row's end are clamped
// to its last element and their values never used.  (Reading the partials as consecutive
// 16-byte quads, a quad a lane, the lanes of a row passing the running sum along, measured
// 9.9 and 38 us: one workgroup's loads in flight bound the read, not its line rate.)
constexpr int kStatRound = 8;
template <bool V4>
__device__ __forceinline__ void head_values(const StatsArgs& a, int row, float (&q)[6]) {
  const int np = a.nparts;
  const float* p[6];
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    p[s] = a.dotp + ((size_t)s * a.B + row) * np;
    q[s] = 0.f;
  }
  for (int i0 = 0; i0 < np; i0 += kStatRound) {
    float x[6][kStatRound];
#pragma unroll
    for (int s = 0; s < 6; ++s) {
      if constexpr (V4) {
#pragma unroll
        for (int h = 0; h < kStatRound / 4; ++h) {
          const int i = min(i0 + 4 * h, np - 4);
          const float4 f = *reinterpret_cast<const float4*>(p[s] + i);
          x[s][4 * h] = f.x; x[s][4 * h + 1] = f.y; x[s][4 * h + 2] = f.z; x[s][4 * h + 3] = f.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < kStatRound; ++j) x[s][j] = p[s][min(i0 + j, np - 1)];
      }
    }
#pragma unroll
    for (int j = 0; j < kStatRound; ++j) {
      if (i0 + j < np) {          // (uniform)
#pragma unroll
        for (int s = 0; s < 6; ++s) q[s] = i0 + j == 0 ? x[s][j] : q[s] + x[s][j];
      }
    }
  }
}

// one row's terms (fp32, rows_coef's own expressions) into the thread's accumulators
__device__ __forceinline__ void add_row(const StatsArgs& a, float alpha, const float (&q)[6], float lp2,
                                        float lpa, float r, float d, double (&v)[kStatAcc]) {
  const float vt = fminf(q[2], q[3]) - alpha * lp2;
  const float qhat = r + ((1.f - d) * a.gamma) * vt;
  const float td = 0.5f * (fabsf(q[0] - qhat) + fabsf(q[1] - qhat));
  v[ACC_Q1] += (double)q[0];
  v[ACC_Q2] += (double)q[1];
  v[ACC_QT] += (double)qhat;
  v[ACC_TD] += (double)td;
  v[ACC_QPI] += (double)fminf(q[4], q[5]);
  v[ACC_LP] += (double)lpa;
  v[ACC_LPT] += (double)(lpa + a.target_entropy);
  v[ACC_R] += (double)r;
  v[ACC_TDMAX] = fmax(v[ACC_TDMAX], (double)td);
}

// this thread's rows (row_lo + t + k * kStatThreads, increasing) into its accumulators
template <bool V4>
__device__ __forceinline__ void accumulate_rows(const StatsArgs& a, int row_lo, int row_hi,
                                                double (&v)[kStatAcc]) {
  const float alpha = a.sc->alpha;
  for (int row = row_lo + (int)threadIdx.x; row < row_hi; row += kStatThreads) {
    float q[6];
    head_values<V4>(a, row, q);
    add_row(a, alpha, q, a.logp[row], a.logp[a.B + row], a.r[row], a.d[row], v);
  }
}

// This workgroup's rows [row_lo, row_hi) into kStatAcc values, valid in s_tot once the
// function returns (every thread calls it, with uniform arguments: it has barriers).
__device__ __forceinline__ void reduce_rows(const StatsArgs& a, int row_lo, int row_hi,
                                            double (*s_wave)[kStatAcc], double* s_tot) {
  const int t = threadIdx.x;
  double v[kStatAcc];
#pragma unroll
  for (int k = 0; k < kStatAcc; ++k) v[k] = 0.0;
  if ((a.nparts & 3) == 0) accumulate_rows<true>(a, row_lo, row_hi, v);
  else accumulate_rows<false>(a, row_lo, row_hi, v);
#pragma unroll
  for (int k = 0; k < kStatAcc; ++k)
#pragma unroll
    for (int off = kWave / 2; off >= 1; off >>= 1) v[k] = acc_join(k, v[k], __shfl_down(v[k], off, kWave));
  if ((t & (kWave - 1)) == 0) {
#pragma unroll
    for (int k = 0; k < kStatAcc; ++k) s_wave[t / kWave][k] = v[k];
  }
  __syncthreads();
  if (t < kStatAcc) {
    double acc = s_wave[0][t];
    for (int w = 1; w < kStatWaves; ++w) acc = acc_join(t, acc, s_wave[w][t]);
    s_tot[t] = acc;
  }
  __syncthreads();
}

// one thread: the row from the batch's accumulators, then the counter
__device__ __forceinline__ void append_row(const StatsArgs& a, const double* tot) {
  const double n = (double)a.B;
  const float alpha = a.sc->alpha, log_alpha = *a.log_alpha;
  const int64_t pos = *a.count;
  float* row = a.ring + (size_t)(pos % kStatRingSlots) * SACMI_STAT_COUNT;
  row[SACMI_STAT_Q1_MEAN] = (float)(tot[ACC_Q1] / n);
  row[SACMI_STAT_Q2_MEAN] = (float)(tot[ACC_Q2] / n);
  row[SACMI_STAT_Q_TARGET_MEAN] = (float)(tot[ACC_QT] / n);
  row[SACMI_STAT_TD_MEAN] = (float)(tot[ACC_TD] / n);
  row[SACMI_STAT_TD_MAX] = (float)tot[ACC_TDMAX];
  row[SACMI_STAT_Q_PI_MEAN] = (float)(tot[ACC_QPI] / n);
  row[SACMI_STAT_ENTROPY] = (float)(-(tot[ACC_LP] / n));
  row[SACMI_STAT_ALPHA] = alpha;
  row[SACMI_STAT_LOG_ALPHA] = log_alpha;
  row[SACMI_STAT_ALPHA_LOSS] = a.auto_entropy ? (float)(-(double)log_alpha * (tot[ACC_LPT] / n)) : 0.f;
  row[SACMI_STAT_REWARD_MEAN] = (float)(tot[ACC_R] / n);
  row[SACMI_STAT_BATCH] = (float)a.B;
  *a.count = pos + 1;
}

// PART 0: the whole batch in this one workgroup, row appended.  PART 1: workgroup b takes rows
// [b * kStatThreads, (b + 1) * kStatThreads) and stores its partials.
template <int PART>
__global__ __launch_bounds__(kStatThreads) void k_update_stats(StatsArgs a) {
  const TlMark tl_mark(a.tl, TL_UPDATE_STATS);
  // read once, before any barrier.  The appending thread's own value decides, and nobody
  // leaves early: a side stream's sampler may raise a bit while this kernel runs, and waves
  // that saw different words must not split at a barrier (a voided update's operands are
  // in bounds like any other's; what they hold is never stored)
  const int err = __atomic_load_n(&a.sc->err, __ATOMIC_RELAXED);
  __shared__ double s_wave[kStatWaves][kStatAcc];
  __shared__ double s_tot[kStatAcc];
  if constexpr (PART) {
    const int row_lo = blockIdx.x * kStatThreads;
    reduce_rows(a, row_lo, min(a.B, row_lo + kStatThreads), s_wave, s_tot);
    if (threadIdx.x < kStatAcc) a.ws[(size_t)blockIdx.x * kStatAcc + threadIdx.x] = s_tot[threadIdx.x];
  } else {
    reduce_rows(a, 0, a.B, s_wave, s_tot);
    if (threadIdx.x == 0 && !err) append_row(a, s_tot);
  }
}

// the workgroup partials folded in index order (one wave), row appended
__global__ __launch_bounds__(kWave) void k_update_stats_fin(StatsArgs a, int nwg) {
  const TlMark tl_mark(a.tl, TL_UPDATE_STATS);
  const int err = __atomic_load_n(&a.sc->err, __ATOMIC_RELAXED);   // (as above)
  __shared__ double s_tot[kStatAcc];
  const int t = threadIdx.x;
  if (t < kStatAcc) {
    double acc = a.ws[t];
    for (int b = 1; b < nwg; ++b) acc = acc_join(t, acc, a.ws[(size_t)b * kStatAcc + t]);
    s_tot[t] = acc;
  }
  __syncthreads();
  if (t == 0 && !err) append_row(a, s_tot);
}

}  // namespace

void launch_update_stats(const StatsArgs& a, hipStream_t s) {
  const int nwg = stats_workgroups(a.B);
  if (nwg == 1) {
    hipLaunchKernelGGL(k_update_stats<0>, dim3(1), dim3(kStatThreads), 0, s, a);
  } else {
    hipLaunchKernelGGL(k_update_stats<1>, dim3(nwg), dim3(kStatThreads), 0, s, a);
    StatsArgs f = a;
    if (f.tl) f.tl += kTlWords;
    hipLaunchKernelGGL(k_update_stats_fin, dim3(1), dim3(kWave), 0, s, f, nwg);
  }
  launch_check("update stats");
}

}  // namespace sacmi
