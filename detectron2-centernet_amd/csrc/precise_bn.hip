// PreciseBN (TEST.PRECISE_BN): population BatchNorm statistics over many batches, merged by Chan's parallel
// formula in f64 -- bn_slot_combine of train_bwd.hip stretched over iterations as well as ranks.
//
// The state is state[3][total] in f64: per channel the row count n, the mean mu and the sum of squared deviations M2 (all
// zeros when fresh).  One step folds a batch of M rows with mean m and sum of squared deviations M2_b into it:
//
//   n' = n + M;  w = M / n';  d = m - mu
//   mu' = mu + d * w
//   M2' = M2 + (M2_b + d * d * (n * w))
//
// and a state with n == 0 takes (M, m, M2_b) as they are, bit for bit.  MERGE reads a batch where the training forward left
// it at momentum 1: running_mean is m, running_var the unbiased variance u, so M2_b = u * (M - 1) with M from rows[s].
// FINISH combines the [world][3][total] rank slots in rank order by the same step and writes running_mean = (float)mu,
// running_var = (float)(M2 / n), the population variance.
//
// Both walk the EMA's kind of table (ema.hip): segment s is channels seg_start[s] .. seg_start[s + 1] of the state on one
// side and mean_ptrs[s][0 ..) / var_ptrs[s][0 ..) on the other.  blockIdx.x is the segment, one thread owns one channel (no
// atomics), scalar accesses: the data is a few KB and the launch is what costs.
#include "common.h"

typedef float __attribute__((address_space(1)))* pbn_gptr;

struct PbnAcc {
  double n, mu, m2;
};

__device__ __forceinline__ void pbn_chan_step(PbnAcc& a, double M, double m, double m2b) {
  if (a.n == 0) {
    a.n = M; a.mu = m; a.m2 = m2b;
    return;
  }
  const double nt = a.n + M, w = M / nt, d = m - a.mu;
  a.mu += d * w;
  a.m2 += m2b + d * d * (a.n * w);
  a.n = nt;
}

__global__ void __launch_bounds__(256) precise_bn_merge_kernel(const float* const* __restrict__ mean_ptrs,
                                                               const float* const* __restrict__ var_ptrs,
                                                               const long* __restrict__ seg_start, const long* __restrict__ rows,
                                                               double* __restrict__ state, long total) {
  const long start = seg_start[blockIdx.x], len = seg_start[blockIdx.x + 1] - start;
  const pbn_gptr mean = (pbn_gptr)mean_ptrs[blockIdx.x], var = (pbn_gptr)var_ptrs[blockIdx.x];
  const double M = (double)rows[blockIdx.x];
  for (long i = (long)blockIdx.y * 256 + threadIdx.x; i < len; i += (long)gridDim.y * 256) {
    const long c = start + i;
    if (c < 0 || c >= total) continue;
    PbnAcc a = {state[c], state[total + c], state[2 * total + c]};
    const double m = (double)mean[i], u = (double)var[i];
    pbn_chan_step(a, M, m, u * (M - 1.0));
    state[c] = a.n;
    state[total + c] = a.mu;
    state[2 * total + c] = a.m2;
  }
}

__global__ void __launch_bounds__(256) precise_bn_finish_kernel(float* const* __restrict__ mean_ptrs,
                                                                float* const* __restrict__ var_ptrs,
                                                                const long* __restrict__ seg_start,
                                                                const double* __restrict__ slots, int world, long total) {
  const long start = seg_start[blockIdx.x], len = seg_start[blockIdx.x + 1] - start;
  const pbn_gptr mean = (pbn_gptr)mean_ptrs[blockIdx.x], var = (pbn_gptr)var_ptrs[blockIdx.x];
  for (long i = (long)blockIdx.y * 256 + threadIdx.x; i < len; i += (long)gridDim.y * 256) {
    const long c = start + i;
    if (c < 0 || c >= total) continue;
    PbnAcc a = {0.0, 0.0, 0.0};
    for (int r = 0; r < world; ++r) {
      const double* slot = slots + (long)r * 3 * total;
      const double nb = slot[c];
      if (!(nb > 0)) continue;              // an empty slot contributes nothing (and no 0 / 0)
      pbn_chan_step(a, nb, slot[total + c], slot[2 * total + c]);
    }
    if (!(a.n > 0)) continue;               // nothing was measured for this channel: its statistics stay
    mean[i] = (float)a.mu;
    var[i] = (float)(a.m2 / a.n);
  }
}

// grid.y: a workgroup per 256 channels of the longest segment, capped (a workgroup loops over what is left)
static dim3 pbn_grid(int nseg, long max_len) {
  long per_seg = (max_len + 255) / 256;
  if (per_seg > 64) per_seg = 64;
  if (per_seg < 1) per_seg = 1;
  return dim3((unsigned)nseg, (unsigned)per_seg);
}

int launch_precise_bn_merge(const float* const* mean_ptrs, const float* const* var_ptrs, const long* seg_start, const long* rows,
                            int nseg, long max_len, double* state, long total, hipStream_t s) {
  if (nseg == 0 || max_len == 0 || total == 0) return 0;
  hipLaunchKernelGGL(precise_bn_merge_kernel, pbn_grid(nseg, max_len), dim3(256), 0, s, mean_ptrs, var_ptrs, seg_start, rows,
                     state, total);
  CTDET_LAUNCH_CHECK();
  return 0;
}

int launch_precise_bn_finish(float* const* mean_ptrs, float* const* var_ptrs, const long* seg_start, int nseg, long max_len,
                             const double* slots, int world, long total, hipStream_t s) {
  if (nseg == 0 || max_len == 0 || total == 0) return 0;
  hipLaunchKernelGGL(precise_bn_finish_kernel, pbn_grid(nseg, max_len), dim3(256), 0, s, mean_ptrs, var_ptrs, seg_start, slots,
                     world, total);
  CTDET_LAUNCH_CHECK();
  return 0;
}
