// Exponential moving average of the weights (SOLVER.EMA): the update behind the optimizer step and the
// in-place exchange that puts the averaged weights under the model for an evaluation.
//
//   t = updates[0];  updates[0] = t + 1
//   d = warmup ? min(decay, (1 + t) / (10 + t)) : decay          (f64)
//   w = (float)(1 - d)                                            (rounded once)
//   e = fmaf(w, p - e, e)                                         (torch's lerp_ for w < 0.5: p - e is exact for nearby values)
//
// The update count lives in device memory for the reason Adam's step count does (train_ops.hip): the captured training step
// replays the update without the host, so a host counter would freeze the warm-up decay at the value of the capture.
//
// Both element kernels walk SEGMENTS: segment s is ema[seg_start[s] .. seg_start[s + 1]) on one side and live_ptrs[s][0 ..)
// on the other.  The flat parameter buffer is one segment shared by many workgroups; the BatchNorm running statistics are
// about a hundred short segments of one workgroup each, read where the modules keep them (nothing is re-pointed, so the
// captured BatchNorm kernels keep their addresses).  Layout as in sgd_runs_body: blockIdx.x is the segment, the blockIdx.y
// workgroups of a segment own contiguous ranges of it, a thread walks its range four elements at a time in steps of 1024.
// Streams per element of the update: e and p read, e written (12 B).
#include "common.h"

__global__ void ema_advance_kernel(long long* __restrict__ updates, float* __restrict__ weight, double decay, int warmup) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const long long t = updates[0];
  updates[0] = t + 1;
  double d = decay;
  if (warmup) {
    const double ramp = (1.0 + (double)t) / (10.0 + (double)t);
    d = ramp < d ? ramp : d;
  }
  weight[0] = (float)(1.0 - d);
}

int launch_ema_advance(long long* updates, float* weight, double decay, int warmup, hipStream_t s) {
  hipLaunchKernelGGL(ema_advance_kernel, dim3(1), dim3(64), 0, s, updates, weight, decay, warmup);
  CTDET_LAUNCH_CHECK();
  return 0;
}

// the live pointers come out of a table: cast to the global address space, or the compiler has to use flat accesses.  Plain
// vector types, because the members of HIP's float4 / uint4 classes want objects in the generic address space
typedef float __attribute__((address_space(1)))* ema_gptr;
typedef unsigned __attribute__((address_space(1)))* ema_gptr_u32;
typedef float ema_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned ema_u32x4 __attribute__((ext_vector_type(4)));

// the range [beg, end) of segment blockIdx.x that workgroup blockIdx.y owns (a multiple of 1024 elements per workgroup, so
// that every thread's first element keeps the alignment of the segment's first), and whether 16-byte accesses are legal:
// both sides 16-byte aligned at the segment's start
struct EmaRange {
  ema_gptr live;
  float* ema;
  long beg, end;
  bool vec;
};

__device__ __forceinline__ EmaRange ema_range(float* const* __restrict__ live_ptrs, float* __restrict__ ema,
                                              const long* __restrict__ seg_start) {
  EmaRange r;
  const long start = seg_start[blockIdx.x], len = seg_start[blockIdx.x + 1] - start;
  r.live = (ema_gptr)live_ptrs[blockIdx.x];
  r.ema = ema + start;
  const long per = (((len + gridDim.y - 1) / gridDim.y) + 1023) & ~1023L;
  r.beg = (long)blockIdx.y * per;
  r.end = r.beg + per < len ? r.beg + per : len;
  r.vec = ((((uintptr_t)live_ptrs[blockIdx.x]) | ((uintptr_t)r.ema)) & 15) == 0;
  return r;
}

__global__ void __launch_bounds__(256) ema_lerp_segments_kernel(const float* const* __restrict__ live_ptrs,
                                                                float* __restrict__ ema, const long* __restrict__ seg_start,
                                                                const float* __restrict__ weight) {
  const EmaRange r = ema_range((float* const*)live_ptrs, ema, seg_start);
  if (r.beg >= r.end) return;
  const float w = weight[0];
  const ema_gptr p = r.live;
  float* __restrict__ e = r.ema;
  for (long i = r.beg + (long)threadIdx.x * 4; i < r.end; i += 1024) {
    if (r.vec && i + 4 <= r.end) {
      const ema_f32x4 pv = *(const ema_f32x4 __attribute__((address_space(1)))*)(p + i);
      ema_f32x4 ev = *(const ema_f32x4*)(e + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) ev[k] = fmaf(w, pv[k] - ev[k], ev[k]);
      *(ema_f32x4*)(e + i) = ev;
    } else {
      for (long j = i; j < i + 4 && j < r.end; ++j) {
        const float ej = e[j];
        e[j] = fmaf(w, p[j] - ej, ej);
      }
    }
  }
}

// the exchange moves integers: a float move may quieten a signalling NaN, an integer move keeps every bit (NaN payloads, -0)
__global__ void __launch_bounds__(256) ema_swap_segments_kernel(float* const* __restrict__ live_ptrs, float* __restrict__ ema,
                                                                const long* __restrict__ seg_start) {
  const EmaRange r = ema_range(live_ptrs, ema, seg_start);
  if (r.beg >= r.end) return;
  const ema_gptr_u32 p = (ema_gptr_u32)r.live;
  unsigned* __restrict__ e = (unsigned*)r.ema;
  for (long i = r.beg + (long)threadIdx.x * 4; i < r.end; i += 1024) {
    if (r.vec && i + 4 <= r.end) {
      const ema_u32x4 pv = *(const ema_u32x4 __attribute__((address_space(1)))*)(p + i), ev = *(const ema_u32x4*)(e + i);
      *(ema_u32x4 __attribute__((address_space(1)))*)(p + i) = ev;
      *(ema_u32x4*)(e + i) = pv;
    } else {
      for (long j = i; j < i + 4 && j < r.end; ++j) {
        const unsigned pj = p[j], ej = e[j];
        p[j] = ej;
        e[j] = pj;
      }
    }
  }
}

// grid.y: enough workgroups for the longest segment at 1024 elements each, capped so that the whole grid stays near the 2048
// workgroups of launch_sgd_runs (eight per CU); a workgroup loops over what its share of a longer segment holds
static dim3 ema_grid(int nseg, long max_len) {
  long per_seg = (max_len + 1023) / 1024, cap = 2048 / nseg;
  if (cap < 1) cap = 1;
  if (per_seg > cap) per_seg = cap;
  if (per_seg < 1) per_seg = 1;
  return dim3((unsigned)nseg, (unsigned)per_seg);
}

int launch_ema_lerp_segments(const float* const* live_ptrs, float* ema, const long* seg_start, int nseg, long max_len,
                             const float* weight, hipStream_t s) {
  if (nseg == 0 || max_len == 0) return 0;
  hipLaunchKernelGGL(ema_lerp_segments_kernel, ema_grid(nseg, max_len), dim3(256), 0, s, live_ptrs, ema, seg_start, weight);
  CTDET_LAUNCH_CHECK();
  return 0;
}

int launch_ema_swap_segments(float* const* live_ptrs, float* ema, const long* seg_start, int nseg, long max_len,
                             hipStream_t s) {
  if (nseg == 0 || max_len == 0) return 0;
  hipLaunchKernelGGL(ema_swap_segments_kernel, ema_grid(nseg, max_len), dim3(256), 0, s, live_ptrs, ema, seg_start);
  CTDET_LAUNCH_CHECK();
  return 0;
}
