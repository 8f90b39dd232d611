// Per-step training metrics without a host synchronisation.
//
// metric_push_kernel: ONE WAVE per step, launched on the step's stream behind the step (an eager step's fresh loss tensors and
// a captured step's fixed ones alike: the K source pointers travel BY VALUE in the kernel arguments).  It copies the K f32
// scalars the pointers name into row `iteration & (ring_rows - 1)` of a device ring:
//
//     row[0]         the iteration number (int32 bits): the tag by which the reader tells an overwritten or unwritten row
//     row[1 .. K]    the K scalars, moved as 32-bit words -- no arithmetic touches them, a NaN keeps its payload
//     row[K + 1]     one f32 the host supplied (the step's data time)
//     row[K + 2 ..]  not written
//
// and keeps one device word, "the first iteration at which one of the K scalars was not finite": an atomic minimum over the
// iteration number (the word starts at INT32_MAX), so the order of the pushes does not matter.  Plain vector stores; the only
// atomic is that integer minimum, issued by one lane and only for a non-finite row.
//
// Built as a small library of its own, libctdet_metrics.so (csrc/Makefile), which the training loop loads when it first builds
// a metric ring: the hot-path library's binary is not touched by it.  Error text and kernel labels go through the plumbing of
// libctdet_hip.so (ctdet_set_error / ctdet_last_error, CTDET_KERNEL), against which this library links.
#include "common.h"
#include "../../include/ctdet_metrics.h"

#define MP_MAX CTDET_METRIC_MAX_SCALARS

struct MetricArgs {
  const float* src[MP_MAX];
  int K;
  float host_scalar;
  float* row;           // the iteration's row of the ring
  int* first_bad;
  int iteration;
};

__global__ void __launch_bounds__(64) metric_push_kernel(MetricArgs a) {
  const int lane = threadIdx.x;
  uint32_t* row = (uint32_t*)a.row;
  const float* p = nullptr;
#pragma unroll
  for (int j = 0; j < MP_MAX; ++j)
    if (lane == j) p = a.src[j];         // selects, not an indexed read of the argument block
  bool bad = false;
  if (lane < a.K) {
    const uint32_t v = *(const uint32_t*)p;
    bad = (v & 0x7F800000u) == 0x7F800000u;      // exponent all ones: inf or NaN
    row[1 + lane] = v;
  }
  if (lane == a.K) row[1 + a.K] = __float_as_uint(a.host_scalar);
  if (lane == a.K + 1) row[0] = (uint32_t)a.iteration;
  const unsigned long long any_bad = __ballot(bad);
  if (any_bad && lane == 0) atomicMin(a.first_bad, a.iteration);
}

static int launch_metric_push(const float* const* ptrs, int K, float host_scalar, float* ring, int ring_rows, int row_floats,
                              int* first_bad, int iteration, hipStream_t s) {
  CTDET_KERNEL("metric_push_kernel");
  MetricArgs a = {};
  for (int j = 0; j < K; ++j) a.src[j] = ptrs[j];
  a.K = K; a.host_scalar = host_scalar; a.first_bad = first_bad; a.iteration = iteration;
  a.row = ring + (long)(iteration & (ring_rows - 1)) * row_floats;
  hipLaunchKernelGGL(metric_push_kernel, dim3(1), dim3(64), 0, s, a);
  CTDET_LAUNCH_CHECK();
  return 0;
}

extern "C" int32_t ctdet_metric_push(const float* const* ptrs, int32_t K, float host_scalar, float* ring, int32_t ring_rows,
                                     int32_t row_floats, int32_t* first_bad, int64_t iteration, void* stream) {
  CTDET_CHECK(K >= 1 && K <= CTDET_METRIC_MAX_SCALARS, "metric_push: K=%d scalars (1..%d)", K, CTDET_METRIC_MAX_SCALARS);
  CTDET_CHECK(ptrs && ring && first_bad, "metric_push: null pointer (ptrs, ring or first_bad)");
  for (int i = 0; i < K; ++i) CTDET_CHECK(ptrs[i], "metric_push: null pointer for scalar %d", i);
  CTDET_CHECK(ring_rows >= 1 && (ring_rows & (ring_rows - 1)) == 0, "metric_push: ring_rows=%d is not a power of two", ring_rows);
  CTDET_CHECK(row_floats >= K + 2, "metric_push: row_floats=%d holds fewer than K + 2 = %d floats", row_floats, K + 2);
  CTDET_CHECK(iteration >= 0 && iteration < (1LL << 31), "metric_push: iteration %lld outside [0, 2^31)", (long long)iteration);
  return launch_metric_push(ptrs, K, host_scalar, ring, ring_rows, row_floats, first_bad, (int)iteration, (hipStream_t)stream);
}
