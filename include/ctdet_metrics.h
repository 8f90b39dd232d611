/* ctdet_metrics.h -- C ABI of libctdet_metrics.so: the per-step metric push of the training loop.
 * A companion of libctdet_hip.so (ctdet_hip.h, ABI 8, unchanged by it): same conventions -- plain C types, caller-owned
 * buffers, 0 or a negative errno, the message through ctdet_last_error() of libctdet_hip.so, nothing synchronises.
 *
 * ctdet_metric_push: one launch of one wave, on `stream`, behind a training step.  The K f32 scalars that the DEVICE pointers
 * ptrs[0..K) name (`ptrs` itself is a HOST array; the pointers are copied into the kernel arguments, so an eager step's
 * fresh loss tensors and a captured step's fixed ones are served alike, and the array may be freed when the call returns) are
 * copied into row `iteration % ring_rows` of `ring` (f32 [ring_rows][row_floats], device):
 *   row[0] = iteration (int32 bits), row[1..K] = the scalars, bit for bit (no arithmetic: a NaN keeps its payload),
 *   row[K+1] = host_scalar; floats beyond K + 2 are not written.
 * `first_bad` (int32, device; the caller starts it at CTDET_METRIC_NO_BAD_ITERATION) receives, by an integer atomic minimum,
 * the smallest iteration at which one of the K scalars was inf or NaN.  A row is complete once the stream has passed the launch.
 * -EINVAL: K < 1, K > CTDET_METRIC_MAX_SCALARS, a null pointer (ptrs, any ptrs[i], ring, first_bad), ring_rows not a power of
 * two (>= 1), row_floats < K + 2, iteration < 0 or >= 2^31. */
#ifndef CTDET_METRICS_H
#define CTDET_METRICS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CTDET_METRIC_MAX_SCALARS 8
#define CTDET_METRIC_NO_BAD_ITERATION 0x7FFFFFFF
int32_t ctdet_metric_push(const float* const* ptrs, int32_t K, float host_scalar, float* ring, int32_t ring_rows,
                          int32_t row_floats, int32_t* first_bad, int64_t iteration, void* stream);

#ifdef __cplusplus
}
#endif
#endif
