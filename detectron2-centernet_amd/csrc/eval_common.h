// What a box-AP scorer needs whatever its rule: the COCO scorer (cocoeval.hip) and the VOC scorer (voceval.hip) both sort the
// detections by a {group | score} key with rocprim, cut the sorted keys into segments, and walk a segment in workgroup-sized
// chunks with a packed scan and a suffix maximum.  Their matchers and their accumulate / AP passes are different algorithms
// and stay in the two files, as do all __global__ kernels.  voceval.hip (libctdet_voceval.so) includes this header;
// cocoeval.hip keeps its own copies of these pieces as long as a change of the hot-path library's binary is to be avoided
// (DESIGN.md 7.7).  Everything here inlines into its caller; the scorers are compiled with floating point contraction off,
// and nothing here depends on that setting either way.
#pragma once
#include "common.h"
#include <rocprim/device/device_radix_sort.hpp>

// ---- host: workspace blocks are multiples of 256 bytes from a 256-byte aligned base
static inline size_t eval_up(size_t v) { return (v + 255) & ~(size_t)255; }
// radix bits that hold every value in [0, v]
static inline int eval_bits(unsigned long v) { int b = 1; while ((v >> b) && b < 32) ++b; return b; }
// the block that ends both layouts: the sort's own temporary storage (bounded here, checked against rocprim's answer below)
static inline size_t eval_sort_bytes(long N) { return eval_up((size_t)N * 16 + ((size_t)16 << 20)); }
#define EVAL_CHECK_WORKSPACE(what, ws) CTDET_CHECK(((uintptr_t)(ws) & 255) == 0, what ": workspace must be 256-byte aligned")

// stable sort of (key, value) pairs by the low `bits` bits of the key; `tmp` is the `have` bytes of the sort block
template <typename Key>
static inline int eval_sort(const char* who, const Key* kin, Key* kout, const uint32_t* vin, uint32_t* vout, long N, int bits,
                            void* tmp, size_t have, hipStream_t s) {
  size_t need = 0;
  hipError_t e = rocprim::radix_sort_pairs(nullptr, need, kin, kout, vin, vout, (size_t)N, 0u, (unsigned)bits, s);
  CTDET_CHECK(e == hipSuccess, "%s: sort size query failed: %s", who, hipGetErrorString(e));
  CTDET_CHECK(need <= have, "%s: the sort needs %zu bytes of temporary storage, the workspace formula provides %zu", who, need,
              have);
  e = rocprim::radix_sort_pairs(tmp, need, kin, kout, vin, vout, (size_t)N, 0u, (unsigned)bits, s);
  CTDET_CHECK(e == hipSuccess, "%s: sort failed: %s", who, hipGetErrorString(e));
  return 0;
}

// N detections, NG ground truths, I images x K `groups` ("categories" / "classes"): the ranges every entry point checks first
static inline int eval_check_dims(const char* what, const char* groups, int64_t N, int64_t NG, int32_t I, int32_t K) {
  CTDET_CHECK(N >= 0 && N < (1LL << 31) - 1024, "%s: N=%lld out of range", what, (long long)N);
  CTDET_CHECK(NG >= 0 && NG < (1LL << 31), "%s: %lld ground truths out of range", what, (long long)NG);
  // one 64-thread workgroup per cell: a grid holds fewer than 2^32 threads
  CTDET_CHECK(I >= 1 && K >= 1 && (int64_t)I * K < (1LL << 26), "%s: I=%d images x K=%d %s out of range (I*K < 2^26)", what, I, K,
              groups);
  return 0;
}

// ---- device
// ascending order of the key = descending order of the score; equal scores (-0 == +0 included) give equal keys
__device__ __forceinline__ uint32_t eval_score_key(float s) {
  uint32_t u = __float_as_uint(s + 0.0f);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~u;
}
__device__ __forceinline__ uint64_t eval_score_key(double s) {
  uint64_t u = (uint64_t)__double_as_longlong(s + 0.0);
  u = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
  return ~u;
}

// body of the 256-thread clear kernels: n counters and the status word
__device__ __forceinline__ void eval_clear(int* __restrict__ counts, int n, int* __restrict__ status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) counts[i] = 0;
  if (i == 0) status[0] = 0;
}

// first position of the N sorted keys whose projection is >= c (N when there is none)
template <typename Key, typename Proj>
__device__ __forceinline__ int eval_lower_bound(const Key* __restrict__ keys, long N, long c, Proj proj) {
  long lo = 0, hi = N;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (proj(keys[mid]) < c) lo = mid + 1;
    else hi = mid;
  }
  return (int)lo;
}

// inclusive scan over the NT-thread workgroup of counters <= NT that the caller packed into one word (no field may carry
// into the next: NT = 256 allows three 10-bit or two 16-bit fields); `tot` = the workgroup's sum; wsum: NT / 64 words of LDS
template <int NT>
__device__ __forceinline__ uint32_t eval_scan_packed(uint32_t v, uint32_t* wsum, uint32_t& tot) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  __syncthreads();     // the previous round's readers of wsum are done
  if (lane == 63) wsum[wv] = v;
  __syncthreads();
  tot = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const uint32_t s = wsum[w];
    tot += s;
    if (w < wv) v += s;
  }
  return v;
}

// sm[tid] = max(v of threads tid .. NT-1), `neutral` standing behind the last; every thread of the workgroup calls it, and
// sm is visible to all of them on return
template <int NT>
__device__ __forceinline__ void eval_suffix_max(double* sm, double v, double neutral) {
  const int tid = threadIdx.x;
  sm[tid] = v;
  __syncthreads();
  for (int o = 1; o < NT; o <<= 1) {
    const double u = tid + o < NT ? sm[tid + o] : neutral;
    __syncthreads();
    sm[tid] = fmax(sm[tid], u);
    __syncthreads();
  }
}
