// The ordering stage that voceval.hip (libctdet_voceval.so) and lviseval.hip (libctdet_lviseval.so) share, written once: what is
// identical in both or differs by a value passed in (DESIGN.md 7.17.1 lists it).  Their key kernels, matchers and AP /
// accumulate passes are different algorithms and stay in the two files.  The two kernels here, eval_clear_kernel and
// eval_offsets_kernel<Key>, are the exception to "all __global__ kernels stay in the scorers' files": they are the same kernel
// in every scorer.  cocoeval.hip does not include this header: it is part of the hot-path library, whose binary stays as it is
// (DESIGN.md 7.7).  Nothing here depends on the scorers' floating point contraction setting.
#pragma once
#include "common.h"
#include <rocprim/device/device_radix_sort.hpp>

// ---- status bits of a detection that takes no part: the public CTDET_*_BAD_* of each scorer equal these
enum { EVAL_BAD_CLASS = 1, EVAL_BAD_IMAGE = 2, EVAL_BAD_SCORE = 4, EVAL_BAD_BOX = 8 };

// the detection side of a match call: N detections over I images x K classes
struct EvalDets { const float* boxes; const float* scores; const int* classes; const int* image; long N; int I, K; };

// ---- host: workspace blocks are multiples of 256 bytes from a 256-byte aligned base
static inline size_t eval_up(size_t v) { return (v + 255) & ~(size_t)255; }
// radix bits that hold every value in [0, v]
static inline int eval_bits(unsigned long v) { int b = 1; while ((v >> b) && b < 32) ++b; return b; }
#define EVAL_CHECK_WORKSPACE(what, ws) CTDET_CHECK(((uintptr_t)(ws) & 255) == 0, what ": workspace must be 256-byte aligned")

// a workspace being laid out: take() appends a block of n elements; `p` is the byte count so far (base 0: sizes only)
struct EvalLayout {
  uintptr_t base;
  size_t p;
  template <typename T> T* take(size_t n) {
    T* at = (T*)(base + p);
    p += eval_up(n * sizeof(T));
    return at;
  }
};

// the ordering stage's blocks: score / {group | score} keys u64 [N] x 2, values / order S u32 [N] x 2, group keys u32 [N] x 2,
// cell order u32 [N], cell offsets i32 [ncell + 2]
struct EvalOrderWs {
  uint64_t *keys64, *keys64_sorted;
  uint32_t *vals, *order_s, *keys32, *keys32_sorted, *cell_order;
  int* dt_off;
};
static inline EvalOrderWs eval_order_layout(EvalLayout& l, long N, long ncell) {
  EvalOrderWs w;
  w.keys64 = l.take<uint64_t>(N); w.keys64_sorted = l.take<uint64_t>(N);
  w.vals = l.take<uint32_t>(N); w.order_s = l.take<uint32_t>(N);
  w.keys32 = l.take<uint32_t>(N); w.keys32_sorted = l.take<uint32_t>(N);
  w.cell_order = l.take<uint32_t>(N);
  w.dt_off = l.take<int>(ncell + 2);
  return w;
}

// "<entry>: null pointer <name>"; the _IF form only where the count n says the array is read
#define EVAL_CHECK_PTR(what, p) CTDET_CHECK(p, "%s: null pointer " #p, what)
#define EVAL_CHECK_PTR_IF(what, n, p) CTDET_CHECK((n) <= 0 || (p), "%s: null pointer " #p, what)
// the pointers both match calls take
static inline int eval_check_match_ptrs(const char* what, int64_t N, int64_t NG, const void* boxes, const void* scores,
                                        const void* classes, const void* image, const void* gt_boxes, const void* gt_off,
                                        const void* workspace, const void* order, const void* cls_off, const void* flags,
                                        const void* status) {
  EVAL_CHECK_PTR(what, gt_off);
  EVAL_CHECK_PTR(what, workspace);
  EVAL_CHECK_PTR(what, cls_off);
  EVAL_CHECK_PTR(what, status);
  EVAL_CHECK_PTR_IF(what, NG, gt_boxes);
  EVAL_CHECK_PTR_IF(what, N, boxes);
  EVAL_CHECK_PTR_IF(what, N, scores);
  EVAL_CHECK_PTR_IF(what, N, classes);
  EVAL_CHECK_PTR_IF(what, N, image);
  EVAL_CHECK_PTR_IF(what, N, order);
  EVAL_CHECK_PTR_IF(what, N, flags);
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
__device__ __forceinline__ int eval_invalid(const EvalDets& d, long i) {
  const int c = d.classes[i], im = d.image[i];
  int st = 0;
  if (c < 0 || c >= d.K) st |= EVAL_BAD_CLASS;
  if (im < 0 || im >= d.I) st |= EVAL_BAD_IMAGE;
  if (!isfinite(d.scores[i])) st |= EVAL_BAD_SCORE;
  const float* b = d.boxes + i * 4;
  if (!(isfinite(b[0]) && isfinite(b[1]) && isfinite(b[2]) && isfinite(b[3]))) st |= EVAL_BAD_BOX;
  return st;
}

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

// n counters and the status word
__global__ void __launch_bounds__(256) eval_clear_kernel(int* __restrict__ counts, int n, int* __restrict__ status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) counts[i] = 0;
  if (i == 0) status[0] = 0;
}

// the group of a sorted key lies above its score: above bit 32 of a 64-bit {group | score} key; a 32-bit key is its group
template <typename Key> constexpr int EVAL_GROUP_SHIFT = 8 * (int)(sizeof(Key) - sizeof(uint32_t));

// off[c] = first position of the N sorted keys whose group is >= c (N when there is none), c in [0, n]
template <typename Key>
__global__ void __launch_bounds__(256) eval_offsets_kernel(const Key* __restrict__ keys, long N, int n, int* __restrict__ off) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c > n) return;
  long lo = 0, hi = N;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if ((long)(keys[mid] >> EVAL_GROUP_SHIFT<Key>) < c) lo = mid + 1;
    else hi = mid;
  }
  off[c] = (int)lo;
}

// ---- host: the sorts of one scorer (`who`) over its N detections; `tmp` is the `have` bytes of the sort block
struct EvalSorter {
  const char* who;
  long N;
  void* tmp;
  size_t have;

  // stable sort of the (key, value) pairs by the low `bits` bits of the key
  template <typename Key> int sort(const Key* kin, Key* kout, const uint32_t* vin, uint32_t* vout, int bits, hipStream_t s) const {
    size_t need = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, need, kin, kout, vin, vout, (size_t)N, 0u, (unsigned)bits, s);
    CTDET_CHECK(e == hipSuccess, "%s: sort size query failed: %s", who, hipGetErrorString(e));
    CTDET_CHECK(need <= have, "%s: the sort needs %zu bytes of temporary storage, the workspace formula provides %zu", who,
                need, have);
    e = rocprim::radix_sort_pairs(tmp, need, kin, kout, vin, vout, (size_t)N, 0u, (unsigned)bits, s);
    CTDET_CHECK(e == hipSuccess, "%s: sort failed: %s", who, hipGetErrorString(e));
    return 0;
  }

  // one order: the pairs sorted by group in [0, n] (and by the score below it in a 64-bit key) when there are any, then
  // off[0 .. n] cut from the sorted keys -- all 0 when N == 0, where the keys are not read
  template <typename Key>
  int sort_cut(const Key* kin, Key* kout, const uint32_t* vin, uint32_t* vout, int n, int* off, hipStream_t s) const {
    if (N)
      if (const int rc = sort(kin, kout, vin, vout, EVAL_GROUP_SHIFT<Key> + eval_bits((unsigned long)n), s)) return rc;
    hipLaunchKernelGGL(eval_offsets_kernel<Key>, dim3((n + 1 + 255) / 256), dim3(256), 0, s, (const Key*)kout, N, n, off);
    return 0;
  }
};
// the block that ends every layout: the sort's own temporary storage (bounded here, checked against rocprim's answer above)
static inline EvalSorter eval_sort_layout(EvalLayout& l, const char* who, long N) {
  const size_t at = l.p;
  void* tmp = l.take<char>((size_t)N * 16 + ((size_t)16 << 20));
  return {who, N, tmp, l.p - at};
}

// ---- device: a class's segment of the total order walked in NT-element chunks
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

// the start of a chunk, for the thread at position j of a segment that ends at s1: the flag of the detection there (column
// `col` of the [N][ncol] flags; 1 = true positive, fp_flag = false positive), the packed scan, and the running totals ctp / cfp
// moved past the chunk.  -> whether the position is a true positive, and the true / false positives up to and including it
struct EvalPos { uint32_t tp; int itp, ifp; };
template <int NT>
__device__ __forceinline__ EvalPos eval_chunk(const int* __restrict__ order, const uint8_t* __restrict__ flags, int ncol, int col,
                                              uint32_t fp_flag, int j, int s1, uint32_t* wsum, int& ctp, int& cfp) {
  uint32_t tp = 0, fp = 0;
  if (j < s1) {
    const uint32_t f = flags[(long)order[j] * ncol + col];
    tp = f == 1; fp = f == fp_flag;
  }
  uint32_t tot;
  const uint32_t sc = eval_scan_packed<NT>(tp | (fp << 16), wsum, tot);     // two 16-bit counters
  const EvalPos at = {tp, ctp + (int)(sc & 0xFFFFu), cfp + (int)(sc >> 16)};
  ctp += (int)(tot & 0xFFFFu); cfp += (int)(tot >> 16);
  return at;
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
