// Pascal VOC box-AP scoring on the device: the matching and the two AP forms (11-point for VOC2007, area for VOC2012) of the
// reference's `voc_eval` (detectron2/evaluation/pascal_voc_evaluation.py:154-299), over the detections of a whole dataset,
// which are in device memory already when the evaluator sees them.  The rule that is reproduced is written out in DESIGN.md
// 7.16; what matters here:
//
//   * the reference's text round trip ("{score:.3f} {x:.1f}") is done in f64: rint(v * 1000) / 1000 and rint(c * 10) / 10,
//     round-half-even, exact products for an f32 operand.  A score only ever decides the order, and v -> rint(v * 1000) is
//     strictly monotone in the quantised score, so the key of the order is that integer-valued double; the quotient is never
//     formed for a score.  This file is compiled with floating point contraction OFF (FLAGS_voceval in the Makefile): the
//     union `(da + ga) - inter` must round twice, as numpy's does.
//   * one total order: class ascending, quantised score descending, input index ascending.  It is three stable rocprim radix
//     sorts: by the 64-bit score key (order S), then from S by class (the total order) and from S by (image, class) cell.
//     A detection whose class or image index is out of range, or whose score or box is not finite, raises a bit of the
//     status word and is sorted behind everything: no kernel looks at it.
//   * match: ONE WAVE per (image, class) cell.  The cell's detections are serial; for each, the 64 lanes stride over the cell's
//     ground truths and reduce (largest overlap, lowest index) over the wave; lane t < T then decides threshold t against
//     bit t of the ground truth's "taken" word, and lane 0 ORs the wave's ballot of true positives into that word.  The taken
//     words are in LDS while the cell has at most VE_LDS_TAKEN ground truths, else in the caller's workspace (flat pointer).
//   * AP: one workgroup per (class, threshold) walks the class's segment of the total order in 256-element chunks, twice.
//     Pass 1 carries tp / fp, writes rec / prec when asked, keeps the eleven running maxima of the 11-point form and leaves
//     every chunk's largest precision in the workspace.  A suffix maximum over those chunk values and a second forward pass
//     give the envelope at every true positive -- the only positions where recall changes -- and the area sum is taken by one
//     thread in position order.
//   * built as a library of its own, libctdet_voceval.so (csrc/Makefile), which the evaluator loads when it first scores: the
//     hot-path library does not grow by it.  Error text and kernel labels go through the plumbing of libctdet_hip.so
//     (ctdet_set_error / ctdet_last_error, CTDET_KERNEL), against which this library links.
//   * the only atomics are integer (non-difficult ground truths per class, the status bits): two runs are bit-identical.
//   * eval_common.h holds the scaffolding a box-AP scorer needs whatever its rule: the score key, the lower bound that cuts
//     the sorted keys into segments, the packed workgroup scan, the in-LDS suffix maximum, the rocprim sort call, the
//     workspace rounding and the common range checks.  The matcher and the AP passes are this scorer's own.  cocoeval.hip
//     still carries its own copies of those pieces: it is part of the hot-path library, whose binary stays as it is.
#include "eval_common.h"
#include "../../include/ctdet_voceval.h"
#include <float.h>
#include <limits.h>

#define VE_LDS_TAKEN 128        // "taken" words (one u32 per ground truth) a cell keeps in LDS; a VOC cell has a few
#define VE_NT 256               // AP workgroup = chunk of the class segment
#define VE_POINTS 11            // recall points of the VOC2007 form

struct VeMatchArgs {
  const float* boxes; const float* scores; const int* classes; const int* image; long N;
  const double* gt_boxes; const uint8_t* gt_difficult; const int* gt_off; int I, K;
  const double* thrs; int T;
  uint64_t* keys64; uint32_t* vals; const uint32_t* order_s; uint32_t* keys32;
  const uint32_t* cell_order; int* dt_off; uint32_t* taken;
  uint8_t* flags; int* npos; int* status;
};

// status bits of a detection that takes no part (0: it does)
__device__ __forceinline__ int ve_invalid(const VeMatchArgs& a, long i) {
  const int c = a.classes[i], im = a.image[i];
  int st = 0;
  if (c < 0 || c >= a.K) st |= CTDET_VOC_BAD_CLASS;
  if (im < 0 || im >= a.I) st |= CTDET_VOC_BAD_IMAGE;
  if (!isfinite(a.scores[i])) st |= CTDET_VOC_BAD_SCORE;
  const float* b = a.boxes + i * 4;
  if (!(isfinite(b[0]) && isfinite(b[1]) && isfinite(b[2]) && isfinite(b[3]))) st |= CTDET_VOC_BAD_BOX;
  return st;
}

__global__ void __launch_bounds__(256) ve_clear_kernel(int* __restrict__ npos, int n, int* __restrict__ status) {
  eval_clear(npos, n, status);
}

// order-S keys: ascending key = descending rint(score * 1000); equal quantised scores (-0 == +0 included) give equal keys
__global__ void __launch_bounds__(256) ve_key_score_kernel(VeMatchArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  const int st = ve_invalid(a, i);
  if (st) atomicOr(a.status, st);
  a.keys64[i] = eval_score_key(rint((double)a.scores[i] * 1000.0));
  a.vals[i] = (uint32_t)i;
}

// keys of the two orders taken from S: the class (by_cell == 0) or the (image, class) cell of the detection at position p of S;
// a detection that takes no part gets the key behind the last one
__global__ void __launch_bounds__(256) ve_key_group_kernel(VeMatchArgs a, int by_cell) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.N) return;
  const long i = a.order_s[p];
  uint32_t key;
  if (ve_invalid(a, i)) key = by_cell ? (uint32_t)a.I * (uint32_t)a.K : (uint32_t)a.K;
  else key = by_cell ? (uint32_t)a.image[i] * (uint32_t)a.K + (uint32_t)a.classes[i] : (uint32_t)a.classes[i];
  a.keys32[p] = key;
}

// off[c] = first position of the sorted keys that is >= c, c in [0, n]
__global__ void __launch_bounds__(256) ve_offsets_kernel(const uint32_t* __restrict__ keys, long N, int n, int* __restrict__ off) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c > n) return;
  off[c] = eval_lower_bound(keys, N, c, [](uint32_t k) { return (long)k; });
}

__global__ void __launch_bounds__(64) ve_match_kernel(VeMatchArgs a) {
  __shared__ uint32_t taken_lds[VE_LDS_TAKEN];
  const int cell = blockIdx.x, lane = threadIdx.x;
  const int g0 = a.gt_off[cell], G = a.gt_off[cell + 1] - g0;
  const int d0 = a.dt_off[cell], D = a.dt_off[cell + 1] - d0;
  if (G == 0 && D == 0) return;
  const double* gb = a.gt_boxes + (long)g0 * 4;
  const uint8_t* gd = a.gt_difficult + g0;
  {   // non-difficult ground truths of the class: an integer sum, order-independent
    int cnt = 0;
    for (int g = lane; g < G; g += 64) cnt += gd[g] == 0;
#pragma unroll
    for (int o = 32; o; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0 && cnt) atomicAdd(&a.npos[cell % a.K], cnt);
  }
  if (D == 0) return;
  uint32_t* taken = G <= VE_LDS_TAKEN ? taken_lds : a.taken + g0;
  for (int g = lane; g < G; g += 64) taken[g] = 0;
  __syncthreads();
  const bool active = lane < a.T;
  const double thr = active ? a.thrs[lane] : 0.0;
  for (int d = 0; d < D; ++d) {
    const long o = a.cell_order[d0 + d];
    // the reference's `xmin += 1` on an f32 scalar, then its "%.1f" round trip
    const float fx1 = a.boxes[o * 4] + 1.0f, fy1 = a.boxes[o * 4 + 1] + 1.0f;
    const double x1 = rint((double)fx1 * 10.0) / 10.0, y1 = rint((double)fy1 * 10.0) / 10.0;
    const double x2 = rint((double)a.boxes[o * 4 + 2] * 10.0) / 10.0, y2 = rint((double)a.boxes[o * 4 + 3] * 10.0) / 10.0;
    const double darea = (x2 - x1 + 1.0) * (y2 - y1 + 1.0);
    double best = -INFINITY;
    int jbest = INT_MAX;
    for (int g = lane; g < G; g += 64) {
      const double gx1 = gb[g * 4L], gy1 = gb[g * 4L + 1], gx2 = gb[g * 4L + 2], gy2 = gb[g * 4L + 3];
      const double iw = fmax(fmin(gx2, x2) - fmax(gx1, x1) + 1.0, 0.0);
      const double ih = fmax(fmin(gy2, y2) - fmax(gy1, y1) + 1.0, 0.0);
      const double inter = iw * ih;
      const double uni = darea + (gx2 - gx1 + 1.0) * (gy2 - gy1 + 1.0) - inter;
      const double ov = inter / uni;
      if (ov > best) { best = ov; jbest = g; }     // ascending g: the first index that attains the maximum; NaN never wins
    }
#pragma unroll
    for (int s = 32; s; s >>= 1) {
      const double ob = __shfl_xor(best, s, 64);
      const int oj = __shfl_xor(jbest, s, 64);
      if (ob > best || (ob == best && oj < jbest)) { best = ob; jbest = oj; }
    }
    // every lane holds (ovmax, jmax); jmax == INT_MAX: no ground truth compared greater than -inf
    const bool have = jbest != INT_MAX;
    const bool difficult = have && gd[jbest] != 0;
    const uint32_t word = have ? taken[jbest] : 0u;
    uint8_t f = 2;
    bool tp = false;
    if (active && have && best > thr) {
      if (difficult) f = 0;
      else if ((word >> lane) & 1u) f = 2;
      else { f = 1; tp = true; }
    }
    const uint32_t newbits = (uint32_t)__ballot(tp);     // lanes >= T vote 0, T <= 32
    if (active) a.flags[o * a.T + lane] = f;
    if (lane == 0 && newbits) taken[jbest] = word | newbits;
    __syncthreads();     // the word is read by every lane of the next detection
  }
}

struct VeApArgs {
  const int* order; const int* cls_off; const uint8_t* flags; const int* npos; long N; int K, T;
  const double* points; double* chunk; long chunk_stride;
  double* ap07; double* ap12; double* rec; double* prec;
};

__global__ void __launch_bounds__(VE_NT) ve_ap_kernel(VeApArgs a) {
  __shared__ double sm[VE_NT];
  __shared__ double pmax[VE_NT / 64][VE_POINTS];
  __shared__ uint32_t wsum[VE_NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int t = blockIdx.x % a.T, k = blockIdx.x / a.T;
  const int s0 = a.cls_off[k], s1 = a.cls_off[k + 1];
  const int np = a.npos[k];
  const double dnp = (double)np;
  // this (class, threshold)'s chunk values: class k's chunks start at s0 / VE_NT + k (every earlier class rounds up once)
  double* cmax = a.chunk + (long)t * a.chunk_stride + s0 / VE_NT + k;
  double pts[VE_POINTS], best[VE_POINTS];
#pragma unroll
  for (int i = 0; i < VE_POINTS; ++i) { pts[i] = a.points[i]; best[i] = 0.0; }
  // ---- pass 1: running counts, rec / prec, the eleven maxima, the largest precision of every chunk
  int ctp = 0, cfp = 0, nchunk = 0;
  for (int base = s0; base < s1; base += VE_NT, ++nchunk) {
    const int j = base + tid;
    uint32_t tp = 0, fp = 0;
    if (j < s1) {
      const uint32_t f = a.flags[(long)a.order[j] * a.T + t];
      tp = f == 1; fp = f == 2;
    }
    uint32_t tot;
    const uint32_t sc = eval_scan_packed<VE_NT>(tp | (fp << 16), wsum, tot);     // two 16-bit counters
    double prec = 0.0;
    if (j < s1) {
      const int itp = ctp + (int)(sc & 0xFFFFu), ifp = cfp + (int)(sc >> 16);
      const double rec = (double)itp / dnp;
      prec = (double)itp / fmax((double)(itp + ifp), DBL_EPSILON);
      if (a.rec) a.rec[(long)t * a.N + j] = rec;
      if (a.prec) a.prec[(long)t * a.N + j] = prec;
#pragma unroll
      for (int i = 0; i < VE_POINTS; ++i)
        if (rec >= pts[i]) best[i] = fmax(best[i], prec);
    }
    double m = prec;     // precision is >= 0: the 0 of an idle thread is neutral
#pragma unroll
    for (int o = 32; o; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    if (lane == 0) sm[wv] = m;
    __syncthreads();
    if (tid == 0) cmax[nchunk] = fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
    ctp += (int)(tot & 0xFFFFu); cfp += (int)(tot >> 16);
  }
  // ---- 11-point AP: the maxima over the workgroup (order-independent), then the reference's ordered sum
#pragma unroll
  for (int i = 0; i < VE_POINTS; ++i) {
    double m = best[i];
#pragma unroll
    for (int o = 32; o; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    if (lane == 0) pmax[wv][i] = m;
  }
  __syncthreads();     // also: cmax[] of pass 1 is written (same thread reads it below)
  if (tid == 0) {
    double ap = 0.0;
    for (int i = 0; i < VE_POINTS; ++i) {
      const double p = fmax(fmax(pmax[0][i], pmax[1][i]), fmax(pmax[2][i], pmax[3][i]));
      ap = ap + p / 11.0;
    }
    a.ap07[(long)k * a.T + t] = ap;
    // chunk values -> largest precision of all LATER chunks (the sentinel 0 behind the last)
    double run = 0.0;
    for (int c = nchunk - 1; c >= 0; --c) {
      const double v = cmax[c];
      cmax[c] = run;
      run = fmax(run, v);
    }
  }
  if (np == 0) {     // rec is 0 / 0 everywhere: numpy's sum over the NaN differences; no detection: the sentinels alone
    if (tid == 0) a.ap12[(long)k * a.T + t] = s1 > s0 ? NAN : 0.0;
    return;
  }
  __threadfence_block();
  __syncthreads();
  // ---- pass 2: envelope (suffix maximum of the precision) at every true positive, area sum in position order
  double ap = 0.0;
  ctp = 0; cfp = 0;
  int c = 0;
  for (int base = s0; base < s1; base += VE_NT, ++c) {
    const int j = base + tid;
    uint32_t tp = 0, fp = 0;
    if (j < s1) {
      const uint32_t f = a.flags[(long)a.order[j] * a.T + t];
      tp = f == 1; fp = f == 2;
    }
    uint32_t tot;
    const uint32_t sc = eval_scan_packed<VE_NT>(tp | (fp << 16), wsum, tot);     // two 16-bit counters
    const int itp = ctp + (int)(sc & 0xFFFFu), ifp = cfp + (int)(sc >> 16);
    eval_suffix_max<VE_NT>(sm, j < s1 ? (double)itp / fmax((double)(itp + ifp), DBL_EPSILON) : 0.0, 0.0);
    const double env = fmax(sm[tid], cmax[c]);
    __syncthreads();
    // recall changes exactly at a true positive: (tp / npos - (tp - 1) / npos) * envelope; 0 elsewhere, which adds nothing
    sm[tid] = tp ? ((double)itp / dnp - (double)(itp - 1) / dnp) * env : 0.0;
    __syncthreads();
    if (tid == 0)
      for (int i = 0; i < VE_NT; ++i) ap = ap + sm[i];
    __syncthreads();
    ctp += (int)(tot & 0xFFFFu); cfp += (int)(tot >> 16);
  }
  if (tid == 0) a.ap12[(long)k * a.T + t] = ap;
}

// ---- workspace: chunk values f64 [T * (N / 256 + K + 1)] (first: the AP call finds them without knowing NG or I), score keys
// u64 [N] x 2, values / order S u32 [N] x 2, group keys u32 [N] x 2, cell order u32 [N], cell offsets i32 [I*K + 2], taken
// words u32 [NG], then the sort block
struct VeWs { size_t chunk, keys64, keys64_sorted, vals, order_s, keys32, keys32_sorted, cell_order, off, taken, sort, total; };
static long ve_chunk_stride(long N, long K) { return N / VE_NT + K + 1; }
static VeWs ve_layout(long N, long NG, long I, long K, long T) {
  VeWs w;
  size_t p = 0;
  w.chunk = p; p += eval_up((size_t)T * (size_t)ve_chunk_stride(N, K) * 8);
  w.keys64 = p; p += eval_up((size_t)N * 8);
  w.keys64_sorted = p; p += eval_up((size_t)N * 8);
  w.vals = p; p += eval_up((size_t)N * 4);
  w.order_s = p; p += eval_up((size_t)N * 4);
  w.keys32 = p; p += eval_up((size_t)N * 4);
  w.keys32_sorted = p; p += eval_up((size_t)N * 4);
  w.cell_order = p; p += eval_up((size_t)N * 4);
  w.off = p; p += eval_up((size_t)(I * K + 2) * 4);
  w.taken = p; p += eval_up((size_t)NG * 4);
  w.sort = p; p += eval_sort_bytes(N);
  w.total = p;
  return w;
}

static int ve_check_dims(const char* what, int64_t N, int64_t NG, int32_t I, int32_t K, int32_t T) {
  if (const int rc = eval_check_dims(what, "classes", N, NG, I, K)) return rc;
  CTDET_CHECK(T >= 1 && T <= 32, "%s: T=%d thresholds (1..32: one bit of a ground truth's taken word each)", what, T);
  return 0;
}

extern "C" {

size_t ctdet_voceval_workspace_bytes(int64_t N, int64_t NG, int32_t I, int32_t K, int32_t T) {
  if (ve_check_dims("voceval_workspace_bytes", N, NG, I, K, T)) return 0;
  return ve_layout(N, NG, I, K, T).total;
}

int32_t ctdet_voceval_match(const float* boxes, const float* scores, const int32_t* classes, const int32_t* image, int64_t N,
                            const double* gt_boxes, const uint8_t* gt_difficult, const int32_t* gt_off, int64_t NG, int32_t I,
                            int32_t K, const double* thrs, int32_t T, void* workspace, int32_t* order, int32_t* cls_off,
                            uint8_t* flags, int32_t* npos, int32_t* status, void* stream) {
  CTDET_CHECK(gt_off, "voceval_match: null pointer gt_off");
  CTDET_CHECK(thrs, "voceval_match: null pointer thrs");
  CTDET_CHECK(workspace, "voceval_match: null pointer workspace");
  CTDET_CHECK(cls_off, "voceval_match: null pointer cls_off");
  CTDET_CHECK(npos, "voceval_match: null pointer npos");
  CTDET_CHECK(status, "voceval_match: null pointer status");
  CTDET_CHECK(NG <= 0 || gt_boxes, "voceval_match: null pointer gt_boxes");
  CTDET_CHECK(NG <= 0 || gt_difficult, "voceval_match: null pointer gt_difficult");
  CTDET_CHECK(N <= 0 || boxes, "voceval_match: null pointer boxes");
  CTDET_CHECK(N <= 0 || scores, "voceval_match: null pointer scores");
  CTDET_CHECK(N <= 0 || classes, "voceval_match: null pointer classes");
  CTDET_CHECK(N <= 0 || image, "voceval_match: null pointer image");
  CTDET_CHECK(N <= 0 || order, "voceval_match: null pointer order");
  CTDET_CHECK(N <= 0 || flags, "voceval_match: null pointer flags");
  const int rc = ve_check_dims("voceval_match", N, NG, I, K, T);
  if (rc) return rc;
  EVAL_CHECK_WORKSPACE("voceval_match", workspace);
  CTDET_KERNEL("ve_match_kernel<wave per cell,%d thresholds>", T);
  hipStream_t s = (hipStream_t)stream;
  const VeWs w = ve_layout(N, NG, I, K, T);
  char* ws = (char*)workspace;
  VeMatchArgs a;
  a.boxes = boxes; a.scores = scores; a.classes = classes; a.image = image; a.N = N;
  a.gt_boxes = gt_boxes; a.gt_difficult = gt_difficult; a.gt_off = gt_off; a.I = I; a.K = K; a.thrs = thrs; a.T = T;
  a.keys64 = (uint64_t*)(ws + w.keys64); a.vals = (uint32_t*)(ws + w.vals); a.order_s = (const uint32_t*)(ws + w.order_s);
  a.keys32 = (uint32_t*)(ws + w.keys32); a.cell_order = (const uint32_t*)(ws + w.cell_order); a.dt_off = (int*)(ws + w.off);
  a.taken = (uint32_t*)(ws + w.taken); a.flags = flags; a.npos = npos; a.status = status;
  const uint32_t* k32s = (const uint32_t*)(ws + w.keys32_sorted);
  const int ncell = I * K;
  const unsigned nb = (unsigned)((N + 255) / 256);
  const auto sort = [&](auto* kin, auto* kout, const uint32_t* vin, uint32_t* vout, int bits) {     // tmp: the sort block
    return eval_sort("voceval", kin, kout, vin, vout, N, bits, ws + w.sort, w.total - w.sort, s);
  };
  hipLaunchKernelGGL(ve_clear_kernel, dim3((K + 255) / 256), dim3(256), 0, s, npos, K, status);
  if (N) {
    hipLaunchKernelGGL(ve_key_score_kernel, dim3(nb), dim3(256), 0, s, a);
    int src = sort(a.keys64, (uint64_t*)(ws + w.keys64_sorted), a.vals, (uint32_t*)(ws + w.order_s), 64);
    if (src) return src;
    hipLaunchKernelGGL(ve_key_group_kernel, dim3(nb), dim3(256), 0, s, a, 0);
    src = sort(a.keys32, (uint32_t*)(ws + w.keys32_sorted), a.order_s, (uint32_t*)order, eval_bits((unsigned long)K));
    if (src) return src;
  }
  hipLaunchKernelGGL(ve_offsets_kernel, dim3((K + 1 + 255) / 256), dim3(256), 0, s, k32s, (long)N, K, cls_off);
  if (N) {
    hipLaunchKernelGGL(ve_key_group_kernel, dim3(nb), dim3(256), 0, s, a, 1);
    const int src = sort(a.keys32, (uint32_t*)(ws + w.keys32_sorted), a.order_s, (uint32_t*)(ws + w.cell_order),
                         eval_bits((unsigned long)ncell));
    if (src) return src;
  }
  hipLaunchKernelGGL(ve_offsets_kernel, dim3((ncell + 1 + 255) / 256), dim3(256), 0, s, k32s, (long)N, ncell, a.dt_off);
  hipLaunchKernelGGL(ve_match_kernel, dim3(ncell), dim3(64), 0, s, a);
  CTDET_LAUNCH_CHECK();
  return 0;
}

int32_t ctdet_voceval_ap(const int32_t* order, const int32_t* cls_off, const uint8_t* flags, const int32_t* npos, int64_t N,
                         int32_t K, int32_t T, const double* points, void* workspace, double* ap07, double* ap12, double* rec,
                         double* prec, void* stream) {
  CTDET_CHECK(cls_off, "voceval_ap: null pointer cls_off");
  CTDET_CHECK(npos, "voceval_ap: null pointer npos");
  CTDET_CHECK(points, "voceval_ap: null pointer points");
  CTDET_CHECK(workspace, "voceval_ap: null pointer workspace");
  CTDET_CHECK(ap07, "voceval_ap: null pointer ap07");
  CTDET_CHECK(ap12, "voceval_ap: null pointer ap12");
  CTDET_CHECK(N <= 0 || order, "voceval_ap: null pointer order");
  CTDET_CHECK(N <= 0 || flags, "voceval_ap: null pointer flags");
  const int rc = ve_check_dims("voceval_ap", N, 0, 1, K, T);
  if (rc) return rc;
  CTDET_CHECK((int64_t)K * T < (1LL << 31), "voceval_ap: K*T too large");
  EVAL_CHECK_WORKSPACE("voceval_ap", workspace);
  CTDET_KERNEL("ve_ap_kernel<workgroup per (k,t),two passes>");
  // the chunk values lead the layout and their size depends on N, K and T alone: the workspace of the match call serves
  VeApArgs a;
  a.order = order; a.cls_off = cls_off; a.flags = flags; a.npos = npos; a.N = N; a.K = K; a.T = T; a.points = points;
  a.chunk_stride = ve_chunk_stride(N, K);
  a.chunk = (double*)((char*)workspace + ve_layout(N, 0, 1, K, T).chunk);
  a.ap07 = ap07; a.ap12 = ap12; a.rec = rec; a.prec = prec;
  hipLaunchKernelGGL(ve_ap_kernel, dim3(K * T), dim3(VE_NT), 0, (hipStream_t)stream, a);
  CTDET_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
