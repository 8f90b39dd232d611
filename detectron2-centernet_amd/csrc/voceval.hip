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
//   * what this scorer has in common with the LVIS one (lviseval.hip) -- the ordering stage around the keys, the checks, the
//     start of a chunk of the AP walk -- is in eval_common.h.  Here are its keys, its matcher, its AP passes and its own
//     workspace blocks (the chunk values, the taken words).
#include "eval_common.h"
#include "../../include/ctdet_voceval.h"
#include <float.h>
#include <limits.h>

static_assert(CTDET_VOC_BAD_CLASS == EVAL_BAD_CLASS && CTDET_VOC_BAD_IMAGE == EVAL_BAD_IMAGE &&
              CTDET_VOC_BAD_SCORE == EVAL_BAD_SCORE && CTDET_VOC_BAD_BOX == EVAL_BAD_BOX, "the public status bits");

#define VE_LDS_TAKEN 128        // "taken" words (one u32 per ground truth) a cell keeps in LDS; a VOC cell has a few
#define VE_NT 256               // AP workgroup = chunk of the class segment
#define VE_POINTS 11            // recall points of the VOC2007 form

struct VeMatchArgs {
  EvalDets d;
  const double* gt_boxes; const uint8_t* gt_difficult; const int* gt_off;
  const double* thrs; int T;
  EvalOrderWs o; uint32_t* taken;
  uint8_t* flags; int* npos; int* status;
};

// order-S keys: ascending key = descending rint(score * 1000); equal quantised scores (-0 == +0 included) give equal keys
__global__ void __launch_bounds__(256) ve_key_score_kernel(VeMatchArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.d.N) return;
  const int st = eval_invalid(a.d, i);
  if (st) atomicOr(a.status, st);
  a.o.keys64[i] = eval_score_key(rint((double)a.d.scores[i] * 1000.0));
  a.o.vals[i] = (uint32_t)i;
}

// keys of the two orders taken from S: the class (by_cell == 0) or the (image, class) cell of the detection at position p of S;
// a detection that takes no part gets the key behind the last one
__global__ void __launch_bounds__(256) ve_key_group_kernel(VeMatchArgs a, int by_cell) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.d.N) return;
  const long i = a.o.order_s[p];
  const uint32_t K = (uint32_t)a.d.K;
  uint32_t key;
  if (eval_invalid(a.d, i)) key = by_cell ? (uint32_t)a.d.I * K : K;
  else key = by_cell ? (uint32_t)a.d.image[i] * K + (uint32_t)a.d.classes[i] : (uint32_t)a.d.classes[i];
  a.o.keys32[p] = key;
}

__global__ void __launch_bounds__(64) ve_match_kernel(VeMatchArgs a) {
  __shared__ uint32_t taken_lds[VE_LDS_TAKEN];
  const int cell = blockIdx.x, lane = threadIdx.x;
  const int g0 = a.gt_off[cell], G = a.gt_off[cell + 1] - g0;
  const int d0 = a.o.dt_off[cell], D = a.o.dt_off[cell + 1] - d0;
  if (G == 0 && D == 0) return;
  const double* gb = a.gt_boxes + (long)g0 * 4;
  const uint8_t* gd = a.gt_difficult + g0;
  {   // non-difficult ground truths of the class: an integer sum, order-independent
    int cnt = 0;
    for (int g = lane; g < G; g += 64) cnt += gd[g] == 0;
#pragma unroll
    for (int o = 32; o; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0 && cnt) atomicAdd(&a.npos[cell % a.d.K], cnt);
  }
  if (D == 0) return;
  uint32_t* taken = G <= VE_LDS_TAKEN ? taken_lds : a.taken + g0;
  for (int g = lane; g < G; g += 64) taken[g] = 0;
  __syncthreads();
  const bool active = lane < a.T;
  const double thr = active ? a.thrs[lane] : 0.0;
  for (int d = 0; d < D; ++d) {
    const long o = a.o.cell_order[d0 + d];
    // the reference's `xmin += 1` on an f32 scalar, then its "%.1f" round trip
    const float fx1 = a.d.boxes[o * 4] + 1.0f, fy1 = a.d.boxes[o * 4 + 1] + 1.0f;
    const double x1 = rint((double)fx1 * 10.0) / 10.0, y1 = rint((double)fy1 * 10.0) / 10.0;
    const double x2 = rint((double)a.d.boxes[o * 4 + 2] * 10.0) / 10.0, y2 = rint((double)a.d.boxes[o * 4 + 3] * 10.0) / 10.0;
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
    const EvalPos at = eval_chunk<VE_NT>(a.order, a.flags, a.T, t, 2, j, s1, wsum, ctp, cfp);     // flag 2: a false positive
    double prec = 0.0;
    if (j < s1) {
      const double rec = (double)at.itp / dnp;
      prec = (double)at.itp / fmax((double)(at.itp + at.ifp), DBL_EPSILON);
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
    const EvalPos at = eval_chunk<VE_NT>(a.order, a.flags, a.T, t, 2, j, s1, wsum, ctp, cfp);
    eval_suffix_max<VE_NT>(sm, j < s1 ? (double)at.itp / fmax((double)(at.itp + at.ifp), DBL_EPSILON) : 0.0, 0.0);
    const double env = fmax(sm[tid], cmax[c]);
    __syncthreads();
    // recall changes exactly at a true positive: (tp / npos - (tp - 1) / npos) * envelope; 0 elsewhere, which adds nothing
    sm[tid] = at.tp ? ((double)at.itp / dnp - (double)(at.itp - 1) / dnp) * env : 0.0;
    __syncthreads();
    if (tid == 0)
      for (int i = 0; i < VE_NT; ++i) ap = ap + sm[i];
    __syncthreads();
  }
  if (tid == 0) a.ap12[(long)k * a.T + t] = ap;
}

// ---- workspace: chunk values f64 [T * (N / 256 + K + 1)] (first: the AP call finds them without knowing NG or I), the ordering
// stage's blocks, taken words u32 [NG], then the sort block.  ws == nullptr: the sizes alone
struct VeWs { double* chunk; EvalOrderWs o; uint32_t* taken; EvalSorter sort; size_t total; };
static long ve_chunk_stride(long N, long K) { return N / VE_NT + K + 1; }
static VeWs ve_layout(void* ws, long N, long NG, long I, long K, long T) {
  EvalLayout l = {(uintptr_t)ws, 0};
  VeWs w;
  w.chunk = l.take<double>((size_t)T * (size_t)ve_chunk_stride(N, K));
  w.o = eval_order_layout(l, N, I * K);
  w.taken = l.take<uint32_t>(NG);
  w.sort = eval_sort_layout(l, "voceval", N);
  w.total = l.p;
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
  return ve_layout(nullptr, N, NG, I, K, T).total;
}

int32_t ctdet_voceval_match(const float* boxes, const float* scores, const int32_t* classes, const int32_t* image, int64_t N,
                            const double* gt_boxes, const uint8_t* gt_difficult, const int32_t* gt_off, int64_t NG, int32_t I,
                            int32_t K, const double* thrs, int32_t T, void* workspace, int32_t* order, int32_t* cls_off,
                            uint8_t* flags, int32_t* npos, int32_t* status, void* stream) {
  const char* what = "voceval_match";
  if (const int rc = eval_check_match_ptrs(what, N, NG, boxes, scores, classes, image, gt_boxes, gt_off, workspace, order,
                                           cls_off, flags, status))
    return rc;
  EVAL_CHECK_PTR(what, thrs);
  EVAL_CHECK_PTR(what, npos);
  EVAL_CHECK_PTR_IF(what, NG, gt_difficult);
  if (const int rc = ve_check_dims(what, N, NG, I, K, T)) return rc;
  EVAL_CHECK_WORKSPACE("voceval_match", workspace);
  CTDET_KERNEL("ve_match_kernel<wave per cell,%d thresholds>", T);
  hipStream_t s = (hipStream_t)stream;
  const VeWs w = ve_layout(workspace, N, NG, I, K, T);
  const VeMatchArgs a = {{boxes, scores, classes, image, N, I, K}, gt_boxes, gt_difficult, gt_off, thrs, T, w.o, w.taken,
                         flags, npos, status};
  const int ncell = I * K;
  const dim3 nb((unsigned)((N + 255) / 256)), nt(256);
  hipLaunchKernelGGL(eval_clear_kernel, dim3((K + 255) / 256), nt, 0, s, npos, K, status);
  if (N) {
    hipLaunchKernelGGL(ve_key_score_kernel, nb, nt, 0, s, a);
    if (const int rc = w.sort.sort(w.o.keys64, w.o.keys64_sorted, w.o.vals, w.o.order_s, 64, s)) return rc;
    hipLaunchKernelGGL(ve_key_group_kernel, nb, nt, 0, s, a, 0);
  }
  if (const int rc = w.sort.sort_cut(w.o.keys32, w.o.keys32_sorted, w.o.order_s, (uint32_t*)order, K, cls_off, s)) return rc;
  if (N) hipLaunchKernelGGL(ve_key_group_kernel, nb, nt, 0, s, a, 1);
  if (const int rc = w.sort.sort_cut(w.o.keys32, w.o.keys32_sorted, w.o.order_s, w.o.cell_order, ncell, w.o.dt_off, s)) return rc;
  hipLaunchKernelGGL(ve_match_kernel, dim3(ncell), dim3(64), 0, s, a);
  CTDET_LAUNCH_CHECK();
  return 0;
}

int32_t ctdet_voceval_ap(const int32_t* order, const int32_t* cls_off, const uint8_t* flags, const int32_t* npos, int64_t N,
                         int32_t K, int32_t T, const double* points, void* workspace, double* ap07, double* ap12, double* rec,
                         double* prec, void* stream) {
  const char* what = "voceval_ap";
  EVAL_CHECK_PTR(what, cls_off);
  EVAL_CHECK_PTR(what, npos);
  EVAL_CHECK_PTR(what, points);
  EVAL_CHECK_PTR(what, workspace);
  EVAL_CHECK_PTR(what, ap07);
  EVAL_CHECK_PTR(what, ap12);
  EVAL_CHECK_PTR_IF(what, N, order);
  EVAL_CHECK_PTR_IF(what, N, flags);
  if (const int rc = ve_check_dims(what, N, 0, 1, K, T)) return rc;
  CTDET_CHECK((int64_t)K * T < (1LL << 31), "voceval_ap: K*T too large");
  EVAL_CHECK_WORKSPACE("voceval_ap", workspace);
  CTDET_KERNEL("ve_ap_kernel<workgroup per (k,t),two passes>");
  // the chunk values lead the layout and their size depends on N, K and T alone: the workspace of the match call serves
  const VeApArgs a = {order, cls_off, flags, npos, N, K, T, points, ve_layout(workspace, N, 0, 1, K, T).chunk,
                      ve_chunk_stride(N, K), ap07, ap12, rec, prec};
  hipLaunchKernelGGL(ve_ap_kernel, dim3(K * T), dim3(VE_NT), 0, (hipStream_t)stream, a);
  CTDET_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
