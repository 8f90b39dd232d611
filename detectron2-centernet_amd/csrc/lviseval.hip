// LVIS box-AP scoring on the device: the federated rule of LVIS (DESIGN.md 7.17 writes it out) over the detections of a whole
// dataset, which are in device memory already when the evaluator sees them.  What matters here:
//
//   * every value is f64 and either a ratio of integers or an IoU.  This file is compiled with floating point contraction OFF
//     (FLAGS_lviseval in the Makefile): `da + ga - inter` must round twice and `(fp + tp) + 2^-52` must stay a sum, as numpy's.
//   * order S: image ascending, score descending, input index ascending -- one stable rocprim radix sort of {image | score}.
//     The position of a detection within its image's segment of S is its rank: an image keeps the max_det first (the
//     per-image cut, ties to the lower input index).  A detection that is cut, whose class is neither positive nor negative in
//     its image (the drop), or that is invalid (index out of range, score or box not finite: a bit of the status word) takes
//     no part: in both orders below it gets the key behind the last one and no kernel looks at it.
//   * from S, two more stable sorts: by {class | score} (the total order of the accumulate pass: class, score descending,
//     image ascending, input index) and by the (image, class) cell (within a cell: score descending, input index).
//   * match: ONE WAVE per (image, class) cell.  The A*T (area range, IoU threshold) greedy matchers of a cell are independent
//     and serial over the cell's detections x G ground truths: matcher (a, t) is lane a*T + t.  All lanes look at the same
//     (detection, ground truth) pair at a time, so box reads are wave-uniform; a lane's "taken" flags are a column of a
//     [G][A*T] byte table -- in LDS while the cell has at most LE_LDS_GT ground truths, else in the caller's workspace (flat
//     pointer, same code).
//   * accumulate: one workgroup per (class, area range, threshold) walks the class's segment of the total order in
//     256-element chunks, twice.  Pass 1 carries tp / fp (packed scan of eval_common.h) and, recall being non-decreasing,
//     records for every recall threshold the first position that reaches it (LDS).  Pass 2 recomputes the precision of every
//     position and folds the per-chunk suffix maximum (eval_common.h) into the recorded positions' envelope values.
//   * built as a library of its own, libctdet_lviseval.so (csrc/Makefile), which the evaluator loads when it first scores: the
//     hot-path library does not grow by it.  Error text and kernel labels go through the plumbing of libctdet_hip.so.
//   * the only atomics are integer (non-ignored ground truths per (class, area range), the status bits): two runs are
//     bit-identical.
//   * what this scorer has in common with the VOC one (voceval.hip) -- the ordering stage around the keys, the checks, the
//     start of a chunk of the accumulate walk -- is in eval_common.h.  Here are its keys (le_cell: the cut and the drop), its
//     matcher with le_iou, its accumulate passes and its own workspace blocks (the image offsets, the taken table).
#include "eval_common.h"
#include "../../include/ctdet_lviseval.h"

#define LE_LDS_GT 128           // ground truths of a cell whose taken flags (one byte per matcher, <= 64 matchers) stay in LDS
#define LE_NT 256               // accumulate workgroup = chunk of the class segment

static_assert(CTDET_LVIS_BAD_CLASS == EVAL_BAD_CLASS && CTDET_LVIS_BAD_IMAGE == EVAL_BAD_IMAGE &&
              CTDET_LVIS_BAD_SCORE == EVAL_BAD_SCORE && CTDET_LVIS_BAD_BOX == EVAL_BAD_BOX, "the public status bits");

struct LeMatchArgs {
  EvalDets d;
  const double* gt_boxes; const double* gt_area; const uint8_t* gt_ignore; const int* gt_off; const uint8_t* lists;
  const double* iou_thrs; int T; const double* area_rngs; int A; int max_det;
  EvalOrderWs o; const int* img_off; uint8_t* taken;
  uint8_t* flags; int* npig; int* status;
};

// the (image, class) cell of the detection at position p of S, or -1: invalid, cut (rank >= max_det) or dropped (its class is
// neither positive -- a cell with ground truth -- nor negative in its image)
__device__ __forceinline__ long le_cell(const LeMatchArgs& a, long p) {
  const long i = a.o.order_s[p];
  if (eval_invalid(a.d, i)) return -1;
  const int im = a.d.image[i];
  if (p - a.img_off[im] >= a.max_det) return -1;
  const long cell = (long)im * a.d.K + a.d.classes[i];
  if (a.gt_off[cell + 1] == a.gt_off[cell] && !(a.lists[cell] & CTDET_LVIS_NEG)) return -1;
  return cell;
}

// order-S keys: {image | score}; an invalid detection goes behind the last image and raises the status word
__global__ void __launch_bounds__(256) le_key_image_kernel(LeMatchArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.d.N) return;
  const int st = eval_invalid(a.d, i);
  if (st) atomicOr(a.status, st);
  const uint32_t im = st ? (uint32_t)a.d.I : (uint32_t)a.d.image[i];
  a.o.keys64[i] = ((uint64_t)im << 32) | eval_score_key(a.d.scores[i]);
  a.o.vals[i] = (uint32_t)i;
}

// keys of the total order, over the positions of S: {class | score}, class K for a detection that takes no part
__global__ void __launch_bounds__(256) le_key_class_kernel(LeMatchArgs a) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.d.N) return;
  const long i = a.o.order_s[p];
  const uint32_t c = le_cell(a, p) < 0 ? (uint32_t)a.d.K : (uint32_t)a.d.classes[i];
  a.o.keys64[p] = ((uint64_t)c << 32) | eval_score_key(a.d.scores[i]);
}

// keys of the cell order, over the positions of S: the cell, I*K for a detection that takes no part
__global__ void __launch_bounds__(256) le_key_cell_kernel(LeMatchArgs a) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.d.N) return;
  const long cell = le_cell(a, p);
  a.o.keys32[p] = cell < 0 ? (uint32_t)a.d.I * (uint32_t)a.d.K : (uint32_t)cell;
}

// ctdet_cocoeval_iou's formula without a crowd
__device__ __forceinline__ double le_iou(double dx, double dy, double dw, double dh, double gx, double gy, double gw, double gh) {
  const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
  const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
  if (w <= 0.0 || h <= 0.0) return 0.0;
  const double inter = w * h, da = dw * dh, ga = gw * gh;
  return inter / (da + ga - inter);
}

__global__ void __launch_bounds__(64) le_match_kernel(LeMatchArgs a) {
  __shared__ uint8_t taken_lds[LE_LDS_GT * 64];
  const int cell = blockIdx.x, lane = threadIdx.x;
  const int g0 = a.gt_off[cell], G = a.gt_off[cell + 1] - g0;
  const int d0 = a.o.dt_off[cell], D = a.o.dt_off[cell + 1] - d0;
  if (G == 0 && D == 0) return;
  const int k = cell % a.d.K, AT = a.A * a.T;
  const bool active = lane < AT;
  const int ar = active ? lane / a.T : 0, t = active ? lane % a.T : 0;
  const double lo = a.area_rngs[ar * 2], hi = a.area_rngs[ar * 2 + 1];
  const double thr = fmin(a.iou_thrs[t], 1 - 1e-10);
  const double* gb = a.gt_boxes + (long)g0 * 4;
  const double* ga = a.gt_area + g0;
  const uint8_t* gi = a.gt_ignore + g0;
  if (active && t == 0) {     // non-ignored ground truths of this (class, area range): an integer sum, order-independent
    int cnt = 0;
    for (int g = 0; g < G; ++g) cnt += !(gi[g] != 0 || ga[g] < lo || ga[g] > hi);
    if (cnt) atomicAdd(&a.npig[k * a.A + ar], cnt);
  }
  if (D == 0) return;
  const bool nel = (a.lists[cell] & CTDET_LVIS_NEL) != 0;
  uint8_t* taken = G <= LE_LDS_GT ? taken_lds : a.taken + (long)g0 * AT;
  for (long i = lane; i < (long)G * AT; i += 64) taken[i] = 0;
  __syncthreads();
  for (int d = 0; d < D; ++d) {
    const long o = a.o.cell_order[d0 + d];
    const float x1 = a.d.boxes[o * 4], y1 = a.d.boxes[o * 4 + 1], x2 = a.d.boxes[o * 4 + 2], y2 = a.d.boxes[o * 4 + 3];
    const double dx = (double)x1, dy = (double)y1, dw = (double)(x2 - x1), dh = (double)(y2 - y1);   // w, h in f32, then widened
    const double darea = dw * dh;
    if (!active) continue;
    double best = thr;
    int match = -1;
    bool match_ign = false;
    // the ground truths in partition order: the non-ignored ones (pass 0), then the ignored ones (pass 1), each in input
    // order.  A detection that holds a non-ignored match stops at the first ignored ground truth: no pass 1.
    for (int pass = 0; pass < 2 && !(pass == 1 && match >= 0); ++pass) {
      for (int g = 0; g < G; ++g) {
        const bool ign = gi[g] != 0 || ga[g] < lo || ga[g] > hi;
        if (ign != (pass == 1)) continue;
        if (taken[(long)g * AT + lane]) continue;
        const double v = le_iou(dx, dy, dw, dh, gb[g * 4L], gb[g * 4L + 1], gb[g * 4L + 2], gb[g * 4L + 3]);
        if (v < best) continue;
        best = v; match = g; match_ign = ign;
      }
    }
    if (match >= 0) taken[(long)match * AT + lane] = 1;     // a lane reads and writes its own column only
    const bool ignored = match >= 0 ? match_ign : (darea < lo || darea > hi || nel);
    a.flags[o * AT + lane] = (uint8_t)((match >= 0 ? 1 : 0) | (ignored ? 2 : 0));
  }
}

struct LeAccArgs {
  const int* order; const int* cls_off; const uint8_t* flags; const int* npig;
  int K, A, T, R;
  const double* rec_thrs; double* precision; double* recall;
};

__global__ void __launch_bounds__(LE_NT) le_accum_kernel(LeAccArgs a) {
  extern __shared__ __attribute__((aligned(16))) char le_dsm[];
  double* env = (double*)le_dsm;              // [R] running envelope value of each recall threshold
  int* own = (int*)(env + a.R);               // [R] position of the first detection that reaches it, or -1
  __shared__ double sm[LE_NT];
  __shared__ uint32_t wsum[LE_NT / 64];
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int t = b % a.T; b /= a.T;
  const int ar = b % a.A;
  const int k = b / a.A;
  const long pstride = (long)a.K * a.A;                                  // precision: [T,R,K,A]
  const long pbase = (long)t * a.R * pstride + (long)k * a.A + ar;
  const long ridx = ((long)t * a.K + k) * a.A + ar;                      // recall: [T,K,A]
  const int np = a.npig[k * a.A + ar];
  if (np == 0) {
    for (int r = tid; r < a.R; r += LE_NT) a.precision[pbase + r * pstride] = -1.0;
    if (tid == 0) a.recall[ridx] = -1.0;
    return;
  }
  for (int r = tid; r < a.R; r += LE_NT) { env[r] = -1.0; own[r] = -1; }
  __syncthreads();
  const int AT = a.A * a.T, col = ar * a.T + t;
  const int s0 = a.cls_off[k], s1 = a.cls_off[k + 1];
  const double dnp = (double)np;
  int ctp = 0, cfp = 0;
  // ---- pass 1: running counts; which position is the first to reach each recall threshold
  for (int base = s0; base < s1; base += LE_NT) {
    const int j = base + tid;
    const EvalPos at = eval_chunk<LE_NT>(a.order, a.flags, AT, col, 0, j, s1, wsum, ctp, cfp);     // flag 0: a false positive
    if (j < s1 && (at.tp || j == s0)) {
      const double rec = (double)at.itp / dnp, prev = (double)(at.itp - (int)at.tp) / dnp;
      for (int r = 0; r < a.R; ++r) {
        const double thr = a.rec_thrs[r];
        if (rec >= thr && (j == s0 || !(prev >= thr))) own[r] = j;
      }
    }
  }
  __syncthreads();
  const int total_tp = ctp;
  // ---- pass 2: precision of every position; envelope (suffix maximum) at the recorded positions
  ctp = 0; cfp = 0;
  for (int base = s0; base < s1; base += LE_NT) {
    const int j = base + tid;
    const EvalPos at = eval_chunk<LE_NT>(a.order, a.flags, AT, col, 0, j, s1, wsum, ctp, cfp);
    eval_suffix_max<LE_NT>(sm, j < s1 ? (double)at.itp / ((double)(at.ifp + at.itp) + 0x1p-52) : -1.0, -1.0);
    for (int r = tid; r < a.R; r += LE_NT) {
      const int o = own[r];
      if (o >= 0 && o < base + LE_NT) env[r] = fmax(env[r], sm[o < base ? 0 : o - base]);
    }
  }
  __syncthreads();
  for (int r = tid; r < a.R; r += LE_NT) a.precision[pbase + r * pstride] = own[r] >= 0 ? env[r] : 0.0;
  if (tid == 0) a.recall[ridx] = (double)total_tp / dnp;
}

// ---- workspace: the ordering stage's blocks, image offsets i32 [I + 2], the taken table u8 [NG * A*T], then the sort block.
// ws == nullptr: the sizes alone
struct LeWs { EvalOrderWs o; int* img_off; uint8_t* taken; EvalSorter sort; size_t total; };
static LeWs le_layout(void* ws, long N, long NG, long I, long K, long A, long T) {
  EvalLayout l = {(uintptr_t)ws, 0};
  LeWs w;
  w.o = eval_order_layout(l, N, I * K);
  w.img_off = l.take<int>(I + 2);
  w.taken = l.take<uint8_t>((size_t)NG * A * T);
  w.sort = eval_sort_layout(l, "lviseval", N);
  w.total = l.p;
  return w;
}

static int le_check_dims(const char* what, int64_t N, int64_t NG, int32_t I, int32_t K, int32_t A, int32_t T) {
  if (const int rc = eval_check_dims(what, "classes", N, NG, I, K)) return rc;
  CTDET_CHECK(A >= 1 && T >= 1 && A * (int64_t)T <= 64, "%s: A=%d area ranges x T=%d thresholds must fit the 64 lanes of a wave",
              what, A, T);
  return 0;
}

extern "C" {

size_t ctdet_lviseval_workspace_bytes(int64_t N, int64_t NG, int32_t I, int32_t K, int32_t A, int32_t T) {
  if (le_check_dims("lviseval_workspace_bytes", N, NG, I, K, A, T)) return 0;
  return le_layout(nullptr, N, NG, I, K, A, T).total;
}

int32_t ctdet_lviseval_match(const float* boxes, const float* scores, const int32_t* classes, const int32_t* image, int64_t N,
                             const double* gt_boxes, const double* gt_area, const uint8_t* gt_ignore, const int32_t* gt_off,
                             int64_t NG, const uint8_t* lists, int32_t I, int32_t K, const double* iou_thrs, int32_t T,
                             const double* area_rngs, int32_t A, int32_t max_det, void* workspace, int32_t* order,
                             int32_t* cls_off, uint8_t* flags, int32_t* npig, int32_t* status, void* stream) {
  const char* what = "lviseval_match";
  if (const int rc = eval_check_match_ptrs(what, N, NG, boxes, scores, classes, image, gt_boxes, gt_off, workspace, order,
                                           cls_off, flags, status))
    return rc;
  EVAL_CHECK_PTR(what, lists);
  EVAL_CHECK_PTR(what, iou_thrs);
  EVAL_CHECK_PTR(what, area_rngs);
  EVAL_CHECK_PTR(what, npig);
  EVAL_CHECK_PTR_IF(what, NG, gt_area);
  EVAL_CHECK_PTR_IF(what, NG, gt_ignore);
  CTDET_CHECK(max_det >= 1, "lviseval_match: max_det=%d", max_det);
  if (const int rc = le_check_dims(what, N, NG, I, K, A, T)) return rc;
  EVAL_CHECK_WORKSPACE("lviseval_match", workspace);
  CTDET_KERNEL("le_match_kernel<wave per cell,%d matchers>", A * T);
  hipStream_t s = (hipStream_t)stream;
  const LeWs w = le_layout(workspace, N, NG, I, K, A, T);
  const LeMatchArgs a = {{boxes, scores, classes, image, N, I, K}, gt_boxes, gt_area, gt_ignore, gt_off, lists, iou_thrs, T,
                         area_rngs, A, max_det, w.o, w.img_off, w.taken, flags, npig, status};
  const int ncell = I * K;
  const dim3 nb((unsigned)((N + 255) / 256)), nt(256);
  hipLaunchKernelGGL(eval_clear_kernel, dim3((K * A + 255) / 256), nt, 0, s, npig, K * A, status);
  if (N) hipLaunchKernelGGL(le_key_image_kernel, nb, nt, 0, s, a);
  if (const int rc = w.sort.sort_cut(w.o.keys64, w.o.keys64_sorted, w.o.vals, w.o.order_s, I, w.img_off, s)) return rc;
  if (N) hipLaunchKernelGGL(le_key_class_kernel, nb, nt, 0, s, a);
  if (const int rc = w.sort.sort_cut(w.o.keys64, w.o.keys64_sorted, w.o.order_s, (uint32_t*)order, K, cls_off, s)) return rc;
  if (N) hipLaunchKernelGGL(le_key_cell_kernel, nb, nt, 0, s, a);
  if (const int rc = w.sort.sort_cut(w.o.keys32, w.o.keys32_sorted, w.o.order_s, w.o.cell_order, ncell, w.o.dt_off, s)) return rc;
  hipLaunchKernelGGL(le_match_kernel, dim3(ncell), dim3(64), 0, s, a);
  CTDET_LAUNCH_CHECK();
  return 0;
}

int32_t ctdet_lviseval_accumulate(const int32_t* order, const int32_t* cls_off, const uint8_t* flags, const int32_t* npig,
                                  int64_t N, int32_t K, int32_t A, int32_t T, const double* rec_thrs, int32_t R,
                                  double* precision, double* recall, void* stream) {
  const char* what = "lviseval_accumulate";
  EVAL_CHECK_PTR(what, cls_off);
  EVAL_CHECK_PTR(what, npig);
  EVAL_CHECK_PTR(what, rec_thrs);
  EVAL_CHECK_PTR(what, precision);
  EVAL_CHECK_PTR(what, recall);
  EVAL_CHECK_PTR_IF(what, N, order);
  EVAL_CHECK_PTR_IF(what, N, flags);
  CTDET_CHECK(R >= 1 && R <= 4096, "lviseval_accumulate: R=%d recall thresholds (1..4096)", R);
  if (const int rc = le_check_dims(what, N, 0, 1, K, A, T)) return rc;
  CTDET_CHECK((int64_t)K * A * T < (1LL << 31), "lviseval_accumulate: K*A*T too large");
  CTDET_KERNEL("le_accum_kernel<workgroup per (k,a,t),two passes>");
  const LeAccArgs a = {order, cls_off, flags, npig, K, A, T, R, rec_thrs, precision, recall};
  hipLaunchKernelGGL(le_accum_kernel, dim3(K * A * T), dim3(LE_NT), (size_t)R * 12, (hipStream_t)stream, a);
  CTDET_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
