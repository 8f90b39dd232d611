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
#include "eval_common.h"
#include "../../include/ctdet_lviseval.h"

#define LE_LDS_GT 128           // ground truths of a cell whose taken flags (one byte per matcher, <= 64 matchers) stay in LDS
#define LE_NT 256               // accumulate workgroup = chunk of the class segment

struct LeMatchArgs {
  const float* boxes; const float* scores; const int* classes; const int* image; long N;
  const double* gt_boxes; const double* gt_area; const uint8_t* gt_ignore; const int* gt_off; const uint8_t* lists; int I, K;
  const double* iou_thrs; int T; const double* area_rngs; int A; int max_det;
  uint64_t* keys64; uint32_t* vals; const uint32_t* order_s; uint32_t* keys32;
  const uint32_t* cell_order; const int* img_off; int* dt_off; uint8_t* taken;
  uint8_t* flags; int* npig; int* status;
};

// status bits of a detection that takes no part (0: it does)
__device__ __forceinline__ int le_invalid(const LeMatchArgs& a, long i) {
  const int c = a.classes[i], im = a.image[i];
  int st = 0;
  if (c < 0 || c >= a.K) st |= CTDET_LVIS_BAD_CLASS;
  if (im < 0 || im >= a.I) st |= CTDET_LVIS_BAD_IMAGE;
  if (!isfinite(a.scores[i])) st |= CTDET_LVIS_BAD_SCORE;
  const float* b = a.boxes + i * 4;
  if (!(isfinite(b[0]) && isfinite(b[1]) && isfinite(b[2]) && isfinite(b[3]))) st |= CTDET_LVIS_BAD_BOX;
  return st;
}

// the (image, class) cell of the detection at position p of S, or -1: invalid, cut (rank >= max_det) or dropped (its class is
// neither positive -- a cell with ground truth -- nor negative in its image)
__device__ __forceinline__ long le_cell(const LeMatchArgs& a, long p) {
  const long i = a.order_s[p];
  if (le_invalid(a, i)) return -1;
  const int im = a.image[i];
  if (p - a.img_off[im] >= a.max_det) return -1;
  const long cell = (long)im * a.K + a.classes[i];
  if (a.gt_off[cell + 1] == a.gt_off[cell] && !(a.lists[cell] & CTDET_LVIS_NEG)) return -1;
  return cell;
}

__global__ void __launch_bounds__(256) le_clear_kernel(int* __restrict__ npig, int n, int* __restrict__ status) {
  eval_clear(npig, n, status);
}

// order-S keys: {image | score}; an invalid detection goes behind the last image and raises the status word
__global__ void __launch_bounds__(256) le_key_image_kernel(LeMatchArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  const int st = le_invalid(a, i);
  if (st) atomicOr(a.status, st);
  const uint32_t im = st ? (uint32_t)a.I : (uint32_t)a.image[i];
  a.keys64[i] = ((uint64_t)im << 32) | eval_score_key(a.scores[i]);
  a.vals[i] = (uint32_t)i;
}

// keys of the total order, over the positions of S: {class | score}, class K for a detection that takes no part
__global__ void __launch_bounds__(256) le_key_class_kernel(LeMatchArgs a) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.N) return;
  const long i = a.order_s[p];
  const uint32_t c = le_cell(a, p) < 0 ? (uint32_t)a.K : (uint32_t)a.classes[i];
  a.keys64[p] = ((uint64_t)c << 32) | eval_score_key(a.scores[i]);
}

// keys of the cell order, over the positions of S: the cell, I*K for a detection that takes no part
__global__ void __launch_bounds__(256) le_key_cell_kernel(LeMatchArgs a) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.N) return;
  const long cell = le_cell(a, p);
  a.keys32[p] = cell < 0 ? (uint32_t)a.I * (uint32_t)a.K : (uint32_t)cell;
}

// off[c] = first position of the sorted keys whose group (the high word of a 64-bit key, a 32-bit key itself) is >= c, c in [0, n]
__global__ void __launch_bounds__(256) le_offsets64_kernel(const uint64_t* __restrict__ keys, long N, int n, int* __restrict__ off) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c > n) return;
  off[c] = eval_lower_bound(keys, N, c, [](uint64_t k) { return (long)(k >> 32); });
}
__global__ void __launch_bounds__(256) le_offsets32_kernel(const uint32_t* __restrict__ keys, long N, int n, int* __restrict__ off) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c > n) return;
  off[c] = eval_lower_bound(keys, N, c, [](uint32_t k) { return (long)k; });
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
  const int d0 = a.dt_off[cell], D = a.dt_off[cell + 1] - d0;
  if (G == 0 && D == 0) return;
  const int k = cell % a.K, AT = a.A * a.T;
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
    const long o = a.cell_order[d0 + d];
    const float x1 = a.boxes[o * 4], y1 = a.boxes[o * 4 + 1], x2 = a.boxes[o * 4 + 2], y2 = a.boxes[o * 4 + 3];
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
    uint32_t tp = 0, fp = 0;
    if (j < s1) {
      const uint32_t f = a.flags[(long)a.order[j] * AT + col];
      tp = f == 1; fp = f == 0;
    }
    uint32_t tot;
    const uint32_t sc = eval_scan_packed<LE_NT>(tp | (fp << 16), wsum, tot);     // two 16-bit counters
    if (j < s1 && (tp || j == s0)) {
      const int itp = ctp + (int)(sc & 0xFFFFu);
      const double rec = (double)itp / dnp, prev = (double)(itp - (int)tp) / dnp;
      for (int r = 0; r < a.R; ++r) {
        const double thr = a.rec_thrs[r];
        if (rec >= thr && (j == s0 || !(prev >= thr))) own[r] = j;
      }
    }
    ctp += (int)(tot & 0xFFFFu); cfp += (int)(tot >> 16);
  }
  __syncthreads();
  const int total_tp = ctp;
  // ---- pass 2: precision of every position; envelope (suffix maximum) at the recorded positions
  ctp = 0; cfp = 0;
  for (int base = s0; base < s1; base += LE_NT) {
    const int j = base + tid;
    uint32_t tp = 0, fp = 0;
    if (j < s1) {
      const uint32_t f = a.flags[(long)a.order[j] * AT + col];
      tp = f == 1; fp = f == 0;
    }
    uint32_t tot;
    const uint32_t sc = eval_scan_packed<LE_NT>(tp | (fp << 16), wsum, tot);
    double prec = -1.0;
    if (j < s1) {
      const int itp = ctp + (int)(sc & 0xFFFFu), ifp = cfp + (int)(sc >> 16);
      prec = (double)itp / ((double)(ifp + itp) + 0x1p-52);
    }
    eval_suffix_max<LE_NT>(sm, prec, -1.0);
    for (int r = tid; r < a.R; r += LE_NT) {
      const int o = own[r];
      if (o >= 0 && o < base + LE_NT) env[r] = fmax(env[r], sm[o < base ? 0 : o - base]);
    }
    ctp += (int)(tot & 0xFFFFu); cfp += (int)(tot >> 16);
  }
  __syncthreads();
  for (int r = tid; r < a.R; r += LE_NT) a.precision[pbase + r * pstride] = own[r] >= 0 ? env[r] : 0.0;
  if (tid == 0) a.recall[ridx] = (double)total_tp / dnp;
}

// ---- workspace: {keys, sorted keys} u64 [N] each, values u32 [N], order S u32 [N], cell keys u32 [N] x 2, cell order u32 [N],
// cell offsets i32 [I*K + 2], image offsets i32 [I + 2], the taken table u8 [NG * A*T], then the sort block
struct LeWs { size_t keys64, keys64_sorted, vals, order_s, keys32, keys32_sorted, cell_order, off, img_off, taken, sort, total; };
static LeWs le_layout(long N, long NG, long I, long K, long A, long T) {
  LeWs w;
  size_t p = 0;
  w.keys64 = p; p += eval_up((size_t)N * 8);
  w.keys64_sorted = p; p += eval_up((size_t)N * 8);
  w.vals = p; p += eval_up((size_t)N * 4);
  w.order_s = p; p += eval_up((size_t)N * 4);
  w.keys32 = p; p += eval_up((size_t)N * 4);
  w.keys32_sorted = p; p += eval_up((size_t)N * 4);
  w.cell_order = p; p += eval_up((size_t)N * 4);
  w.off = p; p += eval_up((size_t)(I * K + 2) * 4);
  w.img_off = p; p += eval_up((size_t)(I + 2) * 4);
  w.taken = p; p += eval_up((size_t)NG * A * T);
  w.sort = p; p += eval_sort_bytes(N);
  w.total = p;
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
  return le_layout(N, NG, I, K, A, T).total;
}

int32_t ctdet_lviseval_match(const float* boxes, const float* scores, const int32_t* classes, const int32_t* image, int64_t N,
                             const double* gt_boxes, const double* gt_area, const uint8_t* gt_ignore, const int32_t* gt_off,
                             int64_t NG, const uint8_t* lists, int32_t I, int32_t K, const double* iou_thrs, int32_t T,
                             const double* area_rngs, int32_t A, int32_t max_det, void* workspace, int32_t* order,
                             int32_t* cls_off, uint8_t* flags, int32_t* npig, int32_t* status, void* stream) {
  CTDET_CHECK(gt_off, "lviseval_match: null pointer gt_off");
  CTDET_CHECK(lists, "lviseval_match: null pointer lists");
  CTDET_CHECK(iou_thrs, "lviseval_match: null pointer iou_thrs");
  CTDET_CHECK(area_rngs, "lviseval_match: null pointer area_rngs");
  CTDET_CHECK(workspace, "lviseval_match: null pointer workspace");
  CTDET_CHECK(cls_off, "lviseval_match: null pointer cls_off");
  CTDET_CHECK(npig, "lviseval_match: null pointer npig");
  CTDET_CHECK(status, "lviseval_match: null pointer status");
  CTDET_CHECK(NG <= 0 || gt_boxes, "lviseval_match: null pointer gt_boxes");
  CTDET_CHECK(NG <= 0 || gt_area, "lviseval_match: null pointer gt_area");
  CTDET_CHECK(NG <= 0 || gt_ignore, "lviseval_match: null pointer gt_ignore");
  CTDET_CHECK(N <= 0 || boxes, "lviseval_match: null pointer boxes");
  CTDET_CHECK(N <= 0 || scores, "lviseval_match: null pointer scores");
  CTDET_CHECK(N <= 0 || classes, "lviseval_match: null pointer classes");
  CTDET_CHECK(N <= 0 || image, "lviseval_match: null pointer image");
  CTDET_CHECK(N <= 0 || order, "lviseval_match: null pointer order");
  CTDET_CHECK(N <= 0 || flags, "lviseval_match: null pointer flags");
  CTDET_CHECK(max_det >= 1, "lviseval_match: max_det=%d", max_det);
  const int rc = le_check_dims("lviseval_match", N, NG, I, K, A, T);
  if (rc) return rc;
  EVAL_CHECK_WORKSPACE("lviseval_match", workspace);
  CTDET_KERNEL("le_match_kernel<wave per cell,%d matchers>", A * T);
  hipStream_t s = (hipStream_t)stream;
  const LeWs w = le_layout(N, NG, I, K, A, T);
  char* ws = (char*)workspace;
  LeMatchArgs a;
  a.boxes = boxes; a.scores = scores; a.classes = classes; a.image = image; a.N = N;
  a.gt_boxes = gt_boxes; a.gt_area = gt_area; a.gt_ignore = gt_ignore; a.gt_off = gt_off; a.lists = lists; a.I = I; a.K = K;
  a.iou_thrs = iou_thrs; a.T = T; a.area_rngs = area_rngs; a.A = A; a.max_det = max_det;
  a.keys64 = (uint64_t*)(ws + w.keys64); a.vals = (uint32_t*)(ws + w.vals); a.order_s = (const uint32_t*)(ws + w.order_s);
  a.keys32 = (uint32_t*)(ws + w.keys32); a.cell_order = (const uint32_t*)(ws + w.cell_order);
  a.img_off = (const int*)(ws + w.img_off); a.dt_off = (int*)(ws + w.off); a.taken = (uint8_t*)(ws + w.taken);
  a.flags = flags; a.npig = npig; a.status = status;
  uint64_t* k64s = (uint64_t*)(ws + w.keys64_sorted);
  uint32_t* k32s = (uint32_t*)(ws + w.keys32_sorted);
  const int ncell = I * K;
  const unsigned nb = (unsigned)((N + 255) / 256);
  const auto sort = [&](auto* kin, auto* kout, const uint32_t* vin, uint32_t* vout, int bits) {     // tmp: the sort block
    return eval_sort("lviseval", kin, kout, vin, vout, N, bits, ws + w.sort, w.total - w.sort, s);
  };
  hipLaunchKernelGGL(le_clear_kernel, dim3((K * A + 255) / 256), dim3(256), 0, s, npig, K * A, status);
  if (N) {
    hipLaunchKernelGGL(le_key_image_kernel, dim3(nb), dim3(256), 0, s, a);
    const int src = sort(a.keys64, k64s, a.vals, (uint32_t*)(ws + w.order_s), 32 + eval_bits((unsigned long)I));
    if (src) return src;
  }
  hipLaunchKernelGGL(le_offsets64_kernel, dim3((I + 1 + 255) / 256), dim3(256), 0, s, k64s, (long)N, I, (int*)(ws + w.img_off));
  if (N) {
    hipLaunchKernelGGL(le_key_class_kernel, dim3(nb), dim3(256), 0, s, a);
    const int src = sort(a.keys64, k64s, a.order_s, (uint32_t*)order, 32 + eval_bits((unsigned long)K));
    if (src) return src;
  }
  hipLaunchKernelGGL(le_offsets64_kernel, dim3((K + 1 + 255) / 256), dim3(256), 0, s, k64s, (long)N, K, cls_off);
  if (N) {
    hipLaunchKernelGGL(le_key_cell_kernel, dim3(nb), dim3(256), 0, s, a);
    const int src = sort(a.keys32, k32s, a.order_s, (uint32_t*)(ws + w.cell_order), eval_bits((unsigned long)ncell));
    if (src) return src;
  }
  hipLaunchKernelGGL(le_offsets32_kernel, dim3((ncell + 1 + 255) / 256), dim3(256), 0, s, k32s, (long)N, ncell, a.dt_off);
  hipLaunchKernelGGL(le_match_kernel, dim3(ncell), dim3(64), 0, s, a);
  CTDET_LAUNCH_CHECK();
  return 0;
}

int32_t ctdet_lviseval_accumulate(const int32_t* order, const int32_t* cls_off, const uint8_t* flags, const int32_t* npig,
                                  int64_t N, int32_t K, int32_t A, int32_t T, const double* rec_thrs, int32_t R,
                                  double* precision, double* recall, void* stream) {
  CTDET_CHECK(cls_off, "lviseval_accumulate: null pointer cls_off");
  CTDET_CHECK(npig, "lviseval_accumulate: null pointer npig");
  CTDET_CHECK(rec_thrs, "lviseval_accumulate: null pointer rec_thrs");
  CTDET_CHECK(precision, "lviseval_accumulate: null pointer precision");
  CTDET_CHECK(recall, "lviseval_accumulate: null pointer recall");
  CTDET_CHECK(N <= 0 || order, "lviseval_accumulate: null pointer order");
  CTDET_CHECK(N <= 0 || flags, "lviseval_accumulate: null pointer flags");
  CTDET_CHECK(R >= 1 && R <= 4096, "lviseval_accumulate: R=%d recall thresholds (1..4096)", R);
  const int rc = le_check_dims("lviseval_accumulate", N, 0, 1, K, A, T);
  if (rc) return rc;
  CTDET_CHECK((int64_t)K * A * T < (1LL << 31), "lviseval_accumulate: K*A*T too large");
  CTDET_KERNEL("le_accum_kernel<workgroup per (k,a,t),two passes>");
  LeAccArgs a;
  a.order = order; a.cls_off = cls_off; a.flags = flags; a.npig = npig; a.K = K; a.A = A; a.T = T; a.R = R;
  a.rec_thrs = rec_thrs; a.precision = precision; a.recall = recall;
  hipLaunchKernelGGL(le_accum_kernel, dim3(K * A * T), dim3(LE_NT), (size_t)R * 12, (hipStream_t)stream, a);
  CTDET_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
