// COCO box-AP scoring on the device ("bbox" task, useCats = 1): the matching and accumulation of the reference's native
// scorer (detectron2/layers/csrc/cocoeval/cocoeval.cpp: EvaluateImages :142-199, Accumulate :372-502) over the detections
// of a whole dataset, which are in device memory already when the evaluator sees them.  The definition that is reproduced
// bit for bit is written out in DESIGN.md 7.7; what matters here:
//
//   * every value is f64 and either a ratio of integers, a copied score or an IoU.  This file is compiled with floating
//     point contraction OFF (FLAGS_cocoeval in the Makefile): `da + ga - inter` must round twice, as the host's does.
//   * two orders, both equal to a stable sort (ties in the score are the rule, not the exception):
//       order 1: (image, category) cell major, score descending, ties in input order  -> `order` [N]
//       order 2: from order 1, category major, score descending, ties in order 1      -> workspace
//     Both are one rocprim device radix sort (stable) of a 64-bit key {cell | category, ~monotone(score bits)}.
//   * match: ONE WAVE per (image, category) cell.  The A*T (area range, IoU threshold) greedy matchers of a cell are
//     independent and serial over the cell's <= max_det detections x G ground truths: matcher (a, t) is lane a*T + t.  All
//     lanes look at the same (detection, ground truth) pair at a time, so box reads are wave-uniform; a lane's "ground truth
//     taken" flags are a column of a [G][A*T] byte table -- in LDS while it fits CE_LDS_TAKEN, else in the caller's workspace
//     (a cell with hundreds of ground truths takes the same code path through a flat pointer).
//   * accumulate: one workgroup per (category, area range, maxDet, threshold) walks the category's segment of order 2 in
//     256-element chunks, twice.  Pass 1 carries the running TP / FP counts and, recall being non-decreasing, records for
//     every recall threshold the first position that reaches it (LDS).  Pass 2 recomputes the precision of every position and
//     folds a per-chunk suffix maximum into the recorded positions' envelope values.  No per-detection buffer per (a, m, t).
//   * the only atomics are integer adds (valid ground truths per (category, area range)): two runs are bit-identical.
#include "common.h"
#include "../../include/ctdet_hip.h"
#include <rocprim/device/device_radix_sort.hpp>

#define CE_LDS_TAKEN 8192       // bytes of "ground truth taken" flags a cell keeps in LDS (G * A*T <= this)
#define CE_NT 256               // accumulate workgroup
#define CE_RANK_NONE 0x7FFFFFFF // rank of a detection that belongs to no cell (image / class index out of range)

struct CeMatchArgs {
  const float* boxes; const float* scores; const int* classes; const int* image; long N;
  const double* gt_boxes; const double* gt_area; const uint8_t* gt_crowd; const int* gt_off; int I, K;
  const double* iou_thrs; int T; const double* area_rngs; int A; int max_det;
  uint64_t* keys; const uint64_t* keys_sorted; uint32_t* vals; int* dt_off; uint8_t* taken;
  int* order; int* rank; uint8_t* flags; int* npig; int* status;
};

__device__ __forceinline__ double ce_iou(double dx, double dy, double dw, double dh, double gx, double gy, double gw,
                                         double gh, bool crowd) {
  const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
  const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
  if (w <= 0.0 || h <= 0.0) return 0.0;
  const double inter = w * h, da = dw * dh, ga = gw * gh;
  return inter / (crowd ? da : da + ga - inter);
}

// ascending order of the key = descending order of the score; equal scores (-0 == +0 included) give equal keys
__device__ __forceinline__ uint32_t ce_score_key(float s) {
  uint32_t u = __float_as_uint(s + 0.0f);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~u;
}

__global__ void __launch_bounds__(256) ce_iou_kernel(const double* __restrict__ dt, int D, const double* __restrict__ gt,
                                                     const uint8_t* __restrict__ crowd, int G, double* __restrict__ iou) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)D * G) return;
  const int d = (int)(i / G), g = (int)(i % G);
  iou[i] = ce_iou(dt[d * 4L], dt[d * 4L + 1], dt[d * 4L + 2], dt[d * 4L + 3], gt[g * 4L], gt[g * 4L + 1], gt[g * 4L + 2],
                  gt[g * 4L + 3], crowd[g] != 0);
}

__global__ void __launch_bounds__(256) ce_clear_kernel(int* __restrict__ npig, int n, int* __restrict__ status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) npig[i] = 0;
  if (i == 0) status[0] = 0;
}

// order-1 keys; a detection whose image or class index is out of range goes to the cell behind the last one (no workgroup
// ever looks at it) and raises the status word
__global__ void __launch_bounds__(256) ce_key1_kernel(CeMatchArgs a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  const int im = a.image[i], c = a.classes[i];
  uint32_t cell = (uint32_t)a.I * (uint32_t)a.K;
  if (im >= 0 && im < a.I && c >= 0 && c < a.K) cell = (uint32_t)im * (uint32_t)a.K + (uint32_t)c;
  else a.status[0] = 1;
  a.keys[i] = ((uint64_t)cell << 32) | ce_score_key(a.scores[i]);
  a.vals[i] = (uint32_t)i;
}

// off[c] = first position of the sorted keys whose high word is >= c, c in [0, ncell]
__global__ void __launch_bounds__(256) ce_offsets_kernel(const uint64_t* __restrict__ keys, long N, int ncell,
                                                         int* __restrict__ off) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c > ncell) return;
  long lo = 0, hi = N;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if ((long)(keys[mid] >> 32) < c) lo = mid + 1;
    else hi = mid;
  }
  off[c] = (int)lo;
}

__global__ void __launch_bounds__(256) ce_rank_kernel(const uint64_t* __restrict__ keys, long N, int ncell,
                                                      const int* __restrict__ off, int* __restrict__ rank) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= N) return;
  const long cell = (long)(keys[p] >> 32);
  rank[p] = cell < ncell ? (int)(p - off[cell]) : CE_RANK_NONE;
}

__global__ void __launch_bounds__(64) ce_match_kernel(CeMatchArgs a) {
  __shared__ uint8_t taken_lds[CE_LDS_TAKEN];
  const int cell = blockIdx.x, lane = threadIdx.x;
  const int g0 = a.gt_off[cell], G = a.gt_off[cell + 1] - g0;
  const int d0 = a.dt_off[cell], nd = a.dt_off[cell + 1] - d0;
  if (G == 0 && nd == 0) return;
  const int k = cell % a.K, AT = a.A * a.T;
  const bool active = lane < AT;
  const int ar = active ? lane / a.T : 0, t = active ? lane % a.T : 0;
  const double lo = a.area_rngs[ar * 2], hi = a.area_rngs[ar * 2 + 1];
  const double thr = fmin(a.iou_thrs[t], 1 - 1e-10);
  const double* gb = a.gt_boxes + (long)g0 * 4;
  const double* ga = a.gt_area + g0;
  const uint8_t* gc = a.gt_crowd + g0;
  if (active && t == 0) {     // valid ground truths of this (category, area range): an integer sum, order-independent
    int cnt = 0;
    for (int g = 0; g < G; ++g) cnt += !(gc[g] != 0 || ga[g] < lo || ga[g] > hi);
    if (cnt) atomicAdd(&a.npig[k * a.A + ar], cnt);
  }
  const int D = nd < a.max_det ? nd : a.max_det;
  if (D == 0) return;
  uint8_t* taken = (long)G * AT <= CE_LDS_TAKEN ? taken_lds : a.taken + (long)g0 * AT;
  for (long i = lane; i < (long)G * AT; i += 64) taken[i] = 0;
  __syncthreads();
  for (int d = 0; d < D; ++d) {
    const long o = a.order[d0 + d];
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
        const bool crowd = gc[g] != 0;
        const bool ign = crowd || ga[g] < lo || ga[g] > hi;
        if (ign != (pass == 1)) continue;
        if (taken[(long)g * AT + lane] && !crowd) continue;
        const double v = ce_iou(dx, dy, dw, dh, gb[g * 4L], gb[g * 4L + 1], gb[g * 4L + 2], gb[g * 4L + 3], crowd);
        if (v >= best) { best = v; match = g; match_ign = ign; }
      }
    }
    if (match >= 0) taken[(long)match * AT + lane] = 1;
    const bool ignored = match >= 0 ? match_ign : (darea < lo || darea > hi);
    a.flags[(long)(d0 + d) * AT + lane] = (uint8_t)((match >= 0 ? 1 : 0) | (ignored ? 2 : 0));
  }
}

struct CeAccArgs {
  const float* scores; const int* classes; const int* order; const int* rank; const uint8_t* flags; const int* npig;
  long N; int K, A, T, R, M, max_det;
  const double* rec_thrs; const int* max_dets;
  uint64_t* keys; const uint64_t* keys_sorted; uint32_t* vals; const uint32_t* order2; int* cat_off;
  double* precision; double* scores_out; double* recall;
};

// order-2 keys over the positions of order 1
__global__ void __launch_bounds__(256) ce_key2_kernel(CeAccArgs a) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.N) return;
  const long o = a.order[p];
  const uint32_t c = a.rank[p] == CE_RANK_NONE ? (uint32_t)a.K : (uint32_t)a.classes[o];
  a.keys[p] = ((uint64_t)c << 32) | ce_score_key(a.scores[o]);
  a.vals[p] = (uint32_t)p;
}

// inclusive scan over the workgroup of three counters <= CE_NT packed into one word (10 bits each); `tot` = the sum
__device__ __forceinline__ uint32_t ce_scan3(uint32_t v, uint32_t* wsum, uint32_t& tot) {
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
  for (int w = 0; w < CE_NT / 64; ++w) {
    const uint32_t s = wsum[w];
    tot += s;
    if (w < wv) v += s;
  }
  return v;
}

__global__ void __launch_bounds__(CE_NT) ce_accum_kernel(CeAccArgs a) {
  extern __shared__ __attribute__((aligned(16))) char ce_dsm[];
  double* env = (double*)ce_dsm;              // [R] running envelope value of each recall threshold
  int* own = (int*)(env + a.R);               // [R] position (order 2) of the first detection that reaches it, or -1
  __shared__ double sm[CE_NT];
  __shared__ uint32_t wsum[CE_NT / 64];
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int t = b % a.T; b /= a.T;
  const int m = b % a.M; b /= a.M;
  const int ar = b % a.A;
  const int k = b / a.A;
  const long pstride = (long)a.K * a.A * a.M;                                    // precision / scores: [T,R,K,A,M]
  const long pbase = (long)t * a.R * pstride + ((long)k * a.A + ar) * a.M + m;
  const long ridx = (((long)t * a.K + k) * a.A + ar) * a.M + m;                  // recall: [T,K,A,M]
  const int np = a.npig[k * a.A + ar];
  if (np == 0) {
    for (int r = tid; r < a.R; r += CE_NT) { a.precision[pbase + r * pstride] = -1.0; a.scores_out[pbase + r * pstride] = -1.0; }
    if (tid == 0) a.recall[ridx] = -1.0;
    return;
  }
  for (int r = tid; r < a.R; r += CE_NT) { env[r] = -1.0; own[r] = -1; }
  __syncthreads();
  // a cell was cut to max_det detections by the matcher (flags beyond are unwritten): a larger maxDet acts as max_det, which
  // is what the reference's `d < size && d < maxDet` over the cut cell does
  const int md = a.max_dets[m] < a.max_det ? a.max_dets[m] : a.max_det, AT = a.A * a.T, col = ar * a.T + t;
  const int s0 = a.cat_off[k], s1 = a.cat_off[k + 1];
  const double dnp = (double)np;
  int ctp = 0, cfp = 0, cn = 0;
  // ---- pass 1: running counts; which position is the lower bound of each recall threshold
  for (int base = s0; base < s1; base += CE_NT) {
    const int j = base + tid;
    uint32_t inc = 0, tp = 0, fp = 0;
    long p = 0;
    if (j < s1) {
      p = a.order2[j];
      if (a.rank[p] < md) {
        const uint32_t f = a.flags[p * AT + col];
        inc = 1; tp = f == 1; fp = f == 0;
      }
    }
    uint32_t tot;
    const uint32_t sc = ce_scan3(inc | (tp << 10) | (fp << 20), wsum, tot);
    if (inc) {
      const int itp = ctp + (int)((sc >> 10) & 1023u), idx = cn + (int)(sc & 1023u);
      const bool first = idx == 1;
      if (tp || first) {
        const double rec = (double)itp / dnp, prev = (double)(itp - (int)tp) / dnp;
        for (int r = 0; r < a.R; ++r) {
          const double thr = a.rec_thrs[r];
          if (rec >= thr && (first || !(prev >= thr))) {
            own[r] = j;
            a.scores_out[pbase + r * pstride] = (double)a.scores[a.order[p]];
          }
        }
      }
    }
    cn += (int)(tot & 1023u); ctp += (int)((tot >> 10) & 1023u); cfp += (int)(tot >> 20);
  }
  __syncthreads();
  const int total_tp = ctp;
  // ---- pass 2: precision of every position; envelope (suffix maximum) at the recorded positions
  ctp = 0; cfp = 0;
  for (int base = s0; base < s1; base += CE_NT) {
    const int j = base + tid;
    uint32_t inc = 0, tp = 0, fp = 0;
    if (j < s1) {
      const long p = a.order2[j];
      if (a.rank[p] < md) {
        const uint32_t f = a.flags[p * AT + col];
        inc = 1; tp = f == 1; fp = f == 0;
      }
    }
    uint32_t tot;
    const uint32_t sc = ce_scan3(inc | (tp << 10) | (fp << 20), wsum, tot);
    double prec = -1.0;
    if (inc) {
      const int itp = ctp + (int)((sc >> 10) & 1023u), ifp = cfp + (int)(sc >> 20);
      prec = itp + ifp > 0 ? (double)itp / (double)(itp + ifp) : 0.0;
    }
    sm[tid] = prec;
    __syncthreads();
    for (int o = 1; o < CE_NT; o <<= 1) {
      const double v = tid + o < CE_NT ? sm[tid + o] : -1.0;
      __syncthreads();
      sm[tid] = fmax(sm[tid], v);
      __syncthreads();
    }
    for (int r = tid; r < a.R; r += CE_NT) {
      const int o = own[r];
      if (o >= 0 && o < base + CE_NT) env[r] = fmax(env[r], sm[o < base ? 0 : o - base]);
    }
    ctp += (int)((tot >> 10) & 1023u); cfp += (int)(tot >> 20);
  }
  __syncthreads();
  for (int r = tid; r < a.R; r += CE_NT) {
    if (own[r] >= 0) a.precision[pbase + r * pstride] = env[r];
    else { a.precision[pbase + r * pstride] = 0.0; a.scores_out[pbase + r * pstride] = 0.0; }
  }
  if (tid == 0) a.recall[ridx] = (double)total_tp / dnp;
}

// ---- workspace: {keys, sorted keys} u64 [N] each, values u32 [N], order 2 u32 [N], offsets i32 [max(I*K, K) + 2], the taken
// table u8 [NG * A*T], then the sort's own temporary storage (bounded here, checked against rocprim's answer at the call)
static inline size_t ce_up(size_t v) { return (v + 255) & ~(size_t)255; }
struct CeWs { size_t keys, keys_sorted, vals, order2, off, taken, sort, total; };
static CeWs ce_layout(long N, long NG, long I, long K, long A, long T) {
  CeWs w;
  size_t p = 0;
  w.keys = p; p += ce_up((size_t)N * 8);
  w.keys_sorted = p; p += ce_up((size_t)N * 8);
  w.vals = p; p += ce_up((size_t)N * 4);
  w.order2 = p; p += ce_up((size_t)N * 4);
  w.off = p; p += ce_up((size_t)((I * K > K ? I * K : K) + 2) * 4);
  w.taken = p; p += ce_up((size_t)NG * A * T);
  w.sort = p; p += ce_up((size_t)N * 16 + ((size_t)16 << 20));
  w.total = p;
  return w;
}

static int ce_bits(unsigned long v) { int b = 1; while ((v >> b) && b < 32) ++b; return b; }

static int ce_sort(const CeWs& w, char* ws, long N, int high_bits, uint32_t* vals_out, hipStream_t s) {
  size_t need = 0;
  const uint64_t* kin = (const uint64_t*)(ws + w.keys);
  uint64_t* kout = (uint64_t*)(ws + w.keys_sorted);
  const uint32_t* vin = (const uint32_t*)(ws + w.vals);
  hipError_t e = rocprim::radix_sort_pairs(nullptr, need, kin, kout, vin, vals_out, (size_t)N, 0u, 32u + high_bits, s);
  CTDET_CHECK(e == hipSuccess, "cocoeval: sort size query failed: %s", hipGetErrorString(e));
  const size_t have = w.total - w.sort;
  CTDET_CHECK(need <= have, "cocoeval: the sort needs %zu bytes of temporary storage, the workspace formula provides %zu", need,
              have);
  e = rocprim::radix_sort_pairs(ws + w.sort, need, kin, kout, vin, vals_out, (size_t)N, 0u, 32u + high_bits, s);
  CTDET_CHECK(e == hipSuccess, "cocoeval: sort failed: %s", hipGetErrorString(e));
  return 0;
}

static int ce_check_dims(const char* what, int64_t N, int64_t NG, int32_t I, int32_t K, int32_t A, int32_t T) {
  CTDET_CHECK(N >= 0 && N < (1LL << 31) - 1024, "%s: N=%lld out of range", what, (long long)N);
  CTDET_CHECK(NG >= 0 && NG < (1LL << 31), "%s: %lld ground truths out of range", what, (long long)NG);
  // one 64-thread workgroup per cell: a grid holds fewer than 2^32 threads
  CTDET_CHECK(I >= 1 && K >= 1 && (int64_t)I * K < (1LL << 26), "%s: I=%d images x K=%d categories out of range (I*K < 2^26)",
              what, I, K);
  CTDET_CHECK(A >= 1 && T >= 1 && A * (int64_t)T <= 64, "%s: A=%d area ranges x T=%d thresholds must fit the 64 lanes of a wave",
              what, A, T);
  return 0;
}

extern "C" {

size_t ctdet_cocoeval_workspace_bytes(int64_t N, int64_t NG, int32_t I, int32_t K, int32_t A, int32_t T) {
  if (ce_check_dims("cocoeval_workspace_bytes", N, NG, I, K, A, T)) return 0;
  return ce_layout(N, NG, I, K, A, T).total;
}

int32_t ctdet_cocoeval_iou(const double* dt, int32_t D, const double* gt, const uint8_t* gt_crowd, int32_t G, double* iou,
                           void* stream) {
  CTDET_CHECK(D >= 0 && G >= 0, "cocoeval_iou: D=%d G=%d", D, G);
  if ((long)D * G == 0) return 0;
  CTDET_CHECK(dt && gt && gt_crowd && iou, "cocoeval_iou: null pointer");
  CTDET_KERNEL("ce_iou_kernel<f64,contract off>");
  hipLaunchKernelGGL(ce_iou_kernel, dim3((unsigned)(((long)D * G + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dt, D, gt,
                     gt_crowd, G, iou);
  CTDET_LAUNCH_CHECK();
  return 0;
}

int32_t ctdet_cocoeval_match(const float* boxes, const float* scores, const int32_t* classes, const int32_t* image, int64_t N,
                             const double* gt_boxes, const double* gt_area, const uint8_t* gt_crowd, const int32_t* gt_off,
                             int64_t NG, int32_t I, int32_t K, const double* iou_thrs, int32_t T, const double* area_rngs,
                             int32_t A, int32_t max_det, void* workspace, int32_t* order, int32_t* rank, uint8_t* flags,
                             int32_t* npig, int32_t* status, void* stream) {
  CTDET_CHECK(gt_off && iou_thrs && area_rngs && workspace && npig && status, "cocoeval_match: null pointer");
  CTDET_CHECK(NG == 0 || (gt_boxes && gt_area && gt_crowd), "cocoeval_match: null ground-truth pointer");
  CTDET_CHECK(N == 0 || (boxes && scores && classes && image && order && rank && flags), "cocoeval_match: null detection pointer");
  CTDET_CHECK(max_det >= 1, "cocoeval_match: max_det=%d", max_det);
  const int rc = ce_check_dims("cocoeval_match", N, NG, I, K, A, T);
  if (rc) return rc;
  CTDET_CHECK(((uintptr_t)workspace & 255) == 0, "cocoeval_match: workspace must be 256-byte aligned");
  CTDET_KERNEL("ce_match_kernel<wave per cell,%d matchers>", A * T);
  hipStream_t s = (hipStream_t)stream;
  const CeWs w = ce_layout(N, NG, I, K, A, T);
  char* ws = (char*)workspace;
  CeMatchArgs a;
  a.boxes = boxes; a.scores = scores; a.classes = classes; a.image = image; a.N = N;
  a.gt_boxes = gt_boxes; a.gt_area = gt_area; a.gt_crowd = gt_crowd; a.gt_off = gt_off; a.I = I; a.K = K;
  a.iou_thrs = iou_thrs; a.T = T; a.area_rngs = area_rngs; a.A = A; a.max_det = max_det;
  a.keys = (uint64_t*)(ws + w.keys); a.keys_sorted = (const uint64_t*)(ws + w.keys_sorted); a.vals = (uint32_t*)(ws + w.vals);
  a.dt_off = (int*)(ws + w.off); a.taken = (uint8_t*)(ws + w.taken);
  a.order = order; a.rank = rank; a.flags = flags; a.npig = npig; a.status = status;
  const int ncell = I * K;
  const unsigned nb = (unsigned)((N + 255) / 256);
  hipLaunchKernelGGL(ce_clear_kernel, dim3((K * A + 255) / 256), dim3(256), 0, s, npig, K * A, status);
  if (N) {
    hipLaunchKernelGGL(ce_key1_kernel, dim3(nb), dim3(256), 0, s, a);
    const int src = ce_sort(w, ws, N, ce_bits((unsigned long)ncell), (uint32_t*)order, s);
    if (src) return src;
  }
  hipLaunchKernelGGL(ce_offsets_kernel, dim3((ncell + 1 + 255) / 256), dim3(256), 0, s, a.keys_sorted, (long)N, ncell, a.dt_off);
  if (N) hipLaunchKernelGGL(ce_rank_kernel, dim3(nb), dim3(256), 0, s, a.keys_sorted, (long)N, ncell, (const int*)a.dt_off, rank);
  hipLaunchKernelGGL(ce_match_kernel, dim3(ncell), dim3(64), 0, s, a);
  CTDET_LAUNCH_CHECK();
  return 0;
}

int32_t ctdet_cocoeval_accumulate(const float* scores, const int32_t* classes, const int32_t* order, const int32_t* rank,
                                  const uint8_t* flags, const int32_t* npig, int64_t N, int32_t K, int32_t A, int32_t T,
                                  const double* rec_thrs, int32_t R, const int32_t* max_dets, int32_t M, int32_t max_det,
                                  void* workspace, double* precision, double* scores_out, double* recall, void* stream) {
  CTDET_CHECK(npig && rec_thrs && max_dets && workspace && precision && scores_out && recall, "cocoeval_accumulate: null pointer");
  CTDET_CHECK(N == 0 || (scores && classes && order && rank && flags), "cocoeval_accumulate: null detection pointer");
  CTDET_CHECK(R >= 1 && R <= 4096 && M >= 1, "cocoeval_accumulate: R=%d recall thresholds (1..4096), M=%d maxDets", R, M);
  CTDET_CHECK(max_det >= 1, "cocoeval_accumulate: max_det=%d", max_det);
  const int rc = ce_check_dims("cocoeval_accumulate", N, 0, 1, K, A, T);
  if (rc) return rc;
  CTDET_CHECK((int64_t)K * A * M * T < (1LL << 31), "cocoeval_accumulate: K*A*M*T too large");
  CTDET_CHECK(((uintptr_t)workspace & 255) == 0, "cocoeval_accumulate: workspace must be 256-byte aligned");
  CTDET_KERNEL("ce_accum_kernel<workgroup per (k,a,m,t),two passes>");
  hipStream_t s = (hipStream_t)stream;
  // the leading blocks of the layout do not depend on NG / I: the same workspace serves both calls
  const CeWs w = ce_layout(N, 0, 1, K, A, T);
  char* ws = (char*)workspace;
  CeAccArgs a;
  a.scores = scores; a.classes = classes; a.order = order; a.rank = rank; a.flags = flags; a.npig = npig;
  a.N = N; a.K = K; a.A = A; a.T = T; a.R = R; a.M = M; a.max_det = max_det; a.rec_thrs = rec_thrs; a.max_dets = max_dets;
  a.keys = (uint64_t*)(ws + w.keys); a.keys_sorted = (const uint64_t*)(ws + w.keys_sorted); a.vals = (uint32_t*)(ws + w.vals);
  a.order2 = (const uint32_t*)(ws + w.order2); a.cat_off = (int*)(ws + w.off);
  a.precision = precision; a.scores_out = scores_out; a.recall = recall;
  if (N) {
    hipLaunchKernelGGL(ce_key2_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, a);
    const int src = ce_sort(w, ws, N, ce_bits((unsigned long)K), (uint32_t*)(ws + w.order2), s);
    if (src) return src;
  }
  hipLaunchKernelGGL(ce_offsets_kernel, dim3((K + 1 + 255) / 256), dim3(256), 0, s, a.keys_sorted, (long)N, K, a.cat_off);
  hipLaunchKernelGGL(ce_accum_kernel, dim3(K * A * M * T), dim3(CE_NT), (size_t)R * 12, s, a);
  CTDET_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
