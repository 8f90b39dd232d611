// Training-side HBM-bound kernels: gaussian target splat, focal loss, masked L1 loss, SGD, Adam / AdamW.
//   gaussian targets : detectron2/data/detection_utils.py:600-705 (gen_heatmap, gaussian_radius, gaussian2D,
//                      draw_umich_gaussian) -- the reference runs this per image / per object in numpy on the
//                      host inside model.forward (centernet.py:188); here one launch covers B x 128 objects.
//   focal loss       : detectron2/modeling/meta_arch/centernet.py:204, 333-369 (_neg_loss)
//   reg L1 loss      : centernet.py:372-397 (RegL1Loss, _transpose_and_gather_feat)
//   SGD              : detectron2/solver/build.py:93-137 -> torch.optim.SGD(momentum, weight_decay)
#include "common.h"

// ------------------------------------------------------------------------------------------------
// gaussian_radius: evaluated in f64 in exactly the reference's operation order; contraction is off so
// no FMA changes a rounding (the int() truncation downstream makes the last ulp matter).
// ------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)
__host__ __device__ inline double ctdet_gaussian_radius_f64(int height, int width) {
  const double min_overlap = 0.7;
  const double hw = (double)(width * height);
  const double b1 = (double)(height + width);
  const double c1 = hw * (1 - min_overlap) / (1 + min_overlap);
  const double sq1 = sqrt(b1 * b1 - 4 * c1);
  const double r1 = (b1 + sq1) / 2;

  const double b2 = (double)(2 * (height + width));
  const double c2 = (1 - min_overlap) * (double)width * (double)height;
  const double sq2 = sqrt(b2 * b2 - 16 * c2);
  const double r2 = (b2 + sq2) / 2;

  const double a3 = 4 * min_overlap;
  const double b3 = -2 * min_overlap * (double)(height + width);
  const double c3 = (min_overlap - 1) * (double)width * (double)height;
  const double sq3 = sqrt(b3 * b3 - 4 * a3 * c3);
  const double r3 = (b3 + sq3) / 2;
  double r = r1 < r2 ? r1 : r2;
  r = r3 < r ? r3 : r;
  return r;
}

__global__ void gaussian_radius_kernel(const int* __restrict__ hw, int n, double* __restrict__ out_r,
                                       int* __restrict__ out_i) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double r = ctdet_gaussian_radius_f64(hw[2 * i], hw[2 * i + 1]);
  if (out_r) out_r[i] = r;
  if (out_i) { const int ri = (int)r; out_i[i] = ri > 0 ? ri : 0; }
}

// one workgroup per (object k, image b)
__global__ void __launch_bounds__(256) gaussian_targets_kernel(const float* __restrict__ boxes,
                                                               const int64_t* __restrict__ classes,
                                                               const int* __restrict__ counts, int Nmax, int H, int W,
                                                               int C, float* __restrict__ hm, float* __restrict__ wh,
                                                               float* __restrict__ reg, int64_t* __restrict__ ind,
                                                               uint8_t* __restrict__ reg_mask) {
  const int k = blockIdx.x, b = blockIdx.y;
  const long o = (long)b * 128 + k;
  int n = counts[b];
  n = n < 128 ? n : 128;
  n = n < Nmax ? n : Nmax;
  bool valid = k < n;
  float bx0 = 0, by0 = 0, bx1 = 0, by1 = 0, h = 0, w = 0;
  if (valid) {
    const float* bp = boxes + ((long)b * Nmax + k) * 4;
    bx0 = bp[0] / 4.f; by0 = bp[1] / 4.f; bx1 = bp[2] / 4.f; by1 = bp[3] / 4.f;
    h = by1 - by0; w = bx1 - bx0;
    valid = h > 0.f && w > 0.f;
  }
  if (!valid) {
    if (threadIdx.x == 0) {
      wh[o * 2] = 0.f; wh[o * 2 + 1] = 0.f; reg[o * 2] = 0.f; reg[o * 2 + 1] = 0.f; ind[o] = 0; reg_mask[o] = 0;
    }
    return;
  }
  const int radius_raw = (int)ctdet_gaussian_radius_f64((int)ceilf(h), (int)ceilf(w));
  const int radius = radius_raw > 0 ? radius_raw : 0;
  const float ctx = (bx0 + bx1) / 2.f, cty = (by0 + by1) / 2.f;
  const int cx = (int)ctx, cy = (int)cty;  // astype(int32): truncation toward zero
  if (cx < 0 || cx >= W || cy < 0 || cy >= H || ctx < 0.f || cty < 0.f) {
    // a box whose centre lies outside the map (unclipped annotations): the reference's gather raises an index error for
    // it (centernet.py:392-397); here the object is dropped instead of writing through an out-of-range index
    if (threadIdx.x == 0) {
      wh[o * 2] = 0.f; wh[o * 2 + 1] = 0.f; reg[o * 2] = 0.f; reg[o * 2 + 1] = 0.f; ind[o] = 0; reg_mask[o] = 0;
    }
    return;
  }
  if (threadIdx.x == 0) {
    wh[o * 2] = w; wh[o * 2 + 1] = h;
    ind[o] = (int64_t)cy * W + cx;
    reg[o * 2] = ctx - (float)cx; reg[o * 2 + 1] = cty - (float)cy;
    reg_mask[o] = 1;
  }
  const int cls = (int)classes[(long)b * Nmax + k];
  if (cls < 0 || cls >= C) return;
  const int diameter = 2 * radius + 1;
  const double sigma = (double)diameter / 6;
  const double denom = 2 * sigma * sigma;
  const double eps = 2.220446049250313e-16;  // np.finfo(float64).eps; h.max() == 1 (the centre)
  unsigned int* hmu = (unsigned int*)hm + (long)b * H * W * C + cls;
  for (int i = threadIdx.x; i < diameter * diameter; i += 256) {
    const int gy = i / diameter, gx = i % diameter;
    const int py = cy - radius + gy, px = cx - radius + gx;
    if (py < 0 || py >= H || px < 0 || px >= W) continue;
    const double yy = (double)(gy - radius), xx = (double)(gx - radius);
    double g = exp(-(xx * xx + yy * yy) / denom);
    if (g < eps) g = 0;
    const float gf = (float)g;
    atomicMax(hmu + ((long)py * W + px) * C, __float_as_uint(gf));  // all values >= 0: uint order == float order
  }
}
#pragma clang fp contract(fast)

int launch_gaussian_radius(const int* hw, int n, double* out_r, int* out_i, hipStream_t s) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(gaussian_radius_kernel, dim3((n + 255) / 256), dim3(256), 0, s, hw, n, out_r, out_i);
  CTDET_LAUNCH_CHECK();
  return 0;
}

// the target map is cleared by a KERNEL, not hipMemsetAsync: inside a captured training step the memset became a memset node,
// and a replay launched on an idle stream ran it out of order with the splat kernel after it (two ranks sharing one GPU, the
// data-parallel step whose SGD launch is eager: hm_loss 93.7 -> 127 ... inf within 12 steps, profiles/r04_graph_memset_node.txt)
__global__ __launch_bounds__(256) void zero_f32_kernel(float* __restrict__ p, long n) {
  const long n4 = n >> 2, stride = (long)gridDim.x * 256;
  float4* p4 = (float4*)p;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) p4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) p[(n4 << 2) + threadIdx.x] = 0.f;
}

int launch_gaussian_targets(const float* boxes, const int64_t* classes, const int* counts, int B, int Nmax, int H,
                            int W, int C, float* hm, float* wh, float* reg, int64_t* ind, uint8_t* reg_mask,
                            hipStream_t s) {
  if (B == 0) return 0;
  CTDET_CHECK(((uintptr_t)hm & 15) == 0, "gaussian_targets: hm must be 16-byte aligned");
  const long n = (long)B * H * W * C;
  if (ctdet_tuning_flags() & CTDET_TUNE_TARGETS_MEMSET) {
    const hipError_t e = hipMemsetAsync(hm, 0, (size_t)n * sizeof(float), s);
    CTDET_CHECK(e == hipSuccess, "gaussian_targets: memset failed: %s", hipGetErrorString(e));
  } else
  hipLaunchKernelGGL(zero_f32_kernel, dim3((unsigned)std::min<long>((n / 4 + 255) / 256 + 1, 2048)), dim3(256), 0, s, hm, n);
  CTDET_LAUNCH_CHECK();
  hipLaunchKernelGGL(gaussian_targets_kernel, dim3(128, B), dim3(256), 0, s, boxes, classes, counts, Nmax, H, W, C, hm,
                     wh, reg, ind, reg_mask);
  CTDET_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// focal loss
// ------------------------------------------------------------------------------------------------
#define FL_VEC_PER_BLOCK (256 * 8)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

template <bool GRAD>
__global__ void __launch_bounds__(256) focal_main_kernel(const float* __restrict__ logits, const float* __restrict__ gt,
                                                         const float* __restrict__ alpha, long nvec, int C,
                                                         float grad_scale, float* __restrict__ grad,
                                                         float* __restrict__ partial) {
  __shared__ float red[3][4];
  float pos = 0.f, neg = 0.f, npos = 0.f;
  const long base = (long)blockIdx.x * FL_VEC_PER_BLOCK;
  for (int it = 0; it < 8; ++it) {
    const long i = base + it * 256 + threadIdx.x;
    if (i >= nvec) break;
    const f32x4 x = *(const f32x4*)(logits + i * 4);
    const f32x4 g = *(const f32x4*)(gt + i * 4);
    const int c0 = (int)((i * 4) % C);
    f32x4 gr = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int ce = c0 + e < C ? c0 + e : c0 + e - C;   // any class count: a vector may straddle two pixels
      const float s = ctdet_sigmoid_exact(x[e]);
      const float p = fminf(fmaxf(s, 1e-4f), 1.f - 1e-4f);
      const float dpdx = (s >= 1e-4f && s <= 1.f - 1e-4f) ? s * (1.f - s) : 0.f;
      float dLdp = 0.f;
      if (g[e] == 1.f) {
        const float a = alpha[ce % C], lp = logf(p), q = 1.f - p;
        pos += a * (lp * (q * q));
        npos += 1.f;
        if (GRAD) dLdp = a * (q * q / p - 2.f * q * lp);
      } else if (g[e] < 1.f) {
        const float om = 1.f - g[e];
        const float nw = (om * om) * (om * om);
        const float l1p = logf(1.f - p);
        neg += l1p * (p * p) * nw;
        if (GRAD) dLdp = nw * (2.f * p * l1p - p * p / (1.f - p));
      }
      gr[e] = -dLdp * dpdx * grad_scale;
    }
    if (GRAD) *(f32x4*)(grad + i * 4) = gr;
  }
  pos = wave_sum(pos); neg = wave_sum(neg); npos = wave_sum(npos);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { red[0][wv] = pos; red[1][wv] = neg; red[2][wv] = npos; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[(long)blockIdx.x * 3 + 0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    partial[(long)blockIdx.x * 3 + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    partial[(long)blockIdx.x * 3 + 2] = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
  }
}

// deterministic fixed-order reduction of the block partials (f64), one workgroup
__global__ void __launch_bounds__(256) focal_finalize_kernel(const float* __restrict__ partial, int nblocks,
                                                             float* __restrict__ loss, float* __restrict__ stats) {
  __shared__ double red[3][256];
  double a = 0, b = 0, c = 0;
  for (int i = threadIdx.x; i < nblocks; i += 256) { a += partial[i * 3]; b += partial[i * 3 + 1]; c += partial[i * 3 + 2]; }
  red[0][threadIdx.x] = a; red[1][threadIdx.x] = b; red[2][threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      red[0][threadIdx.x] += red[0][threadIdx.x + o];
      red[1][threadIdx.x] += red[1][threadIdx.x + o];
      red[2][threadIdx.x] += red[2][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double pos = red[0][0], neg = red[1][0], np = red[2][0];
    const double l = np == 0 ? -neg : -(pos + neg) / np;
    loss[0] = (float)l;
    stats[0] = (float)pos; stats[1] = (float)neg; stats[2] = (float)np;
    stats[3] = np == 0 ? 1.f : (float)(1.0 / np);
  }
}

__global__ void __launch_bounds__(256) scale_by_dev_kernel(float* __restrict__ g, long nvec, const float* __restrict__ sc) {
  const float s = sc[0];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
    f32x4 v = *(f32x4*)(g + i * 4);
    v = v * s;
    *(f32x4*)(g + i * 4) = v;
  }
}

size_t focal_workspace_bytes(long numel) {
  const long nvec = (numel + 3) / 4;
  const long nblocks = (nvec + FL_VEC_PER_BLOCK - 1) / FL_VEC_PER_BLOCK;
  return (size_t)(nblocks * 3 + 4) * sizeof(float);
}

int launch_focal_loss(const float* logits, const float* gt, const float* alpha, int B, int H, int W, int C,
                      float grad_scale, void* workspace, float* loss, float* stats, float* grad, hipStream_t s) {
  const long numel = (long)B * H * W * C;
  CTDET_CHECK(numel % 4 == 0, "focal_loss: B*H*W*C=%ld must be a multiple of 4 (any C; maps are multiples of 4 pixels)", numel);
  CTDET_CHECK(numel > 0, "focal_loss: empty input");
  const long nvec = numel / 4;
  const int nblocks = (int)((nvec + FL_VEC_PER_BLOCK - 1) / FL_VEC_PER_BLOCK);
  float* partial = (float*)workspace;
  if (grad)
    hipLaunchKernelGGL((focal_main_kernel<true>), dim3(nblocks), dim3(256), 0, s, logits, gt, alpha, nvec, C, grad_scale,
                       grad, partial);
  else
    hipLaunchKernelGGL((focal_main_kernel<false>), dim3(nblocks), dim3(256), 0, s, logits, gt, alpha, nvec, C,
                       grad_scale, grad, partial);
  hipLaunchKernelGGL(focal_finalize_kernel, dim3(1), dim3(256), 0, s, partial, nblocks, loss, stats);
  if (grad) {
    int gb = (int)((nvec + 255) / 256);
    if (gb > 4096) gb = 4096;
    hipLaunchKernelGGL(scale_by_dev_kernel, dim3(gb), dim3(256), 0, s, grad, nvec, stats + 3);
  }
  CTDET_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// RegL1Loss: one workgroup; B*N entries (<= a few thousand)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) reg_l1_kernel(const float* __restrict__ pred, int pred_stride,
                                                     const uint8_t* __restrict__ mask, const int64_t* __restrict__ ind,
                                                     const float* __restrict__ target, int B, int N, int HW,
                                                     float grad_scale, float* __restrict__ loss,
                                                     float* __restrict__ grad, int grad_stride) {
  __shared__ double red[2][256];
  double sum = 0, msum = 0;
  const int total = B * N;
  for (int i = threadIdx.x; i < total; i += 256) {
    const int b = i / N;
    const long id = ind[i];
    const float m = (id >= 0 && id < HW) ? (float)mask[i] : 0.f;   // an index outside the map never reaches memory
    const float* p = pred + ((long)b * HW + (m != 0.f ? id : 0)) * pred_stride;
    const float d0 = p[0] * m - target[i * 2] * m, d1 = p[1] * m - target[i * 2 + 1] * m;
    sum += (double)fabsf(d0) + (double)fabsf(d1);
    msum += 2.0 * m;
  }
  red[0][threadIdx.x] = sum; red[1][threadIdx.x] = msum;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; }
    __syncthreads();
  }
  const float denom = (float)red[1][0] + 1e-4f;
  if (threadIdx.x == 0) loss[0] = (float)red[0][0] / denom;
  if (!grad) return;
  for (int i = threadIdx.x; i < total; i += 256) {
    const int b = i / N;
    const float m = (ind[i] >= 0 && ind[i] < HW) ? (float)mask[i] : 0.f;
    if (m == 0.f) continue;
    const float* p = pred + ((long)b * HW + ind[i]) * pred_stride;
    float* gp = grad + ((long)b * HW + ind[i]) * grad_stride;
    const float d0 = p[0] * m - target[i * 2] * m, d1 = p[1] * m - target[i * 2 + 1] * m;
    const float s0 = d0 > 0.f ? 1.f : (d0 < 0.f ? -1.f : 0.f), s1 = d1 > 0.f ? 1.f : (d1 < 0.f ? -1.f : 0.f);
    atomicAdd(gp, s0 * m / denom * grad_scale);
    atomicAdd(gp + 1, s1 * m / denom * grad_scale);
  }
}

int launch_reg_l1(const float* pred, int pred_stride, const uint8_t* mask, const int64_t* ind, const float* target,
                  int B, int N, int HW, float grad_scale, float* loss, float* grad, int grad_stride, hipStream_t s) {
  hipLaunchKernelGGL(reg_l1_kernel, dim3(1), dim3(256), 0, s, pred, pred_stride, mask, ind, target, B, N, HW, grad_scale,
                     loss, grad, grad_stride);
  CTDET_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// SGD with momentum + weight decay
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                  float* __restrict__ m, long n, const float* __restrict__ lr_dev,
                                                  float mom, float wd, int first) {
  const float lr = lr_dev[0];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    float gi = g[i];
    const float pi = p[i];
    if (wd != 0.f) gi = gi + wd * pi;
    const float bi = first ? gi : mom * m[i] + gi;
    m[i] = bi;
    p[i] = pi - lr * bi;
  }
}

// the same update over a flat buffer cut into `nruns` consecutive runs with their own (lr, weight decay): run r covers
// [run_end[r-1], run_end[r]); lr = lr_table[run_lr_index[r]] is read from device memory.  One launch instead of one per run
// (DLA-34: 109 runs, weights / norm / bias parameters alternate in backward order).
//
// CLIP / NEST select what detectron2/solver/build.py:19-58,134 adds to the step, in torch's order -- clip, weight decay,
// momentum, Nesterov look-ahead:
//   SGD_CLIP_VALUE  g = clamp(g, -clip_value, +clip_value)              (torch.nn.utils.clip_grad_value_, per parameter)
//   SGD_CLIP_NORM   g = g * coefs[run], the runs being the parameters    (torch.nn.utils.clip_grad_norm_, per parameter)
//   NEST            p -= lr * (g + mom * buf) instead of p -= lr * buf   (torch.optim.SGD(nesterov=True))
// The clipped gradient lives in registers only: g is never written.  The instantiation <SGD_CLIP_NONE, false> is the
// plain kernel, instruction for instruction.
template <int CLIP, bool NEST>
__device__ __forceinline__ void sgd_runs_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              long n, const long* __restrict__ run_end,
                                              const int* __restrict__ run_lr_index, const float* __restrict__ run_wd,
                                              const float* __restrict__ lr_table, int nruns, float mom, int first,
                                              float clip_value, const float* __restrict__ coefs) {
  // A workgroup owns a contiguous range and a thread walks it in steps of 1024 elements, four at a time: a thread stays
  // inside one run for many iterations, so the run lookup (a binary search over dependent global loads) is rare.  With a
  // grid-wide stride every iteration landed in another run and searched again (204 us for 18.6 M parameters).
  const long per = (((n + gridDim.x - 1) / gridDim.x) + 1023) & ~1023L;
  const long beg = (long)blockIdx.x * per, end = beg + per < n ? beg + per : n;
  long cur_end = -1;
  float lr = 0.f, wd = 0.f, cf = 1.f;
  auto lookup = [&](long i) {
    int lo = 0, hi = nruns - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (run_end[mid] > i) hi = mid; else lo = mid + 1;
    }
    cur_end = run_end[lo];
    lr = lr_table[run_lr_index[lo]];
    wd = run_wd[lo];
    if constexpr (CLIP == SGD_CLIP_NORM) cf = coefs[lo];     // one run per parameter: the search that finds lr finds this
  };
  auto clipped = [&](float gi) {
    if constexpr (CLIP == SGD_CLIP_VALUE) gi = gi > clip_value ? clip_value : (gi < -clip_value ? -clip_value : gi);  // NaN stays
    if constexpr (CLIP == SGD_CLIP_NORM) gi = gi * cf;
    return gi;
  };
  for (long i = beg + (long)threadIdx.x * 4; i < end; i += 1024) {
    if (i >= cur_end) lookup(i);
    if (i + 4 <= cur_end && i + 4 <= end) {
      const float4 gv = *(const float4*)(g + i), pv = *(const float4*)(p + i);
      float4 mv = {0.f, 0.f, 0.f, 0.f};
      if (!first) mv = *(const float4*)(m + i);
      const float ge[4] = {gv.x, gv.y, gv.z, gv.w}, pe[4] = {pv.x, pv.y, pv.z, pv.w}, me[4] = {mv.x, mv.y, mv.z, mv.w};
      float bo[4], po[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float gi = clipped(ge[k]);
        if (wd != 0.f) gi = gi + wd * pe[k];
        bo[k] = first ? gi : mom * me[k] + gi;
        if constexpr (NEST) po[k] = pe[k] - lr * (gi + mom * bo[k]);
        else po[k] = pe[k] - lr * bo[k];
      }
      *(float4*)(m + i) = make_float4(bo[0], bo[1], bo[2], bo[3]);
      *(float4*)(p + i) = make_float4(po[0], po[1], po[2], po[3]);
    } else {
      for (long j = i; j < i + 4 && j < end; ++j) {
        if (j >= cur_end) lookup(j);
        float gi = clipped(g[j]);
        const float pi = p[j];
        if (wd != 0.f) gi = gi + wd * pi;
        const float bi = first ? gi : mom * m[j] + gi;
        m[j] = bi;
        if constexpr (NEST) p[j] = pi - lr * (gi + mom * bi);
        else p[j] = pi - lr * bi;
      }
    }
  }
}

__global__ void __launch_bounds__(256) sgd_runs_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       long n, const long* __restrict__ run_end,
                                                       const int* __restrict__ run_lr_index, const float* __restrict__ run_wd,
                                                       const float* __restrict__ lr_table, int nruns, float mom, int first) {
  sgd_runs_body<SGD_CLIP_NONE, false>(p, g, m, n, run_end, run_lr_index, run_wd, lr_table, nruns, mom, first, 0.f, nullptr);
}

template <int CLIP, bool NEST>
__global__ void __launch_bounds__(256) sgd_runs_clip_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                            float* __restrict__ m, long n, const long* __restrict__ run_end,
                                                            const int* __restrict__ run_lr_index,
                                                            const float* __restrict__ run_wd, const float* __restrict__ lr_table,
                                                            int nruns, float mom, int first, float clip_value,
                                                            const float* __restrict__ coefs) {
  sgd_runs_body<CLIP, NEST>(p, g, m, n, run_end, run_lr_index, run_wd, lr_table, nruns, mom, first, clip_value, coefs);
}

int launch_sgd_runs(float* p, const float* g, float* m, long n, const long* run_end, const int* run_lr_index,
                    const float* run_wd, const float* lr_table, int nruns, float mom, int first, hipStream_t s) {
  if (n == 0 || nruns == 0) return 0;
  long nb = (n + 1023) / 1024;
  if (nb > 2048) nb = 2048;
  hipLaunchKernelGGL(sgd_runs_kernel, dim3((unsigned)nb), dim3(256), 0, s, p, g, m, n, run_end, run_lr_index, run_wd, lr_table,
                     nruns, mom, first);
  CTDET_LAUNCH_CHECK();
  return 0;
}

int launch_sgd_runs_clip(float* p, const float* g, float* m, long n, const long* run_end, const int* run_lr_index,
                         const float* run_wd, const float* lr_table, int nruns, float mom, int first, int nesterov, int clip_type,
                         float clip_value, const float* coefs, hipStream_t s) {
  if (n == 0 || nruns == 0) return 0;
  if (clip_type == SGD_CLIP_NONE && !nesterov)
    return launch_sgd_runs(p, g, m, n, run_end, run_lr_index, run_wd, lr_table, nruns, mom, first, s);
  long nb = (n + 1023) / 1024;
  if (nb > 2048) nb = 2048;
#define SGD_CLIP_CASE(C, N)                                                                                               \
  if (clip_type == C && (nesterov != 0) == N)                                                                             \
    hipLaunchKernelGGL((sgd_runs_clip_kernel<C, N>), dim3((unsigned)nb), dim3(256), 0, s, p, g, m, n, run_end, run_lr_index, \
                       run_wd, lr_table, nruns, mom, first, clip_value, coefs)
  SGD_CLIP_CASE(SGD_CLIP_NONE, true);
  SGD_CLIP_CASE(SGD_CLIP_VALUE, false);
  SGD_CLIP_CASE(SGD_CLIP_VALUE, true);
  SGD_CLIP_CASE(SGD_CLIP_NORM, false);
  SGD_CLIP_CASE(SGD_CLIP_NORM, true);
#undef SGD_CLIP_CASE
  CTDET_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Per-parameter gradient norms of the flat gradient buffer (clip_grad_norm_ called with one tensor at a time,
// detectron2/solver/build.py:26-27,47-51): a segmented reduction over a few hundred segments of 1 .. 2.36 M elements.
// The host cuts the buffer once into chunks of at most 4096 elements (solver/build.py: grad_chunks) that never cross a parameter boundary;
// pass 1 writes one f32 partial per chunk (sum g^2, sum |g| or max |g|), pass 2 combines a parameter's partials and derives
// torch's clip coefficient min(1, clip / (norm + 1e-6)).  Every sum has one fixed shape -- a thread's elements in address
// order, a 64-lane butterfly, the four waves of the workgroup left to right; in pass 2 lane l takes partials l, l + 64, ..
// in table order, then the same butterfly -- and nothing is accumulated with atomics, so the result is the same bits on
// every run.
// ------------------------------------------------------------------------------------------------
template <int NT>
__device__ __forceinline__ float norm_join(float a, float b) {
  if constexpr (NT == GRAD_NORM_INF) return (b > a || b != b) ? b : a;   // a NaN on either side stays, as in torch's max
  else return a + b;
}
template <int NT>
__device__ __forceinline__ float norm_term(float acc, float x) {
  if constexpr (NT == GRAD_NORM_L2) return acc + x * x;
  else return norm_join<NT>(acc, fabsf(x));
}
template <int NT>
__device__ __forceinline__ float norm_wave(float acc) {
#pragma unroll
  for (int o = 32; o; o >>= 1) acc = norm_join<NT>(acc, __shfl_xor(acc, o));
  return acc;
}

template <int NT>
__global__ void __launch_bounds__(256) grad_chunk_norm_kernel(const float* __restrict__ g, long n,
                                                              const long* __restrict__ chunk_start,
                                                              const int* __restrict__ chunk_len, float* __restrict__ partials) {
  // chunk starts are parameter offsets (any residue mod 4): the float4 grid is anchored at the 16-byte boundary below the
  // start, and a group that hangs over either end of the chunk is read element by element
  long s = chunk_start[blockIdx.x], e = s + chunk_len[blockIdx.x];
  if (s < 0) s = 0;
  if (e > n) e = n;      // a table that does not fit the buffer reads nothing outside it
  float acc = 0.f;
  for (long i = (s & ~3L) + (long)threadIdx.x * 4; i < e; i += 1024) {
    if (i >= s && i + 4 <= e) {
      const float4 v = *(const float4*)(g + i);
      acc = norm_term<NT>(norm_term<NT>(norm_term<NT>(norm_term<NT>(acc, v.x), v.y), v.z), v.w);
    } else {
      for (long j = i < s ? s : i; j < i + 4 && j < e; ++j) acc = norm_term<NT>(acc, g[j]);
    }
  }
  acc = norm_wave<NT>(acc);
  __shared__ float wave_part[4];
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    partials[blockIdx.x] = norm_join<NT>(norm_join<NT>(norm_join<NT>(wave_part[0], wave_part[1]), wave_part[2]), wave_part[3]);
}

// one wave per parameter: parameter q owns the chunks [param_chunk_end[q-1], param_chunk_end[q])
template <int NT>
__global__ void __launch_bounds__(256) grad_clip_coef_kernel(const float* __restrict__ partials,
                                                             const int* __restrict__ param_chunk_end, int nparams, int nchunks,
                                                             float clip_value, float* __restrict__ norms,
                                                             float* __restrict__ coefs) {
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (q >= nparams) return;
  int b = q ? param_chunk_end[q - 1] : 0, e = param_chunk_end[q];
  if (b < 0) b = 0;
  if (e > nchunks) e = nchunks;
  float acc = 0.f;
  for (int c = b + lane; c < e; c += 64) acc = norm_join<NT>(acc, partials[c]);
  acc = norm_wave<NT>(acc);
  if (lane == 0) {
    const float norm = NT == GRAD_NORM_L2 ? sqrtf(acc) : acc;
    norms[q] = norm;
    const float c = clip_value / (norm + 1e-6f);
    coefs[q] = c > 1.f ? 1.f : c;          // torch.clamp(c, max=1): a NaN norm gives a NaN coefficient
  }
}

int launch_grad_chunk_norms(const float* g, long n, const long* chunk_start, const int* chunk_len, int nchunks, int norm_type,
                            float* partials, hipStream_t s) {
  if (nchunks == 0) return 0;
  if (norm_type == GRAD_NORM_L2)
    hipLaunchKernelGGL(grad_chunk_norm_kernel<GRAD_NORM_L2>, dim3(nchunks), dim3(256), 0, s, g, n, chunk_start, chunk_len, partials);
  else if (norm_type == GRAD_NORM_L1)
    hipLaunchKernelGGL(grad_chunk_norm_kernel<GRAD_NORM_L1>, dim3(nchunks), dim3(256), 0, s, g, n, chunk_start, chunk_len, partials);
  else
    hipLaunchKernelGGL(grad_chunk_norm_kernel<GRAD_NORM_INF>, dim3(nchunks), dim3(256), 0, s, g, n, chunk_start, chunk_len, partials);
  CTDET_LAUNCH_CHECK();
  return 0;
}

int launch_grad_clip_coefs(const float* partials, const int* param_chunk_end, int nparams, int nchunks, int norm_type,
                           float clip_value, float* norms, float* coefs, hipStream_t s) {
  if (nparams == 0) return 0;
  const dim3 grid((nparams + 3) / 4);
  if (norm_type == GRAD_NORM_L2)
    hipLaunchKernelGGL(grad_clip_coef_kernel<GRAD_NORM_L2>, grid, dim3(256), 0, s, partials, param_chunk_end, nparams, nchunks,
                       clip_value, norms, coefs);
  else if (norm_type == GRAD_NORM_L1)
    hipLaunchKernelGGL(grad_clip_coef_kernel<GRAD_NORM_L1>, grid, dim3(256), 0, s, partials, param_chunk_end, nparams, nchunks,
                       clip_value, norms, coefs);
  else
    hipLaunchKernelGGL(grad_clip_coef_kernel<GRAD_NORM_INF>, grid, dim3(256), 0, s, partials, param_chunk_end, nparams, nchunks,
                       clip_value, norms, coefs);
  CTDET_LAUNCH_CHECK();
  return 0;
}

int launch_sgd(float* p, const float* g, float* m, long n, const float* lr_dev, float mom, float wd, int first,
               hipStream_t s) {
  if (n == 0) return 0;
  long nb = (n + 255) / 256;
  if (nb > 8192) nb = 8192;
  hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)nb), dim3(256), 0, s, p, g, m, n, lr_dev, mom, wd, first);
  CTDET_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Adam / AdamW (optionally AMSGrad) over the same flat buffer and run tables: torch.optim.Adam / AdamW, single-tensor
// non-capturable path, in torch's order per element --
//   g' = clip(g)                               as in sgd_runs_body: none | value | coefs[run]
//   ADAM : g' += wd * p   (when wd != 0)       ADAMW: p *= 1 - lr * wd
//   m = b1 * m + (1 - b1) * g'                 v = b2 * v + (1 - b2) * g'^2
//   AMSGRAD: vmax = max(vmax, v), vh = vmax    else vh = v
//   p -= (lr / (1 - b1^t)) * m / (sqrt(vh) / sqrt(1 - b2^t) + eps)
// The step count t lives in device memory: the captured training step replays optimizer.step() without the host, so a host
// counter would freeze the bias correction at the value of the capture.  adam_advance_kernel (one thread, first launch of
// every step) increments it and writes bias[0] = 1 / (1 - b1^t), bias[1] = 1 / sqrt(1 - b2^t), computed in f64; the update
// kernel reads the two once per thread.  Per element: one sqrt and one division, both correctly rounded (no fast-math).
// ------------------------------------------------------------------------------------------------
__global__ void adam_advance_kernel(long long* __restrict__ step, float* __restrict__ bias, double beta1, double beta2) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const long long t = step[0] + 1;
  step[0] = t;
  bias[0] = (float)(1.0 / (1.0 - pow(beta1, (double)t)));
  bias[1] = (float)(1.0 / sqrt(1.0 - pow(beta2, (double)t)));
}

int launch_adam_advance(long long* step, float* bias, double beta1, double beta2, hipStream_t s) {
  hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, s, step, bias, beta1, beta2);
  CTDET_LAUNCH_CHECK();
  return 0;
}

struct AdamScalars {
  float b1, omb1, b2, omb2, eps, clip_value;
};

// The layout of sgd_runs_body: a workgroup owns a contiguous range, a thread walks it four elements at a time, the run lookup
// happens when a thread leaves its run, element-wise at run ends.  Streams per element: p, g, m, v read and p, m, v written
// (28 B), AMSGrad one more of each (36 B).
template <int CLIP, bool DECOUPLED, bool AMSGRAD>
__global__ void __launch_bounds__(256) adam_runs_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, float* __restrict__ vmax, long n,
                                                        const long* __restrict__ run_end, const int* __restrict__ run_lr_index,
                                                        const float* __restrict__ run_wd, const float* __restrict__ lr_table,
                                                        int nruns, const float* __restrict__ bias, AdamScalars a,
                                                        const float* __restrict__ coefs) {
  const long per = (((n + gridDim.x - 1) / gridDim.x) + 1023) & ~1023L;
  const long beg = (long)blockIdx.x * per, end = beg + per < n ? beg + per : n;
  const float ibc1 = bias[0], ibc2s = bias[1];
  long cur_end = -1;
  float step = 0.f, wd = 0.f, keep = 1.f, cf = 1.f;
  auto lookup = [&](long i) {
    int lo = 0, hi = nruns - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (run_end[mid] > i) hi = mid; else lo = mid + 1;
    }
    cur_end = run_end[lo];
    const float lr = lr_table[run_lr_index[lo]];
    wd = run_wd[lo];
    step = lr * ibc1;
    if constexpr (DECOUPLED) keep = (float)(1.0 - (double)lr * (double)wd);   // torch: 1 - lr * weight_decay in f64, rounded once
    if constexpr (CLIP == SGD_CLIP_NORM) cf = coefs[lo];
  };
  // one element: gi, pi, mi, vi, xi (the running maximum) in, the new values out
  auto update = [&](float gi, float& pi, float& mi, float& vi, float& xi) {
    if constexpr (CLIP == SGD_CLIP_VALUE) gi = gi > a.clip_value ? a.clip_value : (gi < -a.clip_value ? -a.clip_value : gi);  // NaN stays
    if constexpr (CLIP == SGD_CLIP_NORM) gi = gi * cf;
    if constexpr (DECOUPLED) pi = pi * keep;
    else if (wd != 0.f) gi = gi + wd * pi;
    mi = a.b1 * mi + a.omb1 * gi;
    vi = a.b2 * vi + a.omb2 * gi * gi;
    float vh = vi;
    if constexpr (AMSGRAD) vh = xi = (vi > xi || vi != vi) ? vi : xi;        // torch.maximum: a NaN on either side stays
    const float denom = sqrtf(vh) * ibc2s + a.eps;
    pi = pi - step * (mi / denom);
  };
  for (long i = beg + (long)threadIdx.x * 4; i < end; i += 1024) {
    if (i >= cur_end) lookup(i);
    if (i + 4 <= cur_end && i + 4 <= end) {
      const float4 gv = *(const float4*)(g + i), pv = *(const float4*)(p + i), mv = *(const float4*)(m + i),
                   vv = *(const float4*)(v + i);
      float4 xv = {0.f, 0.f, 0.f, 0.f};
      if constexpr (AMSGRAD) xv = *(const float4*)(vmax + i);
      const float ge[4] = {gv.x, gv.y, gv.z, gv.w};
      float pe[4] = {pv.x, pv.y, pv.z, pv.w}, me[4] = {mv.x, mv.y, mv.z, mv.w}, ve[4] = {vv.x, vv.y, vv.z, vv.w},
            xe[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) update(ge[k], pe[k], me[k], ve[k], xe[k]);
      *(float4*)(m + i) = make_float4(me[0], me[1], me[2], me[3]);
      *(float4*)(v + i) = make_float4(ve[0], ve[1], ve[2], ve[3]);
      if constexpr (AMSGRAD) *(float4*)(vmax + i) = make_float4(xe[0], xe[1], xe[2], xe[3]);
      *(float4*)(p + i) = make_float4(pe[0], pe[1], pe[2], pe[3]);
    } else {
      for (long j = i; j < i + 4 && j < end; ++j) {
        if (j >= cur_end) lookup(j);
        float pi = p[j], mi = m[j], vi = v[j], xi = 0.f;
        if constexpr (AMSGRAD) xi = vmax[j];
        update(g[j], pi, mi, vi, xi);
        m[j] = mi;
        v[j] = vi;
        if constexpr (AMSGRAD) vmax[j] = xi;
        p[j] = pi;
      }
    }
  }
}

int launch_adam_runs(float* p, const float* g, float* m, float* v, float* vmax, long n, const long* run_end,
                     const int* run_lr_index, const float* run_wd, const float* lr_table, int nruns, const float* bias,
                     double beta1, double beta2, double eps, int decoupled, int amsgrad, int clip_type, float clip_value,
                     const float* coefs, hipStream_t s) {
  if (n == 0 || nruns == 0) return 0;
  long nb = (n + 1023) / 1024;
  if (nb > 2048) nb = 2048;
  // torch hands (1 - beta) to its kernels as an f64 scalar rounded to f32 once: 1.f - (float)beta2 would be 4.7e-5 off
  const AdamScalars a = {(float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, clip_value};
#define ADAM_CASE(C, D, A)                                                                                             \
  if (clip_type == C && (decoupled != 0) == D && (amsgrad != 0) == A)                                                  \
    hipLaunchKernelGGL((adam_runs_kernel<C, D, A>), dim3((unsigned)nb), dim3(256), 0, s, p, g, m, v, vmax, n, run_end, \
                       run_lr_index, run_wd, lr_table, nruns, bias, a, coefs)
#define ADAM_CLIP_CASES(C) \
  ADAM_CASE(C, false, false); ADAM_CASE(C, false, true); ADAM_CASE(C, true, false); ADAM_CASE(C, true, true)
  ADAM_CLIP_CASES(SGD_CLIP_NONE);
  ADAM_CLIP_CASES(SGD_CLIP_VALUE);
  ADAM_CLIP_CASES(SGD_CLIP_NORM);
#undef ADAM_CLIP_CASES
#undef ADAM_CASE
  CTDET_LAUNCH_CHECK();
  return 0;
}
