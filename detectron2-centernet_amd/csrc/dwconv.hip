// Depthwise 3x3 convolution (Conv2d(C, C, 3, stride, 1, groups=C, bias=False)) of the depthwise VoVNet bodies
// (`V-19-slim-dw-eSE`, `V-19-dw-eSE`: the dw_conv3x3 layers of their stem and OSA modules), forward and backward.
//
//   dwconv3x3_kernel                : y = dwconv(x, w), stride 1 or 2, pad 1; with rot180 the taps are read rotated by 180
//                                     degrees, which makes the same kernel the input gradient of a stride-1 layer
//                                     (dX = dwconv(dY, rot180(W)), pad 1)
//   dwconv3x3_wgrad_kernel          : per-workgroup f32 partial sums of dW[c][t] = sum over n, y, x of dY * X(shifted by tap t)
//   dwconv3x3_wgrad_finalize_kernel : the partials summed in a fixed order in f64, scaled, written to / added into the
//                                     parameter's OIHW [C,1,3,3] gradient
//
// NHWC activations (pixel rows of `*_stride` elements, so a layer may read or write a channel slice of a wider buffer), f32 or
// f16 (f32 accumulation); weights f32 tap-major [9][C], t = ky*3 + kx.  Nine FMAs per output element and no channel
// contraction: the forward and the input gradient are bound by HBM, not by arithmetic.  Every tap sum runs in the same order
// (ky-major, then kx) and the weight gradient uses no atomics, so results do not change from run to run.
#include "common.h"

namespace {

template <typename T> struct DwVec;
template <> struct DwVec<f16> { typedef f16x8 type; static constexpr int N = 8; };
template <> struct DwVec<float> { typedef f32x4 type; static constexpr int N = 4; };

// A thread owns one (output column, 16-byte channel vector) and walks DW3_ROWS output rows with a rolling window of three
// input rows x three columns in registers (stride 1: one new input row per output row; stride 2: two), its nine taps in
// registers too.  Neighbouring lanes share the window's side columns through L1.
constexpr int DW3_ROWS = 4;

template <typename T, int S>
__global__ void __launch_bounds__(256) dwconv3x3_kernel(const T* __restrict__ x, int x_stride, const float* __restrict__ w,
                                                        T* __restrict__ y, int y_stride, int H, int W, int Ho, int Wo, int C,
                                                        int nchunk, int rot180) {
  using V = typename DwVec<T>::type;
  constexpr int N = DwVec<T>::N;
  const int CV = C / N;
  const int chunk = blockIdx.y % nchunk;
  const int b = blockIdx.y / nchunk;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Wo * CV) return;
  const int ox = i / CV, cv = i - ox * CV;
  float wt[9][N];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const float* wp = w + (long)(rot180 ? 8 - t : t) * C + cv * N;
#pragma unroll
    for (int e4 = 0; e4 < N; e4 += 4) {
      const f32x4 wv = *(const f32x4*)(wp + e4);
#pragma unroll
      for (int e = 0; e < 4; ++e) wt[t][e4 + e] = wv[e];
    }
  }
  V zero;
#pragma unroll
  for (int e = 0; e < N; ++e) zero[e] = (T)0.f;
  const int ix0 = ox * S - 1;                 // columns ix0, ix0 + 1 (always inside: ox * S <= W - 1), ix0 + 2
  const bool cl = ix0 >= 0, cr = ix0 + 2 < W;
  const T* xc = x + (long)b * H * W * x_stride + (long)(ox * S) * x_stride + cv * N;
  auto load_row = [&](int iy, V* v) {
    const bool rin = iy >= 0 && iy < H;
    const T* xr = xc + (long)iy * W * x_stride;
    v[0] = (rin && cl) ? *(const V*)(xr - x_stride) : zero;
    v[1] = rin ? *(const V*)xr : zero;
    v[2] = (rin && cr) ? *(const V*)(xr + x_stride) : zero;
  };
  const int oy0 = chunk * DW3_ROWS;
  V r0[3], r1[3], r2[3];                      // input rows oy*S - 1, oy*S, oy*S + 1
  load_row(oy0 * S - 1, r0);
  load_row(oy0 * S, r1);
  load_row(oy0 * S + 1, r2);
  T* yc = y + (long)b * Ho * Wo * y_stride + (long)ox * y_stride + cv * N;
#pragma unroll
  for (int r = 0; r < DW3_ROWS; ++r) {
    const int oy = oy0 + r;
    if (oy >= Ho) break;
    if (r > 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        r0[k] = S == 1 ? r1[k] : r2[k];
        if (S == 1) r1[k] = r2[k];
      }
      if (S == 2) load_row(oy * 2, r1);
      load_row(oy * S + 1, r2);
    }
    V out;
#pragma unroll
    for (int e = 0; e < N; ++e) {
      float acc = (float)r0[0][e] * wt[0][e];
      acc = fmaf((float)r0[1][e], wt[1][e], acc);
      acc = fmaf((float)r0[2][e], wt[2][e], acc);
      acc = fmaf((float)r1[0][e], wt[3][e], acc);
      acc = fmaf((float)r1[1][e], wt[4][e], acc);
      acc = fmaf((float)r1[2][e], wt[5][e], acc);
      acc = fmaf((float)r2[0][e], wt[6][e], acc);
      acc = fmaf((float)r2[1][e], wt[7][e], acc);
      acc = fmaf((float)r2[2][e], wt[8][e], acc);
      out[e] = (T)acc;
    }
    *(V*)(yc + (long)oy * Wo * y_stride) = out;
  }
}

// Weight gradient, stage 1.  A tile is WG3_ROWS rows x XL columns of one image (XL = 256 / (C / N) lanes of a workgroup per
// row); workgroup g takes tiles g, g + G, g + 2G, ... (a fixed assignment).  A lane accumulates its column's nine tap
// products in f32 registers while it walks the tile's rows with the same rolling window as the forward kernel, then the
// workgroup adds its lanes through LDS (one tap at a time, lanes in ascending order) and writes its own slot ws[g][c*9 + t].
// Every slot is written on every launch -- also by a workgroup without a tile -- so the workspace is never cleared.
constexpr int WG3_ROWS = 16;
constexpr int WG3_MAX_GROUPS = 1024;

template <typename T>
__global__ void __launch_bounds__(256) dwconv3x3_wgrad_kernel(const T* __restrict__ x, int x_stride, const T* __restrict__ dy,
                                                              int dy_stride, float* __restrict__ ws, int H, int W, int C, int XL,
                                                              int ncol, int nstrip, int ntiles) {
  using V = typename DwVec<T>::type;
  constexpr int N = DwVec<T>::N;
  extern __shared__ float red[];              // [XL][C]
  const int CV = C / N;
  const int tid = threadIdx.x;
  const int xl = tid / CV, cv = tid - xl * CV;
  const bool lane_on = xl < XL;
  float acc[9][N];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < N; ++e) acc[t][e] = 0.f;
  V zero;
#pragma unroll
  for (int e = 0; e < N; ++e) zero[e] = (T)0.f;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int col = tile % ncol;
    const int strip = (tile / ncol) % nstrip;
    const int b = tile / (ncol * nstrip);
    const int xo = col * XL + xl;
    if (!lane_on || xo >= W) continue;
    const bool cl = xo >= 1, cr = xo + 1 < W;
    const T* xc = x + (long)b * H * W * x_stride + (long)xo * x_stride + cv * N;
    const T* dc = dy + (long)b * H * W * dy_stride + (long)xo * dy_stride + cv * N;
    auto load_row = [&](int iy, V* v) {
      const bool rin = iy >= 0 && iy < H;
      const T* xr = xc + (long)iy * W * x_stride;
      v[0] = (rin && cl) ? *(const V*)(xr - x_stride) : zero;
      v[1] = rin ? *(const V*)xr : zero;
      v[2] = (rin && cr) ? *(const V*)(xr + x_stride) : zero;
    };
    const int y0 = strip * WG3_ROWS;
    V r[3][3];
    load_row(y0 - 1, r[0]);
    load_row(y0, r[1]);
#pragma unroll 2
    for (int k = 0; k < WG3_ROWS; ++k) {
      const int yy = y0 + k;
      if (yy >= H) break;
      if (k > 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { r[0][j] = r[1][j]; r[1][j] = r[2][j]; }
      }
      load_row(yy + 1, r[2]);
      const V g = *(const V*)(dc + (long)yy * W * dy_stride);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int e = 0; e < N; ++e) acc[ky * 3 + kx][e] = fmaf((float)g[e], (float)r[ky][kx][e], acc[ky * 3 + kx][e]);
    }
  }
  float* slot = ws + (long)blockIdx.x * 9 * C;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    __syncthreads();
    if (lane_on) {
#pragma unroll
      for (int e4 = 0; e4 < N; e4 += 4) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[t][e4 + e];
        *(f32x4*)(red + xl * C + cv * N + e4) = v;
      }
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
      float s = 0.f;
      for (int l = 0; l < XL; ++l) s += red[l * C + c];
      slot[c * 9 + t] = s;
    }
  }
}

// Weight gradient, stage 2: dw[o] (+)= scale * sum over g of ws[g][o], o = c*9 + t (the OIHW order of [C,1,3,3]).  64 outputs
// per workgroup, four lanes per output each summing every fourth slot in ascending order in f64, the four sums added in a
// fixed order.
__global__ void __launch_bounds__(256) dwconv3x3_wgrad_finalize_kernel(const float* __restrict__ ws, int G, int n,
                                                                       float* __restrict__ dw, float scale, int accumulate) {
  __shared__ double part[4][64];
  const int lane = threadIdx.x & 63, gl = threadIdx.x >> 6;
  const int o = blockIdx.x * 64 + lane;
  double s = 0.0;
  if (o < n) {
    int g = gl;
    for (; g + 12 < G; g += 16) {
      const float a0 = ws[(long)g * n + o], a1 = ws[(long)(g + 4) * n + o];
      const float a2 = ws[(long)(g + 8) * n + o], a3 = ws[(long)(g + 12) * n + o];
      s += (double)a0;
      s += (double)a1;
      s += (double)a2;
      s += (double)a3;
    }
    for (; g < G; g += 4) s += (double)ws[(long)g * n + o];
  }
  part[gl][lane] = s;
  __syncthreads();
  if (gl == 0 && o < n) {
    const double tot = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    const float v = (float)(tot * (double)scale);
    dw[o] = accumulate ? dw[o] + v : v;
  }
}

struct WgradGeom {
  int XL, ncol, nstrip, ntiles, G;
};

WgradGeom wgrad_geom(int B, int H, int W, int C, int N) {
  WgradGeom g;
  g.XL = 256 / (C / N);
  g.ncol = (W + g.XL - 1) / g.XL;
  g.nstrip = (H + WG3_ROWS - 1) / WG3_ROWS;
  const long nt = (long)B * g.ncol * g.nstrip;
  g.ntiles = (int)nt;
  g.G = (int)(nt < WG3_MAX_GROUPS ? nt : WG3_MAX_GROUPS);
  return g;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int dwconv3x3_check(int dtype, int B, int H, int W, int C, int stride, const int* strides, int nstrides) {
  CTDET_CHECK(dtype == CTDET_F16 || dtype == CTDET_F32, "dwconv3x3: dtype %d (f16 or f32 tensors)", dtype);
  CTDET_CHECK(stride == 1 || stride == 2, "dwconv3x3: stride %d (1 or 2)", stride);
  CTDET_CHECK(B >= 0 && H >= 0 && W >= 0 && C > 0, "dwconv3x3: bad shape B=%d H=%d W=%d C=%d", B, H, W, C);
  const int N = dtype == CTDET_F16 ? 8 : 4;
  CTDET_CHECK(C % N == 0, "dwconv3x3: channels %d must be a multiple of %d", C, N);
  CTDET_CHECK(C / N <= 256, "dwconv3x3: channels %d above %d", C, 256 * N);
  for (int k = 0; k < nstrides; ++k)
    CTDET_CHECK(strides[k] >= C && strides[k] % N == 0, "dwconv3x3: pixel stride %d must be >= C and a multiple of %d",
                strides[k], N);
  return 0;
}

size_t dwconv3x3_wgrad_workspace_bytes(int B, int H, int W, int C, int dtype) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
  const int N = dtype == CTDET_F16 ? 8 : 4;
  if (C % N != 0 || C / N > 256) return 0;
  return (size_t)wgrad_geom(B, H, W, C, N).G * 9 * C * sizeof(float);
}

int launch_dwconv3x3(const void* x, int x_stride, const float* w, void* y, int y_stride, int B, int H, int W, int C, int stride,
                     int rot180, int dtype, hipStream_t s) {
  CTDET_CHECK(aligned16(x) && aligned16(w) && aligned16(y), "dwconv3x3: tensors must be 16-byte aligned");
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  if (B == 0 || H == 0 || W == 0) return 0;
  const int N = dtype == CTDET_F16 ? 8 : 4;
  const int nchunk = (Ho + DW3_ROWS - 1) / DW3_ROWS;
  const long gy = (long)B * nchunk;
  CTDET_CHECK(gy <= 65535, "dwconv3x3: batch x row strips %ld above 65535", gy);
  const dim3 grid((unsigned)(((long)Wo * (C / N) + 255) / 256), (unsigned)gy);
#define DW3(T, S_)                                                                                                        \
  hipLaunchKernelGGL((dwconv3x3_kernel<T, S_>), grid, dim3(256), 0, s, (const T*)x, x_stride, w, (T*)y, y_stride, H, W, Ho, \
                     Wo, C, nchunk, rot180)
  if (dtype == CTDET_F16) { if (stride == 1) DW3(f16, 1); else DW3(f16, 2); }
  else if (dtype == CTDET_F32) { if (stride == 1) DW3(float, 1); else DW3(float, 2); }
  else CTDET_CHECK(false, "dwconv3x3: bad dtype %d", dtype);
#undef DW3
  CTDET_LAUNCH_CHECK();
  return 0;
}

int launch_dwconv3x3_wgrad(const void* x, int x_stride, const void* dy, int dy_stride, float* ws, float* dw, float scale,
                           int accumulate, int B, int H, int W, int C, int dtype, hipStream_t s) {
  CTDET_CHECK(aligned16(x) && aligned16(dy), "dwconv3x3_wgrad: activations must be 16-byte aligned");
  const int N = dtype == CTDET_F16 ? 8 : 4;
  const int n = 9 * C;
  const WgradGeom g = wgrad_geom(B, H, W, C, N);
  if (g.G > 0) {
    const size_t lds = (size_t)g.XL * C * sizeof(float);
    if (dtype == CTDET_F16)
      hipLaunchKernelGGL(dwconv3x3_wgrad_kernel<f16>, dim3((unsigned)g.G), dim3(256), lds, s, (const f16*)x, x_stride,
                         (const f16*)dy, dy_stride, ws, H, W, C, g.XL, g.ncol, g.nstrip, g.ntiles);
    else if (dtype == CTDET_F32)
      hipLaunchKernelGGL(dwconv3x3_wgrad_kernel<float>, dim3((unsigned)g.G), dim3(256), lds, s, (const float*)x, x_stride,
                         (const float*)dy, dy_stride, ws, H, W, C, g.XL, g.ncol, g.nstrip, g.ntiles);
    else CTDET_CHECK(false, "dwconv3x3_wgrad: bad dtype %d", dtype);
    CTDET_LAUNCH_CHECK();
  }
  // an empty problem still writes dw (zeros, or leaves the accumulated gradient as it is)
  hipLaunchKernelGGL(dwconv3x3_wgrad_finalize_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, s, ws, g.G, n, dw, scale,
                     accumulate);
  CTDET_LAUNCH_CHECK();
  return 0;
}
