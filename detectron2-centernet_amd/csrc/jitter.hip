// The training mapper's four colour jitters on the device, byte for byte what the host computes (data/transforms.py:
// RandomContrast, RandomBrightness, RandomSaturation, RandomLighting, each a BlendTransform on the uint8 output of the one
// before; data/jitter.py holds the arithmetic restated in numpy).  Per byte of a drawn transform
//   out = trunc(clip(f64(ws) *f64 src  +f64  f64(f32(wd) *f32 f32(byte)), 0, 255))
// with src = the image mean (contrast), 0 (brightness), the pixel's grey value (saturation) or a per-channel offset
// (lighting, ws = wd = 1).  Every product and sum is rounded on its own: this file is compiled with -ffp-contract=off
// (csrc/Makefile) -- a fused multiply-add rounds once where numpy rounds twice, and that changes bytes.
//
// Two kernels over one descriptor table.  A block is JITTER_TW x JITTER_TH threads on a tile of that many pixels; a thread owns
// one pixel, all three channels (saturation mixes them).
//   byte_sum_u8_batch_kernel      adds the bytes of every image that has a sum slot (contrast drawn) into its uint64 slot:
//                                 64 blocks per image stride over its tiles, wave and block reduction, one 64-bit atomic per
//                                 block.  Integer, so exact and independent of order.
//   colour_jitter_u8_batch_kernel one block per tile, its image found by bisection over blk0; applies the drawn transforms in
//                                 order, in place, rounding to a byte between them; the contrast mean is f64(sum) / f64(3 h w),
//                                 formed here from the slot.  No LDS.
// Addressing is base + row * row_stride + column * pix_stride + channel * chan_stride in bytes, as in resize.hip: planes, a
// window of a staging batch and interleaved pixels are one code path.  Only the h x w x 3 bytes of a window are touched.
#include "common.h"
#include "../../include/ctdet_hip.h"

#define JITTER_TW 64        // pixel columns of a block (tests/jitter_cases.py: TILE_W)
#define JITTER_TH 4         // pixel rows of a block (tests/jitter_cases.py: TILE_H); a block is JITTER_TH waves of 64
#define JITTER_SUM_BLOCKS 64      // blocks that share the tiles of one image in the byte sum

typedef ctdet_jitter_desc JitterDesc;

// the block's descriptor and its pixel; false: nothing to do for this thread
__device__ __forceinline__ bool jitter_locate(const JitterDesc* __restrict__ descs, int n, const JitterDesc*& d, int& x, int& y) {
  const int b = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].blk0 <= b) lo = mid; else hi = mid - 1;
  }
  d = descs + lo;
  const int tiles_x = (d->w + JITTER_TW - 1) / JITTER_TW;
  const int tile = b - d->blk0;
  x = (tile % tiles_x) * JITTER_TW + (int)(threadIdx.x % JITTER_TW);
  y = (tile / tiles_x) * JITTER_TH + (int)(threadIdx.x / JITTER_TW);
  return tile >= 0 && x < d->w && y < d->h;      // y >= h also covers a table whose blk0 leave a gap
}

// JITTER_SUM_BLOCKS blocks per descriptor walk its tiles with that stride; a descriptor without a slot costs blocks that leave
// at once.  One 64-bit atomic per block: per wave one every tile was measured first and is what the time went into (16 images
// of 512 x 683: 90 k atomics on one cache line, 876 us).
__global__ __launch_bounds__(JITTER_TW * JITTER_TH) void byte_sum_u8_batch_kernel(const JitterDesc* __restrict__ descs, int n,
                                                                                   unsigned long long* __restrict__ sums, int n_sums) {
  __shared__ unsigned long long part[JITTER_TH];      // one partial per wave
  const JitterDesc* d = descs + blockIdx.x / JITTER_SUM_BLOCKS;
  const int slot = d->sum_slot;      // uniform over the block
  if (slot < 0 || slot >= n_sums) return;      // no slot: contrast not drawn; a slot outside the buffer is never touched
  const int tiles_x = (d->w + JITTER_TW - 1) / JITTER_TW, tiles_y = (d->h + JITTER_TH - 1) / JITTER_TH;
  const int tx = threadIdx.x % JITTER_TW, ty = threadIdx.x / JITTER_TW;
  const long cs = d->chan;
  unsigned long long s = 0;      // 64-bit from the start: no image size can wrap it
  for (int tile = blockIdx.x % JITTER_SUM_BLOCKS; tile < tiles_x * tiles_y; tile += JITTER_SUM_BLOCKS) {
    const int x = (tile % tiles_x) * JITTER_TW + tx, y = (tile / tiles_x) * JITTER_TH + ty;
    if (x < d->w && y < d->h) {
      const uint8_t* p = (const uint8_t*)d->img + (long)y * d->row + (long)x * d->pix;
      s += (unsigned int)p[0] + (unsigned int)p[cs] + (unsigned int)p[2 * cs];
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
#pragma unroll
    for (int i = 0; i < JITTER_TH; ++i) t += part[i];
    if (t) atomicAdd(sums + slot, t);
  }
}

__device__ __forceinline__ int jitter_blend(double ws, double src, float wd, int byte) {
  const float f = wd * (float)byte;                 // float32 product ...
  double v = ws * src + (double)f;                  // ... widened; one float64 product, one float64 add (never fused)
  v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
  return (int)v;                                    // truncation toward zero
}

__global__ __launch_bounds__(JITTER_TW * JITTER_TH) void colour_jitter_u8_batch_kernel(const JitterDesc* __restrict__ descs, int n,
                                                                                        const unsigned long long* __restrict__ sums, int n_sums) {
  const JitterDesc* d;
  int x, y;
  if (!jitter_locate(descs, n, d, x, y)) return;
  uint8_t* p = (uint8_t*)d->img + (long)y * d->row + (long)x * d->pix;
  const long cs = d->chan;
  int c0 = p[0], c1 = p[cs], c2 = p[2 * cs];
  if (d->on[0] && (unsigned)d->sum_slot < (unsigned)n_sums) {      // contrast: the mean of the image as it arrived
    const double mean = (double)sums[d->sum_slot] / (double)(3ll * d->h * d->w);
    const double ws = d->contrast[0];
    const float wd = (float)d->contrast[1];
    c0 = jitter_blend(ws, mean, wd, c0); c1 = jitter_blend(ws, mean, wd, c1); c2 = jitter_blend(ws, mean, wd, c2);
  }
  if (d->on[1]) {            // brightness: blend with black
    const double ws = d->brightness[0];
    const float wd = (float)d->brightness[1];
    c0 = jitter_blend(ws, 0.0, wd, c0); c1 = jitter_blend(ws, 0.0, wd, c1); c2 = jitter_blend(ws, 0.0, wd, c2);
  }
  if (d->on[2]) {            // saturation: blend with the pixel's grey value, channels in stored order
    const double grey = ((double)c0 * 0.299 + (double)c1 * 0.587) + (double)c2 * 0.114;
    const double ws = d->saturation[0];
    const float wd = (float)d->saturation[1];
    c0 = jitter_blend(ws, grey, wd, c0); c1 = jitter_blend(ws, grey, wd, c1); c2 = jitter_blend(ws, grey, wd, c2);
  }
  if (d->on[3]) {            // lighting: per-channel offset, weights 1 and 1
    c0 = jitter_blend(1.0, d->lighting[0], 1.f, c0);
    c1 = jitter_blend(1.0, d->lighting[1], 1.f, c1);
    c2 = jitter_blend(1.0, d->lighting[2], 1.f, c2);
  }
  p[0] = (uint8_t)c0; p[cs] = (uint8_t)c1; p[2 * cs] = (uint8_t)c2;
}

int jitter_tiles(int h, int w) {
  return ((w + JITTER_TW - 1) / JITTER_TW) * ((h + JITTER_TH - 1) / JITTER_TH);
}

int launch_byte_sum_u8_batch(const ctdet_jitter_desc* descs_dev, int n, uint64_t* sums, int n_sums, hipStream_t s) {
  CTDET_KERNEL("byte_sum_u8_batch_kernel");
  const hipError_t e = hipMemsetAsync(sums, 0, (size_t)n_sums * sizeof(uint64_t), s);
  if (e != hipSuccess) {
    ctdet_set_error("byte_sum_u8_batch: clearing the sums failed: %s", hipGetErrorString(e));
    return -5;
  }
  if (n == 0) return 0;      // no image to sum: the slots stay 0
  hipLaunchKernelGGL(byte_sum_u8_batch_kernel, dim3(n * JITTER_SUM_BLOCKS), dim3(JITTER_TW * JITTER_TH), 0, s, descs_dev, n,
                     (unsigned long long*)sums, n_sums);
  CTDET_LAUNCH_CHECK();
  return 0;
}

int launch_colour_jitter_u8_batch(const ctdet_jitter_desc* descs_dev, int n, int total_blocks, const uint64_t* sums, int n_sums,
                                  hipStream_t s) {
  CTDET_KERNEL("colour_jitter_u8_batch_kernel");
  hipLaunchKernelGGL(colour_jitter_u8_batch_kernel, dim3(total_blocks), dim3(JITTER_TW * JITTER_TH), 0, s, descs_dev, n,
                     (const unsigned long long*)sums, n_sums);
  CTDET_LAUNCH_CHECK();
  return 0;
}
