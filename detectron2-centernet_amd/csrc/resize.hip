// Pillow's 8-bit bilinear resize of 3-channel images on the device, bit for bit (data/resample.py holds the arithmetic and
// builds the tables): a horizontal pass whose result is rounded and clipped to a byte, then a vertical pass over those bytes,
// both in int32 from 1 << 21, shifted right by 22.
//
// Streaming form, no LDS, no intermediate image, one kernel for every scale.  A block of 192 threads owns RESIZE_TW output
// columns x 3 channels x RESIZE_RB output rows; a thread owns one (column, channel) and the RESIZE_RB accumulators of its
// rows.  The block walks the source rows its output rows need, first to last -- any number of them: nothing is sized by the
// span.  Per source row a thread forms the horizontally resampled byte once and adds byte * vertical coefficient to the
// accumulators of the output rows whose bounds hold that row.  Row bounds and vertical coefficients are the same for the
// whole block (scalar loads, uniform branches); column bounds and horizontal coefficients are per thread and stay in
// registers when the row of the table has at most RESIZE_KREG entries (every upscale, downscales below 3.5x).
//
// All addressing goes through byte strides (row, pixel, channel) of source and destination, so HWC and CHW images, a
// reversed channel order (channel stride -1 from channel 2) and a destination window inside a larger buffer are one code
// path.  Only bytes of the [new_h, new_w] window are written.
#include "common.h"
#include "../../include/ctdet_hip.h"

#define RESIZE_TW 64        // output columns of a block (tests/resize_cases.py: COL_TILE)
#define RESIZE_RB 8         // output rows of a block
#define RESIZE_KREG 8       // longest horizontal coefficient row kept in registers
#define RESIZE_SHIFT 22     // Pillow's PRECISION_BITS for 8-bit channels

typedef ctdet_resize_desc ResizeDesc;

__device__ __forceinline__ int resize_clip8(int acc) {
  int v = acc >> RESIZE_SHIFT;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// KREG > 0: the thread's horizontal coefficients are in registers (kh <= KREG); 0: read from the table per source row
template <int KREG>
__device__ __forceinline__ void resize_tile(const ResizeDesc& d, const int* __restrict__ tab, int tile) {
  const int tiles_x = (d.new_w + RESIZE_TW - 1) / RESIZE_TW;
  const int r0 = (tile / tiles_x) * RESIZE_RB;
  const int t = threadIdx.x;
  // lanes run along the axis the SOURCE holds densest: channel first for interleaved pixels, column first for planes
  const bool chan_fast = (d.src_chan < 0 ? -d.src_chan : d.src_chan) < (d.src_pix < 0 ? -d.src_pix : d.src_pix);
  const int c = chan_fast ? t % 3 : t / RESIZE_TW;
  const int x = (tile % tiles_x) * RESIZE_TW + (chan_fast ? t / 3 : t % RESIZE_TW);
  if (x >= d.new_w) return;      // no barrier below

  // rows of this block: bounds clamped into the source (the tables are built that way; a stale table must not fault)
  int yfirst[RESIZE_RB], ycount[RESIZE_RB];
  int ylo = d.H, yhi = 0;
#pragma unroll
  for (int j = 0; j < RESIZE_RB; ++j) {
    const int r = r0 + j;
    int f = 0, n = 0;
    if (r < d.new_h) {
      if (d.kv > 0) { f = tab[d.vb + 2 * r]; n = tab[d.vb + 2 * r + 1]; }
      else { f = r; n = 1; }     // skipped vertical pass: output row r is source row r
      f = max(0, min(f, d.H));
      n = max(0, min(min(n, d.kv > 0 ? d.kv : 1), d.H - f));
      if (n > 0) { ylo = min(ylo, f); yhi = max(yhi, f + n); }
    }
    yfirst[j] = f; ycount[j] = n;
  }

  int xfirst = x, xcount = 1;
  const int* hco = nullptr;
  int cf[KREG > 0 ? KREG : 1];
  if (d.kh > 0) {
    xfirst = tab[d.hb + 2 * x]; xcount = tab[d.hb + 2 * x + 1];
    xfirst = max(0, min(xfirst, d.W));
    xcount = max(0, min(min(xcount, d.kh), d.W - xfirst));
    hco = tab + d.hc + (long)x * d.kh;
    if (KREG > 0) {
#pragma unroll
      for (int k = 0; k < KREG; ++k) cf[k] = k < xcount ? hco[k] : 0;
    }
  }
  const uint8_t* sp = (const uint8_t*)d.src + (long)c * d.src_chan + (long)xfirst * d.src_pix;

  int acc[RESIZE_RB];
#pragma unroll
  for (int j = 0; j < RESIZE_RB; ++j) acc[j] = 1 << (RESIZE_SHIFT - 1);

  for (int y = ylo; y < yhi; ++y) {
    const uint8_t* row = sp + (long)y * d.src_row;
    int h;
    if (d.kh == 0) {
      h = row[0];                // skipped horizontal pass
    } else {
      int s = 1 << (RESIZE_SHIFT - 1);
      if (KREG > 0) {
#pragma unroll
        for (int k = 0; k < KREG; ++k)
          if (k < xcount) s += (int)row[(long)k * d.src_pix] * cf[k];
      } else {
        for (int k = 0; k < xcount; ++k) s += (int)row[(long)k * d.src_pix] * hco[k];
      }
      h = resize_clip8(s);       // the intermediate image is uint8
    }
#pragma unroll
    for (int j = 0; j < RESIZE_RB; ++j) {
      const int k = y - yfirst[j];
      if ((unsigned)k < (unsigned)ycount[j])
        acc[j] += h * (d.kv > 0 ? tab[d.vc + (long)(r0 + j) * d.kv + k] : (1 << RESIZE_SHIFT));
    }
  }

  uint8_t* dp = (uint8_t*)d.dst + (long)c * d.dst_chan + (long)x * d.dst_pix;
#pragma unroll
  for (int j = 0; j < RESIZE_RB; ++j)
    if (r0 + j < d.new_h) dp[(long)(r0 + j) * d.dst_row] = (uint8_t)resize_clip8(acc[j]);
}

__device__ __forceinline__ void resize_dispatch(const ResizeDesc& d, const int* tab, int tile) {
  if (d.kh <= RESIZE_KREG) resize_tile<RESIZE_KREG>(d, tab, tile);
  else resize_tile<0>(d, tab, tile);
}

__global__ __launch_bounds__(RESIZE_TW * 3) void resize_bilinear_u8_kernel(const ResizeDesc d, const int* __restrict__ tab) {
  resize_dispatch(d, tab, blockIdx.x);
}

// descs[n] sorted by blk0 (blk0 of image 0 is 0): the block finds its image by bisection
__global__ __launch_bounds__(RESIZE_TW * 3) void resize_bilinear_u8_batch_kernel(const ResizeDesc* __restrict__ descs, int n,
                                                                                  const int* __restrict__ tab) {
  const int b = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].blk0 <= b) lo = mid; else hi = mid - 1;
  }
  const ResizeDesc d = descs[lo];
  const int tiles = ((d.new_w + RESIZE_TW - 1) / RESIZE_TW) * ((d.new_h + RESIZE_RB - 1) / RESIZE_RB);
  if (b - d.blk0 >= tiles) return;      // a table whose blk0 leave a gap: nothing to do there
  resize_dispatch(d, tab, b - d.blk0);
}

int resize_tiles(int new_h, int new_w) {
  return ((new_w + RESIZE_TW - 1) / RESIZE_TW) * ((new_h + RESIZE_RB - 1) / RESIZE_RB);
}

int launch_resize_u8(const ctdet_resize_desc& d, const int* tab, hipStream_t s) {
  CTDET_KERNEL("resize_bilinear_u8_kernel");
  hipLaunchKernelGGL(resize_bilinear_u8_kernel, dim3(resize_tiles(d.new_h, d.new_w)), dim3(RESIZE_TW * 3), 0, s, d, tab);
  CTDET_LAUNCH_CHECK();
  return 0;
}

int launch_resize_u8_batch(const ctdet_resize_desc* descs_dev, int n, int total_blocks, const int* tab, hipStream_t s) {
  CTDET_KERNEL("resize_bilinear_u8_batch_kernel");
  hipLaunchKernelGGL(resize_bilinear_u8_batch_kernel, dim3(total_blocks), dim3(RESIZE_TW * 3), 0, s, descs_dev, n, tab);
  CTDET_LAUNCH_CHECK();
  return 0;
}
