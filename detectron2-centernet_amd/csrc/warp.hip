// 8-bit bilinear affine warp of 3-channel images on the device, byte for byte what data/warp.py computes on the host
// (warp_affine_u8_reference: the arithmetic, and warp_tables: the four int32 tables the host builds from the inverse matrix).
// Destination pixel (x, y) reads the source at the 10-bit fixed-point coordinate (x0[y] + ax[x], y0[y] + bx[x]): its low 5
// bits are dropped, the next 5 are the phase, the rest is the first tap; four taps with weights that sum to 1 << 15, a tap
// outside the source contributes 0, the sum is rounded and shifted right by 15.  Integer throughout.
//
// Streaming form, the shape of resize.hip: no LDS, no barrier, one kernel for every map.  A block of 192 threads owns WARP_TW
// output columns x 3 channels x WARP_RB output rows; a thread owns one (column, channel), reads its two column table entries
// once and walks its rows.  The row table entries are the same for the whole block (scalar loads).
//
// All addressing goes through byte strides (row, pixel, channel) of source and destination, of either sign, so HWC and CHW
// images, a reversed channel order, a mirrored source (pixel stride negated from the last column) and a destination window
// inside a larger buffer are one code path.  Only bytes of the [out_h, out_w] window are written.  Every tap coordinate is
// clamped into the source before its load, whatever the tables hold: a stale table gives wrong bytes, never a fault.
#include "common.h"
#include "../../include/ctdet_hip.h"

#define WARP_TW 64          // output columns of a block (tests/warp_cases.py: COL_TILE)
#define WARP_RB 8           // output rows of a block
#define WARP_DROP 5         // low coordinate bits dropped: 10 fixed-point bits -> 5 phase bits
#define WARP_PHASE 5
#define WARP_SHIFT 15       // the weights of a pixel sum to 1 << 15

typedef ctdet_warp_desc WarpDesc;

__host__ __device__ __forceinline__ int warp_tiles_of(int out_h, int out_w) {
  return out_h < 1 || out_w < 1 ? 0 : ((out_w + WARP_TW - 1) / WARP_TW) * ((out_h + WARP_RB - 1) / WARP_RB);
}

__device__ __forceinline__ void warp_tile(const WarpDesc& d, const int* __restrict__ tab, int tile) {
  const int tiles_x = (d.out_w + WARP_TW - 1) / WARP_TW;
  const int r0 = (tile / tiles_x) * WARP_RB;
  const int t = threadIdx.x;
  // lanes run along the axis the SOURCE holds densest: channel first for interleaved pixels, column first for planes
  const bool chan_fast = (d.src_chan < 0 ? -d.src_chan : d.src_chan) < (d.src_pix < 0 ? -d.src_pix : d.src_pix);
  const int c = chan_fast ? t % 3 : t / WARP_TW;
  const int x = (tile % tiles_x) * WARP_TW + (chan_fast ? t / 3 : t % WARP_TW);
  if (x >= d.out_w) return;      // no barrier below

  const long ax = tab[d.ax + x], bx = tab[d.bx + x];      // x < out_w: inside the table
  const uint8_t* sp = (const uint8_t*)d.src + (long)c * d.src_chan;
  uint8_t* dp = (uint8_t*)d.dst + (long)c * d.dst_chan + (long)x * d.dst_pix;
  const int rows = min(WARP_RB, d.out_h - r0);
  // rows one after the other: gathering the loads of all WARP_RB rows first (126 registers, half the waves) measured
  // 41 us against 34 us for a batch of 16 at 512 x 512
  for (int j = 0; j < rows; ++j) {
    const int y = r0 + j;      // y < out_h: inside the table
    // the two entries are added in 64 bits: each is an int32, their sum need not be
    const long X = ((long)tab[d.x0 + y] + ax) >> WARP_DROP, Y = ((long)tab[d.y0 + y] + bx) >> WARP_DROP;
    const long sx = X >> WARP_PHASE, sy = Y >> WARP_PHASE;
    const int fx = (int)(X & ((1 << WARP_PHASE) - 1)), fy = (int)(Y & ((1 << WARP_PHASE) - 1));
    // a tap outside [0, H) x [0, W) weighs 0; its address is clamped into the source all the same
    const int wx0 = (sx >= 0 && sx < d.W) ? 32 - fx : 0, wx1 = (sx + 1 >= 0 && sx + 1 < d.W) ? fx : 0;
    const int wy0 = (sy >= 0 && sy < d.H) ? 32 - fy : 0, wy1 = (sy + 1 >= 0 && sy + 1 < d.H) ? fy : 0;
    const long cx0 = max(0L, min(sx, (long)d.W - 1)), cx1 = max(0L, min(sx + 1, (long)d.W - 1));
    const long cy0 = max(0L, min(sy, (long)d.H - 1)), cy1 = max(0L, min(sy + 1, (long)d.H - 1));
    const uint8_t* ra = sp + cy0 * d.src_row;
    const uint8_t* rb = sp + cy1 * d.src_row;
    int acc = 1 << (WARP_SHIFT - 1);
    if ((wx0 | wx1) && (wy0 | wy1)) {      // a pixel whose taps all lie outside reads nothing
      const int p00 = ra[cx0 * d.src_pix], p01 = ra[cx1 * d.src_pix], p10 = rb[cx0 * d.src_pix], p11 = rb[cx1 * d.src_pix];
      acc += 32 * ((p00 * wx0 + p01 * wx1) * wy0 + (p10 * wx0 + p11 * wx1) * wy1);
    }
    dp[(long)y * d.dst_row] = (uint8_t)(acc >> WARP_SHIFT);
  }
}

// descs[n] sorted by blk0 (blk0 of image 0 is 0): the block finds its image by bisection
__global__ __launch_bounds__(WARP_TW * 3) void warp_affine_u8_batch_kernel(const WarpDesc* __restrict__ descs, int n,
                                                                           const int* __restrict__ tab) {
  const int b = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].blk0 <= b) lo = mid; else hi = mid - 1;
  }
  const WarpDesc d = descs[lo];
  if (b - d.blk0 < 0 || b - d.blk0 >= warp_tiles_of(d.out_h, d.out_w)) return;      // blocks the descriptors do not cover: nothing to do
  warp_tile(d, tab, b - d.blk0);
}

int warp_tiles(int out_h, int out_w) { return warp_tiles_of(out_h, out_w); }

int launch_warp_affine_u8_batch(const ctdet_warp_desc* descs_dev, int n, int total_blocks, const int* tab, hipStream_t s) {
  CTDET_KERNEL("warp_affine_u8_batch_kernel");
  hipLaunchKernelGGL(warp_affine_u8_batch_kernel, dim3(total_blocks), dim3(WARP_TW * 3), 0, s, descs_dev, n, tab);
  CTDET_LAUNCH_CHECK();
  return 0;
}
