// Device helpers shared by the conv-shaped kernels (conv_igemm.hip: f16 MFMA path, conv_f32.hip: f32 MFMA path).
#pragma once
#include "common.h"
#include <type_traits>
#include <utility>
// slot permutation for 64-byte LDS rows read as 16-row fragments by ds_read_b128:
// rows r and r+4 share banks, so the 4 rows {r, r+4, r+8, r+12} get distinct slot XORs.
__device__ __forceinline__ int swz(int row) { return (0x78 >> (2 * ((row >> 2) & 3))) & 3; }
// byte offset of a lane's 16-byte fragment in such a tile of 16 rows: row lane % 16, k group lane / 16
__device__ __forceinline__ int swz_frag_off(int lane) { return (lane & 15) * 64 + (((lane >> 4) ^ swz(lane & 15)) << 4); }

// XCD-aware tile mapping (1-D grid of 8*mchunk*nby workgroups).  Workgroups are dealt round-robin over the 8
// XCDs, each with a private L2: XCD x gets the contiguous pixel-tile range [x*mchunk, (x+1)*mchunk) and walks it
// with the cout tile innermost, so workgroups that share an input tile (other cout tiles) or halo rows
// (neighbouring pixel tiles) run on the same L2 close in time.  Placement only affects speed, never results.
__device__ __forceinline__ bool tile_of_block(int nbx, int nby, int& m_tile, int& n_tile) {
  const int lin = blockIdx.x;
  const int xcd = lin & 7, sq = lin >> 3;
  const int mchunk = (nbx + 7) >> 3;
  n_tile = sq % nby;
  const int m_local = sq / nby;
  m_tile = xcd * mchunk + m_local;
  return m_local < mchunk && m_tile < nbx;
}

struct DcnSample {
  int off[4];    // element offsets of the 4 corner pixels (already * in_stride), -1 = contributes 0
  float wt[4];   // bilinear weights
  float mask;    // sigmoid(mask logit)
  f16 wm[4];     // f16(wt[q] * mask): the MFMA path blends in packed f16 (v_pk_fma_f16)
};

// Sampling geometry of one (pixel, tap); follows deform_conv_cuda_kernel.cu:836-861 and :666-699.
// NM (mask mode DCN_MASK_NONE): no mask channel is read, the mask is the constant 1.
template <bool NM = false>
__device__ __forceinline__ void dcn_setup(const ConvArgs& a, bool row_ok, int pix_base, int hb, int wb,
                                          int tr, int ts, const float* omrow, DcnSample& sp) {
  sp.off[0] = sp.off[1] = sp.off[2] = sp.off[3] = -1;
  sp.wt[0] = sp.wt[1] = sp.wt[2] = sp.wt[3] = 0.f;
  sp.wm[0] = sp.wm[1] = sp.wm[2] = sp.wm[3] = (f16)0.f;
  sp.mask = 0.f;
  if (!row_ok || tr >= a.R) return;
  const int tap = tr * a.S + ts;
  const float oh = omrow[2 * tap], ow = omrow[2 * tap + 1];
  if constexpr (NM) {
    sp.mask = 1.f;
  } else {
    const float mraw = omrow[2 * a.R * a.S + tap];
    sp.mask = a.mask_is_prob ? mraw : ctdet_sigmoid_exact(mraw);
  }
  const float h_im = (float)(hb + tr * a.dil) + oh;
  const float w_im = (float)(wb + ts * a.dil) + ow;
  if (!(h_im > -1.f && w_im > -1.f && h_im < (float)a.H && w_im < (float)a.W)) return;
  const int h_low = (int)floorf(h_im), w_low = (int)floorf(w_im);
  const int h_high = h_low + 1, w_high = w_low + 1;
  const float lh = h_im - (float)h_low, lw = w_im - (float)w_low;
  const float hh = 1.f - lh, hw = 1.f - lw;
  sp.wt[0] = hh * hw; sp.wt[1] = hh * lw; sp.wt[2] = lh * hw; sp.wt[3] = lh * lw;
#pragma unroll
  for (int q = 0; q < 4; ++q) sp.wm[q] = (f16)(sp.wt[q] * sp.mask);
  if (h_low >= 0 && w_low >= 0) sp.off[0] = (pix_base + h_low * a.W + w_low) * a.in_stride;
  if (h_low >= 0 && w_high <= a.W - 1) sp.off[1] = (pix_base + h_low * a.W + w_high) * a.in_stride;
  if (h_high <= a.H - 1 && w_low >= 0) sp.off[2] = (pix_base + h_high * a.W + w_low) * a.in_stride;
  if (h_high <= a.H - 1 && w_high <= a.W - 1) sp.off[3] = (pix_base + h_high * a.W + w_high) * a.in_stride;
}

// FIN epilogues (ConvArgs::finite, f32 outputs): the values a lane is about to store get the test of finite_flag_kernel
// (pointwise.hip) -- after scale, bias and activation, and only what reaches the tensor -- and a lane that holds a bad one
// clears the flag with an ordinary store, as that kernel does: the map needs no pass of its own
__device__ __forceinline__ void finite_note(const ConvArgs& a, const f32x4 v0, const f32x4 v1) {
  bool bad = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) bad |= !(fabsf(v0[j]) <= 3.402823466e38f) || !(fabsf(v1[j]) <= 3.402823466e38f);     // NaN compares false
  if (bad) *a.finite = 0;
}

template <typename TOut, bool FIN = false>
__device__ __forceinline__ void epilogue_store4(const ConvArgs& a, int m, int c, f32x4 v) {
  static_assert(!FIN || sizeof(TOut) == 4, "the finite test is made on f32 outputs");
  // c is a multiple of 4; Cout is a multiple of 4 (host guarantees), so a group is all-in or all-out
  if (c >= a.Cout) return;
  if (a.scale) { const f32x4 s = *(const f32x4*)(a.scale + c); v = v * s; }
  if (a.bias) { const f32x4 b = *(const f32x4*)(a.bias + c); v = v + b; }
  if (a.res) {
    const TOut* rp = (const TOut*)a.res + (long)m * a.res_stride + c;
    if constexpr (sizeof(TOut) == 2) {
      const f16x4 r = *(const f16x4*)rp;
      v[0] += (float)r[0]; v[1] += (float)r[1]; v[2] += (float)r[2]; v[3] += (float)r[3];
    } else {
      v = v + *(const f32x4*)rp;
    }
  }
  if (a.act == CTDET_ACT_RELU) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
  } else if (a.act == CTDET_ACT_SIGMOID_CLAMP) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = fminf(fmaxf(ctdet_sigmoid_exact(v[j]), a.clamp_lo), a.clamp_hi);
  }
  TOut* yp = (TOut*)a.y + (long)m * a.out_stride + c;
  if constexpr (sizeof(TOut) == 2) {
    f16x4 o; o[0] = (f16)v[0]; o[1] = (f16)v[1]; o[2] = (f16)v[2]; o[3] = (f16)v[3];
    *(f16x4*)yp = o;
  } else {
    if constexpr (FIN) finite_note(a, v, v);
    *(f32x4*)yp = v;
  }
}

// Cout (relative to the wave's first one) held in accumulator element i of cout tile c by the lanes of quad-group q
// (q = lane / 16).  Tiles pair up: a lane owns 8 consecutive couts per pair, so one 16-byte store per lane lets the
// four q-lanes of a pixel write 64 contiguous bytes (whole 32-byte sectors; the 8-byte pieces of the unpaired layout
// left every sector to be completed by four separate store instructions, and the store tail of a tile cost as much
// as a dozen K steps).  The weight loaders place LDS row (tile tt, row r) = cout_of(tt, r / 4, r % 4) to match.
template <int TC>
__device__ __forceinline__ constexpr int cout_of(int c, int q, int i) {
  if (TC % 2 == 0) return (c >> 1) * 32 + q * 8 + (c & 1) * 4 + i;
  return 4 * TC * q + 4 * c + i;
}

// scale/bias/residual/activation + store of the TC accumulator tiles one lane holds for output pixel m;
// cbase = first cout of the wave.
template <typename TOut, int TC, bool FIN = false>
__device__ __forceinline__ void epilogue_tiles(const ConvArgs& a, int m, int cbase, int q, const f32x4 (&acc)[TC]) {
  if constexpr (TC % 2 != 0) {
#pragma unroll
    for (int c = 0; c < TC; ++c) epilogue_store4<TOut, FIN>(a, m, cbase + cout_of<TC>(c, q, 0), acc[c]);
  } else {
    constexpr int VEC = 16 / sizeof(TOut);  // elements per 16-byte store
    const bool wide = (a.out_stride % VEC) == 0 && (((size_t)a.y) & 15) == 0 &&
                      (!a.res || ((a.res_stride % VEC) == 0 && (((size_t)a.res) & 15) == 0));
#pragma unroll
    for (int h = 0; h < TC / 2; ++h) {
      const int c0 = cbase + h * 32 + q * 8;
      if (!wide || c0 + 8 > a.Cout) {
        epilogue_store4<TOut, FIN>(a, m, c0, acc[2 * h]);
        epilogue_store4<TOut, FIN>(a, m, c0 + 4, acc[2 * h + 1]);
        continue;
      }
      f32x4 v0 = acc[2 * h], v1 = acc[2 * h + 1];
      if (a.scale) { v0 = v0 * *(const f32x4*)(a.scale + c0); v1 = v1 * *(const f32x4*)(a.scale + c0 + 4); }
      if (a.bias) { v0 = v0 + *(const f32x4*)(a.bias + c0); v1 = v1 + *(const f32x4*)(a.bias + c0 + 4); }
      if (a.res) {
        const TOut* rp = (const TOut*)a.res + (long)m * a.res_stride + c0;
        if constexpr (sizeof(TOut) == 2) {
          const f16x8 r = *(const f16x8*)rp;
#pragma unroll
          for (int j = 0; j < 4; ++j) { v0[j] += (float)r[j]; v1[j] += (float)r[4 + j]; }
        } else {
          v0 = v0 + *(const f32x4*)rp; v1 = v1 + *(const f32x4*)(rp + 4);
        }
      }
      if (a.act == CTDET_ACT_RELU) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { v0[j] = fmaxf(v0[j], 0.f); v1[j] = fmaxf(v1[j], 0.f); }
      } else if (a.act == CTDET_ACT_SIGMOID_CLAMP) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v0[j] = fminf(fmaxf(ctdet_sigmoid_exact(v0[j]), a.clamp_lo), a.clamp_hi);
          v1[j] = fminf(fmaxf(ctdet_sigmoid_exact(v1[j]), a.clamp_lo), a.clamp_hi);
        }
      }
      TOut* yp = (TOut*)a.y + (long)m * a.out_stride + c0;
      if constexpr (sizeof(TOut) == 2) {
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) { o[j] = (f16)v0[j]; o[4 + j] = (f16)v1[j]; }
        *(f16x8*)yp = o;
      } else {
        if constexpr (FIN) finite_note(a, v0, v1);
        *(f32x4*)yp = v0;
        *(f32x4*)(yp + 4) = v1;
      }
    }
  }
}

template <int... I, typename F>
__device__ __forceinline__ void static_for_seq(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }
// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): the index is a constant inside f
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) { static_for_seq(std::make_integer_sequence<int, N>{}, f); }

// Wave-level epilogue: scale / bias / residual / activation + store of ALL accumulator tiles a lane holds, acc[p][c] for the
// output pixels m[p] (GUARD: m[p] < 0 = no such pixel, nothing is stored) and the wave's first cout cbase.  Same arithmetic,
// element for element, as epilogue_tiles per pixel (acc * scale, + bias, + residual, activation, in this order, every step
// rounded on its own: contraction is off here, as the compiler could never contract across epilogue_tiles' null tests), but
// the memory operations are batched.  epilogue_tiles issues, per (pixel tile, cout-tile pair) group, scale loads - wait -
// bias loads - wait - residual loads - wait - stores, each wait also waiting for the previous group's stores (vmcnt counts
// them): 2-3 exposed round trips per group, 8-16 groups per lane.  Here the groups go in batches of NB (epilogue_batch below):
//   (a) every load of the batch is issued (scale, bias and the residual pieces of its NB groups),
//   (b) the waits count down in issue order: nothing but the batch's own loads is waited for more than once,
//   (c) the arithmetic of the batch, then all its stores back to back.
// The null tests of scale / bias / residual, the activation switch and the layout test are made once per batch for all its
// groups, not per group.  NB < all: kernels whose registers leave no room for a whole tile of residual (8 VGPRs per group
// in flight: 128 accumulators per lane, or an occupancy of 3-4 waves to keep).
// Groups are numbered g = h * TP + p (h = cout-tile pair, p = pixel tile); NB divides TP or is a multiple of it.
// Aliasing: res may be y itself (same address, same stride: the input gradient of the DCNv2 offset conv accumulates into
// dx that way, ops_train.py).  A lane reads exactly the residual elements of the positions it stores, and reads those of a batch before it
// stores any position of that batch or a later one, so in-place use stays correct; any other overlap of res and y was never
// supported and no caller has one (the residual of a block or Root is its input or projection, a tensor of its own).
// Ragged cases (unaligned / odd strides, a cout-tile pair beyond Cout, odd TC) take epilogue_tiles for the whole wave.
// Groups per batch.  8 VGPRs per group in flight (the residual) on top of the accumulators and 16 of scale / bias: a lane
// with 128 accumulators takes 2 groups at a time, everything else the whole tile.  0 = the per-pixel epilogue_tiles.
template <int TP, int TC>
constexpr int epilogue_batch() { return TP * TC >= 32 ? 2 : TP * (TC / 2); }
// the tiled kernels (BP pixels per workgroup): their 128-pixel forms run at 3-4 waves per SIMD on 128 VGPRs or fewer and keep
// that with 2 groups; ACC_AGPR (the generic kernels: accumulators in AGPRs, copied out batch by batch, which costs a batch
// twice): 2 groups, and the 128-pixel forms stay per pixel -- nothing batched fits under their 4 waves
template <int BP, int TP, int TC, bool ACC_AGPR = false>
constexpr int epilogue_batch_tiled() {
  constexpr int whole = TP * (TC / 2);
  if (ACC_AGPR) return BP == 128 ? 0 : (whole < 2 ? whole : 2);
  if (TP * TC >= 32 || (BP == 128 && TP * TC >= 16)) return 2;
  return whole < 8 ? whole : 8;
}

// FIN: finite_note on every value stored (the DCNv2 layer that writes the heads' input, dcn_split_window_kernel<.., FIN>)
template <typename TOut, int TP, int TC, bool GUARD = false, int NB = epilogue_batch<TP, TC>(), bool FIN = false>
__device__ __forceinline__ void epilogue_wave(const ConvArgs& a, const int (&m)[TP], int cbase, int q,
                                              const f32x4 (&acc)[TP][TC]) {
  constexpr int VEC = 16 / sizeof(TOut);  // elements per 16-byte store
  bool batched = false;
  if constexpr (TC % 2 == 0 && NB > 0)
    batched = (a.out_stride % VEC) == 0 && (((size_t)a.y) & 15) == 0 &&
              (!a.res || ((a.res_stride % VEC) == 0 && (((size_t)a.res) & 15) == 0)) && cbase + 16 * TC <= a.Cout;
  if (NB == 0 || !batched) {
#pragma unroll
    for (int p = 0; p < TP; ++p)
      if (!GUARD || m[p] >= 0) epilogue_tiles<TOut, TC, FIN>(a, m[p], cbase, q, acc[p]);
    return;
  }
  if constexpr (TC % 2 == 0 && NB > 0) {
#pragma clang fp contract(off)
    constexpr int NG = TP * (TC / 2), NBATCH = NG / NB;
    constexpr int HB = NB > TP ? NB / TP : 1;          // cout-tile pairs a batch spans
    constexpr int RV = sizeof(TOut) == 2 ? 1 : 2;      // 16-byte pieces of a group's 8 residual elements
    static_assert(NG % NB == 0 && (NB % TP == 0 || TP % NB == 0), "batch size");
    const bool has_s = a.scale != nullptr, has_b = a.bias != nullptr, has_r = a.res != nullptr;
    const int cw0 = cbase + q * 8;                     // the lane's 8 couts of pair h start at cw0 + 32 h
    f32x4 sc[HB][2], bi[HB][2], rr[NB][RV];
    int cw = cw0, mb[TP];
    auto issue = [&](auto kc) {
      constexpr int k = decltype(kc)::value, h0 = k * NB / TP;
      // the batch's addresses are formed here, behind the stores of the batch before: hoisted to the top by the scheduler, the
      // pointers of 16 groups (and their pixels' row offsets) cost more registers than the residual in flight
      asm volatile("" : "+v"(cw) :: "memory");
#pragma unroll
      for (int j = 0; j < (NB < TP ? NB : TP); ++j) {
        const int p = (k * NB + j) % TP;
        mb[p] = m[p];
        asm volatile("" : "+v"(mb[p]));
      }
      if (has_s) {
#pragma unroll
        for (int hl = 0; hl < HB; ++hl) {
          sc[hl][0] = *(const f32x4*)(a.scale + cw + (h0 + hl) * 32);
          sc[hl][1] = *(const f32x4*)(a.scale + cw + (h0 + hl) * 32 + 4);
        }
      }
      if (has_b) {
#pragma unroll
        for (int hl = 0; hl < HB; ++hl) {
          bi[hl][0] = *(const f32x4*)(a.bias + cw + (h0 + hl) * 32);
          bi[hl][1] = *(const f32x4*)(a.bias + cw + (h0 + hl) * 32 + 4);
        }
      }
      if (has_r) {
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          constexpr int g0 = k * NB;
          const int p = (g0 + j) % TP, h = (g0 + j) / TP;
          const int mm = (GUARD && mb[p] < 0) ? 0 : mb[p];      // a lane without a pixel reads pixel 0's and drops it
          const TOut* rp = (const TOut*)a.res + (long)mm * a.res_stride + cw + h * 32;
          rr[j][0] = *(const f32x4*)rp;
          if constexpr (RV == 2) rr[j][1] = *(const f32x4*)(rp + 4);
        }
      }
    };
    auto finish = [&](auto kc) {
      constexpr int k = decltype(kc)::value, g0 = k * NB, h0 = g0 / TP;
      f32x4 v[NB][2];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int p = (g0 + j) % TP, h = (g0 + j) / TP;
        v[j][0] = acc[p][2 * h];
        v[j][1] = acc[p][2 * h + 1];
      }
      if (has_s) {
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const int hl = (g0 + j) / TP - h0;
          v[j][0] = v[j][0] * sc[hl][0];
          v[j][1] = v[j][1] * sc[hl][1];
        }
      }
      if (has_b) {
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const int hl = (g0 + j) / TP - h0;
          v[j][0] = v[j][0] + bi[hl][0];
          v[j][1] = v[j][1] + bi[hl][1];
        }
      }
      if (has_r) {
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          if constexpr (sizeof(TOut) == 2) {
            const f16x8 r = __builtin_bit_cast(f16x8, rr[j][0]);
#pragma unroll
            for (int i = 0; i < 4; ++i) { v[j][0][i] += (float)r[i]; v[j][1][i] += (float)r[4 + i]; }
          } else {
            v[j][0] = v[j][0] + rr[j][0];
            v[j][1] = v[j][1] + rr[j][RV - 1];
          }
        }
      }
      if (a.act == CTDET_ACT_RELU) {
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) { v[j][0][i] = fmaxf(v[j][0][i], 0.f); v[j][1][i] = fmaxf(v[j][1][i], 0.f); }
      } else if (a.act == CTDET_ACT_SIGMOID_CLAMP) {
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            v[j][0][i] = fminf(fmaxf(ctdet_sigmoid_exact(v[j][0][i]), a.clamp_lo), a.clamp_hi);
            v[j][1][i] = fminf(fmaxf(ctdet_sigmoid_exact(v[j][1][i]), a.clamp_lo), a.clamp_hi);
          }
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int p = (g0 + j) % TP, h = (g0 + j) / TP;
        if (GUARD && mb[p] < 0) continue;
        TOut* yp = (TOut*)a.y + (long)mb[p] * a.out_stride + cw + h * 32;
        if constexpr (sizeof(TOut) == 2) {
          f16x8 o;
#pragma unroll
          for (int i = 0; i < 4; ++i) { o[i] = (f16)v[j][0][i]; o[4 + i] = (f16)v[j][1][i]; }
          *(f16x8*)yp = o;
        } else {
          *(f32x4*)yp = v[j][0];
          *(f32x4*)(yp + 4) = v[j][1];
        }
      }
      if constexpr (FIN) {                                // behind the stores: one test and at most one flag store per batch
        static_assert(!GUARD && sizeof(TOut) == 4, "the finite test is made on f32 outputs of unguarded tiles");
        bool bad = false;
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) bad |= !(fabsf(v[j][0][i]) <= 3.402823466e38f) || !(fabsf(v[j][1][i]) <= 3.402823466e38f);
        if (bad) *a.finite = 0;
      }
    };
    static_for<NBATCH>([&](auto kc) {
      issue(kc);
      finish(kc);
    });
  }
}

// ------------------------------------------------------------------------------------------
// LDS-DMA variant for plain convolutions (everything except the DCNv2 sampler): tiles go HBM/L2 -> LDS
// with global_load_lds_dwordx4 (no staging registers, no ds_write), 3-stage LDS ring, loads two K steps
// ahead kept in flight across the barrier with a counted s_waitcnt vmcnt (never 0 in the main loop),
// one raw s_barrier per K step.  Padding / K-tail / rows beyond M read a 16-byte zero page instead of
// being zero-filled in registers.  The LDS image is the same swizzled [row][32 k] layout as above: the
// DMA writes lane-linear (wave base + lane*16), so the swizzle lives in which k-group a lane *fetches*.
// ------------------------------------------------------------------------------------------
static __device__ __attribute__((aligned(16))) unsigned int g_zero_page[64];

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// All of this wave's LDS operations have completed.  Through the builtin, not inline asm: the compiler's own waitcnt
// bookkeeping then KNOWS the counter is zero.  With an asm wait it still counts fragments that were read before a barrier
// for use behind it as in flight, and puts s_waitcnt lgkmcnt(n) in front of the MFMAs that consume them -- n chosen so
// that they wait for the reads issued AFTER the barrier (the next step's operands): the register double buffer is undone.
// Encoding (gfx9): vmcnt 63 and expcnt 7 = "don't wait", lgkmcnt 0.
__device__ __forceinline__ void wait_lgkm0() { __builtin_amdgcn_s_waitcnt(0xC07F); }

// Global loads of the rare slow paths (a DCNv2 sample outside the LDS window), issued AND awaited inside one asm block.  A
// plain C++ load there leaves "a VMEM load may be pending" in the compiler's waitcnt bookkeeping at the join with the fast
// path, and the pass then puts s_waitcnt vmcnt(0) into the fast path's MFMA stream -- every tap -- which also waits for the
// LDS-DMAs this file issues through asm (weights of the next kernel row, the next window): their latency, meant to be
// hidden until the next barrier, is exposed right behind the issue.
__device__ __forceinline__ void gload2_sync(const float* p, float& v0, float& v1) {
  typedef float f32x2_ __attribute__((ext_vector_type(2)));
  f32x2_ v;
  asm volatile("global_load_dwordx2 %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(p) : "memory");
  v0 = v[0]; v1 = v[1];
}
// the active lanes replace v by the 16 bytes at p (the others keep theirs: call it inside the divergent branch)
__device__ __forceinline__ void gload4_sync_into(const float* p, f32x4& v) {
  asm volatile("global_load_dwordx4 %0, %1, off\n\ts_waitcnt vmcnt(0)" : "+v"(v) : "v"(p) : "memory");
}

// One 16-byte-per-lane global->LDS DMA (global_load_lds_dwordx4: LDS address = M0 + lane*16).  Issued through inline
// asm on purpose: the compiler's waitcnt pass treats every LDS read as possibly aliasing every outstanding
// __builtin_amdgcn_global_load_lds and puts s_waitcnt vmcnt(0) in front of it, which serialises the multi-stage
// rings below.  All consumers here order DMA -> LDS read themselves (wait_vmcnt<N>() + s_barrier before the first
// read of a stage, lgkmcnt(0) + s_barrier before a stage is overwritten).
__device__ __forceinline__ void dma16(const void* g, char* lds_wave_base) {
  const unsigned l = __builtin_amdgcn_readfirstlane((unsigned)(size_t)lds_wave_base);
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(l), "v"(g) : "memory", "m0");
}

// ------------------------------------------------------------------------------------------
// f16x3 ("split") arithmetic of the f32-activation kernels (conv_f32.hip, SP = true): an f32 operand x is carried as
// hi + lo, hi = f16(x), lo = f16(x - hi) (x - hi is exact in f32, so hi + lo reproduces x to ~2^-22 relative, 3e-8
// absolute once lo reaches the f16 subnormals) and a product a*w runs on the f16 matrix pipe as
// a_hi*w_hi + a_lo*w_hi + a_hi*w_lo with f32 accumulation; the dropped a_lo*w_lo is ~2^-22 of the product.  Exact f16
// products, f32 sums: the error of a K-long dot product measures 6e-8 * sum|a w| (tools/split_probe.hip), the f32 MFMA
// chain 1e-7.  Activations stay f32 in HBM and LDS (the f32 kernels' images unchanged); weights are split once at pack
// time (ctdet_split_weights): each group of 4 consecutive k of a packed [Cout_pad][Kpad] f32 row becomes 16 bytes
// {w_hi[4], w_lo[4]}, which IS the A fragment a lane reads with ds_read_b128.  Per 16-k step and (cout tile, pixel tile):
//   acc += A . {a_hi[4], 0}         -> w_hi a_hi
//   acc += A . {a_lo[4], a_hi[4]}   -> w_hi a_lo + w_lo a_hi
// two v_mfma_f32_16x16x32_f16 of the same opcode on one accumulator (dependent issue needs no wait states; a 16x16x16
// second product would cost 87 % of a 16x16x32 and mixes opcodes on one accumulator).
// ------------------------------------------------------------------------------------------
// 4 f32 -> the two B operands of mma_px
__device__ __forceinline__ void split_b(const f32x4 x, f16x8& b1, f16x8& b2) {
  f16x4 hi, lo;
  split_parts(x, hi, lo);
  const f16x4 z = {(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
  b1 = __builtin_shufflevector(hi, z, 0, 1, 2, 3, 4, 5, 6, 7);
  b2 = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// one 16-k step of one pixel tile against TC cout tiles: wf = the lanes' 16-byte weight fragments (4 f32 k, or the split
// group), pf = 4 f32 k of the lane's pixel
template <bool SP, int TC>
__device__ __forceinline__ void mma_px(const f32x4 (&wf)[TC], const f32x4 pf, f32x4 (&acc)[TC]) {
  if constexpr (SP) {
    f16x8 b1, b2;
    split_b(pf, b1, b2);
#pragma unroll
    for (int c = 0; c < TC; ++c)
      acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, wf[c]), b1, acc[c], 0, 0, 0);
#pragma unroll
    for (int c = 0; c < TC; ++c)
      acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, wf[c]), b2, acc[c], 0, 0, 0);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int c = 0; c < TC; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[c][e], pf[e], acc[c], 0, 0, 0);
  }
}

// k-th weight of a packed row as f32 (scalar fallback kernels)
template <bool SP>
__device__ __forceinline__ float packed_w(const float* row, int k) {
  if constexpr (SP) {
    const f16* g = (const f16*)(row + (k & ~3));
    return (float)g[k & 3] + (float)g[4 + (k & 3)];
  } else {
    return row[k];
  }
}

// ------------------------------------------------------------------------------------------
// The LDS input window of the 3x3 / stride 1 / pad 1 halo kernels of conv_igemm.hip (conv3x3_halo_kernel, _pair_, _pair2_,
// _tap2_ and head_fused_x3_kernel): the (TH + 2) x (TW + 2) pixels around a TH x TW output tile of 256 pixels (8 x 32 or
// 16 x 16), one chunk of 64 bytes per pixel (32 f16 or 16 f32 channels).  This type is the only place that knows its image:
//   main [TH + 2 rows][TW px][64 B], the four 16-byte slots of a pixel permuted by swz(px) like the weight tiles, padded to
//        HMAIN = 5 DMA rounds of the workgroup;
//   side [TH + 2 rows][left, right][64 B] behind it: the halo columns tx0 - 1 and tx0 + TW, row stride 128, slots in order.
// A kernel keeps two such buffers (HBUF bytes each) at the start of its LDS and decides itself when to issue and wait.
// ------------------------------------------------------------------------------------------
template <typename TIn, int TW>
struct HaloWindow {
  static constexpr int TH = 256 / TW;
  static constexpr int EN = TW / 16;           // 16-pixel tiles per tile row
  static constexpr int RS = TW * 64;           // LDS bytes per window row
  static constexpr int RPR = 256 * 16 / RS;    // window rows a DMA round of the workgroup covers (2 / 4)
  static constexpr int EPV = 16 / sizeof(TIn), CH = 4 * EPV;   // elements per 16-byte piece, channels per chunk
  static constexpr int HMAIN = 5 * 4096, HSIDE = 4096, HBUF = HMAIN + HSIDE;
  static_assert((TH + 2 + RPR - 1) / RPR == 5 && 8 * (TH + 2) <= 256, "five main rounds and one side round cover the window");

  const TIn *hp0, *hps, *zero;
  long row2;
  unsigned hmask;
  int abase[EN][3], estride0, estride1;

  // window of the tile at (ty0, tx0) of image b; row0 = first tile row of this wave (folded into the fragment bases)
  __device__ __forceinline__ HaloWindow(const ConvArgs& a, int b, int ty0, int tx0, int row0) {
    const int tid = threadIdx.x, lane = tid & 63;
    // the zero page pointer is opaque (conv_igemm_dma_kernel): one DMA per piece, real address or zero page by v_cndmask
    zero = (const TIn*)g_zero_page;
    asm volatile("" : "+v"(zero));
    const TIn* ximg = (const TIn*)a.x + (long)b * a.H * a.W * a.in_stride;
    // ---- loader: 5 main pieces + 1 side piece per thread and chunk ----
    // main piece i of thread t: pid = t + 256 i -> halo row t / (4 TW) + RPR i, pixel (t >> 2) % TW, slot t & 3: rows RPR
    // apart, so one base pointer + a uniform row stride suffice; bit i of hmask = the piece is inside the image (and the
    // window: the 16 x 16 tile's fifth round has two rows), everything else reads the zero page
    const int hslot = tid & 3, hpx = (tid >> 2) & (TW - 1), hr0 = tid / (4 * TW);
    const int y0 = ty0 - 1 + hr0;
    hp0 = ximg + ((long)y0 * a.W + tx0 + hpx) * a.in_stride + (hslot ^ swz(hpx)) * EPV;
    row2 = (long)RPR * a.W * a.in_stride;
    hmask = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) hmask |= (hr0 + RPR * i < TH + 2 && y0 + RPR * i >= 0 && y0 + RPR * i < a.H) ? (1u << i) : 0u;
    {
      const int side = (tid >> 2) & 1, hr = tid >> 3;   // [hr 0..TH+1][side][slot], tid < 8 * (TH + 2)
      const int y = ty0 - 1 + hr, x = side ? tx0 + TW : tx0 - 1;
      const bool ok = tid < 8 * (TH + 2) && y >= 0 && y < a.H && x >= 0 && x < a.W;
      hps = ximg + ((long)(ok ? y : 0) * a.W + (ok ? x : 0)) * a.in_stride + hslot * EPV;
      hmask |= ok ? 32u : 0u;
    }
    // ---- fragment addressing: per lane one LDS base per (px-tile e of the tile row, tap column s) with the wave's first
    // tile row folded in; interior lanes then use immediates for (tile row + tap row) * RS.  The single edge lane of
    // (e = 0, s = 0) [left halo column] and (e = EN - 1, s = 2) [right halo column] reads the side region. ----
    const int l15 = lane & 15, kg = lane >> 4;
#pragma unroll
    for (int e = 0; e < EN; ++e)
#pragma unroll
      for (int s2 = 0; s2 < 3; ++s2) {
        const int X = 16 * e + l15 + s2 - 1;
        if (X < 0) abase[e][s2] = HMAIN + kg * 16 + row0 * 128;
        else if (X > TW - 1) abase[e][s2] = HMAIN + 64 + kg * 16 + row0 * 128;
        else abase[e][s2] = X * 64 + ((kg ^ swz(X)) << 4) + row0 * RS;
      }
    estride0 = (l15 == 0) ? 128 : RS;      // row stride of this lane for (e = 0, s = 0)
    estride1 = (l15 == 15) ? 128 : RS;     // ... for (e = EN - 1, s = 2)
  }

  // this thread's six DMAs of `chunk` into halo buffer hb
  __device__ __forceinline__ void issue(char* smem, int wave, int chunk, int hb) const {
    char* dst = smem + hb * HBUF + wave * 1024;
    const long coff = (long)chunk * CH;
#pragma unroll
    for (int i = 0; i < 5; ++i) dma16((hmask & (1u << i)) ? hp0 + i * row2 + coff : zero, dst + i * 4096);
    dma16((hmask & 32u) ? hps + coff : zero, dst + HMAIN);
  }

  // f32 windows: the thread's own six pieces of halo buffer hb, 4 f32 -> {hi[4], lo[4]} f16, in place.  A thread converts
  // exactly what its own DMAs fetched, so the pass needs no barrier of its own
  __device__ __forceinline__ void split_in_place(char* smem, int wave, int lane, int hb) const {
    static_assert(std::is_same<TIn, float>::value, "only f32 windows are split");
    char* base = smem + hb * HBUF + wave * 1024 + lane * 16;
    f32x4 v[6];
#pragma unroll
    for (int i = 0; i < 5; ++i) v[i] = *(const f32x4*)(base + i * 4096);
    v[5] = *(const f32x4*)(base + HMAIN);
#pragma unroll
    for (int i = 0; i < 6; ++i) *(f16x8*)(base + (i < 5 ? i * 4096 : HMAIN)) = split_hi_lo(v[i]);
  }

  // offset in a halo buffer of this lane's 16-byte fragment of the wave's pixel tile p for tap T
  __device__ __forceinline__ int tap_off(int p, int T) const {
    const int R_ = T / 3, S_ = T % 3;
    const int e = p % EN, lr = p / EN;
    if (e == 0 && S_ == 0) return abase[0][0] + (lr + R_) * estride0;
    if (e == EN - 1 && S_ == 2) return abase[EN - 1][2] + (lr + R_) * estride1;
    return abase[e][S_] + (lr + R_) * RS;
  }
};

// workgroup -> (image b, tile origin, cout tile) of the halo kernels' 1-D grid (halo_grid); false: no tile for this workgroup
template <int TW>
__device__ __forceinline__ bool halo_tile_of_block(int B, int H, int W, int nby, int& b, int& ty0, int& tx0, int& n_tile) {
  constexpr int TH = 256 / TW;
  const int tiles_x = W / TW, tiles_y = H / TH;
  int m_tile;
  if (!tile_of_block(B * tiles_y * tiles_x, nby, m_tile, n_tile)) return false;
  tx0 = (m_tile % tiles_x) * TW;
  ty0 = ((m_tile / tiles_x) % tiles_y) * TH;
  b = m_tile / (tiles_x * tiles_y);
  return true;
}

// output rows of the pixels a lane holds: pixel tile p of the wave = tile row row0 + p / EN, columns 16 (p % EN) + l15
template <int TW, int TP>
__device__ __forceinline__ void halo_out_rows(const ConvArgs& a, int b, int ty0, int tx0, int row0, int l15, int (&mo)[TP]) {
  constexpr int EN = TW / 16;
#pragma unroll
  for (int p = 0; p < TP; ++p) {
    const int y = ty0 + row0 + p / EN, x = tx0 + 16 * (p % EN) + l15;
    mo[p] = (b * a.H + y) * a.W + x;
  }
}

// packed weight rows this thread stages, NLD rounds of 64 LDS rows: LDS row (tile tt, row r) of a wave's TC cout tiles holds
// cout_of<TC>(tt, r / 4, r % 4), slot = k group ^ swz(row); wptr[j] = that row of w (rows n0 on) + the thread's k group.
// Rows beyond BC (only when BC < 64) re-read packed row 0: harmless, their LDS rows are never consumed
template <int BC, int TC, typename T, int NLD>
__device__ __forceinline__ void weight_row_ptrs(const void* w, int n0, int kpad, const T* (&wptr)[NLD]) {
  const int tid = threadIdx.x, lrow = tid >> 2;
  const int gw = (tid & 3) ^ swz(lrow);
#pragma unroll
  for (int j = 0; j < NLD; ++j) {
    const int L = lrow + 64 * j;
    const int Lw = L % (16 * TC), wv = L / (16 * TC);
    const int tt = Lw >> 4, r = Lw & 15;
    const int cl = wv * 16 * TC + cout_of<TC>(tt, r >> 2, r & 3);
    wptr[j] = (const T*)w + (long)(n0 + (L < BC ? cl : 0)) * kpad + gw * (int)(16 / sizeof(T));
  }
}

// cout tile of a conv (= ctdet_conv_cout_tile): packed weight rows are padded to a multiple of it
static inline int pick_bc(int cout) {
  if (cout <= 16) return 16;
  if (cout <= 32) return 32;
  if (cout <= 64) return 64;
  if (cout <= 128) return 128;          // 80 classes: one padded 128-cout tile reads the input once, three 32-cout tiles three times
  if (cout % 128 == 0) return 128;
  if (cout % 64 == 0) return 64;
  return 32;
}
