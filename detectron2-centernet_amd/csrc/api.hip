// C-ABI entry points of libctdet_hip.so (see include/ctdet_hip.h for the contract and the reference
// interfaces each function replaces).  No torch types, no allocation, no synchronisation (except the
// explicit diagnostic helper ctdet_decode_status).
#include "conv_common.h"
#include "../../include/ctdet_hip.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <atomic>

static thread_local char g_err[512] = "";
void ctdet_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

thread_local int g_label_mode = 0;
static thread_local char g_label[128] = "";
bool ctdet_set_label(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_label, sizeof(g_label), fmt, ap);
  va_end(ap);
  return g_label_mode == 2;
}

static_assert(CTDET_DT_F16 == CTDET_F16 && CTDET_DT_F32 == CTDET_F32 && CTDET_DT_U8 == CTDET_U8 && CTDET_DT_F16X3 == CTDET_F16X3,
              "dtypes: header and kernels disagree");
static_assert(CTDET_CLIP_NONE == SGD_CLIP_NONE && CTDET_CLIP_VALUE == SGD_CLIP_VALUE && CTDET_CLIP_NORM == SGD_CLIP_NORM &&
              CTDET_NORM_L1 == GRAD_NORM_L1 && CTDET_NORM_L2 == GRAD_NORM_L2 && CTDET_NORM_INF == GRAD_NORM_INF,
              "clip / norm modes: header and kernels disagree");
static_assert(CTDET_DCN_MASK_LOGIT == DCN_MASK_LOGIT && CTDET_DCN_MASK_PROB == DCN_MASK_PROB && CTDET_DCN_MASK_NONE == DCN_MASK_NONE,
              "mask modes of the ABI and of the kernels");
#define CTDET_DCN_MASK_MODE(what, mode) \
  CTDET_CHECK((mode) >= CTDET_DCN_MASK_LOGIT && (mode) <= CTDET_DCN_MASK_NONE, what ": mask mode %d", mode)

static int fill_args(const ctdet_conv_desc* d, ConvArgs& a) {
  CTDET_CHECK(d != nullptr, "conv: null descriptor");
  CTDET_CHECK(d->B >= 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0, "conv: bad shape B=%d H=%d W=%d Cin=%d Cout=%d",
              d->B, d->H, d->W, d->Cin, d->Cout);
  CTDET_CHECK(d->R > 0 && d->S > 0 && d->stride > 0 && d->dil > 0 && d->pad >= 0, "conv: bad kernel geometry");
  const int idl = d->in_dil > 1 ? d->in_dil : 1;
  const int ho = ((d->H - 1) * idl + 1 + 2 * d->pad - (d->dil * (d->R - 1) + 1)) / d->stride + 1;
  const int wo = ((d->W - 1) * idl + 1 + 2 * d->pad - (d->dil * (d->S - 1) + 1)) / d->stride + 1;
  CTDET_CHECK(d->Ho >= ho && d->Ho < ho + idl && d->Wo >= wo && d->Wo < wo + idl,
              "conv: output size %dx%d does not match geometry (expected %dx%d)", d->Ho, d->Wo, ho, wo);
  CTDET_CHECK(d->in_stride >= d->Cin && d->out_stride >= d->Cout, "conv: pixel strides smaller than channel counts");
  memset(&a, 0, sizeof(a));
  a.B = d->B; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.in_stride = d->in_stride;
  a.Cout = d->Cout; a.Ho = d->Ho; a.Wo = d->Wo; a.out_stride = d->out_stride; a.res_stride = d->res_stride;
  a.R = d->R; a.S = d->S; a.stride = d->stride; a.pad = d->pad; a.dil = d->dil;
  a.K = d->R * d->S * d->Cin; a.Kpad = d->Kpad; a.Cout_pad = d->Cout_pad;
  a.M = d->B * d->Ho * d->Wo;
  a.act = d->act; a.clamp_lo = d->clamp_lo; a.clamp_hi = d->clamp_hi; a.korder = d->korder; a.in_dil = idl;
  CTDET_CHECK(d->korder == 0 || (d->korder == 1 && d->Cin % 32 == 0 && d->compute_dtype == CTDET_DT_F16) ||
                  (d->korder == 2 && d->Cin % 16 == 0 && d->compute_dtype == CTDET_DT_F16X3 && d->R == 3 && d->S == 3) ||
                  (d->korder == 3 && d->Cin % 32 == 0 && d->compute_dtype == CTDET_DT_F16X3 && d->R == 3 && d->S == 3),
              "conv: korder=%d invalid for Cin=%d", d->korder, d->Cin);
  CTDET_CHECK((long)d->B * d->Ho * d->Wo < (1L << 31), "conv: too many output pixels");
  return 0;
}

// the tail of the conv-shaped forward entry points: f16 tensors go to conv_igemm.hip, f32 tensors (f32 or f16x3 arithmetic)
// to conv_f32.hip, which writes f32 only
static int conv_dispatch(const char* op, const ctdet_conv_desc* d, const ConvArgs& a, bool deform, void* stream) {
  if (d->compute_dtype == CTDET_DT_F16) return launch_conv_f16(a, d->out_dtype, deform, (hipStream_t)stream);
  if (d->compute_dtype == CTDET_DT_F32 || d->compute_dtype == CTDET_DT_F16X3) {
    CTDET_CHECK(d->out_dtype == CTDET_DT_F32, "%s(f32 / f16x3): output must be f32", op);
    return launch_conv_f32(a, deform, d->compute_dtype == CTDET_DT_F16X3, (hipStream_t)stream);
  }
  CTDET_CHECK(false, "%s: bad compute dtype %d", op, d->compute_dtype);
}

static std::atomic<unsigned> g_tuning{0};
unsigned ctdet_tuning_flags() { return g_tuning.load(std::memory_order_relaxed); }

int ctdet_device_cu_count() {
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int n = cache[dev].load(std::memory_order_relaxed);
  if (n == 0) {
    hipDeviceProp_t prop;
    n = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    cache[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

extern "C" {

const char* ctdet_last_error(void) { return g_err; }
int32_t ctdet_set_tuning_flags(uint32_t flags) { g_tuning.store(flags, std::memory_order_relaxed); return 0; }
uint32_t ctdet_get_tuning_flags(void) { return g_tuning.load(std::memory_order_relaxed); }
int32_t ctdet_abi_version(void) { return 8; }
int32_t ctdet_set_label_mode(int32_t mode) {
  CTDET_CHECK(mode >= 0 && mode <= 2, "set_label_mode: mode %d (0 off, 1 record, 2 dry run)", mode);
  g_label_mode = mode;
  return 0;
}
const char* ctdet_last_kernel_label(void) { return g_label; }
int32_t ctdet_conv_cout_tile(int32_t cout) { return pick_bc(cout); }

int32_t ctdet_conv2d_fwd(const ctdet_conv_desc* d, const void* x, const void* w_packed, const float* scale,
                         const float* bias, const void* residual, void* y, void* stream) {
  ConvArgs a;
  int rc = fill_args(d, a);
  if (rc) return rc;
  if (a.M == 0) return 0;
  CTDET_CHECK(x && w_packed && y, "conv: null pointer");
  a.x = x; a.w = w_packed; a.scale = scale; a.bias = bias; a.res = residual; a.y = y;
  return conv_dispatch("conv", d, a, false, stream);
}

int32_t ctdet_conv_pair_supported(const ctdet_conv_desc* d, const void* x) {
  ConvArgs a;
  if (fill_args(d, a) || d->compute_dtype != CTDET_DT_F16X3) return 0;
  a.x = x;
  return conv_pair_korder(a);
}

int32_t ctdet_conv1x1_cat_fwd(const ctdet_conv_desc* d, const void* const* xs, const int32_t* cins,
                              const int32_t* strides, int32_t nsrc, const void* w_packed, const float* scale,
                              const float* bias, const void* residual, void* y, void* stream) {
  ConvArgs a;
  int rc = fill_args(d, a);
  if (rc) return rc;
  if (a.M == 0) return 0;
  CTDET_CHECK(xs && cins && strides && w_packed && y, "conv1x1_cat: null pointer");
  CTDET_CHECK(nsrc >= 1 && nsrc <= 4, "conv1x1_cat: nsrc=%d must be 1..4", nsrc);
  CTDET_CHECK(d->R == 1 && d->S == 1 && d->stride == 1 && d->pad == 0, "conv1x1_cat: only 1x1 stride-1 convs");
  a.korder = 0;
  const int align = d->compute_dtype == CTDET_DT_F16 ? 8 : (d->compute_dtype == CTDET_DT_F16X3 ? 4 : 1);
  int cum = 0;
  for (int j = 0; j < 4; ++j) {
    if (j < nsrc) {
      CTDET_CHECK(xs[j] && cins[j] > 0 && cins[j] % align == 0 && strides[j] >= cins[j] && strides[j] % align == 0,
                  "conv1x1_cat: bad source %d (cin=%d stride=%d)", j, cins[j], strides[j]);
      cum += cins[j];
      a.xs[j] = xs[j]; a.xs_stride[j] = strides[j];
    } else {
      a.xs[j] = xs[nsrc - 1]; a.xs_stride[j] = strides[nsrc - 1];
    }
    a.xs_cend[j] = cum;
  }
  CTDET_CHECK(cum == d->Cin, "conv1x1_cat: sources sum to %d channels, descriptor says %d", cum, d->Cin);
  a.nsrc = nsrc < 2 ? 2 : nsrc;  // always take the multi-source path (a single source is sources {0, 0-length})
  if (nsrc == 1) { a.nsrc = 1; a.in_stride = strides[0]; }
  a.x = xs[0]; a.w = w_packed; a.scale = scale; a.bias = bias; a.res = residual; a.y = y;
  return conv_dispatch("conv1x1_cat", d, a, false, stream);
}

int32_t ctdet_dcnv2_fwd(const ctdet_conv_desc* d, const void* x, const float* offset_mask, int32_t om_stride,
                        int32_t mask_is_prob, const void* w_packed, const float* scale, const float* bias, void* y, void* stream) {
  ConvArgs a;
  int rc = fill_args(d, a);
  if (rc) return rc;
  if (a.M == 0) return 0;
  CTDET_CHECK(x && w_packed && y && offset_mask, "dcnv2: null pointer");
  CTDET_DCN_MASK_MODE("dcnv2", mask_is_prob);
  CTDET_CHECK(om_stride >= (mask_is_prob == CTDET_DCN_MASK_NONE ? 2 : 3) * d->R * d->S, "dcnv2: om_stride=%d < %d*R*S", om_stride,
              mask_is_prob == CTDET_DCN_MASK_NONE ? 2 : 3);
  // korder 0: tap-major weights -> gather-from-global kernel; korder 1: chunk-major -> LDS-window kernel
  a.x = x; a.w = w_packed; a.scale = scale; a.bias = bias; a.res = nullptr; a.y = y;
  a.om = offset_mask; a.om_stride = om_stride; a.mask_is_prob = mask_is_prob;
  return conv_dispatch("dcnv2", d, a, true, stream);
}

int32_t ctdet_dcnv2_cols_supported(const ctdet_conv_desc* d, const void* x, const void* y) {
  ConvArgs a;
  if (fill_args(d, a) || d->compute_dtype != CTDET_DT_F16X3 || d->out_dtype != CTDET_DT_F32) return 0;
  a.x = x; a.y = const_cast<void*>(y);
  return dcn_split_window_ok(a) ? 1 : 0;
}

int32_t ctdet_dcnv2_fwd_cols(const ctdet_conv_desc* d, const void* x, const float* offset_mask, int32_t om_stride,
                             int32_t mask_is_prob, const void* w_packed, const float* scale, const float* bias, void* y,
                             float* cols_out, void* stream) {
  ConvArgs a;
  int rc = fill_args(d, a);
  if (rc) return rc;
  if (a.M == 0) return 0;
  CTDET_CHECK(x && w_packed && y && offset_mask && cols_out, "dcnv2_fwd_cols: null pointer");
  CTDET_DCN_MASK_MODE("dcnv2", mask_is_prob);
  CTDET_CHECK(om_stride >= (mask_is_prob == CTDET_DCN_MASK_NONE ? 2 : 3) * d->R * d->S, "dcnv2: om_stride=%d < %d*R*S", om_stride,
              mask_is_prob == CTDET_DCN_MASK_NONE ? 2 : 3);
  CTDET_CHECK(d->compute_dtype == CTDET_DT_F16X3 && d->out_dtype == CTDET_DT_F32 && (((size_t)cols_out) & 15) == 0,
              "dcnv2_fwd_cols: the f16x3 mode's entry point (f32 tensors), 16-byte aligned columns");
  a.x = x; a.w = w_packed; a.scale = scale; a.bias = bias; a.res = nullptr; a.y = y;
  a.om = offset_mask; a.om_stride = om_stride; a.mask_is_prob = mask_is_prob;
  CTDET_CHECK(dcn_split_window_ok(a), "dcnv2_fwd_cols: shape not served by the LDS-window kernel (ask ctdet_dcnv2_cols_supported first)");
  a.cols_out = cols_out;
  return launch_conv_f32(a, true, true, (hipStream_t)stream);
}

int32_t ctdet_dcnv2_offset_supported(const ctdet_conv_desc* d) {
  ConvArgs a;
  if (fill_args(d, a)) return 0;
  a.y = nullptr;
  if (d->compute_dtype == CTDET_DT_F16X3) return (d->out_dtype == CTDET_DT_F32 && dcn_offset_fused_x3_ok(a)) ? 1 : 0;
  if (d->compute_dtype != CTDET_DT_F16) return 0;
  return dcn_offset_fused_ok(a) ? 1 : 0;
}

int32_t ctdet_dcnv2_offset_fwd(const ctdet_conv_desc* d, const void* x, const void* w_off_packed, const float* b_off,
                               float* om_out, int32_t om_out_stride, const void* w_packed, const float* scale,
                               const float* bias, void* y, void* stream) {
  return ctdet_dcnv2_offset_finite_fwd(d, x, w_off_packed, b_off, om_out, om_out_stride, w_packed, scale, bias, y, nullptr, stream);
}

int32_t ctdet_dcnv2_offset_finite_fwd(const ctdet_conv_desc* d, const void* x, const void* w_off_packed, const float* b_off,
                                      float* om_out, int32_t om_out_stride, const void* w_packed, const float* scale,
                                      const float* bias, void* y, int32_t* finite, void* stream) {
  ConvArgs a;
  int rc = fill_args(d, a);
  if (rc) return rc;
  if (a.M == 0) return 0;
  CTDET_CHECK(x && w_off_packed && b_off && w_packed && y, "dcnv2_offset: null pointer");
  a.x = x; a.w = w_packed; a.scale = scale; a.bias = bias; a.res = nullptr; a.y = y;
  a.w_off = w_off_packed; a.b_off = b_off;
  if (d->compute_dtype == CTDET_DT_F16X3) {
    CTDET_CHECK(d->out_dtype == CTDET_DT_F32 && !om_out, "dcnv2_offset(f16x3): f32 output, no om_out (inference form)");
    a.mask_is_prob = DCN_MASK_LOGIT;
    a.finite = (int*)finite;
    return launch_dcn_offset_x3(a, (hipStream_t)stream);
  }
  CTDET_CHECK(d->compute_dtype == CTDET_DT_F16, "dcnv2_offset: f16 or f16x3");
  CTDET_CHECK(!finite, "dcnv2_offset: the finite flag is the f16x3 form's");
  CTDET_CHECK(!om_out || (om_out_stride >= 28 && om_out_stride % 4 == 0 && ((size_t)om_out & 15) == 0),
              "dcnv2_offset: om_out needs a 16-byte aligned row of >= 28 floats (stride %d)", om_out_stride);
  a.om_out = om_out; a.om_out_stride = om_out_stride;
  return launch_conv_f16(a, d->out_dtype, true, (hipStream_t)stream);
}

int32_t ctdet_preprocess(const void* img, int32_t img_dtype, void* out, int32_t out_dtype, int32_t B, int32_t H,
                         int32_t W, int32_t Hp, int32_t Wp, int64_t img_batch_stride, const float* mean3,
                         const float* std3, int32_t out_stride, int32_t border, void* stream) {
  CTDET_CHECK(img && out && mean3 && std3, "preprocess: null pointer");
  return launch_preprocess(img, img_dtype, out, out_dtype, B, H, W, Hp, Wp, (long)img_batch_stride, mean3, std3,
                           out_stride, border, -1, (hipStream_t)stream);
}

int32_t ctdet_preprocess_mirror(const void* img, int32_t img_dtype, void* out, int32_t out_dtype, int32_t B, int32_t H,
                                int32_t W, int32_t Hp, int32_t Wp, int64_t img_batch_stride, const float* mean3,
                                const float* std3, int32_t out_stride, int32_t border, int32_t mirror_from, void* stream) {
  CTDET_CHECK(img && out && mean3 && std3, "preprocess: null pointer");
  CTDET_CHECK(mirror_from >= 0 && mirror_from <= B, "preprocess: mirror_from=%d outside [0, B=%d]", mirror_from, B);
  return launch_preprocess(img, img_dtype, out, out_dtype, B, H, W, Hp, Wp, (long)img_batch_stride, mean3, std3,
                           out_stride, border, mirror_from, (hipStream_t)stream);
}

// the head descriptor -> HeadArgs (everything but the first conv's operands)
static int head_args(const ctdet_head_desc* d, HeadArgs& a) {
  a.nheads = d->nheads; a.B = d->B; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.in_stride = d->in_stride;
  a.clamp_lo = d->clamp_lo; a.clamp_hi = d->clamp_hi;
  CTDET_CHECK(d->nheads >= 1 && d->nheads <= 4, "head_fused: nheads=%d out of range", d->nheads);
  for (int h = 0; h < d->nheads; ++h) {
    CTDET_CHECK(d->w2[h] && d->b2[h] && d->y[h], "head_fused: head %d: null pointer", h);
    a.w2[h] = d->w2[h]; a.b2[h] = (const float*)d->b2[h]; a.y[h] = (float*)d->y[h];
    a.y_stride[h] = d->y_stride[h]; a.cout[h] = d->cout[h]; a.act[h] = d->act[h];
  }
  return 0;
}

int32_t ctdet_head_fused_supported(int32_t compute_dtype, int32_t H, int32_t W, int32_t Cin, int32_t in_stride, const void* x) {
  HeadArgs a = {};
  a.x = x; a.H = H; a.W = W; a.Cin = Cin; a.in_stride = in_stride;
  if (compute_dtype != CTDET_DT_F16 && compute_dtype != CTDET_DT_F16X3) return 0;
  return head_fused_x_ok(a, compute_dtype == CTDET_DT_F16X3) ? 1 : 0;
}

int32_t ctdet_head_fused_fwd(const ctdet_head_desc* d, const void* x, const void* w1, const float* b1, void* stream) {
  CTDET_CHECK(d && x && w1 && b1, "head_fused: null pointer");
  HeadArgs a = {};
  a.x = x; a.w1 = w1; a.b1 = b1;
  if (int rc = head_args(d, a)) return rc;
  return launch_head_fused(a, (hipStream_t)stream);
}

int32_t ctdet_head_fused_x3_fwd(const ctdet_head_desc* d, const void* x, const void* w1, const float* s1, const float* b1,
                                void* stream) {
  CTDET_CHECK(d && x && w1 && s1 && b1, "head_fused_x3: null pointer");
  HeadArgs a = {};
  a.x = x; a.w1 = w1; a.s1 = s1; a.b1 = b1;
  if (int rc = head_args(d, a)) return rc;
  return launch_head_fused_x3(a, (hipStream_t)stream);
}

int32_t ctdet_head_sparse_x3_fwd(const ctdet_head_desc* d, const void* x, const void* w1, const float* s1, const float* b1,
                                 const int32_t* inds, int32_t K, float down_ratio, int32_t flip, float* whreg, float* boxes,
                                 void* stream) {
  CTDET_CHECK(d && x && w1 && s1 && b1 && inds && whreg && boxes, "head_sparse_x3: null pointer");
  CTDET_CHECK(d->nheads == 2 && d->w2[0] && d->w2[1] && d->b2[0] && d->b2[1], "head_sparse_x3: a two-head (wh, reg) pack");
  HeadArgs a = {};
  a.x = x; a.w1 = w1; a.s1 = s1; a.b1 = b1;
  a.nheads = 2; a.B = d->B; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.in_stride = d->in_stride;
  for (int h = 0; h < 2; ++h) { a.w2[h] = d->w2[h]; a.b2[h] = (const float*)d->b2[h]; a.cout[h] = d->cout[h]; }
  return launch_head_sparse_x3(a, inds, whreg, boxes, K, down_ratio, flip != 0, (hipStream_t)stream);
}

// launch: launch_dla_base (f16) or launch_dla_base_x3 (f16x3: out / pooled f32), `what` its name in messages.
// mirror_from < 0: the plain kernels; otherwise output images [mirror_from, B) are computed from the mirrored network input
// of source images [0, B - mirror_from)
static int32_t dla_base_entry(int (*launch)(const BaseArgs&, hipStream_t), const char* what, const ctdet_dla_base_desc* d,
                              int mirror_from, const void* images, const void* w_stem, const float* scale_stem,
                              const float* bias_stem, const void* w_l0, const float* scale_l0, const float* bias_l0,
                              const void* w_l1, const float* scale_l1, const float* bias_l1, void* out, void* pooled,
                              void* stream) {
  CTDET_CHECK(d && images && w_stem && scale_stem && bias_stem && w_l0 && scale_l0 && bias_l0 && w_l1 && scale_l1 && bias_l1 &&
              out, "%s: null pointer", what);
  BaseArgs a = {};
  a.img = images; a.img_dtype = d->img_dtype; a.img_batch_stride = (long)d->img_batch_stride;
  a.B = d->B; a.H = d->H; a.W = d->W; a.Hp = d->Hp; a.Wp = d->Wp;
  for (int i = 0; i < 3; ++i) { a.mean[i] = d->mean[i]; a.stdv[i] = d->std[i]; }
  a.w0 = w_stem; a.s0 = scale_stem; a.b0 = bias_stem;
  a.w1 = w_l0; a.s1 = scale_l0; a.b1 = bias_l0;
  a.w2 = w_l1; a.s2 = scale_l1; a.b2 = bias_l1;
  a.y = out; a.out_stride = d->out_stride;
  a.pool = pooled; a.pool_stride = d->pool_stride;
  a.mirror_from = mirror_from;
  return launch(a, (hipStream_t)stream);
}

int32_t ctdet_dla_base_fwd(const ctdet_dla_base_desc* d, const void* images, const void* w_stem, const float* scale_stem,
                           const float* bias_stem, const void* w_l0, const float* scale_l0, const float* bias_l0,
                           const void* w_l1, const float* scale_l1, const float* bias_l1, void* out, void* pooled,
                           void* stream) {
  return dla_base_entry(launch_dla_base, "dla_base", d, -1, images, w_stem, scale_stem, bias_stem, w_l0, scale_l0, bias_l0, w_l1,
                        scale_l1, bias_l1, out, pooled, stream);
}

int32_t ctdet_dla_base_mirror_fwd(const ctdet_dla_base_desc* d, int32_t mirror_from, const void* images, const void* w_stem,
                                  const float* scale_stem, const float* bias_stem, const void* w_l0, const float* scale_l0,
                                  const float* bias_l0, const void* w_l1, const float* scale_l1, const float* bias_l1,
                                  void* out, void* pooled, void* stream) {
  CTDET_CHECK(d && mirror_from >= 0 && mirror_from <= d->B, "dla_base: mirror_from=%d outside [0, B=%d]", mirror_from,
              d ? d->B : 0);
  return dla_base_entry(launch_dla_base, "dla_base", d, mirror_from, images, w_stem, scale_stem, bias_stem, w_l0, scale_l0,
                        bias_l0, w_l1, scale_l1, bias_l1, out, pooled, stream);
}

int32_t ctdet_dla_base_x3_fwd(const ctdet_dla_base_desc* d, const void* images, const void* w_stem, const float* scale_stem,
                              const float* bias_stem, const void* w_l0, const float* scale_l0, const float* bias_l0,
                              const void* w_l1, const float* scale_l1, const float* bias_l1, float* out, float* pooled,
                              void* stream) {
  return dla_base_entry(launch_dla_base_x3, "dla_base(f16x3)", d, -1, images, w_stem, scale_stem, bias_stem, w_l0, scale_l0,
                        bias_l0, w_l1, scale_l1, bias_l1, out, pooled, stream);
}

int32_t ctdet_dla_base_x3_mirror_fwd(const ctdet_dla_base_desc* d, int32_t mirror_from, const void* images,
                                     const void* w_stem, const float* scale_stem, const float* bias_stem, const void* w_l0,
                                     const float* scale_l0, const float* bias_l0, const void* w_l1, const float* scale_l1,
                                     const float* bias_l1, float* out, float* pooled, void* stream) {
  CTDET_CHECK(d && mirror_from >= 0 && mirror_from <= d->B, "dla_base(f16x3): mirror_from=%d outside [0, B=%d]", mirror_from,
              d ? d->B : 0);
  return dla_base_entry(launch_dla_base_x3, "dla_base(f16x3)", d, mirror_from, images, w_stem, scale_stem, bias_stem, w_l0,
                        scale_l0, bias_l0, w_l1, scale_l1, bias_l1, out, pooled, stream);
}

int32_t ctdet_maxpool2x2(const void* x, void* y, int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C,
                         int32_t in_stride, int32_t out_stride, void* stream) {
  CTDET_CHECK(x && y, "maxpool2x2: null pointer");
  return launch_maxpool2x2(x, y, dtype, B, H, W, C, in_stride, out_stride, (hipStream_t)stream);
}

int32_t ctdet_maxpool3x3s2(const void* x, void* y, int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C,
                           int32_t in_stride, int32_t out_stride, void* stream) {
  CTDET_CHECK(x && y, "maxpool3x3s2: null pointer");
  return launch_maxpool3x3s2(x, y, dtype, B, H, W, C, in_stride, out_stride, 0, (hipStream_t)stream);
}

int32_t ctdet_maxpool3x3s2_ceil(const void* x, void* y, int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C,
                                int32_t in_stride, int32_t out_stride, void* stream) {
  CTDET_CHECK(x && y, "maxpool3x3s2_ceil: null pointer");
  return launch_maxpool3x3s2(x, y, dtype, B, H, W, C, in_stride, out_stride, 1, (hipStream_t)stream);
}

int32_t ctdet_global_avgpool(const void* x, int32_t dtype, int32_t B, int32_t HW, int32_t C, int32_t stride, float* out,
                             void* stream) {
  CTDET_CHECK(x && out, "global_avgpool: null pointer");
  return launch_global_avgpool(x, dtype, B, HW, C, stride, out, (hipStream_t)stream);
}

int32_t ctdet_finite_flag(const float* x, int64_t M, int32_t C, int32_t stride, int32_t* flag, void* stream) {
  CTDET_CHECK(x && flag, "finite_flag: null pointer");
  return launch_finite_flag(x, (long)M, C, stride, (int*)flag, (hipStream_t)stream);
}

int32_t ctdet_ese_scale(const void* x, int32_t x_stride, const float* s, const void* identity, int32_t identity_stride,
                        void* y, int32_t y_stride, int32_t dtype, int32_t B, int32_t HW, int32_t C, void* stream) {
  CTDET_CHECK(x && s && y, "ese_scale: null pointer");
  return launch_ese_scale(x, x_stride, s, identity, identity_stride, y, y_stride, dtype, B, HW, C, (hipStream_t)stream);
}

int32_t ctdet_pack_weights(const float* w, void* packed, int32_t O, int32_t I, int32_t R, int32_t S, int32_t chans_pad,
                           int32_t rows_pad, int32_t Kpad, int32_t korder, int32_t transposed, void* stream) {
  CTDET_CHECK(w && packed, "pack_weights: null pointer");
  return launch_pack_weights(w, packed, O, I, R, S, chans_pad, rows_pad, Kpad, korder, transposed, (hipStream_t)stream);
}

int32_t ctdet_split_weights(const float* w_packed_f32, void* w_split, int64_t n, void* stream) {
  CTDET_CHECK(w_packed_f32 && w_split && n >= 0, "split_weights: bad arguments");
  return launch_split_weights(w_packed_f32, w_split, (long)n, (hipStream_t)stream);
}

int32_t ctdet_pack_weights_batch(const ctdet_pack_desc* table_dev, int32_t n, int32_t total_blocks, void* stream) {
  CTDET_CHECK(n >= 0 && total_blocks >= 0 && (n == 0 || table_dev), "pack_weights_batch: bad arguments");
  static_assert(sizeof(ctdet_pack_desc) == 56, "ctdet_pack_desc layout");
  return launch_pack_weights_batch(table_dev, n, total_blocks, (hipStream_t)stream);
}

int32_t ctdet_pack_weights_x3(const float* w, void* packed, float* scale_out, int32_t O, int32_t I, int32_t R, int32_t S,
                              int32_t chans_pad, int32_t rows_pad, int32_t Kpad, int32_t layout, int32_t transposed,
                              int32_t scale_n, void* stream) {
  return launch_pack_weights_x3(w, packed, scale_out, O, I, R, S, chans_pad, rows_pad, Kpad, layout, transposed, scale_n,
                                (hipStream_t)stream);
}

int32_t ctdet_pack_weights_x3_batch(const ctdet_pack3_desc* table_dev, int32_t n, int32_t total_blocks, void* stream) {
  CTDET_CHECK(n >= 0 && total_blocks >= 0 && (n == 0 || table_dev), "pack_weights_x3_batch: bad arguments");
  static_assert(sizeof(ctdet_pack3_desc) == 72, "ctdet_pack3_desc layout");
  return launch_pack_weights_x3_batch(table_dev, n, total_blocks, (hipStream_t)stream);
}

int32_t ctdet_dwconvT_add(const void* x, const float* w, const void* skip, void* y, int32_t dtype, int32_t B,
                          int32_t H, int32_t W, int32_t C, int32_t f, int32_t in_stride, int32_t skip_stride,
                          int32_t out_stride, void* stream) {
  CTDET_CHECK(x && w && y, "dwconvT: null pointer");
  return launch_dwconvT_add(x, w, skip, y, dtype, B, H, W, C, f, in_stride, skip_stride, out_stride,
                            (hipStream_t)stream);
}

int32_t ctdet_dwconv3x3_fwd(const void* x, int32_t x_stride, const float* w, void* y, int32_t y_stride, int32_t B, int32_t H,
                            int32_t W, int32_t C, int32_t stride, int32_t rot180, int32_t dtype, void* stream) {
  CTDET_CHECK(x && w && y, "dwconv3x3: null pointer");
  CTDET_CHECK(rot180 == 0 || rot180 == 1, "dwconv3x3: rot180 %d", rot180);
  const int strides[2] = {x_stride, y_stride};
  const int rc = dwconv3x3_check(dtype, B, H, W, C, stride, strides, 2);
  if (rc) return rc;
  return launch_dwconv3x3(x, x_stride, w, y, y_stride, B, H, W, C, stride, rot180, dtype, (hipStream_t)stream);
}

size_t ctdet_dwconv3x3_wgrad_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype) {
  return dwconv3x3_wgrad_workspace_bytes(B, H, W, C, dtype);
}

int32_t ctdet_dwconv3x3_wgrad(const void* x, int32_t x_stride, const void* dy, int32_t dy_stride, float* workspace, float* dw,
                              float scale, int32_t accumulate, int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride,
                              int32_t dtype, void* stream) {
  // an empty problem (the tensors of an empty batch have no storage) still writes dw: only then may x / dy be null
  CTDET_CHECK(dw && ((x && dy) || B == 0 || H == 0 || W == 0), "dwconv3x3_wgrad: null pointer");
  CTDET_CHECK(accumulate == 0 || accumulate == 1, "dwconv3x3_wgrad: accumulate %d", accumulate);
  const int strides[2] = {x_stride, dy_stride};
  const int rc = dwconv3x3_check(dtype, B, H, W, C, stride, strides, 2);
  if (rc) return rc;
  CTDET_CHECK(stride == 1, "dwconv3x3_wgrad: stride %d: only the stride-1 backward is built", stride);
  CTDET_CHECK(workspace || dwconv3x3_wgrad_workspace_bytes(B, H, W, C, dtype) == 0, "dwconv3x3_wgrad: null workspace");
  CTDET_CHECK(((uintptr_t)dw & 3) == 0 && ((uintptr_t)workspace & 3) == 0, "dwconv3x3_wgrad: misaligned dw / workspace");
  return launch_dwconv3x3_wgrad(x, x_stride, dy, dy_stride, workspace, dw, scale, accumulate, B, H, W, C, dtype,
                                (hipStream_t)stream);
}

size_t ctdet_decode_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t K) {
  return decode_workspace_bytes(B, H, W, C, K);
}

static int32_t decode_entry(bool flip, const float* heat, int32_t heat_stride, const float* wh, int32_t wh_stride,
                            const float* reg, int32_t reg_stride, int32_t B, int32_t H, int32_t W, int32_t C, int32_t K,
                            float down_ratio, float heat_floor, void* workspace, float* boxes, float* scores,
                            int32_t* classes, int32_t* inds, void* stream) {
  CTDET_CHECK(heat && workspace && scores && classes, "decode: null pointer");
  // wh == NULL: scores, classes and inds only (the boxes come from ctdet_head_sparse_x3_fwd, which needs the inds)
  CTDET_CHECK(wh ? boxes != nullptr : (inds != nullptr && !reg), "decode: %s", wh ? "null boxes" : "without wh: inds required, reg must be null");
  CTDET_CHECK(B >= 0 && H > 0 && W > 0, "decode: bad shape B=%d H=%d W=%d", B, H, W);
  CTDET_CHECK(heat_floor >= 0.f && heat_floor < 1.f, "decode: heat_floor %g outside [0, 1)", (double)heat_floor);
  DecArgs a;
  a.heat = heat; a.wh = wh; a.reg = reg; a.heat_stride = heat_stride; a.wh_stride = wh_stride; a.reg_stride = reg_stride;
  a.B = B; a.H = H; a.W = W; a.C = C; a.K = K; a.down_ratio = down_ratio;
  memcpy(&a.floor_bits, &heat_floor, 4);
  a.ws = (uint32_t*)workspace; a.boxes = boxes; a.scores = scores; a.classes = classes; a.inds = inds;
  return launch_decode(a, flip, (hipStream_t)stream);
}

int32_t ctdet_decode(const float* heat, int32_t heat_stride, const float* wh, int32_t wh_stride, const float* reg,
                     int32_t reg_stride, int32_t B, int32_t H, int32_t W, int32_t C, int32_t K, float down_ratio,
                     float heat_floor, void* workspace, float* boxes, float* scores, int32_t* classes, int32_t* inds,
                     void* stream) {
  return decode_entry(false, heat, heat_stride, wh, wh_stride, reg, reg_stride, B, H, W, C, K, down_ratio, heat_floor,
                      workspace, boxes, scores, classes, inds, stream);
}

int32_t ctdet_decode_flip(const float* heat, int32_t heat_stride, const float* wh, int32_t wh_stride, const float* reg,
                          int32_t reg_stride, int32_t B, int32_t H, int32_t W, int32_t C, int32_t K, float down_ratio,
                          float heat_floor, void* workspace, float* boxes, float* scores, int32_t* classes, int32_t* inds,
                          void* stream) {
  return decode_entry(true, heat, heat_stride, wh, wh_stride, reg, reg_stride, B, H, W, C, K, down_ratio, heat_floor,
                      workspace, boxes, scores, classes, inds, stream);
}

int32_t ctdet_postprocess(const float* boxes, const float* scores, const int32_t* classes, int32_t B, int32_t K,
                          int32_t max_det, float score_thresh, const float* img_params, float* out_boxes,
                          float* out_scores, int32_t* out_classes, int32_t* counts, void* stream) {
  CTDET_CHECK(boxes && scores && classes && img_params && out_boxes && out_scores && out_classes && counts,
              "postprocess: null pointer");
  return launch_postprocess(boxes, scores, classes, B, K, max_det, score_thresh, img_params, out_boxes, out_scores,
                            out_classes, counts, (hipStream_t)stream);
}

int32_t ctdet_postprocess_affine(const float* boxes, const float* scores, const int32_t* classes, int32_t B, int32_t K,
                                 int32_t max_det, float score_thresh, const float* img_params6, float* out_boxes,
                                 float* out_scores, int32_t* out_classes, int32_t* counts, void* stream) {
  CTDET_CHECK(boxes && scores && classes && img_params6 && out_boxes && out_scores && out_classes && counts,
              "postprocess_affine: null pointer");
  CTDET_CHECK(B >= 0 && K >= 1, "postprocess_affine: bad shape B=%d K=%d", B, K);
  return launch_postprocess_affine(boxes, scores, classes, B, K, max_det, score_thresh, img_params6, out_boxes, out_scores,
                                   out_classes, counts, (hipStream_t)stream);
}

int32_t ctdet_decode_status(const void* workspace, int32_t B, int32_t H, int32_t W, int32_t C, int32_t K, void* stream) {
  long words = 0;
  int below = 0;
  const int flag = decode_status_words(H, W, C, K, &words, &below);
  for (int b = 0; b < B; ++b) {
    uint32_t st[16];
    hipError_t e = hipMemcpyAsync(st, (const char*)workspace + (size_t)words * 4 * b, sizeof(st), hipMemcpyDeviceToHost,
                                  (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    CTDET_CHECK(e == hipSuccess, "decode_status: copy failed: %s", hipGetErrorString(e));
    if (st[flag]) {
      ctdet_set_error("decode: image %d overflowed the candidate buffer", b);
      return -75;
    }
    if (st[below]) {
      ctdet_set_error("decode: image %d holds positive heat values below the promised heat_floor", b);
      return -22;
    }
  }
  return 0;
}

int32_t ctdet_gaussian_targets(const float* boxes, const int64_t* classes, const int32_t* counts, int32_t B,
                               int32_t Nmax, int32_t H, int32_t W, int32_t C, float* hm, float* wh, float* reg,
                               int64_t* ind, uint8_t* reg_mask, void* stream) {
  CTDET_CHECK(boxes && classes && counts && hm && wh && reg && ind && reg_mask, "gaussian_targets: null pointer");
  CTDET_CHECK(Nmax >= 1, "gaussian_targets: Nmax must be >= 1");
  return launch_gaussian_targets(boxes, classes, counts, B, Nmax, H, W, C, hm, wh, reg, ind, reg_mask,
                                 (hipStream_t)stream);
}

int32_t ctdet_gaussian_radius(const int32_t* hw_pairs, int32_t n, double* out_radius, int32_t* out_int, void* stream) {
  CTDET_CHECK(hw_pairs, "gaussian_radius: null pointer");
  return launch_gaussian_radius(hw_pairs, n, out_radius, out_int, (hipStream_t)stream);
}

size_t ctdet_focal_loss_workspace_bytes(int64_t numel) { return focal_workspace_bytes((long)numel); }

int32_t ctdet_focal_loss(const float* logits, const float* gt, const float* alpha, int32_t B, int32_t H, int32_t W,
                         int32_t C, float grad_scale, void* workspace, float* loss, float* stats, float* grad,
                         void* stream) {
  CTDET_CHECK(logits && gt && alpha && workspace && loss && stats, "focal_loss: null pointer");
  return launch_focal_loss(logits, gt, alpha, B, H, W, C, grad_scale, workspace, loss, stats, grad, (hipStream_t)stream);
}

int32_t ctdet_reg_l1_loss(const float* pred, int32_t pred_stride, const uint8_t* mask, const int64_t* ind,
                          const float* target, int32_t B, int32_t N, int32_t HW, float grad_scale, float* loss,
                          float* grad, int32_t grad_stride, void* stream) {
  CTDET_CHECK(pred && mask && ind && target && loss, "reg_l1_loss: null pointer");
  return launch_reg_l1(pred, pred_stride, mask, ind, target, B, N, HW, grad_scale, loss, grad, grad_stride,
                       (hipStream_t)stream);
}

size_t ctdet_chan_workspace_bytes(int32_t C) { return chan_reduce_workspace_bytes(C); }

int32_t ctdet_bn_train_fwd(const void* y, int32_t y_stride, const void* res, int32_t res_stride, void* z,
                           int32_t z_stride, int32_t M, int32_t C, const float* gamma, const float* beta, float eps,
                           float momentum, float* running_mean, float* running_var, float* save_mean,
                           float* save_invstd, float* scale, float* shift, void* workspace, int32_t relu, int32_t dtype,
                           void* stream) {
  CTDET_CHECK(y && z && gamma && beta && save_mean && save_invstd && scale && shift && workspace, "bn_train_fwd: null pointer");
  CTDET_CHECK(M > 0, "bn_train_fwd: empty batch");
  BnArgs a = {};
  a.dtype = dtype; a.M = M; a.C = C; a.relu = relu;
  a.y = y; a.y_stride = y_stride; a.res = res; a.res_stride = res_stride; a.z_out = z; a.z_stride = z_stride;
  a.gamma = gamma; a.beta = beta; a.eps = eps; a.momentum = momentum; a.running_mean = running_mean; a.running_var = running_var;
  a.save_mean = save_mean; a.save_invstd = save_invstd; a.save_scale = scale; a.save_shift = shift; a.workspace = workspace;
  return launch_bn_train_fwd(a, (hipStream_t)stream);
}

int32_t ctdet_bn_train_bwd(const void* dz, int32_t dz_stride, const void* z, int32_t z_stride, const void* y,
                           int32_t y_stride, const float* mean, const float* invstd, const float* scale, int32_t M,
                           int32_t C, int32_t relu, void* dy, int32_t dy_stride, void* dres, int32_t dres_stride,
                           float* dgamma, float* dbeta, float grad_mult, void* workspace, int32_t dtype, void* stream) {
  CTDET_CHECK(dz && dy && dgamma && dbeta && workspace, "bn_train_bwd: null pointer");
  CTDET_CHECK(!relu || z, "bn_train_bwd: relu backward needs z");
  CTDET_CHECK(!y || (mean && invstd && scale), "bn_train_bwd: statistics missing");
  BnArgs a = {};
  a.dtype = dtype; a.M = M; a.C = C; a.relu = relu;
  a.dz = dz; a.dz_stride = dz_stride; a.z = z; a.z_stride = z_stride; a.y = y; a.y_stride = y_stride;
  a.mean = mean; a.invstd = invstd; a.scale = scale; a.dy = dy; a.dy_stride = dy_stride; a.dres = dres; a.dres_stride = dres_stride;
  a.dgamma = dgamma; a.dbeta = dbeta; a.grad_mult = grad_mult; a.workspace = workspace;
  return launch_bn_train_bwd(a, (hipStream_t)stream);
}

static const int SYNC_BN_MAX_WORLD = 4096;

int32_t ctdet_bn_local_stats(const void* y, int32_t y_stride, int32_t M, int32_t C, int32_t rank, int32_t world,
                             double* stats, void* workspace, int32_t dtype, void* stream) {
  CTDET_CHECK(M > 0, "bn_local_stats: empty batch on rank %d (SyncBatchNorm needs at least one row on every rank)", rank);
  CTDET_CHECK(y && stats && workspace, "bn_local_stats: null pointer");
  CTDET_CHECK(world >= 1 && world <= SYNC_BN_MAX_WORLD && rank >= 0 && rank < world, "bn_local_stats: rank %d of world %d",
              rank, world);
  BnArgs a = {};
  a.dtype = dtype; a.M = M; a.C = C; a.y = y; a.y_stride = y_stride;
  a.rank = rank; a.world = world; a.slots = stats; a.workspace = workspace;
  return launch_bn_local_stats(a, (hipStream_t)stream);
}

int32_t ctdet_bn_sync_fwd(const void* y, int32_t y_stride, const void* res, int32_t res_stride, void* z, int32_t z_stride,
                          int32_t M, int32_t C, const double* stats, int32_t world, const float* gamma, const float* beta,
                          float eps, float momentum, float* running_mean, float* running_var, float* save_mean,
                          float* save_invstd, float* scale, float* shift, int32_t relu, int32_t dtype, void* stream) {
  CTDET_CHECK(y && z && stats && gamma && beta && save_mean && save_invstd && scale && shift, "bn_sync_fwd: null pointer");
  CTDET_CHECK(!running_mean == !running_var, "bn_sync_fwd: running_mean and running_var go together");
  CTDET_CHECK(M > 0, "bn_sync_fwd: empty batch");
  CTDET_CHECK(world >= 1 && world <= SYNC_BN_MAX_WORLD, "bn_sync_fwd: world %d", world);
  BnArgs a = {};
  a.dtype = dtype; a.M = M; a.C = C; a.relu = relu;
  a.y = y; a.y_stride = y_stride; a.res = res; a.res_stride = res_stride; a.z_out = z; a.z_stride = z_stride;
  a.stats = stats; a.world = world;
  a.gamma = gamma; a.beta = beta; a.eps = eps; a.momentum = momentum; a.running_mean = running_mean; a.running_var = running_var;
  a.save_mean = save_mean; a.save_invstd = save_invstd; a.save_scale = scale; a.save_shift = shift;
  return launch_bn_sync_fwd(a, (hipStream_t)stream);
}

int32_t ctdet_bn_local_grad_sums(const void* dz, int32_t dz_stride, const void* z, int32_t z_stride, const void* y,
                                 int32_t y_stride, const float* mean, const float* invstd, int32_t M, int32_t C, int32_t relu,
                                 int32_t rank, int32_t world, double* sums, float* dgamma, float* dbeta, float grad_mult,
                                 void* workspace, int32_t dtype, void* stream) {
  CTDET_CHECK(dz && sums && dgamma && dbeta && workspace, "bn_local_grad_sums: null pointer");
  CTDET_CHECK(!relu || z, "bn_local_grad_sums: relu backward needs z");
  CTDET_CHECK(!y || (mean && invstd), "bn_local_grad_sums: statistics missing");
  CTDET_CHECK(M > 0, "bn_local_grad_sums: empty batch on rank %d", rank);
  CTDET_CHECK(world >= 1 && world <= SYNC_BN_MAX_WORLD && rank >= 0 && rank < world,
              "bn_local_grad_sums: rank %d of world %d", rank, world);
  BnArgs a = {};
  a.dtype = dtype; a.M = M; a.C = C; a.relu = relu;
  a.dz = dz; a.dz_stride = dz_stride; a.z = z; a.z_stride = z_stride; a.y = y; a.y_stride = y_stride;
  a.mean = mean; a.invstd = invstd; a.rank = rank; a.world = world; a.slots = sums;
  a.dgamma = dgamma; a.dbeta = dbeta; a.grad_mult = grad_mult; a.workspace = workspace;
  return launch_bn_local_grad_sums(a, (hipStream_t)stream);
}

int32_t ctdet_bn_sync_bwd(const void* dz, int32_t dz_stride, const void* z, int32_t z_stride, const void* y, int32_t y_stride,
                          const float* mean, const float* invstd, const float* scale, const double* stats,
                          const double* sums, int32_t world, int32_t M, int32_t C, int32_t relu, void* dy, int32_t dy_stride,
                          void* dres, int32_t dres_stride, int32_t dtype, void* stream) {
  CTDET_CHECK(dz && y && mean && invstd && scale && stats && sums && dy, "bn_sync_bwd: null pointer");
  CTDET_CHECK(!relu || z, "bn_sync_bwd: relu backward needs z");
  CTDET_CHECK(M > 0, "bn_sync_bwd: empty batch");
  CTDET_CHECK(world >= 1 && world <= SYNC_BN_MAX_WORLD, "bn_sync_bwd: world %d", world);
  BnArgs a = {};
  a.dtype = dtype; a.M = M; a.C = C; a.relu = relu;
  a.dz = dz; a.dz_stride = dz_stride; a.z = z; a.z_stride = z_stride; a.y = y; a.y_stride = y_stride;
  a.mean = mean; a.invstd = invstd; a.scale = scale; a.stats = stats; a.sums = sums; a.world = world;
  a.dy = dy; a.dy_stride = dy_stride; a.dres = dres; a.dres_stride = dres_stride;
  return launch_bn_sync_bwd(a, (hipStream_t)stream);
}

int32_t ctdet_conv_wgrad(const ctdet_conv_desc* d, const void* x, const void* dy, float* dw, float scale, void* stream) {
  return ctdet_conv_wgrad_oihw(d, x, dy, dw, scale, 0, 0, 0, 0, stream);
}

int32_t ctdet_conv_wgrad_oihw(const ctdet_conv_desc* d, const void* x, const void* dy, float* dw, float scale, int32_t taps,
                              int32_t cin_k, int32_t cin_real, int32_t cout_real, void* stream) {
  CTDET_CHECK(d && x && dy && dw, "conv_wgrad: null pointer");
  CTDET_CHECK(taps == 0 || (cin_k > 0 && cin_real > 0 && cin_real <= cin_k && taps * cin_k == d->R * d->S * d->Cin &&
                            cout_real > 0 && cout_real <= d->Cout),
              "conv_wgrad_oihw: taps=%d cin_k=%d cin_real=%d do not factor K=%d", taps, cin_k, cin_real, d->R * d->S * d->Cin);
  WgradArgs a;
  a.perm_rs = taps; a.perm_cin = cin_k; a.cin_real = cin_real; a.cout_real = cout_real;
  a.x = x; a.dy = dy; a.dw = dw;
  a.B = d->B; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.in_stride = d->in_stride; a.Cout = d->Cout; a.Ho = d->Ho;
  a.Wo = d->Wo; a.dy_stride = d->out_stride; a.R = d->R; a.S = d->S; a.stride = d->stride; a.pad = d->pad; a.dil = d->dil;
  a.K = d->R * d->S * d->Cin; a.M = d->B * d->Ho * d->Wo; a.msplit = 1; a.scale = scale;
  if (a.M == 0) return 0;
  if (d->compute_dtype == CTDET_DT_F32) return launch_conv_wgrad_f32(a, (hipStream_t)stream);
  if (d->compute_dtype == CTDET_DT_F16X3) return launch_conv_wgrad_x3(a, (hipStream_t)stream);
  CTDET_CHECK(d->compute_dtype == CTDET_DT_F16, "conv_wgrad: bad compute dtype %d", d->compute_dtype);
  return launch_conv_wgrad(a, (hipStream_t)stream);
}

int32_t ctdet_grad_scatter_oihw(const void* const* src, void* const* dst, const int32_t* cout, const int32_t* cin_real,
                                const int32_t* cin_k, const int32_t* taps, int32_t n, void* stream) {
  CTDET_CHECK(n >= 0 && (n == 0 || (src && dst && cout && cin_real && cin_k && taps)), "grad_scatter_oihw: null pointer");
  return launch_grad_scatter_oihw(src, dst, cout, cin_real, cin_k, taps, n, (hipStream_t)stream);
}

int32_t ctdet_depth_to_space2(const void* src, int32_t src_stride, void* dst, int32_t dst_stride, int32_t B, int32_t H,
                              int32_t W, int32_t C, int32_t Hs, int32_t Ws, int32_t dtype, void* stream) {
  CTDET_CHECK(src && dst, "depth_to_space2: null pointer");
  return launch_depth_to_space2(src, src_stride, dst, dst_stride, B, H, W, C, Hs, Ws, dtype, (hipStream_t)stream);
}

int32_t ctdet_maxpool3x3s2_bwd(const void* x, int32_t x_stride, const void* dz, int32_t dz_stride, void* dx, int32_t dx_stride,
                               int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ceil_nopad, void* stream) {
  CTDET_CHECK(x && dz && dx, "maxpool3x3s2_bwd: null pointer");
  int Ho, Wo, pad;
  if (ceil_nopad) {
    pad = 0;
    Ho = (H - 3 + 1) / 2 + 1; Wo = (W - 3 + 1) / 2 + 1;
    if ((Ho - 1) * 2 >= H) --Ho;
    if ((Wo - 1) * 2 >= W) --Wo;
  } else {
    pad = 1;
    Ho = (H - 1) / 2 + 1; Wo = (W - 1) / 2 + 1;
  }
  return launch_maxpool3x3s2_bwd(x, x_stride, dz, dz_stride, dx, dx_stride, dtype, B, H, W, C, pad, Ho, Wo, (hipStream_t)stream);
}

int32_t ctdet_ese_dot(const void* dy, int32_t dy_stride, const void* x, int32_t x_stride, int32_t dtype, int32_t B, int32_t HW,
                      int32_t C, float* out, void* stream) {
  CTDET_CHECK(dy && x && out, "ese_dot: null pointer");
  return launch_ese_dot(dy, dy_stride, x, x_stride, dtype, B, HW, C, out, (hipStream_t)stream);
}

int32_t ctdet_ese_bwd(const void* dy, int32_t dy_stride, const float* gate, const float* pooled_grad, void* dx, int32_t dx_stride,
                      int32_t dtype, int32_t B, int32_t HW, int32_t C, void* stream) {
  CTDET_CHECK(dy && gate && pooled_grad && dx, "ese_bwd: null pointer");
  return launch_ese_bwd(dy, dy_stride, gate, pooled_grad, dx, dx_stride, dtype, B, HW, C, (hipStream_t)stream);
}

int32_t ctdet_maxpool2x2_bwd(const void* x, int32_t x_stride, const void* dz, int32_t dz_stride, void* dx,
                             int32_t dx_stride, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream) {
  CTDET_CHECK(x && dz && dx, "maxpool2x2_bwd: null pointer");
  return launch_maxpool2x2_bwd(x, x_stride, dz, dz_stride, dx, dx_stride, dtype, B, H, W, C, (hipStream_t)stream);
}

int32_t ctdet_dwconvT_bwd(const void* x, int32_t x_stride, const void* dz, int32_t dz_stride, const float* w, void* dx,
                          int32_t dx_stride, float* dw, int32_t B, int32_t H, int32_t W, int32_t C, int32_t f,
                          int32_t dtype, void* stream) {
  CTDET_CHECK(x && dz && w && dx && dw, "dwconvT_bwd: null pointer");
  return launch_dwconvT_bwd(x, x_stride, dz, dz_stride, w, dx, dx_stride, dw, dtype, B, H, W, C, f, (hipStream_t)stream);
}

int32_t ctdet_dcn_cols(const void* x, int32_t x_stride, const float* om, int32_t om_stride, void* col, int32_t B,
                       int32_t H, int32_t W, int32_t Cin, int32_t mask_is_prob, int32_t dtype, void* stream) {
  CTDET_CHECK(x && om && col, "dcn_cols: null pointer");
  CTDET_DCN_MASK_MODE("dcn_cols", mask_is_prob);
  DcnBwdArgs a = {};
  a.dtype = dtype; a.x = x; a.x_stride = x_stride; a.om = om; a.om_stride = om_stride; a.col = col;
  a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.mask_mode = mask_is_prob;
  return launch_dcn_cols(a, (hipStream_t)stream);
}

int32_t ctdet_dcn_col2im_coord(const void* dcol, const void* x, int32_t x_stride, const float* om, int32_t om_stride,
                               float* dx, void* dom, int32_t dom_stride, int32_t dom_dtype, int32_t B, int32_t H, int32_t W,
                               int32_t Cin, int32_t mask_is_prob, int32_t dcol_chunked, int32_t dtype, void* stream) {
  CTDET_CHECK(dcol && x && om && dx && dom, "dcn_col2im_coord: null pointer");
  CTDET_DCN_MASK_MODE("dcn_col2im_coord", mask_is_prob);
  CTDET_CHECK(dom_dtype == CTDET_DT_F32 || (dom_dtype == CTDET_DT_F16 && dtype == CTDET_DT_F16),
              "dcn_col2im_coord: dom dtype %d with data dtype %d", dom_dtype, dtype);
  DcnBwdArgs a = {};
  a.dtype = dtype; a.x = x; a.x_stride = x_stride; a.om = om; a.om_stride = om_stride;
  a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.mask_mode = mask_is_prob;
  a.dcol = dcol; a.dcol_chunked = dcol_chunked; a.dx = dx; a.dom = dom; a.dom_stride = dom_stride; a.dom_dtype = dom_dtype;
  return launch_dcn_col2im_coord(a, (hipStream_t)stream);
}

int32_t ctdet_dcn_col2im_fused(const float* dy, int32_t dy_stride, int32_t K, const void* w_packed, const float* w_scale,
                               const float* x, int32_t x_stride, const float* om, int32_t om_stride, float* dx, float* dom,
                               int32_t dom_stride, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t mask_is_prob, void* stream) {
  CTDET_CHECK(dy && w_packed && w_scale && x && om && dx && dom, "dcn_col2im_fused: null pointer");
  CTDET_DCN_MASK_MODE("dcn_col2im_fused", mask_is_prob);
  DcnBwdArgs a = {};
  a.dtype = CTDET_F32; a.x = x; a.x_stride = x_stride; a.om = om; a.om_stride = om_stride;
  a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.mask_mode = mask_is_prob;
  a.dy = dy; a.dy_stride = dy_stride; a.K = K; a.wpk = w_packed; a.wscale = w_scale;
  a.dx = dx; a.dom = dom; a.dom_stride = dom_stride; a.dom_dtype = CTDET_F32;
  return launch_dcn_col2im_fused(a, (hipStream_t)stream);
}

int32_t ctdet_sgd_momentum(float* param, const float* grad, float* momentum_buf, int64_t n, const float* lr_dev,
                           float momentum, float weight_decay, int32_t first_step, void* stream) {
  CTDET_CHECK(param && grad && momentum_buf && lr_dev, "sgd: null pointer");
  CTDET_CHECK(n >= 0, "sgd: n=%lld", (long long)n);
  return launch_sgd(param, grad, momentum_buf, (long)n, lr_dev, momentum, weight_decay, first_step, (hipStream_t)stream);
}

int32_t ctdet_sgd_momentum_runs(float* param, const float* grad, float* momentum_buf, int64_t n, const int64_t* run_end,
                                const int32_t* run_lr_index, const float* run_weight_decay, const float* lr_table,
                                int32_t nruns, float momentum, int32_t first_step, void* stream) {
  CTDET_CHECK(param && grad && momentum_buf && run_end && run_lr_index && run_weight_decay && lr_table, "sgd_runs: null pointer");
  CTDET_CHECK((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)momentum_buf) & 15) == 0,
              "sgd_runs: param, grad and momentum_buf must be 16-byte aligned");
  CTDET_CHECK(n >= 0 && nruns >= 0, "sgd_runs: n=%lld nruns=%d", (long long)n, nruns);
  return launch_sgd_runs(param, grad, momentum_buf, (long)n, (const long*)run_end, run_lr_index, run_weight_decay, lr_table,
                         nruns, momentum, first_step, (hipStream_t)stream);
}

int32_t ctdet_grad_chunk_norms(const float* grad, int64_t n, const int64_t* chunk_start, const int32_t* chunk_len,
                               int32_t nchunks, int32_t norm_type, float* partials, void* stream) {
  CTDET_CHECK(grad && chunk_start && chunk_len && partials, "grad_chunk_norms: null pointer");
  CTDET_CHECK(n >= 0 && nchunks >= 0, "grad_chunk_norms: n=%lld nchunks=%d", (long long)n, nchunks);
  CTDET_CHECK(norm_type >= CTDET_NORM_L1 && norm_type <= CTDET_NORM_INF, "grad_chunk_norms: norm type %d", norm_type);
  CTDET_CHECK(((uintptr_t)grad & 15) == 0, "grad_chunk_norms: grad must be 16-byte aligned");
  return launch_grad_chunk_norms(grad, (long)n, (const long*)chunk_start, chunk_len, nchunks, norm_type, partials,
                                 (hipStream_t)stream);
}

int32_t ctdet_grad_clip_coefs(const float* partials, const int32_t* param_chunk_end, int32_t nparams, int32_t nchunks,
                              int32_t norm_type, float clip_value, float* norms, float* coefs, void* stream) {
  CTDET_CHECK(partials && param_chunk_end && norms && coefs, "grad_clip_coefs: null pointer");
  CTDET_CHECK(nparams >= 0 && nchunks >= 0, "grad_clip_coefs: nparams=%d nchunks=%d", nparams, nchunks);
  CTDET_CHECK(norm_type >= CTDET_NORM_L1 && norm_type <= CTDET_NORM_INF, "grad_clip_coefs: norm type %d", norm_type);
  CTDET_CHECK(clip_value > 0.f, "grad_clip_coefs: clip value %g", (double)clip_value);
  return launch_grad_clip_coefs(partials, param_chunk_end, nparams, nchunks, norm_type, clip_value, norms, coefs,
                                (hipStream_t)stream);
}

int32_t ctdet_sgd_momentum_runs_clip(float* param, const float* grad, float* momentum_buf, int64_t n, const int64_t* run_end,
                                     const int32_t* run_lr_index, const float* run_weight_decay, const float* lr_table,
                                     int32_t nruns, float momentum, int32_t first_step, int32_t nesterov, int32_t clip_type,
                                     float clip_value, const float* coefs, void* stream) {
  CTDET_CHECK(param && grad && momentum_buf && run_end && run_lr_index && run_weight_decay && lr_table,
              "sgd_runs_clip: null pointer");
  CTDET_CHECK((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)momentum_buf) & 15) == 0,
              "sgd_runs_clip: param, grad and momentum_buf must be 16-byte aligned");
  CTDET_CHECK(n >= 0 && nruns >= 0, "sgd_runs_clip: n=%lld nruns=%d", (long long)n, nruns);
  CTDET_CHECK(clip_type >= CTDET_CLIP_NONE && clip_type <= CTDET_CLIP_NORM, "sgd_runs_clip: clip type %d", clip_type);
  CTDET_CHECK(clip_type == CTDET_CLIP_NONE || clip_value > 0.f, "sgd_runs_clip: clip value %g", (double)clip_value);
  CTDET_CHECK(clip_type != CTDET_CLIP_NORM || coefs, "sgd_runs_clip: norm clipping needs coefs (one per run)");
  return launch_sgd_runs_clip(param, grad, momentum_buf, (long)n, (const long*)run_end, run_lr_index, run_weight_decay, lr_table,
                              nruns, momentum, first_step, nesterov, clip_type, clip_value, coefs, (hipStream_t)stream);
}

#define CTDET_ADAM_BETAS(what)                                                                                          \
  CTDET_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, what ": betas (%g, %g) outside [0, 1)", beta1, beta2)

int32_t ctdet_adam_advance(int64_t* step_dev, float* bias_dev, double beta1, double beta2, void* stream) {
  CTDET_CHECK(step_dev && bias_dev, "adam_advance: null pointer");
  CTDET_ADAM_BETAS("adam_advance");
  return launch_adam_advance((long long*)step_dev, bias_dev, beta1, beta2, (hipStream_t)stream);
}

int32_t ctdet_adam_runs(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, int64_t n,
                        const int64_t* run_end, const int32_t* run_lr_index, const float* run_weight_decay,
                        const float* lr_table, int32_t nruns, const float* bias_dev, double beta1, double beta2, double eps,
                        int32_t decoupled, int32_t amsgrad, int32_t clip_type, float clip_value, const float* coefs,
                        void* stream) {
  CTDET_CHECK(param && grad && exp_avg && exp_avg_sq && run_end && run_lr_index && run_weight_decay && lr_table && bias_dev,
              "adam_runs: null pointer");
  CTDET_CHECK(!amsgrad || max_exp_avg_sq, "adam_runs: amsgrad needs max_exp_avg_sq");
  CTDET_CHECK((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq |
                (amsgrad ? (uintptr_t)max_exp_avg_sq : 0)) & 15) == 0,
              "adam_runs: param, grad and the moment buffers must be 16-byte aligned");
  CTDET_CHECK(n >= 0 && nruns >= 0, "adam_runs: n=%lld nruns=%d", (long long)n, nruns);
  CTDET_ADAM_BETAS("adam_runs");
  CTDET_CHECK(eps > 0.0, "adam_runs: eps %g must be positive", eps);
  CTDET_CHECK(clip_type >= CTDET_CLIP_NONE && clip_type <= CTDET_CLIP_NORM, "adam_runs: clip type %d", clip_type);
  CTDET_CHECK(clip_type == CTDET_CLIP_NONE || clip_value > 0.f, "adam_runs: clip value %g", (double)clip_value);
  CTDET_CHECK(clip_type != CTDET_CLIP_NORM || coefs, "adam_runs: norm clipping needs coefs (one per run)");
  return launch_adam_runs(param, grad, exp_avg, exp_avg_sq, amsgrad ? max_exp_avg_sq : nullptr, (long)n, (const long*)run_end,
                          run_lr_index, run_weight_decay, lr_table, nruns, bias_dev, beta1, beta2, eps, decoupled, amsgrad,
                          clip_type, clip_value, coefs, (hipStream_t)stream);
}

int32_t ctdet_ema_advance(int64_t* updates_dev, float* weight_dev, double decay, int32_t warmup, void* stream) {
  CTDET_CHECK(updates_dev && weight_dev, "ema_advance: null pointer");
  CTDET_CHECK(decay >= 0.0 && decay < 1.0, "ema_advance: decay %g outside [0, 1)", decay);
  return launch_ema_advance((long long*)updates_dev, weight_dev, decay, warmup != 0, (hipStream_t)stream);
}

#define CTDET_EMA_SEGMENTS(what)                                                                               \
  CTDET_CHECK(nseg >= 0 && max_len >= 0, what ": nseg=%d max_len=%lld", nseg, (long long)max_len);             \
  if (nseg == 0) return 0

int32_t ctdet_ema_lerp_segments(const float* const* live_ptrs_dev, float* ema, const int64_t* seg_start_dev, int32_t nseg,
                                int64_t max_len, const float* weight_dev, void* stream) {
  CTDET_EMA_SEGMENTS("ema_lerp_segments");
  CTDET_CHECK(live_ptrs_dev && ema && seg_start_dev && weight_dev, "ema_lerp_segments: null pointer");
  return launch_ema_lerp_segments(live_ptrs_dev, ema, (const long*)seg_start_dev, nseg, (long)max_len, weight_dev,
                                  (hipStream_t)stream);
}

int32_t ctdet_ema_swap_segments(float* const* live_ptrs_dev, float* ema, const int64_t* seg_start_dev, int32_t nseg,
                                int64_t max_len, void* stream) {
  CTDET_EMA_SEGMENTS("ema_swap_segments");
  CTDET_CHECK(live_ptrs_dev && ema && seg_start_dev, "ema_swap_segments: null pointer");
  return launch_ema_swap_segments(live_ptrs_dev, ema, (const long*)seg_start_dev, nseg, (long)max_len, (hipStream_t)stream);
}

#define CTDET_PRECISE_BN_SEGMENTS(what)                                                                                     \
  CTDET_CHECK(nseg >= 0 && max_len >= 0 && total >= 0, what ": nseg=%d max_len=%lld total=%lld", nseg, (long long)max_len, \
              (long long)total);                                                                                            \
  if (nseg == 0) return 0

int32_t ctdet_precise_bn_merge_segments(const float* const* mean_ptrs_dev, const float* const* var_ptrs_dev,
                                        const int64_t* seg_start_dev, const int64_t* rows_dev, int32_t nseg, int64_t max_len,
                                        double* state, int64_t total, void* stream) {
  CTDET_PRECISE_BN_SEGMENTS("precise_bn_merge_segments");
  CTDET_CHECK(mean_ptrs_dev && var_ptrs_dev && seg_start_dev && rows_dev && state, "precise_bn_merge_segments: null pointer");
  CTDET_CHECK(((uintptr_t)state & 7) == 0, "precise_bn_merge_segments: state must be 8-byte aligned");
  return launch_precise_bn_merge(mean_ptrs_dev, var_ptrs_dev, (const long*)seg_start_dev, (const long*)rows_dev, nseg,
                                 (long)max_len, state, (long)total, (hipStream_t)stream);
}

int32_t ctdet_precise_bn_finish_segments(float* const* mean_ptrs_dev, float* const* var_ptrs_dev, const int64_t* seg_start_dev,
                                         int32_t nseg, int64_t max_len, const double* slots, int32_t world, int64_t total,
                                         void* stream) {
  CTDET_PRECISE_BN_SEGMENTS("precise_bn_finish_segments");
  CTDET_CHECK(world >= 1, "precise_bn_finish_segments: world=%d", world);
  CTDET_CHECK(mean_ptrs_dev && var_ptrs_dev && seg_start_dev && slots, "precise_bn_finish_segments: null pointer");
  CTDET_CHECK(((uintptr_t)slots & 7) == 0, "precise_bn_finish_segments: slots must be 8-byte aligned");
  return launch_precise_bn_finish(mean_ptrs_dev, var_ptrs_dev, (const long*)seg_start_dev, nseg, (long)max_len, slots, world,
                                  (long)total, (hipStream_t)stream);
}

int32_t ctdet_resize_bilinear_u8(const ctdet_resize_desc* d, const int32_t* tables_dev, void* stream) {
  CTDET_CHECK(d && d->src && d->dst, "resize_bilinear_u8: null pointer");
  CTDET_CHECK(d->H >= 1 && d->W >= 1 && d->new_h >= 1 && d->new_w >= 1, "resize_bilinear_u8: %dx%d -> %dx%d", d->H, d->W,
              d->new_h, d->new_w);
  CTDET_CHECK(d->kh >= 0 && d->kv >= 0 && (d->kh > 0 || d->W == d->new_w) && (d->kv > 0 || d->H == d->new_h),
              "resize_bilinear_u8: kh=%d kv=%d: a pass may be skipped only when its size does not change", d->kh, d->kv);
  CTDET_CHECK(tables_dev || (d->kh == 0 && d->kv == 0), "resize_bilinear_u8: null table buffer");
  CTDET_CHECK(d->kh == 0 || (d->hb >= 0 && d->hc >= 0), "resize_bilinear_u8: negative table offset");
  CTDET_CHECK(d->kv == 0 || (d->vb >= 0 && d->vc >= 0), "resize_bilinear_u8: negative table offset");
  return launch_resize_u8(*d, tables_dev, (hipStream_t)stream);
}

int32_t ctdet_resize_bilinear_u8_batch(const ctdet_resize_desc* descs_dev, int32_t n, int32_t total_blocks,
                                       const int32_t* tables_dev, void* stream) {
  CTDET_CHECK(descs_dev && tables_dev, "resize_bilinear_u8_batch: null pointer");
  CTDET_CHECK(n >= 0 && total_blocks >= 0, "resize_bilinear_u8_batch: n=%d total_blocks=%d", n, total_blocks);
  if (n == 0 || total_blocks == 0) return 0;
  return launch_resize_u8_batch(descs_dev, n, total_blocks, tables_dev, (hipStream_t)stream);
}

int32_t ctdet_warp_affine_u8_batch(const ctdet_warp_desc* descs_dev, int32_t n, int32_t total_blocks, const int32_t* tables_dev,
                                   void* stream) {
  static_assert(sizeof(ctdet_warp_desc) == 104, "ctdet_warp_desc layout");
  CTDET_CHECK(descs_dev && tables_dev, "warp_affine_u8_batch: null pointer");
  CTDET_CHECK(n >= 0 && total_blocks >= 0, "warp_affine_u8_batch: n=%d total_blocks=%d", n, total_blocks);
  if (n == 0) return 0;      // nothing to warp: nothing is launched
  // the descriptors live on the device and are not read here; what the counts alone can show is checked
  CTDET_CHECK(total_blocks >= n, "warp_affine_u8_batch: total_blocks=%d is not the sum over %d descriptors (at least one block each)",
              total_blocks, n);
  return launch_warp_affine_u8_batch(descs_dev, n, total_blocks, tables_dev, (hipStream_t)stream);
}

int32_t ctdet_byte_sum_u8_batch(const ctdet_jitter_desc* descs_dev, int32_t n, uint64_t* sums_dev, int32_t n_sums, void* stream) {
  CTDET_CHECK(n >= 0 && n < (1 << 24) && n_sums >= 0, "byte_sum_u8_batch: n=%d n_sums=%d", n, n_sums);
  if (n_sums == 0) return 0;
  CTDET_CHECK(sums_dev && ((uintptr_t)sums_dev & 7) == 0, "byte_sum_u8_batch: the sums must be a non-null, 8-byte aligned buffer");
  CTDET_CHECK(descs_dev || n == 0, "byte_sum_u8_batch: null descriptor table");
  return launch_byte_sum_u8_batch(descs_dev, n, sums_dev, n_sums, (hipStream_t)stream);
}

int32_t ctdet_colour_jitter_u8_batch(const ctdet_jitter_desc* descs_dev, int32_t n, int32_t total_blocks, const uint64_t* sums_dev,
                                     int32_t n_sums, void* stream) {
  CTDET_CHECK(n >= 0 && total_blocks >= 0 && n_sums >= 0, "colour_jitter_u8_batch: n=%d total_blocks=%d n_sums=%d", n, total_blocks,
              n_sums);
  if (n == 0 || total_blocks == 0) return 0;      // nothing was drawn: nothing is launched
  CTDET_CHECK(descs_dev, "colour_jitter_u8_batch: null descriptor table");
  CTDET_CHECK(n_sums == 0 || sums_dev, "colour_jitter_u8_batch: n_sums=%d without a sums buffer", n_sums);
  return launch_colour_jitter_u8_batch(descs_dev, n, total_blocks, sums_dev, n_sums, (hipStream_t)stream);
}
int32_t ctdet_soft_nms_merge(const ctdet_softnms_pass* passes, int32_t npass, int32_t B, int32_t num_classes, float sigma,
                             float min_score, int32_t max_det, void* workspace, float* out_boxes, float* out_scores,
                             int32_t* out_classes, int32_t* out_counts, void* stream) {
  CTDET_CHECK(npass >= 1 && npass <= CTDET_SOFTNMS_MAX_PASSES, "soft_nms_merge: %d passes (1..%d)", npass,
              CTDET_SOFTNMS_MAX_PASSES);
  CTDET_CHECK(passes, "soft_nms_merge: null pass table");
  CTDET_CHECK(B >= 0 && num_classes >= 1 && num_classes <= (1 << 20) && (int64_t)B * num_classes < (1LL << 26),
              "soft_nms_merge: B=%d images x %d classes out of range (classes <= 2^20, B*classes < 2^26)", B, num_classes);
  CTDET_CHECK(max_det >= 1, "soft_nms_merge: max_det=%d", max_det);
  CTDET_CHECK(sigma > 0.f, "soft_nms_merge: sigma=%g must be positive", (double)sigma);   // a NaN fails too
  int64_t total = 0;
  for (int i = 0; i < npass; ++i) {
    CTDET_CHECK(passes[i].K >= 0, "soft_nms_merge: pass %d has width %d", i, passes[i].K);
    CTDET_CHECK(passes[i].counts && (passes[i].K == 0 || (passes[i].boxes && passes[i].scores && passes[i].classes)),
                "soft_nms_merge: null pointer in pass %d", i);
    total += passes[i].K;
  }
  CTDET_CHECK(total <= CTDET_SOFTNMS_MAX_CANDIDATES, "soft_nms_merge: %lld candidates per image (at most %d)", (long long)total,
              CTDET_SOFTNMS_MAX_CANDIDATES);
  CTDET_CHECK(B == 0 || (out_boxes && out_scores && out_classes && out_counts), "soft_nms_merge: null output pointer");
  CTDET_CHECK(B == 0 || total == 0 || (workspace && ((uintptr_t)workspace & 3) == 0),
              "soft_nms_merge: the workspace must be a non-null, 4-byte aligned buffer");
  return launch_soft_nms(passes, npass, B, num_classes, sigma, min_score, max_det, workspace, out_boxes, out_scores, out_classes,
                         out_counts, (hipStream_t)stream);
}
#undef CTDET_ADAM_BETAS
#undef CTDET_DCN_MASK_MODE

}  // extern "C"
