// Shared declarations for the CenterNet hot-path HIP kernels (gfx950 / CDNA4 only).
// Data layout everywhere on the device: activations are NHWC ("pixel rows": one
// pixel = `stride` contiguous channel elements), weights are KRSC packed to
// [Cout_pad][Kpad] (f16 MFMA path) or [Kpad][Cout_pad] (f32 exact path).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef _Float16 f16;
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef f16 f16x8 __attribute__((ext_vector_type(8)));
typedef f16 f16x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// the split of the f16x3 mode (conv_common.h), spelled once: hi = f16(x), lo = f16(x - hi) of 4 f32
__device__ __forceinline__ void split_parts(const f32x4 x, f16x4& hi, f16x4& lo) {
  hi = __builtin_convertvector(x, f16x4);
  f32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = x[j] - (float)hi[j];
  lo = __builtin_convertvector(r, f16x4);
}
// 4 f32 -> the 16 bytes {hi[4], lo[4]}: split weights and split windows in memory
__device__ __forceinline__ f16x8 split_hi_lo(const f32x4 x) {
  f16x4 hi, lo;
  split_parts(x, hi, lo);
  return __builtin_shufflevector(hi, lo, 0, 1, 2, 3, 4, 5, 6, 7);
}

// error plumbing (thread-local message, returned through ctdet_last_error()).
void ctdet_set_error(const char* fmt, ...);
#define CTDET_CHECK(cond, ...)            \
  do {                                    \
    if (!(cond)) {                        \
      ctdet_set_error(__VA_ARGS__);       \
      return -22; /* -EINVAL */           \
    }                                     \
  } while (0)
#define CTDET_LAUNCH_CHECK()                                          \
  do {                                                                \
    hipError_t e_ = hipGetLastError();                                \
    if (e_ != hipSuccess) {                                           \
      ctdet_set_error("kernel launch failed: %s (%s:%d)",            \
                      hipGetErrorString(e_), __FILE__, __LINE__);     \
      return -5; /* -EIO */                                           \
    }                                                                 \
  } while (0)

// kernel labels (thread-local, ctdet_set_label_mode() / ctdet_last_kernel_label()): the launchers of the profiled conv
// kernels say which instantiation they launch, on the line that launches it.  Mode 0: nothing is recorded (one thread-local
// load and a branch per launch); 1: the label is formatted, then the kernel is launched; 2 (dry run): the label is formatted
// and the launcher returns 0 instead of launching -- every check and the whole selection ran, nothing touched the device.
extern thread_local int g_label_mode;
bool ctdet_set_label(const char* fmt, ...);   // formats the label; true in the dry-run mode
#define CTDET_KERNEL(...)                                             \
  do {                                                                \
    if (g_label_mode && ctdet_set_label(__VA_ARGS__)) return 0;       \
  } while (0)
// how a label names the output type of a kernel instantiation
template <typename TOut> inline const char* out_name() { return sizeof(TOut) == 2 ? "f16" : "f32"; }

enum { CTDET_F16 = 0, CTDET_F32 = 1, CTDET_U8 = 2, CTDET_F16X3 = 3 };
enum { CTDET_ACT_NONE = 0, CTDET_ACT_RELU = 1, CTDET_ACT_SIGMOID_CLAMP = 2 };
// DCN mask modes (ConvArgs::mask_is_prob and the DCN entry points' argument; CTDET_DCN_MASK_* in ctdet_hip.h)
enum { DCN_MASK_LOGIT = 0, DCN_MASK_PROB = 1, DCN_MASK_NONE = 2 };
// gradient clipping of the flat SGD step (CTDET_CLIP_* / CTDET_NORM_* in ctdet_hip.h)
enum { SGD_CLIP_NONE = 0, SGD_CLIP_VALUE = 1, SGD_CLIP_NORM = 2 };
enum { GRAD_NORM_L1 = 1, GRAD_NORM_L2 = 2, GRAD_NORM_INF = 3 };
// channels of an offset/mask row a DCN kernel reads: 18 offsets (+ 9 mask channels unless the mask is absent)
__host__ __device__ inline int dcn_om_channels(int mask_mode) { return mask_mode == DCN_MASK_NONE ? 18 : 27; }

// Kernel-side argument block for every conv-shaped contraction on the path
// (plain conv, DCNv2 main contraction, offset/mask conv, head convs).
struct ConvArgs {
  const void* x;        // [B,H,W,in_stride] input pixels (channel slice starts at x)
  const void* w;        // packed weights
  const float* scale;   // per-cout multiplier (folded BN gamma/sqrt(var+eps)) or null
  const float* bias;    // per-cout bias (folded BN beta - mean*scale, or conv bias) or null
  const void* res;      // residual added before activation, same dtype as y, or null
  void* y;              // [B,Ho,Wo,out_stride]
  // Root (dla.py:86-94) = 1x1 conv over torch.cat(children): instead of materialising the concat the
  // kernel reads K segments from up to 4 source tensors (nsrc > 1; 1x1, stride 1, pad 0 only).
  const void* xs[4];
  int xs_stride[4];
  int xs_cend[4];       // cumulative channel ends of the sources
  int nsrc;
  const float* om;      // DCNv2 only: [M, om_stride] f32; ch 0..17 offsets (2k=dh,2k+1=dw), 18..26 mask logits
  int om_stride;
  int mask_is_prob;     // DCN mask mode: 0 = mask channels are logits (sigmoid here), 1 = already probabilities,
                        // 2 = no mask (DCNv1: om holds the 18 offset channels only, the kernels' NM instantiations)
  int B, H, W, Cin, in_stride;
  int Cout, Ho, Wo, out_stride, res_stride;
  int R, S, stride, pad, dil;
  int K, Kpad, Cout_pad;
  int M;                // B*Ho*Wo
  int act;
  float clamp_lo, clamp_hi;
  int korder;           // 0 tap-major, 1 chunk-major (see ctdet_conv_desc)
  int in_dil;           // input dilation (zero-stuffed input): >1 only for the input-gradient of strided convs
  // DCNv2 with its offset / mask conv computed in the same kernel (ctdet_dcnv2_offset_fwd): that conv's packed f16 weights
  // (32 rows, chunk-major), its bias (32 f32), and optionally where to keep its f32 output for a backward pass
  const void* w_off; const float* b_off; float* om_out; int om_out_stride;
  // DCNv2, f16x3 window kernel, training: the sampled columns (mask * bilinear(x), f32 [M][9*Cin], k = tap*Cin + c -- what
  // modulated_deformable_im2col produces, kernel.cu:786-868) written as a by-product of the forward pass, or null
  float* cols_out;
  // DCNv2 with the fused offset conv, f16x3 (ctdet_dcnv2_offset_finite_fwd): int32 flag that the epilogue sets to 0 when a value
  // it stores is inf or NaN (the caller set it to 1), or null
  int* finite;
};

// argument block of the fused CenterNet head kernels (conv_igemm.hip): per head 3x3 conv Cin->256 + bias + ReLU, then
// 1x1 conv 256->cout + bias (+ sigmoid/clamp), the 256-channel hidden map never stored.  f16: head_fused_kernel;
// f16x3 (launch_head_fused_x3): the second layout of each field
struct HeadArgs {
  const void* x;          // f16 [B,H,W,in_stride]                  | f32
  const void* w1;         // f16 packed chunk-major [nheads*256][9*Cin] | korder 3 pair image [>= nheads*256][Cin/32*288] (f32 units)
  const float* b1;        // [nheads*256]
  const void* w2[4];      // f16 [round_up(cout,16)][256]           | f16 [round_up(cout,16)][2][256]: {w_hi, w_lo} of the scaled row
  const float* b2[4];     // f32 [round_up(cout,16)]                | f32 [2][round_up(cout,16)]: bias, inverse row scale
  float* y[4];            // f32 [B,H,W,y_stride]
  int y_stride[4], cout[4], act[4];
  int nheads, B, H, W, Cin, in_stride;
  float clamp_lo, clamp_hi;
  const float* s1;        // -                                      | [nheads*256] inverse row scale of w1
};

// argument block of the fused DLA base kernel (dla_base.hip): normalisation + 7x7 stem + level0 + level1
struct BaseArgs {
  const void* img;        // [B,3,H,W] uint8 or f32 planar image batch
  int img_dtype;          // CTDET_U8 / CTDET_F32
  long img_batch_stride;  // elements between images
  int B, H, W;            // image size
  int Hp, Wp;             // network input size (image zero-padded bottom/right after normalisation)
  float mean[3], stdv[3];
  const void* w0;         // f16 [16][7*8*4]   stem, k = (r*8 + s)*4 + c (s = 7 and c = 3 zero)
  const void* w1;         // f16 [16][160]     level0, k = (r*3 + s)*16 + c
  const void* w2;         // f16 [32][160]     level1 (stride 2)
  const float *s0, *b0, *s1, *b1, *s2, *b2;   // folded BatchNorm scale / bias per layer
  void* y;                // f16 [B,Hp/2,Wp/2,out_stride]
  int out_stride;
  void* pool;             // optional f16 [B,Hp/4,Wp/4,pool_stride]: 2x2 max-pool of y
  int pool_stride;
  // flip test: < 0 = none (the plain kernels).  Otherwise output images [mirror_from, B) are computed from the horizontally
  // mirrored network input of SOURCE images [0, B - mirror_from): input column x reads image column Wp-1-x (zero where that
  // is >= W, so the zero padding sits on the left); output images below mirror_from read their own source image, plain
  int mirror_from;
};

// argument block of the batched decode (decode.hip)
struct DecArgs {
  const float* heat; const float* wh; const float* reg;
  int heat_stride, wh_stride, reg_stride;   // pixel strides (elements)
  int B, H, W, C, K;
  float down_ratio;
  uint32_t floor_bits;                      // bits of the promised lower bound of the heat values (0 = none)
  uint32_t* ws;
  float* boxes; float* scores; int* classes; int* inds;   // wh == nullptr: no boxes (launch_head_sparse_x3 writes them), inds required
};

// argument block of the conv weight-gradient launchers (train_bwd.hip; also the kernels' own argument):
// dW[n][k] += sum_m dY[m][n] * im2col(x)[m][k]
struct WgradArgs {
  const void* x; const void* dy; float* dw;   // x, dy: f16 (f16 mode) or f32 (f16x3 mode: split into hi + lo f16 halves on the way to LDS)
  int B, H, W, Cin, in_stride, Cout, Ho, Wo, dy_stride, R, S, stride, pad, dil, K, M, msplit;
  float scale;   // multiplier applied to every partial sum before it is added to dw
  int lw, lh;    // log2(Wo), log2(Ho) when both are powers of two, else -1
  // output layout: perm_rs == 0: dw[n][k], k = tap*Cin + c (tap-major).  perm_rs > 0: the parameter's own OIHW layout,
  // dw[(n*cin_real + c)*perm_rs + tap] with k = tap*perm_cin + c, channels c >= cin_real (input padding)
  // and rows n >= cout_real (output-channel padding of dy) dropped -- the kernel then accumulates straight into the
  // optimizer's gradient buffer
  int perm_rs, perm_cin, cin_real, cout_real;
};

// argument block of the six BatchNorm launchers (train_bwd.hip).  Tensors are [M][*_stride] pixel rows of C channels, all of
// element type `dtype`; per-channel vectors are f32 [C].  A field a launcher does not use is zero.
struct BnArgs {
  int dtype;                 // CTDET_F16 / CTDET_F32
  int M, C, relu;
  const void* y;    int y_stride;      // the conv output BatchNorm normalises
  const void* res;  int res_stride;    // forward: residual added before the ReLU, or null
  void* z_out;                         // forward: the result, pixel stride z_stride
  const void* z;    int z_stride;      // backward: the forward's result (read where relu is set)
  const void* dz;   int dz_stride;     // backward: gradient of z
  void* dy;         int dy_stride;     // backward: gradient of y
  void* dres;       int dres_stride;   // backward: gradient of the residual, or null
  const float *gamma, *beta;
  float eps, momentum;
  float *running_mean, *running_var;   // updated in place, or null
  float *save_mean, *save_invstd, *save_scale, *save_shift;   // forward: batch statistics and the folded affine, written
  const float *mean, *invstd, *scale;  // backward: what the forward saved
  float *dgamma, *dbeta;
  float grad_mult;                     // multiplier of dgamma / dbeta
  void* workspace;                     // chan_reduce_workspace_bytes(C)
  // SyncBatchNorm: rank-slot buffers, f64 [world][K][C]
  int rank, world;
  double* slots;                       // bn_local_stats / bn_local_grad_sums: this rank's slot written, the others zeroed
  const double *stats, *sums;          // the all-reduced buffers of the two
};

// argument block of the DCNv2 backward launchers (train_bwd.hip): dcn_cols, dcn_col2im_coord, dcn_col2im_fused
struct DcnBwdArgs {
  int dtype;                 // element type of x, col and dcol: CTDET_F16, CTDET_F32 or CTDET_F16X3 (f32 tensors; col2im_coord
                             // then takes the LDS-window scatter where the shape allows).  col2im_fused: f32 only, unused
  const void* x;    int x_stride;      // [B,H,W,x_stride] input of the layer
  const float* om;  int om_stride;     // [M, om_stride] offsets (+ mask channels, see mask_mode)
  int B, H, W, Cin, mask_mode;         // DCN_MASK_*
  void* col;                           // dcn_cols: [M][9*Cin] sampled columns (written)
  const void* dcol; int dcol_chunked;  // col2im_coord: d(columns), rows [tap][Cin] or chunked [Cin/32][tap][32]
  float* dx;                           // [M][Cin] f32, accumulated into
  void* dom; int dom_stride, dom_dtype;   // d(offset / mask) rows: CTDET_F32, or CTDET_F16 with f16 tensors
  // col2im_fused: the d(columns) GEMM runs in the scatter kernel.  dy f32 [M][dy_stride] with K channels (multiple of 32;
  // channels beyond the layer's couts zero), wpk / wscale from ctdet_pack_weights_x3 (layout 5, transposed 3)
  const float* dy;  int dy_stride, K;
  const void* wpk;  const float* wscale;
};

__device__ __forceinline__ float ctdet_sigmoid(float v) { return 1.0f / (1.0f + __expf(-v)); }
__device__ __forceinline__ float ctdet_sigmoid_exact(float v) { return 1.0f / (1.0f + expf(-v)); }

// Kernel-selection switches (ctdet_set_tuning_flags in the C ABI; a process-wide word read with one relaxed load per launch
// -- no getenv on the launch path).  0 = every specialised kernel enabled.
enum {
  CTDET_TUNE_NO_HALO = 1,            // 3x3 halo-resident conv -> uniform-K kernel
  CTDET_TUNE_NO_WIN = 2,             // LDS-window kernels of the narrow DLA base layers -> small-channel kernel
  CTDET_TUNE_DCN_MIXED = 4,          // DCNv2 window kernel: per-lane instead of per-wave out-of-window gathers
  CTDET_TUNE_NO_WGRAD_WINDOW = 8,    // weight-gradient window kernel -> generic kernel
  CTDET_TUNE_NO_COL2IM_WINDOW = 16,  // DCNv2 backward LDS-window scatter -> global-atomic kernel
  CTDET_TUNE_NO_F32_DCN_WINDOW = 32, // f32 DCNv2 LDS-window kernel -> global-gather kernel
  CTDET_TUNE_NO_SMALL_GRID_TILES = 128, // convs whose 128-cout grid underfills the chip keep 128-cout tiles (default: 64-cout tiles)
  CTDET_TUNE_NO_HALO_TAP2 = 512,     // f16 3x3 halo conv with Cin % 64 == 0: the per-tap kernel instead of conv3x3_halo_tap2_kernel
  CTDET_TUNE_DCN_SPLIT_4W = 256,     // f16x3 DCNv2 window kernel: 64-cout tiles (four 32-pixel waves) also for the 128- and 256-cout layers
  // 1024, 2048: two variants that lost their A/B and are gone; the numbers are not reused
  CTDET_TUNE_TARGETS_MEMSET = 4096,   // gaussian targets: clear the heat map with hipMemsetAsync (round 3's form: a memset NODE in a captured step;
                                      // kept to reproduce profiles/r04_graph_memset_node.txt and to test the node check)
  CTDET_TUNE_DCN_WINDOW_V1 = 64,     // 64-cout f16 DCNv2: the per-tap-barrier window kernel instead of the row-step one
};
unsigned ctdet_tuning_flags();
// number of CUs of the CURRENT device (cached per device ordinal, not per process)
int ctdet_device_cu_count();

// Everything one .hip file defines and another calls (api.hip, mostly), declared here and nowhere else.  Launchers return 0 or
// a negative errno; tensors whose element type varies are `const void*` with an `int dtype` (CTDET_F16 / CTDET_F32 / ...), and
// a dtype a launcher does not serve is rejected with -22, never run as another one.

// conv_igemm.hip
int launch_conv_f16(const ConvArgs& a, int out_dtype, bool deform, hipStream_t s);
bool halo_pair_x_ok(const ConvArgs& a, int korder);          // activation side of what the f16x3 halo pair kernels need
int launch_halo_pair(const ConvArgs& a, hipStream_t s);      // korder 2 pair image
int launch_halo_pair2(const ConvArgs& a, hipStream_t s);     // korder 3 (cross-chunk) pair image
int launch_halo_split(const ConvArgs& a, hipStream_t s);     // tap-major split weights; 1 if the shape does not qualify
bool head_fused_x_ok(const HeadArgs& a, bool x3);            // may these activations take the fused head kernel?
int launch_head_fused(const HeadArgs& a, hipStream_t s);
int launch_head_fused_x3(const HeadArgs& a, hipStream_t s);
// the wh / reg heads (a two-head f16x3 pack; a.y unused) at the pixels inds[B,K] of a.x, and the decode's boxes from them;
// flip: a.x holds 2 * a.B images, wh is the mean with the mirrored pixel of image b + a.B
int launch_head_sparse_x3(const HeadArgs& a, const int* inds, float* whreg, float* boxes, int K, float down_ratio, bool flip,
                          hipStream_t s);
bool dcn_offset_fused_ok(const ConvArgs& a);                 // geometry the f16 row-step kernel (fused offset conv) serves
// f16 `columns` of the DCNv2 backward from the sampling kernel's LDS window (launch_dcn_cols decides when)
int launch_dcn_cols_window(const DcnBwdArgs& a, hipStream_t s);

// conv_f32.hip
int launch_conv_f32(const ConvArgs& a, bool deform, bool split, hipStream_t s);   // split: the f16x3 mode
int conv_pair_korder(const ConvArgs& a);                     // korder of the pair image an f16x3 3x3 conv would take, 0: none
bool dcn_split_window_ok(const ConvArgs& a);                 // LDS-window kernel that can also write ConvArgs::cols_out?
bool dcn_offset_fused_x3_ok(const ConvArgs& a);              // may the f16x3 DCNv2 compute its own offsets and mask?
int launch_dcn_offset_x3(const ConvArgs& a, hipStream_t s);
int launch_split_weights(const float* src, void* dst, long n, hipStream_t s);

// dla_base.hip
int launch_dla_base(const BaseArgs& a, hipStream_t s);
int launch_dla_base_x3(const BaseArgs& a, hipStream_t s);   // f16x3: w* = ctdet_pack_weights_x3 layout 0 images, y / pool f32

// pointwise.hip
// mirror_from < 0: the plain kernel; otherwise output images [mirror_from, B) are mirrored copies of source images [0, B - mirror_from)
int launch_preprocess(const void* img, int img_dtype, void* out, int out_dtype, int B, int H, int W, int Hp, int Wp,
                      long img_batch_stride, const float* mean, const float* stdv, int out_stride, int border,
                      int mirror_from, hipStream_t s);
int launch_maxpool2x2(const void* x, void* y, int dtype, int B, int H, int W, int C, int in_stride, int out_stride,
                      hipStream_t s);
int launch_maxpool3x3s2(const void* x, void* y, int dtype, int B, int H, int W, int C, int in_stride, int out_stride,
                        int ceil_nopad, hipStream_t s);
int launch_finite_flag(const float* x, long M, int C, int stride, int* flag, hipStream_t s);
int launch_global_avgpool(const void* x, int dtype, int B, int HW, int C, int stride, float* out, hipStream_t s);
int launch_ese_scale(const void* x, int x_stride, const float* sc, const void* idn, int idn_stride, void* y, int y_stride,
                     int dtype, int B, int HW, int C, hipStream_t s);
int launch_pack_weights(const float* w, void* out, int O, int I, int R, int S, int chans_pad, int rows_pad, int Kpad,
                        int korder, int transposed, hipStream_t s);
int launch_pack_weights_batch(const void* table_dev, int n, int total_blocks, hipStream_t s);   // table: ctdet_pack_desc[n]
int launch_pack_weights_x3(const float* w, void* out, float* scale_out, int O, int I, int R, int S, int chans_pad, int rows_pad,
                           int Kpad, int layout, int transposed, int scale_n, hipStream_t s);
int launch_pack_weights_x3_batch(const void* table_dev, int n, int total_blocks, hipStream_t s);   // table: ctdet_pack3_desc[n]
int launch_dwconvT_add(const void* x, const float* w, const void* skip, void* y, int dtype, int B, int H, int W, int C,
                       int f, int in_stride, int skip_stride, int out_stride, hipStream_t s);

// resize.hip
struct ctdet_resize_desc;                                    // include/ctdet_hip.h
int resize_tiles(int new_h, int new_w);                      // blocks of one image
int launch_resize_u8(const ctdet_resize_desc& d, const int* tab, hipStream_t s);
int launch_resize_u8_batch(const ctdet_resize_desc* descs_dev, int n, int total_blocks, const int* tab, hipStream_t s);

// warp.hip
struct ctdet_warp_desc;                                      // include/ctdet_hip.h
int warp_tiles(int out_h, int out_w);                        // blocks of one image
int launch_warp_affine_u8_batch(const ctdet_warp_desc* descs_dev, int n, int total_blocks, const int* tab, hipStream_t s);

// jitter.hip
struct ctdet_jitter_desc;                                   // include/ctdet_hip.h
int jitter_tiles(int h, int w);                              // blocks of one image
int launch_byte_sum_u8_batch(const ctdet_jitter_desc* descs_dev, int n, uint64_t* sums, int n_sums, hipStream_t s);
int launch_colour_jitter_u8_batch(const ctdet_jitter_desc* descs_dev, int n, int total_blocks, const uint64_t* sums, int n_sums,
                                  hipStream_t s);

// softnms.hip
struct ctdet_softnms_pass;                                   // include/ctdet_hip.h
int launch_soft_nms(const ctdet_softnms_pass* passes, int npass, int B, int C, float sigma, float min_score, int max_det,
                    void* workspace, float* out_boxes, float* out_scores, int* out_classes, int* out_counts, hipStream_t s);

// dwconv.hip
// shape / dtype checks shared by the entry points (api.hip validates pointers first)
int dwconv3x3_check(int dtype, int B, int H, int W, int C, int stride, const int* strides, int nstrides);
size_t dwconv3x3_wgrad_workspace_bytes(int B, int H, int W, int C, int dtype);
int launch_dwconv3x3(const void* x, int x_stride, const float* w, void* y, int y_stride, int B, int H, int W, int C, int stride,
                     int rot180, int dtype, hipStream_t s);
int launch_dwconv3x3_wgrad(const void* x, int x_stride, const void* dy, int dy_stride, float* ws, float* dw, float scale,
                           int accumulate, int B, int H, int W, int C, int dtype, hipStream_t s);

// decode.hip
size_t decode_workspace_bytes(int B, int H, int W, int C, int K);
// words of one image's workspace and the index of its below-the-floor word; returns the index of the overflow word
int decode_status_words(int H, int W, int C, int K, long* ws_words, int* below_word);
int launch_decode(const DecArgs& a, bool flip, hipStream_t s);
int launch_postprocess(const float* boxes, const float* scores, const int* classes, int B, int K, int max_det,
                       float thresh, const float* img_params, float* out_boxes, float* out_scores, int* out_classes,
                       int* counts, hipStream_t s);

// unwarp.hip
int launch_postprocess_affine(const float* boxes, const float* scores, const int* classes, int B, int K, int max_det,
                              float thresh, const float* img_params6, float* out_boxes, float* out_scores, int* out_classes,
                              int* counts, hipStream_t s);

// train_ops.hip
int launch_gaussian_radius(const int* hw, int n, double* out_r, int* out_i, hipStream_t s);
int launch_gaussian_targets(const float* boxes, const int64_t* classes, const int* counts, int B, int Nmax, int H,
                            int W, int C, float* hm, float* wh, float* reg, int64_t* ind, uint8_t* reg_mask,
                            hipStream_t s);
size_t focal_workspace_bytes(long numel);
int launch_focal_loss(const float* logits, const float* gt, const float* alpha, int B, int H, int W, int C,
                      float grad_scale, void* workspace, float* loss, float* stats, float* grad, hipStream_t s);
int launch_reg_l1(const float* pred, int pred_stride, const uint8_t* mask, const int64_t* ind, const float* target,
                  int B, int N, int HW, float grad_scale, float* loss, float* grad, int grad_stride, hipStream_t s);
int launch_sgd(float* p, const float* g, float* m, long n, const float* lr_dev, float mom, float wd, int first,
               hipStream_t s);
int launch_sgd_runs(float* p, const float* g, float* m, long n, const long* run_end, const int* run_lr_index,
                    const float* run_wd, const float* lr_table, int nruns, float mom, int first, hipStream_t s);
int launch_sgd_runs_clip(float* p, const float* g, float* m, long n, const long* run_end, const int* run_lr_index,
                         const float* run_wd, const float* lr_table, int nruns, float mom, int first, int nesterov, int clip_type,
                         float clip_value, const float* coefs, hipStream_t s);
int launch_grad_chunk_norms(const float* g, long n, const long* chunk_start, const int* chunk_len, int nchunks, int norm_type,
                            float* partials, hipStream_t s);
int launch_grad_clip_coefs(const float* partials, const int* param_chunk_end, int nparams, int nchunks, int norm_type,
                           float clip_value, float* norms, float* coefs, hipStream_t s);
int launch_adam_advance(long long* step, float* bias, double beta1, double beta2, hipStream_t s);
int launch_adam_runs(float* p, const float* g, float* m, float* v, float* vmax, long n, const long* run_end,
                     const int* run_lr_index, const float* run_wd, const float* lr_table, int nruns, const float* bias,
                     double beta1, double beta2, double eps, int decoupled, int amsgrad, int clip_type, float clip_value,
                     const float* coefs, hipStream_t s);

// ema.hip
int launch_ema_advance(long long* updates, float* weight, double decay, int warmup, hipStream_t s);
int launch_ema_lerp_segments(const float* const* live_ptrs, float* ema, const long* seg_start, int nseg, long max_len,
                             const float* weight, hipStream_t s);
int launch_ema_swap_segments(float* const* live_ptrs, float* ema, const long* seg_start, int nseg, long max_len, hipStream_t s);

// precise_bn.hip
int launch_precise_bn_merge(const float* const* mean_ptrs, const float* const* var_ptrs, const long* seg_start, const long* rows,
                            int nseg, long max_len, double* state, long total, hipStream_t s);
int launch_precise_bn_finish(float* const* mean_ptrs, float* const* var_ptrs, const long* seg_start, int nseg, long max_len,
                             const double* slots, int world, long total, hipStream_t s);

// train_bwd.hip
size_t chan_reduce_workspace_bytes(int C);                   // BnArgs::workspace
int launch_bn_train_fwd(const BnArgs& a, hipStream_t s);
int launch_bn_train_bwd(const BnArgs& a, hipStream_t s);
int launch_bn_local_stats(const BnArgs& a, hipStream_t s);       // SyncBN forward, before the all-reduce of a.slots
int launch_bn_sync_fwd(const BnArgs& a, hipStream_t s);          // ... and after it (a.stats)
int launch_bn_local_grad_sums(const BnArgs& a, hipStream_t s);   // SyncBN backward, before the all-reduce of a.slots
int launch_bn_sync_bwd(const BnArgs& a, hipStream_t s);          // ... and after it (a.stats, a.sums)
int launch_conv_wgrad(const WgradArgs& a, hipStream_t s);        // f16 tensors
int launch_conv_wgrad_x3(const WgradArgs& a, hipStream_t s);     // f32 tensors, split f16 products
int launch_conv_wgrad_f32(const WgradArgs& a, hipStream_t s);    // f32 tensors, f32 FMAs
int launch_grad_scatter_oihw(const void* const* src, void* const* dst, const int* cout, const int* cin_real, const int* cin_k,
                             const int* taps, int n, hipStream_t s);
int launch_depth_to_space2(const void* src, int src_stride, void* dst, int dst_stride, int B, int H, int W, int C, int Hs, int Ws,
                           int dtype, hipStream_t s);
int launch_maxpool2x2_bwd(const void* x, int x_stride, const void* dz, int dz_stride, void* dx, int dx_stride, int dtype, int B,
                          int H, int W, int C, hipStream_t s);
int launch_maxpool3x3s2_bwd(const void* x, int xs, const void* dz, int dzs, void* dx, int dxs, int dtype, int B, int H, int W, int C,
                            int pad, int Ho, int Wo, hipStream_t s);
int launch_ese_dot(const void* dy, int dys, const void* x, int xs, int dtype, int B, int HW, int C, float* out, hipStream_t s);
int launch_ese_bwd(const void* dy, int dys, const float* g, const float* gp, void* dx, int dxs, int dtype, int B, int HW, int C,
                   hipStream_t s);
int launch_dwconvT_bwd(const void* x, int x_stride, const void* dz, int dz_stride, const float* w, void* dx, int dx_stride,
                       float* dw, int dtype, int B, int H, int W, int C, int f, hipStream_t s);
int launch_dcn_cols(const DcnBwdArgs& a, hipStream_t s);
int launch_dcn_col2im_coord(const DcnBwdArgs& a, hipStream_t s);
// 0 if launched, 1 if the shape does not qualify (the caller then produces d(columns) and calls ctdet_dcn_col2im_coord)
int launch_dcn_col2im_fused(const DcnBwdArgs& a, hipStream_t s);
