// The way back from an affine-warped test input (INPUT.AFFINE.TEST_MODE): dec_postprocess_kernel's threshold /
// clip / drop-empty / ordered compaction (decode.hip), with the box map  x' = x * sx + tx,  y' = y * sy + ty  in the place of its
// scale.  data/warp.py states the arithmetic (unwarp_boxes_reference): the product is rounded to f32, then the sum is -- two
// roundings, never a fused multiply-add -- so that the numpy oracle is reproduced bit for bit.  The file is compiled with
// -ffp-contract=off (Makefile) and the two operations are spelt out as __fmul_rn / __fadd_rn besides.
//
// One wave per image; img_params[b * 6 ..] = {sx, sy, tx, ty, orig_w, orig_h} (data.warp.unwarp_params).  Every index is
// b * K + k with k < K, or b * 6 + j with j < 6: nothing else is read or written.
#include "common.h"
#include "../../include/ctdet_hip.h"

#define UNWARP_PARAMS 6      // floats of one image's parameter row

__global__ void __launch_bounds__(64) dec_postprocess_affine_kernel(const float* __restrict__ boxes,
                                                                   const float* __restrict__ scores,
                                                                   const int* __restrict__ classes, int K, int max_det,
                                                                   float thresh, const float* __restrict__ img_params,
                                                                   float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                                   int* __restrict__ out_classes, int* __restrict__ counts) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* p = img_params + (long)b * UNWARP_PARAMS;
  const float sx = p[0], sy = p[1], tx = p[2], ty = p[3], ow = p[4], oh = p[5];
  // multiply, round, add, round
  auto map = [](float v, float s, float t) { return __fadd_rn(__fmul_rn(v, s), t); };
  // as in dec_postprocess_kernel: Boxes.clip's clamp hands a NaN coordinate on, and nonempty() then drops the box (NaN > 0 is
  // false); fminf / fmaxf would return their other operand and turn the coordinate into 0
  auto clip = [](float v, float hi) { return v != v ? v : fminf(fmaxf(v, 0.f), hi); };
  int base = 0;
  for (int k0 = 0; k0 < K; k0 += 64) {      // the trip count is the same for all 64 lanes: every lane reaches the ballot
    const int k = k0 + lane;
    bool keep = false;
    float x1 = 0, y1 = 0, x2 = 0, y2 = 0, sc = 0;
    int cl = 0;
    if (k < K && k < max_det) {
      const long o = (long)b * K + k;
      sc = scores[o];
      cl = classes[o];
      x1 = clip(map(boxes[o * 4 + 0], sx, tx), ow);
      y1 = clip(map(boxes[o * 4 + 1], sy, ty), oh);
      x2 = clip(map(boxes[o * 4 + 2], sx, tx), ow);
      y2 = clip(map(boxes[o * 4 + 3], sy, ty), oh);
      keep = sc > thresh && (x2 - x1) > 0.f && (y2 - y1) > 0.f;
    }
    const unsigned long long m = __ballot(keep);
    if (keep) {
      const int pos = base + __popcll(m & ((1ull << lane) - 1ull));      // pos <= k < K
      const long o = (long)b * K + pos;
      out_boxes[o * 4 + 0] = x1; out_boxes[o * 4 + 1] = y1; out_boxes[o * 4 + 2] = x2; out_boxes[o * 4 + 3] = y2;
      out_scores[o] = sc;
      out_classes[o] = cl;
    }
    base += __popcll(m);
  }
  if (lane == 0) counts[b] = base;
}

int launch_postprocess_affine(const float* boxes, const float* scores, const int* classes, int B, int K, int max_det,
                              float thresh, const float* img_params6, float* out_boxes, float* out_scores, int* out_classes,
                              int* counts, hipStream_t s) {
  if (B == 0) return 0;
  CTDET_KERNEL("dec_postprocess_affine_kernel");
  hipLaunchKernelGGL(dec_postprocess_affine_kernel, dim3(B), dim3(64), 0, s, boxes, scores, classes, K, max_det, thresh,
                     img_params6, out_boxes, out_scores, out_classes, counts);
  CTDET_LAUNCH_CHECK();
  return 0;
}
