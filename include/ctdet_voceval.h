/* C ABI of libctdet_voceval.so: Pascal VOC box-AP scoring (gfx950).  Errors and kernel labels go through libctdet_hip.so
 * (ctdet_last_error, ctdet_set_label_mode / ctdet_last_kernel_label), which this library links against. */
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Pascal VOC box-AP scoring ------------------------------------------------------------------------------------
 * The scorer of the reference's PascalVOCDetectionEvaluator (detectron2/evaluation/pascal_voc_evaluation.py: voc_eval, voc_ap)
 * over the detections of a whole dataset in device memory; DESIGN.md 7.16 holds the rule.  All arithmetic is f64, every
 * operation rounded once.  These calls use a device radix sort and are not meant to be captured into a graph.
 *
 * ctdet_voceval_match: detections concatenated over the dataset -- boxes f32 [N,4] XYXY as the model gives them (0-based; the
 *   call adds 1 to x1 / y1 in f32 and rounds every coordinate to one decimal, every score to three, half-even, in f64: the
 *   reference's text round trip), scores f32 [N], classes i32 [N] in [0,K), image i32 [N] in [0,I); ground truth sorted by
 *   (image, class) with CSR offsets gt_off i32 [I*K+1] into gt_boxes f64 [NG,4] (the XML's 1-based xmin ymin xmax ymax) and
 *   gt_difficult u8 [NG]; thrs f64 [T], T <= 32; I*K < 2^26 (one wave per cell).
 *   Outputs: order i32 [N] (input index of every position of the total order: class ascending, quantised score descending,
 *   input index ascending), cls_off i32 [K+1] (the classes' segments of it), flags u8 [N,T] at the INPUT index (0 neither: the
 *   best match is difficult, 1 true positive, 2 false positive), npos i32 [K] (non-difficult ground truths), status i32 [1]:
 *   OR of CTDET_VOC_BAD_* over the detections that take no part (sorted behind cls_off[K]; their flags are not written).
 * ctdet_voceval_ap: from those, with points f64 [11] = the recall points of the 11-point form (np.arange(0.0, 1.1, 0.1)) in
 *   device memory: ap07 (11-point) and ap12 (area) f64 [K,T], as fractions; rec / prec f64 [T,N] by position of the total
 *   order, or NULL.  A class without non-difficult ground truth: ap07 0, ap12 NaN if it has detections, else 0.
 * Built as a library of its own, libctdet_voceval.so (csrc/Makefile), linked against libctdet_hip.so for ctdet_last_error()
 * and the kernel labels: the hot-path library's binary is not touched by it (DESIGN.md 7.16 says why).
 * One workspace serves both calls: ctdet_voceval_workspace_bytes(N, NG, I, K, T) bytes (0: arguments out of range), 256-byte
 *   aligned: 8 T (N/256 + K + 1) (chunk maxima) + 2 * 8N + 5 * 4N (keys, values, orders) + 4 (I*K + 2) (cell offsets) + 4 NG
 *   (taken words of cells too large for LDS) + 16N + 16 MiB (bound of the sort's temporary storage, checked at the call), each
 *   rounded up to 256 bytes. */
#define CTDET_VOC_BAD_CLASS 1
#define CTDET_VOC_BAD_IMAGE 2
#define CTDET_VOC_BAD_SCORE 4
#define CTDET_VOC_BAD_BOX 8
size_t ctdet_voceval_workspace_bytes(int64_t N, int64_t NG, int32_t I, int32_t K, int32_t T);
int32_t ctdet_voceval_match(const float* boxes, const float* scores, const int32_t* classes, const int32_t* image, int64_t N,
                            const double* gt_boxes, const uint8_t* gt_difficult, const int32_t* gt_off, int64_t NG, int32_t I,
                            int32_t K, const double* thrs, int32_t T, void* workspace, int32_t* order, int32_t* cls_off,
                            uint8_t* flags, int32_t* npos, int32_t* status, void* stream);
int32_t ctdet_voceval_ap(const int32_t* order, const int32_t* cls_off, const uint8_t* flags, const int32_t* npos, int64_t N,
                         int32_t K, int32_t T, const double* points, void* workspace, double* ap07, double* ap12, double* rec,
                         double* prec, void* stream);

#ifdef __cplusplus
}
#endif
