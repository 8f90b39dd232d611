/* C ABI of libctdet_lviseval.so: LVIS box-AP scoring (gfx950).  Errors and kernel labels go through libctdet_hip.so
 * (ctdet_last_error, ctdet_set_label_mode / ctdet_last_kernel_label), which this library links against. */
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- LVIS box-AP scoring -------------------------------------------------------------------------------------------
 * The federated rule of LVIS over the detections of a whole dataset in device memory; DESIGN.md 7.17 holds the rule.  All
 * arithmetic is f64, every operation rounded once.  These calls use a device radix sort and are not meant to be captured into
 * a graph.
 *
 * ctdet_lviseval_match: detections concatenated over the dataset -- boxes f32 [N,4] XYXY (width and height are taken in f32,
 *   then widened), scores f32 [N], classes i32 [N] in [0,K), image i32 [N] in [0,I); ground truth sorted by (image, class) with
 *   CSR offsets gt_off i32 [I*K+1] into gt_boxes f64 [NG,4] XYWH, gt_area f64 [NG], gt_ignore u8 [NG]; lists u8 [I,K]: bit
 *   CTDET_LVIS_NEG = the class is a negative class of the image, bit CTDET_LVIS_NEL = its annotation in the image is not
 *   exhaustive (the positive classes are the cells with ground truth); iou_thrs f64 [T]; area_rngs f64 [A,2], both ends
 *   inclusive; A*T <= 64 (one lane per matcher); I*K < 2^26 (one wave per cell); max_det >= 1: the detections an image keeps.
 *   Outputs: order i32 [N] (input index of every position of the total order: class ascending, score descending, image index
 *   ascending, input index ascending; a detection that takes no part -- cut, dropped or invalid -- lies behind cls_off[K]),
 *   cls_off i32 [K+1] (the classes' segments of it), flags u8 [N, A*T] at the INPUT index (bit 0 matched, bit 1 ignored;
 *   written for the detections that take part only), npig i32 [K,A] (non-ignored ground truths), status i32 [1]: OR of
 *   CTDET_LVIS_BAD_* over the invalid detections.
 * ctdet_lviseval_accumulate: from those, with rec_thrs f64 [R] in device memory, R <= 4096: precision f64 [T,R,K,A] and recall
 *   f64 [T,K,A], every element written; -1 for a (class, area range) without non-ignored ground truth.
 * Built as a library of its own, libctdet_lviseval.so (csrc/Makefile), linked against libctdet_hip.so for ctdet_last_error()
 * and the kernel labels: the hot-path library's binary is not touched by it (DESIGN.md 7.16 says why).
 * ctdet_lviseval_workspace_bytes(N, NG, I, K, A, T) bytes (0: arguments out of range), 256-byte aligned, for the match call:
 *   2 * 8N + 5 * 4N (keys, values, orders) + 4 (I*K + 2) + 4 (I + 2) (cell and image offsets) + NG A T
 *   (taken flags of cells too large for LDS) + 16N + 16 MiB (bound of the sort's temporary storage, checked at the call), each
 *   rounded up to 256 bytes.  The accumulate call needs no workspace. */
#define CTDET_LVIS_BAD_CLASS 1
#define CTDET_LVIS_BAD_IMAGE 2
#define CTDET_LVIS_BAD_SCORE 4
#define CTDET_LVIS_BAD_BOX 8
#define CTDET_LVIS_NEG 1
#define CTDET_LVIS_NEL 2
size_t ctdet_lviseval_workspace_bytes(int64_t N, int64_t NG, int32_t I, int32_t K, int32_t A, int32_t T);
int32_t ctdet_lviseval_match(const float* boxes, const float* scores, const int32_t* classes, const int32_t* image, int64_t N,
                             const double* gt_boxes, const double* gt_area, const uint8_t* gt_ignore, const int32_t* gt_off,
                             int64_t NG, const uint8_t* lists, int32_t I, int32_t K, const double* iou_thrs, int32_t T,
                             const double* area_rngs, int32_t A, int32_t max_det, void* workspace, int32_t* order,
                             int32_t* cls_off, uint8_t* flags, int32_t* npig, int32_t* status, void* stream);
int32_t ctdet_lviseval_accumulate(const int32_t* order, const int32_t* cls_off, const uint8_t* flags, const int32_t* npig,
                                  int64_t N, int32_t K, int32_t A, int32_t T, const double* rec_thrs, int32_t R,
                                  double* precision, double* recall, void* stream);

#ifdef __cplusplus
}
#endif
