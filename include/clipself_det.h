/* Detector post-processing in libclipself_hip.so: box decoding, score threshold, class-aware greedy NMS and the per-image cut.
 *
 * What the reference's F-ViT/models/fvit_head.py:123-164 (FViTBBoxHead.get_bboxes) does after the scores: bbox_coder.decode, rescale,
 * multiclass_nms -- and, in the group form, the batched_nms of the RPN (F-ViT/configs/ov_coco, rpn_proposal).  Not an engine op: this
 * header is separate from clipself_hip.h, whose conventions it keeps (plain pointers, caller-allocated device memory, asynchronous
 * launches on `stream`, 0 on success, negative on error with the text in the library's last-error string (clipself_hip.h), no global
 * state).  Nothing here reads a result back to the host; all outputs have fixed shapes.
 *
 * ---- csd_nms: the contract ---------------------------------------------------------------------------------------------------------
 * Inputs, batched over B images:
 *   boxes  [K, 4] fp32 (x0, y0, x1, y1), row stride ldb >= 4.  Class-agnostic (reg_class_agnostic=True in every F-ViT config).
 *   scores [K, C] fp32, row stride lds >= C: foreground classes only (drop the background column by passing C = classes - 1).
 *   starts [B + 1] int32, device: image b owns rows starts[b] .. starts[b + 1] - 1 (rows grouped by image, the layout bbox2roi builds).
 *   Kmax   host int, an upper bound on boxes per image (sizes grids and workspace); an image with more uses its first Kmax rows.
 *   group  [K] int32 or NULL, G groups: the RPN form, needs C == 1.  A box takes part only in the list of its group (mmcv's `idxs`,
 *          the FPN level); a group id outside [0, G) drops the box.
 * Candidates: (k, c) iff scores[k, c] > score_thr (strict; false for NaN); its list is (image of k, c).  Group form: box k iff
 *   scores[k, 0] > score_thr; its list is (image of k, group[k]).
 * IoU (mmcv nms, offset 0), all fp32, every product and sum rounded on its own (no fma), IEEE division:
 *   area = (x1 - x0) * (y1 - y0); iw = max(min(x1a, x1b) - max(x0a, x0b), 0), ih likewise; inter = iw * ih;
 *   iou = inter / (area_a + area_b - inter).  A kept a suppresses b iff iou > iou_thr (strict).  0/0 and NaN suppress nothing, so a
 *   zero-area box and a box with non-finite coordinates are kept and suppress nobody.
 * Order within a list: score descending, ties by ascending box row (scores compare by their bits' order: -0 below +0).  Per-list NMS on
 *   the un-offset boxes: what mmcv's batched_nms computes with its label * (max + 1) offsets in exact arithmetic, translation-invariant.
 * Cut: per image the max_num best kept candidates, score descending, ties by ascending flat index k_local * C + c (group form: box row).
 * Outputs, written completely on every call (entries past counts[b]: zeros in dets, -1 in labels and inds):
 *   dets [B, max_num, 5] fp32: the four input coordinates bit for bit + the score; labels [B, max_num] int32: class (group form: the
 *   group id); inds [B, max_num] int32: the box row k in `boxes`; counts [B] int32.
 * Limits -- outside them the call returns -1, sets the error text and launches nothing: 1 <= B <= 65535, C >= 1, K >= 0,
 *   0 <= Kmax <= 16384, Kmax * C < 2^31, 1 <= max_num <= 4096, ldb >= 4, lds >= C, group only with C == 1 (then G >= 1), workspace not NULL.
 * Device-side indices: starts is clamped to [0, K] and every image to Kmax rows; a non-monotone starts gives empty images; no loop
 *   length or index comes from an unchecked device value.  K == 0 or an empty image: counts = 0 and padding.  Equal inputs give equal
 *   bits: no floating-point atomics; the integer counters used only order keys that are sorted afterwards.
 * Workspace: csd_nms_workspace(B, Kmax, C or G, max_num) bytes (0 for arguments outside the limits): B * Kmax * ceil(Kmax / 64) * 8 for
 *   the IoU bit matrix, 8 * B * lists * min(max_num, Kmax) for the kept keys, and, when Kmax > 2048 (lists that do not sort in LDS),
 *   8 * B * lists * pow2(Kmax).  Contents need no initialisation and carry nothing between calls.
 */
#ifndef CLIPSELF_DET_H
#define CLIPSELF_DET_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef CLIPSELF_HIP_H
typedef struct ihipStream_t* cs_stream_t; /* == hipStream_t; the same typedef as clipself_hip.h, which may be included before this header */
#endif

#define CSD_MAX_BOXES 16384 /* Kmax */
#define CSD_MAX_NUM 4096    /* max_num */

size_t csd_nms_workspace(int B, int Kmax, int C_or_G, int max_num);

int csd_nms(const float* boxes, long ldb, const float* scores, long lds, int C, const int* starts, const int* group, int G, int K, int B,
            int Kmax, float score_thr, float iou_thr, int max_num, float* dets, int* labels, int* inds, int* counts, void* workspace,
            cs_stream_t stream);

/* mmdet 2.x DeltaXYWHBBoxCoder.decode (delta2bbox with add_ctr_clamp=False, clip_border=True), then the rescale of fvit_head.py:153-156.
 * rois [K, >= 4] columns x0, y0, x1, y1 (pass rois + 1 with ldr = 5 for [K, 5] rois), deltas [K, 4], out_boxes [K, 4]; ld* >= 4.
 * means, stds: HOST float[4].  fp32, every product and sum rounded on its own:
 *   d = delta * std + mean;  pxy = (x0y0 + x1y1) * 0.5;  pwh = x1y1 - x0y0;  dwh = clamp(dwh, +-|log(wh_ratio_clip)|) (the bound is
 *   computed in double from the float argument and rounded once);  g_xy = pxy + pwh * dxy;  g_wh = pwh * expf(dwh);
 *   corners = g_xy -+ (g_wh * 0.5);  with max_shape ([B, 2] = (h, w), device) x is clamped to [0, w] and y to [0, h];  with scale
 *   ([B, 4], device: the image's scale_factor) the corners are DIVIDED by it -- a true IEEE division, as the reference's
 *   `bboxes / scale_factor`; pass the scale factor itself, not its reciprocal.
 * max_shape / scale need starts [B + 1] (device, as in csd_nms): row k belongs to the image b with starts[b] <= k < starts[b + 1]; for
 * any contents of starts the image index used is inside [0, B).  Every row of out_boxes is written. */
int csd_delta2bbox(const float* rois, long ldr, const float* deltas, long ldd, const int* starts, int B, int K, const float* means,
                   const float* stds, float wh_ratio_clip, const float* max_shape, const float* scale, float* out_boxes, long ldo,
                   cs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
