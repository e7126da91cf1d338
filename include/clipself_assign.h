/* Detector training targets in libclipself_hip.so: IoU assignment, random sampling and box-delta targets for the RPN and the box head.
 *
 * What every F-ViT config does twice per step through mmdet 2.x (train_cfg.rpn, train_cfg.rcnn): MaxIoUAssigner.assign, RandomSampler.sample,
 * DeltaXYWHBBoxCoder.encode and the target layouts of AnchorHead._get_targets_single / BBoxHead._get_target_single.  A fourth header,
 * separate from clipself_hip.h, whose conventions it keeps like clipself_det.h: plain pointers, caller-allocated device memory,
 * asynchronous launches on `stream`, 0 on success, -1 with the text in the library's last-error string on arguments outside the limits
 * (then nothing is launched and nothing is written), no global state, nothing read back to the host, every output completely written on
 * every call, workspace contents need no initialisation.  mmcv / mmdet are not available to this project: the text below follows the
 * published mmdet 2.x sources as read (parity-unpinned, like clipself_det.h and clipself_roi.h).
 *
 * ---- batch layout ---------------------------------------------------------------------------------------------------------------------
 *   boxes    [K, 4] fp32 (x0, y0, x1, y1), row stride ldb >= 4, rows grouped by image through starts [B + 1] (device int32, as in csd_nms):
 *            image b owns rows starts[b] .. starts[b + 1] - 1.  starts == NULL is the shared form: all B images use the same K rows (the
 *            RPN's anchors).  "row" below is the row within the image, 0 .. n_b - 1.
 *   gt_boxes [Gtot, 4] fp32, row stride ldg >= 4, with gt_starts [B + 1] (device int32, never NULL); gt_labels [Gtot] int32 or NULL.
 *   valid    [K] uint8 or NULL (mmdet's inside_flags), indexed like boxes.  A row with valid == 0 takes part in no maximum, is never
 *            sampled, and leaves as gt_inds = -1, max_overlaps = 0 and weights 0.
 *   Nmax, Gmax: host upper bounds per image; they size grids, LDS and workspace.  An image with more rows uses its first Nmax / Gmax.
 *   Limits: 1 <= B <= 65535, 0 <= Nmax <= 2^20, 0 <= Gmax <= 1024, 1 <= num <= 4096, K >= 0, Gtot >= 0, ldb >= 4, ldg >= 4.
 *   Device data is never trusted: starts / gt_starts are clamped to [0, K] / [0, Gtot] and a non-monotone pair gives an empty image;
 *   gt_inds read back by csa_sample / csa_targets is range-checked (a value outside [-1, G_b] is treated as -1), as is sel (a row outside
 *   [0, n_b) is a padding slot); no loop length and no index comes from an unchecked device value; every trip count is bounded by a host
 *   argument.  Equal inputs give equal bits: no floating-point atomics.  The only atomics are integer: max over the bit patterns of
 *   non-negative floats (exact and independent of order), min over row numbers, and histogram counters that are only summed.
 *
 * ---- csa_assign: MaxIoUAssigner.assign -> assign_wrt_overlaps with BboxOverlaps2D (bbox_overlaps, mode 'iou', eps = 1e-6) ---------------
 *   IoU in fp32, every product, sum and difference rounded on its own (no fma), a true IEEE division:
 *     area = (x1 - x0) * (y1 - y0);  w = max(min(x1a, x1b) - max(x0a, x0b), 0), h likewise;  inter = w * h;
 *     union = max(area_a + area_b - inter, 1e-6f);  iou = inter / union.
 *   A NaN IoU (and an IoU any of whose intermediates is NaN) counts as 0; mmdet would propagate the NaN.
 *   Per valid row n: max_overlaps[n] = max over the image's ground truths, argmax = that ground truth, ties to the lowest index (as
 *   torch's CPU max).  gt_inds = -1; then 0 where neg_lo <= max < neg_hi (mmdet's scalar neg_iou_thr is neg_lo = 0); then argmax + 1
 *   where max >= pos_iou_thr.  Thresholds are compared as fp32.
 *   match_low_quality != 0: for ground truths i = 0 .. G - 1 IN THIS ORDER, later ones overwriting earlier ones and the positive rule
 *   above: if gt_max[i] >= min_pos_iou (gt_max[i] = max of iou(i, .) over the image's valid rows), then with gt_max_assign_all every
 *   valid row with iou(i, n) == gt_max[i] (float equality) gets i + 1, without it only the lowest such row.  So a row ends with the
 *   largest qualifying i.
 *   An image without ground truths: every valid row has gt_inds = 0, max_overlaps = 0.
 *   gt_prefix != 0 (RandomSampler's add_gt_as_proposals, AssignResult.add_gt_): the first G_b rows of image b are its ground truths
 *   themselves; they are left out of both maxima and leave as gt_inds = row + 1, max_overlaps = 1 (when valid).
 *   Outputs gt_inds [B, Nmax] int32, max_overlaps [B, Nmax] fp32; entries past an image's rows are -1 and 0.  The [G, N] matrix is never
 *   written to memory.
 *
 * ---- csa_sample: RandomSampler.sample with the caller's randomness ---------------------------------------------------------------------
 *   keys [B, Nmax] uint32.  expected_pos = (int)(num * pos_fraction), computed by the caller.  Positives are the rows with gt_inds > 0:
 *   all of them if there are at most expected_pos, otherwise the expected_pos rows with the smallest (key, row) pair in unsigned
 *   lexicographic order.  Negatives are the rows with gt_inds == 0: expected_neg = num - sampled_pos, with neg_pos_ub >= 0 capped at
 *   (int)(neg_pos_ub * (float)max(1, sampled_pos)) (an fp32 product, truncated); the same selection rule.  With independent uniform keys
 *   this is a uniform random subset, which is all mmdet's random_choice promises; it is not the sequence torch.randperm would draw.
 *   Outputs: flags [B, Nmax] uint8 (0 not sampled, 1 positive, 2 negative); sel [B, num] int32: the sampled rows (within the image),
 *   positives in ascending row, then negatives in ascending row, padded with -1; counts [B, 2] int32 = (positives, negatives).
 *
 * ---- csa_targets: AnchorHead._get_targets_single + unmap (sel == NULL) / BBoxHead._get_target_single, class-agnostic (sel != NULL) ------
 *   pos_weight <= 0 is the only supported value (every config).  A sampled positive's label is gt_labels[gt_inds - 1] (0 when gt_labels is
 *   NULL); everything else gets bg_label (the RPN passes 1, the box head 65).
 *   Dense form, per (image, row): labels [B, Nmax] int32; label_weights [B, Nmax] fp32: 1 on sampled rows (flags != 0); bbox_targets,
 *   bbox_weights [B, Nmax, 4]: weights 1 on sampled positives (flags == 1 and gt_inds > 0), targets 0 where the weight is 0.  Rows past
 *   the image: bg_label and zeros.  rois may be NULL.
 *   Compact form, per slot of sel: rois [B, num, 5] = ((float)image, the box bit for bit); labels, label_weights [B, num]; bbox_targets,
 *   bbox_weights [B, num, 4].  A listed row is positive iff its gt_inds > 0.  A padding slot is (-1, 0, 0, 0, 0) with bg_label and all
 *   weights 0 (csr_roi_extract_fwd pools a row with image -1 to zeros and sends it no gradient).  flags may be NULL.
 *   Targets: mmdet's bbox2delta in fp32, every operation rounded on its own: pxy = (x0y0 + x1y1) * 0.5, pwh = x1y1 - x0y0, the same for
 *   the ground truth; dxy = (gxy - pxy) / pwh, dwh = logf(gwh / pwh); then (d - mean) / std, means / stds HOST float[4].  A zero or
 *   negative width gives the Inf / NaN mmdet gives (the data pipeline's FilterAnnotations removes such boxes).
 *
 * Workspace: csa_workspace(B, Nmax, Gmax, num) bytes (0 for arguments outside the limits, otherwise at least 256): 8 * B * Gmax for the
 *   per-ground-truth maximum and its lowest row, rounded up.  csa_assign alone uses it.
 */
#ifndef CLIPSELF_ASSIGN_H
#define CLIPSELF_ASSIGN_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#if !defined(CLIPSELF_HIP_H) && !defined(CLIPSELF_DET_H) && !defined(CLIPSELF_ROI_H)
typedef struct ihipStream_t* cs_stream_t; /* == hipStream_t; the same typedef as the other headers, which may be included before this one */
#endif

#define CSA_MAX_ROWS (1 << 20) /* Nmax */
#define CSA_MAX_GT 1024        /* Gmax */
#define CSA_MAX_NUM 4096       /* num */

size_t csa_workspace(int B, int Nmax, int Gmax, int num);

int csa_assign(const float* boxes, long ldb, const int* starts, int K, const float* gt_boxes, long ldg, const int* gt_starts, int Gtot,
               const unsigned char* valid, int B, int Nmax, int Gmax, float pos_iou_thr, float neg_lo, float neg_hi, float min_pos_iou,
               int match_low_quality, int gt_max_assign_all, int gt_prefix, int* gt_inds, float* max_overlaps, void* workspace,
               cs_stream_t stream);

int csa_sample(const int* gt_inds, const unsigned int* keys, const int* starts, int K, const int* gt_starts, int Gtot, int B, int Nmax,
               int Gmax, int num, int expected_pos, float neg_pos_ub, unsigned char* flags, int* sel, int* counts, cs_stream_t stream);

int csa_targets(const float* boxes, long ldb, const int* starts, int K, const float* gt_boxes, long ldg, const int* gt_labels,
                const int* gt_starts, int Gtot, int B, int Nmax, int Gmax, const int* gt_inds, const unsigned char* flags, const int* sel,
                int num, const float* means, const float* stds, int bg_label, float pos_weight, float* rois, int* labels,
                float* label_weights, float* bbox_targets, float* bbox_weights, cs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
