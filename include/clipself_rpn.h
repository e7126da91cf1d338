/* RPN proposals in libclipself_hip.so: per-level top-k of the RPN head's maps, box decoding and the min-size filter, one call for all
 * images and levels.  Its outputs are the inputs of csd_nms' group form (clipself_det.h), which finishes the step.
 *
 * What every F-ViT config does once per training step and once per served image through mmdet 2.28.1 (the version the reference's README
 * installs): RPNHead._get_bboxes_single (sigmoid, the nms_pre best anchors of each level, DeltaXYWHBBoxCoder.decode against the image
 * shape) and the first half of RPNHead._bbox_post_process (the min_bbox_size filter); batched_nms by level and the cut to max_per_img are
 * csd_nms with group = level.  A seventh header, separate from clipself_hip.h, whose conventions it keeps like clipself_loss.h: plain
 * pointers, caller-allocated device memory, asynchronous launches on `stream`, 0 on success, -1 with the text in the library's last-error
 * string on arguments outside the limits (then nothing is launched and nothing is written), no global state, nothing read back to the
 * host, every output completely written on every call, workspace contents need no initialisation.  mmcv / mmdet are not available to
 * this project: the text below follows the published mmdet 2.28.1 sources as read (parity-unpinned, like clipself_det.h, clipself_roi.h,
 * clipself_assign.h, clipself_loss.h and clipself_mask.h) and says where it fixes what they leave open.  Used together with the other
 * headers, this one is included after them (they share one guarded cs_stream_t typedef and do not know this header's guard).
 *
 * ---- csp_select -------------------------------------------------------------------------------------------------------------------------
 *   levels [L] (HOST array), each: cls [B, A, h, w] and reg [B, 4A, h, w] fp32, contiguous NCHW: the layout of csl_level.
 *   Lists.  A list is one (image b, level l) pair with n_l = h_l * w_l * A anchors.  Anchor i of a level is (y * w + x) * A + a: its logit
 *   is cls[b, a, y, x], its delta j is reg[b, 4a + j, y, x] -- the order csl_rpn_loss documents (cls.permute(0, 2, 3, 1).reshape(-1)).
 *   anchors [N, >= 4] fp32 with row stride lda: all levels one after another, shared by the images, as AnchorGenerator.grid_priors
 *   concatenated gives them and as csa_assign takes them; N = sum n_l.
 *   Selection.  k_l = min(nms_pre, n_l).  A list keeps the k_l anchors with the smallest pair (~ord(logit), i), where ord is the
 *   order-preserving map of the float's bits (u ^ 0x80000000 for u >= 0, ~u below: -0 sorts below +0): the highest logits, ties to the
 *   lower anchor index.  A NaN logit sorts below every number, -inf included (its key is 0xFFFFFFFF, which no number has); NaN logits tie
 *   among themselves by index.
 *   The selection is on the logit, not on the rounded sigmoid: many logits round to one fp32 score (every logit above 17 gives 1), and
 *   mmdet's scores.sort(descending=True) is not stable, so mmdet leaves the order of equal scores open.  Where two fp32 scores differ,
 *   the order here is mmdet's as long as the sigmoid keeps the order of the logits (it is monotone; the form below is monotone up to the
 *   rounding of expf); where they round to equal values this rule fixes what mmdet leaves open.
 *   Output rows.  Ktot = sum k_l.  Image b owns rows b * Ktot .. (b + 1) * Ktot - 1; inside them the block of level l starts at
 *   sum_{l' < l} k_l'; inside a block the rows are in selection order, best first (also when k_l == n_l).
 *   starts [B + 1] int32 = b * Ktot is written by the call (what csd_nms wants; no host-to-device copy is needed).
 *   Per row:
 *     anchor_inds [B * Ktot] int32 (or NULL) = the anchor's row in `anchors`.
 *     scores [B * Ktot] = sigmoid(x) in the form of csl_rpn_loss: e = expf(-|x|); 1 / (1 + e) for x >= 0, e / (1 + e) for x < 0.  A NaN
 *       logit gives a NaN score, which csd_nms drops.
 *     boxes [B * Ktot, 4] contiguous = csd_delta2bbox's arithmetic op for op (mmdet's delta2bbox, add_ctr_clamp=False, clip_border=True),
 *       every product and sum rounded on its own (no fma): d = delta * std + mean; p = (x0 + x1) * 0.5; w = x1 - x0; dwh clamped to
 *       +-|log(wh_ratio_clip)| (computed in double, rounded once); g = p + w * dxy; half = (w * expf(dwh)) * 0.5; (g - half, g + half);
 *       then clamped to [0, w_img] x [0, h_img] with max_shape [B, 2] = (h, w) fp32 on the DEVICE, or not at all with max_shape NULL.
 *       means, stds: HOST float[4].
 *     group [B * Ktot] int32 = l if (x1 - x0) > min_bbox_size && (y1 - y0) > min_bbox_size on the decoded box, else -1.  The comparison
 *       is false for NaN, so a non-finite box gets -1.  A negative min_bbox_size means no filter, as in mmdet (every row gets l).  A group
 *       of -1 is exactly what csd_nms drops.
 *   Limits: 1 <= L <= 8, 1 <= B <= 65535, 1 <= A <= 16, 1 <= h, w <= 512 per level, 1 <= nms_pre <= 4096, Ktot <= 16384 (the Kmax limit
 *   of csd_nms), lda >= 4, wh_ratio_clip > 0, no NULL pointer except max_shape and anchor_inds.
 *   Determinism and safety: grids and every trip count depend on the host arguments only; no floating-point atomics; integer atomics
 *   only on histogram counters, which are only summed; the take of threshold ties is an ordered compaction (prefix sums), never an
 *   arrival order; equal inputs give equal bits.  Indices that pass through the workspace are compared before they index anything.
 *
 * Workspace: csp_workspace(levels, L, B, A, nms_pre) bytes (0 for arguments outside the limits, otherwise at least 256; only h and w of
 * the levels are read): for every list longer than nms_pre three 2048-bin integer histograms, two counters per 2048 anchors and nms_pre
 * 64-bit keys.
 */
#ifndef CLIPSELF_RPN_H
#define CLIPSELF_RPN_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#if !defined(CLIPSELF_HIP_H) && !defined(CLIPSELF_DET_H) && !defined(CLIPSELF_ROI_H) && !defined(CLIPSELF_ASSIGN_H) && !defined(CLIPSELF_LOSS_H) && \
    !defined(CLIPSELF_MASK_H)
typedef struct ihipStream_t* cs_stream_t; /* == hipStream_t; the same typedef as the other headers, which may be included before this one */
#endif

#define CSP_MAX_LEVELS 8
#define CSP_MAX_ANCHORS 16
#define CSP_MAX_SIDE 512
#define CSP_MAX_PRE 4096
#define CSP_MAX_ROWS 16384

typedef struct csp_level {
    const float* cls; /* [B, A, h, w] */
    const float* reg; /* [B, 4A, h, w] */
    int h, w;
} csp_level;

size_t csp_workspace(const csp_level* levels, int L, int B, int A, int nms_pre);

int csp_select(const csp_level* levels, int L, int B, int A, const float* anchors, long lda, int nms_pre, const float* means,
               const float* stds, float wh_ratio_clip, const float* max_shape, float min_bbox_size, float* boxes, float* scores, int* group,
               int* anchor_inds, int* starts, void* workspace, cs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
