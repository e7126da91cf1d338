/* Detector losses in libclipself_hip.so: the RPN's and the box head's losses with their gradients, one call per head.
 *
 * What every F-ViT config does once per step through mmdet 2.28.1 (the version the reference's README installs): RPNHead.loss
 * (CrossEntropyLoss(use_sigmoid=True) + L1Loss over the dense targets of AnchorHead.get_targets) and BBoxHead.loss with
 * reg_class_agnostic=True (the reference's CustomCrossEntropyLoss(use_sigmoid=False) + L1Loss + accuracy).  A fifth header, separate from
 * clipself_hip.h, whose conventions it keeps like clipself_assign.h: plain pointers, caller-allocated device memory, asynchronous
 * launches on `stream`, 0 on success, -1 with the text in the library's last-error string on arguments outside the limits (then nothing
 * is launched and nothing is written), no global state, nothing read back to the host, every output completely written on every call,
 * workspace contents need no initialisation.  mmcv / mmdet are not available to this project: the text below follows the published
 * mmdet 2.28.1 sources as read (parity-unpinned, like clipself_det.h, clipself_roi.h and clipself_assign.h) and says where it departs.
 *
 * Arithmetic is fp32, every operation rounded on its own (no fma), divisions are IEEE divisions; expf / logf / log1pf are the device
 * library's.  FLT_EPSILON = 2^-23 is mmdet's eps of weight_reduce_loss.  Sums: per-workgroup (RPN) or per-row (box head) partial sums go
 * to the workspace and a finishing launch adds them in a fixed order; the grids and the order depend on the host arguments only, never on
 * the part's compute-unit count, so equal inputs give equal bits on any part.  No floating-point atomics, no atomics at all.
 * Device data is never trusted: labels are range-checked where they are read, and every trip count is bounded by a host argument.
 *
 * ---- csl_rpn_loss: RPNHead.loss (AnchorHead.loss_single for every level, all images) --------------------------------------------------
 *   levels [L] (HOST array, 1 <= L <= 8), each: cls [B, A, h, w] and reg [B, 4A, h, w] fp32, contiguous NCHW, and the gradients dcls,
 *   dreg of the same shapes.  Over the whole array the gradient pointers are all given or all NULL (NULL: a forward-only call).
 *   Dense targets exactly as csa_targets' dense form leaves them: labels [B, N] int32 (0 foreground, 1 background), label_weights [B, N],
 *   bbox_targets, bbox_weights [B, N, 4] fp32, N = sum over levels of h * w * A, the levels one after another.  Anchor n of a level is
 *   (y * w + x) * A + a: mmdet's order (cls.permute(0, 2, 3, 1).reshape(-1)); box coordinate k of anchor a is channel 4a + k of reg.
 *   avg_factor: a DEVICE fp32 scalar (mmdet's num_total_samples);  den = avg_factor + FLT_EPSILON, rounded to fp32.
 *   losses [L, 2] = (loss_cls, loss_bbox) per level, mmdet's weight_reduce_loss(reduction='mean', avg_factor) of 2.28.1:
 *     t = (label == 0);  e = expf(-|x|);  bce = (max(x, 0) - x * t) + log1pf(e);      loss_cls  = sum(lw * bce) / den
 *     l1 = |pred - target|;                                                          loss_bbox = sum(bw * l1)  / den
 *   Gradients of the sum of the 2L losses at unit upstream gradient, in the predictions' layout:
 *     sigmoid(x) = 1 / (1 + e) for x >= 0, e / (1 + e) for x < 0;                     dcls = (lw * (sigmoid(x) - t)) / den
 *     sign(d) = 1, -1 or 0 (d == 0, as torch; a NaN d gives NaN);                     dreg = (bw * sign(pred - target)) / den
 *   Departures from mmdet: an element whose weight is 0 contributes exactly 0, gets gradient exactly 0 and its prediction (and box
 *   target) is not read -- mmdet would turn a non-finite prediction there into a NaN (0 * inf); a label outside {0, 1} counts as
 *   weight 0 (mmdet's binary_cross_entropy would take it as background or ignore it).
 *   Limits: 1 <= L <= 8, 1 <= B <= 65535, 1 <= A <= 16, 1 <= h, w <= 512 per level, B * 4A * ceil(h * w / 4) < 2^31 per level.
 *   Stores of 16 bytes are used where the address of a group of four cells is 16-byte aligned (checked on the address, never assumed
 *   from a shape); the rest, and the last group of a plane whose h * w is no multiple of 4, are scalar.
 *
 * ---- csl_bbox_head_loss: BBoxHead.loss, reg_class_agnostic=True, CustomCrossEntropyLoss(use_sigmoid=False) + L1Loss + accuracy ---------
 *   cls_score [R, C1] fp32, row stride ldc >= C1 (C1 = classes + background); labels [R] int32; label_weights [R] fp32; class_weight
 *   [C1] fp32 or NULL (all 1); bbox_pred, bbox_targets, bbox_weights [R, 4] fp32 contiguous; bg_label (mmdet's num_classes).
 *   avg_factor: a DEVICE fp32 scalar or NULL; NULL means avg = max(count(label_weights > 0), 1), computed on the device (mmdet reads it
 *   back with .item()).  den = avg + FLT_EPSILON, rounded to fp32.
 *   Masking: a class with class_weight < 1e-5f takes no part in the softmax or the argmax and has gradient 0.  The reference writes -inf
 *   into the caller's logits; here cls_score is only read.
 *     m = max over unmasked x;  s = sum over unmasked expf(x - m);  loss_r = -class_weight[y] * ((x_y - m) - logf(s))
 *     loss_cls = sum(lw_r * loss_r) / den
 *     acc = 100 * count(argmax_r == label_r) / R over all R rows (zero-weight rows included, as mmdet's accuracy()), argmax over the
 *       unmasked classes, ties to the lowest index (mmdet's topk leaves ties open), a NaN logit is never the argmax; 0 when R == 0.
 *     loss_bbox = sum over rows with 0 <= label < bg_label of bw * |pred - target| / (R + FLT_EPSILON): mmdet's
 *       avg_factor = bbox_targets.size(0); 0 when no row is positive.  A row adds its four terms in the order ((k0 + k1) + k2) + k3.
 *   out [4] = (loss_cls, acc, loss_bbox, the avg used).
 *   dcls [R, C1] with row stride ldc, columns C1 .. ldc - 1 are not written: coef = (lw_r * class_weight[y]) / den,
 *     dcls[r][c] = coef * (expf(x_c - m) / s - [c == y]), and 0 on masked classes.
 *   dbbox [R, 4] = (bw * sign(pred - target)) / (R + FLT_EPSILON) on positive rows, 0 elsewhere.  Either gradient pointer may be NULL.
 *   Departures from mmdet: a row whose label is -100 (torch's ignore_index), is outside [0, C1) (torch asserts), or names a masked class
 *   (torch returns NaN: 0 * -inf) contributes 0 to loss_cls and gets a zero gradient row; it still counts in acc's R, never as a hit
 *   unless its label is the argmax.  A row with lw == 0 contributes 0 and gets a zero gradient row whatever its logits hold; an element
 *   with bw == 0 contributes 0, gets gradient 0 and its prediction is not read.
 *   Limits: 0 <= R <= 2^20, 1 <= C1 <= 4096, ldc >= C1.
 *
 * Workspace: csl_workspace(levels, L, B, A, R) bytes for either call (0 for arguments outside the limits, otherwise at least 256):
 *   one fp32 partial per workgroup of csl_rpn_loss (L >= 1) and 12 bytes per row plus the count partials of csl_bbox_head_loss.
 *   L == 0 (levels ignored) sizes it for csl_bbox_head_loss alone, R == 0 for csl_rpn_loss alone.
 */
#ifndef CLIPSELF_LOSS_H
#define CLIPSELF_LOSS_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#if !defined(CLIPSELF_HIP_H) && !defined(CLIPSELF_DET_H) && !defined(CLIPSELF_ROI_H) && !defined(CLIPSELF_ASSIGN_H)
typedef struct ihipStream_t* cs_stream_t; /* == hipStream_t; the same typedef as the other headers, which may be included before this one */
#endif

#define CSL_MAX_LEVELS 8
#define CSL_MAX_ANCHORS 16
#define CSL_MAX_SIDE 512
#define CSL_MAX_ROWS (1 << 20)
#define CSL_MAX_CLASSES 4096

typedef struct csl_level {
    const float* cls; /* [B, A, h, w] */
    const float* reg; /* [B, 4A, h, w] */
    float* dcls;      /* [B, A, h, w] or NULL */
    float* dreg;      /* [B, 4A, h, w] or NULL */
    int h, w;
} csl_level;

size_t csl_workspace(const csl_level* levels, int L, int B, int A, int R);

int csl_rpn_loss(const csl_level* levels, int L, int B, int A, const int* labels, const float* label_weights, const float* bbox_targets,
                 const float* bbox_weights, const float* avg_factor, float* losses, void* workspace, cs_stream_t stream);

int csl_bbox_head_loss(const float* cls_score, long ldc, const int* labels, const float* label_weights, const float* class_weight,
                       const float* bbox_pred, const float* bbox_targets, const float* bbox_weights, int R, int C1, int bg_label,
                       const float* avg_factor, float* out, float* dcls, float* dbbox, void* workspace, cs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
