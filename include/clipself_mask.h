/* Detector mask branch in libclipself_hip.so: mask targets, the mask loss with its gradient, and the paste of predicted masks.
 *
 * What the four OV-LVIS configs of the reference add to the box branch through mmdet 2.28.1 (the version the reference's README installs):
 * FCNMaskHead(class_agnostic=True, loss_mask=CrossEntropyLoss(use_mask=True)) with train_cfg.rcnn.mask_size = 28 and
 * test_cfg.rcnn.mask_thr_binary = 0.5 -- mask_target / BitmapMasks.crop_and_resize, mask_cross_entropy, and get_seg_masks /
 * _do_paste_mask(skip_empty=False).  A sixth header, separate from clipself_hip.h, whose conventions it keeps like clipself_loss.h: plain
 * pointers, caller-allocated device memory, asynchronous launches on `stream`, 0 on success, -1 with the text in the library's last-error
 * string on arguments outside the limits (then nothing is launched and nothing is written), no global state, nothing read back to the
 * host, every output completely written on every call, workspace contents need no initialisation.  mmcv / mmdet are not available to
 * this project: the text below follows the published mmdet 2.28.1 / mmcv 1.x sources as read (parity-unpinned, like clipself_det.h,
 * clipself_roi.h, clipself_assign.h and clipself_loss.h) and says where it departs.
 *
 * Arithmetic is fp32, every operation rounded on its own (no fma), divisions are IEEE divisions; expf / log1pf are the device library's.
 * No atomics.  Equal inputs give equal bits: every grid depends on the host arguments only, and the order of every sum is stated below.
 * Device data is never trusted: indices are range-checked where they are read, and every trip count is bounded by a host argument.
 *
 * ---- csm_mask_target: mask_target_single / BitmapMasks.crop_and_resize ------------------------------------------------------------------
 *   rois [R, 5] fp32 contiguous = (image index, x0, y0, x1, y1) in pixels, the layout csa_targets leaves; only the box is used.
 *   gt_rows [R] int32: the row of the slot's ground truth in masks.  masks [Gtot, H, W] uint8: byte (g, y, x) is at
 *   masks + g * plane + y * ldm + x, ldm >= W, plane >= H * ldm (bytes); a byte != 0 counts as 1.  M is mmdet's mask_size.
 *   targets [R, M, M]: soft == 0: uint8, t >= 0.5f ? 1 : 0 (a tie goes to 1, as mmdet's `targets >= 0.5`);  soft != 0: fp32 t (mmdet's
 *   soft_mask_target).
 *   The box is first clipped in fp32 (mmdet's np.clip): x0, x1 to [0, W], y0, y1 to [0, H].  t is mmcv's RoIAlign with aligned=True,
 *   spatial_scale=1, sampling_ratio=0, pool_mode='avg', output M x M, on the one-channel plane masks[gt_rows[r]]: the geometry of
 *   clipself_roi.h with s = 1 and P = M, per axis (x with W shown; y with H likewise):
 *     start = x0 - 0.5f;  end = x1 - 0.5f;  extent = end - start;  bin = extent / M;  grid = (int)ceilf(bin);
 *     count = max(grid_h * grid_w, 1);  sample (pw, ix), ix in [0, grid):  x = (start + pw * bin) + ((ix + 0.5f) * bin) / grid.
 *   Bilinear rule: a sample with x outside [-1, W] contributes nothing; otherwise x <= 0 becomes 0; lo = (int)x; lo >= W - 1 gives
 *   lo = hi = W - 1 and x = lo, else hi = lo + 1; lx = x - lo, hx = 1 - lx.  The per-axis weights hx, lx, hy, ly are the contract (fp32
 *   numbers); the weight of a tap is the product of its two axis weights, and t = (sum over the bin's samples and taps of weight * m) /
 *   count with m in {0, 1}.
 *   Order of the sum (the separable form; mmcv adds sample by sample): per bin column pw, Wx[x] = the tap weights that land on pixel x,
 *   added in ascending (ix, lo before hi); Wy[y] likewise for the bin row ph.  row[y] = sum over x ascending of Wx[x] * m[y, x];
 *   rows y = k, k + RC, k + 2 RC, ... ascending give partial k (RC = min(256 / M, 8)) as partial += Wy[y] * row[y]; the partials are
 *   added in ascending k; the division by count comes last.  Every mask byte of the box is read about once per bin row.
 *   Departures from mmdet: a row whose gt_rows is outside [0, Gtot) gets an all-zero target (-1 is the normal case for non-positive
 *   slots); so does a row with a non-finite box coordinate (mmdet's numpy clip would carry the NaN on); an extent <= 0 after the clip
 *   gives grid 0 and an all-zero target, as mmcv does.  The masks are read in place by index: no [R, H, W] float copy exists.
 *   Limits: 0 <= R <= 2^20, 0 <= Gtot <= 2^24, 1 <= H, W <= 2048, ldm >= W, plane >= H * ldm, 1 <= M <= 64.
 *
 * ---- csm_mask_loss: FCNMaskHead.loss / mask_cross_entropy, with gradient ----------------------------------------------------------------
 *   pred [R, C, M, M] fp32 contiguous; labels [R] int32 or NULL (NULL: channel 0 for every row, what mmdet passes as zeros_like(labels)
 *   with class_agnostic=True); targets [R, M, M] uint8 (a byte != 0 is t = 1) or, with soft != 0, fp32 t; row_weights [R] fp32.
 *   A row is counted when row_weights > 0 and its label is in [0, C).  n = max(count of counted rows, 1), counted on the device;
 *   den = (float)n * (float)(M * M), one fp32 product.  No eps: mmdet's reduction='mean' of binary_cross_entropy_with_logits.
 *   On the picked channel of the counted rows, with w the row's weight (the expressions of csl_rpn_loss):
 *     e = expf(-|x|);  bce = (max(x, 0) - x * t) + log1pf(e);                          loss  = sum(w * bce) / den
 *     sigmoid(x) = 1 / (1 + e) for x >= 0, e / (1 + e) for x < 0;                      dpred = (w * (sigmoid(x) - t)) / den
 *   out [2] = (loss, n).  dpred [R, C, M, M] or NULL (a forward-only call): every element is written, 0 on the channels that were not
 *   picked and on the rows that are not counted.  Stores of 16 bytes are used where the address of a group of four cells of a plane is
 *   16-byte aligned (checked on the address, never assumed from a shape); the rest are scalar.  The values do not depend on it.
 *   Order of the sum: one workgroup per (row, channel) plane; thread j adds the groups of four cells j, j + 256, ... in ascending order,
 *   cells ascending inside a group; a butterfly inside each wave, the four waves in ascending order; the per-row sums go to the
 *   workspace and one finishing workgroup adds rows j, j + 256, ... ascending per thread, then in the same fixed order.
 *   Departures from mmdet: a row with weight 0 (or negative, or NaN) or a label outside [0, C) contributes exactly 0, gets a zero
 *   gradient and its prediction is not read; R == 0, or no counted row, gives loss 0 and all gradients 0 (mmdet returns
 *   mask_pred.sum() on an empty batch).
 *   Limits: 0 <= R <= 2^20, 1 <= C <= 4096, 1 <= M <= 64, R * C * M * M < 2^31.
 *
 * ---- csm_paste_masks: FCNMaskHead.get_seg_masks / _do_paste_mask(skip_empty=False) ------------------------------------------------------
 *   logits [N, C, M, M] fp32 contiguous; labels [N] int32 or NULL (channel 0); boxes [N, 4] fp32 contiguous, already in output-image
 *   pixels (the division by scale_factor is the caller's); img_h, img_w, thr >= 0 host values.
 *   out [N, img_h, img_w] uint8 = (v >= thr); soft [N, img_h, img_w] fp32 = v, or NULL (a test and debugging aid).  64-bit indices.
 *   p = sigmoid(x) in the form above.  Per axis (x shown), torch's grid_sample coordinate (align_corners=False), op for op in fp32:
 *     gx = ((X + 0.5f) - x0) / (x1 - x0) * 2 - 1;   ix = ((gx + 1) * M - 1) / 2;   fx = floorf(ix)
 *     wx0 = (fx + 1) - ix  on the tap fx,   wx1 = ix - fx  on the tap fx + 1;   a tap outside [0, M) contributes nothing (zero padding)
 *     v = ((wx0 * wy0) * p_nw + (wx1 * wy0) * p_ne) + (wx0 * wy1) * p_sw) + (wx1 * wy1) * p_se: torch's order nw, ne, sw, se.
 *   A pixel whose ix is outside [-1, M) or whose iy is outside [-1, M) has no tap inside the mask and is exactly 0; such pixels are
 *   written as zero stores, 16 bytes wide where the address allows, without computing a coordinate per pixel.
 *   Departures from mmdet: a box with a non-finite coordinate, or x1 - x0 <= 0, or y1 - y0 <= 0, writes an all-zero mask (mmdet's
 *   inf-to-0 patch would paint the mask's centre value over the whole image); so does a label outside [0, C).  thr < 0 (mmdet's 0 - 255
 *   soft bytes) is refused with -1.
 *   Limits: 0 <= N <= 2^20, 1 <= C <= 4096, 1 <= M <= 64, N * C * M * M < 2^31, 1 <= img_h, img_w <= 16384,
 *   N * ceil(img_h / 16) < 2^31, thr >= 0 and not NaN.
 *
 * Workspace: csm_workspace(R) bytes for csm_mask_loss on R rows (0 for R outside the limits, otherwise at least 256): one fp32 per row
 * and the count partials.  csm_mask_target and csm_paste_masks need none.
 */
#ifndef CLIPSELF_MASK_H
#define CLIPSELF_MASK_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#if !defined(CLIPSELF_HIP_H) && !defined(CLIPSELF_DET_H) && !defined(CLIPSELF_ROI_H) && !defined(CLIPSELF_ASSIGN_H) && !defined(CLIPSELF_LOSS_H)
typedef struct ihipStream_t* cs_stream_t; /* == hipStream_t; the same typedef as the other headers, which may be included before this one */
#endif

#define CSM_MAX_ROWS (1 << 20)
#define CSM_MAX_GT (1 << 24)
#define CSM_MAX_SIDE 2048
#define CSM_MAX_MASK 64
#define CSM_MAX_CLASSES 4096
#define CSM_MAX_IMAGE 16384

size_t csm_workspace(int R);

int csm_mask_target(const float* rois, const int* gt_rows, int R, const unsigned char* masks, int Gtot, int H, int W, long ldm, long plane,
                    int M, int soft, void* targets, cs_stream_t stream);

int csm_mask_loss(const float* pred, const int* labels, const void* targets, int soft, const float* row_weights, int R, int C, int M,
                  float* out, float* dpred, void* workspace, cs_stream_t stream);

int csm_paste_masks(const float* logits, const int* labels, const float* boxes, int N, int C, int M, int img_h, int img_w, float thr,
                    unsigned char* out, float* soft, cs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
