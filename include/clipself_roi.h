/* Detector RoI extractor in libclipself_hip.so: multi-level RoIAlign, forward and backward.
 *
 * What the reference's F-ViT/models/fvit_head.py:267-277 (FViTRoIHead._bbox_forward) calls as `self.bbox_roi_extractor(x, rois)`: mmdet
 * 2.x SingleRoIExtractor (map_roi_levels) over mmcv 1.x RoIAlign(output_size = P, sampling_ratio, aligned=True, pool_mode='avg').  Both are
 * restated from their published sources, not run.  Not an engine op and not post-processing: a third header beside
 * clipself_hip.h and clipself_det.h, whose conventions it keeps (plain pointers, caller-allocated device memory, asynchronous launches
 * on `stream`, 0 on success, negative on error with the text in the library's last-error string (clipself_hip.h), no global state).
 * Nothing here reads a result back to the host.
 *
 * ---- the contract ------------------------------------------------------------------------------------------------------------------
 * Maps: L levels, 1 <= L <= 4, finest first.  Level l is [B, h_l, w_l, C] fp32, channel-last (the storage of a torch.channels_last
 *   tensor): cell (b, y, x) starts at map + ((b * h_l + y) * w_l + x) * ld_l, its C channels are contiguous.  ld_l >= C is the level's
 *   own row stride in floats; C % 4 == 0, ld_l % 4 == 0, map 16-byte aligned; 1 <= h_l, w_l <= 512.  spatial_scale_l = (float)(1.0 /
 *   stride_l) is computed by the caller on the host; strides need not be integers (3.5, 7, 14, 28 for the L/14 towers).
 * Boxes: rois [K, 5] fp32, contiguous = (image index, x0, y0, x1, y1) in pixels, in any order, not grouped by image.
 * Level of a box (mmdet map_roi_levels), fp32, every operation rounded on its own:
 *   scale = sqrtf((x1 - x0) * (y1 - y0));  t = floorf(log2f(scale / finest_scale + 1e-6f));  lvl = t clamped to [0, L - 1];
 *   a NaN t (negative or non-finite area) is level 0.
 * Pooling (mmcv roi_align_forward_cuda_kernel, aligned, avg), fp32, every product, quotient and sum rounded on its own (no fma), per
 *   axis (x with w_l shown; y with h_l likewise), s = spatial_scale_lvl:
 *   start = x0 * s - 0.5f;  end = x1 * s - 0.5f;  extent = end - start;  bin = extent / P;
 *   grid = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(extent / P);  count = max(grid_h * grid_w, 1);
 *   sample (pw, ix), ix in [0, grid):  x = (start + pw * bin) + ((ix + 0.5f) * bin) / grid.
 *   Bilinear rule (oracle/roi_align_ref.py states the same one): a sample with y outside [-1, h] or x outside [-1, w] contributes
 *   nothing and reads nothing; otherwise x <= 0 becomes 0; lo = (int)x; lo >= w - 1 gives lo = hi = w - 1 and x = lo, else hi = lo + 1;
 *   lx = x - lo, hx = 1 - lx; the four taps (y_lo, x_lo), (y_lo, x_hi), (y_hi, x_lo), (y_hi, x_hi) carry the weights hy * hx, hy * lx,
 *   ly * hx, ly * lx.  These weights are the contract; the sum over a bin's taps is an fp32 sum whose order is fixed (bins' samples
 *   in ascending (iy, ix), taps in the order above) but not prescribed, so an implementation is held to a summation bound.
 *   out[k, ph, pw, :] = (sum over the bin's samples and taps of weight * map value) / count.
 * Bounded boxes: a box pools to zeros, sends no gradient and never indexes a map when its image index is not in [0, B) (NaN included)
 *   or its extent on its level is non-finite or, in absolute value, larger than twice the grid side on either axis.  With
 *   sampling_ratio == 0 an extent <= 0 has no samples and pools to zeros by the algorithm itself; with sampling_ratio > 0 an inverted
 *   box is sampled as mmcv samples it.  No loop length or index comes from an unchecked device value: per axis a box has at most
 *   P * grid <= 1024 + P samples.
 * Forward: out [K, P, P, C] fp32, bin (k, ph, pw) starts at out + ((k * P + ph) * P + pw) * ldo, ldo >= C, ldo % 4 == 0.  Every one
 *   of the K * P * P * C elements is written.
 * Backward: dmaps_l[b, y, x, :] += sum of weight * (dout[k, ph, pw, :] / count) over every tap that lands on the cell, for all levels
 *   in one call (pass the gradient maps as `levels`, same shapes and strides as the forward's).  A gather: each cell adds its taps in
 *   ascending box row k; within a box in ascending (ph, pw); within a bin in ascending (iy, ix); taps in the order above.  No
 *   floating-point atomics; equal inputs give equal bits.  Cells no box touches are left as they are.  Boxes are found per 4 x 4 tile
 *   of cells by a scan over the boxes of the tile's (image, level) against a rectangle of cells; a prepass writes the rectangles and
 *   the boxes of every (image, level) in ascending row into the workspace.
 * Limits -- outside them the call returns -1, sets the error text and launches nothing: 1 <= L <= 4, 1 <= B <= 65535, C >= 4 and
 *   C % 4 == 0, 1 <= h_l, w_l <= 512, ld_l >= C and ld_l % 4 == 0, spatial_scale_l and finest_scale finite and > 0, 0 <= K <= 2^24,
 *   1 <= P <= 14, 0 <= sampling_ratio <= 8, ldo >= C and ldo % 4 == 0, no NULL pointer when K > 0, 16-byte aligned maps, out and dout.
 * Workspace (backward only): csr_roi_extract_workspace(K) bytes (0 for K outside its limits): 64 per box for the geometry, 4 per box
 *   (rounded up to 16) for the sorted rows, 32 KiB for the bins' counts and offsets.  16-byte aligned.  Contents need no
 *   initialisation and carry nothing between calls.
 */
#ifndef CLIPSELF_ROI_H
#define CLIPSELF_ROI_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#if !defined(CLIPSELF_HIP_H) && !defined(CLIPSELF_DET_H)
typedef struct ihipStream_t* cs_stream_t; /* == hipStream_t; the same typedef as clipself_hip.h / clipself_det.h, which may be included before this header */
#endif

#define CSR_MAX_LEVELS 4
#define CSR_MAX_SIDE 512
#define CSR_MAX_P 14
#define CSR_MAX_SR 8 /* sampling_ratio */

typedef struct csr_level {
    float* map;          /* forward: the level's map, only read.  backward: the level's gradient map, accumulated into */
    long ld;             /* floats between consecutive cells, >= C */
    int h, w;            /* grid of the level */
    float spatial_scale; /* (float)(1.0 / stride) */
} csr_level;

size_t csr_roi_extract_workspace(int K);

int csr_roi_extract_fwd(const csr_level* levels, int L, int B, int C, const float* rois, int K, int P, int sampling_ratio,
                        float finest_scale, float* out, long ldo, cs_stream_t stream);

int csr_roi_extract_bwd(const float* dout, long ldo, const float* rois, int K, int P, int sampling_ratio, float finest_scale,
                        const csr_level* dlevels, int L, int B, int C, void* workspace, cs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
