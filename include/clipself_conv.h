/* 3 x 3 convolutions of the detector heads in libclipself_hip.so: Conv2d(Cin, Cout, 3, padding=1) on channel-last maps as an implicit GEMM.
 *
 * What every F-ViT config runs through torch otherwise: the shared_convs of FViTBBoxHead, the convs of FCNMaskHead, RPNHead's and the FPN's
 * 3 x 3 convolutions (mmdet 2.28.1 ConvModule -> nn.Conv2d(256, 256, 3, padding=1)).  An eighth header, separate from clipself_hip.h,
 * whose conventions it keeps like clipself_loss.h: plain pointers, caller-allocated device memory, asynchronous launches on `stream`,
 * 0 on success, -1 with the text in the library's last-error string on arguments outside the limits (then nothing is launched and nothing
 * is written), 1 (nothing launched, no error text) on a shape outside an entry point's coverage, as cs_gemm_wgrad_tn; no global state,
 * no workspace, nothing read back to the host, no hipMalloc and no synchronisation in the launch path, every output element written on
 * every call.  The layer is torch's own F.conv2d(padding=1): it is pinned on torch under autograd in float64 (tests/_conv_ref.py).
 *
 * ---- layout, the same for every entry point ------------------------------------------------------------------------------------------
 *   A map is bf16 rows [N * H * W, C] with a row stride ld >= C, ld % 8 == 0, the base 16-byte aligned (a channel-last [N, C, H, W]
 *   tensor is that with ld = C).  Row p = (n * H + y) * W + x.
 *   Tap t = ky * 3 + kx (ky, kx in 0..2) of row p reads pixel (y + ky - 1, x + kx - 1) of the SAME image n, or zeros when that pixel
 *   lies outside the image -- also when the shifted row index would fall on another row (x + kx - 1 outside [0, W)) or into another
 *   image (y + ky - 1 outside [0, H)).  No padded copy of the map exists: the caller supplies no padding.
 *   Packed weights Wg are bf16 [Cout, 9 * Cin], row stride ldw >= 9 * Cin, ldw % 8 == 0:  Wg[co, t * Cin + ci] = weight[co, ci, ky, kx].
 *
 * ---- csc_conv3x3: the convolution as an implicit GEMM --------------------------------------------------------------------------------
 *   y[p, co] = bias[co] + sum over t, ci of x[p shifted by t, ci] * Wg[co, t * Cin + ci]           M = N*H*W rows, Cout columns, K = 9*Cin
 *   bf16 x bf16 products accumulated in fp32 (MFMA), bias (fp32 [Cout], 16-byte aligned, or NULL) added in fp32, ONE rounding at the
 *   output: y is fp32 (out_bf16 == 0) or bf16, round to nearest even (out_bf16 == 1), row stride ldy >= Cout, ldy % 4 == 0, the base
 *   16-byte aligned.  Columns Cout .. ldy - 1 of y are not written.  x and Wg are only read; rows of x outside [0, N*H*W) are never read.
 *   K is ordered (tap, input channel): with Cin % 64 == 0 a 64-wide K tile lies inside one tap, and its A rows are the rows of the map
 *   shifted by (ky - 1) * W + (kx - 1); an out-of-range lane reads a zero-filled device array instead.
 *   Coverage: Cin % 64 == 0, Cout % 8 == 0, N, H, W >= 1; otherwise 1 is returned.
 *   Limits (-1): N * H * W <= 2^31 - 512; ldx, ldw, ldy < 2^31 (byte offsets are 64-bit: N * H * W * ldx may pass 2^31).
 *   The same entry point is the input gradient: dx = csc_conv3x3(dY rows, WgT) with WgT[ci, t * Cout + co] = weight[co, ci, 2 - ky, 2 - kx]
 *   (Cout % 64 == 0 then).  Grid and trip counts depend on the host arguments alone; no atomics: equal inputs give equal bits.
 *
 * ---- csc_im2col3x3: the explicit matrix -------------------------------------------------------------------------------------------------
 *   cols[r, t * Cin + ci] = x[(row0 + r) shifted by t, ci] (zero where the tap is out of range) for r in [0, rows): rows
 *   [row0, row0 + rows) of the [N*H*W, 9*Cin] matrix, bf16, row stride ldc >= 9 * Cin, ldc % 8 == 0, base 16-byte aligned, written in
 *   16-byte stores.  Columns 9 * Cin .. ldc - 1 are not written; cols needs exactly rows * ldc elements (less the last row's padding).
 *   It feeds the weight gradient  dWg[Cout, 9*Cin] += dY^T . cols  (cs_gemm_wgrad_tn on a chunk of rows) and a second forward route
 *   (csc_im2col3x3 + cs_gemm_nt) that the implicit kernel is tested and measured against.
 *   Coverage: Cin % 8 == 0 (else 1).  Limits (-1): 0 <= row0, rows >= 0, row0 + rows <= N*H*W <= 2^31 - 512; Cin <= 2^24.
 *   rows == 0 launches nothing and returns 0.
 */
#ifndef CLIPSELF_CONV_H
#define CLIPSELF_CONV_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#if !defined(CLIPSELF_HIP_H) && !defined(CLIPSELF_DET_H) && !defined(CLIPSELF_ROI_H) && !defined(CLIPSELF_ASSIGN_H) && \
    !defined(CLIPSELF_LOSS_H) && !defined(CLIPSELF_MASK_H) && !defined(CLIPSELF_RPN_H)
typedef struct ihipStream_t* cs_stream_t; /* == hipStream_t; the same typedef as the other headers, which may be included before this one */
#endif

#define CSC_MAX_ROWS 2147483136L /* 2^31 - 512 */

int csc_conv3x3(const void* x, long ldx, const void* wg, long ldw, const float* bias, void* y, long ldy, int out_bf16, int N, int H, int W,
                int Cin, int Cout, cs_stream_t stream);

int csc_im2col3x3(const void* x, long ldx, void* cols, long ldc, long row0, long rows, int N, int H, int W, int Cin, cs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
