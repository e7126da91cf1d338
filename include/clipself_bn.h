/* Batch norm with an optional fused ReLU on channel-last maps in libclipself_hip.so: the training semantics of nn.BatchNorm2d /
 * nn.SyncBatchNorm (batch statistics, running statistics, a count-weighted merge across ranks), forward and backward.
 *
 * What every ConvModule of the F-ViT detector runs behind its convolution (mmcv/cnn/bricks/conv_module.py: conv -> norm -> act with
 * norm_cfg=dict(type='SyncBN' | 'MMSyncBN'), act_cfg=dict(type='ReLU')).  A ninth header, separate from clipself_hip.h, whose conventions
 * it keeps like clipself_conv.h: plain pointers, caller-allocated device memory, asynchronous launches on `stream`, 0 on success, -1 with
 * the text in the library's last-error string on arguments outside the limits (then nothing is launched and nothing is written), 1
 * (nothing launched, no error text) on a shape outside the coverage; no global state, nothing read back to the host, no hipMalloc and no
 * synchronisation in the launch path, grid and trip counts from the host arguments and the device's CU count alone, every output element
 * written on every call.  No floating-point atomics: equal inputs give equal bits.  The layer is torch's own F.batch_norm (+ F.relu): it
 * is pinned on torch under autograd in float64 (tests/_bn_ref.py).
 *
 * ---- maps, the same for every entry point --------------------------------------------------------------------------------------------
 *   A map is rows [M = N*H*W, C] of bf16 (flag 1) or fp32 (flag 0), one flag per operand, row stride ld >= C with ld % 8 == 0 for bf16
 *   and ld % 4 == 0 for fp32, the base 16-byte aligned (a channel-last [N, C, H, W] tensor is that with ld = C).  Columns C .. ld - 1 are
 *   never read and never written.  Row offsets are 64-bit.
 *   Coverage: C % 8 == 0, otherwise 1 is returned.  Limits (-1): 1 <= M <= CSB_MAX_ROWS, 1 <= C <= CSB_MAX_C, ld < 2^31.
 *   A thread owns a 16-byte channel group of the map and walks rows; the rows are cut into P = csb_row_parts(M, C) contiguous parts,
 *   a function of M, C and the device's CU count.
 *
 * ---- blocks of fp32 the entry points exchange (each 16-byte aligned, contiguous) ------------------------------------------------------
 *   record  rec  [2*C + 4]:  mean[C] | M2[C] = sum (x - mean)^2 | the row count as the bits of an int32, then three zero words.  The
 *                count is carried as integer bits, never as a rounded float.  R records back to back (what an all_gather of one record
 *                per rank gives) are the input of csb_finalize.
 *   state   st   [4*C + 4]:  mean[C] | rstd[C] | scale[C] | shift[C] | 1 / N_total, then three zero words.  1 / N_total == 0 marks a state
 *                built from the running statistics (evaluation mode).
 *   sums         [2*C]:      sum g [C] | sum g * xhat [C]   (this rank's dbeta and dgamma; what a host all-reduces before csb_bwd_apply)
 *   workspace:   csb_workspace(M, C) bytes = 2 * P * C floats of per-part partial sums, 16-byte aligned; 0 outside the limits.
 *
 * ---- csb_stats: this rank's record ------------------------------------------------------------------------------------------------------
 *   Two levels, each in a fixed order.  Every part sums s1 = sum (x - K) and s2 = sum (x - K)^2 per channel, K[c] = x[0, c] (the map's
 *   first row: one shift for the whole map, so the parts' sums add), in fp32: a thread's rows in ascending order, then a pairwise tree
 *   over the threads of the workgroup; the partials go to the workspace.  A second small launch adds the P partials (16 contiguous
 *   slices in ascending order, then a pairwise tree over the slices) and writes  mean = K + s1 / M,  M2 = max(s2 - s1 * (s1 / M), 0).
 *   The shifted sums keep the variance of a map whose mean is large against its spread (E[x^2] - E[x]^2 in fp32 does not).
 *
 * ---- csb_finalize: one small launch ----------------------------------------------------------------------------------------------------
 *   recs != NULL (training): merges the R records in ascending order by the parallel-variance formula (Chan et al.), weighted by count,
 *   as torch.nn.SyncBatchNorm's batch_norm_gather_stats_with_counts:
 *       n = na + nb;  d = mean_b - mean_a;  mean = mean_a + d * (nb / n);  M2 = (M2a + M2b) + d * d * (na * (nb / n))
 *   (records with count <= 0 are skipped), then with N = the total count
 *       rstd = 1.0f / sqrtf(M2 / N + eps);  scale = gamma * rstd;  shift = fmaf(-mean, scale, beta)
 *   (gamma == NULL: scale = rstd; beta == NULL: shift = -mean * scale -- affine=False), writes st, and updates in place
 *       running_mean = (1 - momentum) * running_mean + momentum * mean
 *       running_var  = (1 - momentum) * running_var  + momentum * M2 / (N - 1)        (the unbiased variance; skipped when N == 1)
 *   A NULL running_mean / running_var is a statistic that is not tracked.
 *   recs == NULL (evaluation): mean = running_mean, rstd = 1.0f / sqrtf(running_var + eps) (both required), 1 / N_total = 0; nothing else
 *   is written.  gamma, beta, running_mean, running_var are fp32 [C].  Limits: 1 <= R <= CSB_MAX_RECORDS, eps >= 0.
 *
 * ---- csb_apply ------------------------------------------------------------------------------------------------------------------------
 *   y[m, c] = act(fmaf(x[m, c], scale[c], shift[c])),  act 0 = none, 1 = ReLU (v > 0 ? v : 0), one rounding at y's type (bf16: nearest even).
 *
 * ---- csb_bwd_reduce / csb_bwd_apply --------------------------------------------------------------------------------------------------
 *   g = dy where act == 0 or fmaf(x, scale, shift) > 0, else 0: scale and shift are the stored ones, so the mask is the forward's, bit for
 *   bit, and nothing but x and st is kept for the backward.  xhat = (x - mean) * rstd.
 *   csb_bwd_reduce:  sums = sum g | sum g * xhat over this rank's rows, the two levels of csb_stats (plain sums).
 *   csb_bwd_apply:   dx = a * ((g - sums[c] / N) - xhat * (sums[C + c] / N)),  a = gamma * rstd (gamma == NULL: rstd), 1 / N from st,
 *                    one rounding at dx's type.  With 1 / N == 0 (evaluation) the last two terms are absent: dx = a * g.
 *   dy, x and dx each carry their own type flag and row stride.  A thread's channel group is 8 channels when every map it reads is bf16
 *   and 4 otherwise.
 */
#ifndef CLIPSELF_BN_H
#define CLIPSELF_BN_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#if !defined(CLIPSELF_HIP_H) && !defined(CLIPSELF_DET_H) && !defined(CLIPSELF_ROI_H) && !defined(CLIPSELF_ASSIGN_H) && \
    !defined(CLIPSELF_LOSS_H) && !defined(CLIPSELF_MASK_H) && !defined(CLIPSELF_RPN_H) && !defined(CLIPSELF_CONV_H)
typedef struct ihipStream_t* cs_stream_t; /* == hipStream_t; the same typedef as the other headers, which may be included before this one */
#endif

#define CSB_MAX_ROWS 2147483136L /* 2^31 - 512 */
#define CSB_MAX_C 65536
#define CSB_MAX_RECORDS 4096
#define CSB_REC_EXTRA 4 /* a record is 2*C + 4 floats */
#define CSB_ST_EXTRA 4  /* a state is 4*C + 4 floats */

/* P, the number of row parts (and of partials per channel in the workspace); 0 outside the limits or the coverage */
int csb_row_parts(long M, int C);
size_t csb_workspace(long M, int C);

int csb_stats(const void* x, long ldx, int x_bf16, long M, int C, float* rec, void* ws, cs_stream_t stream);

int csb_finalize(const float* recs, int R, int C, const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                 float* running_var, float* st, cs_stream_t stream);

int csb_apply(const void* x, long ldx, int x_bf16, const float* st, int act, void* y, long ldy, int y_bf16, long M, int C, cs_stream_t stream);

int csb_bwd_reduce(const void* dy, long lddy, int dy_bf16, const void* x, long ldx, int x_bf16, const float* st, int act, float* sums,
                   void* ws, long M, int C, cs_stream_t stream);

int csb_bwd_apply(const void* dy, long lddy, int dy_bf16, const void* x, long ldx, int x_bf16, const float* st, int act, const float* sums,
                  const float* gamma, void* dx, long lddx, int dx_bf16, long M, int C, cs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
