/* C ABI of libclipself_hip.so -- the drop-in seam under the CLIPSelf hot path.
 *
 * The reference (wusize/CLIPSelf) is pure Python and has no FFI of its own; the native code it reaches lives in
 * third-party wheels (cuBLAS/cuDNN via torch, torchvision roi_align, xformers attention, apex LayerNorm).  Each
 * entry point below names the reference call site(s) (file:line under /root/reference) whose kernel it replaces.
 *
 * Conventions: plain pointers + sizes, no torch types; every buffer (incl. workspaces) is caller-allocated device
 * memory; launches are asynchronous on `stream`; return 0 on success, negative on error (message via
 * cs_last_error(), thread-local); no global mutable state; re-entrant from any thread that owns the stream.
 * bf16 tensors are passed as `void*` / `const void*`.  Row-major everywhere; `ld*` are row strides in elements.
 */
#ifndef CLIPSELF_HIP_H
#define CLIPSELF_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* cs_stream_t; /* == hipStream_t */

const char* cs_last_error(void);

/* --- matmuls: F.linear at src/open_clip/eva_clip/eva_vit_model.py:99-103 (SwiGLU w1,w2,w3), :177-179 (q/k/v proj),
 *     :219/:253 (attn proj), :250 (v-only proj of the last dense block), :585/:617 (head), nn.Conv2d patch embed :348,355
 *     (as im2row GEMM), and their autograd backward (dgrad / wgrad).
 * C[M,N] (+epilogue) = A[M,K] . B[N,K]^T, bf16 operands, fp32 accumulation.  K % 64 == 0, lda/ldb % 8 == 0.
 * epi: 0 bf16 = acc+bias | 1 f32 = acc+bias | 2 f32 = extra(residual)+acc+bias (in-place allowed) |
 *      3 fused SwiGLU: B=[W1;W2] [2*group,K], bias [2*group], out bf16 [M,group] = silu(x1)*x2 |
 *      4 f32 atomic accumulate (split-K allowed: `splits` >= 1, or <= 0 = chosen by the library) |
 *      5 patch embed: out row = row + row/group + 1, value += extra[(row%group+1)*ldc + col]   (cls/pos layout :540-543) |
 *      7 bf16 = GELU(acc+bias), 8 bf16 = QuickGELU(acc+bias): c_fc + activation of the OpenAI-CLIP ViT MLP
 *        (src/open_clip/transformer.py:209-213 `mlp`, :31-34 `QuickGELU`) |
 *      9 bf16 = ReLU(acc+bias), v < 0 ? 0 : v (a NaN passes): the detector box head's Linear + ReLU
 *        (F-ViT/models/fvit_head.py:82-83, 95-96, 104-105: shared_fcs, cls_fcs, reg_fcs)
 *      10 / 11 / 12 the THIN forms: 1 <= N <= 16 output columns, a stream over the rows and not a tiled GEMM (see below; their own
 *        argument rules replace the ones of this paragraph); 12 is their weight and bias gradient
 * splits: 1 everywhere except
 *      epi 4: the atomic split-K above;
 *      epi 0 / 9: deterministic split-K for skinny, deep problems (the box head's 4096 x 512 outputs behind K = 12 544).  `splits` > 1, or
 *        <= 0 = chosen by the library, cuts the K / 64 K tiles into `splits` contiguous slices of ceil(K / 64 / splits) tiles; `extra` is
 *        then an fp32 WORKSPACE of at least splits * M * N floats, 16-byte aligned, that receives each slice's partial product
 *        [M, N] (contiguous, slice-major); one pass adds the partials in ascending slice order, adds `bias` once, applies the ReLU
 *        of epi 9 and writes the bf16 rows at ldc (columns >= N of a padded C stay untouched).  No atomics: the same (M, N, K, splits)
 *        gives the same bits.  The library's choice for splits <= 0 is a pure function of the shape and the device:
 *            s = 1;  while (s < 8  &&  ceil(M/256) * ceil(N/256) * 2s <= compute units  &&  (K/64) / (2s) >= 16)  s *= 2;
 *        so a caller sizes the workspace with the same expression (cs_num_compute_units); where it yields 1 the call is the plain one
 *        and `extra` is not read.  Errors (-1): splits > K / 64; `extra` NULL or misaligned where more than one slice runs;
 *        splits != 1 on any other epilogue (or on cs_gemm_nt_ln's folded LayerNorm).
 * flags bit0: use register staging instead of the global_load_lds DMA path; bits 4-7: force a tile schedule (0 = heuristic; 11 = the
 * streaming persistent kernel with register-level epilogues, the default for the bf16 / QuickGELU / SwiGLU epilogues of large problems);
 * bits 20-27: compute units the persistent kernels leave free (0 = use all 256; data-parallel runs reserve a few for RCCL's kernels).
 *
 * THIN FORMS, epi 10 / 11: 1 x 1 convolutions with at most 16 output channels on channel-last rows -- the RPN's rpn_cls | rpn_reg
 * (F-ViT/models/custom_rpn_head.py, mmdet RPNHead: 256 -> 3 and 256 -> 12, one launch for both) and the mask head's conv_logits (mmdet
 * FCNMaskHead: 256 -> 1) -- and their input gradient.  1 <= N <= 16, K % 64 == 0, W = B is bf16 [N, K] (ldb % 8 == 0, 16-byte aligned),
 * splits == 1, flags bit 0 = the K-wide rows (X of epi 10, dX of epi 11) are fp32 instead of bf16; the other flag bits are ignored.
 * M rows are pixels in (image, y, x) order.  `group` selects how the N-wide side is laid out:
 *   group == 0, ROWS:   T[m * ld + n], n < N; columns >= N of a row are never touched.
 *   group == R >= 1, PLANES: M % R == 0 (R = h * w pixels per image) and a split s, 1 <= s <= N.  Column n < s of row m is element
 *                       P1[((m / R) * s + n) * R + m % R], column n >= s is P2[((m / R) * (N - s) + (n - s)) * R + m % R]: two contiguous
 *                       NCHW fp32 tensors [M / R, s, h, w] and [M / R, N - s, h, w]; s == N leaves one tensor and P2 unused.
 *   epi 10, forward:  Y[m, n] = bias[n] + sum_k bf16(X[m, k]) * W[n, k].
 *       A = X rows [M, K], bf16 or fp32 (flags bit 0), row stride lda >= K with 16-byte aligned rows (lda % 8 == 0 / lda % 4 == 0); fp32
 *       values are rounded to bf16 (to nearest even) in registers, so the bits equal cs_cast_f32_bf16 followed by the bf16 form.
 *       bias fp32 [N] or NULL.  fp32 accumulation; the output is fp32, acc + bias, not rounded again.
 *       C = Y: rows form T = C with ld = ldc >= N; planes form P1 = C, P2 = C + M * s (ONE allocation of M * N floats) and ldc = s.
 *       Planes are stored 16 bytes (four pixels) at a time where R % 4 == 0 and C is 16-byte aligned, one element per lane otherwise
 *       (any R >= 1).  `extra` is not read.
 *   epi 11, input gradient:  dX[m, k] = gate(m, k) * sum_n bf16(dY[m, n]) * W[n, k].
 *       A = dY, fp32: rows form T = A with ld = lda >= N; planes form P1 = A, P2 = bias (the two gradients autograd hands are separate
 *       allocations; NULL requires s == N) and lda = s.  dY is rounded to bf16 in registers (operands bf16, accumulation fp32).
 *       C = dX rows [M, K], bf16 or fp32 (flags bit 0), row stride ldc >= K with 16-byte aligned rows; rounded once, at its type.
 *       extra = gate, or NULL: bf16 rows [M, K] with dX's row stride ldc, 16-byte aligned.  Where gate <= 0, dX = 0 (a NaN gate passes,
 *       the ReLU rule of epi 9): the ReLU between the mask head's transposed convolution and conv_logits, for the gate's read alone.
 *   Both: plain vector loads and stores, no atomics, no workspace; every output element is written exactly once per call and nothing
 *   outside the stated extents is touched; 64-bit offsets; a wave owns 16 rows at a time on one v_mfma_f32_16x16x32_bf16 tile (the weights
 *   stay in registers for the whole launch when K == 256) and the grid is min(ceil(M / 64), 8 * compute units) workgroups of 256 threads
 *   with a grid-stride loop: a function of the arguments and the device alone.  Equal inputs give equal bits.
 *   Errors (-1, cs_last_error, nothing launched): N > 16, K % 64 != 0, M % R != 0, s outside [1, N], a stride below its width or one that
 *   breaks the 16-byte rows, misaligned bases, a second block with s == N or none with s < N (epi 11), splits != 1.
 *   epi 12, weight and bias gradient:  dW[n, k] = sum_m bf16(dY[m, n]) * bf16(X[m, k]),  db[n] = sum_m bf16(dY[m, n]),  n < N, k < K.
 *       The contraction is the M rows.  Both operands are bf16 (dY and fp32 X are rounded to nearest even in registers, so the bits equal
 *       those of cs_cast_f32_bf16 followed by the bf16 form), the accumulation is fp32 in a fixed order.
 *       A = dY, fp32, exactly as in epi 11: rows form T = A with ld = lda >= N; planes form P1 = A, P2 = bias (NULL requires s == N) and
 *       lda = s.  B = X rows [M, K], bf16 or fp32 (flags bit 0), row stride ldb >= K with 16-byte aligned rows and base.
 *       C = dW fp32 [N, K], row stride ldc >= K (ldc % 4 == 0, 16-byte aligned): OVERWRITTEN, not accumulated; rows >= N and columns >= K
 *       of a padded buffer are never touched.
 *       extra = fp32 WORKSPACE, 16-byte aligned, of at least
 *           16 + P * (N * K + 16) floats,   P = min(ceil(M / 128), 2 * compute units)     (cs_num_compute_units)
 *       On return extra[0 .. N) holds db and extra[N .. 16) zeros; behind them sit the P per-workgroup partials ([N, K] + 16 floats
 *       each).  The workspace need not be zeroed: every element that is read was written by the same call.
 *       A wave owns 32 rows at a time (staged as bf16 in LDS, read back transposed by ds_read_b64_tr_b16 as the B operand of
 *       v_mfma_f32_16x16x32_bf16, dY^T being the A operand); workgroup b of the P x (K / KC) grid (KC = 256 where K % 256 == 0, else 64;
 *       256 threads) takes the 128-row blocks b, b + P, b + 2 P, ... of column chunk blockIdx.y, adds its four waves' register partials in
 *       wave order through LDS and writes partial b.  A second launch adds the partials: 16 contiguous groups of ceil(P / 16) partials
 *       each in ascending order, then the 16 group sums in ascending order.  With P == 1 the first launch writes dW and db directly.
 *       Rows of the last, ragged 32-row step that lie past M are loaded from row M - 1 and enter as zeros.  Planes are read 32 bytes
 *       (eight pixels) at a time where R % 8 == 0 and both blocks are 16-byte aligned, one element at a time otherwise (any R >= 1).
 *       No atomics; equal inputs give equal bits; 64-bit offsets; nothing outside the stated extents is read or written.
 *       Errors (-1, nothing launched): those of epi 11 with the roles above, a stride below its width or off the 16-byte rows,
 *       misaligned X / dW / workspace, splits != 1.  extra == NULL is refused before anything else, in the words the library used for
 *       code 12 before this form existed ("unknown epilogue 12 ..."): the form exists only with a workspace. */
int cs_gemm_nt(const void* A, const void* B, void* C, const float* bias, const float* extra, int M, int N, int K,
               int lda, int ldb, int ldc, int epi, int splits, int group, int flags, cs_stream_t stream);

/* fp8 operands (BASELINE configs[4] "fp8 MFMA weights"; reference call sites: the F.linear calls of eva_vit_model.py:99-103,177-179,218-219 under
 * src/training/region_clip.py:28-67).  cs_quant_rows_fp8: bf16 [M,K] -> OCP e4m3 [M,Kp] (Kp = K rounded up to 128, padding zero; ldq bytes per
 * row) with one fp32 scale per row (amax/448).  cs_gemm_nt_f8: C = row_scale[m] * col_scale[n] * (A8 . B8^T) + bias (+ extra), contracted
 * with the block-scaled fp8 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4, unit block scales), fp32 accumulate; epi 0 = bf16 out, 2 = fp32 residual. */
int cs_quant_rows_fp8(const void* x_bf16, long ldx, void* q_e4m3, long ldq, float* scale, int M, int K, cs_stream_t stream);
int cs_gemm_nt_f8(const void* A8, const void* B8, void* C, const float* bias, const float* extra, const float* row_scale, const float* col_scale,
                  int M, int N, int K8, int lda, int ldb, int ldc, int epi, int flags, cs_stream_t stream);

/* Weight gradient of a Linear (autograd of F.linear at the call sites above): dW[M,N] (f32, row stride ldc) += A[M,K] . B[N,K]^T with
 * A = dY^T, B = X^T (bf16, contraction = tokens, zero padded to K % 64 == 0).  The K range is split into slices whose partial
 * products go through `workspace` (>= cs_gemm_wgrad_workspace bytes, 16-byte aligned) and one pass adds them into dW. */
size_t cs_gemm_wgrad_workspace(int M, int N, int K);
int cs_gemm_wgrad(const void* A, const void* B, float* dW, void* workspace, int M, int N, int K, int lda, int ldb, int ldc,
                  cs_stream_t stream);

/* The same weight gradient without transposed copies: dW[N,K] (f32) += dY[tokens,N]^T . X[tokens,K], both operands token-major as the
 * backward left them (MFMA operands through the transposing LDS read ds_read_b64_tr_b16).  Any token count; N and K multiples of 8
 * (ragged tiles re-read valid rows / columns, the last token tile's missing tokens are zeroed in the fragments): cs_gemm_wgrad_tn_workspace
 * returns 0 and cs_gemm_wgrad_tn returns 1 (nothing launched) otherwise -- use cs_transpose_bf16 + cs_gemm_wgrad then. */
size_t cs_gemm_wgrad_tn_workspace(int N, int K, int tokens);
int cs_gemm_wgrad_tn(const void* dY, const void* X, float* dW, void* workspace, int N, int K, int tokens, int ldy, int ldx, int ldc,
                     cs_stream_t stream);

/* cs_gemm_nt with a LayerNorm folded in (frozen teacher): the GEMM reads the *un-normalised* bf16 rows, B = gamma (.) W,
 * ln_colsum[n] = sum_k B[n,k], bias = W.beta + b, and the epilogue applies rstd[m] * (acc - mean[m] * ln_colsum[n]) + bias[n]:
 *   epi 6: residual form, C = extra + that value                  (SwiGLU.ffn_ln -> w3 eva_vit_model.py:102-103, inner_attn_ln -> proj :218-219)
 *   epi 0 / 3 with ln_mean != NULL: before the bf16 store / before SiLU*mul   (Block.norm1 -> q|k|v :306,176-179; norm2 -> w1|w2 :307,99-101)
 * and the epilogues can emit what the NEXT folded GEMM needs, so that no LayerNorm pass over the activations is left:
 *   epi 3 with stats_part != NULL: per 32-hidden-unit slice s and row m, (sum, sum of squares) of the rounded outputs at
 *          stats_part[(s*M + m)*2 ..]  (4*ceil(group/128) slices);
 *   epi 2 / 6 with stats_part != NULL: the same per 64-column slice of the fp32 outputs (ceil(N/64) slices); with xb_out != NULL a bf16
 *          copy of the fp32 output (row stride ldxb).  cs_ln_stats_finalize turns the partials into mean/rstd.
 * All other arguments as in cs_gemm_nt. */
int cs_gemm_nt_ln(const void* A, const void* B, void* C, const float* bias, const float* extra, const float* ln_mean,
                  const float* ln_rstd, const float* ln_colsum, float* stats_part, void* xb_out, int ldxb, int M, int N, int K, int lda,
                  int ldb, int ldc, int epi, int splits, int group, int flags, cs_stream_t stream);

/* Epilogue 6 of cs_gemm_nt_ln on the "split stream": the frozen tower's fp32 residual stream x (Block.forward, eva_vit_model.py:306-307:
 * x = x + attn(norm1(x)); x = x + mlp(norm2(x))) kept as two 16-bit planes of the word y = bits(x) + 0x8000:
 *   hi[m, n] = y >> 16     -- x rounded to bf16 (halves away from zero), i.e. the operand the next folded GEMM (norm1 -> q|k|v,
 *                             norm2 -> w1|w2) reads as A, row stride ldxb elements;
 *   lo[m, n] = y & 0xffff  -- the rest; x = bits^-1(((hi << 16) | lo) - 0x8000) exactly.
 * A residual GEMM then moves 8 bytes per stream element (4 in, 4 out) instead of 10 (fp32 in, fp32 out, bf16 copy) and nothing is lost.
 *   x_in  != NULL: the stream is read as fp32 [M, ldc] (first block, after the stem);  NULL: as (hi, lo)
 *   x_out != NULL: it is written as fp32 [M, ldc] (last folded block; hi / lo are only read);  NULL: back to (hi, lo), in place
 *   stats_part: per 64-column slice (sum, sum of squares) of the fp32 outputs as in cs_gemm_nt_ln; required when the stream leaves
 *               split (x_out == NULL), rejected with x_out != NULL.
 * out = x + rstd[m] * (A.B^T - mean[m] * ln_colsum[n]) + bias[n];  N % 32 == 0, K % 64 == 0; hi / lo 16-byte aligned with ldxb % 8 == 0
 * (the planes move in 16-byte pieces); flags bits 20-27 as cs_gemm_nt. */
int cs_gemm_nt_ln_split(const void* A, const void* B, const float* bias, const float* ln_mean, const float* ln_rstd,
                        const float* ln_colsum, const float* x_in, float* x_out, void* hi, void* lo, int ldxb, float* stats_part,
                        int M, int N, int K, int lda, int ldb, int ldc, int flags, cs_stream_t stream);

/* --- LayerNorm(eps, biased var): src/open_clip/eva_clip/transformer.py:52-58 used at eva_vit_model.py:306-307 (norm1/2),
 *     :218 (inner_attn_ln), :102 (ffn_ln), :565/:616 (final norm); replaces apex FusedLayerNorm / F.layer_norm.
 * x_dtype 0=f32 1=bf16; y bf16 (NULL = statistics only); mean/rstd [M] f32 (nullable when no backward is needed).
 * C % 4 != 0 (padded rows, e.g. 2730 hidden units in 2752-wide storage) needs ldx, ldy >= C rounded up to 4.  The kernels move whole 4-element
 * vectors: x, gamma and beta must be READABLE up to roundup4(C), but what columns [C, roundup4(C)) of x / gamma / beta hold is ignored
 * (garbage or NaN there changes no result), and columns [C, roundup4(C)) of y are WRITTEN with exact zeros.  Nothing at or past roundup4(C)
 * is touched. */
int cs_layernorm_fwd(const void* x, int x_dtype, long ldx, const float* gamma, const float* beta, void* y, long ldy,
                     float* mean, float* rstd, int M, int C, float eps, cs_stream_t stream);
/* the same, and the e4m3 copy of y for cs_gemm_nt_f8 (precision amp_fp8, src/training/region_clip.py:28-67 under BASELINE configs[4]):
 * q8 [M, ldq >= C rounded up to 128] bytes with zero padding, q_scale [M] = row amax / 448 -- bit-identical to cs_quant_rows_fp8(y) */
int cs_layernorm_fwd_q8(const void* x, int x_dtype, long ldx, const float* gamma, const float* beta, void* y, long ldy,
                        float* mean, float* rstd, void* q8, long ldq, float* q_scale, int M, int C, float eps, cs_stream_t stream);
/* part [P][M][2] f32 = per-slice (sum, sum of squares) over npp columns each (slices past C ignored) -> LayerNorm mean/rstd [M]
 * of a C-wide row; producers: cs_gemm_nt_ln epi 3 (npp 32) and cs_attn_fwd_stats (npp 64, P = heads). */
int cs_ln_stats_finalize(const float* part, int P, int npp, int C, int M, float eps, float* mean, float* rstd, cs_stream_t stream);
/* f32 in -> f32 out: `ln_pre` of the OpenAI-CLIP ViT (src/open_clip/transformer.py:371,477), whose output is the residual stream */
int cs_layernorm_fwd_f32(const float* x, long ldx, const float* gamma, const float* beta, float* y, long ldy, float* mean, float* rstd,
                         int M, int C, float eps, cs_stream_t stream);
size_t cs_layernorm_bwd_workspace(int M, int C);
/* dx_mode 0: bf16 write, 1: f32 write, 2: f32 accumulate (residual gradient stream).  dgamma/dbeta nullable (frozen).
 * dx_copy (modes 1 / 2, nullable): bf16 copy of the dx rows after the write / accumulate (row stride ldcopy) -- the operand of the next
 * dgrad / wgrad GEMMs -- and copy_colsum[C] (nullable) (+)= its column sums = the bias gradient of the linear layer that feeds this
 * residual branch (autograd of x = x + Linear(..) in Block.forward, eva_vit_model.py:306-307): no cast / column-sum pass of their own. */
/* C % 4 != 0 as in cs_layernorm_fwd (lddy, ldx, lddx, ldcopy >= roundup4(C)): columns [C, roundup4(C)) of dy, x and gamma are read and ignored,
 * the same columns of dx (mode 2 included: they are overwritten, not accumulated) and dx_copy are written with exact zeros; dgamma, dbeta and
 * copy_colsum are C long and nothing past C is written.  `workspace` holds cs_layernorm_bwd_workspace(M, C) bytes. */
int cs_layernorm_bwd(const void* dy, long lddy, const void* x, int x_dtype, long ldx, const float* gamma, const float* mean,
                     const float* rstd, void* dx, int dx_mode, long lddx, float* dgamma, float* dbeta, int accumulate_params,
                     void* workspace, void* dx_copy, long ldcopy, float* copy_colsum, int M, int C, cs_stream_t stream);
/* cs_layernorm_bwd whose bf16 copy also leaves as e4m3 bytes (q8 [M, ldq >= C rounded up to 128], zero padding) + fp32 row scales: the A operand
   of an fp8 dgrad through cs_gemm_nt_f8; bit-identical to cs_quant_rows_fp8(dx_copy).  dx_copy required. */
int cs_layernorm_bwd_q8(const void* dy, long lddy, const void* x, int x_dtype, long ldx, const float* gamma, const float* mean,
                        const float* rstd, void* dx, int dx_mode, long lddx, float* dgamma, float* dbeta, int accumulate_params,
                        void* workspace, void* dx_copy, long ldcopy, float* copy_colsum, void* q8, long ldq, float* q_scale, int M, int C,
                        cs_stream_t stream);

/* --- F.normalize(x, dim=-1) of the dense token map: eva_vit_model.py:620 (eps 1e-12) and its backward. */
int cs_l2norm_fwd(const float* x, float* y, float* inv_norm, int M, int C, float eps, cs_stream_t stream);
int cs_l2norm_bwd(const float* dy, const float* y, const float* inv_norm, void* dx_bf16, int M, int C, cs_stream_t stream);

/* --- attention core: xops.memory_efficient_attention / softmax math branch at eva_vit_model.py:198-243 together with
 *     VisionRotaryEmbeddingFast.forward (src/open_clip/eva_clip/rope.py:148-164) on q,k tokens 1.. ; head dim 64.
 * qkv [B*Ntok, ldqkv] bf16 = q|k|v (bias added, not rotated); cos/sin [(Ntok-1),64] f32; out [B*Ntok, ldo] bf16;
 * lse [B*H, Ntok] f32 (nullable in inference).  The forward kernels read the tables separably, exactly as rope.py:118-142 builds
 * them (Ntok-1 = g*g; dims [0,32) depend on the grid row only, dims [32,64) on the grid column only): row r*g supplies the
 * row part, row c the column part.  The rest of that construction is a precondition too: the row part of grid row i equals the column
 * part of grid column i (both come from the same `freqs` tensor, rope.py:134-138) and the two dims of a rotation pair share their entry
 * (`repeat(..., r = 2)`, :137) -- i.e.
 * cos_t[(i*g)*64 + 2j] == cos_t[(i*g)*64 + 2j+1] == cos_t[i*64 + 32 + 2j], same for sin_t.  Identity tables (cos 1, sin 0: the OpenAI-CLIP
 * family) satisfy it.  The Python wrapper (clipself_amd/hip.py) verifies the tables once per tensor and raises otherwise.
 *
 * cos_t == NULL && sin_t == NULL selects the form WITHOUT ROTARY EMBEDDING (the OpenAI-CLIP ViT family), here and in cs_attn_fwd_stats,
 * cs_attn_cls_fwd and cs_attn_bwd:
 *   - q and k rows reach the products as they are: no tables are read or staged, the backward runs no rotation prepass;
 *   - any Ntok > 1 (nothing needs a square token grid; in cs_attn_bwd every token count runs the same kernels);
 *   - the rounding points do not move: every output equals that of the same call with identity tables (cos 1, sin 0) by value -- the
 *     identity rotation rounds bf16 -> fp32 -> x * 1 - y * 0 -> bf16, which is x again (it can only turn -0.0 into +0.0);
 *   - exactly one of the two being NULL returns -1 with a cs_last_error() text, never a launch. */
int cs_attn_fwd(const void* qkv, const float* cos_t, const float* sin_t, void* out, float* lse, int B, int Ntok, int H,
                int ldqkv, int ldo, float scale, cs_stream_t stream);
/* CLS-query attention for the frozen teacher's last block: VisionTransformer.forward_features returns x[:, 0]
 * (eva_vit_model.py:505-519), so only that query row of the last block is live.  q [B, ldq] bf16 (CLS queries, never rotated);
 * kv [B*Ntok, ldkv] bf16 = k|v; out [B, ldo] bf16.  cos_t == sin_t == NULL: keys are not rotated (see cs_attn_fwd; one NULL is an error). */
int cs_attn_cls_fwd(const void* q, const void* kv, const float* cos_t, const float* sin_t, void* out, int B, int Ntok, int H,
                    int ldq, int ldkv, int ldo, float scale, cs_stream_t stream);
/* Extra query tokens of the OpenAI-CLIP family's mask-attention pooling: VisionTransformer.mask_attn_pool / _mask_attn_pool
 * (src/open_clip/transformer.py:736-834), reached through extract_type='v1' (:660-671) and CLIP.encode_masks(mask_attn=True)
 * (src/open_clip/model.py:245-247).  Q query rows per image attend the image's own keys / values of the same depth: key j of query row r
 * is allowed iff allow[r * Ntok + j] != 0 (the reference's bool attn_mask, inverted; key 0 = the CLS token).  q [B*Q, ldq] bf16;
 * kv [B*Ntok, ldkv] bf16 = k|v; out [B*Q, ldo] bf16.  No rotary embedding in this family.  A row that allows
 * no key at all (the reference always allows key 0) yields a zero output row, not NaN.
 * lse (nullable) [B*H, Q] f32: the natural log-sum-exp of the scaled scores over the allowed keys of each (image, head, query), +inf for a
 * query that allows no key (its probabilities are exactly 0 in the backward).  With lse == NULL the output is bit-identical to the call
 * without it.  Differentiated by cs_attn_bwd's `extra` argument (the reference trains through this path: no no_grad on :659-671,736-834).
 *
 * allow == NULL selects CAUSAL SELF-ATTENTION, the text tower's attention (src/open_clip/model.py:269-281, eva_clip/transformer.py:714-737:
 * the additive triu(-inf) mask): B sequences of Ntok tokens, query row r of sequence b attends keys 0..r of sequence b.
 *   - requires Q == Ntok and lse == NULL (inference only: no log-sum-exp, no backward);
 *   - 1 <= Ntok <= 128 (the `Ntok > 1` rule is the masked form's); Ntok > 128 is an argument error, never a launch;
 *   - q [B*Ntok, ldq], kv [B*Ntok, ldkv] = k|v, out [B*Ntok, ldo], all bf16 -- in practice q and kv are strided views of one
 *     [B*Ntok, 3C] q|k|v matrix (ldq = ldkv = 3C); the same stride and alignment rules as the masked form;
 *   - rounding points of cs_attn_fwd: fp32 scores, exp2 of the scaled difference to the row maximum, P rounded to bf16 before P.V, an fp32
 *     row sum of the unrounded exponentials, one rounding of the output to bf16; row 0 of a sequence is its v row 0 bit for bit;
 *   - bit-reproducible (no atomics); rows past a sequence's end are never read from the next sequence or past the tensors.
 * Every violation returns -1 with a cs_last_error() text. */
int cs_attn_query_fwd(const void* q, const void* kv, const unsigned char* allow, void* out, float* lse, int B, int Q, int Ntok, int H,
                      int ldq, int ldkv, int ldo, float scale, cs_stream_t stream);
/* cs_attn_fwd that also emits stats_part [H][B*Ntok][2] f32 = per head (sum, sum of squares) of each output row's 64 values.
 * cos_t == sin_t == NULL as in cs_attn_fwd. */
int cs_attn_fwd_stats(const void* qkv, const float* cos_t, const float* sin_t, void* out, float* lse, float* stats_part, int B, int Ntok,
                      int H, int ldqkv, int ldo, float scale, cs_stream_t stream);
/* The extra query rows ("passengers") of a cs_attn_bwd launch: the Q rows per image that cs_attn_query_fwd ran against the image's keys /
 * values.  q [B*Q, ldq] bf16; o, dout [B*Q, ldo] bf16 (the forward's output and its gradient); lse [B*H, Q] f32 from the forward;
 * allow [B*Q, Ntok] bytes; dq [B*Q, lddq] bf16 (output).  Per image, head, passenger r and key j, with the rounding points of the image rows:
 *   p = allow ? exp(scale * q_r.k_j - lse_r) : 0,  D_r = sum dO_r * O_r,  dS = bf16(p * (dO_r.v_j - D_r) * scale),
 *   dq_r = sum_j dS * k_j,  dk_j += sum_r dS * q_r,  dv_j += sum_r bf16(p) * dO_r. */
typedef struct cs_attn_extra {
    const void* q;
    const void* o;
    const void* dout;
    const float* lse;
    const unsigned char* allow;
    void* dq;
    int Q, ldq, ldo, lddq;
} cs_attn_extra;
/* Q: extra query rows per image of the launch (0 = none). */
size_t cs_attn_bwd_workspace(int B, int Ntok, int H, int Q);
/* o, dout [B*Ntok, ldo] bf16; lse from cs_attn_fwd; dqkv [B*Ntok, ldqkv] bf16 = d(q|k|v) w.r.t. the un-rotated q, k.
 * extra (nullable): the k|v columns of dqkv then hold the image tokens' own gradient plus the passengers' sums (added once, in fp32, after
 * the image rows' kernels; the q columns are not touched by them) and extra->dq receives the passengers' dq.  With extra, o / dout / lse may
 * all be NULL -- a launch without image rows (the last block of the pooling, whose image-token outputs nobody consumes): dqkv =
 * [0 | passenger dK | passenger dV].  Passengers exist in the family without rotary embedding only: the tables must be the identity then,
 * or both NULL, which means the same.
 * No atomics: bit-reproducible.  extra == NULL: every output is bit-identical to the call without the argument.
 * cos_t == sin_t == NULL (see cs_attn_fwd): no rotation of q / k on load, no inverse rotation of dq / dk, any Ntok > 1, dqkv equal by value
 * to the call with identity tables; one NULL table is an argument error.  cs_attn_bwd_workspace() cannot see the tables and stays an upper
 * bound (the rotated q | k image of long sequences is not written in this form). */
int cs_attn_bwd(const void* qkv, const void* o, const void* dout, const float* lse, const float* cos_t, const float* sin_t,
                void* dqkv, void* workspace, int B, int Ntok, int H, int ldqkv, int ldo, float scale, const cs_attn_extra* extra,
                cs_stream_t stream);

/* --- SwiGLU elementwise: eva_vit_model.py:101  hidden = silu(x1) * x2   (x12 = [x1 | x2], each Hd wide) */
int cs_swiglu_fwd(const void* x12, long ldx, void* h, long ldh, int M, int Hd, cs_stream_t stream);
int cs_swiglu_bwd(const void* dh, long lddh, const void* x12, long ldx, void* dx12, long lddx, int M, int Hd, cs_stream_t stream);
/* the same + colsum[2*Hd] += the column sums of dx12 = the bias gradients of w1 | w2 (autograd of F.linear's bias at eva_vit_model.py:99-100),
   bit-identical to cs_swiglu_bwd followed by cs_colsum_bf16(dx12) without its pass over the matrix; workspace >= cs_colsum_workspace(M, 2*Hd) */
int cs_swiglu_bwd_colsum(const void* dh, long lddh, const void* x12, long ldx, void* dx12, long lddx, float* colsum, void* workspace,
                         int M, int Hd, cs_stream_t stream);
/* the same + the e4m3 copy of dx12 (row-wise amax / 448 scales, bytes [dx1 | dx2 | zero padding to a multiple of 128]) for an fp8 dgrad through
   cs_gemm_nt_f8 -- bit-identical to cs_quant_rows_fp8(dx12), without its pass over the matrix; Hd <= 4096 */
int cs_swiglu_bwd_q8(const void* dh, long lddh, const void* x12, long ldx, void* dx12, long lddx, void* q8, long ldq, float* q_scale,
                     int M, int Hd, cs_stream_t stream);

/* --- GELU / QuickGELU elementwise on bf16 [M,N] (training path keeps the c_fc output): src/open_clip/transformer.py:31-34,211
 *     y = act(x); dx = dy * act'(x); quick 0 = nn.GELU (erf), 1 = x*sigmoid(1.702x).  Every finite bf16 x gives a finite y and, with a
 *     finite dy whose product with act'(x) (|act'| < 1.13) is representable, a finite dx: no intermediate overflows, up to the largest
 *     finite |x| (tests/_pointwise_ref.py runs all 65 280 finite inputs) */
int cs_gelu_fwd(const void* x, long ldx, void* y, long ldy, int M, int N, int quick, cs_stream_t stream);
int cs_gelu_bwd(const void* dy, long lddy, const void* x, long ldx, void* dx, long lddx, int M, int N, int quick, cs_stream_t stream);

/* --- data movement helpers of the step */
int cs_cast_f32_bf16(const float* x, void* y, long n, cs_stream_t stream);
/* form 0 (batch == 1): bf16 in [R, Cc] -> bf16 out[c, r], zero pad r in [R, ld_out).
 * form 1 / 2, the token taps of a detector backbone (F-ViT/models/evaclip_vit.py:117-122 `_expand_x`: x[:, 1:].permute(0, 2, 1).contiguous()
 * .view(-1, width, h, w) of the residual stream after a block): in = fp32 x[batch * (R + 1), ld_in], token-major rows of `batch` images,
 * each with its CLS row first and R = h * w patch rows behind it; out = [batch, Cc, R] contiguous (ld_out == R), fp32 (form 1) or bf16
 * (form 2, round to nearest even): out[b, c, p] = x[b * (R + 1) + 1 + p, c].  Any R >= 1, Cc >= 1, ld_in >= Cc; the CLS rows and the
 * columns [Cc, ld_in) are never read.  16-byte accesses where ld_in % 4 == 0 / R % 4 (fp32) or R % 8 (bf16) == 0 and the pointers are
 * 16-byte aligned, one element per lane otherwise.  Plain loads and stores, no workspace.
 * forms 4 / 5 (the LOW BYTE of `form`), a transposed convolution with kernel == stride == s as a GEMM on token rows (the detector neck,
 * clipself_amd/neck.py): with P = h * w, `off` CLS rows in front of each image's P rows and q = di * s + dj,
 *     nchw[b, c, s*i + di, s*j + dj]  <->  rows[b * (P + off) + off + i*w + j, q * C + c]
 * form 4 copies rows -> nchw (in = rows, ld_in = its stride; out contiguous [batch, C, s*h, s*w], ld_out ignored), form 5 nchw -> rows
 * (in contiguous, ld_in ignored; out = rows, ld_out = its stride) and, with off == 1, writes s*s*C zeros into each image's CLS row so
 * that a weight gradient contracted over all rows is right.  The other bits of `form`: bit 8 = s - 1 (s in {1, 2}), bit 9 = off,
 * bit 10 = element type of the rows (0 fp32, 1 bf16; form 5 writes bf16 only), bit 11 = element type of the NCHW tensor, bits 12-31 =
 * the grid width w.  R = h * w (a multiple of w; h != w is fine), Cc = C, batch = B, any of them >= 1, batch * s <= 65535, rows stride
 * >= s*s*C.  fp32 -> bf16 rounds to nearest even, bf16 -> fp32 is exact.  Form 4 never reads CLS rows or columns past s*s*C, form 5
 * never writes columns past s*s*C.  16-byte accesses on the rows side where the stride and C are multiples of 4 (fp32) / 8 (bf16), on the
 * NCHW side where s*w is, with 16-byte aligned pointers; one element per lane otherwise.  Plain loads and stores, no workspace.
 * forms 7 / 8 (the LOW BYTE of `form`), the top-down step of a feature pyramid on channel-last rows (mmdet FPN.forward:
 * laterals[i - 1] += F.interpolate(laterals[i], mode='nearest'), clipself_amd/fpn.py) and its adjoint.  coarse = rows [batch*h*w, C],
 * fine = rows [batch*2h*2w, C], pixel-major (b, y, x), each map with its own row stride >= C and its own element type; offsets are 64-bit.
 * R = h * w of the COARSE grid (a multiple of w; h != w is fine), Cc = C, batch = B.  The other bits of `form`: bit 8 = 1 (the factor 2 is
 * the only one; 0 returns -1), bit 9 = accumulate (1: `out` is read and added to, 0: `out` is overwritten), bit 10 / 11 = element type of
 * the coarse / fine rows (0 fp32, 1 bf16), bits 12-31 = the coarse grid width w.
 *   form 7, in = coarse (ld_in), out = fine (ld_out): for (di, dj) in {0, 1}^2
 *       out[b, 2i+di, 2j+dj, c] = rnd(acc ? float(out[b, 2i+di, 2j+dj, c]) + float(in[b, i, j, c]) : float(in[b, i, j, c]))
 *   form 8, in = fine (ld_in), out = coarse (ld_out): with f(di, dj) = float(in[b, 2i+di, 2j+dj, c]) and
 *       s = ((f(0,0) + f(0,1)) + f(1,0)) + f(1,1) in fp32, in that order,   out[b, i, j, c] = rnd(acc ? float(out[b, i, j, c]) + s : s)
 * One rounding, at out's type (bf16: to nearest even); bf16 -> fp32 is exact.  Every output element is written exactly once per call and
 * read (bit 9) only by its writer, so form 7 accumulates in place without a race.  Columns >= C of a padded row are never read and never
 * written.  Plain loads and stores, no atomics, no workspace, nothing read back; the grid follows from the arguments and the device's
 * compute-unit count alone (a capped grid-stride stream, 8 workgroups of 256 threads per compute unit at the most).  A thread moves one
 * 16-byte channel group of a coarse pixel and of its four fine pixels -- 8 channels when both maps are bf16, 4 otherwise -- where C and
 * both strides are multiples of that count and both pointers are aligned to their access; one element per lane otherwise (any C >= 1).
 * Returns -1 (nothing launched) for w == 0, R no multiple of w, a stride below C, bit 8 clear, or batch * R * C > 2^31 - 1.
 * Any other form (3, 6, or a low byte above 8) returns -1. */
int cs_transpose_bf16(const void* in, long ld_in, void* out, long ld_out, int R, int Cc, int form, int batch, cs_stream_t stream);
/* `count` such transposes in one launch (the W^T shadows the dgrad GEMMs read are rebuilt after every AdamW step: eva_vit_model.py:99-103,
 * 177-179,218-219 are the linears; 49 matrices per step for B/16).  desc = DEVICE array of 48-byte records
 *   { const void* in; void* out; long ld_in; long ld_out; int R; int Cc; int tile0; int tiles_x; }
 * with tiles_x = ceil(Cc / 64), tile0 = sum over the preceding records of tiles_x * ceil(ld_out / 64); total_tiles = that sum over all. */
int cs_transpose_bf16_batched(const void* desc, int count, int total_tiles, cs_stream_t stream);
size_t cs_colsum_workspace(int M, int N);
int cs_colsum_bf16(const void* x, long ldx, float* out, void* workspace, int M, int N, cs_stream_t stream);   /* out[n] += sum_m x[m,n] (bias grads); fixed summation order, no atomics */
/* PatchEmbed unfold, eva_vit_model.py:355: img [B,3,S,S] f32 / bf16 -> out [B*(S/p)^2, ldo] bf16, row = (c, iy, ix) of one patch.  The WHOLE row
 * is written: columns [3*p*p, ldo) with zeros (the K padding of the patch GEMM, p = 14: 588 -> 640), so ldo is the row's width, not a stride
 * past other data. */
int cs_im2row(const void* img, int img_dtype, void* out, int B, int S, int p, int ldo, cs_stream_t stream);
int cs_cls_row(float* x, const float* cls, const float* pos, int B, int Ntok, int C, cs_stream_t stream);      /* x[b,0,:] = cls + pos[0], :540-543 */

/* --- RoIAlign 1x1 / aligned / adaptive sampling on the token-major map: torchvision.ops.roi_align called at
 *     eva_vit_model.py:628-629 with boxes from _denormalize_boxes :655-664 (boxes given normalised to [0,1]).
 *     feat [B, Ntok, E] f32, the grid in tokens tok_off .. tok_off + grid_h*grid_w - 1; rois [K,5] f32 = (image, x0, y0, x1, y1);
 *     pooled [K, E] f32; E % 4 == 0, grid sides <= 128, K >= 0.
 * Trailing arguments (F-ViT/models/fvit_head.py:63-70,108-119,267-277: the detector's open-vocabulary scoring tail):
 *   box_scale   0 = boxes normalised to [0,1], map coordinate = roi * (grid_w, grid_h) - 0.5.  Otherwise pixel boxes and
 *               map coordinate = __fmul_rn(roi, box_scale) - 0.5 with box_scale = 1 / featmap_stride: torchvision's spatial_scale.
 *   B           image count for the index check, 0 = unchecked.
 *   class_embed [C, E] f32 row-major, 16-byte aligned, or NULL.  Given, the launch also writes
 *                 v^ = v / max(|v|_2, 1e-12);  z_c = vlm_temp * <v^, class_embed[c]>;  lv = z - logsumexp(z)
 *                 scores[k*lds + c] = exp(lv_c)                                              det_logits == NULL
 *                 scores[k*lds + c] = exp((1 - expo[c]) * ld_c + expo[c] * lv_c)             ld = log_softmax(det_logits[k*ldd .. + C))
 *               i.e. softmax(det)^(1-expo) * softmax(z)^expo in the log domain.  fp32 operands and accumulation throughout, no atomics,
 *               fixed summation order (equal inputs, equal bits), no workspace.  pooled may then be NULL; given, it receives v.
 *   With class_embed == NULL, box_scale == 0 and B == 0 the launch is the plain pooling kernel, boxes unchecked.  In every other form
 *   boxes are BOUNDED: one whose image index is outside [0, B) (B > 0), or whose extent on the map is not in (0, 2 * grid side] on both
 *   axes -- non-finite coordinates included -- is an empty box: v = 0, hence a uniform softmax(z); the map is never indexed by it.
 *   Returns -1 (cs_last_error) without launching for C < 1, ldd < C, lds < C, scores == NULL, det_logits without expo, det_logits or
 *   scores without class_embed, pooled == NULL without class_embed, or E + C past one workgroup's LDS (E + C <= 40000 fits). */
int cs_roialign_fwd(const float* feat, const float* rois, float* pooled, int K, int Ntok, int grid_h, int grid_w, int E,
                    int tok_off, float box_scale, int B, const float* class_embed, int C, float vlm_temp, const float* det_logits,
                    long ldd, const float* expo, float* scores, long lds, cs_stream_t stream);
/* backward: dfeat [B, Ntok, E] += the boxes' gradients; a gather per map cell over the image's boxes in ascending box order (no atomics:
 * bit-reproducible, unlike torchvision's atomicAdd scatter); any E: 1024 channels per workgroup, wider maps take more workgroups) */
int cs_roialign_bwd(const float* dpooled, const float* rois, float* dfeat, int K, int B, int Ntok, int grid_h, int grid_w, int E,
                    int tok_off, cs_stream_t stream);

/* --- cosine distillation loss: src/training/clipself.py:42-47.  stats [K,3] f32 workspace kept for the backward. */
int cs_cosine_loss_fwd(const float* student, const float* teacher, float* stats, float* loss, int K, int E, float weight,
                       cs_stream_t stream);
/* upstream: optional device scalar d(total)/d(loss) multiplied in on the device (nullable = 1). */
int cs_cosine_loss_bwd(const float* student, const float* teacher, const float* stats, float* dstudent, int K, int E,
                       float weight, float grad_scale, const float* upstream, cs_stream_t stream);

/* --- RegionCLIP federated BCE over the sampled noun columns: src/training/region_clip.py:47-56
 *     (F.binary_cross_entropy_with_logits(...).sum(-1).mean() on logits * temp; one-hot target at tgt[k], -1 = none).
 * bwd writes d(logits) as bf16 [K, ldd] with zeroed padding columns (operand of the d(features) GEMM): the WHOLE row, columns [ns, ldd)
 * with zeros, so ldd is the row's width, not a stride past other data. */
int cs_fed_bce_fwd(const float* logits, long ldz, const int* tgt, float* rowloss, float* loss, int K, int ns, float temp,
                   float weight, cs_stream_t stream);
int cs_fed_bce_bwd(const float* logits, long ldz, const int* tgt, void* dz_bf16, long ldd, int K, int ns, float temp,
                   float weight, const float* upstream, cs_stream_t stream);

/* --- input pipeline on the GPU: the region crops of GridDistillDataset._obtain_image_crops (src/training/data.py:226-245,
 *     transforms[1] = ResizeMaxSize + ToTensor + Normalize, src/open_clip/transform.py:26-49,93-99) and the det image itself
 *     (ResizeLongest, transform.py:169-191) from ONE decoded RGB image resident in HBM.  Pillow's bicubic resampling (PIL.Image.crop +
 *     Image.resize as reached through torchvision.transforms.functional.resize) is restated bit-exactly: fixed-point coefficients,
 *     horizontal pass then vertical pass, uint8 after each.
 * src [H,W,3] u8; boxes [K,4] f32 pixel (x0,y0,x1,y1), device; mean3/std3: HOST arrays of 3 floats; out [K,3,S,S] f32;
 * pad_center 1 = centred zero padding (crop transform), 0 = right/bottom (det transform); workspace >= cs_crop_resize_workspace bytes. */
size_t cs_crop_resize_workspace(int H, int K, int S);
int cs_crop_resize_u8(const void* src, int H, int W, const float* boxes, int K, int S, int pad_center, const float* mean3,
                      const float* std3, float* out, void* workspace, cs_stream_t stream);

/* --multiscale (src/training/clipself.py:17-27): F.interpolate(images, size=(t, t), mode='bilinear') of the student batch.
 * in [planes,H,W] f32 -> out [planes,Ho,Wo] f32, align_corners=False arithmetic of torch. */
int cs_resize_bilinear_f32(const float* in, float* out, int planes, int H, int W, int Ho, int Wo, cs_stream_t stream);

/* --- sharing one GPU between the two towers of a step.  src/training/clipself.py:36-40 runs the frozen teacher (`dist_model.encode_image`
 * under no_grad) and the student one after the other on one CUDA stream; here the teacher's pass over the NEXT batch runs beside the
 * student's step (src/training/train.py:90-115), each on its own share of the compute units: persistent GEMM grids sized by cs_gemm_nt's
 * flags bits 20-27 and, optionally, queues restricted by a CU mask.  cs_num_compute_units: CUs of the current device (256 on MI355X).
 * cs_stream_create_cu_mask: a stream whose kernels only run on mask bits [first_cu, first_cu + n_cus) (multiples of 8: the driver deals
 * bit i to XCD i % 8, so such a range takes n_cus / 8 CUs from every XCD); destroy it with cs_stream_destroy. */
int cs_num_compute_units(void);
int cs_stream_create_cu_mask(int first_cu, int n_cus, cs_stream_t* out);
int cs_stream_destroy(cs_stream_t stream);

/* --- optimizer: torch.optim.AdamW built at src/training/main.py:198-213, stepped at src/training/train.py:115.
 * Flat fp32 master/grad/moment buffers; flags[n/64]: bit0 = tensor has a gradient this step, bit1 = weight decay applies.
 *
 * guard == NULL: one launch; max_norm and skip_nonfinite are ignored.
 *
 * guard != NULL: gradient norm, clipping (torch.nn.utils.clip_grad_norm_, src/training/train.py:104-113) and the skip of a non-finite step
 * (what GradScaler.step() does for the reference's `amp` precision, train.py:98-115) on the device, in three launches on `stream` and
 * without atomics: the same inputs give the same bits.  guard is a device buffer of CS_ADAMW_GUARD_HEAD + ceil(n / CS_ADAMW_GUARD_SPAN)
 * floats that the caller zeroes once:
 *   guard[0]   overwritten: L2 norm of grad_scale * g over the ACTIVE granules (flag bit0); inactive granules are never loaded, so what
 *              they hold -- NaN included -- does not matter.  Partial k sums elements [k * SPAN, (k + 1) * SPAN) in fp32 in a fixed order
 *              that does not depend on the grid or the device, the partials are added in double: relative error of the norm < 1e-6.
 *   guard[1]   overwritten: clip coefficient min(1, max_norm / (norm + 1e-6)) in fp32, clip_grad_norm_'s arithmetic (a NaN norm gives NaN, as
 *              torch's clamp does); 1 when max_norm <= 0 = clipping off.  max_norm must not be NaN.
 *   guard[2]   overwritten: 1.0 if the update was applied, 0.0 if it was skipped.
 *   guard[3]   read-modify-write by one thread: number of skipped steps so far (+1 on a skip).
 *   guard[4..7] never touched (reserved).
 *   guard[8..] overwritten: the partial sums of squares.
 * Skip: skip_nonfinite (0 or 1) != 0 and the norm is not finite (an Inf or NaN in an active granule, or a sum of squares beyond fp32) ->
 * nothing is written to p, m, v and shadow.  With skip_nonfinite == 0 the arithmetic proceeds whatever the norm is, as clip_grad_norm_
 * (error_if_nonfinite=False) followed by AdamW does.
 * Scale: every gradient element is multiplied once by s = grad_scale * guard[1], formed once in fp32; with a coefficient of 1 every output
 * is bit-identical to the guard == NULL call.
 * `step` is the caller's 1-based count of ATTEMPTED steps: a skipped step still advances the bias-correction index, so that the host
 * never reads the device back.  (GradScaler does not count skipped steps: after k skips the bias corrections here are those of step + k.) */
#define CS_ADAMW_GUARD_HEAD 8
#define CS_ADAMW_GUARD_SPAN 16384
int cs_adamw_step(float* p, const float* g, float* m, float* v, void* shadow_bf16, const uint8_t* flags, long n, float lr,
                  float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, float max_norm,
                  int skip_nonfinite, float* guard, cs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
