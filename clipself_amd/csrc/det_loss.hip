// Detector losses (include/clipself_loss.h): the RPN's and the box head's losses with their gradients, all on the stream, nothing read
// back, no atomics.  DESIGN.md §3.16.
//
//   rpn_loss_kernel        thread = four consecutive cells of one (image, channel) plane of one level's GRADIENT, so the dense writes are
//                          whole 16-byte stores in NCHW order; the [B, N] weights are read with the stride A (4A for the boxes), the
//                          predictions only where the weight is non-zero; one partial sum per workgroup
//   rpn_finish_kernel      workgroup = one (level, loss): adds that loss's partials in a fixed order, divides by avg_factor + eps
//   head_count_kernel      avg_factor == NULL: integer counts of label_weights > 0, one per 4096 rows
//   head_rows_kernel<NPL>  wave = one row of cls_score, held in NPL registers per lane and read once: argmax, max, sum of exponentials,
//                          the row's loss and gradient; lanes 0-3 do the row's four box coordinates
//   head_finish_kernel     one workgroup: the per-row values in a fixed order -> out[4]
//
// Every grid and every order of additions is a function of the host arguments alone.  Labels are compared before they index anything.
#include "det_common.h"
#include "../../include/clipself_loss.h"
#include <float.h>
#include <limits.h>

// This file predates the rule of det_common.h (f_add / f_sub / f_mul / f_div): its __f*_rn expressions may still contract under this pragma,
// and stay as they are because un-fusing them would change result bits.  New detector arithmetic takes the f_* of det_common.h.
#pragma clang fp contract(off)

#define CSL_THREADS 256
#define CSL_COUNT_SPAN 4096        // rows per count partial: at most 256 partials for R = 2^20
#define CSL_HEAD_WAVES 4           // rows per workgroup of head_rows_kernel

namespace {

struct RpnLevelArg {
    const float* cls;
    const float* reg;
    float* dcls;
    float* dreg;
    int hw;            // h * w
    int groups;        // ceil(hw / 4)
    long long off;     // first anchor of the level within N
};
struct RpnArgs {
    RpnLevelArg lv[CSL_MAX_LEVELS];
    unsigned first[2 * CSL_MAX_LEVELS + 1];      // first workgroup of segment 2 * level + kind (kind 0 = cls, 1 = reg); [2L] = the grid
    int L, B, A;
    long long N;
};

}  // namespace

// ------------------------------------------------------------------------------------------------ RPN
__global__ __launch_bounds__(CSL_THREADS) void rpn_loss_kernel(const RpnArgs args, const int* __restrict__ labels, const float* __restrict__ label_weights,
                                                               const float* __restrict__ bbox_targets, const float* __restrict__ bbox_weights,
                                                               const float* __restrict__ avg_factor, float* __restrict__ partials) {
    __shared__ float red[4];
    // the segment of this workgroup: a wave-uniform search over at most 16 entries of the argument block
    int seg = 0;
    for (int s = 1; s < 2 * args.L; ++s)
        if (blockIdx.x >= args.first[s]) seg = s;
    const int level = seg >> 1, kind = seg & 1;
    const RpnLevelArg lv = args.lv[level];
    const int A = args.A;
    const int CA = kind ? 4 * A : A;                                             // channels of this tensor
    const unsigned total = (unsigned)args.B * (unsigned)CA * (unsigned)lv.groups;   // < 2^31 (host check)
    const unsigned idx = (blockIdx.x - args.first[seg]) * CSL_THREADS + threadIdx.x;
    const float den = __fadd_rn(avg_factor[0], FLT_EPSILON);
    float acc = 0.f;
    if (idx < total) {
        const unsigned plane = idx / (unsigned)lv.groups;
        const int g = (int)(idx - plane * (unsigned)lv.groups);
        const int b = (int)(plane / (unsigned)CA), c = (int)(plane - (unsigned)b * (unsigned)CA);
        const int a = kind ? (c >> 2) : c, k = c & 3;
        const int p0 = g * 4;
        const int cnt = min(4, lv.hw - p0);
        const size_t cell = (size_t)plane * (size_t)lv.hw + (size_t)p0;          // element offset inside the level's tensor
        const size_t row0 = (size_t)b * (size_t)args.N + (size_t)lv.off;         // anchor 0 of the level in image b
        const float* __restrict__ pred = (kind ? lv.reg : lv.cls) + cell;
        float gr[4] = {0.f, 0.f, 0.f, 0.f};
        // the four weights (and labels) first, as independent loads: a cell past the plane's end re-reads the group's first cell (always
        // inside the level) and takes the weight 0
        size_t nj[4];
        float wv[4];
        int lb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            nj[j] = row0 + (size_t)(p0 + (j < cnt ? j : 0)) * (size_t)A + (size_t)a;
            const float v = kind ? bbox_weights[nj[j] * 4 + k] : label_weights[nj[j]];
            lb[j] = kind ? 0 : labels[nj[j]];
            wv[j] = j < cnt ? v : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (kind == 0) {
                const float lw = wv[j];
                const int lab = lb[j];
                if (lw != 0.f && (lab == 0 || lab == 1)) {
                    const float x = pred[j];
                    const float t = lab == 0 ? 1.f : 0.f;
                    const float e = expf(-fabsf(x));
                    const float lin = __fsub_rn(fmaxf(x, 0.f), __fmul_rn(x, t));
                    const float bce = __fadd_rn(lin, log1pf(e));
                    acc = __fadd_rn(acc, __fmul_rn(lw, bce));
                    const float ope = __fadd_rn(1.f, e);
                    const float sig = x >= 0.f ? __fdiv_rn(1.f, ope) : __fdiv_rn(e, ope);
                    gr[j] = __fdiv_rn(__fmul_rn(lw, __fsub_rn(sig, t)), den);
                }
            } else {
                const float bw = wv[j];
                if (bw != 0.f) {
                    const float d = __fsub_rn(pred[j], bbox_targets[nj[j] * 4 + k]);
                    acc = __fadd_rn(acc, __fmul_rn(bw, fabsf(d)));
                    const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : d);       // d == 0 gives 0, a NaN stays a NaN
                    gr[j] = __fdiv_rn(__fmul_rn(bw, sg), den);
                }
            }
        }
        float* __restrict__ dst = kind ? lv.dreg : lv.dcls;
        if (dst != nullptr) {
            dst += cell;
            if (cnt == 4 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
                *reinterpret_cast<float4*>(dst) = make_float4(gr[0], gr[1], gr[2], gr[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < cnt) dst[j] = gr[j];
            }
        }
    }
    const float s = block_sum_256(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// grid 2L: workgroup = segment.  Thread t adds partials t, t + 256, ... in ascending order; then the fixed order of block_sum_256.
__global__ __launch_bounds__(CSL_THREADS) void rpn_finish_kernel(const RpnArgs args, const float* __restrict__ partials,
                                                                 const float* __restrict__ avg_factor, float* __restrict__ losses) {
    __shared__ float red[4];
    const unsigned lo = args.first[blockIdx.x], hi = args.first[blockIdx.x + 1];
    float acc = 0.f;
    for (unsigned i = lo + threadIdx.x; i < hi; i += CSL_THREADS) acc = __fadd_rn(acc, partials[i]);
    const float s = block_sum_256(acc, red);
    if (threadIdx.x == 0) losses[blockIdx.x] = __fdiv_rn(s, __fadd_rn(avg_factor[0], FLT_EPSILON));
}

// ------------------------------------------------------------------------------------------------ box head
__global__ __launch_bounds__(CSL_THREADS) void head_count_kernel(const float* __restrict__ label_weights, int R, int* __restrict__ counts) {
    __shared__ int red[4];
    const int base = blockIdx.x * CSL_COUNT_SPAN;
    int n = 0;
    for (int i = threadIdx.x; i < CSL_COUNT_SPAN; i += CSL_THREADS) {
        const int r = base + i;
        if (r < R && label_weights[r] > 0.f) ++n;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// the avg_factor both head kernels use: the caller's, or max(count, 1) from the count partials (integers: exact in any order)
__device__ __forceinline__ float head_avg(const float* __restrict__ avg_factor, const int* __restrict__ counts, int nparts) {
    if (avg_factor != nullptr) return avg_factor[0];
    const int lane = threadIdx.x & 63;
    int n = 0;
    for (int i = lane; i < nparts; i += 64) n += counts[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    return (float)max(n, 1);
}

// grid ceil(R / 4), wave = row.  Lane l holds classes l, l + 64, ..., l + 64 * (NPL - 1); NPL = 1, 2, 4, ..., 64 covers C1 <= 4096.
template <int NPL>
__global__ __launch_bounds__(CSL_THREADS) void head_rows_kernel(const float* __restrict__ cls_score, long ldc, const int* __restrict__ labels,
                                                                const float* __restrict__ label_weights, const float* __restrict__ class_weight,
                                                                const float* __restrict__ bbox_pred, const float* __restrict__ bbox_targets,
                                                                const float* __restrict__ bbox_weights, int R, int C1, int bg_label,
                                                                const float* __restrict__ avg_factor, const int* __restrict__ counts, int nparts,
                                                                float* __restrict__ row_loss, int* __restrict__ row_hit, float* __restrict__ row_l1,
                                                                float* __restrict__ dcls, float* __restrict__ dbbox) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * CSL_HEAD_WAVES + (threadIdx.x >> 6);
    if (r >= R) return;                                                          // wave-uniform; no barrier below
    const float den = __fadd_rn(head_avg(avg_factor, counts, nparts), FLT_EPSILON);
    const int y = labels[r];
    const float lw = label_weights[r];
    const bool y_in = y >= 0 && y < C1;
    const float* __restrict__ row = cls_score + (size_t)r * (size_t)ldc;

    // one read of the row.  A masked class, and a lane's slot past C1, holds -inf and the flag 0
    float x[NPL];
    unsigned long long live = 0ull;                                              // bit j: slot j is an unmasked class
    float best = -INFINITY, xy = 0.f, cwy = 0.f;
    int arg = INT_MAX;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        const int c = j * 64 + lane;
        float v = -INFINITY;
        if (c < C1) {
            const float cw = class_weight != nullptr ? class_weight[c] : 1.f;
            if (!(cw < 1e-5f)) {
                v = row[c];
                live |= 1ull << j;
                if (v > best || (v == best && c < arg)) {
                    best = v;
                    arg = c;
                }
                if (c == y) {
                    xy = v;
                    cwy = cw;
                }
            }
        }
        x[j] = v;
    }
    // the label's logit and class weight from the lane that holds them (0 from a masked or out-of-range label)
    const int ylane = y_in ? (y & 63) : 0;
    xy = __shfl(xy, ylane, 64);
    cwy = __shfl(cwy, ylane, 64);
    const bool y_live = y_in && __shfl((int)((live >> (y_in ? (y >> 6) : 0)) & 1ull), ylane, 64) != 0;
    // argmax across the wave: the larger value, the lower class on a tie
    float m = best;
    int am = arg;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(m, o, 64);
        const int oa = __shfl_xor(am, o, 64);
        if (ov > m || (ov == m && oa < am)) {
            m = ov;
            am = oa;
        }
    }
    const bool valid = lw != 0.f && y_live;                                      // the row takes part in loss_cls
    float s = 0.f;
    if (valid) {
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            if ((live >> j) & 1ull) {
                x[j] = expf(__fsub_rn(x[j], m));
                s = __fadd_rn(s, x[j]);
            }
        }
        s = wave_sum(s);
    }
    if (lane == 0) {
        float lr = 0.f;
        if (valid) lr = __fmul_rn(lw, __fmul_rn(-cwy, __fsub_rn(__fsub_rn(xy, m), logf(s))));
        row_loss[r] = lr;
        row_hit[r] = (y_in && am == y) ? 1 : 0;
    }
    if (dcls != nullptr) {
        float* __restrict__ drow = dcls + (size_t)r * (size_t)ldc;
        const float coef = valid ? __fdiv_rn(__fmul_rn(lw, cwy), den) : 0.f;
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            const int c = j * 64 + lane;
            if (c < C1) {
                float g = 0.f;
                if (valid && ((live >> j) & 1ull)) g = __fmul_rn(coef, __fsub_rn(__fdiv_rn(x[j], s), c == y ? 1.f : 0.f));
                drow[c] = g;
            }
        }
    }
    // the box: lanes 0 - 3 take one coordinate each; the row's sum in the order ((k0 + k1) + k2) + k3
    const bool pos = y >= 0 && y < bg_label;
    float term = 0.f, g = 0.f;
    if (lane < 4 && pos) {
        const float bw = bbox_weights[(size_t)r * 4 + lane];
        if (bw != 0.f) {
            const float d = __fsub_rn(bbox_pred[(size_t)r * 4 + lane], bbox_targets[(size_t)r * 4 + lane]);
            term = __fmul_rn(bw, fabsf(d));
            const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : d);
            g = __fdiv_rn(__fmul_rn(bw, sg), __fadd_rn((float)R, FLT_EPSILON));
        }
    }
    const float t1 = __shfl(term, 1, 64), t2 = __shfl(term, 2, 64), t3 = __shfl(term, 3, 64);
    if (lane == 0) row_l1[r] = __fadd_rn(__fadd_rn(__fadd_rn(term, t1), t2), t3);
    if (dbbox != nullptr && lane < 4) dbbox[(size_t)r * 4 + lane] = g;
}

// one workgroup.  Thread t adds rows t, t + 256, ... in ascending order, then the fixed order of block_sum_256.
__global__ __launch_bounds__(CSL_THREADS) void head_finish_kernel(const float* __restrict__ row_loss, const int* __restrict__ row_hit,
                                                                  const float* __restrict__ row_l1, int R, const float* __restrict__ avg_factor,
                                                                  const int* __restrict__ counts, int nparts, float* __restrict__ out) {
    __shared__ float red[4];
    __shared__ float red2[4];
    __shared__ int redi[4];
    const float avg = head_avg(avg_factor, counts, nparts);
    float sl = 0.f, sb = 0.f;
    int hits = 0;
    for (int r = threadIdx.x; r < R; r += CSL_THREADS) {
        sl = __fadd_rn(sl, row_loss[r]);
        sb = __fadd_rn(sb, row_l1[r]);
        hits += row_hit[r] != 0 ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) hits += __shfl_xor(hits, o, 64);
    if ((threadIdx.x & 63) == 0) redi[threadIdx.x >> 6] = hits;
    const float tl = block_sum_256(sl, red);
    const float tb = block_sum_256(sb, red2);
    if (threadIdx.x == 0) {
        const int h = redi[0] + redi[1] + redi[2] + redi[3];
        out[0] = __fdiv_rn(tl, __fadd_rn(avg, FLT_EPSILON));
        out[1] = R > 0 ? __fdiv_rn(__fmul_rn(100.f, (float)h), (float)R) : 0.f;
        out[2] = __fdiv_rn(tb, __fadd_rn((float)R, FLT_EPSILON));
        out[3] = avg;
    }
}

// ================================================================================================ host
namespace {

// Fills the argument block; false with the last-error text when a level is outside the limits.  levels is host memory.
bool rpn_plan(const char* who, const csl_level* levels, int L, int B, int A, bool need_ptrs, RpnArgs* out) {
    if (!(L >= 1 && L <= CSL_MAX_LEVELS)) { cs_set_error("%s: L = %d must be in [1, %d]", who, L, CSL_MAX_LEVELS); return false; }
    if (levels == nullptr) { cs_set_error("%s: levels must not be NULL", who); return false; }
    if (!(B >= 1 && B <= 65535)) { cs_set_error("%s: B = %d must be in [1, 65535]", who, B); return false; }
    if (!(A >= 1 && A <= CSL_MAX_ANCHORS)) { cs_set_error("%s: A = %d must be in [1, %d]", who, A, CSL_MAX_ANCHORS); return false; }
    RpnArgs a = {};
    a.L = L; a.B = B; a.A = A;
    long long off = 0, blocks = 0;
    int with_grad = 0;
    for (int l = 0; l < L; ++l) {
        const csl_level& v = levels[l];
        if (!(v.h >= 1 && v.h <= CSL_MAX_SIDE && v.w >= 1 && v.w <= CSL_MAX_SIDE)) {
            cs_set_error("%s: level %d: h = %d and w = %d must be in [1, %d]", who, l, v.h, v.w, CSL_MAX_SIDE);
            return false;
        }
        if (need_ptrs) {
            if (v.cls == nullptr || v.reg == nullptr) { cs_set_error("%s: level %d: cls and reg must not be NULL", who, l); return false; }
            if ((v.dcls == nullptr) != (v.dreg == nullptr)) { cs_set_error("%s: level %d: dcls and dreg are given together or both NULL", who, l); return false; }
            with_grad += v.dcls != nullptr;
        }
        const int hw = v.h * v.w, groups = (hw + 3) / 4;
        const long long reg_threads = (long long)B * 4 * A * groups;
        if (reg_threads >= (1ll << 31)) { cs_set_error("%s: level %d: B * 4A * ceil(h * w / 4) = %lld must be below 2^31", who, l, reg_threads); return false; }
        a.lv[l] = RpnLevelArg{v.cls, v.reg, v.dcls, v.dreg, hw, groups, off};
        off += (long long)hw * A;
        a.first[2 * l] = (unsigned)blocks;
        blocks += ((long long)B * A * groups + CSL_THREADS - 1) / CSL_THREADS;
        a.first[2 * l + 1] = (unsigned)blocks;
        blocks += (reg_threads + CSL_THREADS - 1) / CSL_THREADS;
        if (blocks >= (1ll << 31)) { cs_set_error("%s: the levels need %lld workgroups, more than a grid holds", who, blocks); return false; }
    }
    if (need_ptrs && with_grad != 0 && with_grad != L) { cs_set_error("%s: the gradient pointers are given on every level or on none", who); return false; }
    a.first[2 * L] = (unsigned)blocks;
    a.N = off;
    *out = a;
    return true;
}

size_t head_ws(int R) {     // row_loss, row_hit, row_l1, the count partials
    return (size_t)R * 12 + (size_t)((R + CSL_COUNT_SPAN - 1) / CSL_COUNT_SPAN) * 4;
}

template <int NPL>
void launch_head_rows(dim3 grid, hipStream_t st, const float* cls_score, long ldc, const int* labels, const float* label_weights,
                      const float* class_weight, const float* bbox_pred, const float* bbox_targets, const float* bbox_weights, int R, int C1,
                      int bg_label, const float* avg_factor, const int* counts, int nparts, float* row_loss, int* row_hit, float* row_l1,
                      float* dcls, float* dbbox) {
    hipLaunchKernelGGL(head_rows_kernel<NPL>, grid, dim3(CSL_THREADS), 0, st, cls_score, ldc, labels, label_weights, class_weight, bbox_pred,
                       bbox_targets, bbox_weights, R, C1, bg_label, avg_factor, counts, nparts, row_loss, row_hit, row_l1, dcls, dbbox);
}

}  // namespace

extern "C" size_t csl_workspace(const csl_level* levels, int L, int B, int A, int R) {
    if (R < 0 || R > CSL_MAX_ROWS) return 0;
    size_t need = head_ws(R);
    if (L != 0) {
        RpnArgs a;
        if (!rpn_plan("csl_workspace", levels, L, B, A, false, &a)) return 0;
        const size_t rpn = (size_t)a.first[2 * L] * 4;
        need = rpn > need ? rpn : need;
    }
    need = (need + 255) / 256 * 256;
    return need < 256 ? 256 : need;
}

extern "C" int csl_rpn_loss(const csl_level* levels, int L, int B, int A, const int* labels, const float* label_weights,
                            const float* bbox_targets, const float* bbox_weights, const float* avg_factor, float* losses, void* workspace,
                            cs_stream_t stream) {
    RpnArgs a;
    if (!rpn_plan("csl_rpn_loss", levels, L, B, A, true, &a)) return -1;
    CS_CHECK_ARG(labels && label_weights && bbox_targets && bbox_weights, "csl_rpn_loss: the four dense targets must not be NULL");
    CS_CHECK_ARG(avg_factor != nullptr, "csl_rpn_loss: avg_factor (a device fp32 scalar) must not be NULL");
    CS_CHECK_ARG(losses != nullptr, "csl_rpn_loss: losses must not be NULL");
    CS_CHECK_ARG(workspace != nullptr, "csl_rpn_loss: workspace is NULL (csl_workspace() bytes are needed)");
    hipStream_t st = (hipStream_t)stream;
    float* partials = (float*)workspace;
    hipLaunchKernelGGL(rpn_loss_kernel, dim3(a.first[2 * L]), dim3(CSL_THREADS), 0, st, a, labels, label_weights, bbox_targets, bbox_weights,
                       avg_factor, partials);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(rpn_finish_kernel, dim3(2 * L), dim3(CSL_THREADS), 0, st, a, (const float*)partials, avg_factor, losses);
    CS_LAUNCH_CHECK();
    return 0;
}

extern "C" int csl_bbox_head_loss(const float* cls_score, long ldc, const int* labels, const float* label_weights, const float* class_weight,
                                  const float* bbox_pred, const float* bbox_targets, const float* bbox_weights, int R, int C1, int bg_label,
                                  const float* avg_factor, float* out, float* dcls, float* dbbox, void* workspace, cs_stream_t stream) {
    CS_CHECK_ARG(R >= 0 && R <= CSL_MAX_ROWS, "csl_bbox_head_loss: R = %d must be in [0, %d]", R, CSL_MAX_ROWS);
    CS_CHECK_ARG(C1 >= 1 && C1 <= CSL_MAX_CLASSES, "csl_bbox_head_loss: C1 = %d must be in [1, %d]", C1, CSL_MAX_CLASSES);
    CS_CHECK_ARG(ldc >= C1, "csl_bbox_head_loss: ldc = %ld must be >= C1 = %d", ldc, C1);
    CS_CHECK_ARG(R == 0 || (cls_score && labels && label_weights), "csl_bbox_head_loss: cls_score, labels and label_weights must not be NULL");
    CS_CHECK_ARG(R == 0 || (bbox_pred && bbox_targets && bbox_weights), "csl_bbox_head_loss: bbox_pred, bbox_targets and bbox_weights must not be NULL");
    CS_CHECK_ARG(out != nullptr, "csl_bbox_head_loss: out must not be NULL");
    CS_CHECK_ARG(workspace != nullptr, "csl_bbox_head_loss: workspace is NULL (csl_workspace() bytes are needed)");
    hipStream_t st = (hipStream_t)stream;
    float* row_loss = (float*)workspace;
    int* row_hit = (int*)(row_loss + R);
    float* row_l1 = (float*)(row_hit + R);
    int* counts = (int*)(row_l1 + R);
    const int nparts = avg_factor == nullptr ? (R + CSL_COUNT_SPAN - 1) / CSL_COUNT_SPAN : 0;
    if (nparts > 0) {
        hipLaunchKernelGGL(head_count_kernel, dim3(nparts), dim3(CSL_THREADS), 0, st, label_weights, R, counts);
        CS_LAUNCH_CHECK();
    }
    if (R > 0) {
        const dim3 grid((R + CSL_HEAD_WAVES - 1) / CSL_HEAD_WAVES);
        const int per_lane = (C1 + 63) / 64;
#define CSL_ROWS(NPL)                                                                                                                      \
    launch_head_rows<NPL>(grid, st, cls_score, ldc, labels, label_weights, class_weight, bbox_pred, bbox_targets, bbox_weights, R, C1,     \
                          bg_label, avg_factor, counts, nparts, row_loss, row_hit, row_l1, dcls, dbbox)
        if (per_lane <= 1) CSL_ROWS(1);
        else if (per_lane <= 2) CSL_ROWS(2);
        else if (per_lane <= 4) CSL_ROWS(4);
        else if (per_lane <= 8) CSL_ROWS(8);
        else if (per_lane <= 16) CSL_ROWS(16);
        else if (per_lane <= 32) CSL_ROWS(32);
        else CSL_ROWS(64);
#undef CSL_ROWS
        CS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(head_finish_kernel, dim3(1), dim3(CSL_THREADS), 0, st, (const float*)row_loss, (const int*)row_hit, (const float*)row_l1, R,
                       avg_factor, (const int*)counts, nparts, out);
    CS_LAUNCH_CHECK();
    return 0;
}
