// Detector mask branch (include/clipself_mask.h): mask targets, the mask loss with its gradient, the paste of predicted masks.  All on the
// stream, nothing read back, no atomics.  DESIGN.md §3.17.
//
//   mask_target_kernel     workgroup = one (RoI, bin row).  The bilinear weights are separable and the plane is binary, so a bin is
//                          sum_y Wy[y] * (sum_x Wx[x] * m[y, x]) / count: the axis weights are built once in LDS (one thread per bin column,
//                          one for the bin row), the rows of the box are staged in LDS through 4-byte loads where the address allows, and
//                          thread (pw, k) adds the rows k, k + RC, ... of bin column pw
//   mask_count_kernel      integer counts of the counted rows, one per 4096 rows
//   mask_loss_kernel       workgroup = one (row, channel) plane of the GRADIENT (of the picked plane alone in a forward-only call): thread =
//                          groups of four cells, 16-byte stores where the address allows; the picked plane's sum goes to the workspace
//   mask_finish_kernel     one workgroup: the per-row sums in a fixed order -> out[2]
//   paste_kernel           workgroup = one (detection, band of 16 image rows), a contiguous byte range of the output: pixels without a tap
//                          inside the mask are written as 16-byte zero stores; the detection's M * M sigmoids sit in LDS for the rest
//
// Every grid is a function of the host arguments alone.  Labels and ground-truth rows are compared before they index anything.
#include "det_common.h"
#include "../../include/clipself_mask.h"
#include <limits.h>

#pragma clang fp contract(off)

#define CSM_THREADS 256
#define CSM_COUNT_SPAN 4096                                   // rows per count partial: at most 256 partials for R = 2^20
#define CSM_WX_CAP (CSM_MAX_SIDE + 4 * CSM_MAX_MASK)          // M * (grid + 2) <= W + 4 M floats of x weights
#define CSM_STAGE_ROWS 8
#define CSM_STAGE_LD (CSM_MAX_SIDE + 16)                      // bytes per staged row: W columns + the 3 bytes of misalignment, a multiple of 4
#define CSM_BAND 16                                           // image rows per workgroup of paste_kernel

namespace {

__device__ __forceinline__ bool finite4(float a, float b, float c, float d) { return isfinite(a) && isfinite(b) && isfinite(c) && isfinite(d); }

// The weights of bin p of one axis onto the pixels base .. base + span - 1 (w, zeroed by the caller): the header's samples in ascending
// order, lo before hi.  grid <= size + 1 (checked by the caller), so the trip count is bounded by a host argument.
__device__ void build_axis(float start, float bin, int grid, int p, int size, float* w, int span, int* base_out) {
    int base = -1;
    const float origin = f_add(start, f_mul((float)p, bin));
    for (int i = 0; i < grid; ++i) {
        float c = f_add(origin, f_div(f_mul(f_add((float)i, 0.5f), bin), (float)grid));
        if (!(c >= -1.f && c <= (float)size)) continue;
        if (c <= 0.f) c = 0.f;
        int lo = (int)c, hi;
        if (lo >= size - 1) {
            lo = hi = size - 1;
            c = (float)lo;
        } else {
            hi = lo + 1;
        }
        const float l = f_sub(c, (float)lo), h = f_sub(1.f, l);
        if (base < 0) base = lo;
        const int a = lo - base, b = hi - base;
        if (a >= 0 && a < span) w[a] = f_add(w[a], h);
        if (b >= 0 && b < span) w[b] = f_add(w[b], l);
    }
    *base_out = base < 0 ? 0 : base;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ mask targets
// grid R * M: workgroup = (r, ph)
__global__ __launch_bounds__(CSM_THREADS) void mask_target_kernel(const float* __restrict__ rois, const int* __restrict__ gt_rows,
                                                                  const unsigned char* __restrict__ masks, int Gtot, int H, int W, long ldm,
                                                                  long plane, int M, int soft, void* __restrict__ targets) {
    __shared__ float Wx[CSM_WX_CAP];
    __shared__ float Wy[CSM_MAX_SIDE + 8];
    __shared__ __attribute__((aligned(16))) unsigned char stage[CSM_STAGE_ROWS * CSM_STAGE_LD];
    __shared__ float part[CSM_STAGE_ROWS * CSM_MAX_MASK];
    __shared__ int bx[CSM_MAX_MASK];
    __shared__ int by;
    const int tid = threadIdx.x;
    const int r = blockIdx.x / M, ph = blockIdx.x - r * M;
    const size_t out0 = ((size_t)r * M + ph) * M;

    // geometry, the same in every thread
    const int g = gt_rows[r];
    float x0 = rois[(size_t)r * 5 + 1], y0 = rois[(size_t)r * 5 + 2], x1 = rois[(size_t)r * 5 + 3], y1 = rois[(size_t)r * 5 + 4];
    bool ok = g >= 0 && g < Gtot && finite4(x0, y0, x1, y1);
    x0 = fminf(fmaxf(x0, 0.f), (float)W);
    x1 = fminf(fmaxf(x1, 0.f), (float)W);
    y0 = fminf(fmaxf(y0, 0.f), (float)H);
    y1 = fminf(fmaxf(y1, 0.f), (float)H);
    const float sx = f_sub(x0, 0.5f), sy = f_sub(y0, 0.5f);
    const float bw = f_div(f_sub(f_sub(x1, 0.5f), sx), (float)M), bh = f_div(f_sub(f_sub(y1, 0.5f), sy), (float)M);
    int gw = 0, gh = 0;
    if (ok) {                                                                    // finite and at most side + 1: the casts are safe
        gw = (int)ceilf(bw);
        gh = (int)ceilf(bh);
    }
    ok = ok && gw >= 1 && gh >= 1 && gw <= W + 1 && gh <= H + 1 && M * (gw + 2) <= CSM_WX_CAP;
    if (!ok) {                                                                   // workgroup-uniform: no barrier was passed
        if (tid < M) {
            if (soft) ((float*)targets)[out0 + tid] = 0.f;
            else ((unsigned char*)targets)[out0 + tid] = 0;
        }
        return;
    }
    const int SPX = gw + 2, SPY = gh + 2;
    for (int i = tid; i < M * SPX; i += CSM_THREADS) Wx[i] = 0.f;
    for (int i = tid; i < SPY; i += CSM_THREADS) Wy[i] = 0.f;
    __syncthreads();
    if (tid < M) build_axis(sx, bw, gw, tid, W, &Wx[tid * SPX], SPX, &bx[tid]);
    else if (tid == CSM_MAX_MASK) build_axis(sy, bh, gh, ph, H, Wy, SPY, &by);
    __syncthreads();

    int xmin = INT_MAX, xmax = 0;
    for (int p = 0; p < M; ++p) {
        xmin = min(xmin, bx[p]);
        xmax = max(xmax, bx[p] + SPX - 1);
    }
    xmax = min(xmax, W - 1);
    const int ncol = xmax - xmin + 1;                                            // 1 .. W
    const int wpr = (ncol + 6) / 4;                                              // 4-byte words of a staged row, misalignment included
    const int RC = min(CSM_THREADS / M, CSM_STAGE_ROWS);
    const int pw = tid % M, ys = tid / M;
    const bool act = ys < RC;
    const int mybase = bx[pw];
    const int jmax = act ? min(SPX, W - mybase) : 0;
    const unsigned char* __restrict__ pl = masks + (size_t)g * (size_t)plane;
    const int ybase = by;
    float acc = 0.f;
    for (int yb = 0; yb < SPY; yb += RC) {
        const int nr = min(RC, SPY - yb);
        for (int idx = tid; idx < nr * wpr; idx += CSM_THREADS) {
            const int k = idx / wpr, i = idx - k * wpr;
            const int y = ybase + yb + k;
            if (y >= H) continue;                                                // slack of the span: its weights are 0
            const unsigned char* src = pl + (size_t)y * (size_t)ldm + xmin;
            const int off = (int)(reinterpret_cast<uintptr_t>(src) & 3);
            const int first = 4 * i - off;                                       // column (relative to xmin) of the word's first byte
            unsigned char* dst = stage + k * CSM_STAGE_LD + 4 * i;
            if (first >= 0 && first + 3 < ncol) {
                *reinterpret_cast<uint32_t*>(dst) = *reinterpret_cast<const uint32_t*>(src + first);
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int q = first + b;
                    if (q >= 0 && q < ncol) dst[b] = src[q];
                }
            }
        }
        __syncthreads();
        if (act && ys < nr) {
            const int y = ybase + yb + ys;
            const float wy = Wy[yb + ys];
            if (y < H && wy != 0.f) {
                const int off = (int)(reinterpret_cast<uintptr_t>(pl + (size_t)y * (size_t)ldm + xmin) & 3);
                const unsigned char* s = stage + ys * CSM_STAGE_LD + (mybase - xmin) + off;
                const float* wx = &Wx[pw * SPX];
                float rs = 0.f;
                for (int j = 0; j < jmax; ++j)
                    if (s[j] != 0) rs = f_add(rs, wx[j]);
                acc = f_add(acc, f_mul(wy, rs));
            }
        }
        __syncthreads();
    }
    if (act) part[ys * CSM_MAX_MASK + pw] = acc;
    __syncthreads();
    if (tid < M) {
        float s = 0.f;
        for (int k = 0; k < RC; ++k) s = f_add(s, part[k * CSM_MAX_MASK + tid]);
        const float t = f_div(s, (float)max(gh * gw, 1));
        if (soft) ((float*)targets)[out0 + tid] = t;
        else ((unsigned char*)targets)[out0 + tid] = t >= 0.5f ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ mask loss
__device__ __forceinline__ bool row_counted(const int* __restrict__ labels, const float* __restrict__ row_weights, int r, int C, int* lab) {
    const int l = labels != nullptr ? labels[r] : 0;
    *lab = l;
    return row_weights[r] > 0.f && l >= 0 && l < C;
}

__global__ __launch_bounds__(CSM_THREADS) void mask_count_kernel(const int* __restrict__ labels, const float* __restrict__ row_weights, int R,
                                                                 int C, int* __restrict__ counts) {
    __shared__ int red[4];
    const int base = blockIdx.x * CSM_COUNT_SPAN;
    int n = 0, lab;
    for (int i = threadIdx.x; i < CSM_COUNT_SPAN; i += CSM_THREADS) {
        const int r = base + i;
        if (r < R && row_counted(labels, row_weights, r, C, &lab)) ++n;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// n = max(count, 1) from the count partials (integers: exact in any order), the same in every lane
__device__ __forceinline__ int mask_n(const int* __restrict__ counts, int nparts) {
    const int lane = threadIdx.x & 63;
    int n = 0;
    for (int i = lane; i < nparts; i += 64) n += counts[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    return max(n, 1);
}

// dpred != NULL: grid R * C, workgroup = plane (r, c).  dpred == NULL: grid R, workgroup = the picked plane of row r.
__global__ __launch_bounds__(CSM_THREADS) void mask_loss_kernel(const float* __restrict__ pred, const int* __restrict__ labels,
                                                                const void* __restrict__ targets, int soft, const float* __restrict__ row_weights,
                                                                int C, int MM, const int* __restrict__ counts, int nparts,
                                                                float* __restrict__ row_sum, float* __restrict__ dpred) {
    __shared__ float red[4];
    int r, c, lab;
    if (dpred != nullptr) {
        r = (int)(blockIdx.x / (unsigned)C);
        c = (int)(blockIdx.x - (unsigned)r * (unsigned)C);
    } else {
        r = (int)blockIdx.x;
        c = -1;
    }
    const bool counted = row_counted(labels, row_weights, r, C, &lab);
    if (dpred == nullptr) {
        if (!counted) return;                                                    // workgroup-uniform, before any barrier
        c = lab;
    }
    const bool picked = counted && c == lab;
    const float w = picked ? row_weights[r] : 0.f;
    const float den = f_mul((float)mask_n(counts, nparts), (float)MM);
    const size_t p0 = ((size_t)r * (size_t)C + (size_t)c) * (size_t)MM;          // < 2^31 elements (host check)
    const size_t t0 = (size_t)r * (size_t)MM;
    const int groups = (MM + 3) / 4;
    float acc = 0.f;
    for (int g = threadIdx.x; g < groups; g += CSM_THREADS) {
        const int e0 = g * 4, cnt = min(4, MM - e0);
        float gr[4] = {0.f, 0.f, 0.f, 0.f};
        if (picked) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < cnt) {
                    const float x = pred[p0 + e0 + j];
                    const float t = soft ? ((const float*)targets)[t0 + e0 + j] : (((const unsigned char*)targets)[t0 + e0 + j] != 0 ? 1.f : 0.f);
                    const float e = expf(-fabsf(x));
                    const float lin = f_sub(fmaxf(x, 0.f), f_mul(x, t));
                    const float bce = f_add(lin, log1pf(e));
                    acc = f_add(acc, f_mul(w, bce));
                    const float ope = f_add(1.f, e);
                    const float sig = x >= 0.f ? f_div(1.f, ope) : f_div(e, ope);
                    gr[j] = f_div(f_mul(w, f_sub(sig, t)), den);
                }
            }
        }
        if (dpred != nullptr) {
            float* __restrict__ dst = dpred + p0 + e0;
            if (cnt == 4 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
                *reinterpret_cast<float4*>(dst) = make_float4(gr[0], gr[1], gr[2], gr[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < cnt) dst[j] = gr[j];
            }
        }
    }
    if (picked) {                                                                // workgroup-uniform
        const float s = block_sum_256(acc, red);
        if (threadIdx.x == 0) row_sum[r] = s;
    }
}

// one workgroup.  Thread t adds the counted rows t, t + 256, ... in ascending order, then the fixed order of block_sum_256.
__global__ __launch_bounds__(CSM_THREADS) void mask_finish_kernel(const int* __restrict__ labels, const float* __restrict__ row_weights, int R, int C,
                                                                  int MM, const int* __restrict__ counts, int nparts,
                                                                  const float* __restrict__ row_sum, float* __restrict__ out) {
    __shared__ float red[4];
    const int n = mask_n(counts, nparts);
    float acc = 0.f;
    int lab;
    for (int r = threadIdx.x; r < R; r += CSM_THREADS)
        if (row_counted(labels, row_weights, r, C, &lab)) acc = f_add(acc, row_sum[r]);
    const float s = block_sum_256(acc, red);
    if (threadIdx.x == 0) {
        out[0] = f_div(s, f_mul((float)n, (float)MM));
        out[1] = (float)n;
    }
}

// ------------------------------------------------------------------------------------------------ paste
// torch's grid_sample coordinate of output pixel X (align_corners=False), op for op
__device__ __forceinline__ float paste_coord(int X, float lo, float extent, float Mf) {
    const float gx = f_sub(f_mul(f_div(f_sub(f_add((float)X, 0.5f), lo), extent), 2.f), 1.f);
    return f_div(f_sub(f_mul(f_add(gx, 1.f), Mf), 1.f), 2.f);
}

// grid N * ceil(img_h / 16): workgroup = (detection, band)
__global__ __launch_bounds__(CSM_THREADS) void paste_kernel(const float* __restrict__ logits, const int* __restrict__ labels,
                                                            const float* __restrict__ boxes, int C, int M, int img_h, int img_w, float thr,
                                                            unsigned char* __restrict__ out, float* __restrict__ soft) {
    __shared__ float p[CSM_MAX_MASK * CSM_MAX_MASK];
    __shared__ float iy_s[CSM_BAND];
    __shared__ int rowlive[CSM_BAND];
    __shared__ int red_lo[4], red_hi[4];
    const int tid = threadIdx.x;
    const int nb = (img_h + CSM_BAND - 1) / CSM_BAND;
    const int n = (int)(blockIdx.x / (unsigned)nb), band = (int)(blockIdx.x - (unsigned)n * (unsigned)nb);
    const int Y0 = band * CSM_BAND, Y1 = min(Y0 + CSM_BAND, img_h);
    const int lab = labels != nullptr ? labels[n] : 0;
    const float x0 = boxes[(size_t)n * 4], y0 = boxes[(size_t)n * 4 + 1], x1 = boxes[(size_t)n * 4 + 2], y1 = boxes[(size_t)n * 4 + 3];
    const float dx = f_sub(x1, x0), dy = f_sub(y1, y0);
    const bool ok = lab >= 0 && lab < C && finite4(x0, y0, x1, y1) && isfinite(dx) && isfinite(dy) && dx > 0.f && dy > 0.f;
    const float Mf = (float)M;

    int rl = 0;
    if (ok && tid < CSM_BAND) {
        const float iy = paste_coord(Y0 + tid, y0, dy, Mf);
        rl = (Y0 + tid < Y1 && iy >= -1.f && iy < Mf) ? 1 : 0;
        iy_s[tid] = iy;
        rowlive[tid] = rl;
    }
    const bool any_row = __syncthreads_or(rl) != 0;                               // also publishes iy_s / rowlive
    int xa = img_w, xb = 0;                                                       // the live columns lie in [xa, xb)
    if (any_row) {                                                               // workgroup-uniform
        for (int X = tid; X < img_w; X += CSM_THREADS) {
            const float ix = paste_coord(X, x0, dx, Mf);
            if (ix >= -1.f && ix < Mf) {
                xa = min(xa, X);
                xb = max(xb, X + 1);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            xa = min(xa, __shfl_xor(xa, o, 64));
            xb = max(xb, __shfl_xor(xb, o, 64));
        }
        if ((tid & 63) == 0) {
            red_lo[tid >> 6] = xa;
            red_hi[tid >> 6] = xb;
        }
        const float* __restrict__ src = logits + ((size_t)n * (size_t)C + (size_t)lab) * (size_t)(M * M);
        for (int i = tid; i < M * M; i += CSM_THREADS) {
            const float x = src[i];
            const float e = expf(-fabsf(x));
            const float ope = f_add(1.f, e);
            p[i] = x >= 0.f ? f_div(1.f, ope) : f_div(e, ope);
        }
        __syncthreads();
        xa = min(min(red_lo[0], red_lo[1]), min(red_lo[2], red_lo[3]));
        xb = max(max(red_hi[0], red_hi[1]), max(red_hi[2], red_hi[3]));
    }

    // the band is one contiguous byte range of out: 16-byte chunks counted from the 16-byte boundary at or before its first byte
    const size_t base = ((size_t)n * (size_t)img_h + (size_t)Y0) * (size_t)img_w;
    const int len = (Y1 - Y0) * img_w;                                           // <= 16 * 16384
    unsigned char* __restrict__ o = out + base;
    float* __restrict__ so = soft != nullptr ? soft + base : nullptr;
    const int a0 = (int)(reinterpret_cast<uintptr_t>(o) & 15);
    const int nchunks = (a0 + len + 15) / 16;
    for (int k = tid; k < nchunks; k += CSM_THREADS) {
        const int lo = max(16 * k - a0, 0), hi = min(16 * k - a0 + 16, len);
        int Y = lo / img_w, X = lo - Y * img_w;                                   // row inside the band, column
        const bool one_row = X + (hi - lo) <= img_w;
        const bool dead = !any_row || (one_row && (rowlive[Y] == 0 || X + (hi - lo) <= xa || X >= xb));
        if (dead) {
            if (hi - lo == 16) {
                *reinterpret_cast<uint4*>(o + lo) = make_uint4(0u, 0u, 0u, 0u);
            } else {
                for (int q = lo; q < hi; ++q) o[q] = 0;
            }
            if (so != nullptr)
                for (int q = lo; q < hi; ++q) so[q] = 0.f;
            continue;
        }
        unsigned long long b0 = 0ull, b1 = 0ull;                                  // the chunk's 16 bytes, in registers
        for (int q = lo; q < hi; ++q) {
            float v = 0.f;
            if (rowlive[Y] != 0) {
                const float iy = iy_s[Y];
                const float ix = paste_coord(X, x0, dx, Mf);
                if (ix >= -1.f && ix < Mf) {
                    const float fx = floorf(ix), fy = floorf(iy);
                    const int xi = (int)fx, yi = (int)fy;                       // in [-1, M - 1]
                    const float wx1 = f_sub(ix, fx), wx0 = f_sub(f_add(fx, 1.f), ix);
                    const float wy1 = f_sub(iy, fy), wy0 = f_sub(f_add(fy, 1.f), iy);
                    if (yi >= 0 && xi >= 0) v = f_add(v, f_mul(f_mul(wx0, wy0), p[yi * M + xi]));
                    if (yi >= 0 && xi + 1 < M) v = f_add(v, f_mul(f_mul(wx1, wy0), p[yi * M + xi + 1]));
                    if (yi + 1 < M && xi >= 0) v = f_add(v, f_mul(f_mul(wx0, wy1), p[(yi + 1) * M + xi]));
                    if (yi + 1 < M && xi + 1 < M) v = f_add(v, f_mul(f_mul(wx1, wy1), p[(yi + 1) * M + xi + 1]));
                }
            }
            const unsigned long long bit = v >= thr ? 1ull : 0ull;
            const int sh = (q - lo) * 8;
            if (sh < 64) b0 |= bit << sh;
            else b1 |= bit << (sh - 64);
            if (so != nullptr) so[q] = v;
            if (++X == img_w) {
                X = 0;
                ++Y;
            }
        }
        if (hi - lo == 16) {
            *reinterpret_cast<uint4*>(o + lo) = make_uint4((unsigned)b0, (unsigned)(b0 >> 32), (unsigned)b1, (unsigned)(b1 >> 32));
        } else {
            for (int q = lo; q < hi; ++q) {
                const int sh = (q - lo) * 8;
                o[q] = (unsigned char)(((sh < 64 ? b0 >> sh : b1 >> (sh - 64))) & 1ull);
            }
        }
    }
}

// ================================================================================================ host
namespace {

size_t loss_ws(int R) {     // row_sum, the count partials
    return (size_t)R * 4 + (size_t)((R + CSM_COUNT_SPAN - 1) / CSM_COUNT_SPAN) * 4;
}

}  // namespace

extern "C" size_t csm_workspace(int R) {
    if (R < 0 || R > CSM_MAX_ROWS) return 0;
    const size_t need = (loss_ws(R) + 255) / 256 * 256;
    return need < 256 ? 256 : need;
}

extern "C" int csm_mask_target(const float* rois, const int* gt_rows, int R, const unsigned char* masks, int Gtot, int H, int W, long ldm,
                               long plane, int M, int soft, void* targets, cs_stream_t stream) {
    CS_CHECK_ARG(R >= 0 && R <= CSM_MAX_ROWS, "csm_mask_target: R = %d must be in [0, %d]", R, CSM_MAX_ROWS);
    CS_CHECK_ARG(Gtot >= 0 && Gtot <= CSM_MAX_GT, "csm_mask_target: Gtot = %d must be in [0, %d]", Gtot, CSM_MAX_GT);
    CS_CHECK_ARG(H >= 1 && H <= CSM_MAX_SIDE && W >= 1 && W <= CSM_MAX_SIDE, "csm_mask_target: H = %d and W = %d must be in [1, %d]", H, W, CSM_MAX_SIDE);
    CS_CHECK_ARG(ldm >= W, "csm_mask_target: ldm = %ld must be >= W = %d", ldm, W);
    CS_CHECK_ARG(plane >= (long)H * ldm, "csm_mask_target: plane = %ld must be >= H * ldm = %ld", plane, (long)H * ldm);
    CS_CHECK_ARG(M >= 1 && M <= CSM_MAX_MASK, "csm_mask_target: M = %d must be in [1, %d]", M, CSM_MAX_MASK);
    CS_CHECK_ARG(R == 0 || (rois && gt_rows && targets), "csm_mask_target: rois, gt_rows and targets must not be NULL");
    CS_CHECK_ARG(R == 0 || Gtot == 0 || masks, "csm_mask_target: masks must not be NULL");
    if (R == 0) return 0;
    hipLaunchKernelGGL(mask_target_kernel, dim3((unsigned)R * (unsigned)M), dim3(CSM_THREADS), 0, (hipStream_t)stream, rois, gt_rows, masks, Gtot, H,
                       W, ldm, plane, M, soft != 0 ? 1 : 0, targets);
    CS_LAUNCH_CHECK();
    return 0;
}

extern "C" int csm_mask_loss(const float* pred, const int* labels, const void* targets, int soft, const float* row_weights, int R, int C, int M,
                             float* out, float* dpred, void* workspace, cs_stream_t stream) {
    CS_CHECK_ARG(R >= 0 && R <= CSM_MAX_ROWS, "csm_mask_loss: R = %d must be in [0, %d]", R, CSM_MAX_ROWS);
    CS_CHECK_ARG(C >= 1 && C <= CSM_MAX_CLASSES, "csm_mask_loss: C = %d must be in [1, %d]", C, CSM_MAX_CLASSES);
    CS_CHECK_ARG(M >= 1 && M <= CSM_MAX_MASK, "csm_mask_loss: M = %d must be in [1, %d]", M, CSM_MAX_MASK);
    const long long total = (long long)R * C * M * M;
    CS_CHECK_ARG(total < (1ll << 31), "csm_mask_loss: R * C * M * M = %lld must be below 2^31", total);
    CS_CHECK_ARG(R == 0 || (pred && targets && row_weights), "csm_mask_loss: pred, targets and row_weights must not be NULL");
    CS_CHECK_ARG(out != nullptr, "csm_mask_loss: out must not be NULL");
    CS_CHECK_ARG(workspace != nullptr, "csm_mask_loss: workspace is NULL (csm_workspace() bytes are needed)");
    hipStream_t st = (hipStream_t)stream;
    float* row_sum = (float*)workspace;
    int* counts = (int*)(row_sum + R);
    const int nparts = (R + CSM_COUNT_SPAN - 1) / CSM_COUNT_SPAN;
    const int MM = M * M;
    if (R > 0) {
        hipLaunchKernelGGL(mask_count_kernel, dim3(nparts), dim3(CSM_THREADS), 0, st, labels, row_weights, R, C, counts);
        CS_LAUNCH_CHECK();
        const unsigned grid = dpred != nullptr ? (unsigned)R * (unsigned)C : (unsigned)R;
        hipLaunchKernelGGL(mask_loss_kernel, dim3(grid), dim3(CSM_THREADS), 0, st, pred, labels, targets, soft != 0 ? 1 : 0, row_weights, C, MM,
                           (const int*)counts, nparts, row_sum, dpred);
        CS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(mask_finish_kernel, dim3(1), dim3(CSM_THREADS), 0, st, labels, row_weights, R, C, MM, (const int*)counts, nparts,
                       (const float*)row_sum, out);
    CS_LAUNCH_CHECK();
    return 0;
}

extern "C" int csm_paste_masks(const float* logits, const int* labels, const float* boxes, int N, int C, int M, int img_h, int img_w, float thr,
                               unsigned char* out, float* soft, cs_stream_t stream) {
    CS_CHECK_ARG(N >= 0 && N <= CSM_MAX_ROWS, "csm_paste_masks: N = %d must be in [0, %d]", N, CSM_MAX_ROWS);
    CS_CHECK_ARG(C >= 1 && C <= CSM_MAX_CLASSES, "csm_paste_masks: C = %d must be in [1, %d]", C, CSM_MAX_CLASSES);
    CS_CHECK_ARG(M >= 1 && M <= CSM_MAX_MASK, "csm_paste_masks: M = %d must be in [1, %d]", M, CSM_MAX_MASK);
    const long long total = (long long)N * C * M * M;
    CS_CHECK_ARG(total < (1ll << 31), "csm_paste_masks: N * C * M * M = %lld must be below 2^31", total);
    CS_CHECK_ARG(img_h >= 1 && img_h <= CSM_MAX_IMAGE && img_w >= 1 && img_w <= CSM_MAX_IMAGE,
                 "csm_paste_masks: img_h = %d and img_w = %d must be in [1, %d]", img_h, img_w, CSM_MAX_IMAGE);
    CS_CHECK_ARG(thr >= 0.f, "csm_paste_masks: thr = %g must be >= 0 (mmdet's soft 0 - 255 bytes are not implemented)", (double)thr);
    const long long blocks = (long long)N * ((img_h + CSM_BAND - 1) / CSM_BAND);
    CS_CHECK_ARG(blocks < (1ll << 31), "csm_paste_masks: N * ceil(img_h / %d) = %lld must be below 2^31", CSM_BAND, blocks);
    CS_CHECK_ARG(N == 0 || (logits && boxes && out), "csm_paste_masks: logits, boxes and out must not be NULL");
    if (N == 0) return 0;
    hipLaunchKernelGGL(paste_kernel, dim3((unsigned)blocks), dim3(CSM_THREADS), 0, (hipStream_t)stream, logits, labels, boxes, C, M, img_h, img_w, thr,
                       out, soft);
    CS_LAUNCH_CHECK();
    return 0;
}
