// Shared device helpers of the detector kernels (det_post, det_assign, det_loss, det_mask, det_proposal, roi_extract): rounded fp32
// arithmetic, box area, the image-range clamp, the order-preserving float key, the u64 bitonic sort, the fixed-order workgroup sums and
// mmdet's DeltaXYWHBBoxCoder.  DESIGN.md §3.19.
#pragma once
#include "cs_common.h"
#include <math.h>

typedef unsigned long long u64;

// ---- "every operation rounded on its own" ------------------------------------------------------
// THE RULE: detector arithmetic that a header under include/ states operation by operation is written with these four and nothing
// else.  Each body is compiled with contraction off, so its result carries no permission to contract and the backend cannot fuse a
// product into a following sum, whatever the including file is compiled with (the pragma has function scope: a plain a + b * c next to
// a call still fuses).  The toolchain's __fmul_rn / __fadd_rn do NOT give this: they are plain operators in a header compiled under the
// default -ffp-contract=fast, and after inlining __fadd_rn(a, __fmul_rn(b, c)) becomes one v_fmac_f32 even below a file-level
// `#pragma clang fp contract(off)`.  det_loss.hip predates the rule and is the known exception.
__device__ __forceinline__ float f_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float f_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ float f_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float f_div(float a, float b) {      // IEEE division
#pragma clang fp contract(off)
    return a / b;
}

__device__ __forceinline__ float box_area(float x0, float y0, float x1, float y1) { return f_mul(f_sub(x1, x0), f_sub(y1, y0)); }

// ---- rows of an image ----------------------------------------------------------------------------
struct Range { int s, n; };

// rows [s, s + n) of image b.  starts is device data: both ends are clamped to [0, total], the length to cap, a non-monotone pair is empty
__device__ __forceinline__ Range img_range(const int* __restrict__ starts, int b, int total, int cap) {
    int s = starts[b], e = starts[b + 1];
    s = min(max(s, 0), total);
    e = min(max(e, 0), total);
    Range r;
    r.s = s;
    r.n = e > s ? min(e - s, cap) : 0;
    return r;
}

// ---- sort keys -------------------------------------------------------------------------------------
// float bits -> unsigned with the same order (-0 below +0); NaNs are the caller's business
__device__ __forceinline__ uint32_t ord_bits(float v) {
    const uint32_t u = __float_as_uint(v);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float ord_float(uint32_t o) {
    return __uint_as_float(o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// ascending bitonic sort of P (a power of two) keys by nthr threads of one workgroup; keys in LDS or in global memory
__device__ __forceinline__ void bitonic_sort(u64* keys, int P, int tid, int nthr) {
    for (int k2 = 2; k2 <= P; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += nthr) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int q = i | j;
                const bool up = (i & k2) == 0;
                const u64 x = keys[i], y = keys[q];
                if ((x > y) == up) {
                    keys[i] = y;
                    keys[q] = x;
                }
            }
            __threadfence_block();
            __syncthreads();
        }
    }
}

__device__ __forceinline__ int next_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// ---- workgroup sums ------------------------------------------------------------------------------
// the sum of a workgroup's 256 values in a fixed order: butterfly inside each wave, then the four waves in ascending order
__device__ __forceinline__ float block_sum_256(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ int block_sum_256(int v, int* part) {       // every thread gets the sum; part: 4 ints of LDS
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((tid & 63) == 0) part[tid >> 6] = v;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}

// ---- box coder -------------------------------------------------------------------------------------
struct BoxCoder { float mean[4], std[4], max_ratio; };

// np.abs(np.log(wh_ratio_clip)) in double, rounded once where fp32 meets it
inline float coder_max_ratio(float wh_ratio_clip) { return (float)fabs(log((double)wh_ratio_clip)); }

// mmdet 2.x DeltaXYWHBBoxCoder.decode (delta2bbox, add_ctr_clamp=False): anchor corners a, raw deltas d -> corners o, every product and
// sum rounded on its own in the order the reference's tensor expressions evaluate them.  hw != NULL: clip_border to (h, w) = hw[0], hw[1].
__device__ __forceinline__ void decode_box(const BoxCoder& bc, const float* __restrict__ a, const float* d, const float* __restrict__ hw,
                                           float* o) {
    float n[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) n[q] = f_add(f_mul(d[q], bc.std[q]), bc.mean[q]);
    const float x0 = a[0], y0 = a[1], x1 = a[2], y1 = a[3];
    const float px = f_mul(f_add(x0, x1), 0.5f), py = f_mul(f_add(y0, y1), 0.5f);
    const float pw = f_sub(x1, x0), ph = f_sub(y1, y0);
    const float dw = fminf(fmaxf(n[2], -bc.max_ratio), bc.max_ratio), dh = fminf(fmaxf(n[3], -bc.max_ratio), bc.max_ratio);
    const float gx = f_add(px, f_mul(pw, n[0])), gy = f_add(py, f_mul(ph, n[1]));
    const float hx = f_mul(f_mul(pw, expf(dw)), 0.5f), hy = f_mul(f_mul(ph, expf(dh)), 0.5f);
    o[0] = f_sub(gx, hx), o[1] = f_sub(gy, hy), o[2] = f_add(gx, hx), o[3] = f_add(gy, hy);
    if (hw) {
        const float h = hw[0], w = hw[1];
        o[0] = fminf(fmaxf(o[0], 0.f), w);
        o[1] = fminf(fmaxf(o[1], 0.f), h);
        o[2] = fminf(fmaxf(o[2], 0.f), w);
        o[3] = fminf(fmaxf(o[3], 0.f), h);
    }
}

// mmdet's bbox2delta of box p against ground truth q, then (d - mean) / std; logf is the only transcendental
__device__ __forceinline__ void encode_delta(const BoxCoder& bc, const float* __restrict__ p, const float* __restrict__ q, float* d) {
    const float px = f_mul(f_add(p[0], p[2]), 0.5f), py = f_mul(f_add(p[1], p[3]), 0.5f);
    const float pw = f_sub(p[2], p[0]), ph = f_sub(p[3], p[1]);
    const float gx = f_mul(f_add(q[0], q[2]), 0.5f), gy = f_mul(f_add(q[1], q[3]), 0.5f);
    const float gw = f_sub(q[2], q[0]), gh = f_sub(q[3], q[1]);
    d[0] = f_div(f_sub(gx, px), pw);
    d[1] = f_div(f_sub(gy, py), ph);
    d[2] = logf(f_div(gw, pw));
    d[3] = logf(f_div(gh, ph));
#pragma unroll
    for (int c = 0; c < 4; ++c) d[c] = f_div(f_sub(d[c], bc.mean[c]), bc.std[c]);
}
