// Flat multi-tensor AdamW for the student (decoupled weight decay, bias-corrected), one launch for all
// trainable tensors.  Reference: torch.optim.AdamW as constructed in src/training/main.py:198-213
// (no-decay group = ndim<2 / "ln" / "bias" / "logit_scale"; decay group wd=args.wd), stepped at train.py:115;
// parameters whose grad is None are skipped entirely (no decay either) -- SURVEY.md D7.
//
// MI355X layout: all trainable parameters live in ONE fp32 master buffer (every tensor starts on a 64-element
// boundary, total padded to 256) with same-layout fp32 grad / exp_avg / exp_avg_sq buffers and a same-layout bf16 "shadow" that the
// MFMA GEMMs read.  A flag byte per 64 elements carries (bit0) "has a gradient this step" and (bit1)
// "weight decay applies".  The kernel is a pure HBM stream: 4 fp32 reads + 3 fp32 writes + 1 bf16 write per element.
#include "cs_common.h"
#include "../../include/clipself_hip.h"

namespace {

struct AdamArgs {
    float* p; const float* g; float* m; float* v; __bf16* shadow; const uint8_t* flags;
    long nchunks;
    float lr, beta1, beta2, eps, wd, bc1, bc2_sqrt, grad_scale;
};

// GUARD = false is the plain step.  GUARD = true (cs_adamw_step with a guard buffer) takes two decisions from the guard head that
// guard_finalize_kernel wrote: head[2] == 0 -> the step is skipped and the launch writes nothing; head[1] = clip coefficient, folded
// into the one multiply every gradient element already gets (coefficient 1 -> the same bits as GUARD = false).
template <bool GUARD>
__global__ __launch_bounds__(256) void adamw_kernel(AdamArgs a, const float* head) {
    float gscale = a.grad_scale;
    if constexpr (GUARD) {
        if (head[2] == 0.f) return;
        gscale = a.grad_scale * head[1];
    }
    // one wave per 256-element chunk, 4 elements per lane
    const long chunk = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= a.nchunks) return;
    const uint8_t f = a.flags[chunk * 4 + ((threadIdx.x & 63) >> 4)];   // one flag byte per 64 elements (= 16 lanes)
    if (!(f & 1)) return;
    const long i = chunk * 256 + (threadIdx.x & 63) * 4;
    float4 p = *(const float4*)(a.p + i);
    const float4 g4 = *(const float4*)(a.g + i);
    float4 m = *(const float4*)(a.m + i), v = *(const float4*)(a.v + i);
    const float decay = (f & 2) ? 1.f - a.lr * a.wd : 1.f;
    const float step = a.lr / a.bc1;
    float pp[4] = {p.x, p.y, p.z, p.w}, gg[4] = {g4.x, g4.y, g4.z, g4.w}, mm[4] = {m.x, m.y, m.z, m.w}, vv[4] = {v.x, v.y, v.z, v.w};
    U64 sh;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float g = gg[e] * gscale;
        pp[e] *= decay;                                       // p.mul_(1 - lr*wd)
        mm[e] = a.beta1 * mm[e] + (1.f - a.beta1) * g;        // exp_avg.lerp_(grad, 1-beta1)
        vv[e] = a.beta2 * vv[e] + (1.f - a.beta2) * g * g;    // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1-beta2)
        const float denom = sqrtf(vv[e]) / a.bc2_sqrt + a.eps;
        pp[e] -= step * (mm[e] / denom);
        sh.e[e] = f2bf(pp[e]);
    }
    *(float4*)(a.p + i) = make_float4(pp[0], pp[1], pp[2], pp[3]);
    *(float4*)(a.m + i) = make_float4(mm[0], mm[1], mm[2], mm[3]);
    *(float4*)(a.v + i) = make_float4(vv[0], vv[1], vv[2], vv[3]);
    if (a.shadow) *(uint2*)(a.shadow + i) = sh.u;
}

// ---- gradient norm of the guarded step: partial sums of squares (a) and their combination (b), no atomics, fixed summation order.
// The buffer's layout is the header's: CS_ADAMW_GUARD_HEAD floats, then one partial per CS_ADAMW_GUARD_SPAN elements.
constexpr int GUARD_CHUNKS = CS_ADAMW_GUARD_SPAN / 256;        // 256-element chunks per partial: 64, 16 per wave
constexpr int GUARD_FINAL_THREADS = 256;

// (a) workgroup k -> guard[CS_ADAMW_GUARD_HEAD + k] = sum over the active granules of [k * SPAN, (k + 1) * SPAN) of (grad_scale * g)^2, whatever the
// grid: wave w takes chunks w, w + 4, ... of the span with adamw_kernel's chunk / flag-byte addressing; inactive granules and chunks past n are not loaded.
// Rounding depth of one element's path: scale (counts twice under the square), square, 16 adds in a lane component, 2 to fold the 4
// components, 6 shuffle levels, 2 across the 4 waves -- at most 29 fp32 roundings; the rest of the sum is done in double by (b), which
// rounds the root once more.  Relative error of the norm <= 29 * 2^-24 / 2 + 2^-24 < 1e-6.
__global__ __launch_bounds__(256) void guard_partial_kernel(const float* __restrict__ g, const uint8_t* __restrict__ flags, long nchunks,
                                                            float grad_scale, float* __restrict__ partials) {
    __shared__ float wsum[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long chunk0 = (long)blockIdx.x * GUARD_CHUNKS + wave;
    // the wave's 64 flag bytes in one load (lane 4j + q: granule q of chunk j), handed round by shuffles: the 16 gradient loads below then
    // wait for nothing but each other
    const long fchunk = chunk0 + (lane >> 2) * 4;
    const int fb = fchunk < nchunks ? flags[fchunk * 4 + (lane & 3)] : 0;
    float4 x[GUARD_CHUNKS / 4];
#pragma unroll
    for (int j = 0; j < GUARD_CHUNKS / 4; ++j) {
        x[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (__shfl(fb, j * 4 + (lane >> 4), 64) & 1) x[j] = *(const float4*)(g + (chunk0 + j * 4) * 256 + lane * 4);
    }
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int j = 0; j < GUARD_CHUNKS / 4; ++j) {
        const float a0 = x[j].x * grad_scale, a1 = x[j].y * grad_scale, a2 = x[j].z * grad_scale, a3 = x[j].w * grad_scale;
        s0 += a0 * a0; s1 += a1 * a1; s2 += a2 * a2; s3 += a3 * a3;
    }
    float s = (s0 + s1) + (s2 + s3);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// (b) one workgroup: thread t adds partials t, t + 256, ... in index order, the 256 thread sums go through a fixed tree, all in double; thread 0
// is the only writer of head[0..3].
__global__ __launch_bounds__(GUARD_FINAL_THREADS) void guard_finalize_kernel(float* guard, long npartials, float max_norm, int skip_nonfinite) {
    __shared__ double tsum[GUARD_FINAL_THREADS];
    double s = 0.0;
    for (long k = threadIdx.x; k < npartials; k += GUARD_FINAL_THREADS) s += (double)guard[CS_ADAMW_GUARD_HEAD + k];
    tsum[threadIdx.x] = s;
    __syncthreads();
    for (int off = GUARD_FINAL_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) tsum[threadIdx.x] += tsum[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const float norm = (float)__builtin_sqrt(tsum[0]);
    float coef = 1.f;
    if (max_norm > 0.f) {                              // clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1), a NaN norm stays NaN
        const float c = max_norm / (norm + 1e-6f);
        coef = c < 1.f ? c : (c != c ? c : 1.f);
    }
    const bool finite = __builtin_isfinite(norm);
    const bool skip = skip_nonfinite && !finite;
    guard[0] = norm;
    guard[1] = coef;
    guard[2] = skip ? 0.f : 1.f;
    if (skip) guard[3] += 1.f;
}

}  // namespace

// n must be a multiple of 256; flags has n/64 bytes (bit0 = active, bit1 = decay).  `step` is the 1-based AdamW
// step count (bias corrections computed here in double like torch's scalar path).  guard == NULL: one launch, max_norm and skip_nonfinite
// are not looked at.  guard != NULL (CS_ADAMW_GUARD_HEAD + ceil(n / CS_ADAMW_GUARD_SPAN) floats): partial sums, finalise, guarded step.
extern "C" int cs_adamw_step(float* p, const float* g, float* m, float* v, void* shadow_bf16, const uint8_t* flags, long n,
                             float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                             float max_norm, int skip_nonfinite, float* guard, hipStream_t stream) {
    CS_CHECK_ARG(n > 0 && n % 256 == 0, "cs_adamw_step: n must be a positive multiple of 256");
    CS_CHECK_ARG(step >= 1, "cs_adamw_step: step is 1-based");
    if (guard) {
        CS_CHECK_ARG(max_norm == max_norm, "cs_adamw_step: max_norm is NaN");
        CS_CHECK_ARG(skip_nonfinite == 0 || skip_nonfinite == 1, "cs_adamw_step: skip_nonfinite must be 0 or 1");
    }
    AdamArgs a;
    a.p = p; a.g = g; a.m = m; a.v = v; a.shadow = (__bf16*)shadow_bf16; a.flags = flags; a.nchunks = n / 256;
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.wd = weight_decay; a.grad_scale = grad_scale;
    a.bc1 = (float)(1.0 - __builtin_pow((double)beta1, (double)step));
    a.bc2_sqrt = (float)__builtin_sqrt(1.0 - __builtin_pow((double)beta2, (double)step));
    if (!guard) {
        hipLaunchKernelGGL(adamw_kernel<false>, dim3((int)((a.nchunks + 3) / 4)), dim3(256), 0, stream, a, (const float*)nullptr);
        CS_LAUNCH_CHECK();
        return 0;
    }
    const long npartials = (n + CS_ADAMW_GUARD_SPAN - 1) / CS_ADAMW_GUARD_SPAN;
    hipLaunchKernelGGL(guard_partial_kernel, dim3((int)npartials), dim3(256), 0, stream, g, flags, a.nchunks, grad_scale, guard + CS_ADAMW_GUARD_HEAD);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(guard_finalize_kernel, dim3(1), dim3(GUARD_FINAL_THREADS), 0, stream, guard, npartials, max_norm, skip_nonfinite);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(adamw_kernel<true>, dim3((int)((a.nchunks + 3) / 4)), dim3(256), 0, stream, a, (const float*)guard);
    CS_LAUNCH_CHECK();
    return 0;
}
