// Epilogues 10 / 11 of cs_gemm_nt (include/clipself_hip.h, "THIN FORMS"): 1 x 1 convolutions with at most 16 output channels on
// channel-last rows, forward and input gradient.  gfx950 only.
//
// Y[M, N <= 16] = X[M, K] . W[N, K]^T reads 2 * K bytes of a row for at most 64 bytes of output: a stream, not a matrix-core problem.  A
// wave owns 16 rows at a time; the N <= 16 columns fit one v_mfma_f32_16x16x32_bf16 tile (columns >= N are zero weights), whose operand
// layout is what a lane loads anyway -- A[row l & 15][k = 8 (l >> 4) + j]: 16 bytes of one row -- and whose C layout (col = l & 15, rows
// 4 (l >> 4) + r) is four consecutive pixels of one NCHW plane: a 16-byte store.  No LDS, no barrier, no workspace.
//   forward  (thin_fwd_kernel):   acc += mfma(A = X fragment, B = W fragment) over K / 32 steps; W fragments stay in registers for the
//            launch when K == 256 (KS = 8: 32 VGPRs), else they are re-read per step (they sit in L1).
//   gradient (thin_dgrad_kernel): the transposed product dX^T[k, m] = sum_n W[n, k] * dY[m, n], contraction n padded to 32 with zeros, so
//            that a lane ends with CONSECUTIVE k of ONE row: tile row i = 4 q + r of the (u, e)-th MFMA stands for channel
//            k = 32 u + 8 q + 4 e + r, and after e = 0, 1 lane (q, m) holds dX[m][32 u + 8 q .. + 8): one 16-byte bf16 store (two for fp32),
//            one 16-byte gate load.  The W^T fragments (a gather) are built once per wave when K == 256 (KU = 8: 64 VGPRs).
//            One MFMA per 16 x 16 output tile with a 16-deep contraction: 1/16 of the matrix pipe's rate suffices beside the stream.
// Rows past M load row M - 1 and store nothing.  All offsets are 64-bit.
#include "gemm_common.h"
#include "../../include/clipself_hip.h"

namespace {

constexpr int THIN_BLOCKS_PER_CU = 8;          // 32 waves per CU at the most: the grid cap of the grid-stride loop
constexpr int THIN_MAX_N = 16;

struct ThinArgs {
    const void* xin;       // epi 10: X rows (bf16 / fp32)
    void* xout;            // epi 11: dX rows (bf16 / fp32)
    const __bf16* W;       // [N, K], row stride ldb
    const float* bias;     // epi 10: [N] or null
    const __bf16* gate;    // epi 11: rows with dX's stride, or null
    float* y1;             // epi 10: rows T / planes P1
    float* y2;             //         planes P2
    const float* d1;       // epi 11: rows T / planes P1
    const float* d2;       //         planes P2 or null
    long ldx;              // stride of the K-wide rows, elements
    long ldt;              // rows form: stride of T
    int M, N, K, ldb;
    int R;                 // 0 = rows form, else pixels per image
    int s;                 // planes form: columns of the first block
    int vec;               // epi 10, planes form: 16-byte stores (R % 4 == 0, aligned base)
    int tiles;             // ceil(M / 16)
};

__device__ __forceinline__ bf16x8 pack8(const float4 a, const float4 b) {
    bf16x8 v;
    v[0] = f2bf(a.x); v[1] = f2bf(a.y); v[2] = f2bf(a.z); v[3] = f2bf(a.w);
    v[4] = f2bf(b.x); v[5] = f2bf(b.y); v[6] = f2bf(b.z); v[7] = f2bf(b.w);
    return v;
}

template <bool F32>
__device__ __forceinline__ bf16x8 load_x8(const void* base, size_t off) {      // 8 consecutive elements of a row as a bf16 fragment (RNE)
    if constexpr (F32) {
        const float4* s = (const float4*)((const float*)base + off);
        return pack8(s[0], s[1]);
    } else {
        U128 u;
        u.u = *(const uint4*)((const __bf16*)base + off);
        return u.h;
    }
}

__device__ __forceinline__ bf16x8 zero8() {
    U128 u;
    u.u = make_uint4(0, 0, 0, 0);
    return u.h;
}

__device__ __forceinline__ bf16x8 w_frag(const ThinArgs& p, int n, int k) {     // W[n][k .. k + 8), zeros for n >= N
    if (n >= p.N) return zero8();
    U128 u;
    u.u = *(const uint4*)(p.W + (size_t)n * p.ldb + k);
    return u.h;
}

// ------------------------------------------------------------------------------------------------ epilogue 10
template <bool XF32, int KS>
__global__ __launch_bounds__(256) void thin_fwd_kernel(const ThinArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int ks = KS ? KS : p.K / 32;
    bf16x8 wf[KS ? KS : 1];
    if constexpr (KS > 0) {
#pragma unroll
        for (int t = 0; t < KS; ++t) wf[t] = w_frag(p, i, 32 * t + 8 * q);
    }
    const float b = (p.bias != nullptr && i < p.N) ? p.bias[i] : 0.f;
    for (long tile = (long)blockIdx.x * 4 + wave; tile < p.tiles; tile += (long)gridDim.x * 4) {
        const long m0 = tile * 16;
        const long row = min(m0 + i, (long)p.M - 1);
        const size_t xoff = (size_t)row * p.ldx + 8 * q;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if constexpr (KS > 0) {
            bf16x8 xf[KS];
#pragma unroll
            for (int t = 0; t < KS; ++t) xf[t] = load_x8<XF32>(p.xin, xoff + 32 * t);
#pragma unroll
            for (int t = 0; t < KS; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[t], wf[t], acc, 0, 0, 0);
        } else {
            for (int t = 0; t < ks; t += 2) {                        // K % 64 == 0: two steps at a time
                const bf16x8 x0 = load_x8<XF32>(p.xin, xoff + 32 * t), x1 = load_x8<XF32>(p.xin, xoff + 32 * t + 32);
                const bf16x8 w0 = w_frag(p, i, 32 * t + 8 * q), w1 = w_frag(p, i, 32 * t + 32 + 8 * q);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x0, w0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x1, w1, acc, 0, 0, 0);
            }
        }
        // lane: column n = i, rows m0 + 4 q + r
        const int n = i;
        const long mr = m0 + 4 * q;
        if (n < p.N && mr < p.M) {
            acc[0] += b; acc[1] += b; acc[2] += b; acc[3] += b;
            const bool first = n < p.s;
            float* plane = first ? p.y1 : p.y2;
            const int width = first ? p.s : p.N - p.s, col = first ? n : n - p.s;
            if (p.R == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (mr + r < p.M) p.y1[(size_t)(mr + r) * p.ldt + n] = acc[r];
            } else if (p.vec) {                                       // R % 4 == 0, M % 4 == 0: four pixels of one image, 16-byte aligned
                const unsigned img = (unsigned)mr / (unsigned)p.R, pix = (unsigned)mr - img * (unsigned)p.R;
                *(float4*)(plane + ((size_t)img * width + col) * p.R + pix) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long m = mr + r;
                    if (m < p.M) {
                        const unsigned img = (unsigned)m / (unsigned)p.R, pix = (unsigned)m - img * (unsigned)p.R;
                        plane[((size_t)img * width + col) * p.R + pix] = acc[r];
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ epilogue 11
// W^T fragment of MFMA (u, e): lane (i, q) holds W[n = 8 q + j][k = 32 u + 8 (i >> 2) + 4 e + (i & 3)], j = 0..7; zeros for n >= N
__device__ __forceinline__ bf16x8 wt_frag(const ThinArgs& p, int i, int q, int u, int e) {
    bf16x8 v = zero8();
    const int k = 32 * u + 8 * (i >> 2) + 4 * e + (i & 3);
    if (q < 2) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int n = 8 * q + j;
            if (n < p.N) v[j] = p.W[(size_t)n * p.ldb + k];
        }
    }
    return v;
}

template <bool DF32>
__device__ __forceinline__ void store_dx8(const ThinArgs& p, size_t off, f32x4 lo, f32x4 hi, bool gated, uint4 g) {
    float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    if (gated) {
        const uint32_t w[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float gv = bfbits2f((uint16_t)(w[j >> 1] >> (16 * (j & 1))));
            if (gv <= 0.f) v[j] = 0.f;                                // a NaN gate passes (the ReLU rule of epilogue 9)
        }
    }
    if constexpr (DF32) {
        float4* d = (float4*)((float*)p.xout + off);
        d[0] = make_float4(v[0], v[1], v[2], v[3]);
        d[1] = make_float4(v[4], v[5], v[6], v[7]);
    } else {
        U128 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o.e[j] = f2bf(v[j]);
        *(uint4*)((__bf16*)p.xout + off) = o.u;
    }
}

template <bool DF32, int KU>
__global__ __launch_bounds__(256) void thin_dgrad_kernel(const ThinArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int ku = KU ? KU : p.K / 32;
    bf16x8 wa[KU ? KU : 1][2];
    if constexpr (KU > 0) {
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            wa[u][0] = wt_frag(p, i, q, u, 0);
            wa[u][1] = wt_frag(p, i, q, u, 1);
        }
    }
    const bool gated = p.gate != nullptr;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (long tile = (long)blockIdx.x * 4 + wave; tile < p.tiles; tile += (long)gridDim.x * 4) {
        const long m = tile * 16 + i;                                 // this lane's row, as B operand column and as output row
        const long mc = min(m, (long)p.M - 1);
        // B operand: dY[mc][n = 8 q + j] rounded to bf16, zeros for n >= N
        bf16x8 dyf = zero8();
        if (q < 2) {
            if (p.R == 0) {
                const float* src = p.d1 + (size_t)mc * p.ldt;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (8 * q + j < p.N) dyf[j] = f2bf(src[8 * q + j]);
            } else {
                const unsigned img = (unsigned)mc / (unsigned)p.R, pix = (unsigned)mc - img * (unsigned)p.R;
                const float* s1 = p.d1 + (size_t)img * p.s * p.R + pix;
                const float* s2 = p.d2 ? p.d2 + (size_t)img * (p.N - p.s) * p.R + pix : nullptr;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int n = 8 * q + j;
                    if (n < p.s) dyf[j] = f2bf(s1[(size_t)n * p.R]);
                    else if (n < p.N) dyf[j] = f2bf(s2[(size_t)(n - p.s) * p.R]);
                }
            }
        }
        const size_t off = (size_t)mc * p.ldx + 8 * q;                // dX / gate [mc][32 u + 8 q ..]
        const bool live = m < p.M;
        if constexpr (KU > 0) {
            uint4 g[KU];
            if (gated) {
#pragma unroll
                for (int u = 0; u < KU; ++u) g[u] = *(const uint4*)(p.gate + off + 32 * u);
            }
#pragma unroll
            for (int u = 0; u < KU; ++u) {
                const f32x4 lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[u][0], dyf, z, 0, 0, 0);
                const f32x4 hi = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[u][1], dyf, z, 0, 0, 0);
                if (live) store_dx8<DF32>(p, off + 32 * u, lo, hi, gated, gated ? g[u] : make_uint4(0, 0, 0, 0));
            }
        } else {
            for (int u = 0; u < ku; ++u) {
                const uint4 g = gated ? *(const uint4*)(p.gate + off + 32 * u) : make_uint4(0, 0, 0, 0);
                const bf16x8 a0 = wt_frag(p, i, q, u, 0), a1 = wt_frag(p, i, q, u, 1);
                const f32x4 lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, dyf, z, 0, 0, 0);
                const f32x4 hi = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, dyf, z, 0, 0, 0);
                if (live) store_dx8<DF32>(p, off + 32 * u, lo, hi, gated, g);
            }
        }
    }
}

}  // namespace

// cs_gemm_nt's argument list, epi 10 / 11 (the header states the packing).  Every check comes before the launch.
int cs_thin_launch(const void* A, const void* B, void* C, const float* bias, const float* extra, int M, int N, int K, int lda, int ldb, int ldc,
                   int epi, int splits, int group, int flags, hipStream_t stream) {
    const bool fwd = epi == EPI_THIN_FWD;
    const int f32 = flags & 1;
    const int R = group;
    const char* who = fwd ? "cs_gemm_nt (thin forward, epilogue 10)" : "cs_gemm_nt (thin input gradient, epilogue 11)";
    CS_CHECK_ARG(A && B && C && M > 0 && N >= 1 && N <= THIN_MAX_N && K > 0 && K % 64 == 0,
                 "%s: M=%d > 0, 1 <= N=%d <= 16, K=%d a positive multiple of 64, no NULL operand", who, M, N, K);
    CS_CHECK_ARG(splits == 1, "%s: splits=%d, the thin forms have no split-K", who, splits);
    CS_CHECK_ARG(ldb >= K && ldb % 8 == 0 && ((uintptr_t)B % 16) == 0, "%s: W is bf16 [N, K] with ldb=%d >= K, ldb %% 8 == 0, 16-byte aligned", who, ldb);
    CS_CHECK_ARG(R >= 0 && (R == 0 || M % R == 0), "%s: group=%d is 0 (rows) or the pixels per image, a divisor of M=%d", who, R, M);
    const int ldk = fwd ? lda : ldc;                                    // stride of the K-wide rows
    const void* krows = fwd ? A : C;
    CS_CHECK_ARG(ldk >= K && ldk % (f32 ? 4 : 8) == 0 && ((uintptr_t)krows % 16) == 0,
                 "%s: the %s rows need a stride=%d >= K=%d that keeps 16-byte rows (%% %d) and a 16-byte aligned base", who, fwd ? "X" : "dX", ldk, K,
                 f32 ? 4 : 8);
    const int thin_arg = fwd ? ldc : lda;                               // rows form: stride of T; planes form: the split s
    const void* thin = fwd ? (const void*)C : A;
    CS_CHECK_ARG(((uintptr_t)thin % 4) == 0, "%s: the fp32 side must be 4-byte aligned", who);
    if (R == 0) CS_CHECK_ARG(thin_arg >= N, "%s: rows form, stride=%d below N=%d", who, thin_arg, N);
    else CS_CHECK_ARG(thin_arg >= 1 && thin_arg <= N, "%s: planes form, split s=%d outside [1, N=%d]", who, thin_arg, N);
    ThinArgs p{};
    p.W = (const __bf16*)B;
    p.M = M; p.N = N; p.K = K; p.ldb = ldb; p.R = R;
    p.ldx = ldk;
    p.ldt = R == 0 ? thin_arg : 0;
    p.s = R == 0 ? N : thin_arg;
    p.tiles = (int)(((long)M + 15) / 16);
    if (fwd) {
        CS_CHECK_ARG(bias == nullptr || ((uintptr_t)bias % 4) == 0, "%s: bias must be 4-byte aligned", who);
        p.xin = A; p.bias = bias;
        p.y1 = (float*)C;
        p.y2 = R ? (float*)C + (size_t)M * p.s : nullptr;
        p.vec = R > 0 && R % 4 == 0 && ((uintptr_t)C % 16) == 0;
    } else {
        if (R == 0) CS_CHECK_ARG(bias == nullptr, "%s: rows form has one dY block (bias must be NULL)", who);
        else CS_CHECK_ARG((bias != nullptr) == (p.s < N) && ((uintptr_t)bias % 4) == 0,
                          "%s: planes form, a 4-byte aligned second dY block (bias) exactly when s=%d < N=%d", who, p.s, N);
        CS_CHECK_ARG(extra == nullptr || (((uintptr_t)extra % 16) == 0 && ldc % 8 == 0),
                     "%s: the gate is bf16 rows with dX's stride=%d (%% 8 == 0), 16-byte aligned", who, ldc);
        p.xout = C; p.gate = (const __bf16*)extra;
        p.d1 = (const float*)A; p.d2 = bias;
    }
    long blocks = ((long)p.tiles + 3) / 4;
    const long cap = (long)THIN_BLOCKS_PER_CU * cs_num_cus();
    if (blocks > cap) blocks = cap;
    const dim3 grid((unsigned)blocks), block(256);
    if (fwd) {
        if (K == 256) {
            if (f32) hipLaunchKernelGGL((thin_fwd_kernel<true, 8>), grid, block, 0, stream, p);
            else hipLaunchKernelGGL((thin_fwd_kernel<false, 8>), grid, block, 0, stream, p);
        } else {
            if (f32) hipLaunchKernelGGL((thin_fwd_kernel<true, 0>), grid, block, 0, stream, p);
            else hipLaunchKernelGGL((thin_fwd_kernel<false, 0>), grid, block, 0, stream, p);
        }
    } else {
        if (K == 256) {
            if (f32) hipLaunchKernelGGL((thin_dgrad_kernel<true, 8>), grid, block, 0, stream, p);
            else hipLaunchKernelGGL((thin_dgrad_kernel<false, 8>), grid, block, 0, stream, p);
        } else {
            if (f32) hipLaunchKernelGGL((thin_dgrad_kernel<true, 0>), grid, block, 0, stream, p);
            else hipLaunchKernelGGL((thin_dgrad_kernel<false, 0>), grid, block, 0, stream, p);
        }
    }
    CS_LAUNCH_CHECK();
    return 0;
}
