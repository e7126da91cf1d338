// Epilogues 10 / 11 / 12 of cs_gemm_nt (include/clipself_hip.h, "THIN FORMS"): 1 x 1 convolutions with at most 16 output channels on
// channel-last rows, forward, input gradient and weight + bias gradient (epilogue 12: see its own section below).  gfx950 only.
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

// ------------------------------------------------------------------------------------------------ epilogue 12
// dW[n, k] = sum_m bf16(dY[m, n]) * bf16(X[m, k]) and db[n] = sum_m bf16(dY[m, n]): the contraction is the row index, so the MFMA's A
// operand is dY^T -- lane (i, q) holds dY[m0 + 8 q + j][n = i], j = 0..7 -- and its B operand X[m0 + 8 q + j][k = 16 t + i], eight rows of
// ONE column: the transpose ds_read_b64_tr_b16 performs.  A wave stages its 32 rows x KC columns in LDS as loaded (bf16; fp32 rows are
// rounded in registers) and reads the KC / 16 B fragments back transposed; the accumulators (4 VGPRs per 16 columns) stay in registers
// over the whole grid-stride loop.  The LDS image is image (b) of the transposed-read note in cdna_hip_programming.md: [32 rows][128
// columns] tiles of 256-byte rows whose 16-byte chunk ch of row r sits at chunk ch ^ (((r & 3) << 2) | ((r >> 2) & 3)).  A 32-lane half reads
// rows 8 q + {0..3} of two groups q, q + 1 (8 rows apart, the same 32 bytes of columns): the XOR sends the eight rows to eight different
// 32-byte bank groups of the 256-byte bank period -- conflict-free by the bank rule (a / 4) % 64.
// The transposed read needs EXEC all ones: every loop and branch around it is wave-uniform, and the ragged last step is padded, not
// masked (rows past M load row M - 1 and are zeroed in registers; the dY fragment is zero there).
constexpr int TW_BLOCKS_PER_CU = 2;            // 64 KiB of LDS per workgroup at KC = 256
constexpr int TW_WG_ROWS = 128;                // four waves x 32 rows
constexpr int TW_SLICES = 16;                  // the reduction adds 16 groups of partials side by side

struct ThinWgradArgs {
    const void* X;         // rows [M, K], bf16 / fp32
    const float* d1;       // rows T / planes P1
    const float* d2;       // planes P2 or null
    float* out;            // dW (direct) or the first partial
    float* dbout;          // db (direct) or the first partial's 16 floats
    long ldx, ldt, ldo;    // strides: X rows, T rows, rows of `out`
    long pstride;          // floats between two workgroups' partials (0 when direct)
    long tiles;            // ceil(M / 32)
    int M, N, K;
    int R, s, vec;         // vec: planes read 32 bytes at a time
};

__device__ __forceinline__ int tw_off(int row, int ch) {               // byte offset of 16-byte chunk ch of row `row` in a wave's image
    return (ch >> 4) * 8192 + 256 * row + 16 * ((ch & 15) ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

typedef __attribute__((ext_vector_type(4))) short tw_s16x4;
typedef __attribute__((ext_vector_type(8))) short tw_s16x8;

// dY[mrow .. mrow + 8)[n] rounded to bf16; zeros for n >= N and for rows >= M
__device__ __forceinline__ bf16x8 tw_dy_frag(const ThinWgradArgs& p, long mrow, int n) {
    bf16x8 v = zero8();
    if (n >= p.N) return v;
    if (p.R == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const long m = mrow + j;
            const float f = p.d1[(size_t)min(m, (long)p.M - 1) * p.ldt + n];
            v[j] = f2bf(m < p.M ? f : 0.f);
        }
        return v;
    }
    const bool first = n < p.s;
    const float* plane = first ? p.d1 : p.d2;
    const int width = first ? p.s : p.N - p.s, col = first ? n : n - p.s;
    if (p.vec) {                                                      // R % 8 == 0: eight pixels of one image, 32-byte aligned
        if (mrow < p.M) {
            const unsigned img = (unsigned)mrow / (unsigned)p.R, pix = (unsigned)mrow - img * (unsigned)p.R;
            const float4* src = (const float4*)(plane + ((size_t)img * width + col) * p.R + pix);
            v = pack8(src[0], src[1]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const long m = mrow + j;
            if (m < p.M) {
                const unsigned img = (unsigned)m / (unsigned)p.R, pix = (unsigned)m - img * (unsigned)p.R;
                v[j] = f2bf(plane[((size_t)img * width + col) * p.R + pix]);
            }
        }
    }
    return v;
}

template <bool XF32, int KC>
__global__ __launch_bounds__(256) void thin_wgrad_kernel(const ThinWgradArgs p) {
    constexpr int TILES = KC / 16;                                    // MFMA output tiles: 16 (n) x 16 (k) each
    constexpr int IMG = (KC + 127) / 128 * 8192;                      // a wave's image, bytes
    constexpr int CPR = KC / 8;                                       // 16-byte chunks per row
    constexpr int LOADS = 32 * CPR / 64;                              // chunks per lane and step
    constexpr int GROUP = (XF32 && LOADS > 8) ? LOADS / 2 : LOADS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, q = lane >> 4;
    char* const img = smem + wave * IMG;
    const int kc0 = blockIdx.y * KC;
    // transposed reads: lane 4 qq + pp of group q supplies row 8 q (+ 4) + qq, columns 16 t + 4 pp .. + 4
    const int qq = i >> 2, pp = i & 3;
    const int row0 = 8 * q + qq, row1 = row0 + 4;
    f32x4 acc[TILES];
#pragma unroll
    for (int t = 0; t < TILES; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dbacc = 0.f;
    for (long tile = (long)blockIdx.x * 4 + wave; tile < p.tiles; tile += (long)gridDim.x * 4) {
        const long m0 = tile * 32;
        const bf16x8 dyf = tw_dy_frag(p, m0 + 8 * q, i);
#pragma unroll
        for (int g0 = 0; g0 < LOADS; g0 += GROUP) {                    // fp32 rows at KC = 256: two halves, 64 VGPRs of loads in flight each
            bf16x8 xv[GROUP];
#pragma unroll
            for (int t = 0; t < GROUP; ++t) {
                const int c = (g0 + t) * 64 + lane, row = c / CPR, ch = c - row * CPR;
                const long m = m0 + row;
                const bf16x8 v = load_x8<XF32>(p.X, (size_t)min(m, (long)p.M - 1) * p.ldx + kc0 + ch * 8);
                xv[t] = m < p.M ? v : zero8();
            }
#pragma unroll
            for (int t = 0; t < GROUP; ++t) {
                const int c = (g0 + t) * 64 + lane, row = c / CPR, ch = c - row * CPR;
                U128 u;
                u.h = xv[t];
                *(uint4*)(img + tw_off(row, ch)) = u.u;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) dbacc += (float)dyf[j];
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
            const int a0 = tw_off(row0, 2 * t + (pp >> 1)) + 8 * (pp & 1), a1 = tw_off(row1, 2 * t + (pp >> 1)) + 8 * (pp & 1);
            const tw_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tw_s16x4*)(img + a0));
            const tw_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tw_s16x4*)(img + a1));
            const tw_s16x8 j8 = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dyf, __builtin_bit_cast(bf16x8, j8), acc[t], 0, 0, 0);
        }
    }
    // the four waves' partials, added in wave order: lane (i, q) holds dW[n = 4 q + r][k = kc0 + 16 t + i]
    __syncthreads();
    float* const red = (float*)smem;                                   // [4 waves][16][KC], over the images
    float* const dbr = (float*)(smem + 4 * IMG);                       // [4 waves][4 q][16]
#pragma unroll
    for (int t = 0; t < TILES; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(wave * 16 + 4 * q + r) * KC + 16 * t + i] = acc[t][r];
    dbr[(wave * 4 + q) * 16 + i] = dbacc;
    __syncthreads();
    float* const out = p.out + (size_t)blockIdx.x * p.pstride;
    for (int e = tid; e < 16 * KC; e += 256) {
        const int n = e / KC, k = e - n * KC;
        if (n < p.N) out[(size_t)n * p.ldo + kc0 + k] = ((red[e] + red[16 * KC + e]) + red[32 * KC + e]) + red[48 * KC + e];
    }
    if (blockIdx.y == 0 && tid < 16) {                                 // columns >= N hold zeros: their fragments were zero
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) v += dbr[w * 16 + tid];
        (p.dbout + (size_t)blockIdx.x * p.pstride)[tid] = v;
    }
}

// dW and db from the P partials ([N * K + 16] floats each, pstride apart): element E of group g = tid >> 4 sums partials
// [g * per, (g + 1) * per) in ascending order, then the 16 group sums are added in ascending order.
__global__ __launch_bounds__(256) void thin_wgrad_reduce_kernel(const float* parts, long pstride, int P, int N, int K, float* dW, long ldc, float* db) {
    __shared__ float red[TW_SLICES][16];
    const int g = threadIdx.x >> 4, e = threadIdx.x & 15;
    const long total = (long)N * K + 16, E = (long)blockIdx.x * 16 + e;
    const int per = (P + TW_SLICES - 1) / TW_SLICES;
    const int b0 = g * per, b1 = min(b0 + per, P);
    float v = 0.f;
    if (E < total)
        for (int b = b0; b < b1; ++b) v += parts[(size_t)b * pstride + E];
    red[g][e] = v;
    __syncthreads();
    if (g == 0 && E < total) {
        v = red[0][e];
#pragma unroll
        for (int s = 1; s < TW_SLICES; ++s) v += red[s][e];
        if (E < (long)N * K) {
            const int n = (int)(E / K), k = (int)(E - (long)n * K);
            dW[(size_t)n * ldc + k] = v;
        } else {
            db[E - (long)N * K] = v;
        }
    }
}

template <bool XF32, int KC>
void tw_launch(const ThinWgradArgs& p, long P, hipStream_t stream) {
    constexpr int LDS = 4 * ((KC + 127) / 128 * 8192) + 1024;
    if (LDS > 65536) (void)hipFuncSetAttribute((const void*)thin_wgrad_kernel<XF32, KC>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    hipLaunchKernelGGL((thin_wgrad_kernel<XF32, KC>), dim3((unsigned)P, (unsigned)(p.K / KC)), dim3(256), LDS, stream, p);
}

int thin_wgrad_launch(const void* A, const void* B, void* C, const float* bias, const float* extra, int M, int N, int K, int lda, int ldb, int ldc,
                      int splits, int group, int flags, hipStream_t stream) {
    const int f32 = flags & 1, R = group;
    const char* who = "cs_gemm_nt (thin weight gradient, epilogue 12)";
    // Code 12 exists only WITH a workspace: a call without one is answered as before this form existed -- an unknown epilogue -- so that
    // a caller written against the library of epilogues 0 .. 11 sees the refusal it knows, whatever else its arguments hold.
    CS_CHECK_ARG(extra != nullptr, "cs_gemm_nt: unknown epilogue 12 without a workspace (the thin weight gradient needs its fp32 workspace in `extra`)");
    CS_CHECK_ARG(A && B && C && M > 0 && N >= 1 && N <= THIN_MAX_N && K > 0 && K % 64 == 0,
                 "%s: M=%d > 0, 1 <= N=%d <= 16, K=%d a positive multiple of 64, no NULL operand", who, M, N, K);
    CS_CHECK_ARG(splits == 1, "%s: splits=%d, the thin forms have no split-K", who, splits);
    CS_CHECK_ARG(((uintptr_t)extra % 16) == 0, "%s: `extra` is the fp32 workspace, 16-byte aligned", who);
    CS_CHECK_ARG(R >= 0 && (R == 0 || M % R == 0), "%s: group=%d is 0 (rows) or the pixels per image, a divisor of M=%d", who, R, M);
    CS_CHECK_ARG(ldb >= K && ldb % (f32 ? 4 : 8) == 0 && ((uintptr_t)B % 16) == 0,
                 "%s: the X rows need a stride=%d >= K=%d that keeps 16-byte rows (%% %d) and a 16-byte aligned base", who, ldb, K, f32 ? 4 : 8);
    CS_CHECK_ARG(ldc >= K && ldc % 4 == 0 && ((uintptr_t)C % 16) == 0, "%s: dW is fp32 [N, K] with ldc=%d >= K=%d, ldc %% 4 == 0, 16-byte aligned", who,
                 ldc, K);
    CS_CHECK_ARG(((uintptr_t)A % 4) == 0, "%s: dY must be 4-byte aligned", who);
    if (R == 0) {
        CS_CHECK_ARG(lda >= N, "%s: rows form, stride=%d below N=%d", who, lda, N);
        CS_CHECK_ARG(bias == nullptr, "%s: rows form has one dY block (bias must be NULL)", who);
    } else {
        CS_CHECK_ARG(lda >= 1 && lda <= N, "%s: planes form, split s=%d outside [1, N=%d]", who, lda, N);
        CS_CHECK_ARG((bias != nullptr) == (lda < N) && ((uintptr_t)bias % 4) == 0,
                     "%s: planes form, a 4-byte aligned second dY block (bias) exactly when s=%d < N=%d", who, lda, N);
    }
    long P = ((long)M + TW_WG_ROWS - 1) / TW_WG_ROWS;
    const long cap = (long)TW_BLOCKS_PER_CU * cs_num_cus();
    if (P > cap) P = cap;
    float* ws = (float*)extra;
    ThinWgradArgs p{};
    p.X = B; p.d1 = (const float*)A; p.d2 = bias;
    p.ldx = ldb; p.ldt = R == 0 ? lda : 0;
    p.M = M; p.N = N; p.K = K; p.R = R;
    p.s = R == 0 ? N : lda;
    p.vec = R > 0 && R % 8 == 0 && ((uintptr_t)A % 16) == 0 && ((uintptr_t)bias % 16) == 0;
    p.tiles = ((long)M + 31) / 32;
    if (P == 1) {
        p.out = (float*)C; p.ldo = ldc; p.dbout = ws; p.pstride = 0;
    } else {
        p.pstride = (long)N * K + 16;
        p.out = ws + 16; p.ldo = K; p.dbout = ws + 16 + (size_t)N * K;
    }
    if (K % 256 == 0) {
        if (f32) tw_launch<true, 256>(p, P, stream);
        else tw_launch<false, 256>(p, P, stream);
    } else {
        if (f32) tw_launch<true, 64>(p, P, stream);
        else tw_launch<false, 64>(p, P, stream);
    }
    CS_LAUNCH_CHECK();
    if (P > 1) {
        const long total = (long)N * K + 16;
        hipLaunchKernelGGL(thin_wgrad_reduce_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, stream, ws + 16, p.pstride, (int)P, N, K,
                           (float*)C, (long)ldc, ws);
        CS_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

// cs_gemm_nt's argument list, epi 10 / 11 / 12 (the header states the packing).  Every check comes before the launch.
int cs_thin_launch(const void* A, const void* B, void* C, const float* bias, const float* extra, int M, int N, int K, int lda, int ldb, int ldc,
                   int epi, int splits, int group, int flags, hipStream_t stream) {
    if (epi == EPI_THIN_WGRAD) return thin_wgrad_launch(A, B, C, bias, extra, M, N, K, lda, ldb, ldc, splits, group, flags, stream);
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
