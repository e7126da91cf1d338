// 3 x 3 convolutions (stride 1, padding 1) on channel-last bf16 maps for the detector heads (gfx950).  Contract: include/clipself_conv.h.
//
//   y[p, co] = bias[co] + sum_{t, ci} x[p shifted by tap t, ci] * Wg[co, t*Cin + ci]       M = N*H*W rows, Cout columns, K = 9*Cin
//
// csc_conv3x3 is gemm_nt_kernel's lockstep schedule (gemm.hip) with a gathered A operand: K is ordered (tap, input channel) and
// Cin % 64 == 0, so a BK = 64 K tile lies inside one tap and its A rows are the rows of the map shifted by (ky-1)*W + (kx-1).  A lane's
// source row (lane_source / source_rows of gemm_common.h) is decomposed into (y, x) once per M tile; per K tile the tap gives one
// wave-uniform element offset and a per-lane in-range predicate, and a lane whose tap falls outside the image points its 16-byte
// global_load_lds at a zero-filled device array.  The LDS image is therefore exactly the one gemm_nt_kernel builds from an explicit
// im2col matrix, and the MFMA loop is the same.  B (the packed weights) is staged as there (stage_tile).
//
// Tile: 256 x 256 x 64, 8 waves (2 x 4, 128 x 64 per wave), two 64 KiB stages = 128 KiB LDS, one workgroup per CU.  Cout of every
// detector convolution is 256, so one N tile covers the whole weight matrix: each gathered A tile (the expensive operand -- nine times
// the map's bytes over the K loop, served from L2 after the first tap) is fetched once per M tile and never re-fetched for another N
// tile, and per MFMA the LDS traffic is the lowest of the three gemm_nt shapes.  (registers, LDS, occupancy.)
//
// csc_im2col3x3 writes rows of the explicit matrix: the B operand of the weight gradient (cs_gemm_wgrad_tn) and the second forward route.
#include "gemm_common.h"
#include "../../include/clipself_conv.h"

namespace {

// what an out-of-image tap reads: chunk c of a lane fetches bytes [16c, 16c + 16), c < 8
static __device__ __attribute__((aligned(128))) unsigned int csc_zero_row[64];

struct ConvArgs {
    GemmArgs g;        // A = map rows, B = Wg, C = y; M = N*H*W, N = Cout, K = 9*Cin; lda / ldb / ldc = ldx / ldw / ldy; tiles_m, tiles_n, gm
    int H, W;
    int kpt;           // K tiles per tap = Cin / 64
};

constexpr int CV_BM = 256, CV_BN = 256, CV_WM = 2, CV_WN = 4;
constexpr int CV_EP_LD = 68;                          // fp32 row stride of the epilogue slab (64 + 4 pad)
constexpr int CV_EP_BYTES = 32 * CV_EP_LD * 4;        // 32 rows per wave slab
constexpr size_t CV_LDS = (size_t)2 * (CV_BM + CV_BN) * BK * 2;

template <bool OUT_BF16>
__global__ __launch_bounds__(CV_WM * CV_WN * 64) void conv3x3_kernel(ConvArgs q) {
    constexpr int BM = CV_BM, BN = CV_BN, WM = CV_WM, WN = CV_WN;
    constexpr int NW = WM * WN;
    constexpr int TM = BM / WM, TN = BN / WN;           // wave tile
    constexpr int FM = TM / 32, FN = TN / 32;
    constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE = A_BYTES + B_BYTES;
    constexpr int A_INSTR = BM / 8 / NW, B_INSTR = BN / 8 / NW;
    static_assert(FN == 2 && (size_t)NW * CV_EP_BYTES <= CV_LDS, "epilogue slabs: 64-column wave tiles inside the operand buffers");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const GemmArgs& p = q.g;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave - wm * WN;
    const int hf = lane >> 5, l31 = lane & 31;
    int tm, tn;
    tile_of_block(p, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;

    int arow[A_INSTR], achk[A_INSTR], brow[B_INSTR], bchk[B_INSTR];
    source_rows<EPI_F32, BM, BN, NW, A_INSTR, B_INSTR>(p, wave, lane, m0, n0, tn, arow, achk, brow, bchk);   // rows clamped to M - 1 / N - 1

    // once per M tile: the lane's source rows as (y, x) of their image, and the address of their centre tap
    const __bf16* abase[A_INSTR];
    const __bf16* azero[A_INSTR];
    int ay[A_INSTR], ax[A_INSTR];
    const int HW = q.H * q.W;
#pragma unroll
    for (int i = 0; i < A_INSTR; ++i) {
        const int rem = arow[i] - (arow[i] / HW) * HW;
        ay[i] = rem / q.W;
        ax[i] = rem - ay[i] * q.W;
        abase[i] = p.A + (size_t)arow[i] * p.lda + achk[i] * 8;
        azero[i] = (const __bf16*)csc_zero_row + achk[i] * 8;
    }

    // per K tile: tap (ky, kx) and channel block cb, wave-uniform; counters of the next tile to stage
    const int ktiles = p.K / BK;
    int s_tap = 0, s_cb = 0;
    auto stage_a = [&](char* lds_tile) {
        const int ky = s_tap / 3, kx = s_tap - ky * 3;
        const int dy = ky - 1, dx = kx - 1;
        const long shift = ((long)dy * q.W + dx) * (long)p.lda + (long)s_cb * BK;      // elements, may be negative
#pragma unroll
        for (int i = 0; i < A_INSTR; ++i) {
            const bool ok = (unsigned)(ay[i] + dy) < (unsigned)q.H && (unsigned)(ax[i] + dx) < (unsigned)q.W;
            const __bf16* g = ok ? abase[i] + shift : azero[i];
            char* dst = lds_tile + (wave * A_INSTR + i) * 1024;                         // wave-uniform
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                             (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
        }
        if (++s_cb == q.kpt) { s_cb = 0; ++s_tap; }
    };

    f32x16 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    stage_a(smem);
    stage_tile<B_INSTR, true>(p.B, p.ldb, 0, smem + A_BYTES, wave * B_INSTR, lane, brow, bchk);
    // fragment addressing: row = base + l31 with base a multiple of 32 -> (row>>1)&15 == l31>>1, row&1 == l31&1
    const int a_base = ((wm * TM + l31) >> 1) << 8;
    const int b_base = ((wn * TN + l31) >> 1) << 8;
    const int par8 = (l31 & 1) << 3, sw = l31 >> 1;
    int cur = 0;
    for (int kt = 0; kt < ktiles; ++kt) {
        __syncthreads();            // tile kt landed (the barrier drains the LDS-DMA queue); buffer cur^1 is free
        if (kt + 1 < ktiles) {
            char* nxt = smem + (cur ^ 1) * STAGE;
            stage_a(nxt);
            stage_tile<B_INSTR, true>(p.B, p.ldb, (kt + 1) * BK, nxt + A_BYTES, wave * B_INSTR, lane, brow, bchk);
        }
        const char* la = smem + cur * STAGE + a_base;
        const char* lb = smem + cur * STAGE + A_BYTES + b_base;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int off = ((par8 | (ks * 2 + hf)) ^ sw) << 4;
            bf16x8 a[FM], b[FN];
#pragma unroll
            for (int i = 0; i < FM; ++i) a[i] = *(const bf16x8*)(la + i * (16 * 256) + off);
#pragma unroll
            for (int j = 0; j < FN; ++j) b[j] = *(const bf16x8*)(lb + j * (16 * 256) + off);
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        cur ^= 1;
    }
    __syncthreads();                                    // every wave is done reading the operand buffers

    // Epilogue through a wave-private LDS slab [32][CV_EP_LD] fp32 (a wave's DS operations execute in order: no workgroup barrier):
    // 16 lanes per row, 4 consecutive columns per lane -> 16-byte (fp32) / 8-byte (bf16) row-contiguous stores.
    float* slab = (float*)(smem + wave * CV_EP_BYTES);
    const int rrow = lane >> 4, rcol = (lane & 15) * 4;
    const int col = n0 + wn * TN + rcol;
    const bool colok = col < p.N;                       // Cout % 8 == 0: a group of four columns is inside or outside as a whole
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.bias && colok) bv = *(const float4*)(p.bias + col);
#pragma unroll
    for (int i = 0; i < FM; ++i) {
        const int row_base = m0 + wm * TM + i * 32;
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) slab[mfma32_row(e, lane) * CV_EP_LD + j * 32 + l31] = acc[i][j][e];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (colok) {
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int rl = rrow + it * 4, row = row_base + rl;
                if (row >= p.M) continue;
                const float4 s = *(const float4*)(slab + rl * CV_EP_LD + rcol);
                const float v[4] = {s.x + bv.x, s.y + bv.y, s.z + bv.z, s.w + bv.w};
                if (OUT_BF16) {
                    U64 ob;
#pragma unroll
                    for (int t = 0; t < 4; ++t) ob.e[t] = f2bf(v[t]);
                    *(uint2*)((__bf16*)p.C + (size_t)row * p.ldc + col) = ob.u;
                } else {
                    *(float4*)((float*)p.C + (size_t)row * p.ldc + col) = make_float4(v[0], v[1], v[2], v[3]);
                }
            }
        }
        if (i + 1 < FM) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // slab reads done before the next block rewrites it
    }
}

// A workgroup writes IM_ROWS rows of the explicit matrix.  A thread owns one (row, 16-byte channel group) at a time and writes its nine
// taps: the row is decomposed once (three 32-bit divisions per nine stores -- one division chain per store makes the kernel VALU-bound),
// the nine loads are independent, and consecutive lanes write consecutive 16-byte pieces of a tap's Cin-wide segment.
constexpr int IM_ROWS = 32;
__global__ __launch_bounds__(256) void im2col3x3_kernel(const __bf16* __restrict__ x, long ldx, __bf16* __restrict__ cols, long ldc, int row0,
                                                        int rows, int H, int W, int Cin) {
    const int c8n = Cin >> 3;
    const int r0 = blockIdx.x * IM_ROWS;
    const int total = min(IM_ROWS, rows - r0) * c8n;
    const int HW = H * W;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int rl = i / c8n, c8 = i - rl * c8n;
        const int r = r0 + rl, prow = row0 + r;                          // prow < N*H*W <= CSC_MAX_ROWS
        const int pix = prow % HW;
        const int y = pix / W, xx = pix - y * W;
        const __bf16* src = x + (long)prow * ldx + c8 * 8;
        __bf16* dst = cols + (long)r * ldc + c8 * 8;
        uint4 v[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int dy = t / 3 - 1, dx = t % 3 - 1;
            v[t] = make_uint4(0u, 0u, 0u, 0u);
            if ((unsigned)(y + dy) < (unsigned)H && (unsigned)(xx + dx) < (unsigned)W) v[t] = *(const uint4*)(src + ((long)dy * W + dx) * ldx);
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) *(uint4*)(dst + (long)t * Cin) = v[t];
    }
}

// N*H*W, or -1 when it passes CSC_MAX_ROWS
long conv_rows(int N, int H, int W) {
    const long nh = (long)N * H;
    if (nh > CSC_MAX_ROWS || nh * W > CSC_MAX_ROWS) return -1;
    return nh * W;
}

}  // namespace

extern "C" int csc_conv3x3(const void* x, long ldx, const void* wg, long ldw, const float* bias, void* y, long ldy, int out_bf16, int N, int H,
                           int W, int Cin, int Cout, hipStream_t stream) {
    CS_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, "csc_conv3x3: empty problem N=%d H=%d W=%d Cin=%d Cout=%d", N, H, W, Cin, Cout);
    if (Cin % 64 != 0 || Cout % 8 != 0) return 1;
    const long M = conv_rows(N, H, W);
    CS_CHECK_ARG(M > 0, "csc_conv3x3: N*H*W must not pass %ld rows", (long)CSC_MAX_ROWS);
    CS_CHECK_ARG(Cin <= (1 << 24) && Cout <= (1 << 24), "csc_conv3x3: more than 2^24 channels");
    CS_CHECK_ARG(x != nullptr && wg != nullptr && y != nullptr && ((uintptr_t)x % 16) == 0 && ((uintptr_t)wg % 16) == 0 && ((uintptr_t)y % 16) == 0,
                 "csc_conv3x3: x, wg and y must be 16-byte aligned");
    CS_CHECK_ARG(ldx >= Cin && ldx % 8 == 0 && ldw >= 9L * Cin && ldw % 8 == 0 && ldy >= Cout && ldy % 4 == 0 && ldx < 0x7fffffffL &&
                     ldw < 0x7fffffffL && ldy < 0x7fffffffL,
                 "csc_conv3x3: row strides ldx >= Cin, ldw >= 9*Cin (multiples of 8), ldy >= Cout (multiple of 4), each below 2^31");
    CS_CHECK_ARG(bias == nullptr || ((uintptr_t)bias % 16) == 0, "csc_conv3x3: bias must be 16-byte aligned");
    CS_CHECK_ARG(out_bf16 == 0 || out_bf16 == 1, "csc_conv3x3: out_bf16 is 0 (fp32) or 1 (bf16)");
    ConvArgs q{};
    GemmArgs& a = q.g;
    a.A = (const __bf16*)x; a.B = (const __bf16*)wg; a.C = y; a.bias = bias;
    a.M = (int)M; a.N = Cout; a.K = 9 * Cin; a.lda = (int)ldx; a.ldb = (int)ldw; a.ldc = (int)ldy;
    a.tiles_m = (a.M + CV_BM - 1) / CV_BM; a.tiles_n = (a.N + CV_BN - 1) / CV_BN; a.gm = 8;
    a.ktiles_per_split = a.K / BK; a.nsplit = 1;
    q.H = H; q.W = W; q.kpt = Cin / BK;
    const long tiles = (long)a.tiles_m * a.tiles_n;
    CS_CHECK_ARG(tiles < 0x7fffffffL, "csc_conv3x3: too many tiles");
    static bool once = ((void)hipFuncSetAttribute((const void*)conv3x3_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CV_LDS),
                        (void)hipFuncSetAttribute((const void*)conv3x3_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CV_LDS), true);
    (void)once;
    const dim3 grid((unsigned)tiles), block(CV_WM * CV_WN * 64);
    if (out_bf16) hipLaunchKernelGGL(conv3x3_kernel<true>, grid, block, CV_LDS, stream, q);
    else hipLaunchKernelGGL(conv3x3_kernel<false>, grid, block, CV_LDS, stream, q);
    CS_LAUNCH_CHECK();
    return 0;
}

extern "C" int csc_im2col3x3(const void* x, long ldx, void* cols, long ldc, long row0, long rows, int N, int H, int W, int Cin,
                             hipStream_t stream) {
    CS_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && Cin >= 1, "csc_im2col3x3: empty problem N=%d H=%d W=%d Cin=%d", N, H, W, Cin);
    if (Cin % 8 != 0) return 1;
    const long M = conv_rows(N, H, W);
    CS_CHECK_ARG(M > 0, "csc_im2col3x3: N*H*W must not pass %ld rows", (long)CSC_MAX_ROWS);
    CS_CHECK_ARG(row0 >= 0 && rows >= 0 && row0 <= M && rows <= M - row0, "csc_im2col3x3: rows [%ld, %ld + %ld) outside the map's %ld rows", row0, row0, rows, M);
    CS_CHECK_ARG(x != nullptr && cols != nullptr && ((uintptr_t)x % 16) == 0 && ((uintptr_t)cols % 16) == 0, "csc_im2col3x3: x and cols must be 16-byte aligned");
    CS_CHECK_ARG(Cin <= (1 << 24) && ldx >= Cin && ldx % 8 == 0 && ldc >= 9L * Cin && ldc % 8 == 0,
                 "csc_im2col3x3: row strides ldx >= Cin, ldc >= 9*Cin, multiples of 8");
    if (rows == 0) return 0;
    hipLaunchKernelGGL(im2col3x3_kernel, dim3((unsigned)((rows + IM_ROWS - 1) / IM_ROWS)), dim3(256), 0, stream, (const __bf16*)x, ldx,
                       (__bf16*)cols, ldc, (int)row0, (int)rows, H, W, Cin);
    CS_LAUNCH_CHECK();
    return 0;
}
