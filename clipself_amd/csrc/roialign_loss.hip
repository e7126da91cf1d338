// RoIAlign(1x1, adaptive sampling, aligned) over the NHWC token map + row-wise cosine distillation loss (fwd/bwd).
//
// Reference call sites:
//   src/open_clip/eva_clip/eva_vit_model.py:625-629,655-664   roi_align(x, boxes*[w,h], (1,1), 1.0, -1, True)[...,0,0]
//   src/training/clipself.py:42-47                              F.normalize both, 1 - mean(sum(s*t))
// The RoIAlign arithmetic itself is torchvision's (absent wheel); algorithm restated in oracle/roi_align_ref.py.
//
// MI355X layout: the student's token map stays token-major [B, Ntok, E] fp32 exactly as the head GEMM wrote it
// (channels contiguous -> every sample row is a coalesced E*4-byte read); there is no NCHW view and no
// .contiguous() copy.  Bilinear weights are separable, so each box first folds its gh x gw sample grid into
// per-row / per-column weights Wy[h], Wx[w] (sequentially, fixed order -> deterministic) and then touches each
// map cell at most once:   pooled = sum_{r,c} Wy[r] Wx[c] F[r,c] / max(gh*gw,1).
#include "cs_common.h"
#include "../../include/clipself_hip.h"

namespace {

constexpr int MAXGRID = 128;   // token grid side limit (1024/8)

// torchvision's per-axis sample handling, float32 like its T=float path
__device__ void axis_weights(float start, float extent, int grid, int size, float* w /*[size]*/) {
    for (int i = 0; i < size; ++i) w[i] = 0.f;
    for (int i = 0; i < grid; ++i) {
        // un-contracted float32 steps (no FMA), same order as torchvision / the numpy oracle
        float c = __fadd_rn(start, __fdiv_rn(__fmul_rn((float)i + 0.5f, extent), (float)grid));
        if (c < -1.0f || c > (float)size) continue;
        if (c <= 0.f) c = 0.f;
        int lo = (int)c, hi;
        if (lo >= size - 1) { hi = lo = size - 1; c = (float)lo; } else { hi = lo + 1; }
        const float l = __fsub_rn(c, (float)lo);
        w[lo] += __fsub_rn(1.f, l);
        w[hi] += l;
    }
}

struct RoiGeom { int b, gh, gw; float inv_count; };

// roi = (image, x0, y0, x1, y1); map coordinate = roi * (sx, sy) - 0.5.  Boxes normalised to [0,1]: (sx, sy) = (gw_map, gh_map), what
// _denormalize_boxes multiplies by; pixel boxes: sx = sy = 1 / featmap_stride (torchvision's spatial_scale).  Thread ty folds the rows'
// weights into Wy, thread tx the columns' into Wx.
// BOUNDED (boxes from an RPN, not from a data loader): a box whose image index is outside [0, B) (B > 0), or whose extent on the map is
// not in (0, 2 * grid side] on both axes -- non-finite coordinates included -- gets gh = gw = 0, image 0 and all-zero weights: an empty
// box, which the callers never walk and never index the map with.
// STRICT: the product roi * scale is rounded before 0.5 is subtracted, as torchvision's `roi * spatial_scale - 0.5` is.  hipcc may contract
// __fmul_rn / __fsub_rn (plain operators in its headers) into one fma, which moves the coordinate by an ulp where the product is inexact
// (1 / 14; a power-of-two scale is exact and both forms agree).  The plain pooling launch keeps the form -- and the bits -- it always had.
__device__ __forceinline__ float mul_rounded(float a, float b) {
    float p = a * b;
    asm volatile("" : "+v"(p));         // no instruction: the product exists as a value of its own, so no fma can absorb it
    return p;
}
template <bool STRICT>
__device__ __forceinline__ float map_coord(float v, float s) {
    return STRICT ? mul_rounded(v, s) - 0.5f : __fsub_rn(__fmul_rn(v, s), 0.5f);
}

template <bool BOUNDED>
__device__ __forceinline__ RoiGeom box_setup(const float* __restrict__ roi, float sx, float sy, int gh_map, int gw_map, int B, float* Wy,
                                             float* Wx, int tid, int ty, int tx) {
    const float x0 = map_coord<BOUNDED>(roi[1], sx), y0 = map_coord<BOUNDED>(roi[2], sy);
    const float x1 = map_coord<BOUNDED>(roi[3], sx), y1 = map_coord<BOUNDED>(roi[4], sy);
    const float rw = __fsub_rn(x1, x0), rh = __fsub_rn(y1, y0);
    RoiGeom g;
    if (BOUNDED) {
        const float bf = roi[0];
        const bool walk = (B <= 0 || (bf >= 0.f && bf < (float)B)) && rh > 0.f && rh <= 2.f * (float)gh_map && rw > 0.f && rw <= 2.f * (float)gw_map;
        g.b = walk ? (int)bf : 0;
        g.gh = walk ? (int)ceilf(rh) : 0;
        g.gw = walk ? (int)ceilf(rw) : 0;
    } else {
        g.b = (int)roi[0];
        g.gh = (int)ceilf(rh);
        g.gw = (int)ceilf(rw);
    }
    const int cnt = g.gh * g.gw;
    g.inv_count = 1.f / (float)(cnt > 1 ? cnt : 1);
    if (tid == ty) axis_weights(y0, rh, g.gh > 0 ? g.gh : 0, gh_map, Wy);
    if (tid == tx) axis_weights(x0, rw, g.gw > 0 ? g.gw : 0, gw_map, Wx);
    return g;
}

// The cells a box touches are a sub-rectangle of the map: the first and one past the last cell of an axis with a weight.
__device__ __forceinline__ void weight_range(const float* W, int size, int& lo, int& hi) {
    lo = 0;
    hi = size;
    while (lo < hi && W[lo] == 0.f) ++lo;
    while (hi > lo && W[hi - 1] == 0.f) --hi;
}

// N consecutive cells of one map row: their loads are issued together (every cell of a box's range is inside the map), the additions
// follow in column order, zero weights skipped
template <int N>
__device__ __forceinline__ void pool_cells(const float* __restrict__ row, const float* Wx, float wy, int c, int E, float4& acc) {
    float w[N];
    float4 v[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        w[j] = wy * Wx[c + j];
        v[j] = *(const float4*)(row + (size_t)(c + j) * E);
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
        if (w[j] == 0.f) continue;
        acc.x += w[j] * v[j].x; acc.y += w[j] * v[j].y; acc.z += w[j] * v[j].z; acc.w += w[j] * v[j].w;
    }
}

// sum_{r,c} Wy[r] Wx[c] F[r, c, ch .. ch+3] over that sub-rectangle, rows outside, zero weights skipped: ONE summation order for every
// kernel that pools (fb = the image's first grid token).  A row is walked in runs of 8, 4 and 1 cells: the order of the additions is the
// columns', whatever the runs.
__device__ __forceinline__ float4 pool_quad(const float* __restrict__ fb, const float* Wy, const float* Wx, int r_lo, int r_hi, int c_lo,
                                            int c_hi, int gw_map, int E, int ch) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = r_lo; r < r_hi; ++r) {
        const float wy = Wy[r];
        if (wy == 0.f) continue;
        const float* row = fb + (size_t)(r * gw_map) * E + ch;
        int c = c_lo;
        for (; c + 8 <= c_hi; c += 8) pool_cells<8>(row, Wx, wy, c, E, acc);
        if (c + 4 <= c_hi) {
            pool_cells<4>(row, Wx, wy, c, E, acc);
            c += 4;
        }
        for (; c < c_hi; ++c) pool_cells<1>(row, Wx, wy, c, E, acc);
    }
    return acc;
}

// feat [B, Ntok, E] f32 (token 0 = CLS, skipped), rois [K,5], pooled [K,E] f32
__global__ __launch_bounds__(256) void roialign_fwd_kernel(const float* __restrict__ feat, const float* __restrict__ rois,
                                                           float* __restrict__ pooled, int Ntok, int gh_map, int gw_map, int E, int tok_off) {
    __shared__ float Wy[MAXGRID], Wx[MAXGRID];
    const int k = blockIdx.x, tid = threadIdx.x;
    const RoiGeom g = box_setup<false>(rois + (size_t)k * 5, (float)gw_map, (float)gh_map, gh_map, gw_map, 0, Wy, Wx, tid, 0, 64);
    __syncthreads();
    const bool empty = g.gh <= 0 || g.gw <= 0;
    const float* fb = feat + ((size_t)g.b * Ntok + tok_off) * E;
    // walk the sub-rectangle, not the whole map (the recipe's 64 x 64 grid: 4096 cells per box and thread, ~250 of them with a weight; zero
    // weights inside the range are still skipped, so the additions and their order are unchanged)
    int r_lo, r_hi, c_lo, c_hi;
    weight_range(Wy, gh_map, r_lo, r_hi);
    weight_range(Wx, gw_map, c_lo, c_hi);
    for (int ch = tid * 4; ch < E; ch += 1024) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!empty) acc = pool_quad(fb, Wy, Wx, r_lo, r_hi, c_lo, c_hi, gw_map, E, ch);
        *(float4*)(pooled + (size_t)k * E + ch) = make_float4(acc.x * g.inv_count, acc.y * g.inv_count, acc.z * g.inv_count, acc.w * g.inv_count);
    }
}

// ---- open-vocabulary box scores (F-ViT/models/fvit_head.py:63-70,108-119,267-277,337-345) --------------------------------------
// One workgroup scores G consecutive boxes (of any images) in four phases separated by workgroup barriers:
//   1. geometry + axis weights of the G boxes (box_setup<true>, two threads per box);
//   2. pooling: one thread per (box, 4 channels) -- at E = 512 two boxes per pass, no idle half -- with pool_quad's summation order;
//      v goes to LDS and, when asked for, to `pooled`;
//   3. v^ = v / max(|v|, 1e-12) in place, one wave per box;
//   4. logits z[g][c] = vlm_temp * <v^_g, A_c> on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: exact fp32 products, an fp32 fma chain
//      in a fixed k order): a wave takes 16 class rows at a time against the group's boxes (columns past G are zero), so a row of A is
//      fetched once per group, 64 contiguous bytes per lane quartet; then per box (one wave each) the two log-sum-exps and the blend in
//      the log domain.
// LDS: P [G][E + 4] pooled rows (the pad spreads the 16 boxes' rows over the banks) | Z [G][Cp] logits | W [G][2][MAXGRID] axis weights |
// geometry.  fp32 throughout, no atomics, plain loads and stores, every sum in a fixed order.
struct BoxGeo { int b, r_lo, r_hi, c_lo, c_hi, empty; float inv_count; int pad; };
constexpr int LOGIT_AHEAD = 8;                            // 16-channel steps of a class row whose loads a lane issues before their MFMAs

__host__ __device__ constexpr size_t box_scores_lds(int G, int E, int Cp) { return ((size_t)G * (E + 4 + Cp + 2 * MAXGRID)) * 4 + (size_t)G * sizeof(BoxGeo); }

template <int G>
__global__ __launch_bounds__(256) void box_scores_kernel(const float* __restrict__ feat, const float* __restrict__ rois, float* __restrict__ pooled,
                                                         int K, int B, int Ntok, int gh_map, int gw_map, int E, int tok_off, float sx, float sy,
                                                         const float* __restrict__ A, int C, int Cp, float vlm_temp,
                                                         const float* __restrict__ det, long ldd, const float* __restrict__ expo,
                                                         float* __restrict__ scores, long lds) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Ep = E + 4;
    float* P = (float*)smem;                              // [G][Ep]
    float* Z = P + (size_t)G * Ep;                        // [G][Cp]
    float* W = Z + (size_t)G * Cp;                        // [G][2][MAXGRID]
    BoxGeo* geo = (BoxGeo*)(W + G * 2 * MAXGRID);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int k0 = blockIdx.x * G;

    // 1. threads 16g (rows) and 16g + 8 (columns) set box g up; a slot past K is an empty box
    if ((tid & 7) == 0 && (tid >> 4) < G) {
        const int g = tid >> 4, k = k0 + g;
        float* Wy = W + g * 2 * MAXGRID;
        float* Wx = Wy + MAXGRID;
        const bool rows = (tid & 8) == 0;
        if (k < K) {
            const RoiGeom rg = box_setup<true>(rois + (size_t)k * 5, sx, sy, gh_map, gw_map, B, Wy, Wx, tid, 16 * g, 16 * g + 8);
            if (rows) {
                geo[g].b = rg.b;
                geo[g].empty = rg.gh <= 0 || rg.gw <= 0;
                geo[g].inv_count = rg.inv_count;
                weight_range(Wy, gh_map, geo[g].r_lo, geo[g].r_hi);
            } else {
                weight_range(Wx, gw_map, geo[g].c_lo, geo[g].c_hi);
            }
        } else if (rows) {
            geo[g].b = 0; geo[g].empty = 1; geo[g].inv_count = 1.f; geo[g].r_lo = geo[g].r_hi = 0;
        } else {
            geo[g].c_lo = geo[g].c_hi = 0;
        }
    }
    __syncthreads();

    // 2. pooling
    const int Q = E >> 2;
    for (int it = tid; it < G * Q; it += 256) {
        const int g = it / Q, ch = (it - g * Q) * 4, k = k0 + g;
        const BoxGeo bg = geo[g];
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!bg.empty) {
            const float* Wy = W + g * 2 * MAXGRID;
            acc = pool_quad(feat + ((size_t)bg.b * Ntok + tok_off) * E, Wy, Wy + MAXGRID, bg.r_lo, bg.r_hi, bg.c_lo, bg.c_hi, gw_map, E, ch);
        }
        const float4 v = make_float4(acc.x * bg.inv_count, acc.y * bg.inv_count, acc.z * bg.inv_count, acc.w * bg.inv_count);
        *(float4*)(P + (size_t)g * Ep + ch) = v;
        if (pooled != nullptr && k < K) *(float4*)(pooled + (size_t)k * E + ch) = v;
    }
    if (C == 0) return;                                   // pooling only (workgroup-uniform)
    __syncthreads();

    // 3. F.normalize(v, dim=-1): a lane rewrites the elements it read
    for (int g = wv; g < G; g += 4) {
        float* p = P + (size_t)g * Ep;
        float ss = 0.f;
        for (int e = lane * 4; e < E; e += 256) {
            const float4 v = *(const float4*)(p + e);
            ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
        const float d = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
        for (int e = lane * 4; e < E; e += 256) {
            const float4 v = *(const float4*)(p + e);
            *(float4*)(p + e) = make_float4(v.x / d, v.y / d, v.z / d, v.w / d);
        }
    }
    __syncthreads();

    // 4a. logits, D[class 16t + 4q + r][box i] = sum_e A[class 16t + i][e] * P[box i][e].  Operand maps of the 16x16x4 fp32 MFMA: lane l
    // gives A[row l & 15][k = l >> 4] and B[k = l >> 4][column l & 15] and receives D[row 4 (l >> 4) + r][column l & 15] in register r.
    // A lane loads 4 consecutive e of its class row and of its box row; MFMA j of a step takes element j of both, so that k = q stands
    // for e = e0 + 4q + j on both sides.  Two accumulators keep the matrix pipe issuing; their sum is the logit.
    {
        const int i = lane & 15, q = lane >> 4;
        const float* pb = P + (size_t)i * Ep;              // read only where i < G
        for (int t = wv; t * 16 < C; t += 4) {             // wave-uniform
            const int ca = min(t * 16 + i, C - 1);         // class rows past C repeat the last one; their results are not stored
            const float* a = A + (size_t)ca * E;
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
            const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
            int e0 = 0;
            for (; e0 + 16 * LOGIT_AHEAD <= E; e0 += 16 * LOGIT_AHEAD) {       // whole runs: LOGIT_AHEAD class-row loads in flight per lane
                float4 av[LOGIT_AHEAD], bv[LOGIT_AHEAD];
#pragma unroll
                for (int s = 0; s < LOGIT_AHEAD; ++s) {
                    av[s] = *(const float4*)(a + e0 + 16 * s + 4 * q);
                    bv[s] = i < G ? *(const float4*)(pb + e0 + 16 * s + 4 * q) : zero;
                }
#pragma unroll
                for (int s = 0; s < LOGIT_AHEAD; ++s) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s].x, bv[s].x, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s].y, bv[s].y, acc1, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s].z, bv[s].z, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s].w, bv[s].w, acc1, 0, 0, 0);
                }
            }
            for (; e0 < E; e0 += 16) {                     // the rest, step by step in the same k order
                const int e = e0 + 4 * q;
                float4 av = zero, bv = zero;
                if (e < E) {                               // E % 16 != 0: the last step's upper quartets contribute zeros
                    av = *(const float4*)(a + e);
                    if (i < G) bv = *(const float4*)(pb + e);
                }
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc1, 0, 0, 0);
            }
            if (i < G) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = t * 16 + 4 * q + r;
                    if (c < C) Z[(size_t)i * Cp + c] = vlm_temp * (acc0[r] + acc1[r]);
                }
            }
        }
    }
    __syncthreads();

    // 4b. out = exp((1 - w) * log_softmax(det) + w * log_softmax(z)), one wave per box
    for (int g = wv; g < G; g += 4) {
        const int k = k0 + g;
        if (k >= K) break;
        const float* z = Z + (size_t)g * Cp;
        float m = -INFINITY, s = 0.f;
        for (int c = lane; c < C; c += 64) m = fmaxf(m, z[c]);
        m = wave_max(m);
        for (int c = lane; c < C; c += 64) s += expf(z[c] - m);
        const float lse_v = m + logf(wave_sum(s));
        float* out = scores + (size_t)k * lds;
        if (det == nullptr) {
            for (int c = lane; c < C; c += 64) out[c] = expf(z[c] - lse_v);
            continue;
        }
        const float* d = det + (size_t)k * ldd;
        m = -INFINITY;
        s = 0.f;
        for (int c = lane; c < C; c += 64) m = fmaxf(m, d[c]);
        m = wave_max(m);
        for (int c = lane; c < C; c += 64) s += expf(d[c] - m);
        const float lse_d = m + logf(wave_sum(s));
        for (int c = lane; c < C; c += 64) {
            const float w = expo[c];
            out[c] = expf((1.f - w) * (d[c] - lse_d) + w * (z[c] - lse_v));
        }
    }
}

// Weight of map cell `cell` along one axis: the same samples, in the same order, as axis_weights() adds into w[cell] -> bit-identical to
// the forward's Wy[cell] / Wx[cell].
__device__ float axis_weight_at(float start, float extent, int grid, int size, int cell) {
    float w = 0.f;
    for (int i = 0; i < grid; ++i) {
        float c = __fadd_rn(start, __fdiv_rn(__fmul_rn((float)i + 0.5f, extent), (float)grid));
        if (c < -1.0f || c > (float)size) continue;
        if (c <= 0.f) c = 0.f;
        int lo = (int)c, hi;
        if (lo >= size - 1) { hi = lo = size - 1; c = (float)lo; } else { hi = lo + 1; }
        const float l = __fsub_rn(c, (float)lo);
        if (lo == cell) w += __fsub_rn(1.f, l);
        if (hi == cell) w += l;
    }
    return w;
}

// Backward as a GATHER: one workgroup owns RB_CELLS consecutive cells of one grid row of one image and adds up, box by box in ascending
// box order, what every box of that image sends to them:  dfeat[b, r, c, :] += sum_k Wy_k[r] Wx_k[c] dpooled[k, :] / count_k.
// No atomics, a fixed summation order -> the gradient is bit-reproducible (torchvision's backward, and round 2's scatter kernel, add with
// float atomics in arrival order: 2.8e-4 relative run-to-run differences on the step's gradients).
constexpr int RB_CELLS = 16, RB_EPT = 4;          // cells per workgroup; channels per thread (256 * RB_EPT channels per workgroup, wider maps: more workgroups)
__global__ __launch_bounds__(256) void roialign_bwd_gather_kernel(const float* __restrict__ dpooled, const float* __restrict__ rois,
                                                                  float* __restrict__ dfeat, int K, int Ntok, int gh_map, int gw_map, int E,
                                                                  int tok_off, int cell_groups) {
    __shared__ int list[256];
    __shared__ int wave_cnt[4];
    __shared__ float Wxs[RB_CELLS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int cg = blockIdx.x % cell_groups, ch0 = (blockIdx.x / cell_groups) * (256 * RB_EPT);      // cell group, first channel of this workgroup
    const int c0 = cg * RB_CELLS, r = blockIdx.y, b = blockIdx.z;
    float acc[RB_CELLS][RB_EPT];
#pragma unroll
    for (int c = 0; c < RB_CELLS; ++c)
#pragma unroll
        for (int j = 0; j < RB_EPT; ++j) acc[c][j] = 0.f;
    for (int k0 = 0; k0 < K; k0 += 256) {
        // ordered compaction of the boxes k0 .. k0+255 that belong to image b
        const int k = k0 + tid;
        const bool mine = k < K && (int)rois[(size_t)k * 5] == b;
        const unsigned long long m = __ballot(mine);
        if (lane == 0) wave_cnt[wv] = __popcll(m);
        __syncthreads();
        int base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wv) base += wave_cnt[w];
            total += wave_cnt[w];
        }
        if (mine) list[base + __popcll(m & ((1ull << lane) - 1ull))] = k;
        __syncthreads();
        for (int n = 0; n < total; ++n) {                  // workgroup-uniform control flow below: every value comes from the box record
            const float* roi = rois + (size_t)list[n] * 5;
            const float x0 = __fsub_rn(__fmul_rn(roi[1], (float)gw_map), 0.5f), y0 = __fsub_rn(__fmul_rn(roi[2], (float)gh_map), 0.5f);
            const float x1 = __fsub_rn(__fmul_rn(roi[3], (float)gw_map), 0.5f), y1 = __fsub_rn(__fmul_rn(roi[4], (float)gh_map), 0.5f);
            const float rw = __fsub_rn(x1, x0), rh = __fsub_rn(y1, y0);
            const int gh = (int)ceilf(rh), gw = (int)ceilf(rw);
            if (gh <= 0 || gw <= 0) continue;
            const float wy = axis_weight_at(y0, rh, gh, gh_map, r);
            if (wy == 0.f) continue;
            const int cnt = gh * gw;
            const float inv_count = 1.f / (float)(cnt > 1 ? cnt : 1);
            __syncthreads();                               // the previous box's Wxs has been consumed
            if (tid < RB_CELLS) Wxs[tid] = c0 + tid < gw_map ? axis_weight_at(x0, rw, gw, gw_map, c0 + tid) : 0.f;
            __syncthreads();
            float gv[RB_EPT];
#pragma unroll
            for (int j = 0; j < RB_EPT; ++j) {
                const int ch = ch0 + tid + 256 * j;
                gv[j] = ch < E ? dpooled[(size_t)list[n] * E + ch] * inv_count : 0.f;
            }
#pragma unroll
            for (int c = 0; c < RB_CELLS; ++c) {
                const float w = wy * Wxs[c];
                if (w != 0.f) {
#pragma unroll
                    for (int j = 0; j < RB_EPT; ++j) acc[c][j] += w * gv[j];
                }
            }
        }
        __syncthreads();                                   // list / wave_cnt are rewritten by the next chunk
    }
#pragma unroll
    for (int c = 0; c < RB_CELLS; ++c) {
        float* cell = dfeat + ((size_t)b * Ntok + tok_off + (size_t)r * gw_map + min(c0 + c, gw_map - 1)) * E;
#pragma unroll
        for (int j = 0; j < RB_EPT; ++j) {
            const int ch = ch0 + tid + 256 * j;
            if (c0 + c < gw_map && ch < E && acc[c][j] != 0.f) cell[ch] += acc[c][j];
        }
    }
}

// ---- cosine loss ----------------------------------------------------------------------------
// per box: cos_k = <s/|s|, t/|t|>  (F.normalize eps 1e-12).  stats[k] = (cos, 1/max(|s|,eps), 1/max(|t|,eps))
__global__ __launch_bounds__(256) void cosine_rows_kernel(const float* __restrict__ s, const float* __restrict__ t, float* __restrict__ stats,
                                                          int K, int E) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;
    float ss = 0.f, tt = 0.f, st = 0.f;
    for (int c = lane * 4; c < E; c += 256) {
        const float4 a = *(const float4*)(s + (size_t)k * E + c), b = *(const float4*)(t + (size_t)k * E + c);
        ss += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
        tt += b.x * b.x + b.y * b.y + b.z * b.z + b.w * b.w;
        st += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
    }
    ss = wave_sum(ss); tt = wave_sum(tt); st = wave_sum(st);
    const float is = 1.f / fmaxf(sqrtf(ss), 1e-12f), it = 1.f / fmaxf(sqrtf(tt), 1e-12f);
    if (lane == 0) { stats[k * 3] = st * is * it; stats[k * 3 + 1] = is; stats[k * 3 + 2] = it; }
}

// loss = weight * (1 - mean_k cos_k); single workgroup, fixed-order tree -> deterministic
__global__ __launch_bounds__(256) void cosine_reduce_kernel(const float* __restrict__ stats, float* __restrict__ loss, int K, float weight) {
    __shared__ float part[256];
    float s = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) s += stats[k * 3];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = weight * (1.f - part[0] / (float)K);
}

// d loss / d s_k = -(weight*gscale/K) * (t_hat - cos_k * s_hat) / |s|
__global__ __launch_bounds__(256) void cosine_bwd_kernel(const float* __restrict__ s, const float* __restrict__ t, const float* __restrict__ stats,
                                                         float* __restrict__ ds, int K, int E, float coef,
                                                         const float* __restrict__ upstream) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)K * E) return;
    if (upstream) coef *= upstream[0];        // d(total)/d(loss) left on the device: no host sync in backward
    const int k = (int)(i / E);
    const float cosv = stats[k * 3], is = stats[k * 3 + 1], it = stats[k * 3 + 2];
    ds[i] = coef * (t[i] * it - cosv * s[i] * is) * is;
}

}  // namespace

// C ABI ------------------------------------------------------------------------------------------
// feat: token-major map [B, Ntok, E] f32; the grid occupies tokens tok_off .. tok_off+gh*gw-1 (tok_off = 1 skips CLS).
// rois [K,5] f32 = (image index, x0, y0, x1, y1) with box coordinates normalised to [0,1] (reference batch contract; box_scale == 0) or
// in pixels, multiplied by box_scale = 1 / featmap_stride (mmdet's bbox2roi layout).  The rest of the contract: include/clipself_hip.h.
namespace {

constexpr size_t BOX_SCORES_MAX_LDS = 160 * 1024;

template <int G>
int box_scores_launch(const float* feat, const float* rois, float* pooled, int K, int B, int Ntok, int grid_h, int grid_w, int E, int tok_off,
                      float sx, float sy, const float* A, int C, int Cp, float vlm_temp, const float* det, long ldd, const float* expo,
                      float* scores, long lds, hipStream_t stream) {
    static bool once = ((void)hipFuncSetAttribute((const void*)box_scores_kernel<G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)BOX_SCORES_MAX_LDS), true);
    (void)once;
    hipLaunchKernelGGL(box_scores_kernel<G>, dim3((K + G - 1) / G), dim3(256), box_scores_lds(G, E, Cp), stream, feat, rois, pooled, K, B, Ntok,
                       grid_h, grid_w, E, tok_off, sx, sy, A, C, Cp, vlm_temp, det, ldd, expo, scores, lds);
    CS_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int cs_roialign_fwd(const float* feat, const float* rois, float* pooled, int K, int Ntok, int grid_h, int grid_w, int E,
                               int tok_off, float box_scale, int B, const float* class_embed, int C, float vlm_temp, const float* det_logits,
                               long ldd, const float* expo, float* scores, long lds, hipStream_t stream) {
    CS_CHECK_ARG(grid_h > 0 && grid_w > 0 && grid_h <= MAXGRID && grid_w <= MAXGRID && E > 0 && E % 4 == 0, "cs_roialign_fwd: bad grid/E");
    CS_CHECK_ARG(tok_off + grid_h * grid_w <= Ntok, "cs_roialign_fwd: grid does not fit the token map");
    CS_CHECK_ARG(K >= 0 && B >= 0 && box_scale >= 0.f && box_scale <= 3.0e38f, "cs_roialign_fwd: K=%d, B=%d, box_scale=%g must be >= 0 and finite", K, B, (double)box_scale);
    if (class_embed == nullptr) {
        CS_CHECK_ARG(scores == nullptr && det_logits == nullptr, "cs_roialign_fwd: scores / det_logits given without class_embed");
        CS_CHECK_ARG(pooled != nullptr || K == 0, "cs_roialign_fwd: pooled is NULL and no scores are asked for");
        C = 0;
    } else {
        CS_CHECK_ARG(C >= 1, "cs_roialign_fwd: C=%d classes (>= 1)", C);
        CS_CHECK_ARG((scores != nullptr || K == 0) && lds >= C, "cs_roialign_fwd: scores is NULL or its row stride lds=%ld < C=%d", lds, C);
        CS_CHECK_ARG(det_logits == nullptr || expo != nullptr, "cs_roialign_fwd: det_logits given without expo (the per-class exponents)");
        CS_CHECK_ARG(det_logits == nullptr || ldd >= C, "cs_roialign_fwd: det_logits row stride ldd=%ld < C=%d", ldd, C);
    }
    const int Cp = (C + 3) & ~3;
    if (class_embed != nullptr)
        CS_CHECK_ARG(box_scores_lds(1, E, Cp) <= BOX_SCORES_MAX_LDS, "cs_roialign_fwd: E=%d + C=%d do not fit one workgroup's LDS", E, C);
    if (K == 0) return 0;
    if (class_embed == nullptr && box_scale == 0.f && B == 0) {      // the distillation path's call: unchecked boxes from the data loader
        hipLaunchKernelGGL(roialign_fwd_kernel, dim3(K), dim3(256), 0, stream, feat, rois, pooled, Ntok, grid_h, grid_w, E, tok_off);
        CS_LAUNCH_CHECK();
        return 0;
    }
    const float sx = box_scale == 0.f ? (float)grid_w : box_scale, sy = box_scale == 0.f ? (float)grid_h : box_scale;
#define BOX_SCORES_GO(G)                                                                                                              \
    return box_scores_launch<G>(feat, rois, pooled, K, B, Ntok, grid_h, grid_w, E, tok_off, sx, sy, class_embed, C, Cp, vlm_temp,     \
                                det_logits, ldd, expo, scores, lds, stream)
    // the largest group whose rows fit: 16 boxes up to E + C = 2292 (OV-LVIS at E = 768: 1972), 8 up to 4852, 4 up to 9972
    if (box_scores_lds(16, E, Cp) <= BOX_SCORES_MAX_LDS) BOX_SCORES_GO(16);
    if (box_scores_lds(8, E, Cp) <= BOX_SCORES_MAX_LDS) BOX_SCORES_GO(8);
    if (box_scores_lds(4, E, Cp) <= BOX_SCORES_MAX_LDS) BOX_SCORES_GO(4);
    BOX_SCORES_GO(1);
#undef BOX_SCORES_GO
}
// dfeat [B, Ntok, E] f32 += the gradient of every box (the caller zeroes it, or accumulates); B = images in the map.  Deterministic: a
// gather per map cell over the image's boxes in ascending box order, no atomics.
extern "C" int cs_roialign_bwd(const float* dpooled, const float* rois, float* dfeat, int K, int B, int Ntok, int grid_h, int grid_w, int E,
                               int tok_off, hipStream_t stream) {
    CS_CHECK_ARG(grid_h > 0 && grid_w > 0 && grid_h <= MAXGRID && grid_w <= MAXGRID, "cs_roialign_bwd: bad grid");
    CS_CHECK_ARG(tok_off + grid_h * grid_w <= Ntok, "cs_roialign_bwd: grid does not fit the token map");
    CS_CHECK_ARG(B > 0 && B <= 65535 && E > 0, "cs_roialign_bwd: B=%d images (1..65535), E=%d channels", B, E);
    if (K == 0) return 0;
    const int cell_groups = (grid_w + RB_CELLS - 1) / RB_CELLS, chunks = (E + 256 * RB_EPT - 1) / (256 * RB_EPT);     // E > 1024 (bigG-class heads): channel chunks
    hipLaunchKernelGGL(roialign_bwd_gather_kernel, dim3(cell_groups * chunks, grid_h, B), dim3(256), 0, stream, dpooled, rois,
                       dfeat, K, Ntok, grid_h, grid_w, E, tok_off, cell_groups);
    CS_LAUNCH_CHECK();
    return 0;
}
// stats: workspace [K,3] f32 kept for the backward.
extern "C" int cs_cosine_loss_fwd(const float* student, const float* teacher, float* stats, float* loss, int K, int E, float weight,
                                  hipStream_t stream) {
    CS_CHECK_ARG(K > 0 && E % 4 == 0, "cs_cosine_loss_fwd: need K > 0 and E %% 4 == 0");
    hipLaunchKernelGGL(cosine_rows_kernel, dim3((K + 3) / 4), dim3(256), 0, stream, student, teacher, stats, K, E);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(cosine_reduce_kernel, dim3(1), dim3(256), 0, stream, stats, loss, K, weight);
    CS_LAUNCH_CHECK();
    return 0;
}
extern "C" int cs_cosine_loss_bwd(const float* student, const float* teacher, const float* stats, float* dstudent, int K, int E,
                                  float weight, float grad_scale, const float* upstream, hipStream_t stream) {
    CS_CHECK_ARG(K > 0, "cs_cosine_loss_bwd: K must be positive");
    const float coef = -weight * grad_scale / (float)K;
    hipLaunchKernelGGL(cosine_bwd_kernel, dim3((int)(((long)K * E + 255) / 256)), dim3(256), 0, stream, student, teacher, stats, dstudent, K, E, coef, upstream);
    CS_LAUNCH_CHECK();
    return 0;
}

// ---- RegionCLIP federated BCE (src/training/region_clip.py:47-56) --------------------------------------------
// z = logits * temp over the `ns` sampled noun columns; target = one-hot at tgt[k] (column index inside the sample,
// -1 = none); row loss = sum_c [max(z,0) - z*t + log(1 + exp(-|z|))]; loss = weight * mean_k row loss.
namespace {

__global__ __launch_bounds__(256) void fed_bce_rows_kernel(const float* __restrict__ logits, long ldz, const int* __restrict__ tgt,
                                                           float* __restrict__ rowloss, int K, int ns, float temp) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;
    const int t = tgt[k];
    float s = 0.f;
    for (int c = lane; c < ns; c += 64) {
        const float z = logits[(size_t)k * ldz + c] * temp;
        s += fmaxf(z, 0.f) - (c == t ? z : 0.f) + log1pf(__expf(-fabsf(z)));
    }
    s = wave_sum(s);
    if (lane == 0) rowloss[k] = s;
}

__global__ __launch_bounds__(256) void fed_bce_reduce_kernel(const float* __restrict__ rowloss, float* __restrict__ loss, int K, float weight) {
    __shared__ float part[256];
    float s = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) s += rowloss[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = weight * part[0] / (float)K;
}

// dz[k,c] = coef * (sigmoid(z) - t) * temp  for c < ns, 0 for the padding columns [ns, ldd)   (bf16: dgrad GEMM operand)
__global__ __launch_bounds__(256) void fed_bce_bwd_kernel(const float* __restrict__ logits, long ldz, const int* __restrict__ tgt,
                                                          __bf16* __restrict__ dz, long ldd, int K, int ns, float temp, float coef,
                                                          const float* __restrict__ upstream) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)K * ldd) return;
    const int k = (int)(i / ldd), c = (int)(i - (long)k * ldd);
    float v = 0.f;
    if (c < ns) {
        if (upstream) coef *= upstream[0];
        const float z = logits[(size_t)k * ldz + c] * temp;
        v = coef * temp * (1.f / (1.f + __expf(-z)) - (c == tgt[k] ? 1.f : 0.f));
    }
    dz[i] = f2bf(v);
}

}  // namespace

extern "C" int cs_fed_bce_fwd(const float* logits, long ldz, const int* tgt, float* rowloss, float* loss, int K, int ns, float temp,
                              float weight, hipStream_t stream) {
    CS_CHECK_ARG(K > 0 && ns > 0 && ldz >= ns, "cs_fed_bce_fwd: bad shape");
    hipLaunchKernelGGL(fed_bce_rows_kernel, dim3((K + 3) / 4), dim3(256), 0, stream, logits, ldz, tgt, rowloss, K, ns, temp);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(fed_bce_reduce_kernel, dim3(1), dim3(256), 0, stream, rowloss, loss, K, weight);
    CS_LAUNCH_CHECK();
    return 0;
}
extern "C" int cs_fed_bce_bwd(const float* logits, long ldz, const int* tgt, void* dz_bf16, long ldd, int K, int ns, float temp,
                              float weight, const float* upstream, hipStream_t stream) {
    CS_CHECK_ARG(K > 0 && ns > 0 && ldz >= ns && ldd >= ns, "cs_fed_bce_bwd: bad shape");
    hipLaunchKernelGGL(fed_bce_bwd_kernel, dim3((int)(((long)K * ldd + 255) / 256)), dim3(256), 0, stream, logits, ldz, tgt, (__bf16*)dz_bf16,
                       ldd, K, ns, temp, weight / (float)K, upstream);
    CS_LAUNCH_CHECK();
    return 0;
}
