// Detector RoI extractor (include/clipself_roi.h): mmdet's SingleRoIExtractor over mmcv's RoIAlign, all levels in one launch, forward
// and an atomic-free backward.  DESIGN.md §3.14.
//
//   roi_extract_fwd_kernel   one workgroup per box: level + geometry, the two axes' sample tables in LDS, then one thread per
//                            (bin, 4 channels): a tap is a float4 of a contiguous channel-last row
//   roi_geom_kernel          backward prepass, one thread per box: level, geometry and the rectangle of cells it can touch -> workspace
//   roi_bin_count_kernel,    backward prepass, one workgroup per (image, level): its boxes in ascending row -> workspace (a stable
//   roi_bin_fill_kernel      counting sort without atomics)
//   roi_extract_bwd_kernel   one wave per 4 x 4 tile of cells of one level and image (and 256 channels): scans the rectangles of its
//                            (image, level)'s boxes in ascending row, and gathers each hit's taps into LDS accumulators in the
//                            contract's order
//
// Every value that comes from device memory (image index, coordinates) is compared before it sizes a loop or forms an index.
#include "det_common.h"
#include "../../include/clipself_roi.h"

#define CSR_TAB 1040                 // samples of one axis of one box: P * grid <= |extent| + P <= 2 * 512 + 14 (sampling_ratio: <= 14 * 8)
#define CSR_FWD_THREADS 256
#define CSR_TILE 4                   // backward: cells per tile side
#define CSR_BWD_QUADS 64             // backward: float4 channel groups per workgroup (one wave)
#define CSR_LIST 128                 // backward: samples of one axis of one box that touch one tile (bound derived at build_list)
#define CSR_MAX_BINS 4096            // backward: (image % 1024, level) bins the boxes are sorted into

namespace {

struct Levels {
    float* map[CSR_MAX_LEVELS];
    long ld[CSR_MAX_LEVELS];
    int h[CSR_MAX_LEVELS], w[CSR_MAX_LEVELS];
    float scale[CSR_MAX_LEVELS];
    int tile_start[CSR_MAX_LEVELS + 1];          // backward: first tile of each level in blockIdx.x
    int L;
};

// What the pooling of one box needs, the same record in the forward and (through the workspace) the backward: 64 bytes.
struct BoxGeo {
    int b, lvl;                      // b = -1: the box pools to zeros (bounded-box rule, or no samples)
    int gh, gw;                      // samples per bin and axis
    int r_lo, r_hi, c_lo, c_hi;      // cells any of its samples can touch, inclusive (backward's reject test)
    float sy, sx, bh, bw;            // start and bin size on the level's map
    float count;                     // max(gh * gw, 1)
    int pad[3];
};
static_assert(sizeof(BoxGeo) == 64, "the workspace holds 64 bytes per box");

// mmdet 2.x SingleRoIExtractor.map_roi_levels for one box
__device__ __forceinline__ int roi_level(float x0, float y0, float x1, float y1, float finest_scale, int L) {
    const float area = f_mul(f_sub(x1, x0), f_sub(y1, y0));
    const float scale = __fsqrt_rn(area);
    const float t = floorf(log2f(f_add(f_div(scale, finest_scale), 1e-6f)));
    return t >= 1.f ? (int)fminf(t, (float)(L - 1)) : 0;          // NaN compares false: level 0
}

// sample i of bin p of one axis:  (start + p * bin) + ((i + 0.5) * bin) / grid
__device__ __forceinline__ float sample_coord(float start, float bin, int grid, int p, int i) {
    return f_add(f_add(start, f_mul((float)p, bin)), f_div(f_mul((float)i + 0.5f, bin), (float)grid));
}

// first and last cell an axis' samples can touch.  The coordinate is monotone in p and in i (every rounded operation is), so its
// extremes are at the two ends; one more cell on either side costs the reject test nothing.
__device__ __forceinline__ void axis_cells(float start, float bin, int grid, int P, int size, int& lo, int& hi) {
    const float a = sample_coord(start, bin, grid, 0, 0), z = sample_coord(start, bin, grid, P - 1, grid - 1);
    const float mn = fminf(fmaxf(fminf(a, z), 0.f), (float)(size - 1)), mx = fminf(fmaxf(fmaxf(a, z), 0.f), (float)(size - 1));
    lo = max((int)mn - 1, 0);
    hi = min((int)mx + 2, size - 1);
}

__device__ __forceinline__ BoxGeo box_geometry(const float* __restrict__ roi, const Levels& lv, int B, int P, int sampling_ratio,
                                               float finest_scale) {
    const float bf = roi[0], x0 = roi[1], y0 = roi[2], x1 = roi[3], y1 = roi[4];
    BoxGeo g;
    g.lvl = roi_level(x0, y0, x1, y1, finest_scale, lv.L);
    float s = lv.scale[0];
    int h = lv.h[0], w = lv.w[0];
#pragma unroll
    for (int l = 1; l < CSR_MAX_LEVELS; ++l)
        if (l == g.lvl) s = lv.scale[l], h = lv.h[l], w = lv.w[l];
    g.sx = f_sub(f_mul(x0, s), 0.5f);
    g.sy = f_sub(f_mul(y0, s), 0.5f);
    const float rw = f_sub(f_sub(f_mul(x1, s), 0.5f), g.sx), rh = f_sub(f_sub(f_mul(y1, s), 0.5f), g.sy);
    g.bw = f_div(rw, (float)P);
    g.bh = f_div(rh, (float)P);
    // NaN and Inf fail every comparison below that would let the box through
    const bool ok = bf >= 0.f && bf < (float)B && fabsf(rw) <= 2.f * (float)w && fabsf(rh) <= 2.f * (float)h;
    g.gw = g.gh = 0;
    if (ok) {
        g.gw = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(g.bw);       // |bin| <= 1024: the conversion is defined
        g.gh = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(g.bh);
    }
    const bool walk = g.gw > 0 && g.gh > 0 && P * g.gw <= CSR_TAB && P * g.gh <= CSR_TAB;      // the table bound holds by the limits above
    g.b = walk ? (int)bf : -1;
    if (!walk) g.gw = g.gh = 0;
    g.count = (float)max(g.gh * g.gw, 1);
    g.r_lo = g.c_lo = 0;
    g.r_hi = g.c_hi = -1;
    if (walk) {
        axis_cells(g.sy, g.bh, g.gh, P, h, g.r_lo, g.r_hi);
        axis_cells(g.sx, g.bw, g.gw, P, w, g.c_lo, g.c_hi);
    }
    g.pad[0] = g.pad[1] = g.pad[2] = 0;
    return g;
}

// mmcv's bilinear_interpolate along one axis.  -> false: the sample is outside [-1, size] and contributes nothing
__device__ __forceinline__ bool axis_sample(float c, int size, int& lo, int& hi, float& wl, float& wh) {
    if (!(c >= -1.f && c <= (float)size)) return false;
    if (c <= 0.f) c = 0.f;
    lo = (int)c;
    if (lo >= size - 1) {
        hi = lo = size - 1;
        c = (float)lo;
    } else {
        hi = lo + 1;
    }
    wh = f_sub(c, (float)lo);
    wl = f_sub(1.f, wh);
    return true;
}

__device__ __forceinline__ void fma4(float4& acc, float w, const float4 v) {
    acc.x = fmaf(w, v.x, acc.x);
    acc.y = fmaf(w, v.y, acc.y);
    acc.z = fmaf(w, v.z, acc.z);
    acc.w = fmaf(w, v.w, acc.w);
}

// ------------------------------------------------------------------------------------------------ forward
// grid (K), 256 threads.  The tables hold, per axis and sample e = p * grid + i, what depends on (box, bin, sample) only: the two cells
// and the two weights; a thread owns (bin, 4 channels) and forms the four tap weights of a sample from them -- four products against
// sixteen fmas and 64 bytes of loads.  With C >= 256 a wave reads one tap as 1 KiB of one cell's row.
__global__ __launch_bounds__(CSR_FWD_THREADS) void roi_extract_fwd_kernel(Levels lv, int B, int C, const float* __restrict__ rois, int P,
                                                                          int sampling_ratio, float finest_scale,
                                                                          float* __restrict__ out, long ldo) {
    __shared__ int ycell[CSR_TAB], xcell[CSR_TAB];       // lo | hi << 16, or -1: no contribution
    __shared__ float ywl[CSR_TAB], ywh[CSR_TAB], xwl[CSR_TAB], xwh[CSR_TAB];
    const int k = blockIdx.x, tid = threadIdx.x;
    const BoxGeo g = box_geometry(rois + (size_t)k * 5, lv, B, P, sampling_ratio, finest_scale);
    const float* map = lv.map[0];
    long ld = lv.ld[0];
    int h = lv.h[0], w = lv.w[0];
#pragma unroll
    for (int l = 1; l < CSR_MAX_LEVELS; ++l)
        if (l == g.lvl) map = lv.map[l], ld = lv.ld[l], h = lv.h[l], w = lv.w[l];
    const int ny = min(P * g.gh, CSR_TAB), nx = min(P * g.gw, CSR_TAB);
    for (int e = tid; e < ny; e += CSR_FWD_THREADS) {
        int lo = 0, hi = 0;
        float wl = 0.f, wh = 0.f;
        const bool in = axis_sample(sample_coord(g.sy, g.bh, g.gh, e / g.gh, e % g.gh), h, lo, hi, wl, wh);
        ycell[e] = in ? (lo | (hi << 16)) : -1;
        ywl[e] = wl, ywh[e] = wh;
    }
    for (int e = tid; e < nx; e += CSR_FWD_THREADS) {
        int lo = 0, hi = 0;
        float wl = 0.f, wh = 0.f;
        const bool in = axis_sample(sample_coord(g.sx, g.bw, g.gw, e / g.gw, e % g.gw), w, lo, hi, wl, wh);
        xcell[e] = in ? (lo | (hi << 16)) : -1;
        xwl[e] = wl, xwh[e] = wh;
    }
    __syncthreads();
    const int nq = C >> 2, items = P * P * nq;
    const float* img = map + (size_t)max(g.b, 0) * h * w * ld;        // g.b = -1: gh = gw = 0 and nothing below reads
    for (int it = tid; it < items; it += CSR_FWD_THREADS) {
        const int q = it % nq, bin = it / nq, ph = bin / P, pw = bin % P;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int iy = 0; iy < g.gh; ++iy) {
            const int ey = ph * g.gh + iy, yc = ycell[ey];
            if (yc < 0) continue;
            const float hy = ywl[ey], ly = ywh[ey];
            const float* row_lo = img + (size_t)(yc & 0xFFFF) * w * ld + q * 4;
            const float* row_hi = img + (size_t)(yc >> 16) * w * ld + q * 4;
            for (int ix = 0; ix < g.gw; ++ix) {
                const int ex = pw * g.gw + ix, xc = xcell[ex];
                if (xc < 0) continue;
                const float hx = xwl[ex], lx = xwh[ex];
                const size_t o_lo = (size_t)(xc & 0xFFFF) * ld, o_hi = (size_t)(xc >> 16) * ld;
                const float4 v1 = *(const float4*)(row_lo + o_lo), v2 = *(const float4*)(row_lo + o_hi);
                const float4 v3 = *(const float4*)(row_hi + o_lo), v4 = *(const float4*)(row_hi + o_hi);
                fma4(acc, f_mul(hy, hx), v1);
                fma4(acc, f_mul(hy, lx), v2);
                fma4(acc, f_mul(ly, hx), v3);
                fma4(acc, f_mul(ly, lx), v4);
            }
        }
        *(float4*)(out + ((size_t)k * P * P + bin) * ldo + q * 4) =
            make_float4(f_div(acc.x, g.count), f_div(acc.y, g.count), f_div(acc.z, g.count), f_div(acc.w, g.count));
    }
}

// ------------------------------------------------------------------------------------------------ backward
__global__ __launch_bounds__(256) void roi_geom_kernel(Levels lv, int B, const float* __restrict__ rois, int K, int P, int sampling_ratio,
                                                       float finest_scale, BoxGeo* __restrict__ geo) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < K) geo[k] = box_geometry(rois + (size_t)k * 5, lv, B, P, sampling_ratio, finest_scale);
}

// Boxes by bin = (image % NB) * L + level, each bin's rows ascending: a stable counting sort without atomics.  One workgroup per bin
// reads the K (image, level) pairs twice -- once to count, once to place by ordered ballot compaction -- and sums the counts of the
// bins in front of its own itself.  A tile then scans its bin's rows, K / (NB * L) on average, where a scan of all K cost 64
// dependent rounds of loads per tile at 4096 boxes (profiles/roi_extract_bench.md).  Integer sums only: any order gives the same list.
__device__ __forceinline__ bool in_bin(const BoxGeo* __restrict__ geo, int k, int NB, int b0, int l) {
    const int2 id = *(const int2*)&geo[k];
    return id.x >= 0 && id.x % NB == b0 && id.y == l;
}

__global__ __launch_bounds__(256) void roi_bin_count_kernel(const BoxGeo* __restrict__ geo, int K, int NB, int L, int* __restrict__ counts) {
    __shared__ int part[4];
    const int bin = blockIdx.x, b0 = bin / L, l = bin % L;
    int n = 0;
    for (int k = threadIdx.x; k < K; k += 256) n += in_bin(geo, k, NB, b0, l) ? 1 : 0;
    n = block_sum_256(n, part);
    if (threadIdx.x == 0) counts[bin] = n;
}

__global__ __launch_bounds__(256) void roi_bin_fill_kernel(const BoxGeo* __restrict__ geo, int K, int NB, int L, const int* __restrict__ counts,
                                                           int* __restrict__ starts, int* __restrict__ order) {
    __shared__ int part[4];
    __shared__ int wave_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int bin = blockIdx.x, b0 = bin / L, l = bin % L;
    int s = 0;
    for (int j = tid; j < bin; j += 256) s += counts[j];
    int pos = block_sum_256(s, part);                                    // the bins in front hold pos <= K rows together
    if (tid == 0) starts[bin] = pos;
    for (int k0 = 0; k0 < K; k0 += 256) {
        const int k = k0 + tid;
        const bool mine = k < K && in_bin(geo, k, NB, b0, l);
        const unsigned long long m = __ballot(mine);
        __syncthreads();                                                 // the previous round's wave_cnt has been read
        if (lane == 0) wave_cnt[wv] = __popcll(m);
        __syncthreads();
        int base = pos;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wv) base += wave_cnt[w];
            pos += wave_cnt[w];
        }
        const int at = base + __popcll(m & ((1ull << lane) - 1ull));
        if (mine && at < K) order[at] = k;                               // at < K: every row is in exactly one bin
    }
}

struct AxisList {
    int tag[CSR_LIST];               // p | lo_rel << 8 | hi_rel << 16, the cells relative to the tile; 0xFF: outside the tile
    float wl[CSR_LIST], wh[CSR_LIST];
};

// The samples of one axis that touch the tile's cells [t0, t0 + CSR_TILE), in ascending (p, i), built by one wave with ordered
// ballot compaction.  A touching sample has its coordinate in (t0 - 1, t0 + CSR_TILE).  With sampling_ratio == 0 and bin > 1 the
// samples are bin / ceil(bin) > 0.5 cells apart: at most 2 * (CSR_TILE + 1) + 1 = 11 of them; with bin <= 1 there are P <= 14 in all;
// with sampling_ratio > 0 at most 14 * 8 = 112.  So CSR_LIST = 128 entries hold every list; the count is clamped all the same.
__device__ __forceinline__ int build_list(AxisList& ls, float start, float bin, int grid, int P, int size, int t0, int lane) {
    const int n = min(P * grid, CSR_TAB);
    int cnt = 0;
    for (int e0 = 0; e0 < n; e0 += 64) {
        const int e = e0 + lane;
        int lo = 0, hi = 0;
        float wl = 0.f, wh = 0.f;
        bool hit = false;
        if (e < n) hit = axis_sample(sample_coord(start, bin, grid, e / grid, e % grid), size, lo, hi, wl, wh);
        const bool lo_in = lo >= t0 && lo < t0 + CSR_TILE, hi_in = hi >= t0 && hi < t0 + CSR_TILE;
        hit = hit && (lo_in || hi_in);
        const unsigned long long m = __ballot(hit);
        const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
        if (hit && pos < CSR_LIST) {
            ls.tag[pos] = (e / grid) | ((lo_in ? lo - t0 : 0xFF) << 8) | ((hi_in ? hi - t0 : 0xFF) << 16);
            ls.wl[pos] = wl, ls.wh[pos] = wh;
        }
        cnt += __popcll(m);
    }
    return min(cnt, CSR_LIST);
}

// grid (tiles of all levels, channel chunks of 256), 64 threads.  Thread = 4 channels; the tile's 16 accumulators of a thread sit in
// LDS (acc[cell][thread]: a wave's access is 1 KiB contiguous), because a tap's cell is a run-time index.  Control flow is wave-uniform:
// the hit mask, the lists and their counts are the same in every lane.
__global__ __launch_bounds__(64) void roi_extract_bwd_kernel(Levels lv, int C, const float* __restrict__ dout, long ldo, int K, int P,
                                                             const BoxGeo* __restrict__ geo, int NB, const int* __restrict__ counts,
                                                             const int* __restrict__ starts, const int* __restrict__ order) {
    __shared__ float4 acc[CSR_TILE * CSR_TILE][CSR_BWD_QUADS];
    __shared__ AxisList ylist, xlist;
    const int lane = threadIdx.x;
    int l = 0;
#pragma unroll
    for (int j = 1; j < CSR_MAX_LEVELS; ++j)
        if (j < lv.L && (int)blockIdx.x >= lv.tile_start[j]) l = j;
    float* map = lv.map[0];
    long ld = lv.ld[0];
    int h = lv.h[0], w = lv.w[0], t = blockIdx.x - lv.tile_start[0];
#pragma unroll
    for (int j = 1; j < CSR_MAX_LEVELS; ++j)
        if (j == l) map = lv.map[j], ld = lv.ld[j], h = lv.h[j], w = lv.w[j], t = blockIdx.x - lv.tile_start[j];
    const int tw = (w + CSR_TILE - 1) / CSR_TILE, th = (h + CSR_TILE - 1) / CSR_TILE;
    const int b = t / (th * tw), r0 = (t / tw % th) * CSR_TILE, c0 = (t % tw) * CSR_TILE;
    const int q = blockIdx.y * CSR_BWD_QUADS + lane;
    const bool live = q < (C >> 2);
#pragma unroll
    for (int c = 0; c < CSR_TILE * CSR_TILE; ++c) acc[c][lane] = make_float4(0.f, 0.f, 0.f, 0.f);
    bool any = false;
    // the rows of this tile's bin: both numbers come from the workspace, so they are clamped before they bound a loop or an index
    const int bin = (b % NB) * lv.L + l;
    const int s0 = min(max(starts[bin], 0), K), n = min(max(counts[bin], 0), K - s0);
    for (int i0 = 0; i0 < n; i0 += 64) {
        int k = -1;
        if (i0 + lane < n) k = order[s0 + i0 + lane];
        bool hit = false;
        if (k >= 0 && k < K) {
            const int4 id = *(const int4*)&geo[k];                         // b, lvl, gh, gw
            const int4 rc = *(const int4*)&geo[k].r_lo;
            hit = id.x == b && id.y == l && rc.x < r0 + CSR_TILE && rc.y >= r0 && rc.z < c0 + CSR_TILE && rc.w >= c0;
        }
        unsigned long long m = __ballot(hit);
        while (m) {                                                        // ascending box row: the bin's rows are ascending
            const int kk = __builtin_amdgcn_readfirstlane(__shfl(k, __ffsll((long long)m) - 1, 64));
            m &= m - 1;
            const BoxGeo g = geo[kk];
            __syncthreads();                                               // the previous box's lists have been consumed
            const int ny = build_list(ylist, g.sy, g.bh, g.gh, P, h, r0, lane);
            const int nx = build_list(xlist, g.sx, g.bw, g.gw, P, w, c0, lane);
            __syncthreads();
            if (ny == 0 || nx == 0) continue;
            any = true;
            const float* dk = dout + (size_t)kk * P * P * ldo + (live ? q * 4 : 0);
            for (int y0 = 0; y0 < ny;) {                                   // runs of one ph, then runs of one pw: bins in ascending (ph, pw)
                const int ph = ylist.tag[y0] & 0xFF;
                int y1 = y0 + 1;
                while (y1 < ny && (ylist.tag[y1] & 0xFF) == ph) ++y1;
                for (int x0 = 0; x0 < nx;) {
                    const int pw = xlist.tag[x0] & 0xFF;
                    int x1 = x0 + 1;
                    while (x1 < nx && (xlist.tag[x1] & 0xFF) == pw) ++x1;
                    float4 gv = *(const float4*)(dk + (size_t)(ph * P + pw) * ldo);
                    gv = make_float4(f_div(gv.x, g.count), f_div(gv.y, g.count), f_div(gv.z, g.count), f_div(gv.w, g.count));
                    for (int a = y0; a < y1; ++a) {
                        const int ty = ylist.tag[a], rl = (ty >> 8) & 0xFF, rh = (ty >> 16) & 0xFF;
                        const float hy = ylist.wl[a], ly = ylist.wh[a];
                        for (int e = x0; e < x1; ++e) {
                            const int tx = xlist.tag[e], cl = (tx >> 8) & 0xFF, ch = (tx >> 16) & 0xFF;
                            const float hx = xlist.wl[e], lx = xlist.wh[e];
                            if (rl != 0xFF && cl != 0xFF) { float4 v = acc[rl * CSR_TILE + cl][lane]; fma4(v, f_mul(hy, hx), gv); acc[rl * CSR_TILE + cl][lane] = v; }
                            if (rl != 0xFF && ch != 0xFF) { float4 v = acc[rl * CSR_TILE + ch][lane]; fma4(v, f_mul(hy, lx), gv); acc[rl * CSR_TILE + ch][lane] = v; }
                            if (rh != 0xFF && cl != 0xFF) { float4 v = acc[rh * CSR_TILE + cl][lane]; fma4(v, f_mul(ly, hx), gv); acc[rh * CSR_TILE + cl][lane] = v; }
                            if (rh != 0xFF && ch != 0xFF) { float4 v = acc[rh * CSR_TILE + ch][lane]; fma4(v, f_mul(ly, lx), gv); acc[rh * CSR_TILE + ch][lane] = v; }
                        }
                    }
                    x0 = x1;
                }
                y0 = y1;
            }
        }
    }
    if (!any || !live) return;
#pragma unroll
    for (int c = 0; c < CSR_TILE * CSR_TILE; ++c) {
        const int r = r0 + c / CSR_TILE, x = c0 + c % CSR_TILE;
        if (r < h && x < w) {
            float4* cell = (float4*)(map + (((size_t)b * h + r) * w + x) * ld + q * 4);
            float4 v = *cell;
            const float4 a = acc[c][lane];
            v.x += a.x, v.y += a.y, v.z += a.z, v.w += a.w;
            *cell = v;
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// ------------------------------------------------------------------------------------------------ host side
static int csr_check(const char* who, const csr_level* levels, int L, int B, int C, const float* rois, int K, int P, int sampling_ratio,
                     float finest_scale, const float* io, long ldo, Levels& lv) {
    CS_CHECK_ARG(L >= 1 && L <= CSR_MAX_LEVELS, "%s: L = %d levels must be in [1, %d]", who, L, CSR_MAX_LEVELS);
    CS_CHECK_ARG(B >= 1 && B <= 65535, "%s: B = %d must be in [1, 65535]", who, B);
    CS_CHECK_ARG(C >= 4 && C % 4 == 0, "%s: C = %d must be a positive multiple of 4", who, C);
    CS_CHECK_ARG(K >= 0 && K <= (1 << 24), "%s: K = %d must be in [0, 2^24]", who, K);
    CS_CHECK_ARG(P >= 1 && P <= CSR_MAX_P, "%s: P = %d (output_size) must be in [1, %d]", who, P, CSR_MAX_P);
    CS_CHECK_ARG(sampling_ratio >= 0 && sampling_ratio <= CSR_MAX_SR, "%s: sampling_ratio = %d must be in [0, %d]", who, sampling_ratio, CSR_MAX_SR);
    CS_CHECK_ARG(finest_scale > 0.f && finest_scale <= 3.0e38f, "%s: finest_scale = %g must be positive and finite", who, (double)finest_scale);
    CS_CHECK_ARG(ldo >= C && ldo % 4 == 0, "%s: ldo = %ld must be a multiple of 4 and >= C = %d", who, ldo, C);
    CS_CHECK_ARG(levels != nullptr, "%s: levels is NULL", who);
    CS_CHECK_ARG(K == 0 || (rois != nullptr && io != nullptr), "%s: rois and out / dout must not be NULL when K > 0", who);
    CS_CHECK_ARG(aligned16(io), "%s: out / dout must be 16-byte aligned", who);
    long long tiles = 0;
    for (int l = 0; l < CSR_MAX_LEVELS; ++l) {
        const csr_level& s = levels[l < L ? l : 0];
        if (l < L) {
            CS_CHECK_ARG(s.h >= 1 && s.h <= CSR_MAX_SIDE && s.w >= 1 && s.w <= CSR_MAX_SIDE, "%s: level %d grid %d x %d: sides must be in [1, %d]",
                         who, l, s.h, s.w, CSR_MAX_SIDE);
            CS_CHECK_ARG(s.ld >= C && s.ld % 4 == 0, "%s: level %d row stride ld = %ld must be a multiple of 4 and >= C = %d", who, l, s.ld, C);
            CS_CHECK_ARG(s.spatial_scale > 0.f && s.spatial_scale <= 3.0e38f, "%s: level %d spatial_scale = %g must be positive and finite", who,
                         l, (double)s.spatial_scale);
            CS_CHECK_ARG(K == 0 || s.map != nullptr, "%s: level %d map is NULL", who, l);
            CS_CHECK_ARG(aligned16(s.map), "%s: level %d map must be 16-byte aligned", who, l);
        }
        lv.map[l] = s.map, lv.ld[l] = s.ld, lv.h[l] = s.h, lv.w[l] = s.w, lv.scale[l] = s.spatial_scale;
        lv.tile_start[l] = (int)tiles;
        if (l < L) tiles += (long long)B * ((s.h + CSR_TILE - 1) / CSR_TILE) * ((s.w + CSR_TILE - 1) / CSR_TILE);
        CS_CHECK_ARG(tiles < (1ll << 31), "%s: B = %d images of these grids have more than 2^31 - 1 tiles of cells", who, B);
    }
    lv.tile_start[CSR_MAX_LEVELS] = (int)tiles;
    lv.L = L;
    return 0;
}

// workspace: geo [K] | order [K rounded up to 4] | counts [CSR_MAX_BINS] | starts [CSR_MAX_BINS]
static size_t csr_order_offset(int K) { return (size_t)(K > 0 ? K : 1) * sizeof(BoxGeo); }
static size_t csr_counts_offset(int K) { return csr_order_offset(K) + (size_t)((K > 0 ? K : 1) + 3) / 4 * 16; }

extern "C" size_t csr_roi_extract_workspace(int K) {
    if (K < 0 || K > (1 << 24)) return 0;
    return csr_counts_offset(K) + 2 * CSR_MAX_BINS * sizeof(int);
}

extern "C" int csr_roi_extract_fwd(const csr_level* levels, int L, int B, int C, const float* rois, int K, int P, int sampling_ratio,
                                   float finest_scale, float* out, long ldo, hipStream_t stream) {
    Levels lv;
    if (int rc = csr_check("csr_roi_extract_fwd", levels, L, B, C, rois, K, P, sampling_ratio, finest_scale, out, ldo, lv)) return rc;
    if (K == 0) return 0;
    hipLaunchKernelGGL(roi_extract_fwd_kernel, dim3(K), dim3(CSR_FWD_THREADS), 0, stream, lv, B, C, rois, P, sampling_ratio, finest_scale, out,
                       ldo);
    CS_LAUNCH_CHECK();
    return 0;
}

extern "C" int csr_roi_extract_bwd(const float* dout, long ldo, const float* rois, int K, int P, int sampling_ratio, float finest_scale,
                                   const csr_level* dlevels, int L, int B, int C, void* workspace, hipStream_t stream) {
    Levels lv;
    if (int rc = csr_check("csr_roi_extract_bwd", dlevels, L, B, C, rois, K, P, sampling_ratio, finest_scale, dout, ldo, lv)) return rc;
    CS_CHECK_ARG(workspace != nullptr && aligned16(workspace), "csr_roi_extract_bwd: workspace is NULL or not 16-byte aligned (csr_roi_extract_workspace() bytes are needed)");
    const int chunks = ((C >> 2) + CSR_BWD_QUADS - 1) / CSR_BWD_QUADS;
    CS_CHECK_ARG(chunks <= 65535, "csr_roi_extract_bwd: C = %d is more than 65535 chunks of 256 channels", C);
    if (K == 0) return 0;
    BoxGeo* geo = (BoxGeo*)workspace;
    hipLaunchKernelGGL(roi_geom_kernel, dim3((K + 255) / 256), dim3(256), 0, stream, lv, B, rois, K, P, sampling_ratio, finest_scale, geo);
    CS_LAUNCH_CHECK();
    int* order = (int*)((char*)workspace + csr_order_offset(K));
    int* counts = (int*)((char*)workspace + csr_counts_offset(K));
    int* starts = counts + CSR_MAX_BINS;
    const int NB = B < CSR_MAX_BINS / CSR_MAX_LEVELS ? B : CSR_MAX_BINS / CSR_MAX_LEVELS;      // more images than that share bins, image % NB
    hipLaunchKernelGGL(roi_bin_count_kernel, dim3(NB * L), dim3(256), 0, stream, geo, K, NB, L, counts);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(roi_bin_fill_kernel, dim3(NB * L), dim3(256), 0, stream, geo, K, NB, L, counts, starts, order);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(roi_extract_bwd_kernel, dim3(lv.tile_start[CSR_MAX_LEVELS], chunks), dim3(64), 0, stream, lv, C, dout, ldo, K, P, geo, NB,
                       counts, starts, order);
    CS_LAUNCH_CHECK();
    return 0;
}
