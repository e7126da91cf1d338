// RPN proposals (include/clipself_rpn.h): per-level top-k of the RPN head's maps, box decoding and the min-size filter.  All on the
// stream, nothing read back.  DESIGN.md §3.18.
//
//   prop_init_kernel     zeroes the per-list histograms of the workspace and writes starts[b] = b * Ktot
//   prop_hist_kernel<P>  radix pass P (digits of 11, 11 and 10 bits of the 32-bit key) over the lists longer than nms_pre: workgroup = 2048
//                        anchors of one list, LDS histogram of the keys that carry the prefix found so far, added to the list's
//                        histogram with integer atomics.  The prefix is not stored: every workgroup re-derives it from the finished
//                        histograms of the earlier passes
//   prop_count_kernel    the same workgroups: how many keys of the chunk are better than the threshold key and how many equal it
//   prop_take_kernel     the same workgroups: ordered compaction.  Better keys go to the slot (better keys of the earlier chunks + rank in
//                        the chunk), threshold ties behind all better keys in ascending anchor index, the first k - better of them
//   prop_rows_kernel     workgroup = one list: bitonic sort of its (key << 32 | i) pairs in LDS (a list no longer than nms_pre skips the
//                        select and comes straight from the map), then one thread per row: sigmoid, decode, filter, stores
//
// Every grid and trip count is a function of the host arguments alone.  An anchor index that passed through the workspace is compared with
// the list's length before it indexes anything, and every slot with the list's k before it is written.
#include "det_common.h"
#include "../../include/clipself_rpn.h"

#pragma clang fp contract(off)

#define CSP_THREADS 256
#define CSP_CHUNK 2048                // anchors per workgroup of the select passes: 8 rounds of 256
#define CSP_BINS 2048                 // bins of one histogram (the third pass uses 1024 of them)
#define CSP_ROWS_THREADS 1024

namespace {

struct LevelP {
    const float* cls;
    const float* reg;
    int hw, n, k;                     // h * w, anchors of a list, rows kept
    int row0, anc0;                   // first output row of the level inside an image, first row of the level in `anchors`
    int lng;                          // ordinal among the levels whose lists are longer than nms_pre, -1 for a short level
    int chunk0, nchunks;              // the level's workgroups in the select grids
};
struct Params {
    LevelP lv[CSP_MAX_LEVELS];
    int L, B, A, Ktot, nms_pre, nlong, chunks;
};

// the sort key of a logit: ~ord_bits(x), smallest = best; NaN = 0xFFFFFFFF, which no number maps to
__device__ __forceinline__ uint32_t key_of(float x) {
    return (__float_as_uint(x) & 0x7FFFFFFFu) > 0x7F800000u ? 0xFFFFFFFFu : ~ord_bits(x);
}
// logit of anchor i = (y * w + x) * A + a of image b
__device__ __forceinline__ float logit_at(const LevelP& lv, int A, int b, int i) {
    const int p = i / A, a = i - p * A;
    return lv.cls[((size_t)b * A + a) * lv.hw + p];
}

template <int P> __device__ __forceinline__ int digit_of(uint32_t key) {
    return P == 0 ? (int)(key >> 21) : P == 1 ? (int)((key >> 10) & 2047u) : (int)(key & 1023u);
}
// the key carries the digits found in the passes before P
template <int P> __device__ __forceinline__ bool carries(uint32_t key, uint32_t prefix) {
    return P == 0 ? true : P == 1 ? (key >> 21) == (prefix >> 21) : (key >> 10) == (prefix >> 10);
}

// The level of select workgroup `chunk`; -1 cannot happen (the grid is the sum of the levels' chunks).
__device__ __forceinline__ int level_of_chunk(const Params& p, int chunk) {
    int l = -1;
    for (int q = 0; q < p.L; ++q)
        if (p.lv[q].lng >= 0 && chunk >= p.lv[q].chunk0 && chunk < p.lv[q].chunk0 + p.lv[q].nchunks) l = q;
    return l;
}

struct Scratch {
    int wave[8];
    int digit, need;
};

// exclusive prefix sum of one int per thread over the 256 threads of the workgroup; *total = the sum.  Two barriers.
__device__ __forceinline__ int block_excl_scan(int v, Scratch& s, int* total) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                       // the scratch may still be read from an earlier call
    if (lane == 63) s.wave[w] = inc;
    __syncthreads();
    int base = 0;
    for (int q = 0; q < w; ++q) base += s.wave[q];
    *total = s.wave[0] + s.wave[1] + s.wave[2] + s.wave[3];
    return base + inc - v;
}

// One radix step on a finished histogram: the bin that holds the need-th smallest key, and how many are still needed inside it.  Thread t
// owns bins 8t .. 8t + 7.  Exactly one thread finds it when 1 <= need <= the histogram's sum; otherwise the digit stays 0 and need as it
// was, which later code survives because every slot is compared with k before it is written.
__device__ __forceinline__ void radix_step(const int* __restrict__ hist, int shift, uint32_t& prefix, int& need, Scratch& s) {
    const int tid = threadIdx.x;
    int h[8], sum = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        h[q] = hist[tid * 8 + q];
        sum += h[q];
    }
    int total;
    const int excl = block_excl_scan(sum, s, &total);
    if (tid == 0) {
        s.digit = 0;
        s.need = need;
    }
    __syncthreads();
    if (excl < need && need <= excl + sum) {
        int cum = excl, q = 0;
        for (; q < 7; ++q) {
            if (cum + h[q] >= need) break;
            cum += h[q];
        }
        s.digit = tid * 8 + q;
        s.need = need - cum;
    }
    __syncthreads();
    prefix |= (uint32_t)s.digit << shift;
    need = s.need;
    __syncthreads();
}

// the state after `passes` finished passes of a list: prefix = the digits found, need = keys still to take among those that carry them
__device__ __forceinline__ void resolve(const int* __restrict__ hist3, int passes, int k, uint32_t& prefix, int& need, Scratch& s) {
    prefix = 0;
    need = k;
    if (passes >= 1) radix_step(hist3, 21, prefix, need, s);
    if (passes >= 2) radix_step(hist3 + CSP_BINS, 10, prefix, need, s);
    if (passes >= 3) radix_step(hist3 + 2 * CSP_BINS, 0, prefix, need, s);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ init
// grid `blocks` (host), 256 threads: grid-stride over the histograms and over starts
__global__ __launch_bounds__(CSP_THREADS) void prop_init_kernel(int* __restrict__ hist, size_t nhist, int* __restrict__ starts, int B, int Ktot) {
    const size_t stride = (size_t)gridDim.x * CSP_THREADS;
    for (size_t i = (size_t)blockIdx.x * CSP_THREADS + threadIdx.x; i < nhist; i += stride) hist[i] = 0;
    for (size_t i = (size_t)blockIdx.x * CSP_THREADS + threadIdx.x; i <= (size_t)B; i += stride) starts[i] = (int)i * Ktot;
}

// ------------------------------------------------------------------------------------------------ histogram passes
// grid (chunks, B), 256 threads
template <int P>
__global__ __launch_bounds__(CSP_THREADS) void prop_hist_kernel(Params p, int* __restrict__ hist) {
    __shared__ int bins[CSP_BINS];
    __shared__ Scratch s;
    const int tid = threadIdx.x, b = blockIdx.y;
    const int l = level_of_chunk(p, blockIdx.x);
    if (l < 0) return;
    const LevelP& lv = p.lv[l];
    int* hist3 = hist + ((size_t)b * p.nlong + lv.lng) * 3 * CSP_BINS;
    uint32_t prefix;
    int need;
    resolve(hist3, P, lv.k, prefix, need, s);
    for (int q = tid; q < CSP_BINS; q += CSP_THREADS) bins[q] = 0;
    __syncthreads();
    const int i0 = (blockIdx.x - lv.chunk0) * CSP_CHUNK;
#pragma unroll 1
    for (int r = 0; r < CSP_CHUNK / CSP_THREADS; ++r) {
        const int i = i0 + r * CSP_THREADS + tid;
        if (i < lv.n) {
            const uint32_t key = key_of(logit_at(lv, p.A, b, i));
            if (carries<P>(key, prefix)) atomicAdd(&bins[digit_of<P>(key)], 1);
        }
    }
    __syncthreads();
    int* dst = hist3 + P * CSP_BINS;
    for (int q = tid; q < CSP_BINS; q += CSP_THREADS) {
        const int c = bins[q];
        if (c) atomicAdd(&dst[q], c);
    }
}

// ------------------------------------------------------------------------------------------------ count
// grid (chunks, B), 256 threads: counts[b][chunk] = (keys below the threshold key, keys equal to it) of the chunk
__global__ __launch_bounds__(CSP_THREADS) void prop_count_kernel(Params p, const int* __restrict__ hist, int* __restrict__ counts) {
    __shared__ Scratch s;
    __shared__ int red[2][4];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int l = level_of_chunk(p, blockIdx.x);
    if (l < 0) return;
    const LevelP& lv = p.lv[l];
    uint32_t thr;
    int need;
    resolve(hist + ((size_t)b * p.nlong + lv.lng) * 3 * CSP_BINS, 3, lv.k, thr, need, s);
    const int i0 = (blockIdx.x - lv.chunk0) * CSP_CHUNK;
    int nb = 0, nt = 0;
#pragma unroll 1
    for (int r = 0; r < CSP_CHUNK / CSP_THREADS; ++r) {
        const int i = i0 + r * CSP_THREADS + tid;
        if (i < lv.n) {
            const uint32_t key = key_of(logit_at(lv, p.A, b, i));
            nb += key < thr;
            nt += key == thr;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nb += __shfl_xor(nb, o, 64);
        nt += __shfl_xor(nt, o, 64);
    }
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = nb;
        red[1][tid >> 6] = nt;
    }
    __syncthreads();
    if (tid < 2) counts[((size_t)b * p.chunks + blockIdx.x) * 2 + tid] = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
}

// ------------------------------------------------------------------------------------------------ take
// grid (chunks, B), 256 threads: sel[b][lng * nms_pre + slot] = key << 32 | i
__global__ __launch_bounds__(CSP_THREADS) void prop_take_kernel(Params p, const int* __restrict__ hist, const int* __restrict__ counts,
                                                                u64* __restrict__ sel) {
    __shared__ Scratch s;
    __shared__ int wsum[2][4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, b = blockIdx.y;
    const int l = level_of_chunk(p, blockIdx.x);
    if (l < 0) return;
    const LevelP& lv = p.lv[l];
    uint32_t thr;
    int need;
    resolve(hist + ((size_t)b * p.nlong + lv.lng) * 3 * CSP_BINS, 3, lv.k, thr, need, s);
    const int better = lv.k - need;                        // keys below the threshold key in the whole list; `need` ties follow them
    // better keys and ties in the chunks before this one
    const int c = blockIdx.x - lv.chunk0;
    const int* cl = counts + ((size_t)b * p.chunks + lv.chunk0) * 2;
    int pb = 0, pt = 0;
    for (int q = tid; q < c; q += CSP_THREADS) {
        pb += cl[q * 2];
        pt += cl[q * 2 + 1];
    }
    int tot;
    block_excl_scan(pb, s, &tot);
    pb = tot;
    block_excl_scan(pt, s, &tot);
    pt = tot;
    u64* out = sel + (size_t)b * ((size_t)p.nlong * p.nms_pre) + (size_t)lv.lng * p.nms_pre;
    const int i0 = c * CSP_CHUNK;
#pragma unroll 1
    for (int r = 0; r < CSP_CHUNK / CSP_THREADS; ++r) {
        const int i = i0 + r * CSP_THREADS + tid;
        uint32_t key = 0;
        bool isb = false, ist = false;
        if (i < lv.n) {
            key = key_of(logit_at(lv, p.A, b, i));
            isb = key < thr;
            ist = key == thr;
        }
        const u64 mb = __ballot(isb), mt = __ballot(ist);
        const u64 below = (1ull << lane) - 1ull;
        __syncthreads();                                   // wsum of the round before has been read
        if (lane == 0) {
            wsum[0][w] = __popcll(mb);
            wsum[1][w] = __popcll(mt);
        }
        __syncthreads();
        int ob = pb, ot = pt;
        for (int q = 0; q < w; ++q) {
            ob += wsum[0][q];
            ot += wsum[1][q];
        }
        int slot = -1;
        if (isb) slot = ob + __popcll(mb & below);
        else if (ist) {
            const int rank = ot + __popcll(mt & below);    // the tie's place among all ties of the list, in ascending anchor index
            if (rank < need) slot = better + rank;
        }
        if (slot >= 0 && slot < lv.k) out[slot] = ((u64)key << 32) | (uint32_t)i;
        pb += wsum[0][0] + wsum[0][1] + wsum[0][2] + wsum[0][3];
        pt += wsum[1][0] + wsum[1][1] + wsum[1][2] + wsum[1][3];
    }
}

// ------------------------------------------------------------------------------------------------ sort, decode, store
// grid (L, B), 1024 threads
__global__ __launch_bounds__(CSP_ROWS_THREADS) void prop_rows_kernel(Params p, BoxCoder dc, float min_size, const u64* __restrict__ sel,
                                                                     const float* __restrict__ anchors, long lda,
                                                                     const float* __restrict__ max_shape, float* __restrict__ boxes,
                                                                     float* __restrict__ scores, int* __restrict__ group,
                                                                     int* __restrict__ anchor_inds) {
    __shared__ u64 keys[CSP_MAX_PRE];
    const int tid = threadIdx.x, l = blockIdx.x, b = blockIdx.y;
    const LevelP& lv = p.lv[l];
    const int k = lv.k;                                    // 1 <= k <= nms_pre <= 4096
    const int P2 = next_pow2(k);
    if (lv.lng >= 0) {
        const u64* src = sel + (size_t)b * ((size_t)p.nlong * p.nms_pre) + (size_t)lv.lng * p.nms_pre;
        for (int t = tid; t < k; t += CSP_ROWS_THREADS) keys[t] = src[t];
    } else {                                               // n <= nms_pre: the whole list, no select
        for (int t = tid; t < k; t += CSP_ROWS_THREADS) keys[t] = ((u64)key_of(logit_at(lv, p.A, b, t)) << 32) | (uint32_t)t;
    }
    for (int t = k + tid; t < P2; t += CSP_ROWS_THREADS) keys[t] = ~0ull;
    __syncthreads();
    bitonic_sort(keys, P2, tid, CSP_ROWS_THREADS);
    for (int t = tid; t < k; t += CSP_ROWS_THREADS) {
        const size_t row = (size_t)b * p.Ktot + lv.row0 + t;
        const uint32_t i = (uint32_t)keys[t];
        float o[4] = {0.f, 0.f, 0.f, 0.f}, sc = 0.f;
        int g = -1, ai = -1;
        if (i < (uint32_t)lv.n) {                          // always: the index was built from i < n
            const int pos = (int)i / p.A, a = (int)i - pos * p.A;
            const float x = lv.cls[((size_t)b * p.A + a) * lv.hw + pos];
            const float e = expf(-fabsf(x));
            sc = x >= 0.f ? f_div(1.f, f_add(1.f, e)) : (x < 0.f ? f_div(e, f_add(1.f, e)) : x);      // NaN stays NaN
            const float* rp = lv.reg + ((size_t)b * 4 * p.A + 4 * a) * lv.hw + pos;
            float d[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) d[q] = rp[(size_t)q * lv.hw];
            ai = lv.anc0 + (int)i;
            decode_box(dc, anchors + (size_t)ai * lda, d, max_shape ? max_shape + b * 2 : nullptr, o);
            const bool keep = min_size < 0.f || (f_sub(o[2], o[0]) > min_size && f_sub(o[3], o[1]) > min_size);
            g = keep ? l : -1;
        }
        float* bp = boxes + row * 4;
        bp[0] = o[0], bp[1] = o[1], bp[2] = o[2], bp[3] = o[3];
        scores[row] = sc;
        group[row] = g;
        if (anchor_inds) anchor_inds[row] = ai;
    }
}

// ------------------------------------------------------------------------------------------------ host side
namespace {
struct Plan {
    Params p;
    size_t off_counts, off_sel, nhist, total;
    bool ok;
};
size_t up256(size_t n) { return (n + 255) / 256 * 256; }

// Fills everything of Params but the pointers; ok = inside the limits of the header.
Plan make_plan(const csp_level* levels, int L, int B, int A, int nms_pre) {
    Plan pl;
    pl.ok = false;
    pl.total = 0;
    if (!levels || L < 1 || L > CSP_MAX_LEVELS || B < 1 || B > 65535 || A < 1 || A > CSP_MAX_ANCHORS || nms_pre < 1 || nms_pre > CSP_MAX_PRE)
        return pl;
    Params& p = pl.p;
    p.L = L, p.B = B, p.A = A, p.nms_pre = nms_pre;
    long long ktot = 0, anc = 0;
    int nlong = 0, chunks = 0;
    for (int l = 0; l < L; ++l) {
        const int h = levels[l].h, w = levels[l].w;
        if (h < 1 || h > CSP_MAX_SIDE || w < 1 || w > CSP_MAX_SIDE) return pl;
        LevelP& lv = p.lv[l];
        lv.cls = nullptr, lv.reg = nullptr;
        lv.hw = h * w;
        lv.n = lv.hw * A;                                  // at most 512 * 512 * 16 = 2^22
        lv.k = lv.n < nms_pre ? lv.n : nms_pre;
        lv.row0 = (int)ktot;
        lv.anc0 = (int)anc;
        lv.lng = -1, lv.chunk0 = 0, lv.nchunks = 0;
        if (lv.n > nms_pre) {
            lv.lng = nlong++;
            lv.chunk0 = chunks;
            lv.nchunks = (lv.n + CSP_CHUNK - 1) / CSP_CHUNK;
            chunks += lv.nchunks;
        }
        ktot += lv.k;
        anc += lv.n;
    }
    for (int l = L; l < CSP_MAX_LEVELS; ++l) p.lv[l] = p.lv[0];
    if (ktot > CSP_MAX_ROWS) return pl;
    p.Ktot = (int)ktot, p.nlong = nlong, p.chunks = chunks;
    pl.nhist = (size_t)B * nlong * 3 * CSP_BINS;
    pl.off_counts = up256(pl.nhist * sizeof(int));
    pl.off_sel = pl.off_counts + up256((size_t)B * chunks * 2 * sizeof(int));
    pl.total = pl.off_sel + up256((size_t)B * nlong * nms_pre * sizeof(u64));
    if (pl.total < 256) pl.total = 256;
    pl.ok = true;
    return pl;
}
}  // namespace

extern "C" size_t csp_workspace(const csp_level* levels, int L, int B, int A, int nms_pre) {
    const Plan pl = make_plan(levels, L, B, A, nms_pre);
    return pl.ok ? pl.total : 0;
}

extern "C" int csp_select(const csp_level* levels, int L, int B, int A, const float* anchors, long lda, int nms_pre, const float* means,
                          const float* stds, float wh_ratio_clip, const float* max_shape, float min_bbox_size, float* boxes, float* scores,
                          int* group, int* anchor_inds, int* starts, void* workspace, hipStream_t stream) {
    CS_CHECK_ARG(L >= 1 && L <= CSP_MAX_LEVELS, "csp_select: L = %d must be in [1, %d]", L, CSP_MAX_LEVELS);
    CS_CHECK_ARG(levels != nullptr, "csp_select: levels is NULL");
    CS_CHECK_ARG(B >= 1 && B <= 65535, "csp_select: B = %d must be in [1, 65535]", B);
    CS_CHECK_ARG(A >= 1 && A <= CSP_MAX_ANCHORS, "csp_select: A = %d must be in [1, %d]", A, CSP_MAX_ANCHORS);
    CS_CHECK_ARG(nms_pre >= 1 && nms_pre <= CSP_MAX_PRE, "csp_select: nms_pre = %d must be in [1, %d]", nms_pre, CSP_MAX_PRE);
    CS_CHECK_ARG(lda >= 4, "csp_select: lda = %ld must be >= 4", lda);
    CS_CHECK_ARG(wh_ratio_clip > 0.f, "csp_select: wh_ratio_clip = %g must be positive", (double)wh_ratio_clip);
    for (int l = 0; l < L; ++l) {
        CS_CHECK_ARG(levels[l].h >= 1 && levels[l].h <= CSP_MAX_SIDE && levels[l].w >= 1 && levels[l].w <= CSP_MAX_SIDE,
                     "csp_select: level %d: h = %d, w = %d must be in [1, %d]", l, levels[l].h, levels[l].w, CSP_MAX_SIDE);
        CS_CHECK_ARG(levels[l].cls && levels[l].reg, "csp_select: level %d: cls and reg must not be NULL", l);
    }
    Plan pl = make_plan(levels, L, B, A, nms_pre);
    CS_CHECK_ARG(pl.ok, "csp_select: Ktot = sum of min(nms_pre, h * w * A) must be at most %d", CSP_MAX_ROWS);
    CS_CHECK_ARG(anchors && means && stds, "csp_select: anchors, means and stds (host float[4]) must not be NULL");
    CS_CHECK_ARG(boxes && scores && group && starts, "csp_select: boxes, scores, group and starts must not be NULL");
    CS_CHECK_ARG(workspace != nullptr, "csp_select: workspace is NULL (csp_workspace() bytes are needed)");
    Params& p = pl.p;
    for (int l = 0; l < L; ++l) p.lv[l].cls = levels[l].cls, p.lv[l].reg = levels[l].reg;
    for (int l = L; l < CSP_MAX_LEVELS; ++l) p.lv[l] = p.lv[0];
    BoxCoder dc;
    for (int q = 0; q < 4; ++q) dc.mean[q] = means[q], dc.std[q] = stds[q];
    dc.max_ratio = coder_max_ratio(wh_ratio_clip);
    char* ws = (char*)workspace;
    int* hist = (int*)ws;
    int* counts = (int*)(ws + pl.off_counts);
    u64* sel = (u64*)(ws + pl.off_sel);

    size_t work = pl.nhist > (size_t)B + 1 ? pl.nhist : (size_t)B + 1;
    size_t blocks = (work + CSP_THREADS * 8 - 1) / (CSP_THREADS * 8);
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(prop_init_kernel, dim3((unsigned)blocks), dim3(CSP_THREADS), 0, stream, hist, pl.nhist, starts, B, p.Ktot);
    CS_LAUNCH_CHECK();
    if (p.chunks > 0) {
        const dim3 grid(p.chunks, B), block(CSP_THREADS);
        hipLaunchKernelGGL(prop_hist_kernel<0>, grid, block, 0, stream, p, hist);
        CS_LAUNCH_CHECK();
        hipLaunchKernelGGL(prop_hist_kernel<1>, grid, block, 0, stream, p, hist);
        CS_LAUNCH_CHECK();
        hipLaunchKernelGGL(prop_hist_kernel<2>, grid, block, 0, stream, p, hist);
        CS_LAUNCH_CHECK();
        hipLaunchKernelGGL(prop_count_kernel, grid, block, 0, stream, p, hist, counts);
        CS_LAUNCH_CHECK();
        hipLaunchKernelGGL(prop_take_kernel, grid, block, 0, stream, p, hist, counts, sel);
        CS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(prop_rows_kernel, dim3(L, B), dim3(CSP_ROWS_THREADS), 0, stream, p, dc, min_bbox_size, sel, anchors, lda, max_shape, boxes, scores,
                       group, anchor_inds);
    CS_LAUNCH_CHECK();
    return 0;
}
