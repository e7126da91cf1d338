// Detector training targets (include/clipself_assign.h): IoU assignment, random sampling and box-delta targets, all on the stream,
// fixed-shape outputs, no host read-back.  DESIGN.md §3.15.
//
//   assign_init_kernel     gt_max = 0, gt_row = INT_MAX for every (image, ground truth) of the workspace
//   assign_max_kernel      thread = one box, the image's ground truths in LDS: max / argmax over them, the thresholds, and the
//                          per-ground-truth maximum through an integer atomicMax on the IoU's bits
//   assign_lowq_kernel     match_low_quality: recomputes the IoUs against the ground truths with gt_max >= min_pos_iou; <true> writes the
//                          largest matching i + 1 (gt_max_assign_all), <false> records each ground truth's lowest matching row
//   assign_lowq_row_kernel ... and gives each row the largest i whose lowest matching row it is
//   sample_kernel          one workgroup per image, both pools per pass: count, radix select on the 32-bit key, ordered take into sel
//   targets_kernel         one thread per (image, row) or per (image, slot of sel)
//
// Every index that comes from device memory (starts, gt_starts, gt_inds, sel) is clamped or compared before it is used.
#include "det_common.h"
#include "../../include/clipself_assign.h"
#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)

#define CSA_THREADS 256
#define CSA_SAMPLE_THREADS 1024

namespace {

// img_range of table tab; tab == NULL (boxes only): the shared form, every image owns rows [0, min(total, cap))
__device__ __forceinline__ Range tab_range(const int* __restrict__ tab, int b, int total, int cap) {
    return tab == nullptr ? Range{0, min(total, cap)} : img_range(tab, b, total, cap);
}

// bbox_overlaps, mode 'iou', eps 1e-6, in the header's arithmetic.  The ONE function both passes call, so that iou == gt_max compares the
// same instructions' results.  Disjoint pairs leave before the division with the 0 the formula gives them (0 / union, union >= 1e-6);
// a NaN anywhere gives 0: a NaN width fails w > 0, a NaN area makes the union NaN (the comparison keeps it), and NaN != NaN at the end.
__device__ __forceinline__ float iou_pair(const float4 a, float area_a, const float4 g, float area_g) {
    const float w = f_sub(fminf(a.z, g.z), fmaxf(a.x, g.x));
    const float h = f_sub(fminf(a.w, g.w), fmaxf(a.y, g.y));
    if (!(w > 0.f && h > 0.f)) return 0.f;
    const float inter = f_mul(w, h);
    const float u = f_sub(f_add(area_a, area_g), inter);
    const float uni = u < 1e-6f ? 1e-6f : u;
    const float iou = f_div(inter, uni);
    return iou == iou ? iou : 0.f;
}

// the image's ground truths into LDS: corners and areas; G <= CSA_MAX_GT
__device__ __forceinline__ void stage_gts(const float* __restrict__ gt_boxes, long ldg, Range g, float4* sg, float* sa) {
    for (int t = threadIdx.x; t < g.n; t += blockDim.x) {
        const float* p = gt_boxes + (size_t)(g.s + t) * ldg;
        const float4 v = make_float4(p[0], p[1], p[2], p[3]);
        sg[t] = v;
        sa[t] = box_area(v.x, v.y, v.z, v.w);
    }
}

// Ground truth i's area, read at the top of the iteration next to its corners.  A plain sa[i] is sunk behind iou_pair's early exit, where
// every intersecting pair then waits for a second LDS round trip (profiles/det_common_ab.md, section 3.1); a volatile read stays put.
// sa is an LDS array: the pointer names the address space because a volatile generic pointer compiles to a flat system-scope load.
__device__ __forceinline__ float area_at(const float* sa, int i) {
    return ((const volatile __attribute__((address_space(3))) float*)sa)[i];
}

}  // namespace

// ------------------------------------------------------------------------------------------------ assign
__global__ __launch_bounds__(CSA_THREADS) void assign_init_kernel(unsigned* __restrict__ gt_max, int* __restrict__ gt_row, int total) {
    const int i = blockIdx.x * CSA_THREADS + threadIdx.x;
    if (i < total) {
        gt_max[i] = 0u;
        gt_row[i] = INT_MAX;
    }
}

// grid (ceil(Nmax / 256), B).  gt_max[b][i] collects max over valid rows of iou(i, row) as an unsigned maximum of the bit patterns: IoUs are
// non-negative and never NaN here, for which the bit order is the value order, and a maximum does not depend on the order of its
// operands -- first among the workgroup's rows in LDS, then one global atomicMax per ground truth the workgroup touched.
__global__ __launch_bounds__(CSA_THREADS) void assign_max_kernel(const float* __restrict__ boxes, long ldb, const int* __restrict__ starts, int K,
                                                                 const float* __restrict__ gt_boxes, long ldg,
                                                                 const int* __restrict__ gt_starts, int Gtot,
                                                                 const unsigned char* __restrict__ valid, int Nmax, int Gmax, float pos_thr,
                                                                 float neg_lo, float neg_hi, int track_gt_max, int gt_prefix,
                                                                 int* __restrict__ gt_inds, float* __restrict__ max_overlaps,
                                                                 unsigned* __restrict__ gt_max) {
    __shared__ float4 sg[CSA_MAX_GT];
    __shared__ float sa[CSA_MAX_GT];
    __shared__ unsigned smax[CSA_MAX_GT];
    const int b = blockIdx.y, row = blockIdx.x * CSA_THREADS + threadIdx.x;
    const Range r = tab_range(starts, b, K, Nmax);
    const Range g = tab_range(gt_starts, b, Gtot, Gmax);
    const int first = blockIdx.x * CSA_THREADS;
    if (first >= r.n) {                                    // the whole workgroup is past the image: padding only
        if (row < Nmax) {
            gt_inds[(size_t)b * Nmax + row] = -1;
            max_overlaps[(size_t)b * Nmax + row] = 0.f;
        }
        return;
    }
    stage_gts(gt_boxes, ldg, g, sg, sa);
    for (int t = threadIdx.x; t < g.n; t += CSA_THREADS) smax[t] = 0u;
    __syncthreads();
    int gi = -1;
    float best = 0.f;
    if (row < r.n) {
        const bool ok = valid == nullptr || valid[r.s + row] != 0;
        if (ok && gt_prefix && row < g.n) {
            gi = row + 1;
            best = 1.f;
        } else if (ok && g.n == 0) {
            gi = 0;
        } else if (ok) {
            const float* p = boxes + (size_t)(r.s + row) * ldb;
            const float4 a = make_float4(p[0], p[1], p[2], p[3]);
            const float area_a = box_area(a.x, a.y, a.z, a.w);
            float mx = -1.f;
            int arg = 0;
#pragma unroll 1                                           // one division in flight: unrolled by three is slower with track_gt_max
            for (int i = 0; i < g.n; ++i) {
                const float v = iou_pair(a, area_a, sg[i], area_at(sa, i));
                if (v > mx) {
                    mx = v;
                    arg = i;
                }
                // smax only grows, so a value that does not exceed what a plain (broadcast) read sees cannot change it; without the
                // read every lane that intersects ground truth i queues on the same LDS word
                if (track_gt_max && v > 0.f && __float_as_uint(v) > smax[i]) atomicMax(&smax[i], __float_as_uint(v));
            }
            best = mx;
            if (mx >= neg_lo && mx < neg_hi) gi = 0;
            if (mx >= pos_thr) gi = arg + 1;
        }
    }
    if (row < Nmax) {
        gt_inds[(size_t)b * Nmax + row] = gi;
        max_overlaps[(size_t)b * Nmax + row] = best;
    }
    if (track_gt_max) {
        __syncthreads();
        for (int t = threadIdx.x; t < g.n; t += CSA_THREADS) {
            const unsigned v = smax[t];
            if (v != 0u) atomicMax(&gt_max[(size_t)b * Gmax + t], v);
        }
    }
}

// grid (ceil(Nmax / 256), B).  ALL: the row takes the largest i with gt_max[i] >= min_pos_iou and iou(i, row) == gt_max[i].  !ALL: each such
// i records its lowest matching row with an integer atomicMin (a minimum does not depend on the order either).
template <bool ALL>
__global__ __launch_bounds__(CSA_THREADS) void assign_lowq_kernel(const float* __restrict__ boxes, long ldb, const int* __restrict__ starts, int K,
                                                                  const float* __restrict__ gt_boxes, long ldg,
                                                                  const int* __restrict__ gt_starts, int Gtot,
                                                                  const unsigned char* __restrict__ valid, int Nmax, int Gmax,
                                                                  float min_pos_iou, int gt_prefix, const unsigned* __restrict__ gt_max,
                                                                  int* __restrict__ gt_row, int* __restrict__ gt_inds) {
    __shared__ float4 sg[CSA_MAX_GT];
    __shared__ float sa[CSA_MAX_GT];
    __shared__ float sm[CSA_MAX_GT];
    const int b = blockIdx.y, row = blockIdx.x * CSA_THREADS + threadIdx.x;
    const Range r = tab_range(starts, b, K, Nmax);
    const Range g = tab_range(gt_starts, b, Gtot, Gmax);
    if ((int)blockIdx.x * CSA_THREADS >= r.n || g.n == 0) return;
    stage_gts(gt_boxes, ldg, g, sg, sa);
    for (int t = threadIdx.x; t < g.n; t += CSA_THREADS) {
        const float m = __uint_as_float(gt_max[(size_t)b * Gmax + t]);
        sm[t] = m >= min_pos_iou ? m : -1.f;               // -1: the rule does not apply to this ground truth (no IoU is negative)
    }
    __syncthreads();
    if (row >= r.n) return;
    if (valid != nullptr && valid[r.s + row] == 0) return;
    if (gt_prefix && row < g.n) return;
    const float* p = boxes + (size_t)(r.s + row) * ldb;
    const float4 a = make_float4(p[0], p[1], p[2], p[3]);
    const float area_a = box_area(a.x, a.y, a.z, a.w);
    int hit = -1;
#pragma unroll 1                                           // as assign_max_kernel
    for (int i = 0; i < g.n; ++i) {
        const float m = sm[i];
        if (m < 0.f) continue;
        if (iou_pair(a, area_a, sg[i], area_at(sa, i)) == m) {
            if (ALL) hit = i;
            else atomicMin(&gt_row[(size_t)b * Gmax + i], row);
        }
    }
    if (ALL && hit >= 0) gt_inds[(size_t)b * Nmax + row] = hit + 1;
}

// grid (ceil(Nmax / 256), B): the row takes the largest i whose recorded lowest matching row it is
__global__ __launch_bounds__(CSA_THREADS) void assign_lowq_row_kernel(const int* __restrict__ starts, int K, const int* __restrict__ gt_starts,
                                                                      int Gtot, int Nmax, int Gmax, const int* __restrict__ gt_row,
                                                                      int* __restrict__ gt_inds) {
    __shared__ int sr[CSA_MAX_GT];
    const int b = blockIdx.y, row = blockIdx.x * CSA_THREADS + threadIdx.x;
    const Range r = tab_range(starts, b, K, Nmax);
    const Range g = tab_range(gt_starts, b, Gtot, Gmax);
    if ((int)blockIdx.x * CSA_THREADS >= r.n || g.n == 0) return;
    for (int t = threadIdx.x; t < g.n; t += CSA_THREADS) sr[t] = gt_row[(size_t)b * Gmax + t];
    __syncthreads();
    if (row >= r.n) return;
    int hit = -1;
    for (int i = 0; i < g.n; ++i)
        if (sr[i] == row) hit = i;
    if (hit >= 0) gt_inds[(size_t)b * Nmax + row] = hit + 1;
}

// ------------------------------------------------------------------------------------------------ sample
namespace {

// 0 not in a pool, 1 positive, 2 negative; gt_inds is device data: anything outside [0, G] is in no pool
__device__ __forceinline__ int pool_of(int gi, int G) { return gi > 0 && gi <= G ? 1 : gi == 0 ? 2 : 0; }

#define CSA_SAMPLE_WAVES (CSA_SAMPLE_THREADS / 64)
#define CSA_SAMPLE_UNROLL 4

struct SampleShared {
    int hist[2][256];
    int wave_cnt[4][CSA_SAMPLE_WAVES];
    int have[2];
    unsigned prefix[2];
    int need[2];
};

}  // namespace

// grid (B), 1024 threads: one workgroup per image, both pools in the same passes over the rows -- one count, four 8-bit radix passes
// (only for a pool that has more rows than wanted), two walks of the ordered take.  A pool's threshold is the want-th smallest key; rows with a
// smaller key are all taken, of those with the threshold key the lowest rows.  The histogram and pool counters are integer sums, the
// same whatever the order of arrival; every position in sel comes from ballots and per-wave counts in row order.
__global__ __launch_bounds__(CSA_SAMPLE_THREADS) void sample_kernel(const int* __restrict__ gt_inds, const unsigned* __restrict__ keys,
                                                                    const int* __restrict__ starts, int K, const int* __restrict__ gt_starts,
                                                                    int Gtot, int Nmax, int Gmax, int num, int expected_pos, float neg_pos_ub,
                                                                    unsigned char* __restrict__ flags, int* __restrict__ sel,
                                                                    int* __restrict__ counts) {
    __shared__ SampleShared sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = tab_range(starts, b, K, Nmax).n, G = tab_range(gt_starts, b, Gtot, Gmax).n;
    const int* gi = gt_inds + (size_t)b * Nmax;
    const unsigned* ky = keys + (size_t)b * Nmax;
    unsigned char* fl = flags + (size_t)b * Nmax;
    int* sl = sel + (size_t)b * num;

    // ---- the pools' sizes
    // The scans below are latency-bound (one workgroup walks up to 2^20 rows): each thread has CSA_SAMPLE_UNROLL independent loads in
    // flight per step.  A row past n reads as gt_inds = -1, which is in no pool.
    int c1 = 0, c2 = 0;
    for (int i0 = tid; i0 < n; i0 += CSA_SAMPLE_UNROLL * CSA_SAMPLE_THREADS) {
        int g4[CSA_SAMPLE_UNROLL];
#pragma unroll
        for (int u = 0; u < CSA_SAMPLE_UNROLL; ++u) {
            const int i = i0 + u * CSA_SAMPLE_THREADS;
            g4[u] = i < n ? gi[i] : -1;
        }
#pragma unroll
        for (int u = 0; u < CSA_SAMPLE_UNROLL; ++u) {
            const int p = pool_of(g4[u], G);
            c1 += p == 1;
            c2 += p == 2;
        }
    }
    if (tid < 2) sh.have[tid] = 0;
    __syncthreads();
    if (c1) atomicAdd(&sh.have[0], c1);
    if (c2) atomicAdd(&sh.have[1], c2);
    __syncthreads();
    const int have1 = sh.have[0], have2 = sh.have[1];
    const int want1 = min(max(expected_pos, 0), num);
    const int npos = min(have1, want1);
    int want2 = num - npos;
    if (neg_pos_ub >= 0.f) {
        const float ub = neg_pos_ub * (float)max(1, npos);
        if (ub < (float)want2) want2 = (int)ub;
    }
    const int nneg = min(have2, want2);

    // ---- thresholds.  Nothing wanted: key < 0 and rank < 0 never hold.  The whole pool wanted: every key is <= 0xFFFFFFFF.
    unsigned thr1 = want1 > 0 ? 0xFFFFFFFFu : 0u, thr2 = want2 > 0 ? 0xFFFFFFFFu : 0u;
    int eq1 = want1 > 0 ? INT_MAX : 0, eq2 = want2 > 0 ? INT_MAX : 0;
    const bool cut1 = want1 > 0 && have1 > want1, cut2 = want2 > 0 && have2 > want2;
    if (cut1 || cut2) {
        unsigned pre1 = 0, pre2 = 0;
        int need1 = want1, need2 = want2;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            if (tid < 512) sh.hist[tid >> 8][tid & 255] = 0;
            __syncthreads();
            for (int i0 = tid; i0 < n; i0 += CSA_SAMPLE_UNROLL * CSA_SAMPLE_THREADS) {
                int g4[CSA_SAMPLE_UNROLL];
                unsigned k4[CSA_SAMPLE_UNROLL];
#pragma unroll
                for (int u = 0; u < CSA_SAMPLE_UNROLL; ++u) {
                    const int i = i0 + u * CSA_SAMPLE_THREADS;
                    g4[u] = i < n ? gi[i] : -1;
                    k4[u] = i < n ? ky[i] : 0u;
                }
#pragma unroll
                for (int u = 0; u < CSA_SAMPLE_UNROLL; ++u) {
                    const int p = pool_of(g4[u], G);
                    if (!((p == 1 && cut1) || (p == 2 && cut2))) continue;
                    const unsigned key = k4[u], pre = p == 1 ? pre1 : pre2;
                    if (pass == 0 || (key >> (shift + 8)) == (pre >> (shift + 8))) atomicAdd(&sh.hist[p - 1][(key >> shift) & 255u], 1);
                }
            }
            __syncthreads();
            if (tid < 128) {                               // wave 0: the positives' digit, wave 1: the negatives'
                const bool cut = wv == 0 ? cut1 : cut2;
                const unsigned pre = wv == 0 ? pre1 : pre2;
                const int need = wv == 0 ? need1 : need2;
                if (cut) {                                 // the digit whose bin holds the need-th key: 4 bins per lane, a wave prefix sum
                    const int* hs = sh.hist[wv];
                    const int h[4] = {hs[4 * lane], hs[4 * lane + 1], hs[4 * lane + 2], hs[4 * lane + 3]};
                    const int s = h[0] + h[1] + h[2] + h[3];
                    int inc = s;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const int v = __shfl_up(inc, o, 64);
                        if (lane >= o) inc += v;
                    }
                    const unsigned long long here = __ballot(inc - s < need && need <= inc);
                    const int src = here ? __ffsll((long long)here) - 1 : 63;      // always found: at least `need` keys carry the prefix
                    if (lane == src) {
                        int cum = inc - s, q = 0;
                        for (; q < 3; ++q) {
                            if (cum + h[q] >= need) break;
                            cum += h[q];
                        }
                        sh.prefix[wv] = pre | ((unsigned)(4 * lane + q) << shift);
                        sh.need[wv] = need - cum;
                    }
                }
            }
            __syncthreads();
            if (cut1) pre1 = sh.prefix[0], need1 = sh.need[0];
            if (cut2) pre2 = sh.prefix[1], need2 = sh.need[1];
            __syncthreads();
        }
        if (cut1) thr1 = pre1, eq1 = need1;
        if (cut2) thr2 = pre2, eq2 = need2;
    }

    // ---- ordered take.  Wave w owns the contiguous rows [w * seg, (w + 1) * seg), so ascending (wave, step, lane) is ascending row and
    // nothing inside a walk needs a workgroup barrier.  Walk A counts, per wave and pool, the rows below the threshold and the rows on it.
    // From those counts every wave knows how many threshold rows and how many taken rows lie in front of it: a threshold row is taken iff
    // fewer than eq threshold rows precede it, so wave w takes below_w + clamp(eq - (threshold rows before w), 0, eq_w).  Walk B then ranks
    // its rows with ballots (the compaction of roi_extract.hip, roi_bin_fill_kernel, per wave) and writes flags and sel.
    const int seg = ((n + CSA_SAMPLE_WAVES - 1) / CSA_SAMPLE_WAVES + 63) / 64 * 64;
    const int r0 = min(wv * seg, n), r1 = min(r0 + seg, n);
    int bl1 = 0, bl2 = 0, on1 = 0, on2 = 0;
    for (int i0 = r0 + lane; i0 < r1; i0 += CSA_SAMPLE_UNROLL * 64) {
        int g4[CSA_SAMPLE_UNROLL];
        unsigned k4[CSA_SAMPLE_UNROLL];
#pragma unroll
        for (int u = 0; u < CSA_SAMPLE_UNROLL; ++u) {
            const int i = i0 + u * 64;
            g4[u] = i < r1 ? gi[i] : -1;
            k4[u] = i < r1 ? ky[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < CSA_SAMPLE_UNROLL; ++u) {
            const int p = pool_of(g4[u], G);
            const unsigned thr = p == 1 ? thr1 : thr2;
            bl1 += p == 1 && k4[u] < thr;
            bl2 += p == 2 && k4[u] < thr;
            on1 += p == 1 && k4[u] == thr;
            on2 += p == 2 && k4[u] == thr;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        bl1 += __shfl_xor(bl1, o, 64);
        bl2 += __shfl_xor(bl2, o, 64);
        on1 += __shfl_xor(on1, o, 64);
        on2 += __shfl_xor(on2, o, 64);
    }
    if (lane == 0) {
        sh.wave_cnt[0][wv] = bl1;
        sh.wave_cnt[1][wv] = bl2;
        sh.wave_cnt[2][wv] = on1;
        sh.wave_cnt[3][wv] = on2;
    }
    for (int i = n + tid; i < Nmax; i += CSA_SAMPLE_THREADS) fl[i] = 0;   // rows past the image; walk B writes every row in front
    __syncthreads();
    int seen1 = 0, seen2 = 0, took1 = 0, took2 = 0;        // threshold rows / taken rows in front of this wave
    {
        int run1 = 0, run2 = 0;
#pragma unroll
        for (int w = 0; w < CSA_SAMPLE_WAVES; ++w) {
            const int o1 = sh.wave_cnt[2][w], o2 = sh.wave_cnt[3][w];
            const int t1 = sh.wave_cnt[0][w] + min(max(eq1 - run1, 0), o1), t2 = sh.wave_cnt[1][w] + min(max(eq2 - run2, 0), o2);
            if (w < wv) seen1 += o1, seen2 += o2, took1 += t1, took2 += t2;
            run1 += o1;
            run2 += o2;
        }
    }
    const unsigned long long lower = (1ull << lane) - 1ull;
    for (int base = r0; base < r1; base += CSA_SAMPLE_UNROLL * 64) {      // wave-uniform bounds: the ballots below see all 64 lanes
        int g4[CSA_SAMPLE_UNROLL];
        unsigned k4[CSA_SAMPLE_UNROLL];
#pragma unroll
        for (int u = 0; u < CSA_SAMPLE_UNROLL; ++u) {
            const int i = base + u * 64 + lane;
            g4[u] = i < r1 ? gi[i] : -1;
            k4[u] = i < r1 ? ky[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < CSA_SAMPLE_UNROLL; ++u) {
            const int i = base + u * 64 + lane;
            const int p = pool_of(g4[u], G);
            const unsigned thr = p == 1 ? thr1 : thr2;
            const bool below = p != 0 && k4[u] < thr, on = p != 0 && k4[u] == thr;
            const unsigned long long e1 = __ballot(on && p == 1), e2 = __ballot(on && p == 2);
            const int rank = p == 1 ? seen1 + __popcll(e1 & lower) : seen2 + __popcll(e2 & lower);
            const bool take = below || (on && rank < (p == 1 ? eq1 : eq2));
            const unsigned long long t1 = __ballot(take && p == 1), t2 = __ballot(take && p == 2);
            if (i < r1) {
                fl[i] = take ? (unsigned char)p : (unsigned char)0;
                if (take) {
                    const int q = p == 1 ? took1 + __popcll(t1 & lower) : took2 + __popcll(t2 & lower);
                    const int lim = p == 1 ? npos : nneg, at = (p == 1 ? 0 : npos) + q;
                    if (q < lim && at < num) sl[at] = i;  // q < lim always: a threshold admits exactly min(have, want) rows
                }
            }
            seen1 += __popcll(e1);
            seen2 += __popcll(e2);
            took1 += __popcll(t1);
            took2 += __popcll(t2);
        }
    }
    for (int t = npos + nneg + tid; t < num; t += CSA_SAMPLE_THREADS) sl[t] = -1;
    if (tid == 0) {
        counts[2 * b] = npos;
        counts[2 * b + 1] = nneg;
    }
}

// ------------------------------------------------------------------------------------------------ targets
// grid (ceil(S / 256), B) with S = Nmax (dense, sel == NULL) or num (compact): one thread per output row
__global__ __launch_bounds__(CSA_THREADS) void targets_kernel(const float* __restrict__ boxes, long ldb, const int* __restrict__ starts, int K,
                                                              const float* __restrict__ gt_boxes, long ldg, const int* __restrict__ gt_labels,
                                                              const int* __restrict__ gt_starts, int Gtot, int Nmax, int Gmax,
                                                              const int* __restrict__ gt_inds, const unsigned char* __restrict__ flags,
                                                              const int* __restrict__ sel, int num, BoxCoder prm, int bg_label,
                                                              float* __restrict__ rois, int* __restrict__ labels,
                                                              float* __restrict__ label_weights, float* __restrict__ bbox_targets,
                                                              float* __restrict__ bbox_weights) {
    const int b = blockIdx.y, t = blockIdx.x * CSA_THREADS + threadIdx.x;
    const int S = sel ? num : Nmax;
    if (t >= S) return;
    const Range r = tab_range(starts, b, K, Nmax);
    const Range g = tab_range(gt_starts, b, Gtot, Gmax);
    int row = t;
    bool sampled;
    if (sel) {
        row = sel[(size_t)b * num + t];
        sampled = row >= 0 && row < r.n;
    } else {
        sampled = row < r.n && flags[(size_t)b * Nmax + row] != 0;
    }
    int gi = -1;
    if (sampled) {
        gi = gt_inds[(size_t)b * Nmax + row];
        if (gi < -1 || gi > g.n) gi = -1;
    }
    const bool pos = sampled && gi > 0 && (sel != nullptr || flags[(size_t)b * Nmax + row] == 1);
    int label = bg_label;
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    const float* p = sampled ? boxes + (size_t)(r.s + row) * ldb : nullptr;
    if (pos) {
        if (gt_labels) label = gt_labels[g.s + gi - 1];
        else label = 0;
        encode_delta(prm, p, gt_boxes + (size_t)(g.s + gi - 1) * ldg, d);
    }
    const size_t o = (size_t)b * S + t;
    labels[o] = label;
    label_weights[o] = sampled ? 1.f : 0.f;
    const float w = pos ? 1.f : 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        bbox_targets[o * 4 + c] = d[c];
        bbox_weights[o * 4 + c] = w;
    }
    if (sel) {
        float* rp = rois + o * 5;
        rp[0] = sampled ? (float)b : -1.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) rp[1 + c] = sampled ? p[c] : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ host side
namespace {
size_t up256(size_t n) { return (n + 255) / 256 * 256; }
bool shape_ok(int B, int Nmax, int Gmax, int num) {
    return B >= 1 && B <= 65535 && Nmax >= 0 && Nmax <= CSA_MAX_ROWS && Gmax >= 0 && Gmax <= CSA_MAX_GT && num >= 1 && num <= CSA_MAX_NUM;
}
}  // namespace

#define CSA_CHECK_SHAPE(who)                                                                                                    \
    CS_CHECK_ARG(B >= 1 && B <= 65535, who ": B = %d must be in [1, 65535]", B);                                                \
    CS_CHECK_ARG(Nmax >= 0 && Nmax <= CSA_MAX_ROWS, who ": Nmax = %d must be in [0, %d]", Nmax, CSA_MAX_ROWS);                  \
    CS_CHECK_ARG(Gmax >= 0 && Gmax <= CSA_MAX_GT, who ": Gmax = %d must be in [0, %d]", Gmax, CSA_MAX_GT);                      \
    CS_CHECK_ARG(K >= 0 && Gtot >= 0, who ": K = %d and Gtot = %d must be >= 0", K, Gtot);                                     \
    CS_CHECK_ARG(gt_starts != nullptr, who ": gt_starts must not be NULL")

extern "C" size_t csa_workspace(int B, int Nmax, int Gmax, int num) {
    if (!shape_ok(B, Nmax, Gmax, num)) return 0;
    return up256((size_t)B * Gmax * sizeof(unsigned)) + up256((size_t)B * Gmax * sizeof(int)) + 256;
}

extern "C" int csa_assign(const float* boxes, long ldb, const int* starts, int K, const float* gt_boxes, long ldg, const int* gt_starts,
                          int Gtot, const unsigned char* valid, int B, int Nmax, int Gmax, float pos_iou_thr, float neg_lo, float neg_hi,
                          float min_pos_iou, int match_low_quality, int gt_max_assign_all, int gt_prefix, int* gt_inds, float* max_overlaps,
                          void* workspace, hipStream_t stream) {
    CSA_CHECK_SHAPE("csa_assign");
    CS_CHECK_ARG(ldb >= 4 && ldg >= 4, "csa_assign: ldb = %ld and ldg = %ld must be >= 4", ldb, ldg);
    CS_CHECK_ARG(K == 0 || boxes, "csa_assign: boxes must not be NULL when K > 0");
    CS_CHECK_ARG(Gtot == 0 || gt_boxes, "csa_assign: gt_boxes must not be NULL when Gtot > 0");
    CS_CHECK_ARG(Nmax == 0 || (gt_inds && max_overlaps), "csa_assign: gt_inds and max_overlaps must not be NULL");
    CS_CHECK_ARG(workspace != nullptr, "csa_assign: workspace is NULL (csa_workspace() bytes are needed)");
    if (Nmax == 0) return 0;
    unsigned* gt_max = (unsigned*)workspace;
    int* gt_row = (int*)((char*)workspace + up256((size_t)B * Gmax * sizeof(unsigned)));
    const int lowq = match_low_quality && Gmax > 0;
    const dim3 grid((Nmax + CSA_THREADS - 1) / CSA_THREADS, B);
    if (lowq) {
        const int total = B * Gmax;
        hipLaunchKernelGGL(assign_init_kernel, dim3((total + CSA_THREADS - 1) / CSA_THREADS), dim3(CSA_THREADS), 0, stream, gt_max, gt_row, total);
        CS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(assign_max_kernel, grid, dim3(CSA_THREADS), 0, stream, boxes, ldb, starts, K, gt_boxes, ldg, gt_starts, Gtot, valid, Nmax,
                       Gmax, pos_iou_thr, neg_lo, neg_hi, lowq, gt_prefix, gt_inds, max_overlaps, gt_max);
    CS_LAUNCH_CHECK();
    if (lowq) {
        hipLaunchKernelGGL(gt_max_assign_all ? assign_lowq_kernel<true> : assign_lowq_kernel<false>, grid, dim3(CSA_THREADS), 0, stream, boxes, ldb,
                           starts, K, gt_boxes, ldg, gt_starts, Gtot, valid, Nmax, Gmax, min_pos_iou, gt_prefix, gt_max, gt_row, gt_inds);
        CS_LAUNCH_CHECK();
        if (!gt_max_assign_all) {
            hipLaunchKernelGGL(assign_lowq_row_kernel, grid, dim3(CSA_THREADS), 0, stream, starts, K, gt_starts, Gtot, Nmax, Gmax, gt_row, gt_inds);
            CS_LAUNCH_CHECK();
        }
    }
    return 0;
}

extern "C" int csa_sample(const int* gt_inds, const unsigned int* keys, const int* starts, int K, const int* gt_starts, int Gtot, int B,
                          int Nmax, int Gmax, int num, int expected_pos, float neg_pos_ub, unsigned char* flags, int* sel, int* counts,
                          hipStream_t stream) {
    CSA_CHECK_SHAPE("csa_sample");
    CS_CHECK_ARG(num >= 1 && num <= CSA_MAX_NUM, "csa_sample: num = %d must be in [1, %d]", num, CSA_MAX_NUM);
    CS_CHECK_ARG(expected_pos >= 0 && expected_pos <= num, "csa_sample: expected_pos = %d must be in [0, num = %d]", expected_pos, num);
    CS_CHECK_ARG(Nmax == 0 || (gt_inds && keys && flags), "csa_sample: gt_inds, keys and flags must not be NULL");
    CS_CHECK_ARG(sel && counts, "csa_sample: sel and counts must not be NULL");
    hipLaunchKernelGGL(sample_kernel, dim3(B), dim3(CSA_SAMPLE_THREADS), 0, stream, gt_inds, keys, starts, K, gt_starts, Gtot, Nmax, Gmax, num,
                       expected_pos, neg_pos_ub, flags, sel, counts);
    CS_LAUNCH_CHECK();
    return 0;
}

extern "C" int csa_targets(const float* boxes, long ldb, const int* starts, int K, const float* gt_boxes, long ldg, const int* gt_labels,
                           const int* gt_starts, int Gtot, int B, int Nmax, int Gmax, const int* gt_inds, const unsigned char* flags,
                           const int* sel, int num, const float* means, const float* stds, int bg_label, float pos_weight, float* rois,
                           int* labels, float* label_weights, float* bbox_targets, float* bbox_weights, hipStream_t stream) {
    CSA_CHECK_SHAPE("csa_targets");
    CS_CHECK_ARG(ldb >= 4 && ldg >= 4, "csa_targets: ldb = %ld and ldg = %ld must be >= 4", ldb, ldg);
    CS_CHECK_ARG(sel == nullptr || (num >= 1 && num <= CSA_MAX_NUM), "csa_targets: num = %d must be in [1, %d]", num, CSA_MAX_NUM);
    CS_CHECK_ARG(pos_weight <= 0.f, "csa_targets: pos_weight = %g is not supported (only pos_weight <= 0)", (double)pos_weight);
    CS_CHECK_ARG(means && stds, "csa_targets: means and stds (host float[4]) must not be NULL");
    CS_CHECK_ARG(K == 0 || boxes, "csa_targets: boxes must not be NULL when K > 0");
    CS_CHECK_ARG(Gtot == 0 || gt_boxes, "csa_targets: gt_boxes must not be NULL when Gtot > 0");
    CS_CHECK_ARG(sel != nullptr || Nmax == 0 || flags, "csa_targets: the dense form (sel == NULL) needs flags");
    CS_CHECK_ARG(sel == nullptr || rois, "csa_targets: the compact form (sel != NULL) needs rois");
    CS_CHECK_ARG(Nmax == 0 || gt_inds, "csa_targets: gt_inds must not be NULL");
    const int S = sel ? num : Nmax;
    if (S == 0) return 0;
    CS_CHECK_ARG(labels && label_weights && bbox_targets && bbox_weights, "csa_targets: the four target outputs must not be NULL");
    BoxCoder prm;                                          // max_ratio belongs to the decode: not read here
    for (int c = 0; c < 4; ++c) prm.mean[c] = means[c], prm.std[c] = stds[c];
    prm.max_ratio = 0.f;
    hipLaunchKernelGGL(targets_kernel, dim3((S + CSA_THREADS - 1) / CSA_THREADS, B), dim3(CSA_THREADS), 0, stream, boxes, ldb, starts, K, gt_boxes,
                       ldg, gt_labels, gt_starts, Gtot, Nmax, Gmax, gt_inds, flags, sel, num, prm, bg_label, rois, labels, label_weights,
                       bbox_targets, bbox_weights);
    CS_LAUNCH_CHECK();
    return 0;
}
