// Detector post-processing (include/clipself_det.h): box decoding, score thresholding, per-list greedy NMS and the per-image top-max_num
// cut, all on the stream, fixed-shape outputs, no host read-back.  DESIGN.md §3.13.
//
//   nms_mask_kernel   M[b][i][j] = iou(i, j) > iou_thr (and same group), one bit matrix per image shared by all C classes
//   nms_scan_kernel   one wave per list (image, class | group): collect candidates as 64-bit keys, sort, greedy scan over M's rows
//   nms_topk_kernel   one workgroup per image: exact radix select of the max_num best kept keys, sort, gather, pad, counts
//   delta2bbox_kernel one thread per box
//
// Every index that comes from device memory (starts, group, the keys in the workspace) is clamped or compared before it is used.
#include "det_common.h"
#include "../../include/clipself_det.h"

// CSD_MAX_BOXES (Kmax): 256 bitset words per row = 4 registers per lane of the scanning wave; CSD_MAX_NUM: the selected keys are
// sorted in 32 KiB of LDS
#define CSD_LDS_KEYS 2048            // most keys a scanning wave sorts in LDS (16 KiB); a longer list sorts in the workspace
#define CSD_TOPK_THREADS 1024

// mmcv nms, offset 0: inter / (area_a + area_b - inter) > thr, fp32, IEEE division.  NaN or 0/0 compares false.
__device__ __forceinline__ bool iou_gt(const float4 a, float area_a, const float4 b, float area_b, float thr) {
    const float iw = fmaxf(f_sub(fminf(a.z, b.z), fmaxf(a.x, b.x)), 0.f);
    const float ih = fmaxf(f_sub(fminf(a.w, b.w), fmaxf(a.y, b.y)), 0.f);
    const float inter = f_mul(iw, ih);
    const float uni = f_sub(f_add(area_a, area_b), inter);
    return f_div(inter, uni) > thr;
}

// ------------------------------------------------------------------------------------------------ mask
// grid (ceil(W / TJ), ceil(Kmax / 256), B), 256 threads: thread = row i of the image, TJ tiles of 64 column boxes staged in LDS.
// TJ = 4 (32 contiguous bytes of the row per thread) for images past 4096 boxes, TJ = 1 below: 1000 boxes x 8 images are only 128
// workgroups at TJ = 4.
template <int TJ>
__global__ __launch_bounds__(256) void nms_mask_kernel(const float* __restrict__ boxes, long ldb, const int* __restrict__ starts,
                                                       const int* __restrict__ group, int K, int Kmax, int W, float iou_thr,
                                                       u64* __restrict__ M, int* __restrict__ img_total) {
    __shared__ float4 cb[64 * TJ];
    __shared__ float ca[64 * TJ];
    __shared__ int cg[64 * TJ];
    const int tid = threadIdx.x, b = blockIdx.z;
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) img_total[b] = 0;      // the scan kernel's per-image append counter
    const Range r = img_range(starts, b, K, Kmax);
    if ((int)blockIdx.y * 256 >= r.n) return;
    const int j0 = blockIdx.x * (64 * TJ);
    if (tid < 64 * TJ) {
        const int j = j0 + tid;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        int g = 0;
        if (j < r.n) {
            const float* p = boxes + (size_t)(r.s + j) * ldb;
            v = make_float4(p[0], p[1], p[2], p[3]);
            if (group) g = group[r.s + j];
        }
        cb[tid] = v;
        ca[tid] = box_area(v.x, v.y, v.z, v.w);
        cg[tid] = g;
    }
    __syncthreads();
    const int i = blockIdx.y * 256 + tid;
    if (i >= r.n) return;
    const float* p = boxes + (size_t)(r.s + i) * ldb;
    const float4 a = make_float4(p[0], p[1], p[2], p[3]);
    const float area_a = box_area(a.x, a.y, a.z, a.w);
    const int ga = group ? group[r.s + i] : 0;
    u64* row = M + ((size_t)b * Kmax + i) * W;
#pragma unroll 1
    for (int t = 0; t < TJ; ++t) {
        const int jt = blockIdx.x * TJ + t;
        if (jt >= W) break;
        const int ncol = min(64, r.n - jt * 64);           // columns past the image's boxes stay 0
        u64 word = 0;
        for (int jj = 0; jj < ncol; ++jj) {
            const int c = t * 64 + jj;
            const bool hit = iou_gt(a, area_a, cb[c], ca[c], iou_thr) && cg[c] == ga;
            word |= (u64)hit << jj;
        }
        row[jt] = word;
    }
}

// ------------------------------------------------------------------------------------------------ scan
// grid (L, B), 64 threads: one wave owns one list.  L = C (list = class blockIdx.x) or G (list = group blockIdx.x, scores column 0).
// CAP: keys of LDS per wave, the smallest of 512 / 1024 / 2048 that holds Kmax (more waves per CU for the many short lists of a large C).
template <int CAP>
__global__ __launch_bounds__(64) void nms_scan_kernel(const float* __restrict__ scores, long lds, int C, const int* __restrict__ starts,
                                                      const int* __restrict__ group, int K, int Kmax, int Kp, int W, float score_thr,
                                                      int max_num, const u64* __restrict__ M, u64* __restrict__ sort_scratch,
                                                      u64* __restrict__ img_keys, int* __restrict__ img_total, int cap_img) {
    __shared__ u64 lds_keys[CAP];
    const int lane = threadIdx.x, l = blockIdx.x, b = blockIdx.y, L = gridDim.x;
    const Range r = img_range(starts, b, K, Kmax);
    if (r.n == 0) return;
    // r.n > CAP happens only with CAP = CSD_LDS_KEYS < Kmax, which is when the host passes sort_scratch (Kp keys per list, Kp = pow2 >= Kmax)
    u64* keys = r.n <= CAP ? lds_keys : sort_scratch + ((size_t)b * L + l) * Kp;
    const int col = group ? 0 : l;

    // (a) candidates: score > score_thr (false for NaN), in the group form also group == l
    int n = 0;
    for (int base = 0; base < r.n; base += 64) {
        const int k = base + lane;
        bool cand = false;
        float sc = 0.f;
        if (k < r.n) {
            sc = scores[(size_t)(r.s + k) * lds + col];
            cand = sc > score_thr;
            if (group) cand = cand && group[r.s + k] == l;
        }
        const u64 m = __ballot(cand);
        if (cand) keys[n + __popcll(m & ((1ull << lane) - 1ull))] = ((u64)(~ord_bits(sc)) << 32) | (uint32_t)k;
        n += __popcll(m);
    }
    if (n == 0) return;
    if (r.n > CAP && n <= CAP) {                           // an image past the LDS share whose list fits it (an FPN level's 2000): sort in LDS
        __threadfence_block();
        __syncthreads();
        for (int t = lane; t < n; t += 64) lds_keys[t] = keys[t];
        keys = lds_keys;
    }

    // (b) sort ascending: score descending, ties by ascending box row
    const int P = next_pow2(n);
    for (int t = n + lane; t < P; t += 64) keys[t] = ~0ull;
    __threadfence_block();
    __syncthreads();
    bitonic_sort(keys, P, lane, 64);

    // (c) greedy scan: the suppressed set is a bitset in registers, word w in lane w & 63, register w >> 6
    u64 sup0 = 0, sup1 = 0, sup2 = 0, sup3 = 0;
    const u64* Mb = M + (size_t)b * Kmax * W;
    int cnt = 0;
    for (int i = 0; i < n && cnt < max_num; ++i) {
        const u64 key = keys[i];
        uint32_t k = __builtin_amdgcn_readfirstlane((uint32_t)key);
        if (k >= (uint32_t)r.n) continue;                   // cannot happen: the key was built above from k < r.n
        const int w = k >> 6, reg = w >> 6;
        const u64 sel = reg == 0 ? sup0 : reg == 1 ? sup1 : reg == 2 ? sup2 : sup3;
        const uint32_t half = (k & 32) ? (uint32_t)(sel >> 32) : (uint32_t)sel;
        const uint32_t word = __builtin_amdgcn_readlane(half, w & 63);
        if ((word >> (k & 31)) & 1u) continue;
        if (lane == 0) keys[cnt] = key;                    // cnt <= i: the kept run grows in place behind the read position
        ++cnt;
        const u64* row = Mb + (size_t)k * W;
        if (lane < W) sup0 |= row[lane];
        if (lane + 64 < W) sup1 |= row[lane + 64];
        if (lane + 128 < W) sup2 |= row[lane + 128];
        if (lane + 192 < W) sup3 |= row[lane + 192];
    }
    __threadfence_block();
    __syncthreads();

    // append the kept run to the image's key buffer with the flat index k_local * C + c (group form: the box row) in the low word.
    // The slot comes from an integer counter; nms_topk_kernel selects and sorts unique keys, so the order of arrival changes nothing.
    int base = 0;
    if (lane == 0) base = atomicAdd(&img_total[b], cnt);
    base = __builtin_amdgcn_readfirstlane(base);
    u64* dst = img_keys + (size_t)b * cap_img;
    for (int t = lane; t < cnt; t += 64) {
        const u64 key = keys[t];
        const uint32_t kl = (uint32_t)key;
        const uint32_t flat = group ? kl : kl * (uint32_t)C + (uint32_t)l;
        if (base >= 0 && base + t < cap_img) dst[base + t] = (key & 0xFFFFFFFF00000000ull) | flat;
    }
}

// ------------------------------------------------------------------------------------------------ top-k
// grid (B), 1024 threads.  Keys are unique (the flat index is), so the max_num-th smallest key is an exact threshold.
__global__ __launch_bounds__(CSD_TOPK_THREADS) void nms_topk_kernel(const float* __restrict__ boxes, long ldb, int C,
                                                                    const int* __restrict__ starts, const int* __restrict__ group, int K,
                                                                    int Kmax, int max_num, const u64* __restrict__ img_keys,
                                                                    const int* __restrict__ img_total, int cap_img, int active,
                                                                    float* __restrict__ dets, int* __restrict__ labels,
                                                                    int* __restrict__ inds, int* __restrict__ counts) {
    __shared__ u64 sel[CSD_MAX_NUM];
    __shared__ int hist[256];
    __shared__ u64 s_prefix;
    __shared__ int s_need, s_cnt;
    const int tid = threadIdx.x, b = blockIdx.x;
    Range r;
    r.s = 0;
    r.n = 0;
    int T = 0;
    if (active) {
        r = img_range(starts, b, K, Kmax);
        if (r.n > 0) T = min(max(img_total[b], 0), cap_img);
    }
    const u64* keys = img_keys + (size_t)b * cap_img;
    u64 thresh = ~0ull;
    if (T > max_num) {
        u64 prefix = 0;
        int need = max_num;
        for (int pass = 0; pass < 8; ++pass) {
            const int shift = 56 - 8 * pass;
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < T; i += CSD_TOPK_THREADS) {
                const u64 key = keys[i];
                if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(int)((key >> shift) & 255)], 1);
            }
            __syncthreads();
            if (tid < 64) {                                // the digit whose bin holds the need-th key: 4 bins per lane, a wave prefix sum
                const int h[4] = {hist[4 * tid], hist[4 * tid + 1], hist[4 * tid + 2], hist[4 * tid + 3]};
                const int s = h[0] + h[1] + h[2] + h[3];
                int inc = s;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int v = __shfl_up(inc, o, 64);
                    if (tid >= o) inc += v;
                }
                const u64 here = __ballot(inc - s < need && need <= inc);
                const int src = here ? __ffsll((long long)here) - 1 : 63;      // always found: at least `need` keys carry the prefix
                if (tid == src) {
                    int cum = inc - s, q = 0;
                    for (; q < 3; ++q) {
                        if (cum + h[q] >= need) break;
                        cum += h[q];
                    }
                    s_prefix = prefix | ((u64)(4 * tid + q) << shift);
                    s_need = need - cum;
                }
            }
            __syncthreads();
            prefix = s_prefix;
            need = s_need;
        }
        thresh = prefix;
    }
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for (int i = tid; i < T; i += CSD_TOPK_THREADS) {
        const u64 key = keys[i];
        if (key <= thresh) {
            const int pos = atomicAdd(&s_cnt, 1);
            if (pos < CSD_MAX_NUM) sel[pos] = key;
        }
    }
    __syncthreads();
    const int m = min(s_cnt, max_num);
    const int P = next_pow2(max(m, 1));
    for (int t = m + tid; t < P; t += CSD_TOPK_THREADS) sel[t] = ~0ull;
    __syncthreads();
    bitonic_sort(sel, P, tid, CSD_TOPK_THREADS);

    for (int t = tid; t < max_num; t += CSD_TOPK_THREADS) {
        uint32_t x0 = 0, y0 = 0, x1 = 0, y1 = 0, sc = 0;
        int lab = -1, ind = -1;
        if (t < m) {
            const u64 key = sel[t];
            const uint32_t flat = (uint32_t)key;
            const uint32_t kl = group ? flat : flat / (uint32_t)C;
            if (kl < (uint32_t)r.n) {
                ind = r.s + (int)kl;
                lab = group ? group[ind] : (int)(flat % (uint32_t)C);
                const uint32_t* p = (const uint32_t*)(boxes + (size_t)ind * ldb);
                x0 = p[0], y0 = p[1], x1 = p[2], y1 = p[3];
                sc = __float_as_uint(ord_float(~(uint32_t)(key >> 32)));
            }
        }
        uint32_t* d = (uint32_t*)(dets + ((size_t)b * max_num + t) * 5);
        d[0] = x0, d[1] = y0, d[2] = x1, d[3] = y1, d[4] = sc;
        labels[(size_t)b * max_num + t] = lab;
        inds[(size_t)b * max_num + t] = ind;
    }
    if (tid == 0) counts[b] = m;
}

// ------------------------------------------------------------------------------------------------ host side of the NMS
namespace {
struct NmsPlan {
    int W, Kp, cap_img;
    size_t off_mask, off_keys, off_scratch, total;
};
size_t up256(size_t n) { return (n + 255) / 256 * 256; }

NmsPlan nms_plan(int B, int Kmax, int L, int max_num, bool group_form) {
    NmsPlan p;
    p.W = (Kmax + 63) / 64;
    p.Kp = 1;
    while (p.Kp < Kmax) p.Kp <<= 1;
    const size_t run = (size_t)(max_num < Kmax ? max_num : Kmax);          // a list stops after max_num keeps
    size_t cap = (size_t)L * run;
    if (group_form && cap > (size_t)Kmax) cap = (size_t)Kmax;              // a box is in one group only
    if (cap > 0x7FFFFFFFu) cap = 0x7FFFFFFFu;                              // never reached: Kmax * C < 2^31
    p.cap_img = (int)cap;
    p.off_mask = up256((size_t)B * sizeof(int));
    p.off_keys = p.off_mask + up256((size_t)B * Kmax * p.W * sizeof(u64));
    p.off_scratch = p.off_keys + up256((size_t)B * cap * sizeof(u64));
    p.total = p.off_scratch + (Kmax > CSD_LDS_KEYS ? up256((size_t)B * L * p.Kp * sizeof(u64)) : 0);
    return p;
}
bool nms_shape_ok(int B, int Kmax, int L, int max_num) {
    return B >= 1 && B <= 65535 && L >= 1 && Kmax >= 0 && Kmax <= CSD_MAX_BOXES && (long long)Kmax * L < (1ll << 31) && max_num >= 1 &&
           max_num <= CSD_MAX_NUM;
}
}  // namespace

// The workspace of the multi-class form (C lists per image) covers the group form with G <= C lists as well.
extern "C" size_t csd_nms_workspace(int B, int Kmax, int C_or_G, int max_num) {
    if (!nms_shape_ok(B, Kmax, C_or_G, max_num)) return 0;
    return nms_plan(B, Kmax, C_or_G, max_num, false).total;
}

extern "C" int csd_nms(const float* boxes, long ldb, const float* scores, long lds, int C, const int* starts, const int* group, int G, int K,
                       int B, int Kmax, float score_thr, float iou_thr, int max_num, float* dets, int* labels, int* inds, int* counts,
                       void* workspace, hipStream_t stream) {
    CS_CHECK_ARG(B >= 1 && B <= 65535, "csd_nms: B = %d must be in [1, 65535]", B);
    CS_CHECK_ARG(C >= 1, "csd_nms: C = %d must be >= 1", C);
    CS_CHECK_ARG(K >= 0, "csd_nms: K = %d must be >= 0", K);
    CS_CHECK_ARG(Kmax >= 0 && Kmax <= CSD_MAX_BOXES, "csd_nms: Kmax = %d must be in [0, %d]", Kmax, CSD_MAX_BOXES);
    CS_CHECK_ARG((long long)Kmax * C < (1ll << 31), "csd_nms: Kmax * C = %lld must be below 2^31", (long long)Kmax * C);
    CS_CHECK_ARG(max_num >= 1 && max_num <= CSD_MAX_NUM, "csd_nms: max_num = %d must be in [1, %d]", max_num, CSD_MAX_NUM);
    CS_CHECK_ARG(ldb >= 4, "csd_nms: ldb = %ld must be >= 4", ldb);
    CS_CHECK_ARG(lds >= C, "csd_nms: lds = %ld must be >= C = %d", lds, C);
    CS_CHECK_ARG(group == nullptr || C == 1, "csd_nms: group is given with C = %d (the group form needs C == 1)", C);
    CS_CHECK_ARG(group == nullptr || (G >= 1 && (long long)Kmax * G < (1ll << 31)), "csd_nms: G = %d must be >= 1 (and Kmax * G < 2^31) when group is given", G);
    CS_CHECK_ARG(starts && dets && labels && inds && counts, "csd_nms: starts and the four outputs must not be NULL");
    CS_CHECK_ARG(K == 0 || (boxes && scores), "csd_nms: boxes and scores must not be NULL when K > 0");
    CS_CHECK_ARG(workspace != nullptr, "csd_nms: workspace is NULL (csd_nms_workspace() bytes are needed)");
    const int L = group ? G : C;
    const NmsPlan p = nms_plan(B, Kmax, L, max_num, group != nullptr);
    char* ws = (char*)workspace;
    int* img_total = (int*)ws;
    u64* M = (u64*)(ws + p.off_mask);
    u64* img_keys = (u64*)(ws + p.off_keys);
    u64* scratch = Kmax > CSD_LDS_KEYS ? (u64*)(ws + p.off_scratch) : nullptr;
    const int active = (K > 0 && Kmax > 0) ? 1 : 0;
    if (active) {
        const int tj = Kmax > 4096 ? 4 : 1;
        dim3 gm((p.W + tj - 1) / tj, (Kmax + 255) / 256, B);
        hipLaunchKernelGGL(tj == 4 ? nms_mask_kernel<4> : nms_mask_kernel<1>, gm, dim3(256), 0, stream, boxes, ldb, starts, group, K, Kmax,
                           p.W, iou_thr, M, img_total);
        CS_LAUNCH_CHECK();
        auto scan = Kmax <= 512 ? nms_scan_kernel<512> : Kmax <= 1024 ? nms_scan_kernel<1024> : nms_scan_kernel<CSD_LDS_KEYS>;
        hipLaunchKernelGGL(scan, dim3(L, B), dim3(64), 0, stream, scores, lds, C, starts, group, K, Kmax, p.Kp, p.W, score_thr, max_num, M,
                           scratch, img_keys, img_total, p.cap_img);
        CS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(nms_topk_kernel, dim3(B), dim3(CSD_TOPK_THREADS), 0, stream, boxes, ldb, C, starts, group, K, Kmax, max_num, img_keys,
                       img_total, p.cap_img, active, dets, labels, inds, counts);
    CS_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------ delta2bbox
// mmdet 2.x DeltaXYWHBBoxCoder.decode (decode_box, clip_border=True), then bboxes / scale_factor
__global__ __launch_bounds__(256) void delta2bbox_kernel(const float* __restrict__ rois, long ldr, const float* __restrict__ deltas, long ldd,
                                                         const int* __restrict__ starts, int B, int K, BoxCoder prm,
                                                         const float* __restrict__ max_shape, const float* __restrict__ scale,
                                                         float* __restrict__ out, long ldo) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    int b = 0;
    if (max_shape || scale) {
        // image of row k: the number of starts[1..B-1] that are <= k.  starts is device data: the result is an index in [0, B) whatever it holds
        int lo = 0, hi = B - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (starts[mid] <= k) lo = mid; else hi = mid - 1;
        }
        b = lo;
    }
    float o[4];
    decode_box(prm, rois + (size_t)k * ldr, deltas + (size_t)k * ldd, max_shape ? max_shape + b * 2 : nullptr, o);
    if (scale) {
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = f_div(o[q], scale[b * 4 + q]);
    }
    float* op = out + (size_t)k * ldo;
    op[0] = o[0], op[1] = o[1], op[2] = o[2], op[3] = o[3];
}

extern "C" int csd_delta2bbox(const float* rois, long ldr, const float* deltas, long ldd, const int* starts, int B, int K, const float* means,
                              const float* stds, float wh_ratio_clip, const float* max_shape, const float* scale, float* out_boxes, long ldo,
                              hipStream_t stream) {
    CS_CHECK_ARG(K >= 0, "csd_delta2bbox: K = %d must be >= 0", K);
    CS_CHECK_ARG(ldr >= 4 && ldd >= 4 && ldo >= 4, "csd_delta2bbox: ldr = %ld, ldd = %ld, ldo = %ld must be >= 4", ldr, ldd, ldo);
    CS_CHECK_ARG(means && stds, "csd_delta2bbox: means and stds (host float[4]) must not be NULL");
    CS_CHECK_ARG(wh_ratio_clip > 0.f, "csd_delta2bbox: wh_ratio_clip = %g must be positive", (double)wh_ratio_clip);
    CS_CHECK_ARG((max_shape == nullptr && scale == nullptr) || (starts != nullptr && B >= 1),
                 "csd_delta2bbox: max_shape / scale are per image and need starts [B + 1] with B >= 1 (B = %d)", B);
    if (K == 0) return 0;
    CS_CHECK_ARG(rois && deltas && out_boxes, "csd_delta2bbox: rois, deltas and out_boxes must not be NULL when K > 0");
    BoxCoder prm;
    for (int q = 0; q < 4; ++q) prm.mean[q] = means[q], prm.std[q] = stds[q];
    prm.max_ratio = coder_max_ratio(wh_ratio_clip);
    hipLaunchKernelGGL(delta2bbox_kernel, dim3((K + 255) / 256), dim3(256), 0, stream, rois, ldr, deltas, ldd, starts, B, K, prm, max_shape,
                       scale, out_boxes, ldo);
    CS_LAUNCH_CHECK();
    return 0;
}
