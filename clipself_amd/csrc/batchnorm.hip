// Batch norm (+ ReLU) on channel-last maps, forward and backward (include/clipself_bn.h).
//
// Streaming kernels: a map is rows [M, C]; a thread owns one 16-byte channel group (8 bf16 or 4 fp32 channels) and walks rows, four
// independent 16-byte loads in flight; GT (a power of two <= 64) neighbouring threads cover GT neighbouring groups of a row, so a wave
// reads whole contiguous segments, and the 256 / GT thread rows of a workgroup take consecutive rows.  The rows are cut into P contiguous
// parts (blockIdx.x), the channel groups into tiles of GT (blockIdx.y).  Reductions have two levels and a fixed order: thread (rows
// ascending) -> pairwise LDS tree over the thread rows -> per-part partials in the workspace -> bn_combine_kernel (16 ascending slices,
// then a pairwise tree).  No atomics.
#include "cs_common.h"
#include "../../include/clipself_bn.h"

namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_MIN_ROWS = 64;          // a row part holds at least this many rows (but for the last)
constexpr int BN_BLOCKS_PER_CU = 4;      // workgroups per CU the row partition aims at: every one resident at once, 16 waves per CU

struct Geo {
    long M, rpb;          // rows, rows per part
    int C, G, gl, P;      // channels, channel groups of VEC, log2(GT), row parts
};

int bn_num_cus() {
    static const int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        return v;
    }();
    return n;
}

// rows per part and P from M, C and the CU count only (not from the operand types): about BN_BLOCKS_PER_CU workgroups per CU over all
// 256-channel column blocks, never fewer than BN_MIN_ROWS rows a part
void row_partition(long M, int C, long* rpb, int* P) {
    const long cb = (C + 255) / 256;
    long maxp = (long)BN_BLOCKS_PER_CU * bn_num_cus() / cb;
    if (maxp < 1) maxp = 1;
    long p = (M + BN_MIN_ROWS - 1) / BN_MIN_ROWS;
    if (p > maxp) p = maxp;
    *rpb = (M + p - 1) / p;
    *P = (int)((M + *rpb - 1) / *rpb);
}

Geo geometry(long M, int C, int vec) {
    Geo q{};
    q.M = M; q.C = C; q.G = C / vec;
    row_partition(M, C, &q.rpb, &q.P);
    int gt = 1;
    while (gt < 64 && gt < q.G) gt <<= 1;                                   // the smallest power of two >= min(G, 64) ...
    for (int d = 64; d >= 8; d >>= 1)                                       // ... or one that divides G and keeps >= 128-byte segments
        if (q.G % d == 0) { gt = d; break; }
    q.gl = 0;
    while ((1 << q.gl) < gt) ++q.gl;
    return q;
}

dim3 grid_of(const Geo& q) { return dim3((unsigned)q.P, (unsigned)((q.G + (1 << q.gl) - 1) >> q.gl)); }

// ---- 16-byte (8-byte: bf16 beside an fp32 operand) accesses ------------------------------------------------------------------------------
template <bool BF, int VEC>
__device__ __forceinline__ uint4 ld_raw(const void* p, long off) {
    if constexpr (BF && VEC == 4) {
        const uint2 t = *(const uint2*)((const __bf16*)p + off);
        return make_uint4(t.x, t.y, 0u, 0u);
    } else if constexpr (BF) {
        return *(const uint4*)((const __bf16*)p + off);
    } else {
        static_assert(VEC == 4, "an fp32 operand is read 4 channels at a time");
        return *(const uint4*)((const float*)p + off);
    }
}

template <bool BF, int VEC>
__device__ __forceinline__ void unpack(const uint4& r, float (&v)[VEC]) {
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
    if constexpr (BF) {
#pragma unroll
        for (int i = 0; i < VEC / 2; ++i) {
            v[2 * i] = __uint_as_float(w[i] << 16);
            v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = __uint_as_float(w[i]);
    }
}

template <bool BF, int VEC>
__device__ __forceinline__ void st_vec(void* p, long off, const float (&v)[VEC]) {
    if constexpr (BF && VEC == 8) {
        U128 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) o.e[i] = f2bf(v[i]);
        *(uint4*)((__bf16*)p + off) = o.u;
    } else if constexpr (BF) {
        U64 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o.e[i] = f2bf(v[i]);
        *(uint2*)((__bf16*)p + off) = o.u;
    } else {
#pragma unroll
        for (int i = 0; i < VEC; i += 4) *(float4*)((float*)p + off + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
    }
}

template <int VEC>
__device__ __forceinline__ void ld_f32(const float* p, float (&v)[VEC]) {
#pragma unroll
    for (int i = 0; i < VEC; i += 4) {
        const float4 t = *(const float4*)(p + i);
        v[i] = t.x; v[i + 1] = t.y; v[i + 2] = t.z; v[i + 3] = t.w;
    }
}

struct Lane {
    int gx, ry, RY, g;
    long r0, r1;
    bool active;
};
__device__ __forceinline__ Lane lane_of(const Geo& q) {
    Lane l;
    const int tid = threadIdx.x;
    l.gx = tid & ((1 << q.gl) - 1);
    l.ry = tid >> q.gl;
    l.RY = BN_THREADS >> q.gl;
    l.g = (blockIdx.y << q.gl) + l.gx;
    l.active = l.g < q.G;
    l.r0 = (long)blockIdx.x * q.rpb;
    l.r1 = l.r0 + q.rpb < q.M ? l.r0 + q.rpb : q.M;
    return l;
}

// acc[0 .. 2*VEC) summed over the thread rows of the workgroup into thread row 0: a pairwise tree in a fixed order
template <int VEC>
__device__ __forceinline__ void tree_sum(float (&a)[VEC], float (&b)[VEC], const Geo& q, const Lane& l) {
    __shared__ float red[16][BN_THREADS];
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < VEC; ++k) { red[k][tid] = a[k]; red[VEC + k][tid] = b[k]; }
    for (int s = l.RY >> 1; s > 0; s >>= 1) {
        __syncthreads();
        if (l.ry < s) {
            const int o = tid + (s << q.gl);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                a[k] += red[k][o]; red[k][tid] = a[k];
                b[k] += red[VEC + k][o]; red[VEC + k][tid] = b[k];
            }
        }
    }
}

template <int VEC>
__device__ __forceinline__ void write_partials(float* ws, const float (&a)[VEC], const float (&b)[VEC], const Geo& q, int col) {
    st_vec<false, VEC>(ws, (long)blockIdx.x * q.C + col, a);
    st_vec<false, VEC>(ws, ((long)q.P + blockIdx.x) * q.C + col, b);
}

// ---- statistics ---------------------------------------------------------------------------------------------------------------------------
template <bool XB>
__global__ __launch_bounds__(BN_THREADS) void bn_stats_kernel(const void* __restrict__ x, long ldx, Geo q, float* __restrict__ ws) {
    constexpr int VEC = XB ? 8 : 4;
    const Lane l = lane_of(q);
    const int col = l.g * VEC;
    float s1[VEC], s2[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) s1[k] = s2[k] = 0.f;
    if (l.active) {
        float K[VEC];
        unpack<XB, VEC>(ld_raw<XB, VEC>(x, col), K);                        // the map's first row: one shift for every part
        auto add = [&](const uint4& raw) {
            float v[VEC];
            unpack<XB, VEC>(raw, v);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float d = v[k] - K[k];
                s1[k] += d;
                s2[k] = fmaf(d, d, s2[k]);
            }
        };
        long r = l.r0 + l.ry;
        const long step = l.RY;
        for (; r + 3 * step < l.r1; r += 4 * step) {
            uint4 raw[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) raw[u] = ld_raw<XB, VEC>(x, (r + u * step) * ldx + col);
#pragma unroll
            for (int u = 0; u < 4; ++u) add(raw[u]);
        }
        for (; r < l.r1; r += step) add(ld_raw<XB, VEC>(x, r * ldx + col));
    }
    tree_sum<VEC>(s1, s2, q, l);
    if (l.active && l.ry == 0) write_partials<VEC>(ws, s1, s2, q, col);
}

// The second level: out_a[c] = sum over parts of ws[p][c], out_b[c] = sum of ws[P + p][c].  256 threads = 16 channels x 16 slices of
// ceil(P / 16) consecutive parts: a slice in ascending order, then a pairwise tree over the slices.  stats != 0: the sums are the
// shifted s1, s2 of csb_stats and the record (mean, M2, count) is written instead.
__global__ __launch_bounds__(BN_THREADS) void bn_combine_kernel(const float* __restrict__ ws, int P, int C, float* __restrict__ out, int stats,
                                                                const void* __restrict__ x, int x_bf16, long M) {
    __shared__ float ra[16][16], rb[16][16];
    const int cl = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    const int per = (P + 15) / 16;
    const int p0 = sl * per, p1 = min(P, p0 + per);
    float a = 0.f, b = 0.f;
    if (c < C) {
#pragma unroll 8                                                            // the loads of eight parts in flight; the additions keep their order
        for (int p = p0; p < p1; ++p) {
            a += ws[(long)p * C + c];
            b += ws[((long)P + p) * C + c];
        }
    }
    ra[sl][cl] = a; rb[sl][cl] = b;
    for (int s = 8; s > 0; s >>= 1) {
        __syncthreads();
        if (sl < s) {
            a += ra[sl + s][cl]; ra[sl][cl] = a;
            b += rb[sl + s][cl]; rb[sl][cl] = b;
        }
    }
    if (sl != 0 || c >= C) return;
    if (!stats) {
        out[c] = a;
        out[C + c] = b;
        return;
    }
    const float K = x_bf16 ? bf2f(((const __bf16*)x)[c]) : ((const float*)x)[c];
    const float q = a / (float)M;
    out[c] = K + q;
    out[C + c] = fmaxf(b - a * q, 0.f);
    if (c == 0) {
        out[2 * C] = __int_as_float((int)M);
        out[2 * C + 1] = out[2 * C + 2] = out[2 * C + 3] = 0.f;
    }
}

// ---- finalize: merge the records, build the state, update the running statistics ----------------------------------------------------------
__global__ __launch_bounds__(BN_THREADS) void bn_finalize_kernel(const float* __restrict__ recs, int R, int C, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float eps, float momentum,
                                                                 float* __restrict__ running_mean, float* __restrict__ running_var,
                                                                 float* __restrict__ st) {
    const int c = blockIdx.x * BN_THREADS + threadIdx.x;
    if (c >= C) return;
    float mean, var, inv_n = 0.f;
    if (recs != nullptr) {
        long long N = 0;
        float M2 = 0.f;
        mean = 0.f;
        const long rl = 2L * C + CSB_REC_EXTRA;
        for (int r = 0; r < R; ++r) {
            const float* rec = recs + r * rl;
            const int cnt = __float_as_int(rec[2 * C]);
            if (cnt <= 0) continue;
            const float mb = rec[c], M2b = rec[C + c];
            if (N == 0) {
                mean = mb; M2 = M2b;
            } else {
                const float na = (float)N, nb = (float)cnt;
                const float w = nb / (float)(N + cnt), d = mb - mean;
                mean = mean + d * w;
                M2 = (M2 + M2b) + d * d * (na * w);
            }
            N += cnt;
        }
        var = N > 0 ? M2 / (float)N : 0.f;
        inv_n = N > 0 ? 1.0f / (float)N : 0.f;
        if (running_mean != nullptr) running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * mean;
        if (running_var != nullptr && N > 1) running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (M2 / (float)(N - 1));
    } else {
        mean = running_mean[c];
        var = running_var[c];
    }
    const float rstd = 1.0f / sqrtf(var + eps);
    const float scale = gamma != nullptr ? gamma[c] * rstd : rstd;
    const float shift = fmaf(-mean, scale, beta != nullptr ? beta[c] : 0.f);
    st[c] = mean;
    st[C + c] = rstd;
    st[2 * C + c] = scale;
    st[3 * C + c] = shift;
    if (c == 0) {
        st[4 * C] = inv_n;
        st[4 * C + 1] = st[4 * C + 2] = st[4 * C + 3] = 0.f;
    }
}

// ---- y = act(fmaf(x, scale, shift)) ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float relu_keep_nan(float v) { return (v > 0.f || v != v) ? v : 0.f; }

template <bool XB, bool YB>
__global__ __launch_bounds__(BN_THREADS) void bn_apply_kernel(const void* __restrict__ x, long ldx, const float* __restrict__ st, int act,
                                                              void* __restrict__ y, long ldy, Geo q) {
    constexpr int VEC = XB ? 8 : 4;
    const Lane l = lane_of(q);
    if (!l.active) return;
    const int col = l.g * VEC;
    float sc[VEC], sh[VEC];
    ld_f32<VEC>(st + 2 * q.C + col, sc);
    ld_f32<VEC>(st + 3 * q.C + col, sh);
    auto put = [&](const uint4& raw, long row) {
        float v[VEC];
        unpack<XB, VEC>(raw, v);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            v[k] = fmaf(v[k], sc[k], sh[k]);
            if (act) v[k] = relu_keep_nan(v[k]);
        }
        st_vec<YB, VEC>(y, row * ldy + col, v);
    };
    long r = l.r0 + l.ry;
    const long step = l.RY;
    for (; r + 3 * step < l.r1; r += 4 * step) {
        uint4 raw[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) raw[u] = ld_raw<XB, VEC>(x, (r + u * step) * ldx + col);
#pragma unroll
        for (int u = 0; u < 4; ++u) put(raw[u], r + u * step);
    }
    for (; r < l.r1; r += step) put(ld_raw<XB, VEC>(x, r * ldx + col), r);
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------------
template <bool DB, bool XB>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_reduce_kernel(const void* __restrict__ dy, long lddy, const void* __restrict__ x, long ldx,
                                                                   const float* __restrict__ st, int act, Geo q, float* __restrict__ ws) {
    constexpr int VEC = (DB && XB) ? 8 : 4;
    const Lane l = lane_of(q);
    const int col = l.g * VEC;
    float sg[VEC], sgx[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) sg[k] = sgx[k] = 0.f;
    if (l.active) {
        float mu[VEC], rs[VEC], sc[VEC], sh[VEC];
        ld_f32<VEC>(st + col, mu);
        ld_f32<VEC>(st + q.C + col, rs);
        ld_f32<VEC>(st + 2 * q.C + col, sc);
        ld_f32<VEC>(st + 3 * q.C + col, sh);
        auto add = [&](const uint4& rd, const uint4& rx) {
            float d[VEC], v[VEC];
            unpack<DB, VEC>(rd, d);
            unpack<XB, VEC>(rx, v);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float g = (!act || fmaf(v[k], sc[k], sh[k]) > 0.f) ? d[k] : 0.f;
                const float xh = (v[k] - mu[k]) * rs[k];
                sg[k] += g;
                sgx[k] = fmaf(g, xh, sgx[k]);
            }
        };
        long r = l.r0 + l.ry;
        const long step = l.RY;
        for (; r + step < l.r1; r += 2 * step) {
            uint4 rd[2], rx[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                rd[u] = ld_raw<DB, VEC>(dy, (r + u * step) * lddy + col);
                rx[u] = ld_raw<XB, VEC>(x, (r + u * step) * ldx + col);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) add(rd[u], rx[u]);
        }
        for (; r < l.r1; r += step) add(ld_raw<DB, VEC>(dy, r * lddy + col), ld_raw<XB, VEC>(x, r * ldx + col));
    }
    tree_sum<VEC>(sg, sgx, q, l);
    if (l.active && l.ry == 0) write_partials<VEC>(ws, sg, sgx, q, col);
}

template <bool DB, bool XB, bool OB>
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_apply_kernel(const void* __restrict__ dy, long lddy, const void* __restrict__ x, long ldx,
                                                                  const float* __restrict__ st, int act, const float* __restrict__ sums,
                                                                  const float* __restrict__ gamma, void* __restrict__ dx, long lddx, Geo q) {
    constexpr int VEC = (DB && XB) ? 8 : 4;
    const Lane l = lane_of(q);
    if (!l.active) return;
    const int col = l.g * VEC;
    float mu[VEC], rs[VEC], sc[VEC], sh[VEC], a[VEC], b[VEC], cc[VEC];
    ld_f32<VEC>(st + col, mu);
    ld_f32<VEC>(st + q.C + col, rs);
    ld_f32<VEC>(st + 2 * q.C + col, sc);
    ld_f32<VEC>(st + 3 * q.C + col, sh);
    const float inv_n = st[4 * q.C];
    if (inv_n != 0.f) {
        ld_f32<VEC>(sums + col, b);
        ld_f32<VEC>(sums + q.C + col, cc);
#pragma unroll
        for (int k = 0; k < VEC; ++k) { b[k] *= inv_n; cc[k] *= inv_n; }
    } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) b[k] = cc[k] = 0.f;
    }
    if (gamma != nullptr) {
        ld_f32<VEC>(gamma + col, a);
#pragma unroll
        for (int k = 0; k < VEC; ++k) a[k] *= rs[k];
    } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) a[k] = rs[k];
    }
    auto put = [&](const uint4& rd, const uint4& rx, long row) {
        float d[VEC], v[VEC];
        unpack<DB, VEC>(rd, d);
        unpack<XB, VEC>(rx, v);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float g = (!act || fmaf(v[k], sc[k], sh[k]) > 0.f) ? d[k] : 0.f;
            const float xh = (v[k] - mu[k]) * rs[k];
            d[k] = a[k] * fmaf(-xh, cc[k], g - b[k]);
        }
        st_vec<OB, VEC>(dx, row * lddx + col, d);
    };
    long r = l.r0 + l.ry;
    const long step = l.RY;
    for (; r + step < l.r1; r += 2 * step) {
        uint4 rd[2], rx[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            rd[u] = ld_raw<DB, VEC>(dy, (r + u * step) * lddy + col);
            rx[u] = ld_raw<XB, VEC>(x, (r + u * step) * ldx + col);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) put(rd[u], rx[u], r + u * step);
    }
    for (; r < l.r1; r += step) put(ld_raw<DB, VEC>(dy, r * lddy + col), ld_raw<XB, VEC>(x, r * ldx + col), r);
}

// ---- argument checks --------------------------------------------------------------------------------------------------------------------------
bool map_ok(const void* p, long ld, int bf16, int C) {
    return p != nullptr && ((uintptr_t)p % 16) == 0 && (bf16 == 0 || bf16 == 1) && ld >= C && ld % (bf16 ? 8 : 4) == 0 && ld < 0x7fffffffL;
}
bool vec_ok(const void* p, bool required) { return p == nullptr ? !required : ((uintptr_t)p % 16) == 0; }

}  // namespace

#define CSB_CHECK_SHAPE(who)                                                                                                    \
    CS_CHECK_ARG(M >= 1 && M <= CSB_MAX_ROWS && C >= 1 && C <= CSB_MAX_C, who ": 1 <= M <= %ld, 1 <= C <= %d (M = %ld, C = %d)", \
                 (long)CSB_MAX_ROWS, (int)CSB_MAX_C, M, C);                                                                      \
    if (C % 8 != 0) return 1
#define CSB_MAP_TEXT ": a map must be 16-byte aligned with a row stride >= C that is a multiple of 8 (bf16) / 4 (fp32) below 2^31, its flag 0 or 1"

extern "C" int csb_row_parts(long M, int C) {
    if (M < 1 || M > CSB_MAX_ROWS || C < 1 || C > CSB_MAX_C || C % 8 != 0) return 0;
    long rpb;
    int P;
    row_partition(M, C, &rpb, &P);
    return P;
}

extern "C" size_t csb_workspace(long M, int C) { return (size_t)csb_row_parts(M, C) * 2 * (size_t)C * sizeof(float); }

extern "C" int csb_stats(const void* x, long ldx, int x_bf16, long M, int C, float* rec, void* ws, hipStream_t stream) {
    CSB_CHECK_SHAPE("csb_stats");
    CS_CHECK_ARG(map_ok(x, ldx, x_bf16, C), "csb_stats" CSB_MAP_TEXT);
    CS_CHECK_ARG(vec_ok(rec, true) && vec_ok(ws, true), "csb_stats: rec and ws must be 16-byte aligned");
    const Geo q = geometry(M, C, x_bf16 ? 8 : 4);
    if (x_bf16) hipLaunchKernelGGL(bn_stats_kernel<true>, grid_of(q), dim3(BN_THREADS), 0, stream, x, ldx, q, (float*)ws);
    else hipLaunchKernelGGL(bn_stats_kernel<false>, grid_of(q), dim3(BN_THREADS), 0, stream, x, ldx, q, (float*)ws);
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_combine_kernel, dim3((unsigned)((C + 15) / 16)), dim3(BN_THREADS), 0, stream, (const float*)ws, q.P, C, rec, 1, x, x_bf16, M);
    CS_LAUNCH_CHECK();
    return 0;
}

extern "C" int csb_finalize(const float* recs, int R, int C, const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                            float* running_var, float* st, hipStream_t stream) {
    CS_CHECK_ARG(C >= 1 && C <= CSB_MAX_C, "csb_finalize: 1 <= C <= %d (C = %d)", (int)CSB_MAX_C, C);
    if (C % 8 != 0) return 1;
    CS_CHECK_ARG(recs == nullptr || (R >= 1 && R <= CSB_MAX_RECORDS), "csb_finalize: 1 <= R <= %d records (R = %d)", (int)CSB_MAX_RECORDS, R);
    CS_CHECK_ARG(eps >= 0.f && momentum == momentum, "csb_finalize: eps >= 0 and a momentum that is a number");
    CS_CHECK_ARG(recs != nullptr || (running_mean != nullptr && running_var != nullptr),
                 "csb_finalize: recs == NULL (evaluation mode) needs running_mean and running_var");
    CS_CHECK_ARG(vec_ok(recs, false) && vec_ok(gamma, false) && vec_ok(beta, false) && vec_ok(running_mean, false) && vec_ok(running_var, false) &&
                     vec_ok(st, true),
                 "csb_finalize: recs, gamma, beta, running_mean, running_var and st must be 16-byte aligned, st not NULL");
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((unsigned)((C + BN_THREADS - 1) / BN_THREADS)), dim3(BN_THREADS), 0, stream, recs, R, C, gamma, beta,
                       eps, momentum, running_mean, running_var, st);
    CS_LAUNCH_CHECK();
    return 0;
}

extern "C" int csb_apply(const void* x, long ldx, int x_bf16, const float* st, int act, void* y, long ldy, int y_bf16, long M, int C,
                         hipStream_t stream) {
    CSB_CHECK_SHAPE("csb_apply");
    CS_CHECK_ARG(map_ok(x, ldx, x_bf16, C) && map_ok(y, ldy, y_bf16, C), "csb_apply" CSB_MAP_TEXT);
    CS_CHECK_ARG(vec_ok(st, true) && (act == 0 || act == 1), "csb_apply: st must be 16-byte aligned, act 0 (none) or 1 (ReLU)");
    const Geo q = geometry(M, C, x_bf16 ? 8 : 4);
    const dim3 grid = grid_of(q), block(BN_THREADS);
#define CSB_APPLY(XB, YB) hipLaunchKernelGGL((bn_apply_kernel<XB, YB>), grid, block, 0, stream, x, ldx, st, act, y, ldy, q)
    if (x_bf16) { if (y_bf16) CSB_APPLY(true, true); else CSB_APPLY(true, false); }
    else { if (y_bf16) CSB_APPLY(false, true); else CSB_APPLY(false, false); }
#undef CSB_APPLY
    CS_LAUNCH_CHECK();
    return 0;
}

extern "C" int csb_bwd_reduce(const void* dy, long lddy, int dy_bf16, const void* x, long ldx, int x_bf16, const float* st, int act, float* sums,
                              void* ws, long M, int C, hipStream_t stream) {
    CSB_CHECK_SHAPE("csb_bwd_reduce");
    CS_CHECK_ARG(map_ok(dy, lddy, dy_bf16, C) && map_ok(x, ldx, x_bf16, C), "csb_bwd_reduce" CSB_MAP_TEXT);
    CS_CHECK_ARG(vec_ok(st, true) && vec_ok(sums, true) && vec_ok(ws, true) && (act == 0 || act == 1),
                 "csb_bwd_reduce: st, sums and ws must be 16-byte aligned, act 0 (none) or 1 (ReLU)");
    const Geo q = geometry(M, C, (dy_bf16 && x_bf16) ? 8 : 4);
    const dim3 grid = grid_of(q), block(BN_THREADS);
#define CSB_RED(DB, XB) hipLaunchKernelGGL((bn_bwd_reduce_kernel<DB, XB>), grid, block, 0, stream, dy, lddy, x, ldx, st, act, q, (float*)ws)
    if (dy_bf16) { if (x_bf16) CSB_RED(true, true); else CSB_RED(true, false); }
    else { if (x_bf16) CSB_RED(false, true); else CSB_RED(false, false); }
#undef CSB_RED
    CS_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_combine_kernel, dim3((unsigned)((C + 15) / 16)), dim3(BN_THREADS), 0, stream, (const float*)ws, q.P, C, sums, 0,
                       (const void*)nullptr, 0, M);
    CS_LAUNCH_CHECK();
    return 0;
}

extern "C" int csb_bwd_apply(const void* dy, long lddy, int dy_bf16, const void* x, long ldx, int x_bf16, const float* st, int act, const float* sums,
                             const float* gamma, void* dx, long lddx, int dx_bf16, long M, int C, hipStream_t stream) {
    CSB_CHECK_SHAPE("csb_bwd_apply");
    CS_CHECK_ARG(map_ok(dy, lddy, dy_bf16, C) && map_ok(x, ldx, x_bf16, C) && map_ok(dx, lddx, dx_bf16, C), "csb_bwd_apply" CSB_MAP_TEXT);
    CS_CHECK_ARG(vec_ok(st, true) && vec_ok(sums, true) && vec_ok(gamma, false) && (act == 0 || act == 1),
                 "csb_bwd_apply: st, sums and gamma must be 16-byte aligned, st and sums not NULL, act 0 (none) or 1 (ReLU)");
    const Geo q = geometry(M, C, (dy_bf16 && x_bf16) ? 8 : 4);
    const dim3 grid = grid_of(q), block(BN_THREADS);
#define CSB_BWD(DB, XB, OB) \
    hipLaunchKernelGGL((bn_bwd_apply_kernel<DB, XB, OB>), grid, block, 0, stream, dy, lddy, x, ldx, st, act, sums, gamma, dx, lddx, q)
    switch ((dy_bf16 << 2) | (x_bf16 << 1) | dx_bf16) {
        case 0: CSB_BWD(false, false, false); break;
        case 1: CSB_BWD(false, false, true); break;
        case 2: CSB_BWD(false, true, false); break;
        case 3: CSB_BWD(false, true, true); break;
        case 4: CSB_BWD(true, false, false); break;
        case 5: CSB_BWD(true, false, true); break;
        case 6: CSB_BWD(true, true, false); break;
        default: CSB_BWD(true, true, true); break;
    }
#undef CSB_BWD
    CS_LAUNCH_CHECK();
    return 0;
}
