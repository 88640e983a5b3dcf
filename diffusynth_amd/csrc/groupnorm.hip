// The GroupNorm kernels (gfx950): statistics, finish and apply over channels-last tensors.
// All of these are HBM-bound: 16-byte vector accesses along the channels-last C axis, fp32 math.
#include <type_traits>

#include "common.hpp"
#include "norm_parts.hpp"

namespace {

// (sum, sum of squares) partials of a producer [B][parts][2] -> gn_ab [B][2]: one block per sample, float64
__global__ void gn_finalize_kernel(const float* part, int parts, double count, float eps, float* ab) {
    __shared__ double r1[256], r2[256];
    const int b = blockIdx.x;
    double a = 0.0, q = 0.0;
    for (int i = threadIdx.x; i < parts; i += blockDim.x) {
        a += (double)part[((size_t)b * parts + i) * 2];
        q += (double)part[((size_t)b * parts + i) * 2 + 1];
    }
    block_tree_sum256(r1, r2, a, q);
    if (threadIdx.x == 0) gn_rstd_pair(r1[0], r2[0], count, eps, ab[2 * b], ab[2 * b + 1]);
}

// direct statistics for (sample, group): one block per (b, g); double accumulation of fp32 partials
template <typename T>
__global__ __launch_bounds__(256) void gn_stats_kernel(const T* x, int HW, int C, int G, float eps, float* ab) {
    __shared__ double r1[256], r2[256];
    const int b = blockIdx.x / G, g = blockIdx.x % G;
    const int cg = C / G;
    const T* xb = x + (size_t)b * HW * C + g * cg;
    double a = 0.0, q = 0.0;
    const long n = (long)HW * cg;
    for (long i = threadIdx.x; i < n; i += blockDim.x) {
        const long pix = i / cg;
        const int c = i - pix * cg;
        const float v = to_f32(xb[pix * C + c]);
        a += v;
        q += (double)v * v;
    }
    block_tree_sum256(r1, r2, a, q);
    if (threadIdx.x == 0) gn_rstd_pair(r1[0], r2[0], (double)n, eps, ab[2 * blockIdx.x], ab[2 * blockIdx.x + 1]);
}

// Streaming statistics for GroupNorm(G, C) over channels-last tensors: the per-(sample, group) kernel above reads a group's
// C/G channels of every pixel as scalars (10-byte pieces of a 160-byte pixel for the VQGAN decoder's last stage: 2.3 TB/s on
// a 1.3 GB tensor).  Here every block streams a contiguous range of one sample's pixels with 16-byte vector loads, each
// thread owning a FIXED channel vector (blockDim is a multiple of the C/V vectors of a pixel) so its partial sums stay in
// registers; per-channel (sum, sumsq) block partials go to a workspace and gn_stats_finish folds channels into groups in
// float64.  No atomics: bit-reproducible.
template <typename T>
__global__ __launch_bounds__(256) void gn_stats_stream_kernel(const T* x, int HW, int C, int pix_per_blk, float* part) {
    constexpr int V = Vec16<T>::N;
    extern __shared__ __attribute__((aligned(16))) char gsm[];
    float* sm = reinterpret_cast<float*>(gsm);                 // [rows][CV][V][2]
    const int CV = C / V, rows = blockDim.x / CV, b = blockIdx.y;
    const int cv = threadIdx.x % CV, row = threadIdx.x / CV;
    const int p0 = blockIdx.x * pix_per_blk, p1 = min(HW, p0 + pix_per_blk);
    float s1[V], s2[V];
#pragma unroll
    for (int v = 0; v < V; ++v) s1[v] = s2[v] = 0.f;
    const T* xb = x + (size_t)b * HW * C + cv * V;
    // four pixels of the thread in flight (one load per iteration left a 240-thread block with 240 x 16 bytes in flight: 1.9 TB/s)
    int pix = p0 + row;
    for (; pix + 3 * rows < p1; pix += 4 * rows) {
        float f[4][V];
#pragma unroll
        for (int k = 0; k < 4; ++k) Vec16<T>::load(xb + (size_t)(pix + k * rows) * C, f[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int v = 0; v < V; ++v) {
                s1[v] += f[k][v];
                s2[v] = fmaf(f[k][v], f[k][v], s2[v]);
            }
    }
    for (; pix < p1; pix += rows) {
        float f[V];
        Vec16<T>::load(xb + (size_t)pix * C, f);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            s1[v] += f[v];
            s2[v] = fmaf(f[v], f[v], s2[v]);
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
        sm[((row * CV + cv) * V + v) * 2] = s1[v];
        sm[((row * CV + cv) * V + v) * 2 + 1] = s2[v];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * 2; i += blockDim.x) {   // i = (channel, which)
        float a = 0.f;
        for (int r = 0; r < rows; ++r) a += sm[r * C * 2 + i];
        part[(((size_t)b * gridDim.x + blockIdx.x) * C) * 2 + i] = a;
    }
}
__global__ void gn_stats_finish_kernel(const float* part, int nblk, int C, int G, double count, float eps, float* ab) {
    // one wave per (sample, group)
    const int b = blockIdx.x / G, g = blockIdx.x % G, cg = C / G, lane = threadIdx.x;
    double a = 0.0, q = 0.0;
    for (int i = lane; i < nblk * cg; i += 64) {
        const int blk = i / cg, c = g * cg + i % cg;
        const float* pp = part + (((size_t)b * nblk + blk) * C + c) * 2;
        a += (double)pp[0];
        q += (double)pp[1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        q += __shfl_xor(q, o, 64);
    }
    if (lane == 0) gn_rstd_pair(a, q, count, eps, ab[2 * blockIdx.x], ab[2 * blockIdx.x + 1]);
}

// One element of the two element-wise apply kernels (generic and lazy): normalise with (a, am) = (rstd, rstd * mean), the channel's affine,
// the activation, then the channel bias of (sample b, channel c) and the residual r (read only where p.res is set).
__device__ __forceinline__ float gn_apply_elem(const ds_gn_apply_params& p, int b, int c, float x, float a, float am, float gm, float bt, const float& r) {
    float y = (x * a - am) * gm + bt;
    y = act_apply(y, p.act);
    if (p.cbias) y += p.cbias[(size_t)b * p.cb_stride + c];
    if (p.res) y += r;
    return y;
}

template <typename T>
__global__ __launch_bounds__(256) void gn_apply_kernel(const ds_gn_apply_params p, size_t nvec) {
    constexpr int V = Vec16<T>::N;
    const int CV = p.C / V, cg = p.C / p.G;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
        const int cv = i % CV;
        const size_t pix = i / CV;
        const int b = pix / p.HW;
        const int c = cv * V;
        float x[V], o[V], r[V];
        vec16_load<T>(reinterpret_cast<const T*>(p.x) + i * V, x, DS_BX_SRC0);
        if (p.res) vec16_load<T>(reinterpret_cast<const T*>(p.res) + i * V, r, DS_BX_RES);
        const float* abp = p.gn_ab + (size_t)b * p.G * 2;
        const float a0 = abp[0], am0 = abp[1];
#pragma unroll
        for (int v = 0; v < V; v += 4) {   // per-channel affine as 16-byte loads (C is a multiple of V, so 16-B aligned)
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(p.gamma + c + v);
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.beta + c + v);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float a = a0, am = am0;
                if (p.G > 1) {
                    const int g = (c + v + q) / cg;
                    a = abp[2 * g];
                    am = abp[2 * g + 1];
                }
                o[v + q] = gn_apply_elem(p, b, c + v + q, x[v + q], a, am, g4[q], b4[q], r[v + q]);
            }
        }
        vec16_store<T>(reinterpret_cast<T*>(p.out) + i * V, o, DS_BX_OUT);
    }
}

// GroupNorm(G, C) apply for G > 1 (the VQGAN's Normalize, VQGAN.py:12-27) with the per-channel (scale, shift) of the block's sample tabulated
// once in LDS and each thread on a FIXED channel vector (blockDim = CV x rows): y = act(x * scale + shift) (+ cbias + res).  The generic kernel
// above divides (c + v) / (C / G) and fetches the group's (rstd, rstd * mean) per ELEMENT behind a runtime activation switch with libm's expf:
// 155 us for the 128 x 64 x 160 tensor of the decoder at batch 64 (2.2 TB/s).
template <typename T, int ACT>
__global__ __launch_bounds__(256) void gn_apply_table_kernel(const ds_gn_apply_params p, int pix_per_blk) {
    constexpr int V = Vec16<T>::N;
    extern __shared__ __attribute__((aligned(16))) float gtab[];       // [C][2]
    const int CV = p.C / V, rows = blockDim.x / CV, b = blockIdx.y, cg = p.C / p.G;
    for (int c = threadIdx.x; c < p.C; c += blockDim.x) {
        const int g = c / cg;
        const float a = p.gn_ab[((size_t)b * p.G + g) * 2], am = p.gn_ab[((size_t)b * p.G + g) * 2 + 1], gm = p.gamma[c];
        gtab[2 * c] = a * gm;
        gtab[2 * c + 1] = p.beta[c] - am * gm + (p.cbias ? p.cbias[(size_t)b * p.cb_stride + c] : 0.f) * (ACT == DS_ACT_NONE ? 1.f : 0.f);
    }
    __syncthreads();
    const int cv = threadIdx.x % CV, row = threadIdx.x / CV;
    float sc[V], sh[V], cb[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        sc[v] = gtab[2 * (cv * V + v)];
        sh[v] = gtab[2 * (cv * V + v) + 1];
        cb[v] = (p.cbias && ACT != DS_ACT_NONE) ? p.cbias[(size_t)b * p.cb_stride + cv * V + v] : 0.f;   // (added AFTER the activation, as above)
    }
    const int p0 = blockIdx.x * pix_per_blk, p1 = min(p.HW, p0 + pix_per_blk);
    const size_t base = (size_t)b * p.HW * p.C + cv * V;
    const T* xb = reinterpret_cast<const T*>(p.x) + base;
    const T* rb = p.res ? reinterpret_cast<const T*>(p.res) + base : nullptr;
    T* ob = reinterpret_cast<T*>(p.out) + base;
    const bool has_res = rb != nullptr;
    auto one = [&](const float (&x)[V], const float (&r)[V], int pix) {
        float o[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float y = fmaf(x[v], sc[v], sh[v]);
            if (ACT == DS_ACT_SILU) y = silu_fast(y);
            else if (ACT == DS_ACT_RELU) y = fmaxf(y, 0.f);
            else if (ACT == DS_ACT_GELU) y = gelu_fast(y);
            y += cb[v];
            if (has_res) y += r[v];
            o[v] = y;
        }
        vec16_store<T>(ob + (size_t)pix * p.C, o, DS_BX_OUT);
    };
    int pix = p0 + row;
    for (; pix + rows < p1; pix += 2 * rows) {                         // two pixels of the thread in flight
        float x0[V], x1[V], r0[V] = {}, r1[V] = {};
        vec16_load<T>(xb + (size_t)pix * p.C, x0, DS_BX_SRC0);
        vec16_load<T>(xb + (size_t)(pix + rows) * p.C, x1, DS_BX_SRC0);
        if (rb) {
            vec16_load<T>(rb + (size_t)pix * p.C, r0, DS_BX_RES);
            vec16_load<T>(rb + (size_t)(pix + rows) * p.C, r1, DS_BX_RES);
        }
        one(x0, r0, pix);
        one(x1, r1, pix + rows);
    }
    if (pix < p1) {
        float x0[V], r0[V] = {};
        vec16_load<T>(xb + (size_t)pix * p.C, x0, DS_BX_SRC0);
        if (rb) vec16_load<T>(rb + (size_t)pix * p.C, r0, DS_BX_RES);
        one(x0, r0, pix);
    }
}

// one sample per blockIdx.y: the block reduces the producer's partials itself (GroupNorm(1, C) only)
template <typename T>
__global__ __launch_bounds__(256) void gn_apply_lazy_kernel(const ds_gn_apply_params p) {
    constexpr int V = Vec16<T>::N;
    const int CV = p.C / V, b = blockIdx.y;
    float a, am;
    gn_from_partials(p.gn_part, p.gn_parts, p.gn_count, p.gn_eps, b, a, am);
    const size_t n = (size_t)p.HW * CV, base = (size_t)b * n;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % CV) * V;
        float x[V], o[V], r[V];
        vec16_load<T>(reinterpret_cast<const T*>(p.x) + (base + i) * V, x, DS_BX_SRC0);
        if (p.res) vec16_load<T>(reinterpret_cast<const T*>(p.res) + (base + i) * V, r, DS_BX_RES);
#pragma unroll
        for (int v = 0; v < V; v += 4) {
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(p.gamma + c + v);
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.beta + c + v);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                o[v + q] = gn_apply_elem(p, b, c + v + q, x[v + q], a, am, g4[q], b4[q], r[v + q]);
            }
        }
        vec16_store<T>(reinterpret_cast<T*>(p.out) + (base + i) * V, o, DS_BX_OUT);
    }
}

// The U-Net's case of the kernel above (bf16, no activation, no channel bias; 96 / 192 / 384 / 768 channels): blocks of 192 threads
// = a whole number of pixels, so a thread keeps ONE channel vector — scale a * gamma and shift beta - a * mean * gamma live in
// registers, no per-element index arithmetic (the generic loop pays a 64-bit modulo and four table loads per 16 bytes) — and
// streams a contiguous pixel range four vectors at a time.  4.3 -> TB/s on 0.4 - 1.2 GB tensors, 16 launches per forward.
template <bool HAS_RES>
__global__ __launch_bounds__(192) void gn_apply_lazy_fast_kernel(const ds_gn_apply_params p, int pix_per_blk) {
    const int CV = p.C >> 3, rows = 192 / CV, b = blockIdx.y;
    const int cv = threadIdx.x % CV, row = threadIdx.x / CV;
    float a, am;
    gn_from_partials(p.gn_part, p.gn_parts, p.gn_count, p.gn_eps, b, a, am);
    float sc[8], sh[8];
#pragma unroll
    for (int v = 0; v < 8; v += 4) {
        const f32x4 g4 = *reinterpret_cast<const f32x4*>(p.gamma + cv * 8 + v);
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.beta + cv * 8 + v);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            sc[v + q] = a * g4[q];
            sh[v + q] = fmaf(-am, g4[q], b4[q]);
        }
    }
    const int p0 = blockIdx.x * pix_per_blk, p1 = min(p.HW, p0 + pix_per_blk);
    const size_t sbase = (size_t)b * p.HW * p.C + cv * 8;
    const bf16* xb = reinterpret_cast<const bf16*>(p.x) + sbase;
    const bf16* rb = reinterpret_cast<const bf16*>(p.res) + sbase;
    bf16* ob = reinterpret_cast<bf16*>(p.out) + sbase;
    constexpr int U = 4;
    for (int pix = p0 + row; pix < p1; pix += rows * U) {
        u32x4 xv[U], rv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = pix + u * rows;
            const int qc = q < p1 ? q : pix;                   // unconditional loads (clamped), predicated stores
            xv[u] = DS_LD(u32x4, xb + (size_t)qc * p.C, DS_BX_SRC0);
            if constexpr (HAS_RES) rv[u] = DS_LD(u32x4, rb + (size_t)qc * p.C, DS_BX_RES);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = pix + u * rows;
            float o[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float lo = __uint_as_float(xv[u][e] << 16), hi = __uint_as_float(xv[u][e] & 0xffff0000u);
                lo = fmaf(lo, sc[2 * e], sh[2 * e]);
                hi = fmaf(hi, sc[2 * e + 1], sh[2 * e + 1]);
                if constexpr (HAS_RES) {
                    lo += __uint_as_float(rv[u][e] << 16);
                    hi += __uint_as_float(rv[u][e] & 0xffff0000u);
                }
                o[2 * e] = lo;
                o[2 * e + 1] = hi;
            }
            if (q < p1) vec16_store<bf16>(ob + (size_t)q * p.C, o, DS_BX_OUT);
        }
    }
}

}  // namespace

extern "C" int ds_gn_finalize(const float* part, int B, int parts, double count, float eps, float* ab, void* stream) {
    DS_REQUIRE(part && ab && B > 0 && parts > 0 && count > 0, "gn_finalize: bad args");
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), part, parts, count, eps, ab);
    DS_CHECK_LAUNCH("gn_finalize");
    return DS_OK;
}

extern "C" int ds_gn_stats(const void* x, int dtype, int B, int HW, int C, int G, float eps, float* ab, void* stream) {
    DS_REQUIRE(x && ab && B > 0 && HW > 0 && C > 0 && G > 0 && C % G == 0, "gn_stats: bad args");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == DS_BF16) hipLaunchKernelGGL(gn_stats_kernel<bf16>, dim3(B * G), dim3(256), 0, st, (const bf16*)x, HW, C, G, eps, ab);
    else if (dtype == DS_F32) hipLaunchKernelGGL(gn_stats_kernel<float>, dim3(B * G), dim3(256), 0, st, (const float*)x, HW, C, G, eps, ab);
    else DS_FAIL(DS_EINVAL, "gn_stats: dtype %d", dtype);
    DS_CHECK_LAUNCH("gn_stats");
    return DS_OK;
}

// blocks per sample of the streaming statistics pass (a function of the shape only)
static int gn_stream_blocks(int HW) {
    int n = (HW + 511) / 512;                    // >= 512 pixels per block (r04: 2048 left a 128 x 64 x 160 tensor at batch 64 with one block per CU)
    return n < 1 ? 1 : (n > 256 ? 256 : n);
}
extern "C" size_t ds_gn_stats_ws_floats(int B, int HW, int C) { return (size_t)B * gn_stream_blocks(HW) * C * 2; }

static int gn_stats_finish_launch(const float* ws, int B, int nblk, int C, int G, int HW, float eps, float* ab, hipStream_t st) {
    hipLaunchKernelGGL(gn_stats_finish_kernel, dim3(B * G), dim3(64), 0, st, ws, nblk, C, G, (double)HW * (C / G), eps, ab);
    DS_CHECK_LAUNCH("gn_stats_finish");
    return DS_OK;
}

extern "C" int ds_gn_stats_stream(const void* x, int dtype, int B, int HW, int C, int G, float eps, float* ws, float* ab, void* stream) {
    DS_REQUIRE(x && ab && ws && B > 0 && HW > 0 && C > 0 && G > 0 && C % G == 0, "gn_stats_stream: bad args");
    DS_REQUIRE(dtype == DS_F32 || dtype == DS_BF16, "gn_stats_stream: dtype %d", dtype);
    const int V = dtype == DS_BF16 ? 8 : 4, CV = C / V;
    DS_REQUIRE(C % V == 0 && CV <= 256 && ds_aligned16(x), "gn_stats_stream: C=%d must be a multiple of %d (at most %d) and x 16-byte aligned", C, V, 256 * V);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int nblk = gn_stream_blocks(HW), ppb = (HW + nblk - 1) / nblk, threads = CV * (256 / CV);
    const size_t lds = (size_t)(threads / CV) * C * 2 * sizeof(float);
    if (dtype == DS_BF16) hipLaunchKernelGGL(gn_stats_stream_kernel<bf16>, dim3(nblk, B), dim3(threads), lds, st, (const bf16*)x, HW, C, ppb, ws);
    else hipLaunchKernelGGL(gn_stats_stream_kernel<float>, dim3(nblk, B), dim3(threads), lds, st, (const float*)x, HW, C, ppb, ws);
    DS_CHECK_LAUNCH("gn_stats_stream");
    return gn_stats_finish_launch(ws, B, nblk, C, G, HW, eps, ab, st);
}

extern "C" int ds_gn_stats_finish(const float* ws, int B, int nblk, int C, int G, int HW, float eps, float* ab, void* stream) {
    DS_REQUIRE(ws && ab && B > 0 && nblk > 0 && C > 0 && G > 0 && C % G == 0 && HW > 0, "gn_stats_finish: bad args");
    return gn_stats_finish_launch(ws, B, nblk, C, G, HW, eps, ab, reinterpret_cast<hipStream_t>(stream));
}

// Which kernel ds_gn_apply launches for p (dtype, C and G already checked; V = elements per 16 bytes).
enum GnApplyPath { GN_LAZY_FAST, GN_LAZY, GN_TABLE, GN_GENERIC };
static GnApplyPath gn_apply_path(const ds_gn_apply_params* p, int V) {
    if (p->gn_part && p->dtype == DS_BF16 && p->act == DS_ACT_NONE && !p->cbias && 192 % (p->C / 8) == 0) return GN_LAZY_FAST;
    if (p->gn_part) return GN_LAZY;
    // (every tier, every G since r04: the per-channel (scale, shift) table kernel — its SiLU is exp2f + v_rcp_f32, ~1 ulp each, where the
    // element-wise generic kernel uses libm's expf and a true divide: the fp32 tier's bits differ from r03's by that much)
    if (p->gn_ab && p->C / V <= 256 && p->C * 8 <= 48 * 1024) return GN_TABLE;
    return GN_GENERIC;
}

// blocks per sample of a launch of (bx, B) blocks: `want`, as long as the whole grid stays within `cap` blocks
static int gn_capped_grid(long long want, int B, int cap) {
    const int per = cap / B > 0 ? cap / B : 1;
    return want > per ? per : (int)want;
}

// f(T{}, act<ACT>) for the dtype and the activation of p: the template arguments of the kernel to launch
template <typename F> static void gn_dispatch(const ds_gn_apply_params* p, F f) {
    auto by_act = [&](auto t) {
        if (p->act == DS_ACT_SILU) f(t, std::integral_constant<int, DS_ACT_SILU>{});
        else if (p->act == DS_ACT_RELU) f(t, std::integral_constant<int, DS_ACT_RELU>{});
        else if (p->act == DS_ACT_GELU) f(t, std::integral_constant<int, DS_ACT_GELU>{});
        else f(t, std::integral_constant<int, DS_ACT_NONE>{});
    };
    if (p->dtype == DS_BF16) by_act(bf16{});
    else by_act(float{});
}

extern "C" int ds_gn_apply(const ds_gn_apply_params* p, void* stream) {
    DS_REQUIRE(p && p->x && p->out && (p->gn_ab || p->gn_part) && p->gamma && p->beta, "gn_apply: null pointer");
    DS_REQUIRE(!p->gn_part || (p->G == 1 && !p->gn_ab && p->gn_parts > 0 && p->gn_count > 0), "gn_apply: partials need G == 1 and no gn_ab");
    DS_REQUIRE(p->dtype == DS_F32 || p->dtype == DS_BF16, "gn_apply: dtype %d", p->dtype);
    const int V = p->dtype == DS_BF16 ? 8 : 4, CV = p->C / V;
    DS_REQUIRE(p->C % V == 0 && p->G > 0 && p->C % p->G == 0, "gn_apply: C=%d must be a multiple of %d and of G=%d", p->C, V, p->G);
    if (!ds_aligned16(p->x) || !ds_aligned16(p->out) || (p->res && !ds_aligned16(p->res)))
        DS_FAIL(DS_EALIGN, "gn_apply: pointers must be 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#if DS_BOUNDS
    {
        const long long es = V == 8 ? 2 : 4, n = (long long)p->B * p->HW * p->C * es;
        DsBxHost h(DS_K_GN_APPLY);
        h.set(DS_BX_SRC0, p->x, n).set(DS_BX_RES, p->res, n).set(DS_BX_OUT, p->out, n);
        h.set(DS_BX_GNPART, p->gn_part, (long long)p->B * p->gn_parts * 2 * 4);
        h.publish(st);
    }
#endif
    switch (gn_apply_path(p, V)) {
        case GN_LAZY_FAST: {
            const int rows = 192 / CV;                                           // four pixels of a thread per trip
            const int bx = gn_capped_grid((p->HW + rows * 4 - 1) / (rows * 4), p->B, 4096), ppb = (p->HW + bx - 1) / bx;
            if (p->res) hipLaunchKernelGGL(gn_apply_lazy_fast_kernel<true>, dim3(bx, p->B), dim3(192), 0, st, *p, ppb);
            else hipLaunchKernelGGL(gn_apply_lazy_fast_kernel<false>, dim3(bx, p->B), dim3(192), 0, st, *p, ppb);
            DS_CHECK_LAUNCH("gn_apply_lazy_fast");
            break;
        }
        case GN_LAZY: {
            const int bx = gn_capped_grid(((long long)p->HW * CV + 255) / 256, p->B, 2048);
            if (p->dtype == DS_BF16) hipLaunchKernelGGL(gn_apply_lazy_kernel<bf16>, dim3(bx, p->B), dim3(256), 0, st, *p);
            else hipLaunchKernelGGL(gn_apply_lazy_kernel<float>, dim3(bx, p->B), dim3(256), 0, st, *p);
            DS_CHECK_LAUNCH("gn_apply_lazy");
            break;
        }
        case GN_TABLE: {
            const int threads = CV * (256 / CV), rows = threads / CV;
            const int bx = gn_capped_grid((p->HW + rows * 8 - 1) / (rows * 8), p->B, 8192), ppb = (p->HW + bx - 1) / bx;      // >= 8 pixels per thread
            const size_t lds = (size_t)p->C * 2 * sizeof(float);
            gn_dispatch(p, [&](auto t, auto act) {
                hipLaunchKernelGGL((gn_apply_table_kernel<decltype(t), decltype(act)::value>), dim3(bx, p->B), dim3(threads), lds, st, *p, ppb);
            });
            DS_CHECK_LAUNCH("gn_apply_table");
            break;
        }
        case GN_GENERIC: {
            const size_t nvec = (size_t)p->B * p->HW * CV;
            const int blocks = (int)((nvec + 255) / 256 < 8192 ? (nvec + 255) / 256 : 8192);
            if (p->dtype == DS_BF16) hipLaunchKernelGGL(gn_apply_kernel<bf16>, dim3(blocks), dim3(256), 0, st, *p, nvec);
            else hipLaunchKernelGGL(gn_apply_kernel<float>, dim3(blocks), dim3(256), 0, st, *p, nvec);
            DS_CHECK_LAUNCH("gn_apply");
            break;
        }
    }
    return DS_OK;
}

#if DS_BOUNDS
extern "C" int ds_bounds_fetch_groupnorm(ds_bounds_rec* out, int reset) { return ds_bounds_fetch_tu(out, reset); }
#endif
