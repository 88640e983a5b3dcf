// Small kernels around the U-Net: conditioning MLPs, boundary layout converts, the fused sampler
// step, Philox noise and the "repeat" noise column gather (gfx950).
#include <stdarg.h>

#include "common.hpp"

// ------------------------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
void ds_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* ds_last_error_string(void) { return g_err; }
extern "C" int ds_abi_version(void) { return 1; }

// fp32 NHWC [npix][C] -> two bf16 planes per pixel [npix][2C] (hi = bf16(x), then lo = bf16(x - hi)): the DS_CONV_F_SPLIT_IN input format
// of the split-precision convolutions, for tensors whose producer is an fp32 kernel
namespace {
__global__ __launch_bounds__(256) void split_planes_kernel(const float* x, bf16* out, size_t nvec, int CV) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
        const size_t pix = i / CV;
        const int cv = (int)(i - pix * CV);
        const f32x4 a = *reinterpret_cast<const f32x4*>(x + i * 8), c = *reinterpret_cast<const f32x4*>(x + i * 8 + 4);
        const float v8[8] = {a[0], a[1], a[2], a[3], c[0], c[1], c[2], c[3]};
        u32x4 hi, lo;
        ds_split8(v8, hi, lo);
        bf16* o = out + (pix * 2 * CV + cv) * 8;
        *reinterpret_cast<u32x4*>(o) = hi;
        *reinterpret_cast<u32x4*>(o + (size_t)CV * 8) = lo;
    }
}
}  // namespace
extern "C" int ds_split_planes(const float* x, void* out, long long npix, int C, void* stream) {
    DS_REQUIRE(x && out && npix > 0 && C > 0 && C % 8 == 0 && ds_aligned16(x) && ds_aligned16(out), "split_planes: C %% 8 == 0, 16-byte aligned pointers");
    const size_t nvec = (size_t)npix * (C / 8);
    const int blocks = (int)((nvec + 255) / 256 < 16384 ? (nvec + 255) / 256 : 16384);
    hipLaunchKernelGGL(split_planes_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, reinterpret_cast<bf16*>(out), nvec, C / 8);
    DS_CHECK_LAUNCH("split_planes");
    return DS_OK;
}

// ---- bounds diagnostics (see common.hpp).  Product build: reports "not a bounds build" (-1).
#if DS_BOUNDS
extern "C" int ds_bounds_fetch_conv_igemm(ds_bounds_rec*, int);
extern "C" int ds_bounds_fetch_conv_splitk(ds_bounds_rec*, int);
extern "C" int ds_bounds_fetch_conv_halo3(ds_bounds_rec*, int);
extern "C" int ds_bounds_fetch_conv_quad(ds_bounds_rec*, int);
extern "C" int ds_bounds_fetch_conv_smalln(ds_bounds_rec*, int);
extern "C" int ds_bounds_fetch_dwconv_gn(ds_bounds_rec*, int);
extern "C" int ds_bounds_fetch_attn_fused(ds_bounds_rec*, int);
extern "C" int ds_bounds_fetch_attn_x3(ds_bounds_rec*, int);
extern "C" int ds_bounds_fetch_linattn(ds_bounds_rec*, int);
extern "C" int ds_bounds_fetch_conv1x1_x3(ds_bounds_rec*, int);
extern "C" int ds_bounds_fetch_conv7x7_c4(ds_bounds_rec*, int);
extern "C" int ds_bounds_fetch_convt4x4_c80(ds_bounds_rec*, int);
extern "C" int ds_bounds_fetch_conv3x3_c80(ds_bounds_rec*, int);
extern "C" int ds_bounds_fetch_conv3x3_f32_n4(ds_bounds_rec*, int);
extern "C" int ds_bounds_fetch_vq_attn(ds_bounds_rec*, int);
extern "C" int ds_bounds_fetch_ui_images(ds_bounds_rec*, int);
extern "C" int ds_bounds_fetch_arranger(ds_bounds_rec*, int);
#endif
extern "C" int ds_bounds_report(char* buf, int n, int reset) {
#if DS_BOUNDS
    static const char* knames[] = {"?", "conv_igemm", "conv3x3_halo", "splitk_reduce", "dwconv7_mfma", "dwconv7_lds", "dwconv7",
                                   "attn_fused_ctx", "attn_fused_out", "gn_apply", "linattn", "conv7x7_c4", "convt4x4_c80", "conv3x3_c80", "conv3x3_f32_n4", "vq_attn_ctx", "vq_attn_apply",
                                   "stft_images", "latent_image", "pv_stft", "pv_vocode", "pv_istft", "resample_sinc", "peak_normalize", "mix_notes"};
    static const char* bnames[] = {"src0", "src1", "weights", "out", "res", "bias", "fold_t1", "fold_t2", "gn_ab", "gn_part", "stats_part",
                                   "aux0", "aux1", "aux2", "aux3"};
    int (*fetch[])(ds_bounds_rec*, int) = {ds_bounds_fetch_conv_igemm, ds_bounds_fetch_conv_splitk, ds_bounds_fetch_conv_halo3, ds_bounds_fetch_conv_quad, ds_bounds_fetch_conv_smalln, ds_bounds_fetch_dwconv_gn,
                                           ds_bounds_fetch_attn_fused, ds_bounds_fetch_attn_x3, ds_bounds_fetch_linattn, ds_bounds_fetch_conv1x1_x3, ds_bounds_fetch_conv7x7_c4, ds_bounds_fetch_convt4x4_c80, ds_bounds_fetch_conv3x3_c80, ds_bounds_fetch_conv3x3_f32_n4, ds_bounds_fetch_vq_attn,
                                           ds_bounds_fetch_ui_images, ds_bounds_fetch_arranger};
    int hits = 0, pos = 0;
    if (buf && n > 0) buf[0] = 0;
    for (auto f : fetch) {
        ds_bounds_rec r;
        if (f(&r, reset) != 0) return -2;
        if (r.hit) {
            ++hits;
            if (buf && pos < n)
                pos += snprintf(buf + pos, n - pos, "%s: %s access of %d bytes at offset %lld outside extent %lld (block %d,%d,%d thread %d); ",
                                knames[r.kernel > 0 && r.kernel < (int)(sizeof(knames) / sizeof(knames[0])) ? r.kernel : 0], bnames[r.buf < DS_BX_N ? r.buf : 0], r.size, r.off, r.extent, r.bx, r.by,
                                r.bz, r.tid);
        }
    }
    return hits;
#else
    if (buf && n > 0) snprintf(buf, n, "not a bounds build (compile with -DDS_BOUNDS=1: tools/build_variants.py bounds)");
    (void)reset;
    return -1;
#endif
}

namespace {

// ------------------------------------------------------------------------------------------------ conditioning
__global__ void sinusoid_kernel(const int64_t* t, const float* freqs, int B, int half, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * half) return;
    const int b = i / half, j = i % half;
    const float arg = (float)t[b] * freqs[j];
    out[(size_t)b * 2 * half + j] = sinf(arg);
    out[(size_t)b * 2 * half + half + j] = cosf(arg);
}

// one wave per output element: y[b][o] = bias[o] + sum_k act(x[b][k]) W[o][k]
__global__ __launch_bounds__(256) void linear_kernel(const float* x, int xs, const float* W, const float* bias, int B, int K,
                                                     int O, int act_in, float* y, int ys) {
    const long wid = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (wid >= (long)B * O) return;
    const int b = wid / O, o = wid % O;
    const float* xr = x + (size_t)b * xs;
    const float* wr = W + (size_t)o * K;
    float acc = 0.f;
    for (int k = lane; k < K; k += 64) acc = fmaf(act_apply(xr[k], act_in), wr[k], acc);
    acc = wave_sum(acc);
    if (lane == 0) y[(size_t)b * ys + o] = acc + (bias ? bias[o] : 0.f);
}

// fp32 MFMA form of the same GEMV stack (16x16x4: exact fp32 fma chains): wave = 16 outputs x NBT tiles of 16 samples.
// A lane loads 16 bytes of its x row and of its W row per 16-deep K step and feeds element s of both to MFMA s, so the k
// assignment (k0 + 4*(lane>>4) + s) agrees between the operands and W stays in nn.Linear's row-major [O][K] layout.
// No cross-lane reduction, every W element is read once per 16 samples: the stacked time-bias GEMV (O ~ 8k) drops from
// ~50 us to a few us and no longer grows with the batch.
template <int NBT>
__global__ __launch_bounds__(256) void linear_mfma_kernel(const float* x, int xs, const float* W, const float* bias, int B, int K, int O,
                                                          int act_in, float* y, int ys) {
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    const int o0 = wave * 16;
    if (o0 >= O) return;                                   // wave-uniform
    const int n = lane & 15, kq = lane >> 4;
    const float* wr = W + (size_t)min(o0 + n, O - 1) * K + 4 * kq;
    const int nbt = (B + 15) / 16;
    for (int bt0 = 0; bt0 < nbt; bt0 += NBT) {
        const float* xr[NBT];
        f32x4 acc[NBT];
#pragma unroll
        for (int t = 0; t < NBT; ++t) {
            xr[t] = x + (size_t)min((bt0 + t) * 16 + n, B - 1) * xs + 4 * kq;
            acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll 6
        for (int k0 = 0; k0 < K; k0 += 16) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + k0);
#pragma unroll
            for (int t = 0; t < NBT; ++t) {
                f32x4 xv = *reinterpret_cast<const f32x4*>(xr[t] + k0);
                if (act_in != DS_ACT_NONE) {
#pragma unroll
                    for (int s4 = 0; s4 < 4; ++s4) xv[s4] = act_apply(xv[s4], act_in);
                }
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s4], wv[s4], acc[t], 0, 0, 0);
            }
        }
        const int o = o0 + n;
        const float bo = (bias && o < O) ? bias[o] : 0.f;
#pragma unroll
        for (int t = 0; t < NBT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int b = (bt0 + t) * 16 + kq * 4 + r;
                if (b < B && o < O) y[(size_t)b * ys + o] = acc[t][r] + bo;
            }
    }
}

// ------------------------------------------------------------------------------------------------ layouts
template <typename T>
__global__ void nchw_to_nhwc_kernel(const float* x, int C, int HW, T* out, int Cp, size_t total) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = i % Cp;
        const size_t bp = i / Cp;
        const size_t b = bp / HW, pix = bp % HW;
        out[i] = from_f32<T>(c < C ? x[(b * C + c) * HW + pix] : 0.f);
    }
}
template <typename T>
__global__ void nhwc_to_nchw_kernel(const T* x, int C, int Cs, int HW, float* out, size_t total) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t pix = i % HW;
        const size_t bc = i / HW;
        const size_t b = bc / C, c = bc % C;
        out[i] = to_f32(x[(b * HW + pix) * Cs + c]);
    }
}

// ------------------------------------------------------------------------------------------------ sampler step
// Every operation below is a separately rounded IEEE fp32 op in the reference's order
// (DiffSynthSampler.py:320,327,337,343,291-293,506): contraction into FMA is switched off.  ddim_step_kernel and step_rows_kernel both
// call step_element, so a row of ds_step_rows is the same bits as ds_ddim_step given the same inputs.
#pragma clang fp contract(off)
// cf: sqrt(1-a_t), sqrt(a_t), sqrt(a_prev), sqrt(1-a_prev-sigma^2), sigma; qc: sqrt(acp[t-1]), sqrt(1-acp[t-1]) (blend mode 1 only);
// m / g / n0: mask, guide and initial noise of the element (blend modes 1 / 2 only)
__device__ __forceinline__ float guided_eps(float eps, bool cfg, float eps_c, float cfg_scale) {
    if (cfg) {
        const float d = eps_c - eps;
        const float sd = cfg_scale * d;
        eps = eps + sd;
    }
    return eps;
}
__device__ __forceinline__ float predicted_x0(float x, float eps, float sigma_t, float alpha_t) {
    const float t0 = sigma_t * eps;
    const float t1 = x - t0;
    return t1 / alpha_t;
}
__device__ __forceinline__ float inpaint_blend(float v, int blend_mode, float m, float g, float n0, float q0, float q1) {
    if (blend_mode) {
        if (blend_mode == 1) {
            const float g0 = q0 * g;
            const float g1 = q1 * n0;
            g = g0 + g1;
        }
        const float w0 = m * g;
        const float w1 = (1.0f - m) * v;
        v = w0 + w1;
    }
    return v;
}
__device__ __forceinline__ float step_element(float x, float eps, bool cfg, float eps_c, float cfg_scale, const float (&cf)[5], float noise,
                                              int blend_mode, float m, float g, float n0, float q0, float q1) {
    eps = guided_eps(eps, cfg, eps_c, cfg_scale);
    const float x0 = predicted_x0(x, eps, cf[0], cf[1]);
    const float u0 = cf[2] * x0;
    const float u1 = cf[3] * eps;
    const float u2 = cf[4] * noise;
    return inpaint_blend((u0 + u1) + u2, blend_mode, m, g, n0, q0, q1);
}
// "dpmpp_2m" (DPM-Solver++(2M)): cf = sigma_t, alpha_t, c_x, c_0, c_1 (sampler.py: _solver_coefficients); x0 is step_element's.  `hist` is the
// previous step's x0 (used only where second, i.e. c_1 != 0) and receives this step's: the blend changes the state, never the history
__device__ __forceinline__ float dpm_element(float x, float eps, bool cfg, float eps_c, float cfg_scale, const float (&cf)[5], bool second,
                                             float& hist, int blend_mode, float m, float g, float n0, float q0, float q1) {
    eps = guided_eps(eps, cfg, eps_c, cfg_scale);
    const float x0 = predicted_x0(x, eps, cf[0], cf[1]);
    const float u0 = cf[2] * x;
    const float u1 = cf[3] * x0;
    float v = u0 + u1;
    if (second) {
        const float u2 = cf[4] * hist;
        v = v + u2;
    }
    hist = x0;
    return inpaint_blend(v, blend_mode, m, g, n0, q0, q1);
}

__global__ __launch_bounds__(256) void ddim_step_kernel(const ds_step_params p, size_t total) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int b = i / p.CHW;
        const float cf[5] = {p.coef[(size_t)b * 5], p.coef[(size_t)b * 5 + 1], p.coef[(size_t)b * 5 + 2], p.coef[(size_t)b * 5 + 3],
                             p.coef[(size_t)b * 5 + 4]};
        float m = 0.f, g = 0.f, n0 = 0.f, q0 = 0.f, q1 = 0.f;
        if (p.blend_mode) {
            const size_t r = i - (size_t)b * p.CHW;
            m = p.mask_chw ? p.mask[i] : p.mask[(size_t)b * p.HW + r % p.HW];
            g = p.guide[i];
            if (p.blend_mode == 1) {
                q0 = p.qcoef[(size_t)b * 2];
                q1 = p.qcoef[(size_t)b * 2 + 1];
                n0 = p.init_noise[i];
            }
        }
        p.out[i] = step_element(p.x[i], p.eps[i], p.eps_cond != nullptr, p.eps_cond ? p.eps_cond[i] : 0.f, p.cfg_scale, cf, p.noise[i],
                                p.blend_mode, m, g, n0, q0, q1);
    }
}
#pragma clang fp contract(fast)

// ------------------------------------------------------------------------------------------------ Philox4x32-10
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
}
// Philox4x32-10 block of counter `ctr` under key `seed`, Box-Muller'd into four N(0,1) lanes; pair h (lanes 2h, 2h+1) only needs
// words 2h, 2h+1 of the block, so a caller that wants one lane computes one pair (same bits as the four-lane form)
__device__ __forceinline__ void philox_block(uint64_t seed, uint64_t ctr, uint32_t (&c)[4]) {
    c[0] = (uint32_t)ctr; c[1] = (uint32_t)(ctr >> 32); c[2] = 0u; c[3] = 0u;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
    const float u1 = ((float)(a >> 8) + 0.5f) * (1.0f / 16777216.0f);      // (0,1)
    const float u2 = ((float)(b >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * logf(u1));
    float s, cs;
    sincospif(2.0f * u2, &s, &cs);
    z0 = r * cs;
    z1 = r * s;
}
// element e of the stream (seed, offset): lane e % 4 of counter offset + e / 4 — what ds_philox_normal writes at out[e]
__device__ __forceinline__ float philox_normal_at(uint64_t seed, uint64_t offset, uint64_t e) {
    uint32_t c[4];
    philox_block(seed, offset + e / 4, c);
    const int lane = (int)(e & 3), h = lane >> 1;
    float z0, z1;
    box_muller(c[2 * h], c[2 * h + 1], z0, z1);
    return (lane & 1) ? z1 : z0;
}

__global__ void philox_normal_kernel(float* out, size_t n, uint64_t seed, uint64_t offset) {
    const size_t nq = (n + 3) / 4;
    for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < nq; q += (size_t)gridDim.x * blockDim.x) {
        uint32_t c[4];
        philox_block(seed, offset + q, c);
        float z[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) box_muller(c[2 * h], c[2 * h + 1], z[2 * h], z[2 * h + 1]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q * 4 + j < n) out[q * 4 + j] = z[j];
    }
}

// ------------------------------------------------------------------------------------------------ step over rows of many requests
template <int V>
__device__ __forceinline__ void load_v(const float* p, bool vec, float (&v)[V]) {
    if constexpr (V == 4) {
        if (vec) {
            const float4 t = *reinterpret_cast<const float4*>(p);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = p[k];
}
template <int V>
__device__ __forceinline__ void store_v(float* p, const float (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else p[0] = v[0];
}

#pragma clang fp contract(off)
// grid (x: pieces of V elements of one row, y: row).  V == 4 only when W % 4 == 0 and x / eps / out are 16-byte aligned: a piece then
// never crosses an image row, and the row's own guide / initial noise / mask are read in 16-byte pieces when their addresses allow it.
template <int V>
__global__ __launch_bounds__(256) void step_rows_kernel(const ds_step_rows_params p) {
    const int r = blockIdx.y;
    const int32_t* ir = p.irow + (size_t)r * DS_SR_NI;
    const float* fr = p.frow + (size_t)r * DS_SR_NF;
    const uint64_t* pr = p.prow + (size_t)r * DS_SR_NP;
    const int xr = ir[DS_SR_X], er = ir[DS_SR_EPS], ecr = ir[DS_SR_EPSC], orow = ir[DS_SR_OUT], dup = ir[DS_SR_DUP];
    const int blend = ir[DS_SR_BLEND], mchw = ir[DS_SR_MASK_CHW], nmode = ir[DS_SR_NOISE];
    const int smp = ir[DS_SR_SAMPLE], drows = ir[DS_SR_DRAW_ROWS], dw = ir[DS_SR_DRAW_W], coff = ir[DS_SR_COLS];
    const float* guide = reinterpret_cast<const float*>(pr[DS_SR_GUIDE]);
    const float* init = reinterpret_cast<const float*>(pr[DS_SR_INIT]);
    const float* mask = reinterpret_cast<const float*>(pr[DS_SR_MASKP]);
    const float* draw = reinterpret_cast<const float*>(pr[DS_SR_DRAW]);
    // the table is the host's.  A row that points outside the declared bounds is never read out of bounds: its output row (and its
    // duplicate, when that one is in range) is filled with NaN so that a malformed table shows in the result, and a row whose output
    // row itself is out of range writes nothing
    const int HW = p.H * p.W;
    const size_t CHW = (size_t)p.C * HW;
    if (orow < 0 || orow >= p.Bout) return;
    const bool bad = xr < 0 || xr >= p.Bx || er < 0 || er >= p.Beps || ecr >= p.Beps || dup >= p.Bout || blend < 0 || blend > 2 ||
                     nmode < 0 || nmode > 2 || (blend && (!guide || !mask || (blend == 1 && !init))) ||
                     (nmode && (smp < 0 || smp >= drows || dw <= 0 || coff < 0 || coff > p.n_cols - p.W || (nmode == 1 && !draw)));
    if (bad) {
        const float nan = __builtin_nanf("");
        for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < CHW; i += (size_t)gridDim.x * blockDim.x) {
            p.out[(size_t)orow * CHW + i] = nan;
            if (dup >= 0 && dup < p.Bout) p.out[(size_t)dup * CHW + i] = nan;
        }
        return;
    }
    const float cf[5] = {fr[DS_SR_COEF], fr[DS_SR_COEF + 1], fr[DS_SR_COEF + 2], fr[DS_SR_COEF + 3], fr[DS_SR_COEF + 4]};
    const float q0 = fr[DS_SR_Q0], q1 = fr[DS_SR_Q1], scale = fr[DS_SR_CFG];
    const uint64_t seed = pr[DS_SR_SEED], offset = pr[DS_SR_OFFSET];
    const bool avec = V == 4 && ((((uint64_t)guide | (uint64_t)init | (uint64_t)mask) & 15) == 0);
    const float* xrow = p.x + (size_t)xr * CHW;
    const float* erow = p.eps + (size_t)er * CHW;
    const float* ecrow = ecr >= 0 ? p.eps + (size_t)ecr * CHW : nullptr;
    float* orow_p = p.out + (size_t)orow * CHW;
    float* drow_p = dup >= 0 ? p.out + (size_t)dup * CHW : nullptr;
    const size_t nv = CHW / V;
    for (size_t v = blockIdx.x * (size_t)blockDim.x + threadIdx.x; v < nv; v += (size_t)gridDim.x * blockDim.x) {
        const size_t i0 = v * V;
        const int j0 = (int)(i0 % p.W);
        const size_t ch = i0 / p.W;                                   // c * H + h
        float xv[V], ev[V], ecv[V], nz[V], mv[V], gv[V], n0[V];
        load_v<V>(xrow + i0, true, xv);
        load_v<V>(erow + i0, true, ev);
        if (ecrow) load_v<V>(ecrow + i0, true, ecv);
        else
#pragma unroll
            for (int k = 0; k < V; ++k) ecv[k] = 0.f;
#pragma unroll
        for (int k = 0; k < V; ++k) mv[k] = gv[k] = n0[k] = 0.f;
        if (blend) {
            load_v<V>(mask + (mchw ? i0 : i0 % HW), avec, mv);
            load_v<V>(guide + i0, avec, gv);
            if (blend == 1) load_v<V>(init + i0, avec, n0);
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            float n = 0.f;
            if (nmode) {
                int col = p.cols[coff + j0 + k];
                col = col < 0 ? 0 : (col >= dw ? dw - 1 : col);
                const uint64_t e = ((uint64_t)smp * p.C * p.H + ch) * (uint64_t)dw + (uint64_t)col;
                n = nmode == 1 ? draw[e] : philox_normal_at(seed, offset, e);
            }
            nz[k] = n;
        }
        float o[V];
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = step_element(xv[k], ev[k], ecrow != nullptr, ecv[k], scale, cf, nz[k], blend, mv[k], gv[k], n0[k], q0, q1);
        store_v<V>(orow_p + i0, o);
        if (drow_p) store_v<V>(drow_p + i0, o);
    }
}

// One row of the solver step: pieces of V elements, grid-strided along x.  ds_dpm_step_kernel and dpm_step_rows_kernel both run this
// loop, so a row of ds_dpm_step_rows is the same bits as ds_dpm_step given the same inputs.  hist may be null only where cf[4] == 0;
// avec / hvec: the blend operands / the history are 16-byte aligned (V == 4 only).
struct dpm_row_args {
    const float* x; const float* eps; const float* eps_c; float* hist; float* out; float* dup;
    const float* mask; const float* guide; const float* init;
    float cf[5], q0, q1, scale;
    int blend, mask_chw;
};
template <int V>
__device__ __forceinline__ void dpm_row(const dpm_row_args& a, int HW, size_t CHW, bool avec, bool hvec) {
    const bool second = a.cf[4] != 0.f;
    const size_t nv = CHW / V;
    for (size_t v = blockIdx.x * (size_t)blockDim.x + threadIdx.x; v < nv; v += (size_t)gridDim.x * blockDim.x) {
        const size_t i0 = v * V;
        float xv[V], ev[V], ecv[V], hv[V], mv[V], gv[V], n0[V];
        load_v<V>(a.x + i0, true, xv);
        load_v<V>(a.eps + i0, true, ev);
        if (a.eps_c) load_v<V>(a.eps_c + i0, true, ecv);
        else
#pragma unroll
            for (int k = 0; k < V; ++k) ecv[k] = 0.f;
        if (second) load_v<V>(a.hist + i0, hvec, hv);
        else
#pragma unroll
            for (int k = 0; k < V; ++k) hv[k] = 0.f;
#pragma unroll
        for (int k = 0; k < V; ++k) mv[k] = gv[k] = n0[k] = 0.f;
        if (a.blend) {
            load_v<V>(a.mask + (a.mask_chw ? i0 : i0 % HW), avec, mv);
            load_v<V>(a.guide + i0, avec, gv);
            if (a.blend == 1) load_v<V>(a.init + i0, avec, n0);
        }
        float o[V];
#pragma unroll
        for (int k = 0; k < V; ++k)
            o[k] = dpm_element(xv[k], ev[k], a.eps_c != nullptr, ecv[k], a.scale, a.cf, second, hv[k], a.blend, mv[k], gv[k], n0[k], a.q0, a.q1);
        store_v<V>(a.out + i0, o);
        if (a.dup) store_v<V>(a.dup + i0, o);
        if (a.hist) {
            if (hvec) store_v<V>(a.hist + i0, hv);
            else
#pragma unroll
                for (int k = 0; k < V; ++k) a.hist[i0 + k] = hv[k];
        }
    }
}
__device__ __forceinline__ void nan_row(float* out, float* dup, size_t CHW) {
    const float nan = __builtin_nanf("");
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < CHW; i += (size_t)gridDim.x * blockDim.x) {
        out[i] = nan;
        if (dup) dup[i] = nan;
    }
}

// grid (x: pieces of a row, y: sample).  V == 4 only when W % 4 == 0 and every pointer given is 16-byte aligned
template <int V>
__global__ __launch_bounds__(256) void dpm_step_kernel(const ds_dpm_step_params p) {
    const int b = blockIdx.y;
    const int HW = p.H * p.W;
    const size_t CHW = (size_t)p.C * HW;
    dpm_row_args a;
#pragma unroll
    for (int k = 0; k < 5; ++k) a.cf[k] = p.coef[(size_t)b * 5 + k];
    a.out = p.out + (size_t)b * CHW;
    a.dup = nullptr;
    if (!p.hist && a.cf[4] != 0.f) {                // a second-order row without a history: shown in the result, nothing is read
        nan_row(a.out, nullptr, CHW);
        return;
    }
    a.x = p.x + (size_t)b * CHW;
    a.eps = p.eps + (size_t)b * CHW;
    a.eps_c = p.eps_cond ? p.eps_cond + (size_t)b * CHW : nullptr;
    a.hist = p.hist ? p.hist + (size_t)b * CHW : nullptr;
    a.blend = p.blend_mode;
    a.mask_chw = p.mask_chw;
    a.mask = a.guide = a.init = nullptr;
    a.q0 = a.q1 = 0.f;
    if (p.blend_mode) {
        a.mask = p.mask + (size_t)b * (p.mask_chw ? CHW : (size_t)HW);
        a.guide = p.guide + (size_t)b * CHW;
        if (p.blend_mode == 1) {
            a.init = p.init_noise + (size_t)b * CHW;
            a.q0 = p.qcoef[(size_t)b * 2];
            a.q1 = p.qcoef[(size_t)b * 2 + 1];
        }
    }
    a.scale = p.cfg_scale;
    dpm_row<V>(a, HW, CHW, V == 4, V == 4);
}

// ds_step_rows' tables and bounds contract (see step_rows_kernel) plus one history address per row
template <int V>
__global__ __launch_bounds__(256) void dpm_step_rows_kernel(const ds_step_rows_params p, const uint64_t* hrow) {
    const int r = blockIdx.y;
    const int32_t* ir = p.irow + (size_t)r * DS_SR_NI;
    const float* fr = p.frow + (size_t)r * DS_SR_NF;
    const uint64_t* pr = p.prow + (size_t)r * DS_SR_NP;
    const int xr = ir[DS_SR_X], er = ir[DS_SR_EPS], ecr = ir[DS_SR_EPSC], orow = ir[DS_SR_OUT], dup = ir[DS_SR_DUP];
    const int blend = ir[DS_SR_BLEND], nmode = ir[DS_SR_NOISE];
    dpm_row_args a;
    a.guide = reinterpret_cast<const float*>(pr[DS_SR_GUIDE]);
    a.init = reinterpret_cast<const float*>(pr[DS_SR_INIT]);
    a.mask = reinterpret_cast<const float*>(pr[DS_SR_MASKP]);
    a.hist = reinterpret_cast<float*>(hrow[r]);
#pragma unroll
    for (int k = 0; k < 5; ++k) a.cf[k] = fr[DS_SR_COEF + k];
    const int HW = p.H * p.W;
    const size_t CHW = (size_t)p.C * HW;
    if (orow < 0 || orow >= p.Bout) return;
    a.out = p.out + (size_t)orow * CHW;
    const bool bad = xr < 0 || xr >= p.Bx || er < 0 || er >= p.Beps || ecr >= p.Beps || dup >= p.Bout || blend < 0 || blend > 2 ||
                     nmode != 0 || (blend && (!a.guide || !a.mask || (blend == 1 && !a.init))) || (!a.hist && a.cf[4] != 0.f);
    if (bad) {
        nan_row(a.out, dup >= 0 && dup < p.Bout ? p.out + (size_t)dup * CHW : nullptr, CHW);
        return;
    }
    a.dup = dup >= 0 ? p.out + (size_t)dup * CHW : nullptr;
    a.x = p.x + (size_t)xr * CHW;
    a.eps = p.eps + (size_t)er * CHW;
    a.eps_c = ecr >= 0 ? p.eps + (size_t)ecr * CHW : nullptr;
    a.blend = blend;
    a.mask_chw = ir[DS_SR_MASK_CHW];
    a.q0 = fr[DS_SR_Q0];
    a.q1 = fr[DS_SR_Q1];
    a.scale = fr[DS_SR_CFG];
    // (a history row is a request's own allocation: its alignment is looked at per row, like the blend operands')
    const bool hvec = V == 4 && (((uint64_t)a.hist) & 15) == 0;
    const bool avec = V == 4 && ((((uint64_t)a.guide | (uint64_t)a.init | (uint64_t)a.mask) & 15) == 0);
    dpm_row<V>(a, HW, CHW, avec, hvec);
}
#pragma clang fp contract(fast)

// ------------------------------------------------------------------------------------------------ guidance rescale
// out = g e with e = guided_eps(eps_u, eps_c, s) and g = phi std(eps_c) / std(e) + (1 - phi) over one row of N elements.  One block of
// CR_THREADS per row: piece v (elements [4v, 4v + 4)) belongs to thread v % CR_THREADS in the 16-byte and in the scalar form alike, a
// thread adds its elements in ascending order into float64 sums, and the sums meet in wave_sum and then wave by wave — an order that
// N alone decides.  Two passes about the mean: sums, then squares of the distances from the means (the common 1 / (N - 1) of the two
// variances cancels in the ratio).  cfg_rescale_kernel and cfg_rescale_rows_kernel both run cfg_rescale_row, so a row of
// ds_cfg_rescale_rows is the same bits as ds_cfg_rescale given the same inputs.
constexpr int CR_THREADS = 1024, CR_WAVES = CR_THREADS / 64;

// piece at element i0: n (1..4) elements are inside the row; vec only where every piece is whole
__device__ __forceinline__ void cr_load(const float* p, int i0, int n, bool vec, float (&v)[4]) {
    if (vec) {
        load_v<4>(p + i0, true, v);
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < n ? p[i0 + k] : 0.f;
}
// both totals to every thread
__device__ __forceinline__ void cr_block_sum(double& a, double& b, double (&red)[2][CR_WAVES]) {
    a = wave_sum(a);
    b = wave_sum(b);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    a = b = 0.0;
#pragma unroll
    for (int w = 0; w < CR_WAVES; ++w) {
        a += red[0][w];
        b += red[1][w];
    }
}
#pragma clang fp contract(off)
__device__ __forceinline__ float cfg_rescale_row(const float* u, const float* c, float* out, int N, float scale, float phi,
                                                 double (&red)[2][2][CR_WAVES]) {
    const bool vec = N % 4 == 0 && ((((uint64_t)u | (uint64_t)c | (uint64_t)out) & 15) == 0);
    const int nv = (N + 3) / 4;
    float g = 1.0f;
    if (phi != 0.f) {                                   // (block-uniform)
        double sc = 0.0, se = 0.0;
        for (int v = threadIdx.x; v < nv; v += CR_THREADS) {
            const int i0 = v * 4, n = min(4, N - i0);
            float uv[4], cv[4];
            cr_load(u, i0, n, vec, uv);
            cr_load(c, i0, n, vec, cv);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) {
                    sc += (double)cv[k];
                    se += (double)guided_eps(uv[k], true, cv[k], scale);
                }
        }
        cr_block_sum(sc, se, red[0]);
        const double mc = sc / N, me = se / N;
        double qc = 0.0, qe = 0.0;
        for (int v = threadIdx.x; v < nv; v += CR_THREADS) {
            const int i0 = v * 4, n = min(4, N - i0);
            float uv[4], cv[4];
            cr_load(u, i0, n, vec, uv);
            cr_load(c, i0, n, vec, cv);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) {
                    const double dc = (double)cv[k] - mc, de = (double)guided_eps(uv[k], true, cv[k], scale) - me;
                    qc += dc * dc;
                    qe += de * de;
                }
        }
        cr_block_sum(qc, qe, red[1]);
        const double ratio = qe > 0.0 ? sqrt(qc / qe) : 1.0;          // std(e) == 0: nothing to scale
        g = (float)((double)phi * ratio + (1.0 - (double)phi));
    }
    for (int v = threadIdx.x; v < nv; v += CR_THREADS) {
        const int i0 = v * 4, n = min(4, N - i0);
        float uv[4], cv[4], o[4];
        cr_load(u, i0, n, vec, uv);
        cr_load(c, i0, n, vec, cv);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = g * guided_eps(uv[k], true, cv[k], scale);
        if (vec) store_v<4>(out + i0, o);
        else
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) out[i0 + k] = o[k];
    }
    return g;
}
#pragma clang fp contract(fast)

// grid: one block per sample
__global__ __launch_bounds__(CR_THREADS) void cfg_rescale_kernel(const ds_cfg_rescale_params p) {
    __shared__ double red[2][2][CR_WAVES];
    const size_t off = (size_t)blockIdx.x * p.CHW;
    const float g = cfg_rescale_row(p.eps_u + off, p.eps_c + off, p.out + off, p.CHW, p.cfg_scale, p.phi, red);
    if (p.gain && threadIdx.x == 0) p.gain[blockIdx.x] = g;
}

// grid: one block per table row.  The table is the host's: a row that points outside the buffer is never read out of bounds (see
// step_rows_kernel)
__global__ __launch_bounds__(CR_THREADS) void cfg_rescale_rows_kernel(const ds_cfg_rescale_rows_params p) {
    __shared__ double red[2][2][CR_WAVES];
    const int r = blockIdx.x;
    const int32_t* ir = p.irow + (size_t)r * DS_CR_NI;
    const float* fr = p.frow + (size_t)r * DS_CR_NF;
    const int ur = ir[DS_CR_U], cr = ir[DS_CR_C], orow = ir[DS_CR_OUT];
    const float scale = fr[DS_CR_SCALE], phi = fr[DS_CR_PHI];
    const bool bad = ur < 0 || ur >= p.Beps || cr < 0 || cr >= p.Beps || !(phi >= 0.f && phi <= 1.f);
    float g = __builtin_nanf("");
    if (orow >= 0 && orow < p.Beps) {                   // (block-uniform, like bad)
        float* out = p.eps + (size_t)orow * p.CHW;
        if (bad)
            for (int i = threadIdx.x; i < p.CHW; i += CR_THREADS) out[i] = g;
        else
            g = cfg_rescale_row(p.eps + (size_t)ur * p.CHW, p.eps + (size_t)cr * p.CHW, out, p.CHW, scale, phi, red);
    }
    if (p.gain && threadIdx.x == 0) p.gain[r] = g;
}

__global__ void gather_cols_kernel(const float* src, int src_w, const int32_t* cols, int out_w, float* out, size_t total) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t row = i / out_w;
        const int j = i % out_w;
        out[i] = src[row * src_w + cols[j]];
    }
}

inline int blocks_for(size_t n, int cap = 8192) {
    const size_t b = (n + 255) / 256;
    return (int)(b < (size_t)cap ? (b ? b : 1) : cap);
}

}  // namespace

namespace {
// one block per row: two-pass (mean, then centred variance) in fp32 with double partial sums
__global__ __launch_bounds__(256) void add_layernorm_kernel(const float* a, const float* r, const float* gamma, const float* beta, int D,
                                                            float eps, float* out) {
    __shared__ double red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* ab = a + (size_t)b * D;
    const float* rb = r + (size_t)b * D;
    double s = 0.0;
    for (int i = tid; i < D; i += 256) s += (double)(ab[i] + rb[i]);
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const float mean = (float)(red[0] / D);
    __syncthreads();
    double q = 0.0;
    for (int i = tid; i < D; i += 256) {
        const float d = (ab[i] + rb[i]) - mean;
        q += (double)d * d;
    }
    red[tid] = q;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const float rstd = 1.0f / sqrtf((float)(red[0] / D) + eps);
    for (int i = tid; i < D; i += 256) out[(size_t)b * D + i] = ((ab[i] + rb[i]) - mean) * rstd * gamma[i] + beta[i];
}
}  // namespace

extern "C" int ds_add_layernorm(const float* a, const float* r, const float* gamma, const float* beta, int B, int D, float eps, float* out,
                                void* stream) {
    DS_REQUIRE(a && r && gamma && beta && out && B > 0 && D > 0, "add_layernorm: bad args");
    hipLaunchKernelGGL(add_layernorm_kernel, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a, r, gamma, beta, D, eps, out);
    DS_CHECK_LAUNCH("add_layernorm");
    return DS_OK;
}

extern "C" int ds_sinusoid(const int64_t* t, const float* freqs, int B, int half, float* out, void* stream) {
    DS_REQUIRE(t && freqs && out && B > 0 && half > 0, "sinusoid: bad args");
    hipLaunchKernelGGL(sinusoid_kernel, dim3((B * half + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), t, freqs, B, half, out);
    DS_CHECK_LAUNCH("sinusoid");
    return DS_OK;
}

// y = act(x) elementwise (fp32; may run in place).  ds_linear's act_in evaluates the activation once per (16-output wave, element): for a
// wide stack of outputs over one small input (the 44 per-block time biases from the 128 x 384 time embedding: 840 waves x 49k exact-erf GELUs,
// 85 us) the host applies it once with this kernel and calls ds_linear with DS_ACT_NONE (same fp32 function: identical results).
__global__ __launch_bounds__(256) void act_kernel(const float* x, size_t n, int act, float* y) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) y[i] = act_apply(x[i], act);
}

extern "C" int ds_activation(const float* x, size_t n, int act, float* y, void* stream) {
    DS_REQUIRE(x && y && n > 0, "activation: bad args");
    DS_REQUIRE(act == DS_ACT_NONE || act == DS_ACT_GELU || act == DS_ACT_SILU, "activation: unknown act %d", act);
    const size_t nb = (n + 255) / 256;
    hipLaunchKernelGGL(act_kernel, dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, n, act, y);
    DS_CHECK_LAUNCH("activation");
    return DS_OK;
}

extern "C" int ds_linear(const float* x, int xs, const float* W, const float* bias, int B, int K, int O, int act_in, float* y,
                         int ys, void* stream) {
    DS_REQUIRE(x && W && y && B > 0 && K > 0 && O > 0 && xs >= K && ys >= O, "linear: bad args");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (K % 16 == 0 && xs % 4 == 0 && ds_aligned16(x) && ds_aligned16(W)) {
        const int nw = (O + 15) / 16;
        dim3 grid((nw + 3) / 4), blk(256);
        if (B <= 16) hipLaunchKernelGGL(linear_mfma_kernel<1>, grid, blk, 0, st, x, xs, W, bias, B, K, O, act_in, y, ys);
        else if (B <= 32) hipLaunchKernelGGL(linear_mfma_kernel<2>, grid, blk, 0, st, x, xs, W, bias, B, K, O, act_in, y, ys);
        else if (B <= 64) hipLaunchKernelGGL(linear_mfma_kernel<4>, grid, blk, 0, st, x, xs, W, bias, B, K, O, act_in, y, ys);
        else hipLaunchKernelGGL(linear_mfma_kernel<8>, grid, blk, 0, st, x, xs, W, bias, B, K, O, act_in, y, ys);
        DS_CHECK_LAUNCH("linear_mfma");
        return DS_OK;
    }
    const long waves = (long)B * O;
    hipLaunchKernelGGL(linear_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, xs, W,
                       bias, B, K, O, act_in, y, ys);
    DS_CHECK_LAUNCH("linear");
    return DS_OK;
}

extern "C" int ds_nchw_to_nhwc(const float* x, int B, int C, int H, int W, void* out, int Cp, int dtype, void* stream) {
    DS_REQUIRE(x && out && B > 0 && C > 0 && Cp >= C && H > 0 && W > 0, "nchw_to_nhwc: bad args");
    const size_t total = (size_t)B * H * W * Cp;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == DS_BF16) hipLaunchKernelGGL(nchw_to_nhwc_kernel<bf16>, dim3(blocks_for(total)), dim3(256), 0, st, x, C, H * W, (bf16*)out, Cp, total);
    else if (dtype == DS_F32) hipLaunchKernelGGL(nchw_to_nhwc_kernel<float>, dim3(blocks_for(total)), dim3(256), 0, st, x, C, H * W, (float*)out, Cp, total);
    else DS_FAIL(DS_EINVAL, "nchw_to_nhwc: dtype %d", dtype);
    DS_CHECK_LAUNCH("nchw_to_nhwc");
    return DS_OK;
}

namespace {
// First layer of the VQGAN decoder (VQGAN.py:345: Conv2d(embedding_dim, hidden, 1, bias=False) on the NCHW latent): out[b][pix][co] = sum_ci w[co][ci] x[b][ci][pix],
// bf16 NHWC.  The layout change + the generic 1x1 tile (K padded to 32, N to 96) were 11 + 85 us for a 168 MB output; here a thread takes one
// pixel's Cin values (coalesced along the pixels of each plane) and writes one 16-byte piece of its output row.
template <int CIN>
__global__ __launch_bounds__(256) void conv1x1_in_nchw_kernel(const float* x, const float* w, const float* bias, int HW, int Cout, bf16* out, size_t npix) {
    // blockDim = NP x rows: a thread keeps ONE 16-byte output piece (its 8 x CIN weights in registers) and walks pixels (the first form fetched
    // its 32 weights per output piece: 160 us, slower than what it replaced)
    const int NP = Cout >> 3, rows = blockDim.x / NP, piece = threadIdx.x % NP, row = threadIdx.x / NP;
    float wr[8][CIN], bv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        bv[j] = bias ? bias[piece * 8 + j] : 0.f;
#pragma unroll
        for (int c = 0; c < CIN; ++c) wr[j][c] = w[(piece * 8 + j) * CIN + c];
    }
    for (size_t bp = (size_t)blockIdx.x * rows + row; bp < npix; bp += (size_t)gridDim.x * rows) {
        const size_t b = bp / HW, pix = bp % HW;
        float xv[CIN];
#pragma unroll
        for (int c = 0; c < CIN; ++c) xv[c] = x[(b * CIN + c) * HW + pix];
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float a = bv[j];
#pragma unroll
            for (int c = 0; c < CIN; ++c) a = fmaf(wr[j][c], xv[c], a);
            o[j] = a;
        }
        Vec16<bf16>::store(out + (bp * Cout + piece * 8), o);
    }
}
}  // namespace

extern "C" int ds_conv1x1_in_nchw(const float* x, int B, int Cin, int HW, const float* w, const float* bias, int Cout, void* out, void* stream) {
    DS_REQUIRE(x && w && out && B > 0 && HW > 0 && Cout > 0 && Cout % 8 == 0, "conv1x1_in_nchw: bad args (Cout %% 8 == 0)");
    DS_REQUIRE(Cin == 4 || Cin == 8, "conv1x1_in_nchw: Cin=%d unsupported (4, 8)", Cin);
    if (!ds_aligned16(out)) DS_FAIL(DS_EALIGN, "conv1x1_in_nchw: out must be 16-byte aligned");
    DS_REQUIRE(Cout / 8 <= 256, "conv1x1_in_nchw: Cout=%d too large", Cout);
    const size_t npix = (size_t)B * HW;
    const int NP = Cout / 8, threads = NP * (256 / NP), rows = threads / NP;
    const int blocks = blocks_for((npix + rows - 1) / rows * 64, 16384);                 // (blocks_for counts 256 items per block: >= 4 pixels per thread)
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (Cin == 4) hipLaunchKernelGGL(conv1x1_in_nchw_kernel<4>, dim3(blocks), dim3(threads), 0, st, x, w, bias, HW, Cout, (bf16*)out, npix);
    else hipLaunchKernelGGL(conv1x1_in_nchw_kernel<8>, dim3(blocks), dim3(threads), 0, st, x, w, bias, HW, Cout, (bf16*)out, npix);
    DS_CHECK_LAUNCH("conv1x1_in_nchw");
    return DS_OK;
}

namespace {
// dst[0, n) = dst[n, 2n) = src[0, n) in 16-byte pieces: one read, two writes (two device-to-device copies read the source twice)
// INPLACE (dst == src, r05): the first half is already where it belongs — one read, ONE write (the plan computes the shared prefix of a
// classifier-free-guidance batch straight into the first half of the full-batch tensor)
template <bool INPLACE>
__global__ __launch_bounds__(256) void dup_batch_kernel(const u32x4* src, u32x4* dst, size_t nvec) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
        const u32x4 v = src[i];
        if (!INPLACE) dst[i] = v;
        dst[i + nvec] = v;
    }
}
}  // namespace

extern "C" int ds_dup_batch(const void* src, void* dst, size_t nbytes, void* stream) {
    DS_REQUIRE(src && dst && nbytes > 0, "dup_batch: bad args");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nbytes % 16 == 0 && ds_aligned16(src) && ds_aligned16(dst)) {
        const size_t nvec = nbytes / 16;
        const size_t want = (nvec + 255) / 256;
        const dim3 grid((unsigned)(want < 16384 ? want : 16384));
        if (src == dst) hipLaunchKernelGGL(dup_batch_kernel<true>, grid, dim3(256), 0, st, reinterpret_cast<const u32x4*>(src), reinterpret_cast<u32x4*>(dst), nvec);
        else hipLaunchKernelGGL(dup_batch_kernel<false>, grid, dim3(256), 0, st, reinterpret_cast<const u32x4*>(src), reinterpret_cast<u32x4*>(dst), nvec);
        DS_CHECK_LAUNCH("dup_batch");
        return DS_OK;
    }
    hipError_t e = src == dst ? hipSuccess : hipMemcpyAsync(dst, src, nbytes, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(static_cast<char*>(dst) + nbytes, src, nbytes, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) DS_FAIL(DS_ELAUNCH, "dup_batch: %s", hipGetErrorString(e));
    return DS_OK;
}

extern "C" int ds_nhwc_to_nchw(const void* x, int dtype, int B, int C, int Cs, int H, int W, float* out, void* stream) {
    DS_REQUIRE(x && out && B > 0 && C > 0 && Cs >= C && H > 0 && W > 0, "nhwc_to_nchw: bad args");
    const size_t total = (size_t)B * C * H * W;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == DS_BF16) hipLaunchKernelGGL(nhwc_to_nchw_kernel<bf16>, dim3(blocks_for(total)), dim3(256), 0, st, (const bf16*)x, C, Cs, H * W, out, total);
    else if (dtype == DS_F32) hipLaunchKernelGGL(nhwc_to_nchw_kernel<float>, dim3(blocks_for(total)), dim3(256), 0, st, (const float*)x, C, Cs, H * W, out, total);
    else DS_FAIL(DS_EINVAL, "nhwc_to_nchw: dtype %d", dtype);
    DS_CHECK_LAUNCH("nhwc_to_nchw");
    return DS_OK;
}

extern "C" int ds_ddim_step(const ds_step_params* p, void* stream) {
    DS_REQUIRE(p && p->x && p->eps && p->noise && p->out && p->coef, "ddim_step: null pointer");
    DS_REQUIRE(p->B > 0 && p->CHW > 0 && p->HW > 0 && p->CHW % p->HW == 0, "ddim_step: bad sizes");
    DS_REQUIRE(p->blend_mode >= 0 && p->blend_mode <= 2, "ddim_step: blend_mode %d", p->blend_mode);
    DS_REQUIRE(p->blend_mode == 0 || (p->guide && p->mask), "ddim_step: blend needs guide and mask");
    DS_REQUIRE(p->blend_mode != 1 || (p->init_noise && p->qcoef), "ddim_step: blend 1 needs init_noise and qcoef");
    const size_t total = (size_t)p->B * p->CHW;
    hipLaunchKernelGGL(ddim_step_kernel, dim3(blocks_for(total)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *p, total);
    DS_CHECK_LAUNCH("ddim_step");
    return DS_OK;
}

extern "C" int ds_step_rows(const ds_step_rows_params* p, void* stream) {
    DS_REQUIRE(p && p->x && p->eps && p->out && p->irow && p->frow && p->prow, "step_rows: null pointer");
    DS_REQUIRE(p->R > 0 && p->R <= 65535 && p->C > 0 && p->H > 0 && p->W > 0, "step_rows: bad sizes (R=%d C=%d H=%d W=%d)", p->R, p->C, p->H, p->W);
    DS_REQUIRE(p->Bx > 0 && p->Beps > 0 && p->Bout > 0 && p->n_cols >= 0, "step_rows: bad row counts (Bx=%d Beps=%d Bout=%d n_cols=%d)",
               p->Bx, p->Beps, p->Bout, p->n_cols);
    DS_REQUIRE(p->n_cols == 0 || p->cols, "step_rows: n_cols > 0 needs cols");
    const size_t CHW = (size_t)p->C * p->H * p->W;
    const bool vec = p->W % 4 == 0 && ds_aligned16(p->x) && ds_aligned16(p->eps) && ds_aligned16(p->out);
    const size_t nv = vec ? CHW / 4 : CHW;
    const dim3 grid((unsigned)blocks_for(nv, 4096), (unsigned)p->R);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(step_rows_kernel<4>, grid, dim3(256), 0, st, *p);
    else hipLaunchKernelGGL(step_rows_kernel<1>, grid, dim3(256), 0, st, *p);
    DS_CHECK_LAUNCH("step_rows");
    return DS_OK;
}

extern "C" int ds_dpm_step(const ds_dpm_step_params* p, void* stream) {
    DS_REQUIRE(p && p->x && p->eps && p->out && p->coef, "dpm_step: null pointer");
    DS_REQUIRE(p->B > 0 && p->B <= 65535 && p->C > 0 && p->H > 0 && p->W > 0, "dpm_step: bad sizes (B=%d C=%d H=%d W=%d)", p->B, p->C, p->H, p->W);
    DS_REQUIRE(p->blend_mode >= 0 && p->blend_mode <= 2, "dpm_step: blend_mode %d", p->blend_mode);
    DS_REQUIRE(p->blend_mode == 0 || (p->guide && p->mask), "dpm_step: blend needs guide and mask");
    DS_REQUIRE(p->blend_mode != 1 || (p->init_noise && p->qcoef), "dpm_step: blend 1 needs init_noise and qcoef");
    const size_t CHW = (size_t)p->C * p->H * p->W;
    // (NULL is 16-byte aligned: an operand that is not given does not decide the path)
    const bool vec = p->W % 4 == 0 && ds_aligned16(p->x) && ds_aligned16(p->eps) && ds_aligned16(p->eps_cond) && ds_aligned16(p->hist) &&
                     ds_aligned16(p->out) && ds_aligned16(p->guide) && ds_aligned16(p->init_noise) && ds_aligned16(p->mask);
    const dim3 grid((unsigned)blocks_for(vec ? CHW / 4 : CHW, 4096), (unsigned)p->B);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(dpm_step_kernel<4>, grid, dim3(256), 0, st, *p);
    else hipLaunchKernelGGL(dpm_step_kernel<1>, grid, dim3(256), 0, st, *p);
    DS_CHECK_LAUNCH("dpm_step");
    return DS_OK;
}

extern "C" int ds_dpm_step_rows(const ds_step_rows_params* p, const uint64_t* hrow, void* stream) {
    DS_REQUIRE(p && p->x && p->eps && p->out && p->irow && p->frow && p->prow && hrow, "dpm_step_rows: null pointer");
    DS_REQUIRE(p->R > 0 && p->R <= 65535 && p->C > 0 && p->H > 0 && p->W > 0, "dpm_step_rows: bad sizes (R=%d C=%d H=%d W=%d)", p->R, p->C, p->H, p->W);
    DS_REQUIRE(p->Bx > 0 && p->Beps > 0 && p->Bout > 0, "dpm_step_rows: bad row counts (Bx=%d Beps=%d Bout=%d)", p->Bx, p->Beps, p->Bout);
    const size_t CHW = (size_t)p->C * p->H * p->W;
    const bool vec = p->W % 4 == 0 && ds_aligned16(p->x) && ds_aligned16(p->eps) && ds_aligned16(p->out);
    const dim3 grid((unsigned)blocks_for(vec ? CHW / 4 : CHW, 4096), (unsigned)p->R);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(dpm_step_rows_kernel<4>, grid, dim3(256), 0, st, *p, hrow);
    else hipLaunchKernelGGL(dpm_step_rows_kernel<1>, grid, dim3(256), 0, st, *p, hrow);
    DS_CHECK_LAUNCH("dpm_step_rows");
    return DS_OK;
}

extern "C" int ds_cfg_rescale(const ds_cfg_rescale_params* p, void* stream) {
    DS_REQUIRE(p && p->eps_u && p->eps_c && p->out, "cfg_rescale: null pointer");
    DS_REQUIRE(p->B > 0 && p->CHW > 0 && p->CHW <= (1 << 30), "cfg_rescale: bad sizes (B=%d CHW=%d)", p->B, p->CHW);
    DS_REQUIRE(p->phi >= 0.f && p->phi <= 1.f, "cfg_rescale: phi %g is not in [0, 1]", (double)p->phi);
    hipLaunchKernelGGL(cfg_rescale_kernel, dim3((unsigned)p->B), dim3(CR_THREADS), 0, reinterpret_cast<hipStream_t>(stream), *p);
    DS_CHECK_LAUNCH("cfg_rescale");
    return DS_OK;
}

extern "C" int ds_cfg_rescale_rows(const ds_cfg_rescale_rows_params* p, void* stream) {
    DS_REQUIRE(p && p->eps && p->irow && p->frow, "cfg_rescale_rows: null pointer");
    DS_REQUIRE(p->R > 0 && p->CHW > 0 && p->CHW <= (1 << 30) && p->Beps > 0, "cfg_rescale_rows: bad sizes (R=%d CHW=%d Beps=%d)", p->R, p->CHW,
               p->Beps);
    hipLaunchKernelGGL(cfg_rescale_rows_kernel, dim3((unsigned)p->R), dim3(CR_THREADS), 0, reinterpret_cast<hipStream_t>(stream), *p);
    DS_CHECK_LAUNCH("cfg_rescale_rows");
    return DS_OK;
}

extern "C" int ds_philox_normal(float* out, size_t n, uint64_t seed, uint64_t offset, void* stream) {
    DS_REQUIRE(out && n > 0, "philox_normal: bad args");
    hipLaunchKernelGGL(philox_normal_kernel, dim3(blocks_for((n + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), out, n, seed, offset);
    DS_CHECK_LAUNCH("philox_normal");
    return DS_OK;
}

extern "C" int ds_gather_cols(const float* src, int rows, int src_w, const int32_t* cols, int out_w, float* out, void* stream) {
    DS_REQUIRE(src && cols && out && rows > 0 && src_w > 0 && out_w > 0, "gather_cols: bad args");
    const size_t total = (size_t)rows * out_w;
    hipLaunchKernelGGL(gather_cols_kernel, dim3(blocks_for(total)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, src_w, cols, out_w, out, total);
    DS_CHECK_LAUNCH("gather_cols");
    return DS_OK;
}
