// The pictures the reference's UI shows beside every sound (gfx950): the spectrogram and phase images of an STFT+ tensor
// (webUI/natural_language_guided_4/utils.py:8-86 applied to tools.decode_stft / tools.depad_STFT, utils.py:172-181,229-238,249-259)
// and the latent image (utils.py:89-128), rendered from tensors that are already in HBM.
//
// ds_stft_images.  Per clip, with m = expm1(enc[0]) (or of the second magnitude source `amp`), s = |m|:
//   spectrogram  red = green = trunc(255 (dB + 80) / 80), dB = 10 log10(max(s, 1e-16) + 1e-16) - 10 log10(max(ref, 1e-16) + 1e-16) clipped below
//                at -80, ref = the clip's largest s; blue = 63 (the reference's constant -60 dB through the same map)
//   phase        phi = atan2(m sin, m cos) — the angle of m e^{i atan2(sin, cos)}: turned by pi where m < 0, 0 for a zero-padded column
//                (0, 1, 0) — red = green = the low byte of int32(255 (phi + 1) / 2) (phi spans (-pi, pi]: a third of the values leave [0, 255];
//                the reference leaves them to numpy's float -> uint8 cast, which wraps on x86; here the cast is defined), blue = 51
//   both (F + 1, T, 3), row 0 = the highest bin, the last row = the implied zero bin (spectrogram: the floor, phase: 127).
// Two launches: (a) minimum and maximum of the raw magnitude channel per clip — expm1 is monotonic, so max s = max(expm1(max), -expm1(min)) —
// as per-block partials in the workspace, finished by every consumer block (no atomics; max / min do not depend on the order); (b) the image
// pass.  An image is a dense stream of 3-byte pixels, so a block owns UI_NP consecutive pixels of the flattened (row, t) order = one
// contiguous range of output bytes: a thread reads four consecutive t of one bin (one 16-byte load per channel), packs its twelve bytes per
// image into LDS (three dword writes, 3-dword lane stride: conflict free), and the block then streams the range out in 16-byte stores.  The
// range is placed in LDS at the offset its first byte has inside its 16-byte line of global memory, so every aligned 16-byte store reads an
// aligned 16 bytes of LDS whatever 3 T and the clip's byte offset are; the (at most 15 + 15) bytes in front of the first and behind the last
// boundary go out one by one.  T % 4 != 0 or tensors that are not 16-byte aligned take the same kernel with one pixel per thread and round
// (4-byte loads, byte writes into LDS); the stores are the same.
//
// ds_latent_image.  (x - min) / (max - min) * 255 per (sample, channel) in fp32 IN THAT ORDER (the reference works on the tensor's own float32
// array), truncated, channels last, flipped vertically: [B][H][W][4] bytes.  A constant channel (0 / 0) renders 0.  The reference's 8 x 8
// enlargement is a repeat of bytes: done here it would put 64 x the bytes (2.1 MB per production latent, whose fp32 source is 131 KB) on the
// way to the host, so the Python wrapper enlarges after the copy (np.repeat of bytes: exact).  The input is not written (the reference
// normalises in place when it is handed a CPU tensor; that is not reproduced).
#include "common.hpp"

namespace {

constexpr int UI_NB_MAX = 64;            // partial (min, max) pairs per clip: one wave of the consumer finishes them
constexpr int UI_MM_ELEMS = 4096;        // elements per extremes block and round
constexpr int UI_NP = 2048;              // pixels per image block
constexpr int UI_ROW = 3 * UI_NP + 16;   // bytes of one image's LDS range incl. the alignment shift

inline int ui_mm_blocks(long long n) {
    const long long nb = (n + UI_MM_ELEMS - 1) / UI_MM_ELEMS;
    return nb < 1 ? 1 : (nb > UI_NB_MAX ? UI_NB_MAX : (int)nb);
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

// block minimum / maximum -> thread 0
__device__ __forceinline__ void block_minmax(float& mn, float& mx, float* red) {
    mn = wave_min(mn);
    mx = wave_max(mx);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[2 * wave] = mn;
        red[2 * wave + 1] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) {
            mn = fminf(mn, red[2 * w]);
            mx = fmaxf(mx, red[2 * w + 1]);
        }
}

// minimum and maximum of n floats at src + b * bstride: block (x, b) takes every nb-th group of 256 16-byte pieces; the (at most 3 + 3)
// elements outside the 16-byte aligned body belong to block 0.  part [B][nb][2].
__global__ __launch_bounds__(256) void ui_minmax_kernel(const float* src, long long bstride, int n, int nb, float* part) {
    __shared__ float red[8];
    const int tid = threadIdx.x, b = blockIdx.y;
    const float* p = src + (size_t)b * bstride;
    float mn = INFINITY, mx = -INFINITY;
    int head = (int)((4 - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3);
    head = head < n ? head : n;
    const int nv = (n - head) >> 2;
    const f32x4* pv = reinterpret_cast<const f32x4*>(p + head);
    for (int i = blockIdx.x * 256 + tid; i < nv; i += nb * 256) {
        const f32x4 v = DS_LD(f32x4, pv + i, DS_BX_SRC1);
        mn = fminf(fminf(mn, fminf(v[0], v[1])), fminf(v[2], v[3]));
        mx = fmaxf(fmaxf(mx, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
    }
    if (blockIdx.x == 0 && tid < 8) {
        const int j = tid < 4 ? (tid < head ? tid : -1) : head + 4 * nv + (tid - 4);
        if (j >= 0 && j < n) {
            const float v = DS_LD(float, p + j, DS_BX_SRC1);
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
    }
    block_minmax(mn, mx, red);
    if (tid == 0) {
        float* dst = part + ((size_t)b * nb + blockIdx.x) * 2;
        DS_ST(float, dst, DS_BX_AUX0, mn);
        DS_ST(float, dst + 1, DS_BX_AUX0, mx);
    }
}

// one element of the representation -> the red (= green) bytes of the two images; rr = max(ref, 1e-16) + 1e-16
__device__ __forceinline__ void ui_pixel(float c0, float c1, float c2, float rr, unsigned& sp, unsigned& ph) {
    const float m = expm1f(c0);                                   // the iSTFT kernel's magnitude (tail.hip): sound and picture agree
    const float a = fmaxf(fabsf(m), 1e-16f) + 1e-16f;
    // 10 log10(a) - 10 log10(rr) as ONE logarithm of the correctly rounded quotient: the difference of two fp32 logarithms of up to 37
    // carries 4e-6 of rounding, which is 1e-5 of a grey level; libm logf and an IEEE division, no fast forms
    const float db = fmaxf(4.34294481903251828f * logf(a / rr), -80.0f);
    const int si = (int)(255.0f * ((db + 80.0f) / 80.0f));
    sp = (unsigned)(si > 255 ? 255 : si);
    const float phi = atan2f(m * c2, m * c1);
    ph = (unsigned)(int)(255.0f * ((phi + 1.0f) / 2.0f)) & 255u;  // int32, low byte: the defined form of the reference's wrapping cast
}

// V = 4: T % 4 == 0, enc / amp 16-byte aligned (incl. their batch strides), images 4-byte aligned.  V = 1: anything.
template <int V>
__global__ __launch_bounds__(256) void stft_images_kernel(const float* enc, const float* amp, long long amp_bstride, int F, int T, const float* part,
                                                          int nb, unsigned char* spec, unsigned char* phase) {
    __shared__ __attribute__((aligned(16))) unsigned char sm[2][UI_ROW];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int npix = (F + 1) * T, p0 = blockIdx.x * UI_NP;
    const int np = npix - p0 < UI_NP ? npix - p0 : UI_NP;
    // the clip's reference magnitude from the producer's partials (every wave on its own: no LDS, no barrier)
    float mn = INFINITY, mx = -INFINITY;
    {
        const int lane = tid & 63;
        if (lane < nb) {
            const float* pp = part + ((size_t)b * nb + lane) * 2;
            mn = DS_LD(float, pp, DS_BX_AUX0);
            mx = DS_LD(float, pp + 1, DS_BX_AUX0);
        }
        mn = wave_min(mn);
        mx = wave_max(mx);
    }
    const float ref = fmaxf(fmaxf(expm1f(mx), -expm1f(mn)), 0.0f);    // (0: the implied zero row)
    const float rr = fmaxf(ref, 1e-16f) + 1e-16f;
    const float* e0 = enc + (size_t)b * 3 * F * T;
    const float* a0 = amp ? amp + (size_t)b * amp_bstride : e0;
    const size_t FT = (size_t)F * T;
    unsigned char* const gs = spec + ((size_t)b * npix + p0) * 3;
    unsigned char* const gp = phase + ((size_t)b * npix + p0) * 3;
    const int shs = (int)(reinterpret_cast<uintptr_t>(gs) & 15), shp = (int)(reinterpret_cast<uintptr_t>(gp) & 15);
#pragma unroll
    for (int it = 0; it < UI_NP / (256 * V); ++it) {
        const int q = (it * 256 + tid) * V;                        // first pixel of this thread's run inside the block
        if (q >= np) continue;
        const int p = p0 + q, r = p / T, t = p - r * T;            // image row r = bin F - r; r == F: the implied zero bin
        float c0[V], c1[V], c2[V];
        if (r < F) {
            const size_t o = (size_t)(F - 1 - r) * T + t;
            if constexpr (V == 4) {
                const f32x4 x0 = DS_LD(f32x4, a0 + o, DS_BX_SRC1), x1 = DS_LD(f32x4, e0 + FT + o, DS_BX_SRC0),
                            x2 = DS_LD(f32x4, e0 + 2 * FT + o, DS_BX_SRC0);
#pragma unroll
                for (int k = 0; k < V; ++k) { c0[k] = x0[k]; c1[k] = x1[k]; c2[k] = x2[k]; }
            } else {
                c0[0] = DS_LD(float, a0 + o, DS_BX_SRC1);
                c1[0] = DS_LD(float, e0 + FT + o, DS_BX_SRC0);
                c2[0] = DS_LD(float, e0 + 2 * FT + o, DS_BX_SRC0);
            }
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) { c0[k] = 0.0f; c1[k] = 1.0f; c2[k] = 0.0f; }
        }
        unsigned s[V], h[V];
#pragma unroll
        for (int k = 0; k < V; ++k) ui_pixel(c0[k], c1[k], c2[k], rr, s[k], h[k]);
        if constexpr (V == 4) {
            // twelve bytes R G B R | G B R G | B R G B per image (shs, shp and 3 q are multiples of 4 here)
            unsigned* ws = reinterpret_cast<unsigned*>(sm[0] + shs + 3 * q);
            unsigned* wp = reinterpret_cast<unsigned*>(sm[1] + shp + 3 * q);
            ws[0] = s[0] | (s[0] << 8) | (63u << 16) | (s[1] << 24);
            ws[1] = s[1] | (63u << 8) | (s[2] << 16) | (s[2] << 24);
            ws[2] = 63u | (s[3] << 8) | (s[3] << 16) | (63u << 24);
            wp[0] = h[0] | (h[0] << 8) | (51u << 16) | (h[1] << 24);
            wp[1] = h[1] | (51u << 8) | (h[2] << 16) | (h[2] << 24);
            wp[2] = 51u | (h[3] << 8) | (h[3] << 16) | (51u << 24);
        } else {
            unsigned char* ws = sm[0] + shs + 3 * q;
            unsigned char* wp = sm[1] + shp + 3 * q;
            ws[0] = (unsigned char)s[0]; ws[1] = (unsigned char)s[0]; ws[2] = 63;
            wp[0] = (unsigned char)h[0]; wp[1] = (unsigned char)h[0]; wp[2] = 51;
        }
    }
    __syncthreads();
    // the block's byte range of each image: 16-byte stores between the first and the last 16-byte boundary, single bytes outside
    const int nbytes = 3 * np;
#pragma unroll
    for (int im = 0; im < 2; ++im) {
        unsigned char* const g = im ? gp : gs;
        const unsigned char* const l = sm[im] + (im ? shp : shs);
        const int bx = im ? DS_BX_AUX1 : DS_BX_OUT;
        int head = (16 - (im ? shp : shs)) & 15;
        head = head < nbytes ? head : nbytes;
        const int nv = (nbytes - head) >> 4, tail0 = head + 16 * nv;
        for (int i = tid; i < nv; i += 256)
            DS_ST(u32x4, g + head + 16 * i, bx, *reinterpret_cast<const u32x4*>(l + head + 16 * i));
        if (tid < 32) {
            const int j = tid < 16 ? (tid < head ? tid : -1) : tail0 + (tid - 16);
            if (j >= 0 && j < nbytes) DS_ST(unsigned char, g + j, bx, l[j]);
        }
    }
}

// per (sample, channel) extremes of a latent: one block each.  mm [B * C][2]
__global__ __launch_bounds__(256) void latent_minmax_kernel(const float* lat, int HW, float* mm) {
    __shared__ float red[8];
    const float* p = lat + (size_t)blockIdx.x * HW;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < HW; i += 256) {
        const float v = DS_LD(float, p + i, DS_BX_SRC0);
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    block_minmax(mn, mx, red);
    if (threadIdx.x == 0) {
        DS_ST(float, mm + 2 * (size_t)blockIdx.x, DS_BX_AUX0, mn);
        DS_ST(float, mm + 2 * (size_t)blockIdx.x + 1, DS_BX_AUX0, mx);
    }
}

// thread = one RGBA pixel (one dword store); image row h shows latent row H - 1 - h
__global__ __launch_bounds__(256) void latent_image_kernel(const float* lat, int H, int W, const float* mm, unsigned* img) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, HW = H * W;
    if (i >= HW) return;
    const int h = i / W, w = i - h * W;
    unsigned px = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float mn = DS_LD(float, mm + ((size_t)b * 4 + c) * 2, DS_BX_AUX0), mx = DS_LD(float, mm + ((size_t)b * 4 + c) * 2 + 1, DS_BX_AUX0);
        const float x = DS_LD(float, lat + ((size_t)b * 4 + c) * HW + (size_t)(H - 1 - h) * W + w, DS_BX_SRC0);
        // the reference's order, every step rounded to fp32: subtract, divide (IEEE), multiply.  0 / 0 (a constant channel) -> 0
        const float v = __fmul_rn(__fdiv_rn(__fsub_rn(x, mn), __fsub_rn(mx, mn)), 255.0f);
        const int iv = v == v ? (int)v : 0;
        px |= ((unsigned)iv & 255u) << (8 * c);
    }
    DS_ST(unsigned, img + (size_t)b * HW + i, DS_BX_OUT, px);
}

}  // namespace

extern "C" size_t ds_stft_images_ws_floats(int B, int F, int T) {
    if (B <= 0 || F <= 0 || T <= 0) return 0;
    return (size_t)B * ui_mm_blocks((long long)F * T) * 2;
}

extern "C" int ds_stft_images(const float* enc, const float* amp, long long amp_batch_stride, int B, int F, int T, float* ws, unsigned char* spec_img,
                              unsigned char* phase_img, void* stream) {
    DS_REQUIRE(enc && ws && spec_img && phase_img && B > 0 && F > 0 && T > 0, "stft_images: bad args (B=%d F=%d T=%d)", B, F, T);
    DS_REQUIRE(B <= 65535, "stft_images: at most 65535 clips per call (got %d)", B);
    DS_REQUIRE(((long long)F + 1) * T * 3 < (1ll << 31), "stft_images: one image must stay below 2^31 bytes (F=%d T=%d)", F, T);
    DS_REQUIRE(!amp || B == 1 || amp_batch_stride >= (long long)F * T, "stft_images: amp_batch_stride %lld is smaller than F*T", amp_batch_stride);
    if ((reinterpret_cast<uintptr_t>(enc) & 3) || (reinterpret_cast<uintptr_t>(amp) & 3) || (reinterpret_cast<uintptr_t>(ws) & 3))
        DS_FAIL(DS_EALIGN, "stft_images: enc / amp / ws must be 4-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long FT = (long long)F * T;
    const int nb = ui_mm_blocks(FT);
    const float* mag = amp ? amp : enc;
    const long long mstride = amp ? amp_batch_stride : 3 * FT;
    const int npix = (F + 1) * T;
#if DS_BOUNDS
    {   // ONE table for both launches (the extremes kernel reads its source as DS_BX_SRC1, like the image kernel's magnitude channel): with a
        // table per launch, published between the two launches of one call, the image kernel was seen checking against the first table
        DsBxHost h(DS_K_STFT_IMAGES);
        h.set(DS_BX_SRC0, enc, (long long)B * 3 * FT * 4);
        h.set(DS_BX_SRC1, mag, ((B - 1) * mstride + FT) * 4);
        h.set(DS_BX_AUX0, ws, (long long)B * nb * 8);
        h.set(DS_BX_OUT, spec_img, (long long)B * npix * 3);
        h.set(DS_BX_AUX1, phase_img, (long long)B * npix * 3);
        h.publish(st);
    }
#endif
    hipLaunchKernelGGL(ui_minmax_kernel, dim3(nb, B), dim3(256), 0, st, mag, mstride, (int)FT, nb, ws);
    DS_CHECK_LAUNCH("stft_images (extremes)");
    const bool vec = T % 4 == 0 && ds_aligned16(enc) && (!amp || (ds_aligned16(amp) && amp_batch_stride % 4 == 0)) &&
                     !(reinterpret_cast<uintptr_t>(spec_img) & 3) && !(reinterpret_cast<uintptr_t>(phase_img) & 3);
    const dim3 grid((npix + UI_NP - 1) / UI_NP, B);
    if (vec) hipLaunchKernelGGL(stft_images_kernel<4>, grid, dim3(256), 0, st, enc, amp, amp_batch_stride, F, T, ws, nb, spec_img, phase_img);
    else hipLaunchKernelGGL(stft_images_kernel<1>, grid, dim3(256), 0, st, enc, amp, amp_batch_stride, F, T, ws, nb, spec_img, phase_img);
    DS_CHECK_LAUNCH("stft_images");
    return DS_OK;
}

extern "C" size_t ds_latent_image_ws_floats(int B, int C) { return B > 0 && C > 0 ? (size_t)B * C * 2 : 0; }

extern "C" int ds_latent_image(const float* lat, int B, int C, int H, int W, float* ws, unsigned char* img, void* stream) {
    DS_REQUIRE(lat && ws && img && B > 0 && H > 0 && W > 0, "latent_image: bad args (B=%d H=%d W=%d)", B, H, W);
    DS_REQUIRE(C == 4, "latent_image: %d channels unsupported (the image is RGBA: 4 only)", C);
    DS_REQUIRE(B <= 16383, "latent_image: at most 16383 latents per call (got %d)", B);
    DS_REQUIRE((long long)H * W < (1ll << 29), "latent_image: H * W must stay below 2^29");
    if ((reinterpret_cast<uintptr_t>(lat) & 3) || (reinterpret_cast<uintptr_t>(ws) & 3) || (reinterpret_cast<uintptr_t>(img) & 3))
        DS_FAIL(DS_EALIGN, "latent_image: lat / ws / img must be 4-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int HW = H * W;
#if DS_BOUNDS
    {
        DsBxHost h(DS_K_LATENT_IMAGE);
        h.set(DS_BX_SRC0, lat, (long long)B * 4 * HW * 4);
        h.set(DS_BX_AUX0, ws, (long long)B * 4 * 8);
        h.set(DS_BX_OUT, img, (long long)B * HW * 4);
        h.publish(st);
    }
#endif
    hipLaunchKernelGGL(latent_minmax_kernel, dim3(B * 4), dim3(256), 0, st, lat, HW, ws);
    DS_CHECK_LAUNCH("latent_image (extremes)");
    hipLaunchKernelGGL(latent_image_kernel, dim3((HW + 255) / 256, B), dim3(256), 0, st, lat, H, W, ws, reinterpret_cast<unsigned*>(img));
    DS_CHECK_LAUNCH("latent_image");
    return DS_OK;
}

#if DS_BOUNDS
extern "C" int ds_bounds_fetch_ui_images(ds_bounds_rec* out, int reset) { return ds_bounds_fetch_tu(out, reset); }
#endif
