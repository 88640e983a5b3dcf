// The Inpaint tab's latent mask for a ragged batch of masks (gfx950): what webUI/natural_language_guided_4/inpaint_with_text.py:204-233 does
// with numpy and scipy.ndimage.zoom — layers -> binary plane -> cubic B-spline prefilter -> 4 x 4 taps, rounding, clip, rectangle, inversion,
// flip.  Definition and table layout in include/diffusynth_hip.h; float64 wherever scipy is float64.
//
// A mask is one row of a device table (int32 [n][DS_IM_NI]); blockIdx.y (blockIdx.z in the prefilter) is the mask, the other grid dimensions
// are sized for the largest mask of the batch and a block beyond its own mask's extent returns.
//
// ds_mask_layers     thread = 4 consecutive pixels of the flat plane: one 16-byte load per layer, OR, alpha byte of each pixel != 0, one
//                    4-byte store.  A mask whose offsets or size are no multiple of 4 pixels takes single-pixel accesses.
// ds_mask_prefilter  two launches.  Both cut a line into segments of IM_SEG samples, one thread each: the causal recursion from zero over
//                    IM_RUN mirror-extended samples of run-in, the segment (its c+ kept in registers: the loops are unrolled) and IM_RUN
//                    samples behind it, which also accumulate the start value of the anticausal recursion; then that recursion down the
//                    registers.  A segment that reaches beyond the line's end runs on over the mirror extension (the solution on the
//                    extended line is mirror-symmetric too) and does not store those samples.
//                      axis 0: lane = column, so a wave reads and writes 64 consecutive elements of a row at every step: coalesced as it is,
//                              no staging.  Block = 64 columns x 4 segments (one per wave).
//                      axis 1: lane = row would walk global memory with a stride of W.  Block = 32 rows x 128 columns: the tile and IM_RUN
//                              columns on either side go to LDS with consecutive threads on consecutive columns, thread (row r, segment s)
//                              walks LDS row r, the results go back into the tile (after a barrier: a segment's samples are its
//                              neighbours' run-in) and out again coalesced.  Row pitch 209 float64: the 32 lanes of a ds_read_b64 group are
//                              32 rows at one column, 418 r mod 64 = 34 r mod 64 — 32 different even banks.
// ds_mask_zoom       thread = one output pixel: tap indices and weights of both axes in float64, 16 coefficient loads, rounding half away
//                    from zero (0 for an output whose coordinate is outside the input), clip, rectangle, inversion, one fp32 store at the
//                    flipped row (and the float64 value for the tests).
// No atomics; a mask's result does not depend on what else is in the launch.
#include "common.hpp"

namespace {

constexpr int IM_T = 256;                                // threads per block
constexpr int IM_SEG = 16;                               // samples per thread of the prefilter (32 VGPRs of c+)
constexpr int IM_RUN = DS_IM_RUN_IN;                     // run-in and run-out: |z|^40 = (0.26795)^40 = 1.3e-23, far below float64's 1.1e-16
constexpr double IM_Z = -0.26794919243112270647;         // sqrt(3) - 2, the cubic B-spline's pole
constexpr int IM_ROWS = 32, IM_COLS = 128;               // axis 1: tile of a block (IM_COLS / IM_SEG = 8 segments x 32 rows = 256 threads)
constexpr int IM_TW = IM_COLS + 2 * IM_RUN;              // its staged width
constexpr int IM_PITCH = IM_TW + 1;                      // odd: see the bank arithmetic above
static_assert(IM_ROWS * (IM_COLS / IM_SEG) == IM_T && (IM_PITCH & 1) == 1, "axis-1 block geometry");

struct ImRow {
    int loff, nl, poff, h, w, ooff, ho, wo, r0, r1, c0, c1, inv;
};
__device__ __forceinline__ ImRow im_row(const int32_t* tab, int s) {
    const int32_t* r = tab + (size_t)s * DS_IM_NI;
    ImRow o;
    o.loff = DS_LD(int32_t, r + DS_IM_LOFF, DS_BX_AUX0);
    o.nl = DS_LD(int32_t, r + DS_IM_NL, DS_BX_AUX0);
    o.poff = DS_LD(int32_t, r + DS_IM_POFF, DS_BX_AUX0);
    o.h = DS_LD(int32_t, r + DS_IM_H, DS_BX_AUX0);
    o.w = DS_LD(int32_t, r + DS_IM_W, DS_BX_AUX0);
    o.ooff = DS_LD(int32_t, r + DS_IM_OOFF, DS_BX_AUX0);
    o.ho = DS_LD(int32_t, r + DS_IM_HO, DS_BX_AUX0);
    o.wo = DS_LD(int32_t, r + DS_IM_WO, DS_BX_AUX0);
    o.r0 = DS_LD(int32_t, r + DS_IM_R0, DS_BX_AUX0);
    o.r1 = DS_LD(int32_t, r + DS_IM_R1, DS_BX_AUX0);
    o.c0 = DS_LD(int32_t, r + DS_IM_C0, DS_BX_AUX0);
    o.c1 = DS_LD(int32_t, r + DS_IM_C1, DS_BX_AUX0);
    o.inv = DS_LD(int32_t, r + DS_IM_INV, DS_BX_AUX0);
    return o;
}
// a plane of h x w >= 2 x 2 elements at off inside a buffer of `total`
__device__ __forceinline__ bool im_fits(int off, int h, int w, long long total) {
    return off >= 0 && h >= 2 && w >= 2 && (long long)h * w <= 0x7fffffffll && (long long)off + (long long)h * w <= total;
}
// whole-sample mirror of any index into [0, n - 1], n >= 2: -1 -> 1, n -> n - 2, period 2 (n - 1)
__device__ __forceinline__ int im_mirror(int j, int n) {
    const int p = 2 * (n - 1);
    int m = j % p;
    m = m < 0 ? m + p : m;
    return m > n - 1 ? p - m : m;
}

// ---------------------------------------------------------------------------------------------------- layers -> binary plane
__global__ __launch_bounds__(IM_T) void mask_layers_kernel(const uint8_t* layers, const int32_t* tab, long long total_layer_px, long long total_px,
                                                           uint8_t* planes) {
    const ImRow r = im_row(tab, blockIdx.y);
    if (r.nl < 1 || !im_fits(r.poff, r.h, r.w, total_px)) return;
    const long long hw = (long long)r.h * r.w;
    if (r.loff < 0 || (long long)r.loff + hw * r.nl > total_layer_px) return;
    const long long p0 = ((long long)blockIdx.x * IM_T + threadIdx.x) * 4;
    if (p0 >= hw) return;
    const uint8_t* src = layers + ((long long)r.loff + p0) * 4;
    uint8_t* dst = planes + r.poff + p0;
    if (((r.loff | r.poff) & 3) == 0 && (hw & 3) == 0) {
        u32x4 a = {0u, 0u, 0u, 0u};
        for (int l = 0; l < r.nl; ++l) a |= DS_LD(u32x4, src + (long long)l * hw * 4, DS_BX_SRC0);
        // (alpha is byte 3 of a pixel: the top byte of its little-endian dword)
        const unsigned v = (a[0] >> 24 ? 1u : 0u) | (a[1] >> 24 ? 0x100u : 0u) | (a[2] >> 24 ? 0x10000u : 0u) | (a[3] >> 24 ? 0x1000000u : 0u);
        DS_ST(unsigned, dst, DS_BX_OUT, v);
    } else {
        for (int k = 0; k < 4 && p0 + k < hw; ++k) {
            unsigned a = 0;
            for (int l = 0; l < r.nl; ++l) a |= DS_LD(uint8_t, src + ((long long)l * hw + k) * 4 + 3, DS_BX_SRC0);
            DS_ST(uint8_t, dst + k, DS_BX_OUT, (uint8_t)(a ? 1 : 0));
        }
    }
}

// ---------------------------------------------------------------------------------------------------- prefilter
// The segment [s0, s0 + IM_SEG) of the line e (any index: the caller mirrors; e returns the sample times the gain): c[i] = coefficient s0 + i.
template <class Line>
__device__ __forceinline__ void im_segment(Line e, int s0, double (&c)[IM_SEG]) {
    double cp = 0.0;
    for (int j = s0 - IM_RUN; j < s0; ++j) cp = fma(IM_Z, cp, e(j));
#pragma unroll
    for (int i = 0; i < IM_SEG; ++i) {
        cp = fma(IM_Z, cp, e(s0 + i));
        c[i] = cp;
    }
    double acc = 0.0, zp = IM_Z;                         // c[s1] = -sum_k z^(k+1) c+[s1 + k]
    for (int j = s0 + IM_SEG; j < s0 + IM_SEG + IM_RUN; ++j) {
        cp = fma(IM_Z, cp, e(j));
        acc = fma(-zp, cp, acc);
        zp *= IM_Z;
    }
#pragma unroll
    for (int i = IM_SEG - 1; i >= 0; --i) {
        acc = IM_Z * (acc - c[i]);
        c[i] = acc;
    }
}

// axis 0: thread = (column, segment of rows); planes -> ws0
__global__ __launch_bounds__(IM_T) void mask_prefilter_rows_kernel(const uint8_t* planes, const int32_t* tab, long long total_px, double* ws0) {
    const ImRow r = im_row(tab, blockIdx.z);
    if (!im_fits(r.poff, r.h, r.w, total_px)) return;
    const int col = blockIdx.x * 64 + (threadIdx.x & 63);
    const int s0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * IM_SEG;
    if (col >= r.w || s0 >= r.h) return;
    const uint8_t* x = planes + r.poff + col;
    double c[IM_SEG];
    im_segment([&](int j) { return 6.0 * (double)DS_LD(uint8_t, x + (long long)im_mirror(j, r.h) * r.w, DS_BX_SRC0); }, s0, c);
    double* o = ws0 + r.poff + (long long)s0 * r.w + col;
#pragma unroll
    for (int i = 0; i < IM_SEG; ++i)
        if (s0 + i < r.h) DS_ST(double, o + (long long)i * r.w, DS_BX_AUX1, c[i]);
}

// axis 1: block = IM_ROWS rows x IM_COLS columns through LDS; ws0 -> ws1
__global__ __launch_bounds__(IM_T) void mask_prefilter_cols_kernel(const double* ws0, const int32_t* tab, long long total_px, double* ws1) {
    __shared__ double tile[IM_ROWS * IM_PITCH];
    const ImRow r = im_row(tab, blockIdx.z);
    if (!im_fits(r.poff, r.h, r.w, total_px)) return;                  // (uniform for the block, as is the next line: no barrier is skipped by some)
    const int h0 = blockIdx.y * IM_ROWS, c0 = blockIdx.x * IM_COLS, tid = threadIdx.x;
    if (h0 >= r.h || c0 >= r.w) return;
    const double* src = ws0 + r.poff;
    for (int i = tid; i < IM_ROWS * IM_TW; i += IM_T) {
        const int rr = i / IM_TW, jj = i - rr * IM_TW;
        if (h0 + rr < r.h) tile[rr * IM_PITCH + jj] = DS_LD(double, src + (long long)(h0 + rr) * r.w + im_mirror(c0 - IM_RUN + jj, r.w), DS_BX_AUX1);
    }
    __syncthreads();
    const int row = tid & (IM_ROWS - 1), seg = tid / IM_ROWS;
    const bool mine = h0 + row < r.h && c0 + seg * IM_SEG < r.w;
    double c[IM_SEG];
    const double* line = tile + row * IM_PITCH + IM_RUN;                // line[k]: column c0 + k, k in [-IM_RUN, IM_COLS + IM_RUN)
    if (mine) im_segment([&](int k) { return 6.0 * line[k]; }, seg * IM_SEG, c);
    __syncthreads();
    if (mine) {
#pragma unroll
        for (int i = 0; i < IM_SEG; ++i) tile[row * IM_PITCH + IM_RUN + seg * IM_SEG + i] = c[i];
    }
    __syncthreads();
    double* dst = ws1 + r.poff;
    for (int i = tid; i < IM_ROWS * IM_COLS; i += IM_T) {
        const int rr = i / IM_COLS, jj = i - rr * IM_COLS;
        if (h0 + rr < r.h && c0 + jj < r.w) DS_ST(double, dst + (long long)(h0 + rr) * r.w + c0 + jj, DS_BX_AUX2, tile[rr * IM_PITCH + IM_RUN + jj]);
    }
}

// ---------------------------------------------------------------------------------------------------- taps, rounding, rectangle, flip
// the 4 taps of output i of an axis zoomed from n to n_out samples: mirrored indices and cubic B-spline weights.  Returns whether the
// coordinate lies inside the input: scipy's mode "constant" gives cval = 0 for x < 0 or x > n - 1, and for about one n in ten (30, 63, 120,
// 252, 416 ...) the LAST output's product rounds an ulp above n - 1 — the same comparison on the same float64 product as scipy's
__device__ __forceinline__ bool im_taps(int i, int n, int n_out, int (&idx)[4], double (&w)[4]) {
    const double x = (double)i * ((double)(n - 1) / (double)(n_out - 1));
    const int f = (int)floor(x);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int k = f - 1 + a;
        const double t = fabs(x - (double)k);
        w[a] = t < 1.0 ? 2.0 / 3.0 - t * t + t * t * t / 2.0 : (t < 2.0 ? (2.0 - t) * (2.0 - t) * (2.0 - t) / 6.0 : 0.0);
        idx[a] = im_mirror(k, n);
    }
    return !(x < 0.0 || x > (double)(n - 1));
}

__global__ __launch_bounds__(IM_T) void mask_zoom_kernel(const double* coef, const int32_t* tab, long long total_px, long long total_out, float* out,
                                                         double* pre) {
    const ImRow r = im_row(tab, blockIdx.y);
    if (!im_fits(r.poff, r.h, r.w, total_px) || !im_fits(r.ooff, r.ho, r.wo, total_out)) return;
    const long long p = (long long)blockIdx.x * IM_T + threadIdx.x;
    if (p >= (long long)r.ho * r.wo) return;
    const int i = (int)(p / r.wo), j = (int)(p - (long long)i * r.wo);
    int ih[4], iw[4];
    double wh[4], ww[4];
    const bool in_h = im_taps(i, r.h, r.ho, ih, wh), in_w = im_taps(j, r.w, r.wo, iw, ww);
    const double* c = coef + r.poff;
    double v = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) s = fma(ww[b], DS_LD(double, c + (long long)ih[a] * r.w + iw[b], DS_BX_AUX2), s);
        v = fma(wh[a], s, v);
    }
    if (!(in_h && in_w)) v = 0.0;                                      // outside the input on either axis: cval
    if (pre) DS_ST(double, pre + r.ooff + p, DS_BX_AUX3, v);
    double m = v > 0.0 ? floor(v + 0.5) : ceil(v - 0.5);               // scipy's float64 -> int64 output
    m = m < 0.0 ? 0.0 : (m > 1.0 ? 1.0 : m);                            // np.clip(.., 0, 1)
    if (i >= r.r0 && i < r.r1 && j >= r.c0 && j < r.c1) m = 1.0;
    if (r.inv) m = 1.0 - m;
    DS_ST(float, out + r.ooff + (long long)(r.ho - 1 - i) * r.wo + j, DS_BX_OUT, (float)m);
}

inline bool im_al(const void* p, int a) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(a - 1)) == 0; }
constexpr long long IM_MAX_ELEMS = (1ll << 31) - 1 - 4 * IM_T;      // the table's offsets are int32

}  // namespace

extern "C" int ds_mask_layers(const uint8_t* layers, const int32_t* tab, int n_masks, int max_px, long long total_layer_px, long long total_px,
                              uint8_t* planes, void* stream) {
    DS_REQUIRE(layers && tab && planes && n_masks > 0 && max_px >= 4 && total_layer_px > 0 && total_px > 0,
               "mask_layers: bad args (n_masks=%d max_px=%d total_layer_px=%lld total_px=%lld)", n_masks, max_px, total_layer_px, total_px);
    DS_REQUIRE(n_masks <= 65535 && total_layer_px <= IM_MAX_ELEMS && total_px <= IM_MAX_ELEMS, "mask_layers: at most 65535 masks and %lld pixels per buffer",
               IM_MAX_ELEMS);
    if (!im_al(layers, 16) || !im_al(planes, 4) || !im_al(tab, 4)) DS_FAIL(DS_EALIGN, "mask_layers: layers must be 16-byte, planes and tab 4-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#if DS_BOUNDS
    {
        DsBxHost h(DS_K_MASK_LAYERS);
        h.set(DS_BX_SRC0, layers, total_layer_px * 4);
        h.set(DS_BX_AUX0, tab, (long long)n_masks * DS_IM_NI * 4);
        h.set(DS_BX_OUT, planes, total_px);
        h.publish(st);
    }
#endif
    hipLaunchKernelGGL(mask_layers_kernel, dim3((max_px + 4 * IM_T - 1) / (4 * IM_T), n_masks), dim3(IM_T), 0, st, layers, tab, total_layer_px, total_px, planes);
    DS_CHECK_LAUNCH("mask_layers");
    return DS_OK;
}

extern "C" size_t ds_mask_ws_bytes(long long total_px) { return total_px > 0 ? (size_t)total_px * 2 * sizeof(double) : 0; }

extern "C" int ds_mask_prefilter(const uint8_t* planes, const int32_t* tab, int n_masks, int max_h, int max_w, long long total_px, double* ws,
                                 void* stream) {
    DS_REQUIRE(planes && tab && ws && n_masks > 0 && max_h >= 2 && max_w >= 2 && total_px > 0, "mask_prefilter: bad args (n_masks=%d max_h=%d max_w=%d total_px=%lld)",
               n_masks, max_h, max_w, total_px);
    DS_REQUIRE(n_masks <= 65535 && total_px <= IM_MAX_ELEMS && max_h <= (1 << 20) && max_w <= (1 << 20),
               "mask_prefilter: at most 65535 masks, 2^20 samples per axis and %lld pixels", IM_MAX_ELEMS);
    if (!im_al(ws, 8) || !im_al(tab, 4)) DS_FAIL(DS_EALIGN, "mask_prefilter: ws must be 8-byte, tab 4-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#if DS_BOUNDS
    {
        DsBxHost h(DS_K_MASK_PREFILTER);
        h.set(DS_BX_SRC0, planes, total_px);
        h.set(DS_BX_AUX0, tab, (long long)n_masks * DS_IM_NI * 4);
        h.set(DS_BX_AUX1, ws, total_px * 8);
        h.set(DS_BX_AUX2, ws + total_px, total_px * 8);
        h.publish(st);
    }
#endif
    hipLaunchKernelGGL(mask_prefilter_rows_kernel, dim3((max_w + 63) / 64, (max_h + 4 * IM_SEG - 1) / (4 * IM_SEG), n_masks), dim3(IM_T), 0, st, planes, tab,
                       total_px, ws);
    DS_CHECK_LAUNCH("mask_prefilter (axis 0)");
    hipLaunchKernelGGL(mask_prefilter_cols_kernel, dim3((max_w + IM_COLS - 1) / IM_COLS, (max_h + IM_ROWS - 1) / IM_ROWS, n_masks), dim3(IM_T), 0, st, ws, tab,
                       total_px, ws + total_px);
    DS_CHECK_LAUNCH("mask_prefilter (axis 1)");
    return DS_OK;
}

extern "C" int ds_mask_zoom(const double* ws, const int32_t* tab, int n_masks, int max_out_px, long long total_px, long long total_out, float* out,
                            double* pre, void* stream) {
    DS_REQUIRE(ws && tab && out && n_masks > 0 && max_out_px >= 4 && total_px > 0 && total_out > 0,
               "mask_zoom: bad args (n_masks=%d max_out_px=%d total_px=%lld total_out=%lld)", n_masks, max_out_px, total_px, total_out);
    DS_REQUIRE(n_masks <= 65535 && total_px <= IM_MAX_ELEMS && total_out <= IM_MAX_ELEMS, "mask_zoom: at most 65535 masks and %lld elements per buffer", IM_MAX_ELEMS);
    if (!im_al(ws, 8) || !im_al(pre, 8) || !im_al(out, 4) || !im_al(tab, 4)) DS_FAIL(DS_EALIGN, "mask_zoom: ws and pre must be 8-byte, out and tab 4-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#if DS_BOUNDS
    {
        DsBxHost h(DS_K_MASK_ZOOM);
        h.set(DS_BX_AUX0, tab, (long long)n_masks * DS_IM_NI * 4);
        h.set(DS_BX_AUX2, ws + total_px, total_px * 8);
        h.set(DS_BX_OUT, out, total_out * 4);
        h.set(DS_BX_AUX3, pre, total_out * 8);
        h.publish(st);
    }
#endif
    hipLaunchKernelGGL(mask_zoom_kernel, dim3((max_out_px + IM_T - 1) / IM_T, n_masks), dim3(IM_T), 0, st, ws + total_px, tab, total_px, total_out, out, pre);
    DS_CHECK_LAUNCH("mask_zoom");
    return DS_OK;
}

#if DS_BOUNDS
extern "C" int ds_bounds_fetch_inpaint_mask(ds_bounds_rec* out, int reset) { return ds_bounds_fetch_tu(out, reset); }
#endif
