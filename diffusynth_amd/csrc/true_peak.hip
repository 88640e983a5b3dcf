// True peak (BS.1770 Annex 2: 4x oversampling) of a ragged batch of mono signals (gfx950): the largest magnitude of the interpolated
// waveform per signal and, where asked for, its envelope per sample, the detector of ds_master_limit_tp.  fp32 samples, float64 sums;
// definition and table layout in include/diffusynth_hip.h ("true peak").
//
// ds_true_peak  block = one tile of DS_TP_TILE samples of one signal, [t0, t0 + tn):
//               sx[j]  = x[t0 - 6 + j], j < tn + 12 (lanes read consecutive words; zero outside the signal);
//               siv[m] = fp32(iv(t0 - 1 + m)), m <= tn: the three phases of 12 taps each out of sx[m .. m + 11] (consecutive lanes,
//                        consecutive words: no bank conflict), float64 multiply then add in ascending tap order, the 36 coefficients in
//                        scalar registers (a kernel argument);
//               one barrier;  e[t0 + i] = max(|sx[i + 6]|, siv[i], siv[i + 1]), the store where env is given, the block's maximum -> one
//               fp32 partial in ws.  A second kernel, one block per signal, takes the maximum of the partials.
//               A maximum has no order and the rounding to fp32 is monotone: the bits are the definition's, alone and in any batch.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int TP_T = 256;                                   // threads per block
constexpr int TILE = DS_TP_TILE, TAPS = DS_TP_TAPS, PH = DS_TP_PHASES;
constexpr int TP_NQ = (TILE + 1 + TP_T - 1) / TP_T;         // iv values a thread computes, at most
static_assert(TAPS == 12 && PH == 3 && DS_TP_NCOEF == PH * TAPS, "three phases of twelve taps");
static_assert(TILE % TP_T == 0 && 4 * (TILE + TAPS) + 4 * (TILE + 1) <= 64 * 1024, "the two tiles fit the default LDS");

struct TpCoef {
    float h[DS_TP_NCOEF];
};
struct TpRow {
    int xoff, len;
};
__device__ __forceinline__ TpRow tp_row(const int32_t* tab, int s) {
    const int32_t* r = tab + (size_t)s * DS_PV_NI;
    TpRow o;
    o.xoff = DS_LD(int32_t, r + DS_PV_XOFF, DS_BX_AUX0);
    o.len = DS_LD(int32_t, r + DS_PV_LEN, DS_BX_AUX0);
    return o;
}
// a signal [off, off + n) of legal length (at most the launch's max_len: the workspace is laid out for it) inside a buffer of `total` elements
__device__ __forceinline__ bool fits(const TpRow& r, long long total, int max_len) {
    return r.xoff >= 0 && r.len >= 1 && r.len <= max_len && (long long)r.xoff + r.len <= total;
}
__host__ __device__ inline int tp_tiles(int n) { return (n + TILE - 1) / TILE; }

__global__ __launch_bounds__(TP_T) void true_peak_kernel(const float* x, const int32_t* tab, long long total_samples, int max_len, const TpCoef K, int stride,
                                                         float* env, float* part) {
    __shared__ float sx[TILE + TAPS];
    __shared__ float siv[TILE + 1];
    __shared__ float rmax[TP_T / 64];
    const int s = blockIdx.y, tid = threadIdx.x;
    const TpRow row = tp_row(tab, s);
    if (!fits(row, total_samples, max_len)) return;
    if ((int)blockIdx.x >= tp_tiles(row.len)) return;
    const int t0 = blockIdx.x * TILE;                            // < len <= 2^24
    const int tn = row.len - t0 < TILE ? row.len - t0 : TILE;    // this block owns [t0, t0 + tn)
    const float* xg = x + row.xoff;
    for (int j = tid; j < tn + TAPS; j += TP_T) {
        const int n = t0 - 6 + j;
        sx[j] = n >= 0 && n < row.len ? DS_LD(float, xg + n, DS_BX_SRC0) : 0.0f;
    }
    __syncthreads();
#pragma unroll 1
    for (int q = 0; q < TP_NQ; ++q) {
        const int m = tid + q * TP_T;                            // iv(t0 - 1 + m)
        if (m <= tn) {
            double xs[TAPS];
#pragma unroll
            for (int k = 0; k < TAPS; ++k) xs[k] = (double)sx[m + k];
            double iv = 0.0;
#pragma unroll
            for (int p = 0; p < PH; ++p) {
                double acc = (double)K.h[p * TAPS] * xs[0];
#pragma unroll
                for (int k = 1; k < TAPS; ++k) acc = acc + (double)K.h[p * TAPS + k] * xs[k];
                acc = fabs(acc);
                iv = acc > iv ? acc : iv;
            }
            siv[m] = (float)iv;
        }
    }
    __syncthreads();
    float mx = 0.f;
    for (int i = tid; i < tn; i += TP_T) {
        const float e = fmaxf(fabsf(sx[i + 6]), fmaxf(siv[i], siv[i + 1]));
        if (env) DS_ST(float, env + row.xoff + t0 + i, DS_BX_OUT, e);
        mx = fmaxf(mx, e);
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) rmax[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) DS_ST(float, part + (size_t)s * stride + blockIdx.x, DS_BX_AUX1, fmaxf(fmaxf(rmax[0], rmax[1]), fmaxf(rmax[2], rmax[3])));
}

__global__ __launch_bounds__(TP_T) void true_peak_finish_kernel(const int32_t* tab, long long total_samples, int max_len, int stride, const float* part, float* tp) {
    __shared__ float rmax[TP_T / 64];
    const int s = blockIdx.x, tid = threadIdx.x;
    const TpRow row = tp_row(tab, s);
    if (!fits(row, total_samples, max_len)) return;
    const int nb = tp_tiles(row.len);
    float mx = 0.f;
    for (int j = tid; j < nb; j += TP_T) mx = fmaxf(mx, DS_LD(float, part + (size_t)s * stride + j, DS_BX_AUX1));
    mx = wave_max(mx);
    if ((tid & 63) == 0) rmax[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) DS_ST(float, tp + s, DS_BX_RES, fmaxf(fmaxf(rmax[0], rmax[1]), fmaxf(rmax[2], rmax[3])));
}

inline bool al(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
constexpr long long MAX_ELEMS = (1ll << 31) - 1 - TILE;         // the table's offsets are int32, and t0 + i must not wrap

}  // namespace

extern "C" size_t ds_true_peak_ws_bytes(int n_signals, int max_len) {
    return n_signals > 0 && max_len > 0 && max_len <= DS_MS_MAX_LEN ? (size_t)n_signals * tp_tiles(max_len) * 4 : 0;
}

extern "C" int ds_true_peak(const float* x, const int32_t* tab, int n_signals, int max_len, long long total_samples, const float* coef, float* env, void* ws,
                            float* tp, void* stream) {
    DS_REQUIRE(x && tab && coef && ws && tp && n_signals > 0 && max_len > 0 && total_samples > 0,
               "true_peak: bad args (n_signals=%d max_len=%d total_samples=%lld)", n_signals, max_len, total_samples);
    DS_REQUIRE(n_signals <= 65535 && max_len <= DS_MS_MAX_LEN && total_samples <= MAX_ELEMS,
               "true_peak: at most 65535 signals of %d samples and 2^31 - 1 - %d samples in all", DS_MS_MAX_LEN, TILE);
    DS_REQUIRE((const void*)env != (const void*)x, "true_peak: env may not be x (a tile reads its neighbours' inputs)");
    if (!al(x, 4) || !al(tab, 4) || !al(coef, 4) || !al(env, 4) || !al(ws, 4) || !al(tp, 4)) DS_FAIL(DS_EALIGN, "true_peak: x / tab / coef / env / ws / tp 4-byte aligned");
    TpCoef K;
    for (int i = 0; i < DS_TP_NCOEF; ++i) {
        K.h[i] = coef[i];
        DS_REQUIRE(K.h[i] - K.h[i] == 0.0f, "true_peak: coef[%d] is not finite", i);
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int stride = tp_tiles(max_len);
    float* part = reinterpret_cast<float*>(ws);
#if DS_BOUNDS
    {
        DsBxHost h(DS_K_TRUE_PEAK);
        h.set(DS_BX_SRC0, x, total_samples * 4);
        h.set(DS_BX_AUX0, tab, (long long)n_signals * DS_PV_NI * 4);
        h.set(DS_BX_AUX1, part, (long long)n_signals * stride * 4);
        h.set(DS_BX_OUT, env, total_samples * 4);
        h.set(DS_BX_RES, tp, (long long)n_signals * 4);
        h.publish(st);
    }
#endif
    hipLaunchKernelGGL(true_peak_kernel, dim3(stride, n_signals), dim3(TP_T), 0, st, x, tab, total_samples, max_len, K, stride, env, part);
    DS_CHECK_LAUNCH("true_peak (tiles)");
    hipLaunchKernelGGL(true_peak_finish_kernel, dim3(n_signals), dim3(TP_T), 0, st, tab, total_samples, max_len, stride, part, tp);
    DS_CHECK_LAUNCH("true_peak");
    return DS_OK;
}

#if DS_BOUNDS
extern "C" int ds_bounds_fetch_true_peak(ds_bounds_rec* out, int reset) { return ds_bounds_fetch_tu(out, reset); }
#endif
