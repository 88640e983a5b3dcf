// Pitch detection for the arranger's tuned mode (gfx950): YIN (de Cheveigne & Kawahara, JASA 111(4), 2002) per frame of a ragged batch of
// signals, then the lower median of each signal's voiced periods.  fp32; semantics and table layout in include/diffusynth_hip.h.
//
// ds_yin_frames   one block of 256 threads per (frame, signal).  The frame's W + tau_max samples are staged once in LDS (12 KB at the largest
//                 W = 2048, tau_max = 1024; 5 KB at the defaults).  Lane t owns tau = t, t + 256, ...: per j it reads s[j] (one address for the
//                 wave: a broadcast) and s[j + tau] (consecutive addresses: conflict-free) and adds the squared DIFFERENCE (energies minus
//                 correlation cancels where the frame is periodic, which is where the answer lies) into accumulator j mod 4; the four are
//                 summed as (a0 + a1) + (a2 + a3).  The running sum of d is one lane's walk over <= 1024 LDS entries (k order: the scan's
//                 order is part of the result), c(tau) is computed by all lanes, the first tau under the threshold is an integer
//                 min-reduction, and one lane walks down the dip and fits the parabola.
// ds_pitch_median one block per signal: the periods go to LDS (unvoiced ones as +inf), the voiced count is an integer reduction, and every
//                 voiced element counts the elements in front of it in (value, index) order; the one whose count is the rank writes itself.
//                 Exact selection: the result is one of the inputs.  O(NF^2) compares, NF <= 8192 (a note has ~100 - 300 frames).
// No atomics, no float reductions across lanes: every output has one owner and one summation order, whatever else is in the batch.
#include <limits.h>
#include <math.h>

#include "common.hpp"

namespace {

constexpr int YT = 256;                                  // threads per block, both kernels
constexpr int MAX_W = DS_YIN_MAX_W, MAX_TAU = DS_YIN_MAX_TAU, MAX_NF = DS_PITCH_MAX_FRAMES;

struct YinRow {
    int xoff, len, foff, nf;
};
__device__ __forceinline__ YinRow yin_row(const int32_t* tab, int s) {
    const int32_t* r = tab + (size_t)s * DS_YIN_NI;
    YinRow o;
    o.xoff = DS_LD(int32_t, r + DS_YIN_XOFF, DS_BX_AUX0);
    o.len = DS_LD(int32_t, r + DS_YIN_LEN, DS_BX_AUX0);
    o.foff = DS_LD(int32_t, r + DS_YIN_FOFF, DS_BX_AUX0);
    o.nf = DS_LD(int32_t, r + DS_YIN_NF, DS_BX_AUX0);
    return o;
}
// a range [off, off + n) inside a buffer of `total` elements
__device__ __forceinline__ bool fits(int off, int n, long long total) { return off >= 0 && n >= 0 && (long long)off + n <= total; }

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------------------------------------ YIN
__global__ __launch_bounds__(YT) void yin_frames_kernel(const float* x, const int32_t* tab, long long total_samples, long long total_frames, int W, int hop,
                                                        int tau_min, int tau_max, float thr, float* period, float* aper) {
    __shared__ float s[MAX_W + MAX_TAU];
    __shared__ float d[MAX_TAU + 1];                     // d(tau), then c(tau)
    __shared__ float cs[MAX_TAU + 1];                    // sum_{k = 1 .. tau} d(k)
    __shared__ int red[YT / 64];
    const int tid = threadIdx.x, f = blockIdx.x, n = W + tau_max;
    const YinRow r = yin_row(tab, blockIdx.y);
    if (f >= r.nf || !fits(r.xoff, r.len, total_samples) || !fits(r.foff, r.nf, total_frames)) return;
    const long long first = (long long)f * hop;
    if (first + n > r.len) return;                       // a frame count the signal does not have: nothing is read
    const float* xs = x + r.xoff + first;
    for (int i = tid; i < n; i += YT) s[i] = DS_LD(float, xs + i, DS_BX_SRC0);
    __syncthreads();

    for (int tau = tid; tau <= tau_max; tau += YT) {
        const float* st = s + tau;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int j = 0;
        for (; j + 4 <= W; j += 4) {
            const float e0 = s[j] - st[j], e1 = s[j + 1] - st[j + 1], e2 = s[j + 2] - st[j + 2], e3 = s[j + 3] - st[j + 3];
            a0 = fmaf(e0, e0, a0);
            a1 = fmaf(e1, e1, a1);
            a2 = fmaf(e2, e2, a2);
            a3 = fmaf(e3, e3, a3);
        }
        if (j < W) { const float e = s[j] - st[j]; a0 = fmaf(e, e, a0); }
        if (j + 1 < W) { const float e = s[j + 1] - st[j + 1]; a1 = fmaf(e, e, a1); }
        if (j + 2 < W) { const float e = s[j + 2] - st[j + 2]; a2 = fmaf(e, e, a2); }
        d[tau] = (a0 + a1) + (a2 + a3);
    }
    __syncthreads();
    if (tid == 0) {
        float run = 0.f;
        cs[0] = 0.f;
        for (int t = 1; t <= tau_max; ++t) {
            run += d[t];
            cs[t] = run;
        }
    }
    __syncthreads();
    int best = INT_MAX;
    for (int tau = tid; tau <= tau_max; tau += YT) {
        const float sum = cs[tau];
        const float c = tau > 0 && sum > 0.f ? d[tau] * (float)tau / sum : 1.f;
        d[tau] = c;                                      // the lane's own entry
        if (tau >= tau_min && tau < tau_max && c < thr && tau < best) best = tau;
    }
    best = wave_min_i(best);
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int w = 0; w < YT / 64; ++w) best = red[w] < best ? red[w] : best;
    float p = 0.f, ap = 1.f;
    if (best < tau_max) {
        int t = best;
        while (t + 1 < tau_max && d[t + 1] < d[t]) ++t;
        const float a = d[t - 1], b = d[t], c = d[t + 1];    // tau_min >= 2 and t < tau_max: both neighbours exist
        const float den = (a - 2.0f * b) + c;
        const float off = den > 0.f && b <= a && b <= c ? 0.5f * (a - c) / den : 0.f;
        p = (float)t + off;
        ap = b;
    }
    DS_ST(float, period + r.foff + f, DS_BX_OUT, p);
    DS_ST(float, aper + r.foff + f, DS_BX_AUX1, ap);
}

// ------------------------------------------------------------------------------------------------ lower median of the voiced periods
__global__ __launch_bounds__(YT) void pitch_median_kernel(const float* period, const int32_t* tab, int n_signals, long long total_frames, float* med,
                                                          int32_t* voiced) {
    __shared__ float p[MAX_NF];
    __shared__ int red[YT / 64];
    const int tid = threadIdx.x, s = blockIdx.x;
    if (s >= n_signals) return;
    const YinRow r = yin_row(tab, s);
    const int nf = r.nf > 0 && r.nf <= MAX_NF && fits(r.foff, r.nf, total_frames) ? r.nf : 0;
    int cnt = 0;
    for (int i = tid; i < nf; i += YT) {
        const float v = DS_LD(float, period + r.foff + i, DS_BX_SRC0);
        const bool vo = v > 0.f && v < INFINITY;
        p[i] = vo ? v : INFINITY;
        cnt += vo ? 1 : 0;
    }
    cnt = wave_sum_i(cnt);
    if ((tid & 63) == 0) red[tid >> 6] = cnt;
    __syncthreads();
    int nv = 0;
#pragma unroll
    for (int w = 0; w < YT / 64; ++w) nv += red[w];
    if (tid == 0) DS_ST(int32_t, voiced + s, DS_BX_AUX1, nv);
    if (nv == 0) {
        if (tid == 0) DS_ST(float, med + s, DS_BX_OUT, 0.f);
        return;
    }
    const int rank = (nv - 1) / 2;
    for (int i = tid; i < nf; i += YT) {
        const float v = p[i];
        if (!(v < INFINITY)) continue;
        int c = 0;
#pragma unroll 4
        for (int j = 0; j < nf; ++j) {
            const float u = p[j];
            c += (u < v || (u == v && j < i)) ? 1 : 0;
        }
        if (c == rank) DS_ST(float, med + s, DS_BX_OUT, v);      // (value, index) is a strict order: exactly one element has this count
    }
}

inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
constexpr long long MAX_ELEMS = (1ll << 31) - 1;      // the table's offsets are int32

}  // namespace

extern "C" int ds_yin_frames(const float* x, const int32_t* tab, int n_signals, int max_frames, long long total_samples, long long total_frames,
                             int frame_length, int hop, int tau_min, int tau_max, float threshold, float* period, float* aperiodicity, void* stream) {
    DS_REQUIRE(x && tab && period && aperiodicity && n_signals > 0 && max_frames > 0 && total_samples > 0 && total_frames > 0,
               "yin_frames: bad args (n_signals=%d max_frames=%d total_samples=%lld total_frames=%lld)", n_signals, max_frames, total_samples, total_frames);
    DS_REQUIRE(frame_length >= 1 && frame_length <= MAX_W && hop >= 1 && tau_min >= 2 && tau_min < tau_max && tau_max <= MAX_TAU,
               "yin_frames: 1 <= frame_length <= %d, hop >= 1, 2 <= tau_min < tau_max <= %d (frame_length=%d hop=%d tau_min=%d tau_max=%d)", MAX_W, MAX_TAU,
               frame_length, hop, tau_min, tau_max);
    DS_REQUIRE(threshold > 0.f && threshold < 1.f, "yin_frames: threshold must lie in (0, 1) (threshold=%g)", (double)threshold);
    DS_REQUIRE(n_signals <= 65535 && total_samples <= MAX_ELEMS && total_frames <= MAX_ELEMS, "yin_frames: at most 65535 signals and 2^31 - 1 elements per buffer");
    if (!al4(x) || !al4(tab) || !al4(period) || !al4(aperiodicity)) DS_FAIL(DS_EALIGN, "yin_frames: every pointer must be 4-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#if DS_BOUNDS
    {
        DsBxHost h(DS_K_YIN_FRAMES);
        h.set(DS_BX_SRC0, x, total_samples * 4);
        h.set(DS_BX_AUX0, tab, (long long)n_signals * DS_YIN_NI * 4);
        h.set(DS_BX_OUT, period, total_frames * 4);
        h.set(DS_BX_AUX1, aperiodicity, total_frames * 4);
        h.publish(st);
    }
#endif
    hipLaunchKernelGGL(yin_frames_kernel, dim3(max_frames, n_signals), dim3(YT), 0, st, x, tab, total_samples, total_frames, frame_length, hop, tau_min,
                       tau_max, threshold, period, aperiodicity);
    DS_CHECK_LAUNCH("yin_frames");
    return DS_OK;
}

extern "C" int ds_pitch_median(const float* period, const int32_t* tab, int n_signals, int max_frames, long long total_frames, float* median,
                               int32_t* voiced, void* stream) {
    DS_REQUIRE(period && tab && median && voiced && n_signals > 0 && max_frames > 0 && total_frames > 0,
               "pitch_median: bad args (n_signals=%d max_frames=%d total_frames=%lld)", n_signals, max_frames, total_frames);
    DS_REQUIRE(max_frames <= MAX_NF, "pitch_median: a signal of %d frames (at most %d)", max_frames, MAX_NF);
    DS_REQUIRE(total_frames <= MAX_ELEMS, "pitch_median: at most 2^31 - 1 frames");
    if (!al4(period) || !al4(tab) || !al4(median) || !al4(voiced)) DS_FAIL(DS_EALIGN, "pitch_median: every pointer must be 4-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#if DS_BOUNDS
    {
        DsBxHost h(DS_K_PITCH_MEDIAN);
        h.set(DS_BX_SRC0, period, total_frames * 4);
        h.set(DS_BX_AUX0, tab, (long long)n_signals * DS_YIN_NI * 4);
        h.set(DS_BX_OUT, median, (long long)n_signals * 4);
        h.set(DS_BX_AUX1, voiced, (long long)n_signals * 4);
        h.publish(st);
    }
#endif
    hipLaunchKernelGGL(pitch_median_kernel, dim3(n_signals), dim3(YT), 0, st, period, tab, n_signals, total_frames, median, voiced);
    DS_CHECK_LAUNCH("pitch_median");
    return DS_OK;
}

#if DS_BOUNDS
extern "C" int ds_bounds_fetch_pitch(ds_bounds_rec* out, int reset) { return ds_bounds_fetch_tu(out, reset); }
#endif
