// The arranger's audio stage (gfx950): what webUI/natural_language_guided_4/track_maker.py does on the host per note event — peak
// normalisation (:142), ceil((note - 52) / 4) chained librosa.effects.pitch_shift calls (:12-47: STFT 4096 / 1024 -> phase_vocoder -> iSTFT ->
// resample -> fix_length) and the mix into the track (:147) — as batched fp32 kernels over "signals" of different lengths.
//
// A signal is one row of a device table (int32 [n][DS_PV_NI], include/diffusynth_hip.h): where its samples, analysis frames, synthesis
// frames and stretched samples start in the concatenated buffers, and how many there are.  Everything that is floored or rounded (frame
// counts, round(len / rate), ceil(len * rate), the time steps' floor and fraction) comes from the host in float64; a row that does not
// fit the totals the caller states reads and writes nothing.  No atomics: every output element has one owner and a fixed summation order.
//
// ds_pv_stft     a block transforms TWO consecutive frames of one signal as one 4096-point complex radix-4 Stockham FFT in LDS (frame t in
//                the real part, t + 1 in the imaginary part; separated by symmetry afterwards): six passes between two 32 KB buffers, no bit
//                reversal, three twiddles from one table entry.  Window and centring are fused into the load; the zero padding is the range
//                check of a buffer load.
// ds_pv_vocode   thread = (signal, bin), a recurrence over the synthesis frames: interpolated magnitude x accumulated unit phasor.  librosa's
//                accumulator phi + wrap(angle R - angle L - phi) is angle R - angle L modulo 2 pi, so the phase is kept as the running
//                product of u(R) conj(u(L)), u(z) = z / |z| (1 for z = 0, as np.angle(0) = 0), renormalised every frame: no angle ever
//                reaches the 10^5 rad an fp32 accumulator would lose 1e-4 on, and no atan2f / sinf / cosf is evaluated.
// ds_pv_formant  (opt-in, in place on the synthesis frames) two frames per block once more: the log magnitudes of frames t and t + 1 as the real
//                and imaginary part of one forward transform (both real and even: no separation), lifter, one inverse transform, then
//                V[k] *= exp(clamp(S(k / rate) - S(k))): the envelope the resampler is about to move is put where it will land.
// ds_pv_istft    two frames per block again (Z = A + i B with both Hermitian extensions; the real part of the inverse transform is frame t,
//                the imaginary part frame t + 1), window, frames to the workspace; then overlap-add as a gather: an output sample sums its
//                <= 4 frames in frame order and divides by its window-sum-square.
// ds_resample_sinc  output sample m at input position m / rate (float64 position; integer part + fp32 fraction), windowed sinc
//                h(t) = fc sinc(fc t) kaiser(t fc / Z; beta), fc = 0.95 min(1, rate), Z = 32, beta = 12; the Kaiser window is tabulated per
//                block in LDS (4096 intervals of |t| fc / Z, float64 power series of I0, linear interpolation: 1e-7 of the window's peak);
//                fused with fix_length (zeros from ceil(len_stretched * rate) on).
// ds_peak_normalize  max |x| per signal as per-block partials finished by every consumer wave, then x / max (IEEE division).
// ds_mix_notes   track[s] = sum of the notes covering s in event order: a block walks the host-built list of the events that touch its 1024
//                samples.  With fp32 notes this is bit for bit numpy's float32 += float64.
// ds_mix_notes_shaped  the same walk and store with every sample weighted first: w = gain x ADSR envelope in closed form from the row's
//                segment lengths, rounded to fp32 once, then fl(w x) and the fp32 sum in event order (velocity and gate of the performed mode).
//                The two forms differ on an event that overhangs the track (start + length > track_len): ds_mix_notes mixes it clipped at the
//                track's end, ds_mix_notes_shaped skips it.  arranger.mix_notes refuses such an event for both, so neither is reached.
#include "common.hpp"

namespace {

constexpr int N_FFT = 4096, HOP = 1024, NBINS = N_FFT / 2 + 1;
constexpr int FFT_LDS = 2 * N_FFT * 8 + 1024 * 8;      // two buffers of 4096 complex + 1024 twiddles
constexpr int KW_N = 4096;                            // intervals of the Kaiser table
constexpr int PN_NB_MAX = 64;                         // partial maxima per signal: one wave finishes them
constexpr int RS_SPB = 1024;                          // samples per block: resampler, normaliser, mixer (DS_MIX_BLOCK)
static_assert(RS_SPB == DS_MIX_BLOCK, "the host builds the mixer's per-block lists with DS_MIX_BLOCK");

struct PvRow {
    int xoff, len, foff, nf, toff, nout, soff, slen, nres;
};
__device__ __forceinline__ PvRow pv_row(const int32_t* tab, int s) {
    const int32_t* r = tab + (size_t)s * DS_PV_NI;
    PvRow o;
    o.xoff = DS_LD(int32_t, r + DS_PV_XOFF, DS_BX_AUX0);
    o.len = DS_LD(int32_t, r + DS_PV_LEN, DS_BX_AUX0);
    o.foff = DS_LD(int32_t, r + DS_PV_FOFF, DS_BX_AUX0);
    o.nf = DS_LD(int32_t, r + DS_PV_NF, DS_BX_AUX0);
    o.toff = DS_LD(int32_t, r + DS_PV_TOFF, DS_BX_AUX0);
    o.nout = DS_LD(int32_t, r + DS_PV_NOUT, DS_BX_AUX0);
    o.soff = DS_LD(int32_t, r + DS_PV_SOFF, DS_BX_AUX0);
    o.slen = DS_LD(int32_t, r + DS_PV_SLEN, DS_BX_AUX0);
    o.nres = DS_LD(int32_t, r + DS_PV_NRES, DS_BX_AUX0);
    return o;
}
// a range [off, off + n) inside a buffer of `total` elements
__device__ __forceinline__ bool fits(int off, int n, long long total) { return off >= 0 && n >= 0 && (long long)off + n <= total; }

// x[i] for 0 <= i < n, zero outside.  Product build: the range check of a raw buffer load (a negative i is a huge unsigned offset)
__device__ __forceinline__ float ld_zero(const float* x, int i, int n, int bx) {
#if DS_BOUNDS
    return i >= 0 && i < n ? DS_LD(float, x + i, bx) : 0.f;
#else
    (void)bx;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), (short)0, n * 4, 0x00020000);
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, i * 4, 0, 0));
#endif
}

__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return float2{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }

// exp(-+ 2 pi i m / 4096), m < 1024 (INV: +)
template <bool INV> __device__ __forceinline__ void fill_twiddles(float2* tw, int tid) {
    for (int m = tid; m < 1024; m += 256) {
        float sn, cs;
        sincospif(2.0f * (float)m / (float)N_FFT, &sn, &cs);
        tw[m] = float2{cs, INV ? sn : -sn};
    }
}
// 4096-point complex transform of b0 (natural order in and out, result in b0), 256 threads: four radix-4 butterflies per thread and pass
template <bool INV> __device__ __forceinline__ void fft4096(float2* b0, float2* b1, const float2* tw, int tid) {
    float2 *x = b0, *y = b1;
#pragma unroll 1
    for (int s = 0; s < 6; ++s) {
        const int p = 1 << (2 * s), sh = 10 - 2 * s;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = tid + 256 * r, k = i & (p - 1), j = ((i - k) << 2) + k;
            const float2 w1 = tw[k << sh], w2 = cmul(w1, w1), w3 = cmul(w2, w1);
            const float2 u0 = x[i], u1 = cmul(x[i + 1024], w1), u2 = cmul(x[i + 2048], w2), u3 = cmul(x[i + 3072], w3);
            const float2 a0 = {u0.x + u2.x, u0.y + u2.y}, a1 = {u0.x - u2.x, u0.y - u2.y}, a2 = {u1.x + u3.x, u1.y + u3.y};
            const float2 d = {u1.x - u3.x, u1.y - u3.y};
            const float2 a3 = INV ? float2{-d.y, d.x} : float2{d.y, -d.x};          // +- i (u1 - u3)
            y[j] = float2{a0.x + a2.x, a0.y + a2.y};
            y[j + p] = float2{a1.x + a3.x, a1.y + a3.y};
            y[j + 2 * p] = float2{a0.x - a2.x, a0.y - a2.y};
            y[j + 3 * p] = float2{a1.x - a3.x, a1.y - a3.y};
        }
        __syncthreads();
        float2* t = x; x = y; y = t;
    }
}
__device__ __forceinline__ float hann_at(int n) { return 0.5f - 0.5f * cospif(2.0f * (float)n / (float)N_FFT); }

// ------------------------------------------------------------------------------------------------ STFT
__global__ __launch_bounds__(256) void pv_stft_kernel(const float* x, const int32_t* tab, long long total_samples, long long total_frames, float2* spec) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    float2 *b0 = sm, *b1 = sm + N_FFT, *tw = sm + 2 * N_FFT;
    const int tid = threadIdx.x, t0 = 2 * blockIdx.x;
    const PvRow r = pv_row(tab, blockIdx.y);
    if (t0 >= r.nf || !fits(r.xoff, r.len, total_samples) || !fits(r.foff, r.nf, total_frames)) return;
    const bool two = t0 + 1 < r.nf;
    fill_twiddles<false>(tw, tid);
    const float* xs = x + r.xoff;
    for (int n = tid; n < N_FFT; n += 256) {
        const float w = hann_at(n);
        const int i = t0 * HOP + n - N_FFT / 2;
        const float a = ld_zero(xs, i, r.len, DS_BX_SRC0), b = two ? ld_zero(xs, i + HOP, r.len, DS_BX_SRC0) : 0.f;
        b0[n] = float2{a * w, b * w};
    }
    __syncthreads();
    fft4096<false>(b0, b1, tw, tid);
    // Z = FFT(a + i b): A[k] = (Z[k] + conj Z[N - k]) / 2, B[k] = -i (Z[k] - conj Z[N - k]) / 2
    float2* o = spec + ((size_t)r.foff + t0) * NBINS;
    for (int k = tid; k < NBINS; k += 256) {
        const float2 z1 = b0[k], z2 = b0[(N_FFT - k) & (N_FFT - 1)];
        DS_ST(float2, o + k, DS_BX_OUT, (float2{0.5f * (z1.x + z2.x), 0.5f * (z1.y - z2.y)}));
        if (two) DS_ST(float2, o + NBINS + k, DS_BX_OUT, (float2{0.5f * (z1.y + z2.y), -0.5f * (z1.x - z2.x)}));
    }
}

// ------------------------------------------------------------------------------------------------ phase vocoder
// |v| and v / |v| (1 for v = 0).  The pair is scaled by an exact power of two first so that the squares neither underflow nor overflow.
__device__ __forceinline__ float2 unit_mag(float2 v, float& mag) {
    const float pm = fmaxf(fabsf(v.x), fabsf(v.y));
    if (!(pm > 0.f)) {
        mag = 0.f;
        return float2{1.f, 0.f};
    }
    const int e = __builtin_amdgcn_frexp_expf(pm);
    const float a = ldexpf(v.x, -e), b = ldexpf(v.y, -e);
    const float n = sqrtf(a * a + b * b);
    mag = ldexpf(n, e);
    return float2{a / n, b / n};
}

constexpr int PV_U = 4;       // synthesis frames whose operands are requested before the recurrence consumes them
__global__ __launch_bounds__(256) void pv_vocode_kernel(const float2* spec, const int32_t* tab, const int32_t* step_idx, const float* step_alpha,
                                                        long long total_frames, long long total_out, float2* voc) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    const PvRow r = pv_row(tab, blockIdx.y);
    if (k >= NBINS || r.nf <= 0 || !fits(r.foff, r.nf, total_frames) || !fits(r.toff, r.nout, total_out)) return;
    const float2* D = spec + (size_t)r.foff * NBINS + k;
    float m0;
    float2 acc = unit_mag(DS_LD(float2, D, DS_BX_SRC0), m0);
    for (int t0 = 0; t0 < r.nout; t0 += PV_U) {
        float2 Lc[PV_U], Rc[PV_U];
        float al[PV_U];
#pragma unroll
        for (int u = 0; u < PV_U; ++u) {
            const int t = t0 + u < r.nout ? t0 + u : r.nout - 1;
            const int i0 = DS_LD(int32_t, step_idx + r.toff + t, DS_BX_AUX1);
            al[u] = DS_LD(float, step_alpha + r.toff + t, DS_BX_AUX2);
            const bool okl = i0 >= 0 && i0 < r.nf, okr = i0 >= -1 && i0 + 1 < r.nf;       // the two zero frames librosa appends
            Lc[u] = okl ? DS_LD(float2, D + (size_t)i0 * NBINS, DS_BX_SRC0) : float2{0.f, 0.f};
            Rc[u] = okr ? DS_LD(float2, D + (size_t)(i0 + 1) * NBINS, DS_BX_SRC0) : float2{0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < PV_U; ++u) {
            if (t0 + u >= r.nout) break;
            float ml, mr;
            const float2 ul = unit_mag(Lc[u], ml), ur = unit_mag(Rc[u], mr);
            const float mag = (1.0f - al[u]) * ml + al[u] * mr;
            DS_ST(float2, voc + ((size_t)r.toff + t0 + u) * NBINS + k, DS_BX_OUT, (float2{mag * acc.x, mag * acc.y}));
            acc = cmul(acc, cmul(ur, float2{ul.x, -ul.y}));
            const float n = sqrtf(acc.x * acc.x + acc.y * acc.y);
            acc = float2{acc.x / n, acc.y / n};
        }
    }
}

// ------------------------------------------------------------------------------------------------ formant correction
// V[k] *= exp(clamp(S(k warp) - S(k), +- limit)), S = the cepstrally smoothed log magnitude of the frame (include/diffusynth_hip.h).
// L_t and L_{t+1} are real and even, so are their transforms: Re FFT(L_t + i L_{t+1}) is frame t's cepstrum and Im frame t + 1's, the
// lifter is a real mask, and the inverse transform's real / imaginary parts are S_t / S_{t+1} — two frames per transform pair and no
// separation step.  The frames stay in registers between the load and the store: one read and one write of voc.
constexpr int FM_PER = (NBINS + 255) / 256;           // bins per thread (the last round holds bin 2048 alone)
constexpr float FM_FLOOR = 1e-6f;
__device__ __forceinline__ float log_mag(float2 v) {
    float m;
    (void)unit_mag(v, m);
    return logf(fmaxf(m, FM_FLOOR));
}
__device__ __forceinline__ float formant_gain(float sk, float lo, float hi, float f, float limit) {
    const float sq = (1.0f - f) * lo + f * hi;
    return expf(fminf(fmaxf(sq - sk, -limit), limit));
}

__global__ __launch_bounds__(256) void pv_formant_kernel(float2* voc, const int32_t* tab, const int32_t* order, const float* warp, float limit,
                                                         long long total_out) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    float2 *b0 = sm, *b1 = sm + N_FFT, *tw = sm + 2 * N_FFT;
    const int tid = threadIdx.x, t0 = 2 * blockIdx.x;
    const PvRow r = pv_row(tab, blockIdx.y);
    if (t0 >= r.nout || !fits(r.toff, r.nout, total_out)) return;
    const int ord = DS_LD(int32_t, order + blockIdx.y, DS_BX_AUX1);
    if (ord < 1 || ord > DS_PV_ORDER_MAX) return;
    const float wp = DS_LD(float, warp + blockIdx.y, DS_BX_AUX2);
    const bool two = t0 + 1 < r.nout;
    fill_twiddles<false>(tw, tid);
    float2* v = voc + ((size_t)r.toff + t0) * NBINS;
    float2 va[FM_PER], vb[FM_PER];
#pragma unroll
    for (int j = 0; j < FM_PER; ++j) {
        const int k = tid + 256 * j;
        if (k >= NBINS) continue;
        va[j] = DS_LD(float2, v + k, DS_BX_OUT);
        vb[j] = two ? DS_LD(float2, v + NBINS + k, DS_BX_OUT) : float2{0.f, 0.f};      // an odd last frame: the lane stays at ln(floor)
        const float2 l = {log_mag(va[j]), log_mag(vb[j])};
        b0[k] = l;
        if (k != 0 && k != N_FFT / 2) b0[N_FFT - k] = l;                                 // the even extension
    }
    __syncthreads();
    fft4096<false>(b0, b1, tw, tid);
    for (int n = tid; n < N_FFT; n += 256) {                                             // lifter and 1 / N, each element by its own thread
        const int m = n < N_FFT - n ? n : N_FFT - n;
        const float2 c = b0[n];
        b0[n] = m <= ord ? float2{c.x * (1.0f / N_FFT), c.y * (1.0f / N_FFT)} : float2{0.f, 0.f};
    }
    for (int m = tid; m < 1024; m += 256) tw[m].y = -tw[m].y;                            // the inverse transform's twiddles: the conjugates
    __syncthreads();
    fft4096<true>(b0, b1, tw, tid);
#pragma unroll
    for (int j = 0; j < FM_PER; ++j) {
        const int k = tid + 256 * j;
        if (k >= NBINS) continue;
        const float q = fminf((float)k * wp, (float)(N_FFT / 2));
        int i = (int)floorf(q);
        i = i < N_FFT / 2 - 1 ? i : N_FFT / 2 - 1;
        i = i > 0 ? i : 0;                                                               // (a NaN or negative warp stays inside the buffer)
        const float f = q - (float)i;
        const float2 sk = b0[k], lo = b0[i], hi = b0[i + 1];
        const float ga = formant_gain(sk.x, lo.x, hi.x, f, limit);
        DS_ST(float2, v + k, DS_BX_OUT, (float2{va[j].x * ga, va[j].y * ga}));
        if (two) {
            const float gb = formant_gain(sk.y, lo.y, hi.y, f, limit);
            DS_ST(float2, v + NBINS + k, DS_BX_OUT, (float2{vb[j].x * gb, vb[j].y * gb}));
        }
    }
}

// ------------------------------------------------------------------------------------------------ iSTFT
__global__ __launch_bounds__(256) void pv_istft_frames_kernel(const float2* voc, const int32_t* tab, long long total_out, float* frames) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    float2 *b0 = sm, *b1 = sm + N_FFT, *tw = sm + 2 * N_FFT;
    const int tid = threadIdx.x, t0 = 2 * blockIdx.x;
    const PvRow r = pv_row(tab, blockIdx.y);
    if (t0 >= r.nout || !fits(r.toff, r.nout, total_out)) return;
    const bool two = t0 + 1 < r.nout;
    fill_twiddles<true>(tw, tid);
    const float2* v = voc + ((size_t)r.toff + t0) * NBINS;
    for (int k = tid; k < NBINS; k += 256) {
        float2 a = DS_LD(float2, v + k, DS_BX_SRC0), b = two ? DS_LD(float2, v + NBINS + k, DS_BX_SRC0) : float2{0.f, 0.f};
        const bool edge = k == 0 || k == N_FFT / 2;               // the imaginary parts of DC and Nyquist do not exist for a real signal
        if (edge) a.y = b.y = 0.f;
        b0[k] = float2{a.x - b.y, a.y + b.x};                     // A + i B
        if (!edge) b0[N_FFT - k] = float2{a.x + b.y, b.x - a.y};  // conj A + i conj B
    }
    __syncthreads();
    fft4096<true>(b0, b1, tw, tid);
    float* f = frames + ((size_t)r.toff + t0) * N_FFT;
    for (int n = tid; n < N_FFT; n += 256) {
        const float w = hann_at(n) * (1.0f / N_FFT);
        const float2 z = b0[n];
        DS_ST(float, f + n, DS_BX_AUX1, z.x * w);
        if (two) DS_ST(float, f + N_FFT + n, DS_BX_AUX1, z.y * w);
    }
}

__global__ __launch_bounds__(256) void pv_ola_kernel(const float* frames, const int32_t* tab, long long total_out, long long total_stretched, float* y) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    const PvRow r = pv_row(tab, blockIdx.y);
    if (s >= r.slen || !fits(r.toff, r.nout, total_out) || !fits(r.soff, r.slen, total_stretched)) return;
    const int pos = s + N_FFT / 2;
    int t_hi = pos / HOP;
    t_hi = t_hi < r.nout - 1 ? t_hi : r.nout - 1;
    const int t_lo = pos < N_FFT ? 0 : (pos - N_FFT) / HOP + 1;          // the smallest t with t * HOP > pos - N_FFT
    const float* f = frames + (size_t)r.toff * N_FFT;
    float v = 0.f, wss = 0.f;
    for (int t = t_lo; t <= t_hi; ++t) {
        const int n = pos - t * HOP;
        const float w = hann_at(n);
        v += DS_LD(float, f + (size_t)t * N_FFT + n, DS_BX_AUX1);
        wss += w * w;
    }
    DS_ST(float, y + r.soff + s, DS_BX_OUT, wss > 1.17549435e-38f ? v / wss : v);
}

// ------------------------------------------------------------------------------------------------ resampler
__device__ __forceinline__ double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, s = 1.0;
#pragma unroll
    for (int k = 1; k < 40; ++k) {
        term *= q * (1.0 / (double)(k * k));      // (a constant after unrolling: a float64 division per term was 100 us per launch)
        s += term;
    }
    return s;
}

__global__ __launch_bounds__(256) void resample_sinc_kernel(const float* ys, const int32_t* tab, const double* rates, long long total_stretched,
                                                            long long total_samples, float* out) {
    __shared__ float kw[KW_N + 2];
    const int tid = threadIdx.x;
    const PvRow r = pv_row(tab, blockIdx.y);
    const int m0 = blockIdx.x * RS_SPB;
    if (m0 >= r.len || !fits(r.xoff, r.len, total_samples) || !fits(r.soff, r.slen, total_stretched)) return;
    const double rate = DS_LD(double, rates + blockIdx.y, DS_BX_AUX1);
    if (!(rate > 0.0)) return;
    {
        const double inv = 1.0 / bessel_i0(DS_RS_BETA);
        for (int i = tid; i < KW_N + 2; i += 256) {
            const double u = (double)i / KW_N, a = 1.0 - u * u;
            kw[i] = a > 0.0 ? (float)(bessel_i0(DS_RS_BETA * sqrt(a)) * inv) : (i == KW_N ? (float)inv : 0.f);
        }
    }
    __syncthreads();
    const double fcd = DS_RS_FC * (rate < 1.0 ? rate : 1.0), half = DS_RS_ZEROS / fcd;
    const float fc = (float)fcd, uscale = (float)(fcd / DS_RS_ZEROS * KW_N);
    const int K = (int)ceil(half) + 1;
    const float* x = ys + r.soff;
#pragma unroll 1
    for (int q = 0; q < RS_SPB / 256; ++q) {
        const int m = m0 + q * 256 + tid;
        if (m >= r.len) break;
        float acc = 0.f;
        if (m < r.nres) {
            const double p = (double)m / rate, pf = floor(p), fracd = p - pf;
            const int base = (int)pf;
            const float frac = (float)fracd;
            for (int j = -K; j <= K; ++j) {
                const int n = base + j;
                if (fabs(fracd - (double)j) > half || n < 0 || n >= r.slen) continue;
                const float t = frac - (float)j, a = fc * t;
                const float u = fabsf(t) * uscale;
                int iu = (int)u;
                iu = iu < KW_N ? iu : KW_N;
                const float fu = u - (float)iu, w = kw[iu] + fu * (kw[iu + 1] - kw[iu]);
                const float sinc = a == 0.f ? 1.0f : sinpif(a) / (3.14159265358979323846f * a);
                acc += fc * sinc * w * DS_LD(float, x + n, DS_BX_SRC0);
            }
        }
        DS_ST(float, out + r.xoff + m, DS_BX_OUT, acc);
    }
}

// ------------------------------------------------------------------------------------------------ peak normalisation
__global__ __launch_bounds__(256) void peak_partial_kernel(const float* x, const int32_t* tab, long long total_samples, int nb, float* part) {
    __shared__ float red[4];
    const PvRow r = pv_row(tab, blockIdx.y);
    float mx = 0.f;
    if (fits(r.xoff, r.len, total_samples))
        for (int i = blockIdx.x * 256 + threadIdx.x; i < r.len; i += nb * 256) mx = fmaxf(mx, fabsf(DS_LD(float, x + r.xoff + i, DS_BX_SRC0)));
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) DS_ST(float, part + (size_t)blockIdx.y * nb + blockIdx.x, DS_BX_AUX1, fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
}

__global__ __launch_bounds__(256) void peak_divide_kernel(const float* x, const int32_t* tab, long long total_samples, int nb, const float* part, float* out) {
    const PvRow r = pv_row(tab, blockIdx.y);
    if (blockIdx.x * RS_SPB >= r.len || !fits(r.xoff, r.len, total_samples)) return;
    const int lane = threadIdx.x & 63;
    const float mx = wave_max(lane < nb ? DS_LD(float, part + (size_t)blockIdx.y * nb + lane, DS_BX_AUX1) : 0.f);
#pragma unroll
    for (int q = 0; q < RS_SPB / 256; ++q) {
        const int i = blockIdx.x * RS_SPB + q * 256 + threadIdx.x;
        if (i < r.len) DS_ST(float, out + r.xoff + i, DS_BX_OUT, __fdiv_rn(DS_LD(float, x + r.xoff + i, DS_BX_SRC0), mx));
    }
}

// ------------------------------------------------------------------------------------------------ mix
// ev [n_ev][3]: start sample in the track, offset of the note in `notes`, length.  Block b walks blk_ev[blk_ptr[b] .. blk_ptr[b + 1]):
// the events that touch its samples, in event order.  SHAPED: rows of DS_MX_NI words (the same three first), every sample weighted by
// w = gain * env(j) before it is added; `length` is then the mixed length min(note, envelope).

// The envelope of one shaped row: segment ends and numpy's linspace per segment (start + k * step, the last element of a segment of more
// than one sample exactly its stop; the host hands a step of 0 for segments of 0 or 1 samples).
struct MixShape {
    int b1, b2, b3, b4, na, nd, nr;
    float gain, sus, sa, sd, sr, wsus;
    bool ok;
};
__device__ __forceinline__ MixShape mix_shape(const int32_t* r) {
    MixShape h;
    h.na = DS_LD(int32_t, r + DS_MX_NA, DS_BX_AUX0);
    h.nd = DS_LD(int32_t, r + DS_MX_ND, DS_BX_AUX0);
    const int ns = DS_LD(int32_t, r + DS_MX_NS, DS_BX_AUX0);
    h.nr = DS_LD(int32_t, r + DS_MX_NR, DS_BX_AUX0);
    h.gain = DS_LD(float, r + DS_MX_GAIN, DS_BX_AUX0);
    h.sus = DS_LD(float, r + DS_MX_SUSTAIN, DS_BX_AUX0);
    h.sa = DS_LD(float, r + DS_MX_STEP_A, DS_BX_AUX0);
    h.sd = DS_LD(float, r + DS_MX_STEP_D, DS_BX_AUX0);
    h.sr = DS_LD(float, r + DS_MX_STEP_R, DS_BX_AUX0);
    const long long end = (long long)h.na + h.nd + ns + h.nr;
    h.ok = h.na >= 0 && h.nd >= 0 && ns >= 0 && h.nr >= 0 && end <= 0x7fffffffll;
    h.b1 = h.na;
    h.b2 = h.b1 + h.nd;
    h.b3 = h.b2 + ns;
    h.b4 = h.b3 + h.nr;
    h.wsus = (float)((double)h.gain * (double)h.sus);
    return h;
}
// gain * env(j), the product formed in fp64 from the fp32 table entries and rounded to fp32 ONCE.  Most of a held note is sustain, and a
// wave's 64 consecutive samples are mostly all in it: that side is one value per event and whole waves skip the ramps (selects, no
// further branches; the caller has the note loads in flight meanwhile).
__device__ __forceinline__ float mix_weight(const MixShape& h, int j) {
#pragma clang fp contract(off)                           // a + k * st as numpy forms it: a product, then a sum
    if (j >= h.b2 && j < h.b3) return h.wsus;
    const bool atk = j < h.b1, dec = !atk && j < h.b2, past = j >= h.b4, rel = !past && j >= h.b3 && !atk && !dec;
    const int k = atk ? j : dec ? j - h.b1 : rel ? j - h.b3 : 0;
    const int n = atk ? h.na : dec ? h.nd : rel ? h.nr : 0;                      // sustain and after: env = a + 0 * 0
    const float a = atk || past ? 0.f : dec ? 1.f : h.sus;
    const float st = atk ? h.sa : dec ? h.sd : rel ? h.sr : 0.f;
    const float stop = atk ? 1.f : rel ? 0.f : h.sus;
    const double env = (n > 1 && k == n - 1) ? (double)stop : (double)a + (double)k * (double)st;
    return (float)((double)h.gain * env);
}

template <bool SHAPED>
__global__ __launch_bounds__(256) void mix_notes_kernel(const float* notes, long long total_samples, const int32_t* ev, int n_ev, const int32_t* blk_ptr,
                                                        const int32_t* blk_ev, int n_blk_ev, float* track, int track_len) {
    constexpr int NI = SHAPED ? DS_MX_NI : DS_MX_NI_PLAIN;
    const int s0 = blockIdx.x * RS_SPB + threadIdx.x;
    float acc[RS_SPB / 256];
#pragma unroll
    for (int q = 0; q < RS_SPB / 256; ++q) acc[q] = 0.f;
    int e0 = DS_LD(int32_t, blk_ptr + blockIdx.x, DS_BX_AUX1), e1 = DS_LD(int32_t, blk_ptr + blockIdx.x + 1, DS_BX_AUX1);
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > n_blk_ev ? n_blk_ev : e1;
    for (int e = e0; e < e1; ++e) {
        const int id = DS_LD(int32_t, blk_ev + e, DS_BX_AUX2);
        if (id < 0 || id >= n_ev) continue;
        const int32_t* r = ev + (size_t)NI * id;
        const int start = DS_LD(int32_t, r + DS_MX_START, DS_BX_AUX0), off = DS_LD(int32_t, r + DS_MX_OFF, DS_BX_AUX0),
                  len = DS_LD(int32_t, r + DS_MX_LEN, DS_BX_AUX0);
        if constexpr (SHAPED) {
            const MixShape h = mix_shape(r);             // the whole row before any test of it: early exits between its loads serialise them
            if (!fits(off, len, total_samples) || !fits(start, len, track_len) || !h.ok) continue;
            float x[RS_SPB / 256];
#pragma unroll
            for (int q = 0; q < RS_SPB / 256; ++q) {     // the note loads first, all in flight while the weights are formed
                const int j = s0 + q * 256 - start;
                x[q] = (j >= 0 && j < len) ? DS_LD(float, notes + off + j, DS_BX_SRC0) : 0.f;
            }
#pragma unroll
            for (int q = 0; q < RS_SPB / 256; ++q) {
                // HIP contracts by default, and __fmul_rn / __fadd_rn are inline `*` / `+` that carry their header's contraction with
                // them: plain operators under the pragma, or the pair is one v_fma_f32 and the product is never rounded
#pragma clang fp contract(off)
                const int j = s0 + q * 256 - start;
                const float p = mix_weight(h, j) * x[q];
                const float sum = acc[q] + p;
                acc[q] = (j >= 0 && j < len) ? sum : acc[q];
            }
        } else {
            if (!fits(off, len, total_samples)) continue;
#pragma unroll
            for (int q = 0; q < RS_SPB / 256; ++q) {
                const int j = s0 + q * 256 - start;
                if (j >= 0 && j < len) acc[q] = __fadd_rn(acc[q], DS_LD(float, notes + off + j, DS_BX_SRC0));
            }
        }
    }
#pragma unroll
    for (int q = 0; q < RS_SPB / 256; ++q)
        if (s0 + q * 256 < track_len) DS_ST(float, track + s0 + q * 256, DS_BX_OUT, acc[q]);
}

inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
constexpr long long MAX_ELEMS = (1ll << 31) - 1;      // the table's offsets are int32
constexpr long long STFT_MAX_SAMPLES = (1ll << 30) - N_FFT / 2;       // ld_zero: byte counts and byte offsets of 32 bits

}  // namespace

extern "C" int ds_pv_stft(const float* x, const int32_t* tab, int n_signals, int max_frames, long long total_samples, long long total_frames, float* spec,
                          void* stream) {
    DS_REQUIRE(x && tab && spec && n_signals > 0 && max_frames > 0 && total_samples > 0 && total_frames > 0,
               "pv_stft: bad args (n_signals=%d max_frames=%d total_samples=%lld total_frames=%lld)", n_signals, max_frames, total_samples, total_frames);
    DS_REQUIRE(n_signals <= 65535 && total_samples <= MAX_ELEMS && total_frames * NBINS <= MAX_ELEMS, "pv_stft: at most 65535 signals and 2^31 - 1 elements per buffer");
    // ld_zero's range check is a buffer descriptor of len * 4 bytes and a byte offset of i * 4, both 32-bit words: a frame reaches
    // i = len + 2047, and from (len + 2047) * 4 = 2^32 on the offset wraps back into the signal instead of reading the zero padding
    DS_REQUIRE(total_samples <= STFT_MAX_SAMPLES, "pv_stft: at most 2^30 - 2048 samples (total_samples=%lld): the zero padding is the range check of a 32-bit byte offset",
               total_samples);
    if (!al4(x) || !al4(tab) || !al8(spec)) DS_FAIL(DS_EALIGN, "pv_stft: x / tab must be 4-byte, spec 8-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#if DS_BOUNDS
    {
        DsBxHost h(DS_K_PV_STFT);
        h.set(DS_BX_SRC0, x, total_samples * 4);
        h.set(DS_BX_AUX0, tab, (long long)n_signals * DS_PV_NI * 4);
        h.set(DS_BX_OUT, spec, total_frames * NBINS * 8);
        h.publish(st);
    }
#endif
    DS_SET_MAX_LDS(pv_stft_kernel, FFT_LDS, "pv_stft");
    hipLaunchKernelGGL(pv_stft_kernel, dim3((max_frames + 1) / 2, n_signals), dim3(256), FFT_LDS, st, x, tab, total_samples, total_frames,
                       reinterpret_cast<float2*>(spec));
    DS_CHECK_LAUNCH("pv_stft");
    return DS_OK;
}

extern "C" int ds_pv_vocode(const float* spec, const int32_t* tab, const int32_t* step_idx, const float* step_alpha, int n_signals, long long total_frames,
                            long long total_out, float* voc, void* stream) {
    DS_REQUIRE(spec && tab && step_idx && step_alpha && voc && n_signals > 0 && total_frames > 0 && total_out > 0,
               "pv_vocode: bad args (n_signals=%d total_frames=%lld total_out=%lld)", n_signals, total_frames, total_out);
    DS_REQUIRE(n_signals <= 65535 && total_frames * NBINS <= MAX_ELEMS && total_out * NBINS <= MAX_ELEMS, "pv_vocode: at most 65535 signals and 2^31 - 1 elements per buffer");
    if (!al8(spec) || !al8(voc) || !al4(tab) || !al4(step_idx) || !al4(step_alpha)) DS_FAIL(DS_EALIGN, "pv_vocode: spec / voc must be 8-byte, the tables 4-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#if DS_BOUNDS
    {
        DsBxHost h(DS_K_PV_VOCODE);
        h.set(DS_BX_SRC0, spec, total_frames * NBINS * 8);
        h.set(DS_BX_AUX0, tab, (long long)n_signals * DS_PV_NI * 4);
        h.set(DS_BX_AUX1, step_idx, total_out * 4);
        h.set(DS_BX_AUX2, step_alpha, total_out * 4);
        h.set(DS_BX_OUT, voc, total_out * NBINS * 8);
        h.publish(st);
    }
#endif
    hipLaunchKernelGGL(pv_vocode_kernel, dim3((NBINS + 255) / 256, n_signals), dim3(256), 0, st, reinterpret_cast<const float2*>(spec), tab, step_idx,
                       step_alpha, total_frames, total_out, reinterpret_cast<float2*>(voc));
    DS_CHECK_LAUNCH("pv_vocode");
    return DS_OK;
}

extern "C" int ds_pv_formant(float* voc, const int32_t* tab, const int32_t* order, const float* warp, float limit, int n_signals, int max_out,
                             long long total_out, void* stream) {
    DS_REQUIRE(voc && tab && order && warp && n_signals > 0 && max_out > 0 && total_out > 0, "pv_formant: bad args (n_signals=%d max_out=%d total_out=%lld)",
               n_signals, max_out, total_out);
    DS_REQUIRE(n_signals <= 65535 && total_out * NBINS <= MAX_ELEMS, "pv_formant: at most 65535 signals and 2^31 - 1 elements per buffer");
    // (0, DS_PV_GAIN_DB_MAX dB] in nepers; the slack is an fp32 rounding of the caller's product
    DS_REQUIRE(limit > 0.f && (double)limit <= DS_PV_GAIN_DB_MAX * (2.302585092994046 / 20.0) * (1.0 + 1e-6),
               "pv_formant: the limit must be inside (0, %d dB] in nepers, dB ln 10 / 20 (limit=%g)", DS_PV_GAIN_DB_MAX, (double)limit);
    if (!al8(voc) || !al4(tab) || !al4(order) || !al4(warp)) DS_FAIL(DS_EALIGN, "pv_formant: voc must be 8-byte, tab / order / warp 4-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#if DS_BOUNDS
    {
        DsBxHost h(DS_K_PV_FORMANT);
        h.set(DS_BX_AUX0, tab, (long long)n_signals * DS_PV_NI * 4);
        h.set(DS_BX_AUX1, order, (long long)n_signals * 4);
        h.set(DS_BX_AUX2, warp, (long long)n_signals * 4);
        h.set(DS_BX_OUT, voc, total_out * NBINS * 8);
        h.publish(st);
    }
#endif
    DS_SET_MAX_LDS(pv_formant_kernel, FFT_LDS, "pv_formant");
    hipLaunchKernelGGL(pv_formant_kernel, dim3((max_out + 1) / 2, n_signals), dim3(256), FFT_LDS, st, reinterpret_cast<float2*>(voc), tab, order, warp, limit,
                       total_out);
    DS_CHECK_LAUNCH("pv_formant");
    return DS_OK;
}

extern "C" size_t ds_pv_istft_ws_bytes(long long total_out) { return total_out > 0 ? (size_t)total_out * N_FFT * 4 : 0; }

extern "C" int ds_pv_istft(const float* voc, const int32_t* tab, int n_signals, int max_out, int max_stretched, long long total_out, long long total_stretched,
                           float* ws, float* y, void* stream) {
    DS_REQUIRE(voc && tab && ws && y && n_signals > 0 && max_out > 0 && max_stretched > 0 && total_out > 0 && total_stretched > 0,
               "pv_istft: bad args (n_signals=%d max_out=%d max_stretched=%d total_out=%lld total_stretched=%lld)", n_signals, max_out, max_stretched, total_out,
               total_stretched);
    DS_REQUIRE(n_signals <= 65535 && total_out * N_FFT <= MAX_ELEMS && total_stretched <= MAX_ELEMS, "pv_istft: at most 65535 signals and 2^31 - 1 elements per buffer");
    if (!al8(voc) || !al4(tab) || !al4(ws) || !al4(y)) DS_FAIL(DS_EALIGN, "pv_istft: voc must be 8-byte, tab / ws / y 4-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#if DS_BOUNDS
    {   // one table for both launches (see ui_images.hip)
        DsBxHost h(DS_K_PV_ISTFT);
        h.set(DS_BX_SRC0, voc, total_out * NBINS * 8);
        h.set(DS_BX_AUX0, tab, (long long)n_signals * DS_PV_NI * 4);
        h.set(DS_BX_AUX1, ws, total_out * N_FFT * 4);
        h.set(DS_BX_OUT, y, total_stretched * 4);
        h.publish(st);
    }
#endif
    DS_SET_MAX_LDS(pv_istft_frames_kernel, FFT_LDS, "pv_istft");
    hipLaunchKernelGGL(pv_istft_frames_kernel, dim3((max_out + 1) / 2, n_signals), dim3(256), FFT_LDS, st, reinterpret_cast<const float2*>(voc), tab, total_out, ws);
    DS_CHECK_LAUNCH("pv_istft (frames)");
    hipLaunchKernelGGL(pv_ola_kernel, dim3((max_stretched + 255) / 256, n_signals), dim3(256), 0, st, ws, tab, total_out, total_stretched, y);
    DS_CHECK_LAUNCH("pv_istft (overlap-add)");
    return DS_OK;
}

extern "C" int ds_resample_sinc(const float* ys, const int32_t* tab, const double* rates, int n_signals, int max_len, long long total_stretched,
                                long long total_samples, float* out, void* stream) {
    DS_REQUIRE(ys && tab && rates && out && n_signals > 0 && max_len > 0 && total_stretched > 0 && total_samples > 0,
               "resample_sinc: bad args (n_signals=%d max_len=%d total_stretched=%lld total_samples=%lld)", n_signals, max_len, total_stretched, total_samples);
    DS_REQUIRE(n_signals <= 65535 && total_stretched <= MAX_ELEMS && total_samples <= MAX_ELEMS, "resample_sinc: at most 65535 signals and 2^31 - 1 elements per buffer");
    if (!al4(ys) || !al4(tab) || !al8(rates) || !al4(out)) DS_FAIL(DS_EALIGN, "resample_sinc: rates must be 8-byte, ys / tab / out 4-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#if DS_BOUNDS
    {
        DsBxHost h(DS_K_RESAMPLE_SINC);
        h.set(DS_BX_SRC0, ys, total_stretched * 4);
        h.set(DS_BX_AUX0, tab, (long long)n_signals * DS_PV_NI * 4);
        h.set(DS_BX_AUX1, rates, (long long)n_signals * 8);
        h.set(DS_BX_OUT, out, total_samples * 4);
        h.publish(st);
    }
#endif
    hipLaunchKernelGGL(resample_sinc_kernel, dim3((max_len + RS_SPB - 1) / RS_SPB, n_signals), dim3(256), 0, st, ys, tab, rates, total_stretched, total_samples, out);
    DS_CHECK_LAUNCH("resample_sinc");
    return DS_OK;
}

static inline int peak_blocks(int max_len) {
    const int nb = (max_len + 4095) / 4096;
    return nb < 1 ? 1 : (nb > PN_NB_MAX ? PN_NB_MAX : nb);
}

extern "C" size_t ds_peak_normalize_ws_bytes(int n_signals, int max_len) { return n_signals > 0 && max_len > 0 ? (size_t)n_signals * peak_blocks(max_len) * 4 : 0; }

extern "C" int ds_peak_normalize(const float* x, const int32_t* tab, int n_signals, int max_len, long long total_samples, float* ws, float* out, void* stream) {
    DS_REQUIRE(x && tab && ws && out && n_signals > 0 && max_len > 0 && total_samples > 0, "peak_normalize: bad args (n_signals=%d max_len=%d total_samples=%lld)",
               n_signals, max_len, total_samples);
    DS_REQUIRE(n_signals <= 65535 && total_samples <= MAX_ELEMS, "peak_normalize: at most 65535 signals and 2^31 - 1 samples");
    if (!al4(x) || !al4(tab) || !al4(ws) || !al4(out)) DS_FAIL(DS_EALIGN, "peak_normalize: x / tab / ws / out must be 4-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int nb = peak_blocks(max_len);
#if DS_BOUNDS
    {
        DsBxHost h(DS_K_PEAK_NORMALIZE);
        h.set(DS_BX_SRC0, x, total_samples * 4);
        h.set(DS_BX_AUX0, tab, (long long)n_signals * DS_PV_NI * 4);
        h.set(DS_BX_AUX1, ws, (long long)n_signals * nb * 4);
        h.set(DS_BX_OUT, out, total_samples * 4);
        h.publish(st);
    }
#endif
    hipLaunchKernelGGL(peak_partial_kernel, dim3(nb, n_signals), dim3(256), 0, st, x, tab, total_samples, nb, ws);
    DS_CHECK_LAUNCH("peak_normalize (partials)");
    hipLaunchKernelGGL(peak_divide_kernel, dim3((max_len + RS_SPB - 1) / RS_SPB, n_signals), dim3(256), 0, st, x, tab, total_samples, nb, ws, out);
    DS_CHECK_LAUNCH("peak_normalize");
    return DS_OK;
}

template <bool SHAPED>
static int mix_launch(const char* name, const float* notes, long long total_samples, const int32_t* ev, int n_events, const int32_t* blk_ptr,
                      const int32_t* blk_ev, int n_blk_ev, float* track, int track_len, void* stream) {
    DS_REQUIRE(notes && ev && blk_ptr && blk_ev && track && total_samples > 0 && n_events > 0 && n_blk_ev >= 0 && track_len > 0,
               "%s: bad args (total_samples=%lld n_events=%d n_blk_ev=%d track_len=%d)", name, total_samples, n_events, n_blk_ev, track_len);
    DS_REQUIRE(total_samples <= MAX_ELEMS && track_len <= MAX_ELEMS - DS_MIX_BLOCK, "%s: at most 2^31 - 1 samples", name);
    DS_REQUIRE(!SHAPED || n_events <= MAX_ELEMS / DS_MX_NI, "%s: at most %lld events", name, MAX_ELEMS / DS_MX_NI);
    if (!al4(notes) || !al4(ev) || !al4(blk_ptr) || !al4(blk_ev) || !al4(track)) DS_FAIL(DS_EALIGN, "%s: every pointer must be 4-byte aligned", name);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int nblk = (track_len + RS_SPB - 1) / RS_SPB;
#if DS_BOUNDS
    {
        DsBxHost h(SHAPED ? DS_K_MIX_NOTES_SHAPED : DS_K_MIX_NOTES);
        h.set(DS_BX_SRC0, notes, total_samples * 4);
        h.set(DS_BX_AUX0, ev, (long long)n_events * (SHAPED ? DS_MX_NI : DS_MX_NI_PLAIN) * 4);
        h.set(DS_BX_AUX1, blk_ptr, (long long)(nblk + 1) * 4);
        h.set(DS_BX_AUX2, blk_ev, (long long)(n_blk_ev > 0 ? n_blk_ev : 1) * 4);
        h.set(DS_BX_OUT, track, (long long)track_len * 4);
        h.publish(st);
    }
#endif
    hipLaunchKernelGGL(mix_notes_kernel<SHAPED>, dim3(nblk), dim3(256), 0, st, notes, total_samples, ev, n_events, blk_ptr, blk_ev, n_blk_ev, track, track_len);
    DS_CHECK_LAUNCH(name);
    return DS_OK;
}

extern "C" int ds_mix_notes(const float* notes, long long total_samples, const int32_t* ev, int n_events, const int32_t* blk_ptr, const int32_t* blk_ev,
                            int n_blk_ev, float* track, int track_len, void* stream) {
    return mix_launch<false>("mix_notes", notes, total_samples, ev, n_events, blk_ptr, blk_ev, n_blk_ev, track, track_len, stream);
}

extern "C" int ds_mix_notes_shaped(const float* notes, long long total_samples, const int32_t* ev, int n_events, const int32_t* blk_ptr,
                                   const int32_t* blk_ev, int n_blk_ev, float* track, int track_len, void* stream) {
    return mix_launch<true>("mix_notes_shaped", notes, total_samples, ev, n_events, blk_ptr, blk_ev, n_blk_ev, track, track_len, stream);
}

#if DS_BOUNDS
extern "C" int ds_bounds_fetch_arranger(ds_bounds_rec* out, int reset) { return ds_bounds_fetch_tu(out, reset); }
#endif
