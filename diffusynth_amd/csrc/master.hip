// Mastering of a ragged batch of signals (gfx950): an RMS gain and a look-ahead limiter with a peak hold, the stage behind the sum of the
// arranger's tracks.  fp32 samples; definition (steps 1-7), table and stats layout in include/diffusynth_hip.h.
//
// ds_master_gain   step 1.  Signal s is reduced by nb = clamp(ceil(N / DS_MS_CHUNK), 1, DS_MS_MAX_PARTS) blocks: a thread adds the exact
//                  float64 squares of its samples in ascending order, the wave and the block add in a fixed order, and the block writes one
//                  (float64 sum, fp32 max) partial.  A second kernel, one block per signal, adds the nb partials in a fixed order and writes
//                  GAIN, RMS, PEAK, MIN_GAIN = 1 and limited = 0.  nb and every order depend on N alone.
// ds_master_limit  steps 2-7, block = one tile of DS_MS_TILE output samples of one signal.  With A = lookahead, R = hold, W = R + A + 1:
//                  rs[i] = r[t0 - A - R + i], i < T + R + 3 A, computed from x and GAIN as it loads (1 outside the signal);
//                  doubling in place: after step k, rs[i] = min r over 2^(k+1) samples from i; a thread keeps its own elements in registers
//                  and reads only its partners, so a step is one read, a barrier, one write, a barrier;  with d the largest power of two
//                  <= W:  ms[j] = min(rs[j], rs[j + W - d]) = m[t0 - A + j], j < T + 2 A;
//                  g = fp32(sum of ms[i .. i + 2 A] in float64 / (2 A + 1)), y = clamp(fl(g fl(gL x))), the stores, and the block's
//                  (min g, #{g < 1}) through one integer atomic each per wave that limited anything.
//                  A minimum does not depend on order and the float64 sum is exact inside the stated range: the bits are the definition's.
// ds_master_limit_tp  the same kernel with step 2's detector read from env, the true-peak envelope of x (csrc/true_peak.hip): one more
//                  template argument, the same LDS and grid.
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int MS_T = 256;                                 // threads per block
constexpr int TILE = DS_MS_TILE, MAX_A = DS_MS_MAX_LOOKAHEAD, MAX_R = DS_MS_MAX_HOLD;
constexpr int MS_MAX_LDS = 4 * (TILE + MAX_R + 3 * MAX_A) + 4 * (TILE + 2 * MAX_A);
constexpr int MS_NQ = (TILE + MAX_R + 3 * MAX_A + MS_T - 1) / MS_T;      // elements of the r tile a thread owns, at the caps
static_assert(MS_MAX_LDS <= 160 * 1024, "the two tiles fit a CU's LDS");
static_assert(DS_MS_MAX_PARTS <= 2 * MS_T, "the finishing block reads at most two partials per thread");

struct MsRow {
    int xoff, len;
};
__device__ __forceinline__ MsRow ms_row(const int32_t* tab, int s) {
    const int32_t* r = tab + (size_t)s * DS_PV_NI;
    MsRow o;
    o.xoff = DS_LD(int32_t, r + DS_PV_XOFF, DS_BX_AUX0);
    o.len = DS_LD(int32_t, r + DS_PV_LEN, DS_BX_AUX0);
    return o;
}
// a signal [off, off + n) of legal length inside a buffer of `total` elements
__device__ __forceinline__ bool fits(int off, int n, long long total) { return off >= 0 && n >= 1 && n <= DS_MS_MAX_LEN && (long long)off + n <= total; }

// partials of a signal of n samples: a function of n alone
__host__ __device__ inline int ms_parts(int n) {
    const int nb = (n + DS_MS_CHUNK - 1) / DS_MS_CHUNK;
    return nb < 1 ? 1 : (nb > DS_MS_MAX_PARTS ? DS_MS_MAX_PARTS : nb);
}

// ------------------------------------------------------------------------------------------------ gain
// ws = [n_signals][stride] float64 sums, then [n_signals][stride] fp32 maxima
__global__ __launch_bounds__(MS_T) void master_partial_kernel(const float* x, const int32_t* tab, long long total_samples, int stride, double* psum, float* pmax) {
    __shared__ double rsum[MS_T / 64];
    __shared__ float rmax[MS_T / 64];
    const MsRow r = ms_row(tab, blockIdx.y);
    if (!fits(r.xoff, r.len, total_samples)) return;
    const int nb = ms_parts(r.len);
    if ((int)blockIdx.x >= nb) return;
    double acc = 0.0;
    float mx = 0.f;
    for (int i = blockIdx.x * MS_T + threadIdx.x; i < r.len; i += nb * MS_T) {
        const float v = DS_LD(float, x + r.xoff + i, DS_BX_SRC0);
        const double d = (double)v;
        acc += d * d;
        mx = fmaxf(mx, fabsf(v));
    }
    acc = wave_sum(acc);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) {
        rsum[threadIdx.x >> 6] = acc;
        rmax[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const size_t o = (size_t)blockIdx.y * stride + blockIdx.x;
        DS_ST(double, psum + o, DS_BX_AUX1, (rsum[0] + rsum[1]) + (rsum[2] + rsum[3]));
        DS_ST(float, pmax + o, DS_BX_AUX2, fmaxf(fmaxf(rmax[0], rmax[1]), fmaxf(rmax[2], rmax[3])));
    }
}

__global__ __launch_bounds__(MS_T) void master_finish_kernel(const int32_t* tab, long long total_samples, int stride, const double* psum, const float* pmax,
                                                             float target_rms, float max_gain, float* stats, int32_t* limited) {
    __shared__ double rsum[MS_T / 64];
    __shared__ float rmax[MS_T / 64];
    const int s = blockIdx.x, tid = threadIdx.x;
    const MsRow r = ms_row(tab, s);
    if (!fits(r.xoff, r.len, total_samples)) return;
    const int nb = ms_parts(r.len);
    const size_t o = (size_t)s * stride;
    double acc = 0.0;
    float mx = 0.f;
    if (tid < nb) {
        acc = DS_LD(double, psum + o + tid, DS_BX_AUX1);
        mx = DS_LD(float, pmax + o + tid, DS_BX_AUX2);
    }
    if (tid + MS_T < nb) {
        acc += DS_LD(double, psum + o + tid + MS_T, DS_BX_AUX1);
        mx = fmaxf(mx, DS_LD(float, pmax + o + tid + MS_T, DS_BX_AUX2));
    }
    acc = wave_sum(acc);
    mx = wave_max(mx);
    if ((tid & 63) == 0) {
        rsum[tid >> 6] = acc;
        rmax[tid >> 6] = mx;
    }
    __syncthreads();
    if (tid == 0) {
        const double rms = sqrt(((rsum[0] + rsum[1]) + (rsum[2] + rsum[3])) / (double)r.len);
        float gain = 1.0f;
        if (target_rms > 0.f) {
            const double q = (double)target_rms / rms;               // silence: +inf, and the minimum is max_gain
            gain = (float)(q < (double)max_gain ? q : (double)max_gain);
        }
        float* st = stats + (size_t)s * DS_MS_NS;
        DS_ST(float, st + DS_MS_GAIN, DS_BX_STATS, gain);
        DS_ST(float, st + DS_MS_RMS, DS_BX_STATS, (float)rms);
        DS_ST(float, st + DS_MS_PEAK, DS_BX_STATS, fmaxf(fmaxf(rmax[0], rmax[1]), fmaxf(rmax[2], rmax[3])));
        DS_ST(float, st + DS_MS_MIN_GAIN, DS_BX_STATS, 1.0f);
        DS_ST(int32_t, limited + s, DS_BX_AUX3, 0);
    }
}

// ------------------------------------------------------------------------------------------------ limiter
// ENV: the detector of step 2 is fl(gL env[n]), the true-peak envelope of x (ds_true_peak), instead of |fl(gL x[n])|
template <bool ENV>
__global__ __launch_bounds__(MS_T) void master_limit_kernel(const float* x, const float* env, const int32_t* tab, long long total_samples, float c, int A, int R,
                                                            float* stats, int32_t* limited, float* out, int16_t* pcm) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int s = blockIdx.y, tid = threadIdx.x;
    const MsRow row = ms_row(tab, s);
    if (!fits(row.xoff, row.len, total_samples)) return;
    const long long b0 = (long long)blockIdx.x * TILE;
    if (b0 >= row.len) return;
    const int t0 = (int)b0;
    const int tn = row.len - t0 < TILE ? row.len - t0 : TILE;          // this block writes [t0, t0 + tn)
    const int nr = tn + R + 3 * A, nm = tn + 2 * A, W = R + A + 1;      // nr <= the launch's LDS: tn <= TILE
    float* rs = sm;
    float* ms = sm + (TILE + R + 3 * A);
    const float gl = DS_LD(float, stats + (size_t)s * DS_MS_NS + DS_MS_GAIN, DS_BX_STATS);
    const float* xg = x + row.xoff;

    // step 2 into LDS and into the owner's registers: element i is sample t0 - A - R + i
    float v[MS_NQ];
    const int base = t0 - A - R;
#pragma unroll
    for (int q = 0; q < MS_NQ; ++q) {
        const int i = tid + q * MS_T, n = base + i;
        float r = 1.0f;
        if (i < nr && n >= 0 && n < row.len) {
            const float au = ENV ? gl * DS_LD(float, env + row.xoff + n, DS_BX_SRC1) : fabsf(gl * DS_LD(float, xg + n, DS_BX_SRC0));
            if (au > c) r = __fdiv_rn(c, au);
        }
        if (i < nr) rs[i] = r;
        v[q] = r;
    }
    __syncthreads();
    // step 3: rs[i] = min over [i, i + d) for d = 2, 4, ... up to the largest power of two <= W (elements whose span leaves the tile keep
    // an older, shorter span: nothing below reads them)
    int d = 1;
    for (; 2 * d <= W; d *= 2) {
#pragma unroll
        for (int q = 0; q < MS_NQ; ++q) {
            const int i = tid + q * MS_T;
            if (i + d < nr) v[q] = fminf(v[q], rs[i + d]);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < MS_NQ; ++q) {
            const int i = tid + q * MS_T;
            if (i + d < nr) rs[i] = v[q];
        }
        __syncthreads();
    }
    // the window [j, j + W) as two spans of d: j + W - d + d - 1 <= nm - 1 + W - 1 = nr - 1
    for (int j = tid; j < nm; j += MS_T) ms[j] = fminf(rs[j], rs[j + W - d]);
    __syncthreads();

    // steps 4-7
    const double taps = (double)(2 * A + 1);
    float gmin = 1.0f;
    int cnt = 0;
    // one sample at a time, its taps in ascending order (a thread's 16 samples side by side, tap by tap, measured slower: DESIGN §7o)
    for (int i = tid; i < tn; i += MS_T) {
        double acc = 0.0;
#pragma unroll 8
        for (int k = 0; k <= 2 * A; ++k) acc += (double)ms[i + k];
        const float g = (float)(acc / taps);
        const float u = gl * DS_LD(float, xg + t0 + i, DS_BX_SRC0);
        float y = g * u;
        if (y > c) y = c;
        if (y < -c) y = -c;
        DS_ST(float, out + row.xoff + t0 + i, DS_BX_OUT, y);
        if (pcm) DS_ST(int16_t, pcm + row.xoff + t0 + i, DS_BX_RES, (int16_t)rintf(y * 32767.0f));
        if (g < 1.0f) {
            ++cnt;
            gmin = fminf(gmin, g);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        gmin = fminf(gmin, __shfl_xor(gmin, o, 64));
    }
    if ((tid & 63) == 0 && cnt > 0) {
        unsigned* pm = reinterpret_cast<unsigned*>(stats + (size_t)s * DS_MS_NS + DS_MS_MIN_GAIN);
#if DS_BOUNDS
        if (ds_bx_ok(pm, DS_BX_STATS, 4) && ds_bx_ok(limited + s, DS_BX_AUX3, 4))
#endif
        {
            atomicMin(pm, __float_as_uint(gmin));                       // g >= 0: the order of the bit patterns is the order of the values
            atomicAdd(limited + s, cnt);
        }
    }
}

inline bool al(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
constexpr long long MAX_ELEMS = (1ll << 31) - 1 - TILE;         // the table's offsets are int32, and t0 + i must not wrap

}  // namespace

extern "C" size_t ds_master_ws_bytes(int n_signals, int max_len) {
    return n_signals > 0 && max_len > 0 && max_len <= DS_MS_MAX_LEN ? (size_t)n_signals * ms_parts(max_len) * 12 : 0;
}

extern "C" int ds_master_gain(const float* x, const int32_t* tab, int n_signals, int max_len, long long total_samples, float target_rms, float max_gain,
                              void* ws, float* stats, int32_t* limited, void* stream) {
    DS_REQUIRE(x && tab && ws && stats && limited && n_signals > 0 && max_len > 0 && total_samples > 0,
               "master_gain: bad args (n_signals=%d max_len=%d total_samples=%lld)", n_signals, max_len, total_samples);
    DS_REQUIRE(n_signals <= 65535 && max_len <= DS_MS_MAX_LEN && total_samples <= MAX_ELEMS,
               "master_gain: at most 65535 signals of %d samples and 2^31 - 1 - %d samples in all", DS_MS_MAX_LEN, TILE);
    DS_REQUIRE(max_gain > 0.f && max_gain <= 3.0e38f && target_rms <= 3.0e38f, "master_gain: max_gain must be positive and finite, target_rms finite (<= 0: none)");
    if (!al(x, 4) || !al(tab, 4) || !al(stats, 4) || !al(limited, 4) || !al(ws, 8)) DS_FAIL(DS_EALIGN, "master_gain: x / tab / stats / limited 4-byte, ws 8-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int stride = ms_parts(max_len);
    double* psum = reinterpret_cast<double*>(ws);
    float* pmax = reinterpret_cast<float*>(psum + (size_t)n_signals * stride);
#if DS_BOUNDS
    {
        DsBxHost h(DS_K_MASTER_GAIN);
        h.set(DS_BX_SRC0, x, total_samples * 4);
        h.set(DS_BX_AUX0, tab, (long long)n_signals * DS_PV_NI * 4);
        h.set(DS_BX_AUX1, psum, (long long)n_signals * stride * 8);
        h.set(DS_BX_AUX2, pmax, (long long)n_signals * stride * 4);
        h.set(DS_BX_STATS, stats, (long long)n_signals * DS_MS_NS * 4);
        h.set(DS_BX_AUX3, limited, (long long)n_signals * 4);
        h.publish(st);
    }
#endif
    hipLaunchKernelGGL(master_partial_kernel, dim3(stride, n_signals), dim3(MS_T), 0, st, x, tab, total_samples, stride, psum, pmax);
    DS_CHECK_LAUNCH("master_gain (partials)");
    hipLaunchKernelGGL(master_finish_kernel, dim3(n_signals), dim3(MS_T), 0, st, tab, total_samples, stride, psum, pmax, target_rms, max_gain, stats, limited);
    DS_CHECK_LAUNCH("master_gain");
    return DS_OK;
}

namespace {

// ds_master_limit (env == nullptr) and ds_master_limit_tp: one set of checks, one launch
template <bool ENV>
int master_limit_launch(const char* who, int kernel_id, const float* x, const float* env, const int32_t* tab, int n_signals, int max_len, long long total_samples,
                        float ceiling, int lookahead, int hold, float* stats, int32_t* limited, float* out, int16_t* pcm, void* stream) {
    DS_REQUIRE(x && (!ENV || env) && tab && stats && limited && out && n_signals > 0 && max_len > 0 && total_samples > 0,
               "%s: bad args (n_signals=%d max_len=%d total_samples=%lld)", who, n_signals, max_len, total_samples);
    DS_REQUIRE(n_signals <= 65535 && max_len <= DS_MS_MAX_LEN && total_samples <= MAX_ELEMS,
               "%s: at most 65535 signals of %d samples and 2^31 - 1 - %d samples in all", who, DS_MS_MAX_LEN, TILE);
    DS_REQUIRE(lookahead >= 0 && lookahead <= MAX_A && hold >= lookahead && hold <= MAX_R,
               "%s: 0 <= lookahead <= %d and lookahead <= hold <= %d samples (lookahead=%d hold=%d)", who, MAX_A, MAX_R, lookahead, hold);
    DS_REQUIRE(ceiling > 0.f && ceiling <= 1.f, "%s: the ceiling must be inside (0, 1] (ceiling=%g)", who, (double)ceiling);
    DS_REQUIRE((const void*)out != (const void*)x && (!ENV || (const void*)out != (const void*)env),
               "%s: out may not be x%s (a tile reads its neighbours' inputs)", who, ENV ? " or env" : "");
    if (!al(x, 4) || !al(env, 4) || !al(tab, 4) || !al(stats, 4) || !al(limited, 4) || !al(out, 4) || !al(pcm, 2))
        DS_FAIL(DS_EALIGN, "%s: x /%s tab / stats / limited / out 4-byte, pcm 2-byte aligned", who, ENV ? " env /" : "");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#if DS_BOUNDS
    {
        DsBxHost h(kernel_id);
        h.set(DS_BX_SRC0, x, total_samples * 4);
        h.set(DS_BX_SRC1, env, total_samples * 4);
        h.set(DS_BX_AUX0, tab, (long long)n_signals * DS_PV_NI * 4);
        h.set(DS_BX_STATS, stats, (long long)n_signals * DS_MS_NS * 4);
        h.set(DS_BX_AUX3, limited, (long long)n_signals * 4);
        h.set(DS_BX_OUT, out, total_samples * 4);
        h.set(DS_BX_RES, pcm, total_samples * 2);
        h.publish(st);
    }
#else
    (void)kernel_id;
#endif
    DS_SET_MAX_LDS(master_limit_kernel<ENV>, MS_MAX_LDS, who);
    const size_t lds = 4 * ((size_t)TILE + hold + 3 * lookahead) + 4 * ((size_t)TILE + 2 * lookahead);
    hipLaunchKernelGGL(master_limit_kernel<ENV>, dim3((max_len + TILE - 1) / TILE, n_signals), dim3(MS_T), lds, st, x, env, tab, total_samples, ceiling, lookahead,
                       hold, stats, limited, out, pcm);
    DS_CHECK_LAUNCH(who);
    return DS_OK;
}

}  // namespace

extern "C" int ds_master_limit(const float* x, const int32_t* tab, int n_signals, int max_len, long long total_samples, float ceiling, int lookahead,
                               int hold, float* stats, int32_t* limited, float* out, int16_t* pcm, void* stream) {
    return master_limit_launch<false>("master_limit", DS_K_MASTER_LIMIT, x, nullptr, tab, n_signals, max_len, total_samples, ceiling, lookahead, hold, stats, limited,
                                      out, pcm, stream);
}

extern "C" int ds_master_limit_tp(const float* x, const float* env, const int32_t* tab, int n_signals, int max_len, long long total_samples, float ceiling,
                                  int lookahead, int hold, float* stats, int32_t* limited, float* out, int16_t* pcm, void* stream) {
    return master_limit_launch<true>("master_limit_tp", DS_K_MASTER_LIMIT_TP, x, env, tab, n_signals, max_len, total_samples, ceiling, lookahead, hold, stats,
                                     limited, out, pcm, stream);
}

#if DS_BOUNDS
extern "C" int ds_bounds_fetch_master(ds_bounds_rec* out, int reset) { return ds_bounds_fetch_tu(out, reset); }
#endif
