// K-weighted gated loudness (BS.1770) of a ragged batch of mono signals (gfx950), and the gain that takes a signal to a loudness target.
// fp32 samples, float64 arithmetic throughout; definition, coefficient layout and outputs in include/diffusynth_hip.h ("loudness").
//
// The two biquads are one linear recursion with a state of four float64 values (transposed direct form II: two per stage).  A signal is cut
// at every hop boundary (h samples, 100 ms), a hop into nc = ceil(h / Lc) chunks of Lc = ceil(h / 256) | 1 samples (the last one shorter):
// a block of 256 threads is one hop, a thread one chunk.
//   lu_hop_kernel<false>  stages the hop in LDS (lanes read consecutive words), runs every chunk from zero state, carries the end states
//                         along the hop by a Kogge-Stone scan (step k: state[t] += P^(2^k) state[t - 2^k], P = the transition over Lc
//                         samples, all eight powers from the host) and writes the hop's end state from zero, E_i.
//   lu_carry_kernel       one wave per signal walks the hops: G_0 = 0, G_(i+1) = Q G_i + E_i, Q = the transition over h samples.
//   lu_hop_kernel<true>   the same staging, zero-state run and scan, now with chunk 0's end state started from G_i: every chunk has its true
//                         start state, runs again from it and adds the squares of its outputs in ascending order; the wave and the block add
//                         in a fixed order -> q_i.
//   lu_finish_kernel      one block per signal: z_j from four q, the two gates in the energy domain (three fixed-order reductions), the
//                         logarithms of the results.
// Lc is odd, so the 64 lanes of a wave (stride Lc words) read 64 different LDS banks.  Everything depends on (N, h) alone: a signal has the
// same bits alone and inside any batch.  No float atomics.
#include <math.h>

#include "common.hpp"

namespace {

constexpr int LU_T = DS_LU_THREADS;
static_assert(LU_T == 256 && (1 << DS_LU_SCAN_STEPS) == LU_T, "the scan covers the block in DS_LU_SCAN_STEPS doublings");
static_assert(DS_LU_C_PSCAN + 16 * DS_LU_SCAN_STEPS == DS_LU_NCOEF && DS_LU_NCOEF * 8 <= 2048, "the coefficients travel as a kernel argument");
static_assert(4 * DS_LU_MAX_HOP + 2 * LU_T * 32 + 64 <= 160 * 1024, "a hop and the scan's two buffers fit a CU's LDS");

struct LuCoef {
    double c[DS_LU_NCOEF];
};
struct St {
    double v[4];
};

struct LuRow {
    int xoff, len, boff;
};
__device__ __forceinline__ LuRow lu_row(const int32_t* tab, int s) {
    const int32_t* r = tab + (size_t)s * DS_PV_NI;
    LuRow o;
    o.xoff = DS_LD(int32_t, r + DS_PV_XOFF, DS_BX_AUX0);
    o.len = DS_LD(int32_t, r + DS_PV_LEN, DS_BX_AUX0);
    o.boff = DS_LD(int32_t, r + DS_LU_TAB_BOFF, DS_BX_AUX0);
    return o;
}
__host__ __device__ inline int lu_blocks(int len, int h) { return len / h > 3 ? len / h - 3 : 0; }
// a signal [off, off + n) of legal length (at most the launch's max_len: the workspace is laid out for it) inside a buffer of `total`
// elements, and (where the block energies are wanted) its blocks inside theirs
__device__ __forceinline__ bool fits(const LuRow& r, long long total, int max_len, int h, bool want_blocks, long long total_blocks) {
    if (!(r.xoff >= 0 && r.len >= 1 && r.len <= max_len && (long long)r.xoff + r.len <= total)) return false;
    return !want_blocks || (r.boff >= 0 && (long long)r.boff + lu_blocks(r.len, h) <= total_blocks);
}
__host__ __device__ inline int lu_chunk(int h) { return ((h + LU_T - 1) / LU_T) | 1; }

// one sample through both stages
__device__ __forceinline__ double lu_step(const LuCoef& K, St& s, double x) {
    const double y1 = K.c[DS_LU_C_B1] * x + s.v[0];
    s.v[0] = (K.c[DS_LU_C_B1 + 1] * x - K.c[DS_LU_C_A1] * y1) + s.v[1];
    s.v[1] = K.c[DS_LU_C_B1 + 2] * x - K.c[DS_LU_C_A1 + 1] * y1;
    const double y2 = K.c[DS_LU_C_B2] * y1 + s.v[2];
    s.v[2] = (K.c[DS_LU_C_B2 + 1] * y1 - K.c[DS_LU_C_A2] * y2) + s.v[3];
    s.v[3] = K.c[DS_LU_C_B2 + 2] * y1 - K.c[DS_LU_C_A2 + 1] * y2;
    return y2;
}
// a += M b, M = the 4 x 4 matrix at K.c[OFF] (row-major)
template <int OFF> __device__ __forceinline__ void lu_madd(const LuCoef& K, St& a, const St& b) {
#pragma unroll
    for (int r = 0; r < 4; ++r) a.v[r] += ((K.c[OFF + 4 * r] * b.v[0] + K.c[OFF + 4 * r + 1] * b.v[1]) + (K.c[OFF + 4 * r + 2] * b.v[2] + K.c[OFF + 4 * r + 3] * b.v[3]));
}
template <int STEP> __device__ __forceinline__ void lu_scan_step(const LuCoef& K, St& cur, St (*buf)[LU_T], int nc, int tid) {
    constexpr int D = 1 << STEP;
    if (D < nc) {                                                // uniform over the block
        buf[STEP & 1][tid] = cur;
        __syncthreads();
        if (tid >= D) lu_madd<DS_LU_C_PSCAN + 16 * STEP>(K, cur, buf[STEP & 1][tid - D]);
    }
}

// ws of n signals with `stride` hops each: E [n][stride][4], G [n][stride][4], q [n][stride], float64
struct LuWs {
    double *E, *G, *q;
};
__host__ __device__ inline LuWs lu_ws(void* ws, int n, int stride) {
    LuWs o;
    o.E = reinterpret_cast<double*>(ws);
    o.G = o.E + (size_t)n * stride * 4;
    o.q = o.G + (size_t)n * stride * 4;
    return o;
}

// ------------------------------------------------------------------------------------------------ a hop
template <bool SECOND>
__global__ __launch_bounds__(LU_T) void lu_hop_kernel(const float* x, const int32_t* tab, long long total_samples, const LuCoef K, int max_len, int h, int stride,
                                                       LuWs w, bool want_blocks, long long total_blocks) {
    extern __shared__ __attribute__((aligned(16))) float sx[];
    __shared__ St buf[2][LU_T];
    __shared__ double rsum[LU_T / 64];
    const int s = blockIdx.y, i = blockIdx.x, tid = threadIdx.x;
    const LuRow row = lu_row(tab, s);
    if (!fits(row, total_samples, max_len, h, want_blocks, total_blocks)) return;
    const int nh = row.len / h;
    if (nh < 4 || i >= nh) return;                               // fewer than four hops: no block, nothing to filter
    const float* xg = x + row.xoff + (size_t)i * h;              // (i + 1) h <= len
    for (int j = tid; j < h; j += LU_T) sx[j] = DS_LD(float, xg + j, DS_BX_SRC0);
    __syncthreads();

    const int Lc = lu_chunk(h), nc = (h + Lc - 1) / Lc;           // nc <= LU_T
    const int n0 = tid * Lc, len = tid < nc ? (h - n0 < Lc ? h - n0 : Lc) : 0;
    St e = {{0.0, 0.0, 0.0, 0.0}};
    for (int k = 0; k < len; ++k) (void)lu_step(K, e, (double)sx[n0 + k]);
    St g = {{0.0, 0.0, 0.0, 0.0}};
    if (SECOND) {
        const size_t o = ((size_t)s * stride + i) * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) g.v[r] = DS_LD(double, w.G + o + r, DS_BX_AUX1);
        if (tid == 0) {                                          // chunk 0 from the hop's true start state
            if (nc > 1) lu_madd<DS_LU_C_PSCAN>(K, e, g);
            else lu_madd<DS_LU_C_PTAIL>(K, e, g);
        }
    }
    // inclusive scan over the full-length chunks: cur[t] = the state behind chunk t (the short last chunk's own value is not used)
    St cur = e;
    lu_scan_step<0>(K, cur, buf, nc, tid);
    lu_scan_step<1>(K, cur, buf, nc, tid);
    lu_scan_step<2>(K, cur, buf, nc, tid);
    lu_scan_step<3>(K, cur, buf, nc, tid);
    lu_scan_step<4>(K, cur, buf, nc, tid);
    lu_scan_step<5>(K, cur, buf, nc, tid);
    lu_scan_step<6>(K, cur, buf, nc, tid);
    lu_scan_step<7>(K, cur, buf, nc, tid);
    __syncthreads();                                             // the last step's reads are over (it may have read buf[0])
    buf[0][tid] = cur;
    __syncthreads();
    St st = g;
    if (tid > 0) st = buf[0][tid - 1];

    if (!SECOND) {
        if (tid == nc - 1) {                                     // the hop's end state from zero: the last chunk's own plus its start carried over it
            if (nc > 1) lu_madd<DS_LU_C_PTAIL>(K, e, st);
            const size_t o = ((size_t)s * stride + i) * 4;
#pragma unroll
            for (int r = 0; r < 4; ++r) DS_ST(double, w.E + o + r, DS_BX_AUX1, e.v[r]);
        }
    } else {
        double acc = 0.0;
        for (int k = 0; k < len; ++k) {
            const double y = lu_step(K, st, (double)sx[n0 + k]);
            acc += y * y;
        }
        acc = wave_sum(acc);
        if ((tid & 63) == 0) rsum[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) DS_ST(double, w.q + (size_t)s * stride + i, DS_BX_AUX1, (rsum[0] + rsum[1]) + (rsum[2] + rsum[3]));
    }
}

// ------------------------------------------------------------------------------------------------ the carry along a signal
__global__ __launch_bounds__(64) void lu_carry_kernel(const int32_t* tab, long long total_samples, const LuCoef K, int max_len, int h, int stride, LuWs w,
                                                       bool want_blocks, long long total_blocks) {
    __shared__ St sE[64], sG[64];
    const int s = blockIdx.x, lane = threadIdx.x;
    const LuRow row = lu_row(tab, s);
    if (!fits(row, total_samples, max_len, h, want_blocks, total_blocks)) return;
    const int nh = row.len / h;
    if (nh < 4) return;
    const size_t o = (size_t)s * stride * 4;
    St g = {{0.0, 0.0, 0.0, 0.0}};
    for (int base = 0; base < nh; base += 64) {
        const int n = nh - base < 64 ? nh - base : 64;
        if (lane < n) {
#pragma unroll
            for (int r = 0; r < 4; ++r) sE[lane].v[r] = DS_LD(double, w.E + o + (size_t)(base + lane) * 4 + r, DS_BX_AUX1);
        }
        __syncthreads();
        if (lane == 0) {
            for (int j = 0; j < n; ++j) {
                sG[j] = g;
                St nx = sE[j];
                lu_madd<DS_LU_C_PHOP>(K, nx, g);
                g = nx;
            }
        }
        __syncthreads();
        if (lane < n) {
#pragma unroll
            for (int r = 0; r < 4; ++r) DS_ST(double, w.G + o + (size_t)(base + lane) * 4 + r, DS_BX_AUX1, sG[lane].v[r]);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ blocks, gates, results
__device__ __forceinline__ double lu_block_sum(double v, double* red, int tid) {
    v = wave_sum(v);
    __syncthreads();                                             // the last use of red is over
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ double lu_lufs(double z) { return z > 0.0 ? -0.691 + 10.0 * log10(z) : -INFINITY; }

__global__ __launch_bounds__(LU_T) void lu_finish_kernel(const int32_t* tab, long long total_samples, int max_len, int h, int stride, LuWs w, double z_abs, double* lu,
                                                          int32_t* cnt, double* blocks, long long total_blocks) {
    __shared__ double red[LU_T / 64];
    const int s = blockIdx.x, tid = threadIdx.x;
    const LuRow row = lu_row(tab, s);
    if (!fits(row, total_samples, max_len, h, blocks != nullptr, total_blocks)) return;
    const int nb = lu_blocks(row.len, h);
    const double* q = w.q + (size_t)s * stride;
    const double span = 4.0 * (double)h;
    double s1 = 0.0, c1 = 0.0, mx = 0.0;
    for (int j = tid; j < nb; j += LU_T) {
        const double z = ((DS_LD(double, q + j, DS_BX_AUX1) + DS_LD(double, q + j + 1, DS_BX_AUX1)) +
                          (DS_LD(double, q + j + 2, DS_BX_AUX1) + DS_LD(double, q + j + 3, DS_BX_AUX1))) / span;
        if (blocks) DS_ST(double, blocks + row.boff + j, DS_BX_RES, z);
        if (z > z_abs) {
            s1 += z;
            c1 += 1.0;
        }
        mx = z > mx ? z : mx;
    }
    s1 = lu_block_sum(s1, red, tid);
    c1 = lu_block_sum(c1, red, tid);                             // (counts below 2^24: exact)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double m = __shfl_xor(mx, o, 64);
        mx = m > mx ? m : mx;
    }
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    const double m01 = red[0] > red[1] ? red[0] : red[1], m23 = red[2] > red[3] ? red[2] : red[3];
    mx = m01 > m23 ? m01 : m23;
    const double z_rel = c1 > 0.0 ? 0.1 * (s1 / c1) : 0.0;
    double s2 = 0.0, c2 = 0.0;
    for (int j = tid; j < nb; j += LU_T) {
        const double z = ((DS_LD(double, q + j, DS_BX_AUX1) + DS_LD(double, q + j + 1, DS_BX_AUX1)) +
                          (DS_LD(double, q + j + 2, DS_BX_AUX1) + DS_LD(double, q + j + 3, DS_BX_AUX1))) / span;
        if (z > z_abs && z > z_rel) {
            s2 += z;
            c2 += 1.0;
        }
    }
    s2 = lu_block_sum(s2, red, tid);
    c2 = lu_block_sum(c2, red, tid);
    if (tid == 0) {
        const double Z = c2 > 0.0 ? s2 / c2 : 0.0;
        double* o = lu + (size_t)s * DS_LU_NS;
        DS_ST(double, o + DS_LU_ENERGY, DS_BX_OUT, Z);
        DS_ST(double, o + DS_LU_INTEGRATED, DS_BX_OUT, lu_lufs(Z));
        DS_ST(double, o + DS_LU_MOMENTARY_MAX, DS_BX_OUT, lu_lufs(mx));
        DS_ST(double, o + DS_LU_THRESHOLD, DS_BX_OUT, lu_lufs(z_rel));
        int32_t* c = cnt + (size_t)s * 3;
        DS_ST(int32_t, c, DS_BX_AUX2, nb);
        DS_ST(int32_t, c + 1, DS_BX_AUX2, (int32_t)c1);
        DS_ST(int32_t, c + 2, DS_BX_AUX2, (int32_t)c2);
    }
}

// ------------------------------------------------------------------------------------------------ the gain
__global__ void lu_gain_kernel(const double* lu, int n_signals, double zt, float max_gain, float* stats) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_signals) return;
    const double Z = DS_LD(double, lu + (size_t)s * DS_LU_NS + DS_LU_ENERGY, DS_BX_SRC0);
    float g = 1.0f;
    if (Z > 0.0) {
        const double r = __dsqrt_rn(__ddiv_rn(zt, Z));
        g = (float)(r < (double)max_gain ? r : (double)max_gain);
    }
    DS_ST(float, stats + (size_t)s * DS_MS_NS + DS_MS_GAIN, DS_BX_STATS, g);
}

inline bool al(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
constexpr long long MAX_ELEMS = (1ll << 31) - 1;                 // the table's offsets are int32
inline int lu_stride(int max_len, int h) { return max_len / h > 0 ? max_len / h : 1; }

}  // namespace

extern "C" size_t ds_loudness_ws_bytes(int n_signals, int max_len, int h) {
    if (!(n_signals > 0 && max_len > 0 && max_len <= DS_MS_MAX_LEN && h >= DS_LU_MIN_HOP && h <= DS_LU_MAX_HOP)) return 0;
    return (size_t)n_signals * lu_stride(max_len, h) * 9 * 8;
}

extern "C" int ds_loudness(const float* x, const int32_t* tab, int n_signals, int max_len, long long total_samples, const double* coef, int h, double z_abs,
                           void* ws, double* lu, int32_t* cnt, double* blocks, long long total_blocks, void* stream) {
    DS_REQUIRE(x && tab && coef && ws && lu && cnt && n_signals > 0 && max_len > 0 && total_samples > 0,
               "loudness: bad args (n_signals=%d max_len=%d total_samples=%lld)", n_signals, max_len, total_samples);
    DS_REQUIRE(n_signals <= 65535 && max_len <= DS_MS_MAX_LEN && total_samples <= MAX_ELEMS, "loudness: at most 65535 signals of %d samples and 2^31 - 1 samples in all",
               DS_MS_MAX_LEN);
    DS_REQUIRE(h >= DS_LU_MIN_HOP && h <= DS_LU_MAX_HOP, "loudness: the hop h must be inside [%d, %d] samples (h=%d)", DS_LU_MIN_HOP, DS_LU_MAX_HOP, h);
    DS_REQUIRE(z_abs >= 0.0 && z_abs <= 1.0e300, "loudness: z_abs must be finite and not negative (z_abs=%g)", z_abs);
    DS_REQUIRE(!blocks || (total_blocks > 0 && total_blocks <= MAX_ELEMS), "loudness: blocks needs 0 < total_blocks < 2^31 (total_blocks=%lld)", total_blocks);
    LuCoef K;
    for (int i = 0; i < DS_LU_NCOEF; ++i) {
        K.c[i] = coef[i];
        DS_REQUIRE(K.c[i] - K.c[i] == 0.0, "loudness: coef[%d] is not finite", i);
    }
    if (!al(x, 4) || !al(tab, 4) || !al(cnt, 4) || !al(ws, 8) || !al(lu, 8) || !al(blocks, 8) || !al(coef, 8))
        DS_FAIL(DS_EALIGN, "loudness: x / tab / cnt 4-byte, coef / ws / lu / blocks 8-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int stride = lu_stride(max_len, h);
    const LuWs w = lu_ws(ws, n_signals, stride);
    const bool want_blocks = blocks != nullptr;
#if DS_BOUNDS
    {
        DsBxHost b(DS_K_LOUDNESS);
        b.set(DS_BX_SRC0, x, total_samples * 4);
        b.set(DS_BX_AUX0, tab, (long long)n_signals * DS_PV_NI * 4);
        b.set(DS_BX_AUX1, ws, (long long)n_signals * stride * 9 * 8);
        b.set(DS_BX_OUT, lu, (long long)n_signals * DS_LU_NS * 8);
        b.set(DS_BX_AUX2, cnt, (long long)n_signals * 3 * 4);
        b.set(DS_BX_RES, blocks, total_blocks * 8);
        b.publish(st);
    }
#endif
    const size_t lds = (size_t)h * 4;
    if (max_len / h >= 4) {                                       // otherwise no signal has a block
        DS_SET_MAX_LDS(lu_hop_kernel<false>, DS_LU_MAX_HOP * 4, "loudness (first pass)");
        DS_SET_MAX_LDS(lu_hop_kernel<true>, DS_LU_MAX_HOP * 4, "loudness (second pass)");
        hipLaunchKernelGGL(lu_hop_kernel<false>, dim3(stride, n_signals), dim3(LU_T), lds, st, x, tab, total_samples, K, max_len, h, stride, w, want_blocks, total_blocks);
        DS_CHECK_LAUNCH("loudness (first pass)");
        hipLaunchKernelGGL(lu_carry_kernel, dim3(n_signals), dim3(64), 0, st, tab, total_samples, K, max_len, h, stride, w, want_blocks, total_blocks);
        DS_CHECK_LAUNCH("loudness (carry)");
        hipLaunchKernelGGL(lu_hop_kernel<true>, dim3(stride, n_signals), dim3(LU_T), lds, st, x, tab, total_samples, K, max_len, h, stride, w, want_blocks, total_blocks);
        DS_CHECK_LAUNCH("loudness (second pass)");
    }
    hipLaunchKernelGGL(lu_finish_kernel, dim3(n_signals), dim3(LU_T), 0, st, tab, total_samples, max_len, h, stride, w, z_abs, lu, cnt, blocks, total_blocks);
    DS_CHECK_LAUNCH("loudness");
    return DS_OK;
}

extern "C" int ds_loudness_gain(const double* lu, int n_signals, double zt, float max_gain, float* stats, void* stream) {
    DS_REQUIRE(lu && stats && n_signals > 0 && n_signals <= 65535, "loudness_gain: bad args (n_signals=%d)", n_signals);
    DS_REQUIRE(zt > 0.0 && zt <= 1.0e300 && max_gain > 0.f && max_gain <= 3.0e38f, "loudness_gain: zt and max_gain must be positive and finite (zt=%g max_gain=%g)", zt,
               (double)max_gain);
    if (!al(lu, 8) || !al(stats, 4)) DS_FAIL(DS_EALIGN, "loudness_gain: lu 8-byte, stats 4-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#if DS_BOUNDS
    {
        DsBxHost b(DS_K_LOUDNESS_GAIN);
        b.set(DS_BX_SRC0, lu, (long long)n_signals * DS_LU_NS * 8);
        b.set(DS_BX_STATS, stats, (long long)n_signals * DS_MS_NS * 4);
        b.publish(st);
    }
#endif
    hipLaunchKernelGGL(lu_gain_kernel, dim3((n_signals + 255) / 256), dim3(256), 0, st, lu, n_signals, zt, max_gain, stats);
    DS_CHECK_LAUNCH("loudness_gain");
    return DS_OK;
}

#if DS_BOUNDS
extern "C" int ds_bounds_fetch_loudness(ds_bounds_rec* out, int reset) { return ds_bounds_fetch_tu(out, reset); }
#endif
