// Sample-rate conversion of a ragged batch (gfx950): scipy.signal.resample_poly(x, up, down) with its defaults — what
// librosa.resample(res_type="polyphase") is, and what tools.adjust_audio_length (tools.py:126-151) means in this package — fused with its
// crop / zero-pad to a stated length.  fp32; definition and table layout in include/diffusynth_hip.h.
//
//   y[m] = sum_n x[n] h[HALF + m DOWN - n UP],  0 <= n < LEN, tap index inside [0, 2 HALF];  out[m] = y[m] for m < min(OLEN, NRES), else 0.
//
// A signal is one row of a device table (int32 [n][DS_RP_NI]); each row names its own UP, DOWN, HALF and the place of its 2 HALF + 1 fp32 taps
// in one filter buffer (designed on the host in float64, one per distinct (UP, DOWN), shared by the rows of that pair).  Everything the host
// can floor, ceil or divide it does, in integers (NRES, OLEN, the outputs per block); what is left to the device is the one division that says
// which input sample and which phase an output starts from, done once per thread in 64 bits — the following outputs of the thread advance by
// (256 DOWN) div UP and (256 DOWN) mod UP with a carry.  m DOWN and n UP are 64-bit products: nothing wraps.
//
// ds_resample_poly   block = 256 threads = BLK consecutive outputs of one signal (BLK <= 1024 from the row: the host shrinks it for steep
//                    decimations so that the block's input span fits `span` floats).  The signal's filter and the block's input span are
//                    staged in LDS; thread t owns outputs m0 + t, m0 + t + 256, ...  Per output the taps are walked in ascending tap index
//                    (descending n): acc = fma(x[n], h[k], acc), k = phase, phase + UP, ...: one LDS read of a tap, one of a sample, one FMA.
//                    The filter keeps its natural (strided) layout: lane l of a wave reads tap phase_l + j UP with
//                    phase_l = (HALF + m_l DOWN) mod UP, so the bank (dword address mod 32 per half wave for ds_read_b32) depends on
//                    phase_l alone — a by-phase layout permutes the same residues and conflicts exactly as often.
// No atomics: an output has one owner and one summation order, whatever else is in the launch.
#include "common.hpp"

namespace {

constexpr int RP_T = 256;                                // threads per block
constexpr int MAX_TAPS = DS_RP_MAX_TAPS, MAX_SPAN = DS_RP_MAX_SPAN, MAX_BLK = DS_RP_MAX_BLK;
constexpr int RP_MAX_LDS = (MAX_TAPS + MAX_SPAN) * 4;

struct RpRow {
    int xoff, len, ooff, olen, nres, up, down, half, hoff, blk;
};
__device__ __forceinline__ RpRow rp_row(const int32_t* tab, int s) {
    const int32_t* r = tab + (size_t)s * DS_RP_NI;
    RpRow o;
    o.xoff = DS_LD(int32_t, r + DS_RP_XOFF, DS_BX_AUX0);
    o.len = DS_LD(int32_t, r + DS_RP_LEN, DS_BX_AUX0);
    o.ooff = DS_LD(int32_t, r + DS_RP_OOFF, DS_BX_AUX0);
    o.olen = DS_LD(int32_t, r + DS_RP_OLEN, DS_BX_AUX0);
    o.nres = DS_LD(int32_t, r + DS_RP_NRES, DS_BX_AUX0);
    o.up = DS_LD(int32_t, r + DS_RP_UP, DS_BX_AUX0);
    o.down = DS_LD(int32_t, r + DS_RP_DOWN, DS_BX_AUX0);
    o.half = DS_LD(int32_t, r + DS_RP_HALF, DS_BX_AUX0);
    o.hoff = DS_LD(int32_t, r + DS_RP_HOFF, DS_BX_AUX0);
    o.blk = DS_LD(int32_t, r + DS_RP_BLK, DS_BX_AUX0);
    return o;
}
// a range [off, off + n) inside a buffer of `total` elements
__device__ __forceinline__ bool fits(int off, int n, long long total) { return off >= 0 && n >= 0 && (long long)off + n <= total; }

__global__ __launch_bounds__(RP_T) void resample_poly_kernel(const float* x, const int32_t* tab, const float* filt, long long total_in, long long total_out,
                                                             long long total_filt, int max_taps, int span, float* out) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *hs = sm, *xs = sm + max_taps;
    const int tid = threadIdx.x;
    const RpRow r = rp_row(tab, blockIdx.y);
    // (UP, DOWN < 2^16 keeps 256 DOWN and a span's worth of UP inside int32; a pair that fits MAX_TAPS is far below)
    if (r.up < 1 || r.down < 1 || r.up > 65535 || r.down > 65535 || r.half < 1 || r.half > (max_taps - 1) / 2 || r.blk < 1 || r.blk > MAX_BLK || r.nres < 0) return;
    const int nt = 2 * r.half + 1;
    if (!fits(r.xoff, r.len, total_in) || !fits(r.ooff, r.olen, total_out) || !fits(r.hoff, nt, total_filt)) return;
    const long long b0 = (long long)blockIdx.x * r.blk;
    if (b0 >= r.olen) return;
    const int m0 = (int)b0;
    const int m1 = r.olen - m0 < r.blk ? r.olen : m0 + r.blk;           // this block writes [m0, m1)
    const int mr = m1 < r.nres ? m1 : r.nres;                           // and computes [m0, mr); zeros behind
    int n_lo = 0, cnt = 0;
    if (mr > m0) {
        // the block's inputs: ceil((m0 DOWN - HALF) / UP) <= n <= floor((HALF + (mr - 1) DOWN) / UP), inside the signal
        const long long tlo = (long long)m0 * r.down - r.half, thi = (long long)r.half + (long long)(mr - 1) * r.down;
        const long long lo = tlo <= 0 ? 0 : (tlo + r.up - 1) / r.up;
        long long hi = thi / r.up;
        hi = hi < r.len ? hi : (long long)r.len - 1;
        if (hi - lo + 1 > span) return;                                 // a BLK the host did not size to `span`: the row does not fit
        if (hi >= lo) {
            n_lo = (int)lo;
            cnt = (int)(hi - lo + 1);
        }
    }
    if (cnt > 0) {                                                      // (uniform for the block: every thread reaches the barrier or none)
        const float* hg = filt + r.hoff;
        for (int k = tid; k < nt; k += RP_T) hs[k] = DS_LD(float, hg + k, DS_BX_W);
        const float* xg = x + r.xoff + n_lo;
        for (int i = tid; i < cnt; i += RP_T) xs[i] = DS_LD(float, xg + i, DS_BX_SRC0);
        __syncthreads();
    }
    // output m starts at input q = floor((HALF + m DOWN) / UP) with tap index p = (HALF + m DOWN) mod UP; 256 outputs on: (q, p) + (dq, dp)
    const long long t = (long long)r.half + ((long long)m0 + tid) * r.down;
    long long q = t / r.up;
    int p = (int)(t - q * r.up);
    const int dq = (RP_T * r.down) / r.up, dp = (RP_T * r.down) % r.up;
    float* o = out + r.ooff;
    for (int m = m0 + tid; m < m1; m += RP_T) {
        float acc = 0.f;
        if (m < mr && cnt > 0) {
            // n = q, q - 1, ... with tap p, p + UP, ...: skip the samples behind the signal's end, stop at its start or at the last tap
            const long long skip = q - (n_lo + cnt - 1) > 0 ? q - (n_lo + cnt - 1) : 0;
            const long long k0 = p + skip * r.up, i0 = q - skip - n_lo;
            if (k0 < nt && i0 >= 0) {
                const long long kl = k0 + i0 * r.up;                    // the tap that meets xs[0]
                const int kend = kl < nt - 1 ? (int)kl : nt - 1;
                int i = (int)i0;
#pragma unroll 4
                for (int k = (int)k0; k <= kend; k += r.up, --i) acc = fmaf(xs[i], hs[k], acc);
            }
        }
        DS_ST(float, o + m, DS_BX_OUT, acc);
        q += dq;
        p += dp;
        if (p >= r.up) {
            p -= r.up;
            ++q;
        }
    }
}

inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
constexpr long long MAX_ELEMS = (1ll << 31) - 1 - MAX_BLK;      // the table's offsets are int32, and m + 256 must not wrap

}  // namespace

extern "C" int ds_resample_poly(const float* x, const int32_t* tab, const float* filt, int n_signals, int max_blocks, int max_taps, int span,
                                long long total_in, long long total_out, long long total_filt, float* out, void* stream) {
    DS_REQUIRE(x && tab && filt && out && n_signals > 0 && max_blocks > 0 && total_in > 0 && total_out > 0 && total_filt > 0,
               "resample_poly: bad args (n_signals=%d max_blocks=%d total_in=%lld total_out=%lld total_filt=%lld)", n_signals, max_blocks, total_in, total_out,
               total_filt);
    DS_REQUIRE(max_taps >= 3 && max_taps <= MAX_TAPS && span >= 1 && span <= MAX_SPAN, "resample_poly: 3 <= max_taps <= %d, 1 <= span <= %d (max_taps=%d span=%d)",
               MAX_TAPS, MAX_SPAN, max_taps, span);
    DS_REQUIRE(n_signals <= 65535 && total_in <= MAX_ELEMS && total_out <= MAX_ELEMS && total_filt <= MAX_ELEMS,
               "resample_poly: at most 65535 signals and 2^31 - 1 - %d elements per buffer", MAX_BLK);
    if (!al4(x) || !al4(tab) || !al4(filt) || !al4(out)) DS_FAIL(DS_EALIGN, "resample_poly: every pointer must be 4-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#if DS_BOUNDS
    {
        DsBxHost h(DS_K_RESAMPLE_POLY);
        h.set(DS_BX_SRC0, x, total_in * 4);
        h.set(DS_BX_AUX0, tab, (long long)n_signals * DS_RP_NI * 4);
        h.set(DS_BX_W, filt, total_filt * 4);
        h.set(DS_BX_OUT, out, total_out * 4);
        h.publish(st);
    }
#endif
    DS_SET_MAX_LDS(resample_poly_kernel, RP_MAX_LDS, "resample_poly");
    hipLaunchKernelGGL(resample_poly_kernel, dim3(max_blocks, n_signals), dim3(RP_T), (size_t)(max_taps + span) * 4, st, x, tab, filt, total_in, total_out,
                       total_filt, max_taps, span, out);
    DS_CHECK_LAUNCH("resample_poly");
    return DS_OK;
}

#if DS_BOUNDS
extern "C" int ds_bounds_fetch_resample_poly(ds_bounds_rec* out, int reset) { return ds_bounds_fetch_tu(out, reset); }
#endif
