// The parts that the VQGAN decoder's two 80-output-channel MFMA kernels share (conv3x3_c80.hip: the 80 -> 80 ResnetBlock body,
// convt4x4_c80.hip: the two ConvTranspose2d(., 80, 4, 2, 1) upsamples), one definition each.
//   K       : a K step of 32 = two (tap, 16-channel group) pairs; the pixel fragment of lane (pixel m, k group kq) is 16 contiguous bytes of
//             a staged halo pixel: pair 2 ks + (kq >> 1), channels 16 g + 8 (kq & 1) .. + 7
//   block   : persistent, 4 waves, works through one RUN of input tiles of TH x 32 pixels; the weight fragments stay in LDS for the whole
//             run, one halo image beside them; the halo of tile t+1 is requested before the MFMAs of tile t (range-checked buffer loads)
//   MFMA    : mfma(W, X): a lane owns one pixel and 4 consecutive channels per channel tile; accumulators start from the bias
// What differs stays in the two files: block -> run mapping, residual loads, the store pattern, the second halo image, the entry points.
#pragma once
#include "common.hpp"

namespace {

constexpr int C80_CO = 80, C80_NJ = C80_CO / 16;               // output channels: 5 channel tiles of 16
constexpr int C80_TW = 32, C80_NT = 256;

// NGI = input channels / 16, KW = taps per side of the gather (3: the 3x3; 2: one phase of the transposed 4x4), TH = tile rows (a wave =
// TH / 4 rows), DB = two halo images (one barrier per tile) or one (two barriers), BPC = blocks per CU (BPC x LDS <= 160 KB)
template <int NGI, int KW_, int TH_, bool DB_, int BPC_ = 1>
struct C80Geom {
    static constexpr int BPC = BPC_, KW = KW_, NG = NGI, CI = 16 * NGI, TH = TH_, RPW = TH_ / 4, NPT = 2 * RPW;
    static constexpr int NP = KW * KW * NGI, KS = (NP + 1) / 2;   // (tap, group) pairs, K steps: an odd count's last pair has zero weights
    static constexpr bool DB = DB_;
    static constexpr int HR = TH + KW - 1, HC = C80_TW + KW - 1, PIXB = CI * 2 + 16, QPP = CI * 2 / 16;   // halo pixels; the 16-byte pad keeps the
    static constexpr int HBYTES = HR * HC * PIXB;                                                          // 16 lanes of a ds_read_b128 on distinct banks
    static constexpr int WBYTES = KS * C80_NJ * 1024;               // (per phase)
    static constexpr int OFF_H = WBYTES, LDS = OFF_H + (DB ? 2 : 1) * HBYTES;
    static constexpr int NPX = HR * HC;
    static constexpr int PPI = C80_NT / QPP, LT = PPI * QPP;        // loader threads: thread = (pixel of PPI, chunk tid % QPP) — one chunk index per thread
    static constexpr int LIT = (NPX + PPI - 1) / PPI;
    static_assert(LDS * BPC <= 160 * 1024, "BPC blocks per CU");
    static_assert((PIXB / 4) % 4 == 0 && ((PIXB / 4) / 4) % 2 == 1, "pixel pitch: an odd number of 16-byte slots");
};

typedef __amdgpu_buffer_rsrc_t c80_rsrc_t;

struct C80Params {
    const void* x;      // [B][H][W][CI] bf16
    const void* wpk;    // packed weight fragments ([phase])[KS][5][64][8] bf16
    const float* bias;  // [80] or null
    void* out;
    const float* gn_ab; const float* gamma; const float* beta; int G;   // optional act(GroupNorm(G, CI)(x)) applied on the way into LDS
    float* stats_ws;    // optional [B][rps * slots per run][80][2]: per-channel (sum, sum of squares) of the output — ds_gn_stats_finish
    int B, H, W, tiles_w, tiles_h, rps, per;       // runs per sample, tiles per run
};

// ---- host: the partition of a sample's tiles into runs --------------------------------------------------------------------------------------
// A run never leaves its sample: the rps runs of a sample cut ITS tiles [0, tps) into pieces of `per`, so a block computes the sample's
// base pointers, buffer resources and GroupNorm affine once (runs past the end are empty: rps * per >= tps).
static void c80_partition(int B, int H, int W, int TH, int blocks, int& tiles_w, int& tiles_h, int& rps, int& per) {
    tiles_w = (W + C80_TW - 1) / C80_TW;
    tiles_h = (H + TH - 1) / TH;
    const int tps = tiles_w * tiles_h;
    rps = blocks / B;                                          // persistent: about one block per CU (x BPC)
    if (rps < 1) rps = 1;
    if (rps > tps) rps = tps;
    per = (tps + rps - 1) / rps;
}

// the shared parameter fields, and the extents of the bounds build (spr = statistics slots per run; res = a separate residual source or null)
template <typename M>
static void c80_fill(C80Params& p, int kernel_id, const void* x, const void* res, int B, int H, int W, const void* wpk, long long wbytes, const float* bias,
                     void* out, long long out_bytes, const float* gn_ab, int G, const float* gamma, const float* beta, float* stats_ws, int spr,
                     int blocks, hipStream_t st) {
    p.x = x; p.wpk = wpk; p.bias = bias; p.out = out;
    p.gn_ab = gn_ab; p.gamma = gamma; p.beta = beta; p.G = gn_ab ? G : 1;
    p.stats_ws = stats_ws;
    p.B = B; p.H = H; p.W = W;
    c80_partition(B, H, W, M::TH, blocks, p.tiles_w, p.tiles_h, p.rps, p.per);
#if DS_BOUNDS
    DsBxHost h(kernel_id);
    h.set(DS_BX_SRC0, x, (long long)B * H * W * M::CI * 2);
    h.set(DS_BX_RES, res, (long long)B * H * W * M::CI * 2);
    h.set(DS_BX_W, wpk, wbytes);
    h.set(DS_BX_BIAS, bias, bias ? C80_CO * 4 : 0);
    h.set(DS_BX_GNAB, gn_ab, gn_ab ? (long long)B * G * 2 * 4 : 0);
    h.set(DS_BX_AUX0, gamma, gn_ab ? M::CI * 4 : 0);
    h.set(DS_BX_AUX1, beta, gn_ab ? M::CI * 4 : 0);
    h.set(DS_BX_OUT, out, out_bytes);
    h.set(DS_BX_STATS, stats_ws, stats_ws ? (long long)B * p.rps * spr * C80_CO * 2 * 4 : 0);
    h.publish(st);
#endif
}

// ---- device: run of a block -------------------------------------------------------------------------------------------------------------------
// slot (sum, sum of squares) of channel 16 j + 4 kq + e in this wave's statistics
__device__ __forceinline__ void c80_stats_put(float* sws, int kq, int j, int e, float s1, float s2) {
    DS_ST(float, sws + (16 * j + 4 * kq + e) * 2, DS_BX_STATS, s1);
    DS_ST(float, sws + (16 * j + 4 * kq + e) * 2 + 1, DS_BX_STATS, s2);
}

struct C80Run { int b, q0, nt; float* sws; };       // sample, first tile inside it, tiles; this wave's statistics slot
// run -> tiles; spr = statistics slots per run, slot = this wave's.  False for an empty run, whose slots are zeroed here (it still owns them).
__device__ __forceinline__ bool c80_run(const C80Params& p, int run, int spr, int slot, int m, int kq, C80Run& r) {
    const int tps = p.tiles_w * p.tiles_h;
    r.b = run / p.rps;
    const int li = run - r.b * p.rps;
    r.q0 = min(tps, li * p.per);
    r.nt = min(tps, (li + 1) * p.per) - r.q0;
    r.sws = p.stats_ws ? p.stats_ws + ((size_t)r.b * (p.rps * spr) + li * spr + slot) * C80_CO * 2 : nullptr;
    if (r.nt > 0) return true;
    if (r.sws && m == 0)
#pragma unroll
        for (int j = 0; j < C80_NJ; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) c80_stats_put(r.sws, kq, j, e, 0.f, 0.f);
    return false;
}

// tile q of a sample -> its first row and column
template <typename M>
__device__ __forceinline__ void c80_locate(const C80Params& p, int q, int& i0, int& j0) {
    const int th = q / p.tiles_w;
    i0 = th * M::TH;
    j0 = (q - th * p.tiles_w) * C80_TW;
}

__device__ __forceinline__ c80_rsrc_t c80_rsrc(const char* base, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(base), (short)0, bytes, 0x00020000);
}

// WBYTES of weight fragments -> LDS (once per block; NB batches of loads)
template <int WBYTES, int NB>
__device__ __forceinline__ void c80_stage_weights(char* sm, const void* wpk, int tid) {
    constexpr int NV = WBYTES / 16, WIT = (NV + C80_NT - 1) / C80_NT, PER = (WIT + NB - 1) / NB;
    const u32x4* src = reinterpret_cast<const u32x4*>(wpk);
#pragma unroll
    for (int bt = 0; bt < NB; ++bt) {
        u32x4 wst[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) wst[k] = DS_LD(u32x4, src + min(tid + (bt * PER + k) * C80_NT, NV - 1), DS_BX_W);
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = tid + (bt * PER + k) * C80_NT;
            if (i < NV) *reinterpret_cast<u32x4*>(sm + i * 16) = wst[k];
        }
    }
}

// bias of this lane's rows of channel tile j: channels 16 j + 4 kq + r
__device__ __forceinline__ void c80_bias(const float* bias, int kq, f32x4 (&bv)[C80_NJ]) {
#pragma unroll
    for (int j = 0; j < C80_NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[j][r] = bias ? DS_LD(float, bias + 16 * j + 4 * kq + r, DS_BX_BIAS) : 0.f;
}

// ---- device: this thread's share of the halo staging ---------------------------------------------------------------------------------------
// Iteration it -> halo pixel it * PPI + tid / QPP, always the 16-byte chunk tid % QPP of it (so that the GroupNorm affine of its 8 channels
// lives in 16 registers); packed (row << 8 | col) and the LDS offset; the threads from LT on carry none.
template <typename M>
struct C80Halo {
    int lq, lp;
    bool loader;
    int s_rc[M::LIT], s_lds[M::LIT];
    u32x4 hv[M::LIT];
    float gsc[8], gsh[8];

    __device__ __forceinline__ void init(int tid) {
        lq = tid % M::QPP;
        lp = tid / M::QPP;
        loader = tid < M::LT;
#pragma unroll
        for (int it = 0; it < M::LIT; ++it) {
            const int hp = min(it * M::PPI + lp, M::NPX - 1), hr = hp / M::HC, hc = hp - hr * M::HC;
            s_rc[it] = (hr << 8) | hc;
            s_lds[it] = hp * M::PIXB + lq * 16;
        }
    }
    // request the halo whose first pixel is (oi, oj) of the sample at base
    __device__ __forceinline__ void issue(const C80Params& p, const char* base, c80_rsrc_t rs, int oi, int oj) {
#pragma unroll
        for (int it = 0; it < M::LIT; ++it) {
            const int ih = oi + (s_rc[it] >> 8), iw = oj + (s_rc[it] & 0xff);
            // (arithmetic out-of-range offsets: bit 31 = beyond the buffer; cut to 28 bits first — see conv7x7_c4.hip)
            const unsigned bad = (unsigned)(!loader) | (unsigned)(it * M::PPI + lp >= M::NPX) | (unsigned)((unsigned)ih >= (unsigned)p.H) | (unsigned)((unsigned)iw >= (unsigned)p.W);
            const unsigned off = (((unsigned)((ih * p.W + iw) * M::CI + lq * 8) * 2u) & 0x0fffffffu) | (bad << 31);
#if DS_BOUNDS
            if (bad || !ds_bx_ok(base + off, DS_BX_SRC0, 16)) { hv[it] = u32x4{0u, 0u, 0u, 0u}; continue; }
#endif
            hv[it] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0);
        }
    }
    // GroupNorm affine of this thread's 8 channels for sample b: v = act(x * sc + sh)
    __device__ __forceinline__ void load_gn(const C80Params& p, int b) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = lq * 8 + e, g = c / (M::CI / p.G);
            const float a = DS_LD(float, p.gn_ab + ((size_t)b * p.G + g) * 2, DS_BX_GNAB), am = DS_LD(float, p.gn_ab + ((size_t)b * p.G + g) * 2 + 1, DS_BX_GNAB);
            const float gm = DS_LD(float, p.gamma + c, DS_BX_AUX0);
            gsc[e] = a * gm;
            gsh[e] = DS_LD(float, p.beta + c, DS_BX_AUX1) - am * gm;
        }
    }
    // the requested halo -> image h; gn (block-uniform): through act(affine).  Zero padding applies AFTER it (pixels outside the image must
    // stay 0: they are written as loaded — the range check returned zeros — and act(sh) would not be 0)
    template <typename Act>
    __device__ __forceinline__ void fill(char* h, const C80Params& p, bool gn, int oi, int oj, Act act) {
#pragma unroll
        for (int it = 0; it < M::LIT; ++it) {
            u32x4 v = hv[it];
            if (gn) {
                const int ih = oi + (s_rc[it] >> 8), iw = oj + (s_rc[it] & 0xff);
                const float keep = ((unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W) ? 1.f : 0.f;
                bf16x8 o8;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float lo = __uint_as_float(v[e] << 16), hi = __uint_as_float(v[e] & 0xffff0000u);
                    o8[2 * e] = (bf16)(keep * act(fmaf(lo, gsc[2 * e], gsh[2 * e])));
                    o8[2 * e + 1] = (bf16)(keep * act(fmaf(hi, gsc[2 * e + 1], gsh[2 * e + 1])));
                }
                v = __builtin_bit_cast(u32x4, o8);
            }
            if (loader && (it + 1 < M::LIT || it * M::PPI + lp < M::NPX)) *reinterpret_cast<u32x4*>(h + s_lds[it]) = v;
        }
    }
};

// ---- device: the K loop ---------------------------------------------------------------------------------------------------------------------
// pixel fragment of K step ks: pair pidx = 2 ks + (kq >> 1) = (tap = KW dy + dx; group g), channels 16 g + 8 (kq & 1): byte offset inside the
// halo; the last pair of an odd count (zero weights) re-reads the one before
template <typename M>
__device__ __forceinline__ void c80_xoff(int kq, int (&xoff)[M::KS]) {
#pragma unroll
    for (int ks = 0; ks < M::KS; ++ks) {
        const int pidx = (M::NP & 1) ? min(2 * ks + (kq >> 1), M::NP - 1) : 2 * ks + (kq >> 1), tap = pidx / M::NG, g = pidx - tap * M::NG;
        xoff[ks] = ((tap / M::KW) * M::HC + (tap % M::KW)) * M::PIXB + (g * 16 + (kq & 1) * 8) * 2;
    }
}
// acc[i][j] = bias + W_j . X_i over the halo image: hx = image + this lane's first pixel (row RPW * wave, column m), pixel tile i of the wave
// at + ((i >> 1) * HC + 16 (i & 1)) * PIXB; wl = weights + lane * 16, fragment (ks, j) at + (ks * 5 + j) * 1024
template <typename M>
__device__ __forceinline__ void c80_mma(const char* hx, const char* wl, const int (&xoff)[M::KS], const f32x4 (&bv)[C80_NJ], f32x4 (&acc)[M::NPT][C80_NJ]) {
#pragma unroll
    for (int ks = 0; ks < M::KS; ++ks) {
        bf16x8 xf[M::NPT], wf[C80_NJ];
#pragma unroll
        for (int i = 0; i < M::NPT; ++i) xf[i] = *reinterpret_cast<const bf16x8*>(hx + ((i >> 1) * M::HC + 16 * (i & 1)) * M::PIXB + xoff[ks]);
#pragma unroll
        for (int j = 0; j < C80_NJ; ++j) wf[j] = *reinterpret_cast<const bf16x8*>(wl + (ks * C80_NJ + j) * 1024);
#pragma unroll
        for (int i = 0; i < M::NPT; ++i)
#pragma unroll
            for (int j = 0; j < C80_NJ; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], xf[i], ks == 0 ? bv[j] : acc[i][j], 0, 0, 0);
    }
}

// ---- device: statistics of this lane's 20 output channels (fp32 values before rounding) ---------------------------------------------------------
struct C80Stats {
    float s1[C80_NJ][4], s2[C80_NJ][4];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < C80_NJ; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) s1[j][e] = s2[j][e] = 0.f;
    }
    __device__ __forceinline__ void add(int j, int e, float v) {
        s1[j][e] += v;
        s2[j][e] = fmaf(v, v, s2[j][e]);
    }
    // sum over the 16 pixel lanes of a k group, lane m = 0 writes its 20 channels
    __device__ __forceinline__ void finish(float* sws, int m, int kq) const {
#pragma unroll
        for (int j = 0; j < C80_NJ; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = s1[j][e], b2 = s2[j][e];
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) {
                    a += __shfl_xor(a, d, 64);
                    b2 += __shfl_xor(b2, d, 64);
                }
                if (m == 0) c80_stats_put(sws, kq, j, e, a, b2);
            }
    }
};

}  // namespace
