// Windowed decoding (diffusynth_amd/windowed.py WindowedDecoder): the blend of the decoded windows of a long or looping
// latent, on the complex spectrum.  The windows are STFT+ representations (log1p|D|, cos, sin), which is no linear space: a frame
// under two or more windows is decoded like istft_frames_r4_kernel decodes it (stft_codec.hpp), blended with ds_window_merge's tables
// and rule, and encoded again; a frame under one window keeps that window's bits.  window.hip's conventions: tables are the host's, a
// malformed row reads nothing and shows as NaN, 16-byte pieces where alignment allows and scalar ones otherwise, no LDS.
#include "common.hpp"
#include "stft_codec.hpp"

namespace {

constexpr float kNaN = __builtin_nanf("");

// Every operation of the blend is a separately rounded IEEE fp32 op in table order (tests/decode_window_ref.py restates it in float64);
// the decode and the encode are stft_codec.hpp's, with the contraction they have in tail.hip
#pragma clang fp contract(off)
// grid (x: pieces of F * T, y: output row).  A thread owns V adjacent frames of one bin, all three channels.  V == 4 only when T % 4 == 0,
// w % 4 == 0 and encw / out / wcol / wcoef are 16-byte aligned: the tables of the four frames of a piece are three 16-byte loads per
// entry m, and the windows' values three where the four frames name one window at four adjacent frames from a multiple of 4 on
template <int V>
__global__ __launch_bounds__(256) void stft_window_merge_kernel(const ds_stft_window_merge_params p) {
    const int r = blockIdx.y;                           // (< R <= Bout: the launcher's)
    const size_t FT = (size_t)p.F * p.T, Fw = (size_t)p.F * p.w;
    float* out = p.out + (size_t)r * 3 * FT;
    const int32_t* er = p.erow + (size_t)r * p.n;
    bool bad = false;
    for (int j = 0; j < p.n; ++j) bad |= er[j] < 0 || er[j] >= p.Bw;              // (block-uniform)
    if (bad) {
        for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < 3 * FT; i += (size_t)gridDim.x * blockDim.x) out[i] = kNaN;
        return;
    }
    const size_t nv = FT / V;
    for (size_t v = blockIdx.x * (size_t)blockDim.x + threadIdx.x; v < nv; v += (size_t)gridDim.x * blockDim.x) {
        const size_t i0 = v * V, k = i0 / p.T;
        const int x = (int)(i0 % p.T);
        // a frame's state: cnt entries so far; with one, its three values e0 and its coefficient f0; from the second on the sum z
        int cnt[V];
        float e0[V][3], f0[V], zr[V], zi[V];
#pragma unroll
        for (int q = 0; q < V; ++q) {
            cnt[q] = 0;
            e0[q][0] = e0[q][1] = e0[q][2] = kNaN;       // a frame without an entry shows
        }
        for (int m = 0; m < DS_WM_MAXM; ++m) {
            const size_t t0 = (size_t)m * p.T + x;
            int j[V], c[V];
            float f[V], e[V][3];
            if constexpr (V == 4) {
                const int4 a = *reinterpret_cast<const int4*>(p.wcol + t0 * DS_WM_NI);
                const int4 b = *reinterpret_cast<const int4*>(p.wcol + (t0 + 2) * DS_WM_NI);
                const float4 g = *reinterpret_cast<const float4*>(p.wcoef + t0);
                j[0] = a.x; c[0] = a.y; j[1] = a.z; c[1] = a.w; j[2] = b.x; c[2] = b.y; j[3] = b.z; c[3] = b.w;
                f[0] = g.x; f[1] = g.y; f[2] = g.z; f[3] = g.w;
            } else {
                j[0] = p.wcol[t0 * DS_WM_NI + DS_WM_WIN];
                c[0] = p.wcol[t0 * DS_WM_NI + DS_WM_COL];
                f[0] = p.wcoef[t0];
            }
            bool any = false;
#pragma unroll
            for (int q = 0; q < V; ++q) any |= j[q] >= 0;
            if (!any) break;
            bool one = false;
            if constexpr (V == 4) {
                one = j[0] >= 0 && j[0] < p.n && j[1] == j[0] && j[2] == j[0] && j[3] == j[0] && c[0] >= 0 && (c[0] & 3) == 0 && c[0] + 3 < p.w &&
                      c[1] == c[0] + 1 && c[2] == c[0] + 2 && c[3] == c[0] + 3;
                if (one) {
                    const float* src = p.encw + (size_t)er[j[0]] * 3 * Fw + k * p.w + c[0];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const float4 t = *reinterpret_cast<const float4*>(src + ch * Fw);
                        e[0][ch] = t.x; e[1][ch] = t.y; e[2][ch] = t.z; e[3][ch] = t.w;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < V; ++q) {
                if (j[q] < 0) continue;                 // (the frame's entries are over)
                if (!one) {
                    const bool ok = j[q] < p.n && c[q] >= 0 && c[q] < p.w;        // (a malformed entry reads nothing)
                    const float* src = p.encw + (ok ? (size_t)er[j[q]] * 3 * Fw + k * p.w + c[q] : 0);
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) e[q][ch] = ok ? src[ch * Fw] : kNaN;
                }
                if (cnt[q] == 0) {
                    e0[q][0] = e[q][0]; e0[q][1] = e[q][1]; e0[q][2] = e[q][2];
                    f0[q] = f[q];
                } else {
                    if (cnt[q] == 1) {
                        const float2 d = stft_plus_decode(e0[q][0], e0[q][1], e0[q][2]);
                        zr[q] = f0[q] * d.x;
                        zi[q] = f0[q] * d.y;
                    }
                    const float2 d = stft_plus_decode(e[q][0], e[q][1], e[q][2]);
                    const float tr = f[q] * d.x, ti = f[q] * d.y;
                    zr[q] = zr[q] + tr;
                    zi[q] = zi[q] + ti;
                }
                ++cnt[q];
            }
        }
        float o[3][V];
#pragma unroll
        for (int q = 0; q < V; ++q) {
            if (cnt[q] <= 1) {                          // the window's bits (or NaN)
                o[0][q] = e0[q][0]; o[1][q] = e0[q][1]; o[2][q] = e0[q][2];
            } else {
                stft_plus_encode(zr[q], zi[q], o[0][q], o[1][q], o[2][q]);
                if (zr[q] != zr[q] || zi[q] != zi[q]) o[0][q] = o[1][q] = o[2][q] = kNaN;       // (a malformed entry among them)
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            if constexpr (V == 4) {
                *reinterpret_cast<float4*>(out + ch * FT + i0) = make_float4(o[ch][0], o[ch][1], o[ch][2], o[ch][3]);
            } else {
                out[ch * FT + i0] = o[ch][0];
            }
        }
    }
}
#pragma clang fp contract(fast)

}  // namespace

extern "C" int ds_stft_window_merge(const ds_stft_window_merge_params* p, void* stream) {
    DS_REQUIRE(p && p->encw && p->out && p->erow && p->wcol && p->wcoef, "stft_window_merge: null pointer");
    DS_REQUIRE(p->R > 0 && p->R <= 65535 && p->n > 0 && p->F > 0 && p->T > 0 && p->w > 0, "stft_window_merge: bad sizes (R=%d n=%d F=%d T=%d w=%d)",
               p->R, p->n, p->F, p->T, p->w);
    DS_REQUIRE(p->Bw > 0 && p->Bout >= p->R, "stft_window_merge: bad row counts (Bw=%d Bout=%d R=%d)", p->Bw, p->Bout, p->R);
    const bool vec = p->T % 4 == 0 && p->w % 4 == 0 && ds_aligned16(p->encw) && ds_aligned16(p->out) && ds_aligned16(p->wcol) &&
                     ds_aligned16(p->wcoef);
    const size_t n = (size_t)p->F * p->T;
    const dim3 grid((unsigned)blocks_for(vec ? n / 4 : n, 4096), (unsigned)p->R);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(stft_window_merge_kernel<4>, grid, dim3(256), 0, st, *p);
    else hipLaunchKernelGGL(stft_window_merge_kernel<1>, grid, dim3(256), 0, st, *p);
    DS_CHECK_LAUNCH("stft_window_merge");
    return DS_OK;
}
