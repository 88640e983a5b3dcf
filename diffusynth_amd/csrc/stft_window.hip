// Windowed decoding (diffusynth_amd/windowed.py WindowedDecoder): the blend of the decoded windows of a long or looping
// latent, on the complex spectrum.  The windows are STFT+ representations (log1p|D|, cos, sin), which is no linear space: a frame
// under two or more windows is decoded like istft_frames_r4_kernel decodes it (stft_codec.hpp), blended with ds_window_merge's tables
// and rule, and encoded again; a frame under one window keeps that window's bits.  A row kernel (row_kernels.hpp): the tables are
// the host's and are read through window_tables.hpp, a malformed row reads nothing and shows as NaN, no LDS.
#include "stft_codec.hpp"
#include "window_tables.hpp"

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
    if (!window_rows_ok(er, p.n, p.Bw)) {
        nan_row(out, nullptr, 3 * FT, blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
        return;
    }
    DS_FOR_PIECES(V, FT, i0) {
        const size_t k = i0 / p.T;
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
            int j[V], c[V];
            float f[V], e[V][3];
            window_entry<V>(p.wcol, p.wcoef, (size_t)m * p.T + x, j, c, f);
            bool any = false;
#pragma unroll
            for (int q = 0; q < V; ++q) any |= j[q] >= 0;
            if (!any) break;
            const bool one = window_entry_one<V>(j, c, p.n, p.w);
            if (one) {
                const float* src = p.encw + (size_t)er[j[0]] * 3 * Fw + k * p.w + c[0];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    float s4[V];
                    load_v<V>(src + ch * Fw, true, s4);
#pragma unroll
                    for (int q = 0; q < V; ++q) e[q][ch] = s4[q];
                }
            }
#pragma unroll
            for (int q = 0; q < V; ++q) {
                if (j[q] < 0) continue;                 // (the frame's entries are over)
                if (!one) {
                    const bool ok = window_entry_ok(j[q], c[q], p.n, p.w);        // (a malformed entry reads nothing)
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
        for (int ch = 0; ch < 3; ++ch) store_v<V>(out + ch * FT + i0, true, o[ch]);
    }
}
#pragma clang fp contract(fast)

}  // namespace

extern "C" int ds_stft_window_merge(const ds_stft_window_merge_params* p, void* stream) {
    DS_REQUIRE(p && p->encw && p->out && p->erow && p->wcol && p->wcoef, "stft_window_merge: null pointer");
    DS_REQUIRE_ROW_SIZES("stft_window_merge", p, R, n, F, T);
    DS_REQUIRE(p->w > 0, "stft_window_merge: bad sizes (w=%d)", p->w);
    DS_REQUIRE(p->Bw > 0 && p->Bout >= p->R, "stft_window_merge: bad row counts (Bw=%d Bout=%d R=%d)", p->Bw, p->Bout, p->R);
    const bool vec = p->T % 4 == 0 && p->w % 4 == 0 && ds_aligned16(p->encw) && ds_aligned16(p->out) && ds_aligned16(p->wcol) &&
                     ds_aligned16(p->wcoef);
    DS_LAUNCH_ROWS(stft_window_merge_kernel, "stft_window_merge", vec, (size_t)p->F * p->T, p->R, stream, *p);
    return DS_OK;
}
