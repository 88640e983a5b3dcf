// Windowed sampling (MultiDiffusion; diffusynth_amd/windowed.py): the windows of a wide latent as one batch of rows of the
// trained width (ds_window_split, a copy), and the blend of their predictions with a partition of unity (ds_window_merge).  fp32 NCHW.
// sampler_step.hip's conventions: tables are the host's and are read per row, a malformed row reads nothing and shows as NaN in its
// output row when that row is in range (table_row's rule), 16-byte pieces where alignment allows and scalar ones otherwise, no LDS.
#include "common.hpp"

namespace {

__device__ __forceinline__ void nan_fill(float* out, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = __builtin_nanf("");
}

// grid (x: pieces of a destination row, y: table row).  V == 4 only when W % 4 == 0, w % 4 == 0 and x / out are 16-byte aligned: a piece
// is then inside one image row of the window; it is read in one piece where the row's offset is a multiple of 4 (it then neither
// crosses the wrap nor leaves the alignment), element by element otherwise
template <int V>
__global__ __launch_bounds__(256) void window_split_kernel(const ds_window_split_params p) {
    const int32_t* ir = p.rows + (size_t)blockIdx.y * DS_WS_NI;
    const int s = ir[DS_WS_SRC], o = ir[DS_WS_OFF], d = ir[DS_WS_DST];
    const size_t CHw = (size_t)p.C * p.H * p.w;
    if (d < 0 || d >= p.Bout) return;
    float* dst = p.out + (size_t)d * CHw;
    if (s < 0 || s >= p.Bx || o < 0 || o >= p.W) {
        nan_fill(dst, CHw);
        return;
    }
    const float* src = p.x + (size_t)s * p.C * p.H * p.W;
    const bool vec = V == 4 && (o & 3) == 0;
    const size_t nv = CHw / V;
    for (size_t v = blockIdx.x * (size_t)blockDim.x + threadIdx.x; v < nv; v += (size_t)gridDim.x * blockDim.x) {
        const size_t i0 = v * V, ch = i0 / p.w;
        const float* srow = src + ch * p.W;
        int col = o + (int)(i0 % p.w);                  // (o < W and c < w <= W: one subtraction brings it back)
        if (col >= p.W) col -= p.W;
        if constexpr (V == 4) {
            float4 t;
            if (vec) {
                t = *reinterpret_cast<const float4*>(srow + col);
            } else {
                int c1 = col + 1, c2 = col + 2, c3 = col + 3;
                if (c1 >= p.W) c1 -= p.W;
                if (c2 >= p.W) c2 -= p.W;
                if (c3 >= p.W) c3 -= p.W;
                t = make_float4(srow[col], srow[c1], srow[c2], srow[c3]);
            }
            *reinterpret_cast<float4*>(dst + i0) = t;
        } else {
            dst[i0] = srow[col];
        }
    }
}

// Every operation below is a separately rounded IEEE fp32 op in table order (tests/window_ref.py restates it in numpy)
#pragma clang fp contract(off)
// grid (x: pieces of an output row, y: output row).  V == 4 only when W % 4 == 0, w % 4 == 0 and eps / out / wcol / wcoef are 16-byte
// aligned: the tables of the four columns of a piece are three 16-byte loads per entry m, and the windows' values one where the four
// columns name one window at four adjacent columns from a multiple of 4 on
template <int V>
__global__ __launch_bounds__(256) void window_merge_kernel(const ds_window_merge_params p) {
    const int r = blockIdx.y;                           // (< R <= Bout: the launcher's)
    const size_t CHW = (size_t)p.C * p.H * p.W, CHw = (size_t)p.C * p.H * p.w;
    float* out = p.out + (size_t)r * CHW;
    const int32_t* er = p.erow + (size_t)r * p.n;
    bool bad = false;
    for (int j = 0; j < p.n; ++j) bad |= er[j] < 0 || er[j] >= p.Beps;            // (block-uniform)
    if (bad) {
        nan_fill(out, CHW);
        return;
    }
    const size_t nv = CHW / V;
    for (size_t v = blockIdx.x * (size_t)blockDim.x + threadIdx.x; v < nv; v += (size_t)gridDim.x * blockDim.x) {
        const size_t i0 = v * V, ch = i0 / p.W;
        const int x = (int)(i0 % p.W);
        float o[V];
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = __builtin_nanf("");                    // a column without an entry shows
        for (int m = 0; m < DS_WM_MAXM; ++m) {
            const size_t t0 = (size_t)m * p.W + x;
            int j[V], c[V];
            float f[V], e[V];
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
            for (int k = 0; k < V; ++k) any |= j[k] >= 0;
            if (!any) break;
            bool one = false;
            if constexpr (V == 4) {
                one = j[0] >= 0 && j[0] < p.n && j[1] == j[0] && j[2] == j[0] && j[3] == j[0] && c[0] >= 0 && (c[0] & 3) == 0 && c[0] + 3 < p.w &&
                      c[1] == c[0] + 1 && c[2] == c[0] + 2 && c[3] == c[0] + 3;
                if (one) {
                    const float4 t = *reinterpret_cast<const float4*>(p.eps + (size_t)er[j[0]] * CHw + ch * p.w + c[0]);
                    e[0] = t.x; e[1] = t.y; e[2] = t.z; e[3] = t.w;
                }
            }
#pragma unroll
            for (int k = 0; k < V; ++k) {
                if (j[k] < 0) continue;                 // (the column's entries are over)
                if (!one) {
                    const bool ok = j[k] < p.n && c[k] >= 0 && c[k] < p.w;
                    e[k] = ok ? p.eps[(size_t)er[j[k]] * CHw + ch * p.w + c[k]] : __builtin_nanf("");     // (a malformed entry reads nothing)
                }
                const float t = f[k] * e[k];
                o[k] = m == 0 ? t : o[k] + t;
            }
        }
        if constexpr (V == 4) {
            *reinterpret_cast<float4*>(out + i0) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
            out[i0] = o[0];
        }
    }
}
#pragma clang fp contract(fast)

dim3 row_grid(bool vec, size_t n, int rows) { return dim3((unsigned)blocks_for(vec ? n / 4 : n, 4096), (unsigned)rows); }

}  // namespace

extern "C" int ds_window_split(const ds_window_split_params* p, void* stream) {
    DS_REQUIRE(p && p->x && p->out && p->rows, "window_split: null pointer");
    DS_REQUIRE(p->R > 0 && p->R <= 65535 && p->C > 0 && p->H > 0 && p->w > 0 && p->w <= p->W, "window_split: bad sizes (R=%d C=%d H=%d W=%d w=%d)",
               p->R, p->C, p->H, p->W, p->w);
    DS_REQUIRE(p->Bx > 0 && p->Bout > 0, "window_split: bad row counts (Bx=%d Bout=%d)", p->Bx, p->Bout);
    const bool vec = p->W % 4 == 0 && p->w % 4 == 0 && ds_aligned16(p->x) && ds_aligned16(p->out);
    const dim3 grid = row_grid(vec, (size_t)p->C * p->H * p->w, p->R);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(window_split_kernel<4>, grid, dim3(256), 0, st, *p);
    else hipLaunchKernelGGL(window_split_kernel<1>, grid, dim3(256), 0, st, *p);
    DS_CHECK_LAUNCH("window_split");
    return DS_OK;
}

extern "C" int ds_window_merge(const ds_window_merge_params* p, void* stream) {
    DS_REQUIRE(p && p->eps && p->out && p->erow && p->wcol && p->wcoef, "window_merge: null pointer");
    DS_REQUIRE(p->R > 0 && p->R <= 65535 && p->n > 0 && p->C > 0 && p->H > 0 && p->W > 0 && p->w > 0,
               "window_merge: bad sizes (R=%d n=%d C=%d H=%d W=%d w=%d)", p->R, p->n, p->C, p->H, p->W, p->w);
    DS_REQUIRE(p->Beps > 0 && p->Bout >= p->R, "window_merge: bad row counts (Beps=%d Bout=%d R=%d)", p->Beps, p->Bout, p->R);
    const bool vec = p->W % 4 == 0 && p->w % 4 == 0 && ds_aligned16(p->eps) && ds_aligned16(p->out) && ds_aligned16(p->wcol) &&
                     ds_aligned16(p->wcoef);
    const dim3 grid = row_grid(vec, (size_t)p->C * p->H * p->W, p->R);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(window_merge_kernel<4>, grid, dim3(256), 0, st, *p);
    else hipLaunchKernelGGL(window_merge_kernel<1>, grid, dim3(256), 0, st, *p);
    DS_CHECK_LAUNCH("window_merge");
    return DS_OK;
}
