// Windowed sampling (MultiDiffusion; diffusynth_amd/windowed.py): the windows of a wide latent as one batch of rows of the
// trained width (ds_window_split, a copy), and the blend of their predictions with a partition of unity (ds_window_merge).  fp32 NCHW.
// Row kernels (row_kernels.hpp: pieces, row fill, grid and dispatch): tables are the host's and are read per row, a
// malformed row reads nothing and shows as NaN in its output row when that row is in range, no LDS.  The blend reads its column tables
// through window_tables.hpp, as ds_stft_window_merge does.
#include "window_tables.hpp"

namespace {

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
        nan_row(dst, nullptr, CHw);
        return;
    }
    const float* src = p.x + (size_t)s * p.C * p.H * p.W;
    const bool vec = V == 4 && (o & 3) == 0;
    DS_FOR_PIECES(V, CHw, i0) {
        const float* srow = src + i0 / p.w * p.W;
        int col = o + (int)(i0 % p.w);                  // (o < W and c < w <= W: one subtraction brings it back)
        if (col >= p.W) col -= p.W;
        if constexpr (V == 4) {                         // (one 16-byte read or four reads: the compiler makes one code of the two)
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
// aligned (window_tables.hpp: the tables of the four columns of a piece, and the windows' values, in 16-byte loads)
template <int V>
__global__ __launch_bounds__(256) void window_merge_kernel(const ds_window_merge_params p) {
    const int r = blockIdx.y;                           // (< R <= Bout: the launcher's)
    const size_t CHW = (size_t)p.C * p.H * p.W, CHw = (size_t)p.C * p.H * p.w;
    float* out = p.out + (size_t)r * CHW;
    const int32_t* er = p.erow + (size_t)r * p.n;
    if (!window_rows_ok(er, p.n, p.Beps)) {
        nan_row(out, nullptr, CHW);
        return;
    }
    DS_FOR_PIECES(V, CHW, i0) {
        const size_t ch = i0 / p.W;
        const int x = (int)(i0 % p.W);
        float o[V];
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = __builtin_nanf("");                    // a column without an entry shows
        for (int m = 0; m < DS_WM_MAXM; ++m) {
            int j[V], c[V];
            float f[V], e[V];
            window_entry<V>(p.wcol, p.wcoef, (size_t)m * p.W + x, j, c, f);
            bool any = false;
#pragma unroll
            for (int k = 0; k < V; ++k) any |= j[k] >= 0;
            if (!any) break;
            const bool one = window_entry_one<V>(j, c, p.n, p.w);
            if (one) load_v<V>(p.eps + (size_t)er[j[0]] * CHw + ch * p.w + c[0], true, e);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                if (j[k] < 0) continue;                 // (the column's entries are over)
                if (!one) e[k] = window_entry_ok(j[k], c[k], p.n, p.w) ? p.eps[(size_t)er[j[k]] * CHw + ch * p.w + c[k]] : __builtin_nanf("");
                const float t = f[k] * e[k];
                o[k] = m == 0 ? t : o[k] + t;
            }
        }
        store_v<V>(out + i0, true, o);
    }
}
#pragma clang fp contract(fast)

}  // namespace

extern "C" int ds_window_split(const ds_window_split_params* p, void* stream) {
    DS_REQUIRE(p && p->x && p->out && p->rows, "window_split: null pointer");
    DS_REQUIRE_ROW_SIZES("window_split", p, R, C, H, w);
    DS_REQUIRE(p->w <= p->W, "window_split: bad sizes (W=%d w=%d)", p->W, p->w);
    DS_REQUIRE(p->Bx > 0 && p->Bout > 0, "window_split: bad row counts (Bx=%d Bout=%d)", p->Bx, p->Bout);
    const bool vec = p->W % 4 == 0 && p->w % 4 == 0 && ds_aligned16(p->x) && ds_aligned16(p->out);
    DS_LAUNCH_ROWS(window_split_kernel, "window_split", vec, (size_t)p->C * p->H * p->w, p->R, stream, *p);
    return DS_OK;
}

extern "C" int ds_window_merge(const ds_window_merge_params* p, void* stream) {
    DS_REQUIRE(p && p->eps && p->out && p->erow && p->wcol && p->wcoef, "window_merge: null pointer");
    DS_REQUIRE_ROW_SIZES("window_merge", p, R, C, H, W);
    DS_REQUIRE(p->n > 0 && p->w > 0, "window_merge: bad sizes (n=%d w=%d)", p->n, p->w);
    DS_REQUIRE(p->Beps > 0 && p->Bout >= p->R, "window_merge: bad row counts (Beps=%d Bout=%d R=%d)", p->Beps, p->Bout, p->R);
    const bool vec = p->W % 4 == 0 && p->w % 4 == 0 && ds_aligned16(p->eps) && ds_aligned16(p->out) && ds_aligned16(p->wcol) &&
                     ds_aligned16(p->wcoef);
    DS_LAUNCH_ROWS(window_merge_kernel, "window_merge", vec, (size_t)p->C * p->H * p->W, p->R, stream, *p);
    return DS_OK;
}
