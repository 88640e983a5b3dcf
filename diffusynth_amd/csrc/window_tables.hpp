// The reader of the window tables of ds_window_merge and ds_stft_window_merge (include/diffusynth_hip.h: DS_WM_*): erow names the n
// window rows of an output row; wcol / wcoef hold, per entry m < DS_WM_MAXM and output column, the window j, its column c and the
// coefficient f.  The tables are the host's: a malformed entry reads nothing.  Nothing here rounds.
// A merge kernel reads entry m of its V columns (window_entry), stops where no column has an entry left (every j < 0: that test is three
// lines in each kernel, see profiles/row_kernels_refactor_isa.txt), takes the windows' values in one 16-byte load per plane where
// window_entry_one says so and element by element under window_entry_ok otherwise.
#pragma once
#include "row_kernels.hpp"

// every window row of the output row is a row of a buffer of B rows (block-uniform)
__device__ __forceinline__ bool window_rows_ok(const int32_t* er, int n, int B) {
    bool bad = false;
    for (int j = 0; j < n; ++j) bad |= er[j] < 0 || er[j] >= B;
    return !bad;
}
// entry t0 = m * (columns of a table row) + the first column, of V adjacent columns.  V == 4: three 16-byte loads
template <int V>
__device__ __forceinline__ void window_entry(const int32_t* wcol, const float* wcoef, size_t t0, int (&j)[V], int (&c)[V], float (&f)[V]) {
    if constexpr (V == 4) {
        const int4 a = *reinterpret_cast<const int4*>(wcol + t0 * DS_WM_NI);
        const int4 b = *reinterpret_cast<const int4*>(wcol + (t0 + 2) * DS_WM_NI);
        j[0] = a.x; c[0] = a.y; j[1] = a.z; c[1] = a.w; j[2] = b.x; c[2] = b.y; j[3] = b.z; c[3] = b.w;
    } else {
        j[0] = wcol[t0 * DS_WM_NI + DS_WM_WIN];
        c[0] = wcol[t0 * DS_WM_NI + DS_WM_COL];
    }
    load_v<V>(wcoef + t0, true, f);
}
// the four columns name one of the n windows (of w columns) at four adjacent columns from a multiple of 4 on
template <int V>
__device__ __forceinline__ bool window_entry_one(const int (&j)[V], const int (&c)[V], int n, int w) {
    if constexpr (V == 4)
        return j[0] >= 0 && j[0] < n && j[1] == j[0] && j[2] == j[0] && j[3] == j[0] && c[0] >= 0 && (c[0] & 3) == 0 && c[0] + 3 < w &&
               c[1] == c[0] + 1 && c[2] == c[0] + 2 && c[3] == c[0] + 3;
    return false;
}
// a column's entry (j >= 0) names a window and a column that exist
__device__ __forceinline__ bool window_entry_ok(int j, int c, int n, int w) { return j < n && c >= 0 && c < w; }
