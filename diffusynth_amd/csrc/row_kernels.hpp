// What every row kernel shares (sampler_step.hip, window.hip, stft_window.hip): a launch is grid (x: pieces of a row, y: row),
// in a 16-byte instantiation (V == 4) where sizes and addresses allow and a scalar one (V == 1) otherwise; a malformed row reads nothing
// and shows as NaN.  Nothing here rounds: the arithmetic of a kernel, and its `#pragma clang fp contract`, stay with the kernel.
#pragma once
#include "common.hpp"

// ---- pieces of V floats (vec: the address allows one 16-byte access; V == 4 only) ----------------------------------------------------
template <int V>
__device__ __forceinline__ void load_v(const float* p, bool vec, float (&v)[V]) {
    if constexpr (V == 4) {
        if (vec) {
            const float4 t = *reinterpret_cast<const float4*>(p);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = p[k];
}
template <int V>
__device__ __forceinline__ void store_v(float* p, bool vec, const float (&v)[V]) {
    if constexpr (V == 4) {
        if (vec) {
            *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) p[k] = v[k];
}
// what a row owns itself (its blend operands, its history) may be moved in 16-byte pieces: looked at per row
template <int V>
__device__ __forceinline__ bool row_vec(const void* p0, const void* p1 = nullptr, const void* p2 = nullptr) {
    return V == 4 && ((((uint64_t)p0 | (uint64_t)p1 | (uint64_t)p2) & 15) == 0);
}

// ---- the grid-strided loops along x --------------------------------------------------------------------------------------------------
// `DS_FOR_PIECES(V, n, i0) { ... }`: the body for the first element i0 of every whole piece of V among n elements.  A loop header and
// not a function taking a lambda: the body stays in the caller, under the caller's `#pragma clang fp contract`, and is optimised there
// (behind a lambda stft_window_merge_kernel<4> contracted four sums of the decode that it does not contract otherwise)
#define DS_FOR_PIECES(V, n, i0)                                                                                                    \
    for (size_t v_ = blockIdx.x * (size_t)blockDim.x + threadIdx.x, nv_ = (size_t)(n) / (V); v_ < nv_; v_ += (size_t)gridDim.x * blockDim.x) \
        if (const size_t i0 = v_ * (V); true)
// out[i] (and dup[i] where dup is given) = v for i = first, first + stride, ... below n: the grid-strided kernels fill a row along x, a
// block-per-row kernel from threadIdx.x in steps of its block
template <class I>
__device__ __forceinline__ void fill_row(float* out, float* dup, I n, float v, I first, I stride) {
    for (I i = first; i < n; i += stride) {
        out[i] = v;
        if (dup) dup[i] = v;
    }
}
__device__ __forceinline__ void fill_row(float* out, float* dup, size_t n, float v) {
    fill_row(out, dup, n, v, blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}
// a malformed row shows in the result
template <class I>
__device__ __forceinline__ void nan_row(float* out, float* dup, I n, I first, I stride) { fill_row(out, dup, n, __builtin_nanf(""), first, stride); }
__device__ __forceinline__ void nan_row(float* out, float* dup, size_t n) { fill_row(out, dup, n, __builtin_nanf("")); }

// ---- launchers -----------------------------------------------------------------------------------------------------------------------
// grid (x: pieces of one row of n elements, y: rows) of the 16-byte (vec) or the scalar instantiation
static inline dim3 row_grid(bool vec, size_t n, int rows) { return dim3((unsigned)blocks_for(vec ? n / 4 : n, 4096), (unsigned)rows); }
// kernel<4> where vec, kernel<1> otherwise, on row_grid(vec, n, rows) with blocks of 256; returns from the launcher if the launch failed
#define DS_LAUNCH_ROWS(kernel, name, vec, n, rows, stream, ...)                                  \
    do {                                                                                          \
        const bool vec_ = (vec);                                                                  \
        const dim3 grid_ = row_grid(vec_, (n), (rows));                                           \
        hipStream_t st_ = reinterpret_cast<hipStream_t>(stream);                                  \
        if (vec_) hipLaunchKernelGGL(kernel<4>, grid_, dim3(256), 0, st_, __VA_ARGS__);           \
        else hipLaunchKernelGGL(kernel<1>, grid_, dim3(256), 0, st_, __VA_ARGS__);                \
        DS_CHECK_LAUNCH(name);                                                                    \
    } while (0)
// the sizes of a row launch: R rows (grid y: at most 65535) of D0 x D1 x D2 elements, all members of *p, named in the message as they are here
#define DS_REQUIRE_ROW_SIZES(name, p, R, D0, D1, D2)                                                                                   \
    DS_REQUIRE((p)->R > 0 && (p)->R <= 65535 && (p)->D0 > 0 && (p)->D1 > 0 && (p)->D2 > 0, "%s: bad sizes (" #R "=%d " #D0 "=%d " #D1 "=%d " #D2 "=%d)", \
               name, (p)->R, (p)->D0, (p)->D1, (p)->D2)
