// The STFT+ representation (log1p|D|, cos arg D, sin arg D) of one bin, to and from the complex value: the one copy of the decode of
// istft_frames_r4_kernel (tail.hip) and of the window blend (stft_window.hip), and of the encode of stft_plus_kernel and that blend.
// Included before any `#pragma clang fp contract`: both functions are compiled with the default contraction wherever they are inlined.
#pragma once
#include <hip/hip_runtime.h>

// mag * exp(i atan2(sin, cos)) = mag * (cos, sin) / |(cos, sin)| — no atan2f / cosf / sinf (three libm calls per bin were half of the first
// iSTFT kernel's 168 us); atan2(0, 0) = 0 in the reference's formula: (mag, 0).  The pair need not be of unit length (the decoder's are
// tanh outputs).
__device__ __forceinline__ float2 stft_plus_decode(float c0, float c1, float c2) {
    const float mag = expm1f(c0);
    // (the pair is first scaled by an exact power of two so that max(|cos|, |sin|) lies in [0.5, 1): c^2 + s^2 neither underflows —
    // v_rsq_f32 returns +inf for a denormal argument, and a pair of 1e-23s used to lose its phase to n2 == 0 — nor overflows)
    const float pm = fmaxf(fabsf(c1), fabsf(c2));
    const bool z0 = !(pm > 0.f) || !(pm < 3.0e38f);               // 0 (and nothing finite): the reference's phase is 0 (resp. undefined)
    const int pe = z0 ? 0 : __builtin_amdgcn_frexp_expf(pm);
    const float pa = ldexpf(c1, -pe), pb = ldexpf(c2, -pe);
    const float n2 = pa * pa + pb * pb;
    float ri = __builtin_amdgcn_rsqf(n2);
    ri = ri * (1.5f - 0.5f * n2 * ri * ri);
    return float2{z0 ? mag : mag * (pa * ri), z0 ? 0.f : mag * (pb * ri)};
}

// tools.encode_stft of one bin; a zero spectrum has phase 0: (0, 1, 0)
__device__ __forceinline__ void stft_plus_encode(float xr, float xi, float& c0, float& c1, float& c2) {
    // (as in the decode, the pair is first scaled by an exact power of two so that max(|xr|, |xi|) lies in [0.5, 1): the squares of a bin
    // below 1e-19 are denormal or zero, and its (cos, sin) used to come out far off unit length or as (1, 0); those of a bin above 1e19
    // overflow.  Scaling by a power of two commutes with every rounding below, so a bin in the normal range keeps its bits.)
    const float pm = fmaxf(fabsf(xr), fabsf(xi));
    const int pe = pm > 0.f && pm < 3.0e38f ? __builtin_amdgcn_frexp_expf(pm) : 0;
    const float pa = ldexpf(xr, -pe), pb = ldexpf(xi, -pe);
    const float n = sqrtf(pa * pa + pb * pb);
    c0 = log1pf(ldexpf(n, pe));
    c1 = n > 0.f ? pa / n : 1.f;
    c2 = n > 0.f ? pb / n : 0.f;
}
