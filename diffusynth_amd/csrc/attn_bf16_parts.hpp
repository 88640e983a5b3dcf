// The parts the bf16 linear-attention kernels are put together from — ONE copy of each, so that a fix to a part reaches every kernel
// that runs it (gfx950).  Users: attn_fused.hip (first generation), attn_out2.hpp (second generation), vq_attn.hip (the VQGAN's block).
//
//   XStage                   a group of x rows, one group ahead in registers, double-buffered in LDS        (fused ctx, fused out, vq ctx, vq apply)
//   load_x_frags             x fragments straight from global memory, one tile ahead                        (out2, ctx2)
//   tile_row_max             ragged-row mask + row maximum of a k accumulator                               (fused ctx, ctx2, vq ctx)
//   softmax_tile_step        online softmax over the pixels of one tile + the two ctx^T += V^T P MFMAs      (fused ctx, ctx2, vq ctx)
//   write_partial            one (max, sum, ctx[d][e]) partial for attn_ctx_combine                          (fused ctx, ctx2, vq ctx)
//   q_softmax                softmax over d of a q accumulator, scaled, packed as two B operands            (fused out, out2)
// and from common.hpp: RowStage (weight rows -> LDS), read_gn, shq_entry / fill_shq, pack8, PARTF, LOG2E, acc_row32, exp2_hw.
//
// Where the kernels differ ON PURPOSE the part takes the difference as a template flag or a small callable and does not harmonise it: each
// form is a different rounding (or a different instruction count in a kernel bound by it), and every buffer keeps its bits.
#pragma once
#include "common.hpp"

#ifndef DS_ATTN_ABL
#define DS_ATTN_ABL 0   // diagnostic builds only: bit0 no y stores, bit1 no statistics, bit2 no Z phase, bit3 no q softmax, bit4 no x prefetch
#endif

namespace {

// A block walks a contiguous range of TP-pixel groups of one sample.  The group's x rows (contiguous in NHWC) are fetched with fully
// coalesced 16-byte loads one group ahead, staged in LDS (rows padded by 16 B: an odd number of 16-byte slots, conflict-free ds_read_b128)
// and shared by the block's waves.
// PIECE_BOUND: the load compares the piece index with the group's piece count.  It folds where the count is a multiple of the block's 256
// threads; the first-generation kernels keep it all the same (see attn_fused.hip).
template <int NKS, int TP, bool PIECE_BOUND = (TP * 2 * NKS) % 256 != 0>
struct XStage {
    static constexpr int C = NKS * 16, RS = 2 * C + 16;                // row stride in bytes
    static constexpr int BYTES = TP * RS;
    static constexpr int PIECES = TP * 2 * NKS;                        // 16-byte pieces of one group
    static constexpr int IT = (PIECES + 255) / 256;
    u32x4 r[IT];
    // unconditional loads (clamped address + select): a load under a branch would serialise the prefetch
    __device__ __forceinline__ void load(const bf16* x, int N, int group) {
        const long base = (long)group * TP * C;
        const long lim = (long)N * C;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int piece = threadIdx.x + it * 256;
            const long e = base + (long)piece * 8;
            const bool ok = (!PIECE_BOUND || piece < PIECES) && e < lim;
            const u32x4 v = DS_LD(u32x4, x + (ok ? e : 0), DS_BX_SRC0);
            r[it] = ok ? v : u32x4{0u, 0u, 0u, 0u};
        }
    }
    __device__ __forceinline__ void store(char* buf) const {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int piece = threadIdx.x + it * 256;
            if (PIECES % 256 == 0 || piece < PIECES) {
                const int row = piece / (2 * NKS), col = piece - row * (2 * NKS);
                *reinterpret_cast<u32x4*>(buf + row * RS + col * 16) = r[it];
            }
        }
    }
    // The double-buffer step: the group loaded a full iteration ago -> `buf`, the next one requested (it stays in flight across the
    // following iteration); the caller's __syncthreads() comes behind it.  Prologue: next(sm, .., g0 + 1 < g1 ? g0 + 1 : g0), end of
    // group g: next(the other buffer, .., g + 2 < g1 ? g + 2 : g).
    template <bool PREFETCH = true>
    __device__ __forceinline__ void next(char* buf, const bf16* x, int N, int group) {
        store(buf);
        if constexpr (PREFETCH) load(x, N, group);
    }
};

// x fragments of tile t for a wave whose lane (pixel n, k group kg) reads channels ks*16 + kg*8 .. + 7 of its pixel for every K step.
// (pixels past the end of a ragged last tile read pixel 0 instead: finite values, masked resp. never stored)
template <int NKS>
__device__ __forceinline__ void load_x_frags(bf16x8 (&xf)[NKS], const bf16* x, int N, int t, int n, int kg) {
    const int px = t * 32 + n;
    const bf16* row = x + (size_t)(px < N ? px : 0) * (16 * NKS) + kg * 8;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) xf[ks] = DS_LD(bf16x8, row + ks * 16, DS_BX_SRC0);
}

// Row maximum of a k accumulator (lane: d, registers: 16 pixel rows of lane half fh) over this lane half's rows; RAGGED: the rows at or
// past N are first set to -inf (exp2(-inf) = 0).  FROM_FIRST: the chain starts from ak[0] instead of -inf (one v_max_f32 fewer).
template <bool RAGGED, bool FROM_FIRST>
__device__ __forceinline__ float tile_row_max(f32x16& ak, int px0, int fh, int N) {
    float mr = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if constexpr (RAGGED) ak[r] = px0 + acc_row32(r, fh) >= N ? -INFINITY : ak[r];
        mr = FROM_FIRST && r == 0 ? ak[0] : fmaxf(mr, ak[r]);
    }
    return mr;
}

// One 32-pixel tile of the online softmax over the pixels, in the log2 domain (every exponential is a bare v_exp_f32), and
// ctx^T[e][d] += V^T P with the accumulators themselves as the MFMA operands: the rescale by exp2(m_old - m_new) is a per-LANE factor.
//   mr         tile_row_max() of this lane half
//   ga2        factor of the softmax argument (> 0: the maximum of the affine image is the affine image of the raw maximum)
//   mt_of(mr)  the tile's maximum of the argument;  cexp_of(mn) its additive part under the new running maximum mn: P = exp2(ga2 ak + cexp)
//   v_of(av)   what enters the context for a v accumulator element
//   TWO_CHAINS the sum of P in two chains of eight and the update as one fma (a kernel bound by its VALU instruction count)
template <bool TWO_CHAINS, class MtOf, class CexpOf, class VOf>
__device__ __forceinline__ void softmax_tile_step(const f32x16& ak, const f32x16& av, float mr, float ga2, MtOf mt_of, CexpOf cexp_of, VOf v_of,
                                                  float& m, float& ls, f32x16& ctx) {
    mr = fmaxf(mr, __shfl_xor(mr, 32, 64));                 // the running maximum per d is shared by the two lane halves
    const float mn = fmaxf(m, mt_of(mr));                   // finite: every tile holds >= 1 real pixel
    const float sc = exp2_hw(m - mn);                       // m = -inf on the first tile -> 0
    m = mn;
    const float cexp = cexp_of(mn);
    float P[16], V[16], psum = 0.f;
    if constexpr (TWO_CHAINS) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            P[r] = exp2_hw(fmaf(ga2, ak[r], cexp));
            V[r] = v_of(av[r]);
        }
        float ps1 = 0.f;                                    // (v_dot2c_f32_bf16 on the packed pairs measured slower: 21 cycles per
#pragma unroll
        for (int r = 0; r < 8; ++r) {                       //  instruction beside a busy matrix pipe against 2 x 8.4)
            psum += P[r];
            ps1 += P[8 + r];
        }
        psum += ps1;
        ls = fmaf(ls, sc, psum);
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            P[r] = exp2_hw(fmaf(ga2, ak[r], cexp));
            V[r] = v_of(av[r]);
            psum += P[r];
        }
        ls = ls * sc + psum;
    }
    if (__any(sc != 1.0f)) {                                // the running maximum rarely moves after the first tiles
#pragma unroll
        for (int r = 0; r < 16; ++r) ctx[r] *= sc;
    }
    ctx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pack8(V), pack8(P), ctx, 0, 0, 0);          // ctx^T[e][d]
    ctx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pack8(V + 8), pack8(P + 8), ctx, 0, 0, 0);
}

// One partial of the context pass: [32 max][32 sum][ctx[d][e]], d on the lane (frow), e in registers.  m goes back to the natural-log
// domain of the combine kernel; lsum = the sum of P over BOTH lane halves (the caller sums them, inside its own branch where it has one);
// ctx_of(r) = the context element of register r.
template <class CtxOf>
__device__ __forceinline__ void write_partial(float* out, int frow, int fh, float m, float lsum, CtxOf ctx_of) {
    if (fh == 0) {
        DS_ST(float, out + frow, DS_BX_AUX0, m * (1.0f / LOG2E));
        DS_ST(float, out + 32 + frow, DS_BX_AUX0, lsum);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) DS_ST(float, out + 64 + frow * 32 + acc_row32(r, fh), DS_BX_AUX0, ctx_of(r));
}

// Softmax over d of one head's q accumulator (rows d in registers, column = pixel on the lane; the two lane halves hold 16 rows each) in
// the log2 domain, scaled, packed: registers 0..7 / 8..15 are the eight k values of K step 0 / 1 of the next product's B operand.
// sh4(k) = the additive part of q (shq_entry) of rows 4k .. 4k + 3 of this lane half.  SOFTMAX = false: the ablation build's bare affine map.
template <bool SOFTMAX = true, class Sh4>
__device__ __forceinline__ void q_softmax(const f32x16& aq, Sh4 sh4, float ga2, float scale, bf16x8& q0, bf16x8& q1) {
    float q[16], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const f32x4 s4 = sh4(k);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            q[4 * k + e] = fmaf(ga2, aq[4 * k + e], s4[e]);
            mx = fmaxf(mx, q[4 * k + e]);
        }
    }
    if constexpr (SOFTMAX) {
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sq = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            q[r] = exp2_hw(q[r] - mx);
            sq += q[r];
        }
        sq += __shfl_xor(sq, 32, 64);
        const float inv = scale / sq;
#pragma unroll
        for (int r = 0; r < 16; ++r) q[r] *= inv;
    }
    q0 = pack8(q);
    q1 = pack8(q + 8);
}

}  // namespace
