// Fused linear attention for the U-Net's Residual(PreNorm(LinearCrossAttentionAdd)) block
// (diffusion_components.py:142-152,252-293), bf16, 4 heads x 32 (gfx950).
//
// The unfused path materialises the 384-channel qkv tensor (the largest tensor of the network) and reads
// it twice.  Here x is the only input stream:
//
//   pass 1 (context):  per wave = one head; k,v tiles = x[32 px] . Wk^T, Wv^T on MFMA (PreNorm folded into the
//                      weights + a per-channel shift), two sweeps over the segment (max, then exp/accumulate).
//                      The 32x32 accumulators of P = exp(k - max) and V already have the operand layout of the
//                      next product (column on the lane, rows in registers), so ctx += P^T V is two more MFMAs
//                      on the bf16-packed accumulators — no LDS, no transposes.
//   combine:           (linattn.hip) merges the segments' (max, sum, ctx).
//   pass 2 (output):   per wave = one 32-pixel tile; q^T = Wq . x^T (pixels on lanes => the softmax over d runs
//                      over registers), Y_h = ctx_h^T . q~_h and Z = Wout . [Y_0..Y_3] are chained the same way
//                      (accumulator tile as the B operand; the A operands ctx^T / Wout use the matching permuted
//                      k order), + bias, GroupNorm partials, row-major store through a wave-private LDS stage.
//
// HBM traffic per pixel: 2 reads of x (second one L2-resident) + 1 read of x + 1 write of y,
// instead of x + 2.67x(384 ch) + ... of the unfused chain.
//
// This file: the first-generation kernels (attn_fused_ctx, attn_fused_out: block = 4 waves = the 4 heads, x staged in LDS, every weight
// fragment of a wave in its registers), the weight packing, and the launch decisions and launches of BOTH generations; the
// second-generation kernels (wave = pixel tile, weights in LDS) are attn_out2.hpp.  Both are put together from the parts of
// attn_bf16_parts.hpp (x stage, online-softmax tile step, partial write-out, q softmax) and common.hpp (RowStage, read_gn, shq_entry).
#include "common.hpp"
#include "conv_epilogue.hpp"   // permlane32_swap
#include "attn_bf16_parts.hpp"
#include "attn_out2.hpp"       // the second-generation kernels: one translation unit, one bounds table

int ds_linattn_launch_combine(const ds_attn_params* p, hipStream_t st);  // linattn.hip

namespace {

// The x stage of the first generation: 32 T pixels per group.  Its load keeps the piece bound where it would fold (a multiple of 256 pieces):
// with `e < lim` alone attn_fused_ctx<12, 1> ran 21.70 -> 21.94 us at batch 16 and attn_fused_out<24, 1> 23.92 -> 24.10 us at 32x8, batch
// 128, each outside the parent's spread; with the bound both are the parent's again (profiles/attn_bf16_refactor_ab.txt)
template <int NKS, int T> using FusedXStage = XStage<NKS, 32 * T, true>;

// ------------------------------------------------------------------------------------------------ pass 1
// k, v tiles of this head: acc layout = (lane: d resp. e, registers: 16 pixel rows).  Online softmax over the pixels
// (running max per d, shared by the two lane halves), ctx^T[e][d] += V^T P with the accumulators themselves as the
// MFMA operands: the rescale by exp(m_old - m_new) is then a per-LANE factor.
template <int NKS, int T>
__global__ __launch_bounds__(256, NKS >= 24 ? 1 : 2) void attn_fused_ctx_kernel(const ds_attn_fused_params p) {
    constexpr int TP = 32 * T;
    using XS = FusedXStage<NKS, T>;
    constexpr int C = XS::C, RS = XS::RS;
    constexpr int KCH = NKS < 12 ? NKS : 12;                    // fragment reads in flight per chunk
    extern __shared__ __attribute__((aligned(16))) char sm[];   // x[2][XS::BYTES]
    const int seg = blockIdx.x, b = blockIdx.y, lane = threadIdx.x & 63, head = threadIdx.x >> 6;
    const int frow = lane & 31, fh = lane >> 5;
    const int ngroups = (p.N + TP - 1) / TP, per = (ngroups + p.nseg - 1) / p.nseg;
    const int g0 = seg * per, g1 = min(ngroups, g0 + per);
    const bf16* x = reinterpret_cast<const bf16*>(p.x) + (size_t)b * p.N * C;
    const int nk = 128 + head * 32 + frow, nv = 256 + head * 32 + frow;
    float* out = p.part + (((size_t)b * 4 + head) * p.nseg + seg) * PARTF;

    float m = -INFINITY, ls = 0.f;
    f32x16 ctx;
#pragma unroll
    for (int r = 0; r < 16; ++r) ctx[r] = 0.f;
    if (g0 < g1) {                                    // block-uniform
        XS xs;
        xs.load(x, p.N, g0);
        bf16x8 Wk[NKS], Wv[NKS];
        {
            const bf16* wk = reinterpret_cast<const bf16*>(p.wqkv) + (size_t)nk * C + fh * 8;
            const bf16* wv = reinterpret_cast<const bf16*>(p.wqkv) + (size_t)nv * C + fh * 8;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                Wk[ks] = DS_LD(bf16x8, wk + ks * 16, DS_BX_W);
                Wv[ks] = DS_LD(bf16x8, wv + ks * 16, DS_BX_W);
            }
        }
        float ga, gam;
        read_gn(p, b, ga, gam);
        const float shk = DS_LD(float, p.t1 + nk, DS_BX_T1) - gam * DS_LD(float, p.t2 + nk, DS_BX_T2);
        const float shv = DS_LD(float, p.t1 + nv, DS_BX_T1) - gam * DS_LD(float, p.t2 + nv, DS_BX_T2);
        const float ga2 = ga * LOG2E, shk2 = shk * LOG2E;
        xs.next(sm, x, p.N, g0 + 1 < g1 ? g0 + 1 : g0);
        __syncthreads();
        for (int g = g0; g < g1; ++g) {
            const int cur = (g - g0) & 1;
            const char* xb = sm + cur * XS::BYTES + frow * RS + fh * 16;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                f32x16 ak, av;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    ak[r] = 0.f;
                    av[r] = 0.f;
                }
                // all fragment reads of a chunk are issued before its first MFMA (left alone, the scheduler reuses one
                // register quad and waits out the full LDS latency in front of every MFMA)
#pragma unroll
                for (int k0 = 0; k0 < NKS; k0 += KCH) {
                    bf16x8 xf[KCH];
#pragma unroll
                    for (int ks = 0; ks < KCH; ++ks) xf[ks] = *reinterpret_cast<const bf16x8*>(xb + t * 32 * RS + (k0 + ks) * 32);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int ks = 0; ks < KCH; ++ks) {
                        ak = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xf[ks], Wk[k0 + ks], ak, 0, 0, 0);
                        av = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xf[ks], Wv[k0 + ks], av, 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                // online softmax in the log2 domain: ga2 / shk2 carry log2(e); v is normalised per element before the bf16 pack
                const int px0 = g * TP + t * 32;
                const bool full = px0 + 32 <= p.N;                    // wave-uniform: only the last group can be ragged
                float mr;
                if (full) mr = tile_row_max<false, false>(ak, px0, fh, p.N);
                else mr = tile_row_max<true, false>(ak, px0, fh, p.N);
                softmax_tile_step<false>(ak, av, mr, ga2, [&](float mx) { return fmaf(ga2, mx, shk2); }, [&](float mn) { return shk2 - mn; },
                                         [&](float v) { return ga * v + shv; }, m, ls, ctx);
            }
            xs.next(sm + (cur ^ 1) * XS::BYTES, x, p.N, g + 2 < g1 ? g + 2 : g);
            __syncthreads();
        }
        ls += __shfl_xor(ls, 32, 64);
    }
    write_partial(out, frow, fh, m, ls, [&](int r) { return ctx[r]; });
}

// ------------------------------------------------------------------------------------------------ pass 2
// wave = head: q^T = Wq_h . x^T (pixels on lanes => softmax over d runs over registers), Y_h = ctx_h^T . q~_h with the
// accumulator tile as the B operand; the four heads' Y tiles (bf16, already B-operand shaped) are exchanged through LDS
// and each wave then produces the 32-channel blocks {wave, wave+4, ..} of Z = Wout . [Y_0..Y_3] + bias.  Z's accumulators
// hold one pixel per lane: v_permlane32_swap pairs the lane halves into 8 consecutive channels = one 16-byte store.
template <int NKS, int T>
__global__ __launch_bounds__(256, NKS >= 24 ? 1 : 2) void attn_fused_out_kernel(const ds_attn_fused_params p) {
    constexpr int TP = 32 * T;
    using XS = FusedXStage<NKS, T>;
    constexpr int C = XS::C, CB = C / 32, RS = XS::RS;
    constexpr int NCB = (CB + 3) / 4;
    constexpr int KCH = NKS < 12 ? NKS : 12;                    // fragment reads in flight per chunk
    constexpr int YBYTES = 4 * T * 2 * 1024;
    extern __shared__ __attribute__((aligned(16))) char sm[];   // x[2][XS::BYTES] | y[2][4 heads][T][2][64 lanes] x 16 B
    __shared__ __attribute__((aligned(16))) float red[8];
    __shared__ __attribute__((aligned(16))) float sbias[C];     // to_out bias: loop-invariant, but a global load inside the loop is re-issued per tile
    const int b = blockIdx.y, lane = threadIdx.x & 63, head = threadIdx.x >> 6;
    const int frow = lane & 31, fh = lane >> 5;
    char* const ybase = sm + 2 * XS::BYTES;
    const int ngroups = (p.N + TP - 1) / TP, per = (ngroups + gridDim.x - 1) / gridDim.x;
    const int g0 = blockIdx.x * per, g1 = min(ngroups, g0 + per);
    const bf16* x = reinterpret_cast<const bf16*>(p.x) + (size_t)b * p.N * C;
    bf16* yout = reinterpret_cast<bf16*>(p.y) + (size_t)b * p.N * C;
    float s1 = 0.f, s2 = 0.f;
    if (g0 < g1) {                                    // block-uniform
        XS xs;
        xs.load(x, p.N, g0);
        // ---- register-resident operands of this wave
        bf16x8 Wq[NKS], Wo[NCB][8], cA[2];
        {
            const bf16* wq = reinterpret_cast<const bf16*>(p.wqkv) + (size_t)(head * 32 + frow) * C + fh * 8;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) Wq[ks] = DS_LD(bf16x8, wq + ks * 16, DS_BX_W);
#pragma unroll
            for (int c = 0; c < NCB; ++c) {
                const int cb = head + 4 * c < CB ? head + 4 * c : 0;
                const bf16* wo = reinterpret_cast<const bf16*>(p.wout_perm) + (size_t)(cb * 32 + frow) * 128 + fh * 8;
#pragma unroll
                for (int k = 0; k < 8; ++k) Wo[c][k] = DS_LD(bf16x8, wo + k * 16, DS_BX_AUX1);
            }
            const float* ctx = p.ctx + ((size_t)b * 4 + head) * 1024;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                float ca[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) ca[j] = DS_LD(float, ctx + (16 * s + 8 * (j >> 2) + 4 * fh + (j & 3)) * 32 + frow, DS_BX_AUX2);
                cA[s] = pack8(ca);
            }
        }
        float ga, gam;
        read_gn(p, b, ga, gam);
        float shq[16];                                   // additive part of q (fold shift + label_q) for this lane's 16 rows d
#pragma unroll
        for (int r = 0; r < 16; ++r) shq[r] = shq_entry(p, head * 32 + acc_row32(r, fh), b, gam);
        const float ga2 = ga * LOG2E;                    // softmax over d in the log2 domain: bare v_exp_f32
        xs.store(sm);                                    // (XStage::next() spelled out: the bias row is requested between its two halves, as ever)
        for (int i = threadIdx.x; i < C; i += 256) sbias[i] = DS_LD(float, p.bias_out + i, DS_BX_BIAS);
        xs.load(x, p.N, g0 + 1 < g1 ? g0 + 1 : g0);
        __syncthreads();
        for (int g = g0; g < g1; ++g) {
            const int cur = (g - g0) & 1;
            const char* xb = sm + cur * XS::BYTES + frow * RS + fh * 16;
            bf16x8* const yw = reinterpret_cast<bf16x8*>(ybase + cur * YBYTES) + (head * T * 2) * 64 + lane;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                f32x16 aq;
#pragma unroll
                for (int r = 0; r < 16; ++r) aq[r] = 0.f;
#pragma unroll
                for (int k0 = 0; k0 < NKS; k0 += KCH) {
                    bf16x8 xf[KCH];
#pragma unroll
                    for (int ks = 0; ks < KCH; ++ks) xf[ks] = *reinterpret_cast<const bf16x8*>(xb + t * 32 * RS + (k0 + ks) * 32);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int ks = 0; ks < KCH; ++ks) aq = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Wq[k0 + ks], xf[ks], aq, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                bf16x8 qB[2];
                q_softmax<!(DS_ATTN_ABL & 8)>(aq, [&](int k) { return f32x4{shq[4 * k], shq[4 * k + 1], shq[4 * k + 2], shq[4 * k + 3]}; }, ga2, p.scale, qB[0], qB[1]);
                // Y_h[e][px] = sum_d ctx[d][e] q~[d][px]: A = ctx^T in the permuted k order of the accumulator operand
                f32x16 Y;
#pragma unroll
                for (int r = 0; r < 16; ++r) Y[r] = 0.f;
                Y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cA[0], qB[0], Y, 0, 0, 0);
                Y = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cA[1], qB[1], Y, 0, 0, 0);
                float yv[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) yv[r] = Y[r];
                yw[(t * 2 + 0) * 64] = pack8(yv);
                yw[(t * 2 + 1) * 64] = pack8(yv + 8);
            }
            xs.template next<!(DS_ATTN_ABL & 16)>(sm + (cur ^ 1) * XS::BYTES, x, p.N, g + 2 < g1 ? g + 2 : g);   // group g+2 stays in flight across the Z phase and the next Q phase
            __syncthreads();
            // ---- Z[c][px] = sum_{h,e} Wout[c][h*32+e] Y_h[e][px] + bias[c] for this wave's channel blocks
            const bf16x8* const yr = reinterpret_cast<const bf16x8*>(ybase + cur * YBYTES) + lane;
#pragma unroll
            for (int t = 0; t < ((DS_ATTN_ABL & 4) ? 0 : T); ++t) {
                bf16x8 yB[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) yB[k] = yr[(((k >> 1) * T + t) * 2 + (k & 1)) * 64];
                __builtin_amdgcn_sched_barrier(0);
                const int px = g * TP + t * 32 + frow;
#pragma unroll
                for (int c = 0; c < NCB; ++c) {
                    const int cb = head + 4 * c;
                    if (cb < CB) {                   // wave-uniform
                        f32x16 Z;
#pragma unroll
                        for (int r = 0; r < 16; ++r) Z[r] = 0.f;
#pragma unroll
                        for (int k = 0; k < 8; ++k) Z = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Wo[c][k], yB[k], Z, 0, 0, 0);
                        asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" : "+v"(Z));   // MFMA write -> inline-asm read (tied to Z: cannot move off the accumulators)
#pragma unroll
                        for (int q2 = 0; q2 < 2; ++q2) {
                            float v[8];
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                v[k] = Z[8 * q2 + k];
                                v[4 + k] = Z[8 * q2 + 4 + k];
                                permlane32_swap(v[k], v[4 + k]);
                            }
                            const int c0 = cb * 32 + 16 * q2 + 8 * fh;
                            const f32x4 b0 = *reinterpret_cast<const f32x4*>(sbias + c0), b1 = *reinterpret_cast<const f32x4*>(sbias + c0 + 4);
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                v[k] += b0[k];
                                v[4 + k] += b1[k];
                            }
                            if (px < p.N) {
                                if constexpr (!(DS_ATTN_ABL & 1)) vec16_store<bf16>(yout + (size_t)px * C + c0, v, DS_BX_OUT);
                                else if (v[0] == 12345.678f) yout[0] = (bf16)v[1];
#pragma unroll
                                for (int k = 0; k < ((DS_ATTN_ABL & 2) ? 0 : 8); ++k) {
                                    s1 += v[k];
                                    s2 += v[k] * v[k];
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    if (p.stats_part) block_stats_write(s1, s2, red, p.stats_part + ((size_t)b * gridDim.x + blockIdx.x) * 2);
}

__global__ void pack_attn_kernel(const float* wqkv, const float* gamma, const float* wout, bf16* wq_out, bf16* wo_out, int C) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 384 * C) wq_out[i] = (bf16)(wqkv[i] * gamma[i % C]);
    if (i < C * 128) {
        // column permutation inside each head block of 32: position s*16 + h*8 + j  <-  e = 16s + 8(j>>2) + 4h + (j&3)
        const int c = i / 128, pcol = i % 128, hh = pcol / 32, pp = pcol % 32, s = pp / 16, h = (pp / 8) & 1, j = pp & 7;
        const int e = 16 * s + 8 * (j >> 2) + 4 * h + (j & 3);
        wo_out[i] = (bf16)wout[c * 128 + hh * 32 + e];
    }
}

// ------------------------------------------------------------------------------------------------ launch decisions (host)
// The batch the batch-dependent choices look at (generation, blocks per sample of the output pass): ds_attn_fused_params.batch_hint where
// the caller gives one, else B.
int fused_batch(const ds_attn_fused_params* p) { return p->batch_hint > 0 ? p->batch_hint : p->B; }

// pixels per group of the first generation: 64 where the image is large enough to keep every CU busy with fewer, longer iterations
int group_t(int C, int N) { return (C == 96 && N >= 4096) ? 2 : 1; }

// blocks per sample: the whole grid is resident at once (2 blocks per CU; 1 for the 384-channel variant) — a second,
// partial round of blocks would double the kernel's duration
int out_blocks(int ngroups, int B, int C) {
    int nb = (C == 384 ? 256 : 512) / B;
    if (nb > ngroups) nb = ngroups;
    if (nb < 1) nb = 1;
    const int per = (ngroups + nb - 1) / nb;
    return (ngroups + per - 1) / per;
}

// second generation: every CU busy with few, long-lived blocks (a block pays 53 / 104 KB of operand staging)
int attn_out2_blocks(int N, int B, int C) {
    const int ntiles = (N + 31) / 32;
    const int nw = C == 96 ? 4 : 8, per_cu = C == 96 ? 3 : 1;
    int nb = (256 * per_cu + B - 1) / B;                      // blocks per sample that fill the chip once
    const int max_nb = (ntiles + nw - 1) / nw;                // at least one tile per wave
    if (nb > max_nb) nb = max_nb;
    if (nb < 1) nb = 1;
    const int per = (ntiles + nb - 1) / nb;
    return (ntiles + per - 1) / per;
}

// Which generation runs (ds_attn_fused_params.gen; 0 = by batch): the second-generation kernels stage 50 - 100 KB of weights per block and
// walk pixel tiles with them — measured per level at U-Net batch 16 / 32 / 64 / 128 (tools/ab.sh -m attn): context pass 53 / 70 / 95 / 176 us
// against 32 / 52 / 92 / 222 us of the first generation at C = 96, output pass 42 / 62 / 129 / 233 against 35 / 67 / 151 / 272
bool ctx2_exists(int C, int N) { return C == 96 || C == 192 || (C == 384 && N >= 1024); }
bool use_ctx2(const ds_attn_fused_params* p) {
    if (p->gen == 1 || !ctx2_exists(p->C, p->N)) return false;
    return p->gen == 2 || fused_batch(p) >= 96;
}
bool use_out2(const ds_attn_fused_params* p) {
    if (p->gen == 1 || !p->mfold || !(p->C == 96 || p->C == 192)) return false;
    return p->gen == 2 || fused_batch(p) >= (p->C == 96 ? 32 : 96);
}

int check(const ds_attn_fused_params* p) {
    DS_REQUIRE(p && p->x && p->wqkv && p->t1 && p->t2 && (p->gn_ab || p->gn_part) && p->part && p->ctx, "attn_fused: null pointer");
    DS_REQUIRE(p->C == 96 || p->C == 192 || p->C == 384, "attn_fused: C=%d unsupported (96, 192, 384)", p->C);
    DS_REQUIRE(p->B > 0 && p->N > 0 && p->nseg > 0, "attn_fused: bad sizes");
    DS_REQUIRE(p->batch_hint >= 0, "attn_fused: batch_hint must be 0 (use B) or the batch the launch decisions look at, got %d", p->batch_hint);
    if (!ds_aligned16(p->x) || !ds_aligned16(p->wqkv)) DS_FAIL(DS_EALIGN, "attn_fused: pointers must be 16-byte aligned");
    return DS_OK;
}

#if DS_BOUNDS
void attn_publish_bounds(const ds_attn_fused_params* p, int kernel, int stats_parts, hipStream_t st) {
    DsBxHost h(kernel);
    h.set(DS_BX_SRC0, p->x, (long long)p->B * p->N * p->C * 2);
    h.set(DS_BX_W, p->wqkv, (long long)384 * p->C * 2);
    h.set(DS_BX_AUX1, p->wout_perm, (long long)p->C * 128 * 2);
    h.set(DS_BX_T1, p->t1, 384 * 4).set(DS_BX_T2, p->t2, 384 * 4);
    h.set(DS_BX_GNAB, p->gn_ab, (long long)p->B * 2 * 4);
    h.set(DS_BX_GNPART, p->gn_part, (long long)p->B * p->gn_parts * 2 * 4);
    h.set(DS_BX_AUX0, p->part, (long long)p->B * 4 * p->nseg * PARTF * 4);
    h.set(DS_BX_AUX2, p->ctx, (long long)p->B * 4 * 1024 * 4);
    h.set(DS_BX_AUX3, p->label_q, p->label_q ? ((long long)(p->B - 1) * p->lq_stride + 128) * 4 : 0);
    h.set(DS_BX_BIAS, p->bias_out, (long long)p->C * 4);
    h.set(DS_BX_OUT, p->y, (long long)p->B * p->N * p->C * 2);
    h.set(DS_BX_STATS, p->stats_part, (long long)p->B * stats_parts * 2 * 4);
    h.set(DS_BX_RES, p->mfold, p->mfold ? (long long)p->B * p->C * 256 : 0);
    h.publish(st);
}
#endif

// The one launch of this file: LDS limit of the kernel, the operand extents of the bounds build, the launch, its check.
// (KERN is a template argument: DS_SET_MAX_LDS remembers per expansion, i.e. per kernel, that the limit is set)
template <auto KERN, class... Extra>
int launch(const ds_attn_fused_params* p, dim3 grid, int threads, int lds, const char* name, int bx_kernel, int stats_parts, hipStream_t st, Extra... extra) {
    DS_SET_MAX_LDS(KERN, lds, name);
#if DS_BOUNDS
    attn_publish_bounds(p, bx_kernel, stats_parts, st);
#else
    (void)bx_kernel; (void)stats_parts;
#endif
    hipLaunchKernelGGL(KERN, grid, dim3(threads), lds, st, *p, extra...);
    DS_CHECK_LAUNCH(name);
    return DS_OK;
}

template <int NKS, int T>
int launch_ctx(const ds_attn_fused_params* p, hipStream_t st) {
    return launch<attn_fused_ctx_kernel<NKS, T>>(p, dim3(p->nseg, p->B), 256, 2 * FusedXStage<NKS, T>::BYTES, "attn_fused_ctx", DS_K_ATTN_CTX, 0, st);
}

template <int NKS, int T>
int launch_out(const ds_attn_fused_params* p, hipStream_t st) {
    const int nb = out_blocks((p->N + 32 * T - 1) / (32 * T), fused_batch(p), p->C);
    return launch<attn_fused_out_kernel<NKS, T>>(p, dim3(nb, p->B), 256, 2 * FusedXStage<NKS, T>::BYTES + 2 * 4 * T * 2 * 1024, "attn_fused_out",
                                                 DS_K_ATTN_OUT, nb, st);
}

// (C = 384: two heads per block, half of the k / v weights — 100 KB)
template <int NKS, int NW, int HPW, int HG>
int launch_ctx2(const ds_attn_fused_params* p, hipStream_t st) {
    return launch<attn_ctx2_kernel<NKS, NW, HPW, HG>>(p, dim3((p->nseg + NW - 1) / NW, p->B, HG), NW * 64, C2<NKS>::LDS / HG, "attn_ctx2", DS_K_ATTN_CTX, 0, st);
}

template <int NKS, int NW>
int launch_out2(const ds_attn_fused_params* p, hipStream_t st) {
    const int nb = attn_out2_blocks(p->N, fused_batch(p), p->C), ntiles = (p->N + 31) / 32, per = (ntiles + nb - 1) / nb;
    const bf16* const mfold = reinterpret_cast<const bf16*>(p->mfold);
    hipLaunchKernelGGL(attn_fold_out_kernel, dim3(p->C / 32, p->B), dim3(256), 0, st, p->ctx, reinterpret_cast<const bf16*>(p->wout_perm),
                       reinterpret_cast<bf16*>(p->mfold), p->C);
    DS_CHECK_LAUNCH("attn_fold_out");
    return launch<attn_out2_kernel<NKS, NW>>(p, dim3(nb, p->B), NW * 64, O2<NKS>::LDS, "attn_out2", DS_K_ATTN_OUT, nb, st, mfold, per);
}

}  // namespace

extern "C" int ds_pack_attn_fused(const float* wqkv, const float* gamma, const float* wout, void* wq_bf16, void* wo_perm_bf16, int C,
                                  void* stream) {
    DS_REQUIRE(wqkv && gamma && wout && wq_bf16 && wo_perm_bf16 && C > 0, "pack_attn_fused: bad args");
    hipLaunchKernelGGL(pack_attn_kernel, dim3((384 * C + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), wqkv, gamma,
                       wout, (bf16*)wq_bf16, (bf16*)wo_perm_bf16, C);
    DS_CHECK_LAUNCH("pack_attn_fused");
    return DS_OK;
}

#if DS_BOUNDS
extern "C" int ds_bounds_fetch_attn_fused(ds_bounds_rec* out, int reset) { return ds_bounds_fetch_tu(out, reset); }
#endif

extern "C" int ds_attn_fused_context(const ds_attn_fused_params* p, void* stream) {
    int rc = check(p);
    if (rc) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int T = group_t(p->C, p->N);
    if (use_ctx2(p)) rc = p->C == 96 ? launch_ctx2<6, 4, 4, 1>(p, st) : p->C == 192 ? launch_ctx2<12, 8, 4, 1>(p, st) : launch_ctx2<24, 8, 2, 2>(p, st);
    else if (p->C == 96) rc = T == 2 ? launch_ctx<6, 2>(p, st) : launch_ctx<6, 1>(p, st);
    else if (p->C == 192) rc = launch_ctx<12, 1>(p, st);
    else rc = launch_ctx<24, 1>(p, st);
    if (rc) return rc;
    ds_attn_params q;
    memset(&q, 0, sizeof(q));
    q.B = p->B; q.N = p->N; q.heads = 4; q.nseg = p->nseg; q.part = p->part; q.ctx = p->ctx;
    return ds_linattn_launch_combine(&q, st);
}

extern "C" int ds_attn_fused_output(const ds_attn_fused_params* p, void* stream) {
    int rc = check(p);
    if (rc) return rc;
    DS_REQUIRE(p->wout_perm && p->bias_out && p->y, "attn_fused_output: null pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (use_out2(p)) {
        DS_REQUIRE(ds_aligned16(p->mfold) && ds_aligned16(p->y), "attn_fused_output: mfold / y must be 16-byte aligned");
        return p->C == 96 ? launch_out2<6, 4>(p, st) : launch_out2<12, 8>(p, st);
    }
    const int T = group_t(p->C, p->N);
    if (p->C == 96) return T == 2 ? launch_out<6, 2>(p, st) : launch_out<6, 1>(p, st);
    if (p->C == 192) return launch_out<12, 1>(p, st);
    return launch_out<24, 1>(p, st);
}

extern "C" int ds_attn_fused_segments_gen(int B, int N, int C, int gen) {
    ds_attn_fused_params q;
    memset(&q, 0, sizeof(q));
    q.B = B; q.N = N; q.C = C; q.gen = gen;
    const int ntiles = (N + 31) / 32;
    if (use_ctx2(&q)) {
        int s = (C == 384 ? 1024 : 2048) / (B > 0 ? B : 1);
        if (s > 64) s = 64;
        if (s > ntiles) s = ntiles;
        return s < 1 ? 1 : s;
    }
    int s = N / 128;                                            // >= 128-pixel segments; <= 32 keeps the combine short
    if (s > 32) s = 32;
    return s < 1 ? 1 : s;
}

extern "C" int ds_attn_fused_segments(int B, int N, int C) { return ds_attn_fused_segments_gen(B, N, C, 0); }

extern "C" int ds_attn_fused_generations(const ds_attn_fused_params* p) { return (use_ctx2(p) ? 1 : 0) | (use_out2(p) ? 2 : 0); }

extern "C" int ds_attn_fused_stats_parts(const ds_attn_fused_params* p) {
    if (use_out2(p)) return attn_out2_blocks(p->N, fused_batch(p), p->C);
    const int tp = 32 * group_t(p->C, p->N);
    return out_blocks((p->N + tp - 1) / tp, fused_batch(p), p->C);
}
