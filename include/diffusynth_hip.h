/*
 * diffusynth_hip.h — C ABI of libdiffusynth_hip.so (gfx950 / MI355X).
 *
 * The reference (WxuanYuan/diffusynth) is pure Python on PyTorch eager: it has no FFI, plugin or
 * operator registry.  Its boundary for the denoising hot path is the Python duck type
 *     eps = model(x, mapped_t, condition)           model/DiffSynthSampler.py:312,319
 * plus the nn.Module state-dict names of model/diffusion.py:21-175.  The entry points below are
 * therefore the ATen operator call sites of that path, one exported function per kernel class
 * (SURVEY.md §8a/§8b); each comment cites the reference line(s) the function replaces.  The Python
 * host code (diffusynth_amd/) mirrors ConditionedUnet / DiffSynthSampler on top of these and binds
 * them with ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - activations between kernels are channels-last: [B][H][W][C], element type ds_dtype;
 *     the public boundary tensors (x, eps, latents) stay NCHW fp32 like the reference;
 *   - functions only enqueue work on `stream` (a hipStream_t passed as void*), never synchronise,
 *     never allocate, and are re-entrant (no global mutable state) => HIP-graph capturable;
 *   - return 0 on success or a negative DS_E* code; ds_last_error_string() (thread local) explains.
 */
#ifndef DIFFUSYNTH_HIP_H
#define DIFFUSYNTH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DS_OK 0
#define DS_EINVAL (-1)   /* bad argument / unsupported shape */
#define DS_ELAUNCH (-2)  /* HIP launch error */
#define DS_EALIGN (-3)   /* pointer or channel count not aligned as the kernel requires */

typedef enum { DS_F32 = 0, DS_BF16 = 1 } ds_dtype;
typedef enum { DS_ACT_NONE = 0, DS_ACT_GELU = 1, DS_ACT_SILU = 2, DS_ACT_RELU = 3 } ds_act;

const char* ds_last_error_string(void);
int ds_abi_version(void);

/* ---------------------------------------------------------------- convolution (implicit GEMM on MFMA)
 * Replaces nn.Conv2d 3x3 p1 (diffusion_components.py:64,122,125; diffusion.py:174), 1x1
 * (components:128,93,180-181,263-264), Downsample Conv2d(4,2,1) (components:37-39), Upsample
 * ConvTranspose2d(4,2,1) (components:32-34, as 4 sub-pixel 2x2 convolutions), init Conv2d 7x7
 * (diffusion.py:82) and the VQGAN decoder convolutions (VQGAN.py:154-171,190-221,254-259,342).
 * Fused: zero-copy skip concat of two sources (components:236-249), GroupNorm(1,C) of the INPUT
 * folded into weights/epilogue (components:121,124,148), bias, GELU/SiLU/ReLU (components:123),
 * residual add (components:139,29) and per-sample sum / sum-of-squares partials for the next
 * GroupNorm. */
#define DS_CONV_TILE_128x192 0
#define DS_CONV_TILE_256x96 1
#define DS_CONV_TILE_128x32 2
#define DS_CONV_TILE_64x96 3          /* 64 x 192 block tile (name kept for ABI stability) */
/* (ids 4 .. 10 were the first- and second-generation LDS-halo kernels, retired in round 3: ds_conv_igemm rejects them) */
#define DS_CONV_TILE_HALO3_256x96 11     /* 3x3 stride-1 pad-1, bf16 (conv3x3_halo3.hip): 256-pixel patch x 96 channels per block (4 waves of 64 px x 96 ch,
                                            two blocks per CU), the input halo of a 32-channel chunk staged once in LDS (XOR-swizzled 64-byte rows),
                                            16x16x32 MFMAs, hand-scheduled K loop; wk_order = 1; fused res_conv, split precision (flags) and split-K
                                            (ksplit dividing Cin / 32, raw slices to slab + ds_conv_splitk_reduce) supported */
#define DS_CONV_TILE_QUAD_HALO3 12       /* Conv2d(4, 2, 1) and ConvTranspose2d(4, 2, 1) (Downsample / Upsample, components:88-93) on the
                                            HALO3 pipeline with four taps per chunk (conv_quad_halo3.hip): bf16, wk_order = 2, Cin % 32 == 0
                                            with (transposed ? 1 : 4) * Cin / 32 a multiple of 6; transposed: cout_pad = 4 * Cout, Cout % 96 == 0 */

/* ds_conv_params.flags (DS_CONV_TILE_HALO3_256x96): the split-precision tier runs a 3x3 convolution of fp32 tensors on bf16 matrix
 * cores as x*w ~ x_hi*w_hi + x_lo*w_hi + x_hi*w_lo (fp32 accumulate; x = x_hi + x_lo to 2^-17).
 *   SPLIT_IN : src0 = 2C bf16 channels per pixel (the hi plane, then the lo plane, of a C-channel fp32 tensor), C0 = 2C; wpk holds
 *              3C input channels (chunk-major, wk_order = 1; GroupNorm gain folded before the split): per 32-channel source chunk c the
 *              three virtual chunks [W_hi_c | W_lo_c | W_hi_c], the first two for the hi plane's chunk c, the third for the lo plane's
 *              (diffusynth_amd/engine.py:split3_weight).  DS_CONV_TILE_QUAD_HALO3 takes [W_hi | W_hi | W_lo] over 3C input channels.
 *   OUT_SPLIT: the result is stored as hi / lo bf16 planes (out_C = 2 * Cout bf16 channels): the SPLIT_IN format of the next layer
 *   OUT_F32  : the result (+ an fp32 residual `res`) is stored as fp32 (out_C counts fp32 elements) */
#define DS_CONV_F_SPLIT_IN 1
#define DS_CONV_F_OUT_SPLIT 2
#define DS_CONV_F_OUT_F32 4
#define DS_CONV_F_IN_F32 8               /* ds_conv1x1_x3 only: src0 / src1 are fp32 tensors, split into hi / lo bf16 inside the kernel */

#define DS_CONV_TILE_HALO3_N16 13        /* 3x3 stride 1 pad 1 with Cout <= 16 (the U-Net's final 96 -> 4 convolution; conv3x3_smalln.hip): bf16, wk_order = 1 with
                                            cout_pad = 16, Cin % 32 == 0, bias (+ GELU) epilogue only */

typedef struct {
    /* input: channels [0,C0) come from src0, [C0,C0+C1) from src1 placed at (off_h1,off_w1) */
    const void* src0; const void* src1;
    int32_t C0, C1, H, W, H1, W1, off_h1, off_w1;
    /* weights packed by ds_pack_conv_weight: [phase][kchunks][cout_pad][32] */
    const void* wpk;
    int32_t Cout, cout_pad, KH, KW, stride, pad_h, pad_w;
    int32_t Ho, Wo;              /* output positions iterated by the GEMM M dimension (per sample)   */
    int32_t transposed;          /* 1: 4-phase ConvTranspose2d(4,2,1); KH=KW=2, out is 2Ho x 2Wo     */
    /* output */
    void* out;                   /* NHWC, ds_dtype, out_C channels per pixel, written at out_c0.. in 16-B
                                    groups: Cout is rounded up to 4 (fp32) / 8 (bf16), pad channels = 0 */
    int32_t out_C, out_c0;
    int32_t out_nchw_f32;        /* must be 0 (reserved; use ds_nhwc_to_nchw for the fp32 NCHW boundary)  */
    /* epilogue */
    const float* bias;           /* [Cout] or NULL                                                    */
    const float* gn_ab;          /* [B][2] = (rstd, rstd*mean) of the input's GroupNorm(1,C), or NULL */
    const float* fold_t1; const float* fold_t2; /* [ncls][Cout]; t1 already contains the bias         */
    int32_t ncls;                /* 1 or 9 (3x3 pad 1 border classes)                                 */
    int32_t act;                 /* DS_ACT_NONE or DS_ACT_GELU, applied before the residual           */
    const void* res;             /* NHWC residual with out_C channels (same indexing as out) or NULL  */
    float* stats_part;           /* [B][gridDim.x*gridDim.y][2] partial (sum, sumsq) of stored values */
    int32_t B, dtype, tile;
    /* split-K (halo tiles only): ksplit > 1 makes ds_conv_igemm write raw fp32 partial sums of K-slice z to
     * slab[z][B][Ho*Wo][roundup(Cout,8)]; ds_conv_splitk_reduce then sums the slices and runs the epilogue. */
    int32_t ksplit;
    int32_t wk_order;            /* K order of wpk: 2 = quad tiles [chunk][2x2 tap][cout_pad][32] of DS_CONV_TILE_QUAD_HALO3 (transposed: chunk =
                                    Cin / 32 group, row n = phase * Cout + co holds w[ci][co][3 - py - 2a][3 - px - 2b]; strided: chunk =
                                    (parity plane, Cin / 32 group), row co holds w[co][ci][1 - p + 2a][1 - q + 2b]; packed on the host side by
                                    diffusynth_amd/engine.py:pack_quad_weights),
                                    0 = tap-major [tap*NCC + cc] (generic kernel),
                                    1 = chunk-major [cc*9 + tap] (DS_CONV_TILE_HALO3_256x96 / _N16: one pointer increment per step) */
    int32_t batch_hint;          /* 0 = B.  The batch the launcher's batch-dependent choice looks at instead of B, as ds_dwconv_params.batch_hint:
                                    the two-samples-per-block tile of the split-precision DS_CONV_TILE_HALO3_256x96 launches (images of at most
                                    16 x 8) is taken when this batch is >= 2; the kernel runs any B >= 1 (a lone last sample has its block to
                                    itself).  Grids, slabs and buffer extents always follow B.  ksplit is the caller's choice already.
                                    Every entry point that takes this struct rejects a negative value (ds_conv_igemm for all the tiles it
                                    dispatches, ds_conv1x1_x3, ds_conv_splitk_reduce); only that one launch reads it. */
    float* slab;
    /* alternative to gn_ab: the producer's raw (sum, sumsq) partials [B][gn_parts][2]; every wave reduces them
     * itself (float64) at kernel start, which removes the ds_gn_finalize launch between producer and consumer */
    const float* gn_part; int32_t gn_parts; float gn_eps; double gn_count;
    /* DS_CONV_TILE_HALO3_256x96 only: the ConvNeXt block's 1x1 res_conv (components:128,139) fused into this launch.
     * res_steps = (res_C0 + res_C1) / 32 > 0 (a multiple of 3) runs that many 32-channel K steps over the block input x
     * (two-source zero-copy concat like src0/src1 of the generic kernel, same H x W as the output) in front of the 3x3
     * K loop: acc = sum Wres[n][c] x[c] at the centre tap, divided by the GroupNorm factor a in registers, then the
     * nine-tap chunks accumulate on top and the epilogue's a * acc + shift yields res + a * conv3x3.  wpk must hold
     * res_steps tiles [cout_pad][32] (k_order 1 packing of the 1x1 weight) followed by the 3x3 tiles, res must be NULL,
     * res_bias[Cout] is added to every border class. */
    const void* res_src0; const void* res_src1;
    int32_t res_C0, res_C1, res_H1, res_W1, res_off_h1, res_off_w1;
    int32_t res_steps;
    int32_t flags;               /* DS_CONV_TILE_HALO3_256x96 only, 0 elsewhere: DS_CONV_F_* (split-precision tier) */
    const float* res_bias;
} ds_conv_params;

int ds_conv_igemm(const ds_conv_params* p, void* stream);
/* fp32 NHWC [npix][C] -> hi / lo bf16 planes [npix][2C] (the DS_CONV_F_SPLIT_IN format) for tensors produced by fp32 kernels */
int ds_split_planes(const float* x, void* out_bf16, long long npix, int C, void* stream);
/* 1x1 convolution (stride 1) of fp32 NHWC tensors in split precision on the bf16 matrix cores (tier "bf16x3": to_qkv, to_out, res_conv —
 * diffusion_components.py:128,139,263-264): flags = DS_CONV_F_IN_F32 | DS_CONV_F_OUT_F32, dtype DS_BF16, src0 / src1 fp32 with C0, C1
 * multiples of 32 (src1 placed at (off_h1, off_w1): pad_and_concat, components:210-249), wpk = [chunk of 32 input channels][hi, lo]
 * [cout_pad][32] bf16 with cout_pad a multiple of 96 (ds_conv1x1_x3_weight_elems elements; hi = bf16(w), lo = bf16(w - hi), PreNorm gain
 * folded before the split), out / res fp32 [B][H*W][out_C], bias or gn_ab + fold_t1 / fold_t2 (ncls = 1), optional stats_part
 * [B][ds_conv1x1_x3_stats_parts][2]. */
int ds_conv1x1_x3(const ds_conv_params* p, void* stream);
int ds_conv1x1_x3_stats_parts(const ds_conv_params* p);
size_t ds_conv1x1_x3_weight_elems(int Cin, int Cout);
int ds_conv_splitk_reduce(const ds_conv_params* p, void* stream);
/* number of (sum,sumsq) partial slots per sample that ds_conv_igemm writes for this problem */
int ds_conv_stats_parts(const ds_conv_params* p);
/* block N-tile of a tile id (weights must be packed with cout_pad = multiple of it) */
int ds_conv_tile_bn(int tile);

/* OIHW fp32 (or IOHW for transposed) -> packed kernel layout, optionally pre-scaled per input
 * channel by a GroupNorm gain (the GN fold).  dst holds nphase*kchunks*cout_pad*32 elements. */
typedef struct {
    const float* w;              /* [Cout][Cin][KH][KW], or [Cin][Cout][4][4] when transposed         */
    const float* gamma;          /* [Cin] or NULL                                                     */
    void* dst; int32_t dtype;
    int32_t Cout, Cin, cin_pad, KH, KW, cout_pad, transposed;
    int32_t k_order;             /* 0: k = tap*cin_pad + c (default); 1: chunk-major k = (c/32)*KH*KW*32 + tap*32 + c%32
                                    (cin_pad must be a multiple of 32; ds_conv_params.wk_order = 1)              */
} ds_pack_conv_params;
int ds_pack_conv_weight(const ds_pack_conv_params* p, void* stream);
size_t ds_pack_conv_elems(int Cin_pad, int KH, int KW, int cout_pad, int transposed);
/* fold tables for a GroupNorm(1,C)-fed convolution: t1[cls][o] = bias[o] + sum_{taps in cls,c} w*beta[c],
 * t2[cls][o] = sum w*gamma[c]; ncls = 9 for 3x3 pad 1, 1 for 1x1. */
int ds_conv_fold_tables(const float* w, const float* bias, const float* gamma, const float* beta,
                        int Cout, int Cin, int KH, int KW, float* t1, float* t2, void* stream);

/* ---------------------------------------------------------------- depthwise 7x7 (+bias +time bias)
 * Replaces ConvNextBlock.ds_conv and the broadcast add of mlp(time_emb) (components:118,131-136);
 * reads the skip concat from two sources; emits GroupNorm partials. */
typedef struct {
    const void* src0; const void* src1;
    int32_t C0, C1, H, W, H1, W1, off_h1, off_w1;
    const float* wt;             /* [49][C] tap-major fp32 (ds_pack_dw_weight)                        */
    const float* bias;           /* [C]                                                                */
    const float* tbias;          /* [B][tb_stride] time bias, this block's slice starts at tbias, or NULL */
    int32_t tb_stride;
    void* out;                   /* NHWC [B][H][W][C]                                                  */
    float* stats_part;           /* [B][parts][2]                                                      */
    int32_t B, dtype;
    /* bf16 only, optional: Toeplitz-expanded weights (ds_pack_dw_weight_mfma).  When given (and the channel
     * counts are multiples of 32) the 7x7 stencil runs on the matrix cores: per channel, a 16x16 output block
     * is A[16 rows][(dh, 24 cols)] x T_c[(dh, 24 cols)][16 cols] with T_c the banded matrix of the 7 row taps. */
    const void* wexp;
    int32_t out_split;           /* fp32 only: store the result as two bf16 planes (hi = bf16(v), then lo = bf16(v - hi)) of a 2C-channel image,
                                    the DS_CONV_F_SPLIT_IN input format of the split-precision 3x3 convolution */
    int32_t strip;               /* fp32 32-channel blocks only: 0 = the library chooses between the tile kernel and the strip kernel (an LDS ring walking
                                    down a 16-column strip: every input row leaves HBM once) by shape and batch, 1 = the strip kernel wherever its shape
                                    conditions hold (W >= 16, H >= 32), 2 = never.  Outputs are identical bit for bit; the statistics partials are
                                    grouped differently (ds_dwconv_stats_parts answers for the same setting) */
    int32_t batch_hint;          /* 0 = B.  The batch every batch-dependent launch decision looks at instead of B (tile or strip kernel and the row
                                    ranges per image of the fp32 kernels, the chunk length of the bf16 matrix-core kernel): the shared prefix of a
                                    paired classifier-free-guidance plan runs at half the batch and passes the FULL batch here, so that its GroupNorm
                                    partials are grouped - and therefore rounded - exactly as the plain plan's.  A caller that passes one fixed
                                    value at every B gets the same choices, and the same bits per sample, at every B: a chunk of several whole
                                    samples (bf16, images of fewer than 8 tiles) is chosen when it divides THIS batch, and the last chunk of a
                                    B it does not divide is short (one partial per sample either way) */
} ds_dwconv_params;
int ds_dwconv7(const ds_dwconv_params* p, void* stream);
int ds_dwconv_stats_parts(const ds_dwconv_params* p);
/* What ds_dwconv7 would launch for p, for plan inspection (no launch, pointers are not read except for NULL tests):
 * *family = DS_DW_DIRECT / DS_DW_TILE / DS_DW_STRIP / DS_DW_MFMA; *ranges = GroupNorm partials per image and channel block that follow from a
 * batch-dependent choice (strip kernel: row ranges per image, `hparts`; matrix-core kernel: chunks per image; else 1); *samples_per_chunk =
 * whole samples one chunk of the matrix-core kernel covers (1 elsewhere).  Returns DS_OK. */
#define DS_DW_DIRECT 0
#define DS_DW_TILE 1
#define DS_DW_STRIP 2
#define DS_DW_MFMA 3
int ds_dwconv_launch_choice(const ds_dwconv_params* p, int32_t* family, int32_t* ranges, int32_t* samples_per_chunk);
int ds_pack_dw_weight(const float* w_c1kk, int C, float* dst_tap_major, void* stream);
/* [C][1][7][7] fp32 -> [C][6 k-steps][64 lanes][8] bf16 B-operand fragments of v_mfma_f32_16x16x32_bf16 */
int ds_pack_dw_weight_mfma(const float* w_c1kk, int C, void* dst_bf16, void* stream);

/* ---------------------------------------------------------------- GroupNorm
 * nn.GroupNorm(1,C) (components:121,124,148,181,264): statistics are produced as partials by the
 * producing kernel; ds_gn_finalize reduces them (float64) to (rstd, rstd*mean) per sample.
 * ds_gn_apply is the explicit normalise+affine(+act)(+residual) pass used where the norm cannot be
 * folded into a following convolution (attention output norm + Residual, components:181,29; VQGAN
 * Normalize + swish/ReLU, VQGAN.py:12-27,225-226,360-361).  ds_gn_stats computes per-(sample,group)
 * statistics of a tensor directly (groups > 1: components:65, VQGAN.py:17). */
int ds_gn_finalize(const float* stats_part, int B, int parts, double count, float eps, float* gn_ab, void* stream);
int ds_gn_stats(const void* x, int dtype, int B, int HW, int C, int G, float eps, float* gn_ab, void* stream);
/* the same statistics as one streaming pass (16-byte loads over whole pixels, per-channel block partials in `ws`, channels
 * folded into groups in float64 by a second tiny launch): what the engines use; C must be a multiple of 4 (fp32) / 8 (bf16). */
size_t ds_gn_stats_ws_floats(int B, int HW, int C);
int ds_gn_stats_stream(const void* x, int dtype, int B, int HW, int C, int G, float eps, float* ws, float* gn_ab, void* stream);
typedef struct {
    const void* x; const void* res; void* out;   /* NHWC [B][HW][C]; res may be NULL                  */
    const float* gn_ab;          /* [B][G][2]                                                          */
    const float* gamma; const float* beta;       /* [C]                                                */
    const float* cbias;          /* [B][cb_stride] per-(sample,channel) add after norm+act (components:98-101), or NULL    */
    int32_t cb_stride;
    int32_t B, HW, C, G, act, dtype;
    /* G == 1 only: raw (sum, sumsq) partials of x instead of gn_ab (gn_ab NULL) — the kernel reduces them itself, like
     * ds_conv_params.gn_part, which saves the ds_gn_finalize launch */
    const float* gn_part; int32_t gn_parts; float gn_eps; double gn_count;
} ds_gn_apply_params;
int ds_gn_apply(const ds_gn_apply_params* p, void* stream);

/* ---------------------------------------------------------------- linear attention
 * LinearCrossAttentionAdd.forward / LinearCrossAttention.forward (components:271-293,187-207) and
 * VQGAN LinearAttention (VQGAN.py:261-272) on a precomputed qkv tensor [B][N][3*heads*32]:
 *   pass 1: per (sample, head, segment) softmax_n(k) . v^T partial context (max, sum, 32x32)
 *   combine: merges segments (+ the optional extra key/value token of linear_cat)
 *   pass 2: q~ = softmax_d(q + label_q) * scale;  out[n][h*32+e] = sum_d ctx[d][e] q~[d]
 * Limits (refused with an error code otherwise): heads <= 8 (pass 2 keeps every head's context in LDS: (heads * 1056 + 9216) * 4
 * bytes in fp32, 70 656 at 8 heads) and 1 <= nseg <= N.  With nseg < N a segment can still be empty (per = ceil(N / nseg) pixels
 * each, e.g. N = 10, nseg = 7: segments 5 and 6): it contributes (max = -inf, sum = 0, context = 0), which the combine weighs with
 * exp(-inf) = 0.  The label strides are counted in floats and may exceed heads * 32.                   */
typedef struct {
    const void* qkv;             /* [B][N][3*heads*32]: q | k | v, each (head, d)                      */
    int32_t B, N, heads, dtype;
    int32_t nseg;                /* segments of N used by pass 1                                       */
    float* part;                 /* [B][heads][nseg][32+32+1024] scratch                               */
    float* ctx;                  /* [B][heads][32][32]                                                 */
    const float* label_q;        /* [B][lq_stride]: + (head*32+d); NULL = none                         */
    const float* label_k; const float* label_v;  /* linear_cat extra token, [B][l*_stride]; NULL = none */
    int32_t lq_stride, lk_stride, lv_stride;
    int32_t q_softmax;           /* 1: softmax over d and * scale (U-Net); 0: raw q (VQGAN)            */
    float scale;
    void* out;                   /* [B][N][heads*32]                                                   */
} ds_attn_params;
int ds_linattn_context(const ds_attn_params* p, void* stream);   /* pass 1 + combine */
int ds_linattn_output(const ds_attn_params* p, void* stream);    /* pass 2           */
size_t ds_linattn_part_floats(int B, int heads, int nseg);

/* Fused form of the whole Residual(PreNorm(LinearCrossAttentionAdd)) block up to the output GroupNorm
 * (components:142-152,252-293), bf16, heads = 4 x 32, C in {96,192,384}: x is the only activation stream
 * (no qkv tensor).  context = k/v projection + softmax_n + k.v^T (+ segment combine); output = q projection
 * + softmax_d + ctx^T.q + to_out 1x1 + bias + GroupNorm partials.  Follow with ds_gn_finalize + ds_gn_apply(res = x). */
typedef struct {
    const void* x;               /* [B][N][C] bf16                                                     */
    int32_t B, N, C, nseg;
    const void* wqkv;            /* [384][C] bf16 row-major, PreNorm gain folded in (ds_pack_attn_fused) */
    const float* t1; const float* t2;   /* [384] fold tables of the PreNorm (ds_conv_fold_tables, bias NULL) */
    const float* gn_ab;          /* [B][2] statistics of x, or NULL when gn_part is given               */
    const float* gn_part; int32_t gn_parts; float gn_eps; double gn_count;   /* raw partials of x (see ds_conv_params) */
    const float* label_q;        /* [B][lq_stride] or NULL                                              */
    int32_t lq_stride; float scale;
    float* part; float* ctx;     /* scratch as in ds_attn_params (heads = 4)                            */
    const void* wout_perm;       /* [C][128] bf16, columns permuted per head (ds_pack_attn_fused)       */
    const float* bias_out;       /* [C]                                                                 */
    void* y;                     /* [B][N][C] bf16 = to_out.0 output                                    */
    float* stats_part;           /* [B][ds_attn_fused_stats_parts][2]                                   */
    void* mfold;                 /* [B][C][128] bf16 scratch or NULL.  Given (C = 96 / 192): the output pass runs attn_out2 — to_out folded
                                    into the per-sample context (M_b = Wout . ctx_b^T), wave = pixel tile, no LDS exchange (attn_out2.hpp);
                                    NULL: the first-generation output kernel.  ds_attn_fused_stats_parts depends on it.               */
    int32_t gen;                 /* kernel generation: 0 = chosen by the batch (the second-generation kernels — wave = 32-pixel tile, weights in
                                    LDS, attn_out2.hpp — pay from about 100 samples on: context pass from B >= 96, output pass from B >= 32 at
                                    C = 96 and B >= 96 at C = 192; below that a block stages 50 - 100 KB of weights for a handful of tiles);
                                    1 / 2 = the first / second generation wherever it exists (tests, A/B)                              */
    int32_t batch_hint;          /* 0 = B.  The batch every batch-dependent launch decision looks at instead of B (gen = 0: which generation runs;
                                    blocks per sample of the output pass = ds_attn_fused_stats_parts), as ds_dwconv_params.batch_hint: a caller
                                    that wants a sample's partial sums grouped the same way in every batch passes one fixed value, and takes
                                    nseg from ds_attn_fused_segments at that same value.  Grids and buffer extents always follow B.     */
} ds_attn_fused_params;
int ds_pack_attn_fused(const float* wqkv_384xC, const float* gamma_C, const float* wout_Cx128, void* wqkv_bf16,
                       void* wout_perm_bf16, int C, void* stream);
int ds_attn_fused_context(const ds_attn_fused_params* p, void* stream);
int ds_attn_fused_output(const ds_attn_fused_params* p, void* stream);
int ds_attn_fused_stats_parts(const ds_attn_fused_params* p);
/* segments of partials per (sample, head) the context pass wants for gen = 0 at this shape (nseg; part = ds_linattn_part_floats(B, 4, nseg)):
 * the second generation works one segment per wave and wants one round of blocks (2048 / B, 1024 / B at C = 384), the first N / 128 <= 32 */
int ds_attn_fused_segments(int B, int N, int C);
/* the same for an explicit kernel generation (ds_attn_fused_params.gen = 1 / 2; 0 = by batch, as above): a caller that forces a generation
 * sizes `part` from THIS count */
int ds_attn_fused_segments_gen(int B, int N, int C, int gen);
/* which generation the two passes would run for p, for plan inspection (no launch): bit 0 = the context pass runs the second generation,
 * bit 1 = the output pass does */
int ds_attn_fused_generations(const ds_attn_fused_params* p);
/* Limits of both passes (tests/test_hip_attn_paths.py runs each): nseg is any count >= 1.  The pixels are cut into ceil(units / nseg) units per
 * segment (units: 32-pixel tiles; 64-pixel groups in the first generation at C = 96, N >= 4096); a count above the number of units leaves
 * the surplus segments empty — they write the neutral partial (max -inf, sum 0, context 0) and the combine gives them weight 0 — so `part`
 * is always ds_linattn_part_floats(B, 4, nseg) and every one of its partials is written.  ds_attn_fused_segments(_gen) look at B alone:
 * a caller with a batch_hint passes the hint as B.  Every block of the output pass has at least one tile, so every stats_part slot is
 * written by a block with work.  label_q rows are lq_stride floats apart and only their first 128 are read. */

/* ---------------------------------------------------------------- fused LinearAttention of the VQGAN (bf16 tier; csrc/vq_attn.hip)
 * VQGAN.py:246-272 (heads = 1, dim_head = 32, softmax over n on k only): q enters linearly, so after the context the block is one 1x1
 * convolution with a per-sample weight, y = (Wnin + Wout ctx_b^T Wq) x + bias.  Replaces to_qkv + ds_linattn_context + ds_linattn_output +
 * to_out / nin_shortcut of the decoder / encoder plans — no qkv tensor; x is read twice, y written once.  C in {80, 160}.
 *   ds_vq_attn_context: ctx[b][d][e] (softmax_n(Wk x) (Wv x)^T, segment partials merged);
 *   ds_vq_attn_output:  W_b per sample (fp32 fold, bf16 operands), y = W_b x + bias, optional per-channel statistics of y. */
typedef struct {
    const void* x;               /* [B][N][C] bf16                                                      */
    int32_t B, N, C, nseg;       /* nseg = ds_vq_attn_segments(B, N, C): 4 per block (one partial per wave) */
    const void* wqkv;            /* [96][C] bf16 = to_qkv.weight (rows q | k | v)                       */
    const float* wq;             /* [32][C] fp32 = to_qkv.weight[:32]                                   */
    const float* wout;           /* [C][32] fp32 = to_out.weight                                        */
    const float* wnin;           /* [C][C] fp32 = nin_shortcut.weight, or NULL (with_skip = False)      */
    const float* bias;           /* [C] = to_out.bias (+ nin_shortcut.bias)                             */
    float* part; float* ctx;     /* scratch: ds_linattn_part_floats(B, 1, nseg) floats / B * 1024 floats */
    void* wfold;                 /* scratch: ds_vq_attn_wfold_bytes(B, C)                               */
    void* y;                     /* [B][N][C] bf16                                                      */
    float* stats_ws;             /* optional [B][nseg / 4][C][2]: per-channel (sum, sum of squares) of the stored y per block —
                                    ds_gn_stats_finish(slots = nseg / 4) turns them into the next Normalize's statistics */
} ds_vq_attn_params;
int ds_vq_attn_segments(int B, int N, int C);
size_t ds_vq_attn_wfold_bytes(int B, int C);
int ds_vq_attn_context(const ds_vq_attn_params* p, void* stream);
int ds_vq_attn_output(const ds_vq_attn_params* p, void* stream);

/* ---------------------------------------------------------------- fused linear attention, split precision (tier "bf16x3")
 * The same block (Residual(PreNorm(LinearCrossAttentionAdd)) up to the output GroupNorm, components:142-152,252-293) on FP32 tensors,
 * every dense product as x_hi w_hi + x_lo w_hi + x_hi w_lo on the bf16 matrix cores with fp32 accumulation (csrc/attn_x3.hip): replaces
 * to_qkv (ds_conv1x1_x3) + ds_linattn_context + ds_linattn_output + to_out of that tier — no qkv tensor.
 *   ds_attn_x3_context: k / v / q projections of x (read once from HBM), softmax_n(k), ctx = k v^T per (sample, head) (+ segment combine),
 *                       softmax_d(q) * scale written as ready-made MFMA operands ("q planes");
 *   ds_attn_x3_output:  M_b = Wout ctx_b^T per sample, y = M_b q~ + bias (fp32 NHWC) + GroupNorm partials of y (form A: follow with
 *                       ds_gn_apply(res = x), whose gn_part form reduces stats_part itself), or the finished block output (form B, `out`).
 * heads = 4 x 32, C in {96, 192, 384}. */
typedef struct {
    const float* x;              /* [B][N][C] fp32                                                      */
    int32_t B, N, C, nseg;       /* nseg: ds_attn_x3_segments(B, N, C) (one segment of partials per wave) */
    const void* wqkv_hl;         /* [2][384][C] bf16: hi plane, lo plane of to_qkv.weight * PreNorm gain (ds_pack_attn_x3) */
    const float* t1; const float* t2;   /* [384] fold tables of the PreNorm (ds_conv_fold_tables, bias NULL) */
    const float* gn_ab;          /* [B][2] statistics of x, or NULL when gn_part is given               */
    const float* gn_part; int32_t gn_parts; float gn_eps; double gn_count;   /* raw partials of x (see ds_conv_params) */
    const float* label_q;        /* [B][lq_stride] or NULL                                              */
    int32_t lq_stride; float scale;
    float* part; float* ctx;     /* scratch as in ds_attn_params (heads = 4): ds_linattn_part_floats(B, 4, nseg) / B*4*1024 floats */
    void* qplanes;               /* scratch, ds_attn_x3_qplane_bytes(B, N)                              */
    void* mfold;                 /* scratch, ds_attn_x3_mfold_bytes(B, C)                               */
    const float* wout;           /* [C][128] fp32 = to_out.0.weight                                     */
    const float* bias_out;       /* [C]                                                                 */
    float* y;                    /* [B][N][C] fp32 = to_out.0 output (form A), or NULL with `out` (form B)   */
    float* stats_part;           /* [B][ds_attn_x3_stats_parts][2] (form A: may be NULL; form B: required scratch) */
    /* form B — the whole Residual(PreNorm(attention)) block: out = x + GroupNorm(1, C)(y) * on_gamma + on_beta (to_out.1, components:264 /
     * :22-29) without materialising y.  ds_attn_x3_output then runs pass 2 TWICE: once for the statistics of y alone, once more to
     * normalise it and add the residual while it is computed — two matrix passes instead of a 3 C N x 4 B apply pass over HBM.   */
    float* out;                  /* [B][N][C] fp32 or NULL                                              */
    const float* on_gamma; const float* on_beta;   /* [C] affine of the output GroupNorm (to_out.1)     */
    float on_eps;
    int32_t batch_hint;          /* 0 = B.  The batch the batch-dependent launch decision looks at instead of B (pixel tiles per block of the output
                                    pass, hence ds_attn_x3_stats_parts), as ds_dwconv_params.batch_hint; nseg is the caller's: from
                                    ds_attn_x3_segments at that same value.  Grids and buffer extents always follow B. */
    void* out_planes;            /* form B: the block output also (or, with out = NULL, only) as hi / lo bf16 planes [B][N][2C] — the input
                                    format of a DS_CONV_F_SPLIT_IN convolution (the Down / Upsample that follows): no ds_split_planes pass */
} ds_attn_x3_params;
int ds_pack_attn_x3(const float* wqkv_384xC, const float* gamma_C, void* wqkv_hl, int C, void* stream);
int ds_attn_x3_context(const ds_attn_x3_params* p, void* stream);
int ds_attn_x3_output(const ds_attn_x3_params* p, void* stream);
int ds_attn_x3_stats_parts(const ds_attn_x3_params* p);
int ds_attn_x3_segments(int B, int N, int C);
size_t ds_attn_x3_qplane_bytes(int B, int N);
size_t ds_attn_x3_mfold_bytes(int B, int C);
/* Limits (tests/test_hip_attn_paths.py): nseg is any count >= 1, as for ds_attn_fused_params — surplus segments are empty and weigh 0 in
 * the combine; a count that is no multiple of 8 leaves the last block's surplus waves without a partial to write.  At C = 192 / 384 the q
 * projection is a launch of its own that cuts the tiles by a count taken from B (one round of blocks), never from batch_hint or nseg: it
 * decides which wave projects which tile and no stored bit, the q planes being per tile.  Form B reads stats_part with the slot count
 * of its own first pass (ds_attn_x3_stats_parts), every slot of which that pass has written. */

/* ---------------------------------------------------------------- diagnostics
 * libdiffusynth_hip_bounds.so (tools/build_variants.py bounds; -DDS_BOUNDS=1) checks every global access of the
 * convolution / depthwise / attention / GroupNorm-apply kernels against the operand extents implied by the parameter
 * structs and records the first violation per translation unit instead of performing it.  Returns the number of
 * records (0 = every access in range) and a description in buf; -1 from the product build. */
int ds_bounds_report(char* buf, int n, int reset);

/* ---------------------------------------------------------------- few-output fp32 3x3 (fp32 / bf16x3 tiers)
 * The U-Net's final_conv = Conv2d(dim, out_dim = 4, 3, padding = 1) (diffusion.py:103-105) on fp32 NHWC tensors: out [B][H][W][4] fp32 =
 * conv3x3(x [B][H][W][C], stride 1, zero padding 1) + bias, outputs beyond Cout zero.  C % 32 == 0, Cout <= 4.  ds_pack_conv3x3_f32_n4 turns
 * the Conv2d-layout weight [Cout][C][3][3] (+ bias or NULL) into ds_conv3x3_f32_n4_weight_floats(C) floats. */
size_t ds_conv3x3_f32_n4_weight_floats(int C);
int ds_pack_conv3x3_f32_n4(const float* w, const float* bias, int Cout, int C, float* dst, void* stream);
int ds_conv3x3_f32_n4(const float* x, int B, int H, int W, int C, const float* wpk, float* out, void* stream);

/* ---------------------------------------------------------------- conditioning MLPs
 * SinusoidalPositionEmbeddings (components:42-56), nn.Linear / GELU stacks (diffusion.py:99-105,
 * components:112-116,155-168,267-268).  y[b][o] = bias[o] + sum_k act_in(x[b][k]) W[o][k], fp32. */
int ds_sinusoid(const int64_t* t, const float* freqs, int B, int half, float* out, void* stream);
int ds_linear(const float* x, int x_stride, const float* W, const float* bias, int B, int K, int O, int act_in,
              float* y, int y_stride, void* stream);
/* y[i] = act(x[i]), fp32, in place allowed (act in {DS_ACT_NONE, DS_ACT_GELU, DS_ACT_SILU}): the activation in front of a wide nn.Linear
 * stack over one small input (the `mlp = Sequential(GELU, Linear)` of all 44 blocks, components:112-116) applied ONCE instead of once per
 * 16 outputs by ds_linear's act_in — the same fp32 function, so the results are identical. */
int ds_activation(const float* x, size_t n, int act, float* y, void* stream);

/* out[b][:] = LayerNorm(a[b][:] + r[b][:]) * gamma + beta over D (biased variance, eps inside the sqrt), fp32:
 * the tail of ProjectionLayer.forward (multimodal_model.py:29-31; SURVEY 8f row 3, text-condition head). */
int ds_add_layernorm(const float* a, const float* r, const float* gamma, const float* beta, int B, int D, float eps,
                     float* out, void* stream);

/* ---------------------------------------------------------------- layout converts at the boundary */
int ds_nchw_to_nhwc(const float* x, int B, int C, int H, int W, void* out, int C_pad, int dtype, void* stream);
/* The VQGAN decoder's first layer on the NCHW latent (VQGAN.py:345, Conv2d(embedding_dim, hidden, 1)): layout change + 1x1 convolution in one
 * pass, fp32 NCHW in, bf16 NHWC [B][HW][Cout] out.  Cin in {4, 8}, Cout % 8 == 0; w = [Cout][Cin] fp32, bias [Cout] or NULL. */
int ds_conv1x1_in_nchw(const float* x_nchw, int B, int Cin, int HW, const float* w, const float* bias, int Cout, void* out, void* stream);
/* dst[0, nbytes) = dst[nbytes, 2 nbytes) = src[0, nbytes): the two halves of a classifier-free-guidance batch (DiffSynthSampler.py:311-320 evaluates
 * model(cat([x, x]), cat([t, t]), cat([uncond, cond]))) are identical up to the first operator that reads the condition — the plan computes
 * that prefix once at half the batch and duplicates its result (engine.py, `paired`).  dst == src: the first half is in place already,
 * only dst[nbytes, 2 nbytes) is written (r05: the plan computes the prefix into the first half of the full-batch tensor).
 * Either src == dst, or [src, src + nbytes) and [dst, dst + 2 nbytes) are disjoint: any other overlap is refused on the host with
 * DS_EINVAL and nothing is launched (the copy would read bytes it has already overwritten).  Any nbytes and alignment: 16-byte aligned
 * pointers with nbytes % 16 == 0 take the vector kernel, everything else two device-to-device copies (one when src == dst). */
int ds_dup_batch(const void* src, void* dst, size_t nbytes, void* stream);
int ds_nhwc_to_nchw(const void* x, int dtype, int B, int C, int C_stride, int H, int W, float* out, void* stream);

/* ---------------------------------------------------------------- sampler step
 * DiffSynthSampler.ddim_sample (DiffSynthSampler.py:311-343): classifier-free-guidance combine,
 * predicted x0, sigma, direction and the update — and, for inpainting, the q_sample + mask blend of
 * p_sample_loop (DiffSynthSampler.py:499-510, 271-294).  fp32 NCHW, reference operation order,
 * no fused multiply-add: bit-exact with the CPU reference given identical inputs.  16-byte accesses when
 * HW % 4 == 0 and x / eps / eps_cond / noise / out are 16-byte aligned (guide / init_noise / mask: per sample,
 * when their addresses allow it), element by element otherwise: the same bits either way. */
typedef struct {
    const float* x; const float* eps; const float* eps_cond; /* eps_cond != NULL => eps is the uncond half */
    const float* noise; float* out;
    const float* coef;           /* [B][5]: sqrt(1-a_t), sqrt(a_t), sqrt(a_prev), sqrt(1-a_prev-sigma^2), sigma */
    float cfg_scale;
    /* inpaint blend (mode 0 none, 1: mask*q_sample(guide)+(1-mask)*x', 2: mask*guide+(1-mask)*x') */
    int32_t blend_mode;
    const float* guide; const float* init_noise; const float* mask; /* mask [B][1][H][W] (mask_chw == 0)  */
    const float* qcoef;          /* [B][2]: sqrt(acp[t-1]), sqrt(1-acp[t-1])                           */
    int32_t B, CHW, HW;
    int32_t mask_chw;            /* != 0: mask is [B][C][H][W] (the reference blends by broadcasting, and its
                                    inpaint UI passes a per-channel mask: inpaint_with_text.py:229-231)    */
} ds_step_params;
int ds_ddim_step(const ds_step_params* p, void* stream);
/* One sampler step over R rows that belong to different requests (diffusynth_amd/batching.py: concurrent sampler calls sharing one
 * U-Net batch).  Row r reads its state from x[irow[r][DS_SR_X]], its eps (the unconditional half under CFG) from eps[irow[r][DS_SR_EPS]]
 * and, when irow[r][DS_SR_EPSC] >= 0, the conditional eps from that row of eps; it writes the new state to out[irow[r][DS_SR_OUT]] and,
 * when irow[r][DS_SR_DUP] >= 0, a second copy to that row (the classifier-free-guidance duplicate of the next U-Net input).  Rows are
 * C*H*W fp32 each.  The arithmetic is ds_ddim_step's (same row loop, no FMA contraction), with the row's own CFG scale,
 * coefficients (frow: coef[5] as ds_step_params.coef, qcoef[2], cfg scale), blend mode and mask layout.
 * Step noise (irow[r][DS_SR_NOISE]): 0 none (sigma == 0), 1 read from a raw draw, 2 computed in the kernel.  For element (c, h, j) of
 * the row, the source index into its request's draw of shape (draw_rows, C, H, draw_w) is
 *     e = ((sample * C + c) * H + h) * draw_w + cols[cols_off + j]
 * mode 1 reads draw[e] (prow DS_SR_DRAW), mode 2 computes lane e % 4 of Philox counter offset + e / 4 under key seed (prow DS_SR_SEED /
 * DS_SR_OFFSET): what ds_philox_normal followed by ds_gather_cols gives.  prow DS_SR_GUIDE / DS_SR_INIT / DS_SR_MASKP address the row's
 * own guide, initial noise and mask (mask: H*W floats, or C*H*W when irow DS_SR_MASK_CHW != 0); with W % 4 == 0 they are read in
 * 16-byte pieces when 16-byte aligned.  The tables are device arrays, row-major [R][DS_SR_NI] int32, [R][DS_SR_NF] float,
 * [R][DS_SR_NP] uint64; Bx / Beps / Bout are the row counts of x / eps / out and n_cols the length of cols.  A row whose entries fall
 * outside those bounds (or name an unknown mode, or lack a pointer its modes need) reads nothing: its output row, and its duplicate
 * when that is in range, is filled with NaN; a row whose output row is out of range writes nothing. */
#define DS_SR_X 0
#define DS_SR_EPS 1
#define DS_SR_EPSC 2
#define DS_SR_OUT 3
#define DS_SR_DUP 4
#define DS_SR_BLEND 5
#define DS_SR_MASK_CHW 6
#define DS_SR_NOISE 7
#define DS_SR_SAMPLE 8
#define DS_SR_DRAW_ROWS 9
#define DS_SR_DRAW_W 10
#define DS_SR_COLS 11
#define DS_SR_NI 12
#define DS_SR_COEF 0                   /* frow: coef[5] at 0..4 */
#define DS_SR_Q0 5
#define DS_SR_Q1 6
#define DS_SR_CFG 7
#define DS_SR_NF 8
#define DS_SR_GUIDE 0                  /* prow */
#define DS_SR_INIT 1
#define DS_SR_MASKP 2
#define DS_SR_DRAW 3
#define DS_SR_SEED 4
#define DS_SR_OFFSET 5
#define DS_SR_NP 6
typedef struct {
    const float* x; const float* eps; float* out;
    const int32_t* irow; const float* frow; const uint64_t* prow;
    const int32_t* cols;
    int32_t R, C, H, W;
    int32_t Bx, Beps, Bout, n_cols;
} ds_step_rows_params;
int ds_step_rows(const ds_step_rows_params* p, void* stream);
/* One step of the "dpmpp_2m" sampler (DPM-Solver++(2M): data prediction, second-order multistep, deterministic).  With the
 * guidance combine and the blend of ds_ddim_step:
 *     x0  = (x - coef[0] * eps') / coef[1]                     (ds_ddim_step's x0: same operations, same two coefficients)
 *     out = (coef[2] * x + coef[3] * x0) + coef[4] * hist      (the last term only where coef[4] != 0: hist is not read otherwise)
 *     out = blend(out);  hist = x0
 * coef [B][5] = sigma_t, alpha_t, c_x, c_0, c_1 (diffusynth_amd/sampler.py builds them in float64).  hist [B][C*H*W] is the x0
 * prediction of the previous step, updated in place (each element is read and written by the same thread); it may be NULL
 * when no row has coef[4] != 0 — a row that needs a history it was not given is filled with NaN.  fp32 NCHW, no fused
 * multiply-add; 16-byte accesses when W % 4 == 0 and x / eps / eps_cond / hist / out are 16-byte aligned. */
typedef struct {
    const float* x; const float* eps; const float* eps_cond; /* eps_cond != NULL => eps is the uncond half */
    float* hist; float* out;
    const float* coef;           /* [B][5] */
    float cfg_scale;
    int32_t blend_mode;          /* as ds_step_params */
    const float* guide; const float* init_noise; const float* mask;
    const float* qcoef;          /* [B][2] */
    int32_t B, C, H, W;
    int32_t mask_chw;
} ds_dpm_step_params;
int ds_dpm_step(const ds_dpm_step_params* p, void* stream);
/* ds_dpm_step over R rows that belong to different requests: ds_step_rows' tables, bounds contract, duplicate write and 16-byte
 * paths, with frow's coef[5] holding the solver's five numbers and irow DS_SR_NOISE == 0 (the solver draws no step noise; any
 * other value makes the row malformed).  hrow [R] holds each row's history address (C*H*W floats, updated in place); 0 is allowed
 * only where the row's coef[4] == 0, anywhere else the row is malformed.  A malformed row reads nothing, writes no history and
 * fills its output row (and its duplicate, when in range) with NaN.  A row is the same bits as ds_dpm_step on the same inputs. */
int ds_dpm_step_rows(const ds_step_rows_params* p, const uint64_t* hrow, void* stream);
/* Guidance rescale of the classifier-free-guidance combine (Lin et al., "Common Diffusion Noise Schedules and Sample Steps are
 * Flawed", section 3.4), per sample (row) of CHW fp32 elements:
 *     e     = eps_u + cfg_scale * (eps_c - eps_u)              (the step kernels' combine: three separately rounded fp32 operations)
 *     ratio = std(eps_c) / std(e)                              (over the row; 1 where std(e) == 0)
 *     g     = phi * ratio + (1 - phi),   out = g * e
 * The step kernels then take `out` as a plain eps (eps_cond NULL / DS_SR_EPSC -1).  phi in [0, 1]; phi == 0 reduces nothing and
 * writes e itself (g == 1).  One block works on a row, in two passes about the mean (float64 sums of the fp32 elements: the row's
 * mean, then the squares of the distances from it): element i belongs to thread (i / 4) % 1024, and the order of every sum
 * depends on CHW only, not on the rows in the launch, on their number or on the addresses.  So a row is the same bits alone, in
 * any batch and in either entry point.  No atomics, no workspace.  eps_u / eps_c / out are [B][CHW]; out may be eps_u (each
 * element is read and written by the same thread).  gain (may be NULL) receives g [B].  A row is moved in 16-byte pieces when
 * CHW % 4 == 0 and its three addresses are 16-byte aligned, element by element otherwise. */
typedef struct {
    const float* eps_u; const float* eps_c; float* out;
    float* gain;
    float cfg_scale, phi;
    int32_t B, CHW;
} ds_cfg_rescale_params;
int ds_cfg_rescale(const ds_cfg_rescale_params* p, void* stream);
/* ds_cfg_rescale over R rows that belong to different requests, inside one eps buffer of Beps rows (the U-Net output of a
 * SamplingBatcher tick).  Row r reads the unconditional eps from eps[irow[r][DS_CR_U]] and the conditional one from
 * eps[irow[r][DS_CR_C]], and writes eps[irow[r][DS_CR_OUT]] (its own unconditional row is allowed, a row that another table row
 * reads is not), with its own scale frow[r][DS_CR_SCALE] and phi frow[r][DS_CR_PHI]; gain (may be NULL) receives g [R].  Rows of eps
 * that the table does not name are not touched.  A row whose input rows fall outside [0, Beps), or whose phi is not in [0, 1],
 * reads nothing: its output row is filled with NaN (and its gain is NaN); a row whose output row is out of range writes no eps.
 * A row is the same bits as ds_cfg_rescale on the same inputs. */
#define DS_CR_U 0
#define DS_CR_C 1
#define DS_CR_OUT 2
#define DS_CR_NI 3
#define DS_CR_SCALE 0                  /* frow */
#define DS_CR_PHI 1
#define DS_CR_NF 2
typedef struct {
    float* eps;
    const int32_t* irow; const float* frow;
    float* gain;
    int32_t R, CHW, Beps;
} ds_cfg_rescale_rows_params;
int ds_cfg_rescale_rows(const ds_cfg_rescale_rows_params* p, void* stream);
/* Weighted multi-prompt guidance: the classifier-free-guidance combine of one unconditional and K conditional predictions, with
 * guidance rescale.  Per sample (one row of N = C*H*W elements, column j = i mod W):
 *     u            the unconditional eps
 *     c_1 ... c_K  the conditional eps, 1 <= K <= DS_CC_MAXK (8)
 *     a_k(j)       the mixture weights: a scalar per condition, or one value per latent column (a time envelope); any finite sign or
 *                  size, the sum is free
 *     S, phi       the CFG scale and the guidance rescale
 *
 *     d_k = c_k - u
 *     acc = a_1(j) d_1 + a_2(j) d_2 + ... + a_K(j) d_K      ascending k
 *     p   = u + acc                                         the mixture's "conditional" prediction
 *     e   = u + S acc
 *     g   = phi std(p) / std(e) + (1 - phi)                 std over the row; std(e) == 0 -> ratio 1; phi == 0 -> g = 1
 *     out = g e
 * Every fp32 operation above is rounded on its own (no contraction into FMA); the products are summed in ascending k, starting from
 * the first product, not from 0; the statistics are ds_cfg_rescale's (float64, two passes about the mean, a summation order that N
 * alone decides: element i belongs to thread (i / 4) % 1024); with phi == 0 the row is multiplied by nothing (not by 1.0f).  So
 * K = 1, a = 1, phi = 0 is ds_cfg_rescale(phi = 0) (the step kernels' combine) bit for bit, two copies of one condition at weights
 * 0.5 / 0.5 are plain CFG's bits for that condition, and an envelope that is 1 on some columns and 0 on the others selects whole
 * columns of the single-prompt results.  The step kernels then take `out` as a plain eps (eps_cond NULL / DS_SR_EPSC -1).
 * eps_u [B][CHW]; eps_c [K][B][CHW], k-major (the chunks behind the first of a U-Net call on [u; c_1; ...; c_K]); wt [K][wt_w]
 * device floats with wt_w in {1, W}: 1 = scalar weights (no column lookup), W = one weight per column (then W <= DS_CC_MAXW: the
 * block keeps the row's table in LDS); out [B][CHW], out == eps_u is allowed (each element is read and written by the same
 * thread); gain (may be NULL) receives g [B].  CHW % W == 0, phi in [0, 1].  One block per row; a row is moved in 16-byte pieces
 * when W % 4 == 0 (a piece then never crosses an image row) and u, every c_k and out are 16-byte aligned, element by element
 * otherwise, and either way a row is the same bits alone, in any batch, at any address and in either entry point. */
#define DS_CC_MAXK 8
#define DS_CC_MAXW 256
typedef struct {
    const float* eps_u; const float* eps_c; const float* wt; float* out;
    float* gain;
    float cfg_scale, phi;
    int32_t B, K, CHW, W, wt_w;
} ds_cfg_compose_params;
int ds_cfg_compose(const ds_cfg_compose_params* p, void* stream);
/* ds_cfg_compose over R rows that belong to different requests, inside one eps buffer of Beps rows (the U-Net output of a
 * SamplingBatcher tick).  Row r reads u from eps[irow[r][DS_CC_U]] and c_k (k = 1 ... irow[r][DS_CC_K]) from
 * eps[irow[r][DS_CC_C0] + (k - 1) * irow[r][DS_CC_CSTRIDE]], takes its weight table [K][irow[r][DS_CC_WTW]] at
 * wt + irow[r][DS_CC_WT] (wt holds n_wt floats) and writes eps[irow[r][DS_CC_OUT]] (its own unconditional row is allowed, a row
 * that another table row reads is not), with its own scale frow[r][DS_CC_SCALE] and phi frow[r][DS_CC_PHI]; gain (may be NULL)
 * receives g [R].  Rows of eps that the table does not name are not touched.  A row that names an eps row outside [0, Beps), a K
 * outside [1, DS_CC_MAXK], a weight table that does not fit n_wt, a DS_CC_WTW that is neither 1 nor W (or is W > DS_CC_MAXW) or a
 * phi outside [0, 1] reads nothing: its output row is filled with NaN (and its gain is NaN); a row whose output row is out of
 * range writes no eps.  A row is the same bits as ds_cfg_compose on the same inputs. */
#define DS_CC_U 0
#define DS_CC_OUT 1
#define DS_CC_K 2
#define DS_CC_C0 3                     /* the row of c_1 */
#define DS_CC_CSTRIDE 4                /* the row distance from c_k to c_{k+1} */
#define DS_CC_WT 5                     /* the offset of the row's weight table in wt */
#define DS_CC_WTW 6                    /* 1 or W */
#define DS_CC_NI 7
#define DS_CC_SCALE 0                  /* frow */
#define DS_CC_PHI 1
#define DS_CC_NF 2
typedef struct {
    float* eps;
    const int32_t* irow; const float* frow; const float* wt;
    float* gain;
    int32_t R, CHW, W, Beps, n_wt;
} ds_cfg_compose_rows_params;
int ds_cfg_compose_rows(const ds_cfg_compose_rows_params* p, void* stream);
/* buf[pairs[r][1]] = buf[pairs[r][0]] for R (src, dst) pairs of device int32, rows of CHW floats inside buf [Bbuf][CHW] (the further
 * copies of a multi-prompt request's state row in the next U-Net input).  A pair with a row outside [0, Bbuf), or with src == dst,
 * is skipped.  No dst may be another pair's src: the pairs are copied in no particular order. */
int ds_copy_rows(float* buf, const int32_t* pairs, int R, int CHW, int Bbuf, void* stream);
/* q_sample (DiffSynthSampler.py:271-294) over R rows with a coefficient pair each: the noisy states of a DDPM inversion
 * (diffusynth_amd/sampler.py: edit_invert), one launch for rows at different timesteps.  Row r writes
 *     out[irow[r][DS_QS_OUT]] = q0 * x0[irow[r][DS_QS_SRC]] + q1 * noise          (two products, one sum: no FMA contraction)
 * and, when irow[r][DS_QS_DUP] >= 0, a second copy to that row of out.  The noise is the step noise of ds_step_rows: element
 * (c, h, j) is element e = ((sample * C + c) * H + h) * draw_w + cols[cols_off + j] of the row's raw draw of shape
 * (draw_rows, C, H, draw_w) (irow DS_QS_NOISE == 1, prow DS_QS_DRAW) or of the Philox stream (seed, offset) (DS_QS_NOISE == 2, prow
 * DS_QS_SEED / DS_QS_OFFSET), so a row is the bits of q_sample on the tensor get_deterministic_noise_tensor returns.  Rows are C*H*W
 * fp32; x0 has Bx0 rows, out Bout, cols n_cols entries.  16-byte pieces when W % 4 == 0 and x0 / out are 16-byte aligned.  A row
 * whose entries fall outside those bounds (or name another noise mode, or lack the draw) reads nothing: its output row, and its
 * duplicate when that is in range, is filled with NaN; a row whose output row is out of range writes nothing. */
#define DS_QS_SRC 0
#define DS_QS_OUT 1
#define DS_QS_DUP 2
#define DS_QS_NOISE 3
#define DS_QS_SAMPLE 4
#define DS_QS_DRAW_ROWS 5
#define DS_QS_DRAW_W 6
#define DS_QS_COLS 7
#define DS_QS_NI 8
#define DS_QS_Q0 0                     /* frow: sqrt(acp[i]), sqrt(1 - acp[i]) */
#define DS_QS_Q1 1
#define DS_QS_NF 2
#define DS_QS_DRAW 0                   /* prow */
#define DS_QS_SEED 1
#define DS_QS_OFFSET 2
#define DS_QS_NP 3
typedef struct {
    const float* x0; float* out;
    const int32_t* irow; const float* frow; const uint64_t* prow;
    const int32_t* cols;
    int32_t R, C, H, W;
    int32_t Bx0, Bout, n_cols;
} ds_q_sample_rows_params;
int ds_q_sample_rows(const ds_q_sample_rows_params* p, void* stream);
/* The step noise of "edit-friendly" DDPM inversion (Huberman-Spiegelglas et al., 2024): the z for which the eta = 1 step of
 * ds_ddim_step goes from x to x_prev.  Row r, with coef[5] = frow[r][DS_EN_COEF ...] as ds_step_params.coef and the step kernels'
 * guidance combine (eps_c read only when irow[r][DS_EN_EPSC] >= 0, with the scale frow[r][DS_EN_CFG]):
 *     e  = guided eps of eps[irow[r][DS_EN_EPS]]                x^ = (x - coef[0] e) / coef[1]        x = X[irow[r][DS_EN_X]]
 *     u0 = coef[2] x^     u1 = coef[3] e     mu = u0 + u1       d = x_prev - mu                       z = d / coef[4]
 * every operation rounded on its own, written to z[irow[r][DS_EN_OUT]].  x_prev is X[irow[r][DS_EN_PREV]] or, when that is < 0, the
 * C*H*W floats at the address prow[r][DS_EN_PREVP] (any 4-byte alignment: such a row is read element by element).  A row with
 * coef[4] == 0 (the step to the clean sample) is zeros and reads nothing but its table.  X / eps / z have Bx / Beps / Bz rows of
 * C*H*W fp32; 16-byte pieces when W % 4 == 0 and X / eps / z are 16-byte aligned.  A row that points outside those bounds, or has
 * neither a row nor an address for x_prev, reads nothing and is filled with NaN; a row whose output row is out of range writes
 * nothing. */
#define DS_EN_X 0
#define DS_EN_PREV 1
#define DS_EN_EPS 2
#define DS_EN_EPSC 3
#define DS_EN_OUT 4
#define DS_EN_NI 5
#define DS_EN_COEF 0                   /* frow: coef[5] at 0..4 */
#define DS_EN_CFG 5
#define DS_EN_NF 6
#define DS_EN_PREVP 0                  /* prow */
#define DS_EN_NP 1
typedef struct {
    const float* X; const float* eps; float* z;
    const int32_t* irow; const float* frow; const uint64_t* prow;
    int32_t R, C, H, W;
    int32_t Bx, Beps, Bz;
} ds_edit_noise_rows_params;
int ds_edit_noise_rows(const ds_edit_noise_rows_params* p, void* stream);
/* Windowed sampling (MultiDiffusion; diffusynth_amd/windowed.py): the windows of a wide latent as one batch of rows of
 * the trained width.  Row i of the table rows[R][DS_WS_NI] copies, for c in [0, w),
 *     out[rows[i][DS_WS_DST]][:, :, c] = x[rows[i][DS_WS_SRC]][:, :, (rows[i][DS_WS_OFF] + c) mod W]
 * x: [Bx][C][H][W] fp32, out: [Bout][C][H][w] fp32, w <= W; the destination row is the caller's to choose (paired halves, chunks).  A
 * pure copy: the bits of the source.  16-byte pieces when W % 4 == 0, w % 4 == 0 and x / out are 16-byte aligned, for the rows whose
 * offset is a multiple of 4 (the others go element by element).  A row whose source row or offset ([0, W)) is out of range reads
 * nothing: its destination row is filled with NaN; a row whose destination row is out of range writes nothing. */
#define DS_WS_SRC 0
#define DS_WS_OFF 1
#define DS_WS_DST 2
#define DS_WS_NI 3
typedef struct {
    const float* x; float* out;
    const int32_t* rows;
    int32_t R, C, H, W, w;
    int32_t Bx, Bout;
} ds_window_split_params;
int ds_window_split(const ds_window_split_params* p, void* stream);
/* The blend of the windows' predictions with a partition of unity.  Output row r in [0, R) of out [Bout][C][H][W] is
 *     out[r][:, :, x] = sum_m wcoef[m][x] * eps[erow[r * n + j]][:, :, c]        j = wcol[m][x][DS_WM_WIN], c = wcol[m][x][DS_WM_COL]
 * over the entries m = 0, 1, ... of column x up to the first with j < 0 (at most DS_WM_MAXM; ascending in j, the rest padded with
 * j = -1): every product is rounded on its own, the first one starts the sum and the others are added in table order (no FMA
 * contraction), so a coefficient of 1.0 returns the window's bits.  eps: [Beps][C][H][w] fp32; erow [R][n]: the eps row of window j of
 * output row r; wcol [DS_WM_MAXM][W][DS_WM_NI] int32 and wcoef [DS_WM_MAXM][W] fp32 belong to the call, not to a row.  Only the eps
 * rows and columns the tables name are read.  16-byte pieces when W % 4 == 0, w % 4 == 0 and eps / out / wcol / wcoef are 16-byte
 * aligned, for the pieces whose four columns name the same windows at four adjacent source columns from a multiple of 4 on (so it
 * is when every window offset is a multiple of 4); the others go element by element.  A row with an erow entry outside [0, Beps)
 * reads nothing and is filled with NaN; a column entry with j >= n or c outside [0, w) makes that column NaN; rows of out from R on
 * are not written. */
#define DS_WM_MAXM 8
#define DS_WM_WIN 0
#define DS_WM_COL 1
#define DS_WM_NI 2
typedef struct {
    const float* eps; float* out;
    const int32_t* erow; const int32_t* wcol; const float* wcoef;
    int32_t R, n, C, H, W, w;
    int32_t Beps, Bout;
} ds_window_merge_params;
int ds_window_merge(const ds_window_merge_params* p, void* stream);
/* Windowed decoding (diffusynth_amd/windowed.py WindowedDecoder): the blend of decoded windows, which are STFT+
 * representations (log1p|D|, cos, sin) and so no linear space, on the complex spectrum.  encw: [Bw][3][F][w] fp32, out: [Bout][3][F][T]
 * fp32; erow [R][n], wcol [DS_WM_MAXM][T][DS_WM_NI] and wcoef [DS_WM_MAXM][T] are ds_window_merge's tables, in frames.  Per output
 * row r, bin k and frame x:
 *   one entry:      the three values of that window frame, bit for bit (its coefficient is 1.0 in a plan);
 *   two or more:    every entry is decoded as ds_istft_plus decodes (magnitude expm1, the (cos, sin) pair normalised — it need not be
 *                   of unit length —, phase 0 for a (0, 0) or non-finite pair), z = sum_m wcoef[m][x] * (re_m, im_m) by
 *                   ds_window_merge's rule (every product rounded on its own, the first starts the sum, the others are added in
 *                   table order: two windows commute), and out = (log1p|z|, z / |z|), (0, 1, 0) where z is 0 as from ds_stft_plus.
 * 16-byte pieces when T % 4 == 0, w % 4 == 0 and encw / out / wcol / wcoef are 16-byte aligned, for the pieces whose four frames
 * name the same windows at four adjacent frames from a multiple of 4 on (so it is for a frame plan made of a latent plan); the
 * others go element by element.  A row with an erow entry outside [0, Bw) reads nothing and is filled with NaN; an entry with j >= n or
 * c outside [0, w) makes that frame NaN in all three channels; rows of out from R on are not written. */
typedef struct {
    const float* encw; float* out;
    const int32_t* erow; const int32_t* wcol; const float* wcoef;
    int32_t R, n, F, T, w;
    int32_t Bw, Bout;
} ds_stft_window_merge_params;
int ds_stft_window_merge(const ds_stft_window_merge_params* p, void* stream);
/* counter-based N(0,1) generator (Philox4x32-10 + Box-Muller) for the throughput mode */
int ds_philox_normal(float* out, size_t n, uint64_t seed, uint64_t offset, void* stream);
/* column gather of the "repeat" noise layout (DiffSynthSampler.py:97-167): out[b][c][h][j] = src[b][c][h][cols[j]] */
int ds_gather_cols(const float* src, int rows, int src_w, const int32_t* cols, int out_w, float* out, void* stream);

/* ---------------------------------------------------------------- VQ + vocoder tail
 * VectorQuantizerEMA.forward eval (VQGAN.py:98-146): nearest code (first minimum, as torch.argmin); writes quantised NCHW fp32 (the
 * straight-through form z + (e - z)) and int64 indices.  Up to 8192 codes of dimension 4 run on the matrix cores: |e|^2 - 2 z.e in split
 * precision (three bf16 parts per fp32 number) — the codebook is re-packed into a per-device module buffer on every call, so concurrent calls
 * on different streams of one device must not overlap; larger codebooks take the scalar kernel with the reference's
 * |z|^2 + |e|^2 - 2 z.e expression. */
int ds_vq_nearest(const float* z_nchw, const float* codebook, const float* code_sqnorm, int B, int D, int HW,
                  int ncodes, float* q_nchw, int64_t* idx, void* stream);
/* The quantiser's scalars from its outputs (VQGAN.py:62-73 / :131-144): out3[0] = mean((q - z)^2), out3[1] = perplexity =
 * exp(-sum_j p_j log(p_j + 1e-10)) (p = usage frequencies of the codes), out3[2] = the module's loss: commitment_cost * out3[0] (ema != 0:
 * VectorQuantizerEMA) or out3[0] + commitment_cost * out3[0] (VectorQuantizer), the product and the sum each rounded to fp32 on its own as
 * the module's two torch ops are.  Indices outside [0, ncodes) count for no code.  ws: ds_vq_stats_ws_bytes. */
size_t ds_vq_stats_ws_bytes(int ncodes);
int ds_vq_stats(const float* z_nchw, const float* q_nchw, const int64_t* idx, int B, int D, int HW, int ncodes, float commitment_cost, int ema,
                float* out3, void* ws, void* stream);
/* Decoder tail activations (VQGAN.py:394-398): softplus / tanh / tanh on NHWC[.,C_stride] -> NCHW fp32 [B][3][H][W] */
int ds_decoder_tail(const void* x, int dtype, int B, int C_stride, int HW, float* out, void* stream);
/* The body of the VQGAN decoder's 80-channel ResnetBlock as one kernel (csrc/conv3x3_c80.hip; VQGAN.py:223-244 with temb = None, no
 * nin_shortcut): out = [x +] conv3x3(act(GroupNorm(G, 80)(x))) + bias, bf16 NHWC.  wpk = ds_conv3x3_c80_weight_elems() bf16 written by
 * ds_pack_conv3x3_c80 from the fp32 [80][80][3][3] Conv2d weight; gn_ab [B][G][2] (rstd, rstd * mean) with gamma / beta [80] and
 * act in {DS_ACT_NONE, DS_ACT_RELU, DS_ACT_SILU}: applied to x on load (NULL: the convolution reads x as it is); add_x: add the raw x
 * (the block's residual).  out must not alias x.  A sample must stay below 256 MB. */
size_t ds_conv3x3_c80_weight_elems(void);
int ds_pack_conv3x3_c80(const float* w, int Cout, int Cin, void* dst, void* stream);
int ds_conv3x3_c80(const void* x, int B, int H, int W, const void* wpk, const float* bias, void* out, const float* gn_ab, int G,
                   const float* gamma, const float* beta, int act, int add_x, float* stats_ws, void* stream);
/* stats_ws (both 80-channel kernels; NULL: none): [B][slots][80][2] floats, slots = ds_*_c80_stats_slots(B, H, W) — per-channel (sum, sum of
 * squares) partials of the OUTPUT, every slot written; ds_gn_stats_finish(stats_ws, B, slots, 80, G, output pixels per sample, eps, ab) turns
 * them into the (rstd, rstd * mean) pairs of GroupNorm(G, 80) of that output: the next Normalize needs no pass over the tensor. */
int ds_conv3x3_c80_stats_slots(int B, int H, int W);
/* The same block as two launches: h = act(GroupNorm(res)) written by ds_gn_apply, then out = res + conv3x3(h) + bias (no arithmetic while the halo
 * is staged: 377 us against 637 us at 64 x 256 x 128 x 80, + ~110 us for the apply pass). */
int ds_conv3x3_c80_res(const void* h, const void* res, int B, int H, int W, const void* wpk, const float* bias, void* out, float* stats_ws,
                       void* stream);
int ds_convt4x4_c80_stats_slots(int B, int H, int W, int Cin);
/* second stage of ds_gn_stats_stream on its own: ws [B][nblk][C][2] per-channel partial sums -> ab [B][G][2] */
int ds_gn_stats_finish(const float* ws, int B, int nblk, int C, int G, int HW, float eps, float* ab, void* stream);

/* ConvTranspose2d(Cin, 80, 4, 2, 1) with Cin = 80 or 160, bf16 NHWC in / out, on its own kernel (csrc/convt4x4_c80.hip): the VQGAN decoder's
 * two Upsample layers (VQGAN.py Decoder `up` layers, SURVEY §8a tail row).  x [B][H][W][Cin]; wpk = ds_convt4x4_c80_weight_elems(Cin) bf16
 * written by ds_pack_convt4x4_c80 from the fp32 [Cin][80][4][4] weight (ConvTranspose2d layout [Cin][Cout][kh][kw]); bias [80] or NULL;
 * out [B][2H][2W][80] bf16.  gn_ab [B][G][2] (rstd, rstd * mean per group, e.g. from ds_gn_stats_stream) with gamma / beta [Cin]: the
 * layer reads relu(GroupNorm(G, Cin)(x)) instead of x (the decoder's Normalize + ReLU), applied on load; NULL: plain x.
 * stats_ws: see ds_conv3x3_c80.  A sample must stay below 256 MB. */
size_t ds_convt4x4_c80_weight_elems(int Cin);
int ds_pack_convt4x4_c80(const float* w, int Cin, int Cout, void* dst, void* stream);
int ds_convt4x4_c80(const void* x, int B, int H, int W, int Cin, const void* wpk, const float* bias, void* out, const float* gn_ab, int G,
                    const float* gamma, const float* beta, float* stats_ws, void* stream);

/* The U-Net's 7x7 init convolution (<= 4 real input channels -> 96, stride 1, pad 3; bf16 NHWC in / out) on its own kernel
 * (csrc/conv7x7_c4.hip).  Replaces: ConditionedUnet.init_conv = nn.Conv2d(channels, init_dim, 7, padding=3), model/DiffSynth.py
 * (SURVEY §8a row "init_conv").  x [B][H][W][Cx] with Cx = 8 (the engine's padded input image; channels 4..7 ignored) or 4;
 * wpk = ds_conv7x7_c4_weight_elems() bf16 written by ds_pack_conv7x7_c4 from the fp32 [96][Cin][7][7] weight; bias [96] or NULL;
 * out [B][H][W][96] bf16.  A sample must stay below 256 MB. */
size_t ds_conv7x7_c4_weight_elems(void);
int ds_pack_conv7x7_c4(const float* w, int Cout, int Cin, void* dst, void* stream);
int ds_conv7x7_c4(const void* x, int B, int H, int W, int Cx, const void* wpk, const float* bias, void* out, void* stream);
/* The same convolution in split precision for the bf16x3 tier: x [B][H][W][4] FP32, out [B][H][W][96] FP32 = x_hi w_hi + x_lo w_hi + x_hi w_lo
 * on bf16 MFMAs with fp32 accumulation (x split on its way to LDS); wpk = 2 x ds_conv7x7_c4_weight_elems() bf16 (hi fragments, then lo)
 * written by ds_pack_conv7x7_c4_x3. */
int ds_pack_conv7x7_c4_x3(const float* w, int Cout, int Cin, void* dst, void* stream);
int ds_conv7x7_c4_x3(const float* x, int B, int H, int W, const void* wpk, const float* bias, float* out, void* stream);

/* The decoder's last ResnetBlock(C -> 3) and the output activations in one pass over its input (VQGAN.py:177-244,390-398), bf16:
 * out[b] = [softplus, tanh, tanh](conv3x3(swish(GroupNorm(G, C)(x))) + nin_shortcut_1x1(x)).  x [B][H][W][C] bf16 (C % 8 == 0, C <= 96, W > 8),
 * gn_ab [B][G][2] = (rstd, rstd * mean) of x (ds_gn_stats / ds_gn_stats_stream), gamma / beta [C], w3 = the 3x3 weight packed by
 * ds_pack_conv_weight with cin_pad 96, cout_pad 16, k_order 1 (bf16), b3 [3], wnin [3][C] fp32, bnin [3]; out [B][3][H][W] fp32. */
int ds_dec_final(const void* x, int B, int H, int W, int C, const float* gn_ab, int G, const float* gamma, const float* beta,
                 const void* w3, const float* b3, const float* wnin, const float* bnin, float* out, void* stream);
/* ISTFT+ and iSTFT (tools.py:334-345,185-191; librosa.istft(D, hop_length=256, win_length=1024) at
 * webUI/natural_language_guided_4/utils.py:241): enc [B][3][F][T] fp32 -> audio [B][hop*(T-1)] fp32.
 * n_fft = 2*F, window = periodic Hann(n_fft), center=True. */
int ds_istft_plus(const float* enc, int B, int F, int T, int hop, float* frames_ws, float* audio, void* stream);
size_t ds_istft_ws_floats(int B, int F, int T);
/* One period of a loop: the T frames lie on a circle of hop*T samples (frame 0 follows frame T-1), audio [B][hop*T].  Sample s sums the
 * n_fft/hop frames that reach it in order of the position inside the frame, n = ((s + n_fft/2) mod hop) + k*hop, and is divided by the
 * sum of the squared window over the same positions: rolling enc by d frames rolls audio by d*hop samples bit for bit.  T >= n_fft/hop
 * (no frame overlaps itself); workspace as for ds_istft_plus. */
int ds_istft_plus_loop(const float* enc, int B, int F, int T, int hop, float* frames_ws, float* audio, void* stream);
/* Audio -> STFT+ representation: librosa.stft(y, n_fft=1024, hop_length=hop, win_length=1024)
 * (call sites load_presets.py:68, sound2sound_with_text.py:85, inpaint_with_text.py:97) + tools.pad_STFT
 * (tools.py:170-182: drop the DC row, zero-pad time to T_out) + tools.encode_stft (tools.py:320-331), fused:
 * audio [B][L] fp32 -> enc [B][3][512][T_out] fp32, T_out >= 1 + L/hop.  reflect_pad: 0 = zero padding of the
 * centred frames (librosa >= 0.10 default), 1 = reflect (older librosa).  The (cos, sin) pair of a bin is of unit length to 6 x 2^-24
 * whatever the bin's magnitude (1e-30 as well as 1e30: the pair is scaled by a power of two before it is squared); a bin of exactly 0
 * and every column past the signal's frames is (0, 1, 0). */
int ds_stft_plus(const float* audio, int B, int L, int hop, int reflect_pad, int T_out, float* enc, void* stream);
/* The spectrogram and phase images the reference's UI shows for an STFT+ tensor (csrc/ui_images.hip; per clip tools.decode_stft +
 * tools.depad_STFT + np.abs / np.angle + spectrogram_to_Gradio_image / phase_to_Gradio_image: webUI/natural_language_guided_4/utils.py:8-86
 * as called at utils.py:172-181, 229-238 and 249-259; tools.np_power_to_db: tools.py:41-50).  enc [B][3][F][T] fp32 -> spec_img, phase_img
 * [B][F+1][T][3] uint8, row 0 = the highest bin, the last row = the implied zero bin.  amp (or NULL): a second source of the log-magnitude
 * channel, clip b at amp + b * amp_batch_stride floats ([F][T] each; the "with original amplitude" variant reads channel 0 of the original
 * batch in place).  Out-of-range phase bytes are the low byte of the int32 value (the reference's cast wraps on x86).  Pointers need
 * 4-byte alignment only; 16-byte aligned tensors with T % 4 == 0 take the 16-byte path.  ws: ds_stft_images_ws_floats floats. */
size_t ds_stft_images_ws_floats(int B, int F, int T);
int ds_stft_images(const float* enc, const float* amp, long long amp_batch_stride, int B, int F, int T, float* ws, unsigned char* spec_img,
                   unsigned char* phase_img, void* stream);
/* The latent image (latent_representation_to_Gradio_image, webUI/natural_language_guided_4/utils.py:89-128) without its 8 x 8 enlargement:
 * lat [B][C][H][W] fp32 (C must be 4) -> img [B][H][W][4] uint8 = trunc((x - min) / (max - min) * 255) per (sample, channel) in fp32,
 * channels last, flipped vertically; a constant channel renders 0.  lat is not written.  The enlargement is a repeat of bytes and is left
 * to the caller, after the copy to the host.  ws: ds_latent_image_ws_floats floats. */
size_t ds_latent_image_ws_floats(int B, int C);
int ds_latent_image(const float* lat, int B, int C, int H, int W, float* ws, unsigned char* img, void* stream);

/* ---------------------------------------------------------------- arranger audio stage (csrc/arranger.hip)
 * What webUI/natural_language_guided_4/track_maker.py does on the host per note event: peak normalisation (:142), chained
 * librosa.effects.pitch_shift(y, sr, n_steps, n_fft=4096, hop_length=1024) calls (:12-47) and the mix into the track (:147).  One
 * pitch_shift = ds_pv_stft -> ds_pv_vocode -> ds_pv_istft -> ds_resample_sinc, each batched over n_signals signals of different lengths.
 * A signal is row s of tab, a device array [n_signals][DS_PV_NI] int32 (offsets and counts in ELEMENTS of the concatenated buffers):
 *   XOFF, LEN    its samples in x (ds_pv_stft, ds_peak_normalize) and in out (ds_resample_sinc, ds_peak_normalize: fix_length to LEN)
 *   FOFF, NF     its analysis frames in spec [total_frames][2049][2]; NF = 1 + LEN / 1024 (centred, zero padded, periodic Hann 4096)
 *   TOFF, NOUT   its synthesis frames in voc [total_out][2049][2], in the frame workspace and in step_idx / step_alpha:
 *                NOUT = len(arange(0, NF, rate)), step_idx = floor(step), step_alpha = step mod 1, both computed in float64
 *   SOFF, SLEN   its stretched samples in y; SLEN = round(LEN / rate)
 *   NRES         ceil(SLEN * rate): output samples from NRES on are zero
 * Whatever is floored or rounded is the host's, in float64.  A row that does not fit the stated totals reads and writes nothing.
 * No atomics: results are bit-reproducible and do not depend on what else is in the batch.
 * ds_pv_vocode keeps the phase as a running product of unit phasors u(R) conj(u(L)) (u(0) = 1), which is librosa's accumulator
 * phi + wrap(angle R - angle L - phi) modulo 2 pi.  ds_pv_istft: window-sum-square normalisation where it exceeds FLT_MIN, zeros where no
 * frame reaches; ws = ds_pv_istft_ws_bytes(total_out) bytes.
 * ds_resample_sinc (rates: device array of n_signals doubles) is this library's definition, not librosa's soxr_hq: output sample m
 * sits at input position m / rates[s]; kernel h(t) = fc sinc(fc t) kaiser(t fc / Z; beta), fc = DS_RS_FC min(1, rate), Z = DS_RS_ZEROS zero
 * crossings each side, beta = DS_RS_BETA; samples outside the stretched signal are zero. */
#define DS_PV_XOFF 0
#define DS_PV_LEN 1
#define DS_PV_FOFF 2
#define DS_PV_NF 3
#define DS_PV_TOFF 4
#define DS_PV_NOUT 5
#define DS_PV_SOFF 6
#define DS_PV_SLEN 7
#define DS_PV_NRES 8
#define DS_PV_NI 9
#define DS_RS_FC 0.95
#define DS_RS_ZEROS 32.0
#define DS_RS_BETA 12.0
int ds_pv_stft(const float* x, const int32_t* tab, int n_signals, int max_frames, long long total_samples, long long total_frames, float* spec,
               void* stream);
int ds_pv_vocode(const float* spec, const int32_t* tab, const int32_t* step_idx, const float* step_alpha, int n_signals, long long total_frames,
                 long long total_out, float* voc, void* stream);
/* Formant correction (opt-in, between ds_pv_vocode and ds_pv_istft; in place on voc): a shift followed by the resampler moves the content of
 * bin k to k / rate and the spectral envelope with it; this gives bin k beforehand the source's envelope AT k / rate, so the envelope stays
 * where it was.  Per synthesis frame V[k], k = 0 .. 2048, of row s, with order[s] (quefrency samples) and warp[s] = fl32(1 / rate):
 *   L[k]  = ln(max(|V[k]|, 1e-6))                          extended evenly to 4096 points
 *   c     = FFT4096(L) / 4096                              the real cepstrum
 *   c'[n] = c[n] where min(n, 4096 - n) <= order, else 0   rectangular lifter
 *   S     = inverse FFT4096 of c' (unnormalised)           the smoothed log envelope
 *   q     = min(fl32(k) * warp, 2048)                      ONE fp32 product
 *   Sq    = (1 - f) S[i] + f S[i + 1],  i = min(floor(q), 2047),  f = q - i
 *   d     = clamp(Sq - S[k], -limit, +limit)               limit = max_gain_db ln 10 / 20, 0 < max_gain_db <= DS_PV_GAIN_DB_MAX
 *   V'[k] = V[k] exp(d)
 * in fp32 with logf / expf, |V| by the scaled form ds_pv_vocode uses.  A row with warp == 1 has d == 0: its frames keep their bits.
 * order, warp: device arrays of n_signals entries.  Grid (ceil(max_out / 2), n_signals): a block takes two consecutive frames of one signal
 * through ONE transform pair (L_t in the real part, L_{t+1} in the imaginary part: both are real and even, so are their transforms).
 * A row whose (TOFF, NOUT) does not fit total_out reads (beyond its table row) and writes nothing; a row whose order is outside
 * [1, DS_PV_ORDER_MAX] reads that order and nothing else, and writes nothing.  No atomics, no workspace; a frame's result depends on nothing
 * outside the frame. */
#define DS_PV_ORDER_MAX 512
#define DS_PV_GAIN_DB_MAX 60
int ds_pv_formant(float* voc, const int32_t* tab, const int32_t* order, const float* warp, float limit, int n_signals, int max_out,
                  long long total_out, void* stream);
size_t ds_pv_istft_ws_bytes(long long total_out);
int ds_pv_istft(const float* voc, const int32_t* tab, int n_signals, int max_out, int max_stretched, long long total_out, long long total_stretched,
                float* ws, float* y, void* stream);
int ds_resample_sinc(const float* ys, const int32_t* tab, const double* rates, int n_signals, int max_len, long long total_stretched,
                     long long total_samples, float* out, void* stream);
/* out = x / max|x| per signal (IEEE division; rows XOFF, LEN of tab).  ws: ds_peak_normalize_ws_bytes bytes. */
size_t ds_peak_normalize_ws_bytes(int n_signals, int max_len);
int ds_peak_normalize(const float* x, const int32_t* tab, int n_signals, int max_len, long long total_samples, float* ws, float* out, void* stream);
/* track[s] = sum, in event order, of the notes that cover s (every sample of track is written).  ev [n_events][3] int32: start sample in the
 * track, offset of the note in notes, length.  Block b owns samples [b DS_MIX_BLOCK, (b + 1) DS_MIX_BLOCK) and walks
 * blk_ev[blk_ptr[b] .. blk_ptr[b + 1]): the ascending indices of the events that touch them (blk_ptr has ceil(track_len / DS_MIX_BLOCK) + 1
 * entries).  fp32 additions in that order: what numpy's `float32 += float64` gives for fp32-valued notes. */
#define DS_MIX_BLOCK 1024
int ds_mix_notes(const float* notes, long long total_samples, const int32_t* ev, int n_events, const int32_t* blk_ptr, const int32_t* blk_ev,
                 int n_blk_ev, float* track, int track_len, void* stream);
/* The shaped mix: track[s] = sum, in event order, of fl(w x) with x = the event's note sample j = s - START and w = fl(GAIN env(j)), one fp32
 * weight per sample (the product is formed in fp64 from the fp32 row entries and rounded once); fl(w x) and the running sum are fp32
 * roundings.  ev [n_events][DS_MX_NI] 32-bit words, the first three as ds_mix_notes' (DS_MX_NI_PLAIN), then four int32 segment lengths and
 * five fp32 values.  env is an ADSR envelope in closed form:
 *   attack   j in [0, NA)               linspace(0, 1, NA)[j]             = 0 + j STEP_A
 *   decay    the next ND samples        linspace(1, SUSTAIN, ND)[k]       = 1 + k STEP_D
 *   sustain  the next NS samples        SUSTAIN
 *   release  the next NR samples        linspace(SUSTAIN, 0, NR)[k]       = SUSTAIN + k STEP_R
 *   after                               0
 * linspace is numpy's: start + k step with step = (stop - start) / (n - 1), the last element exactly stop when n > 1, the single element
 * start when n = 1.  The steps (0 for n <= 1) and GAIN are the host's, computed in float64 and rounded to fp32.  LEN is the MIXED length
 * min(note length, NA + ND + NS + NR): the host builds blk_ptr / blk_ev from it, so a block that only a note's silent remainder would touch
 * does not walk the event.  A row with a negative segment length, whose note range [OFF, OFF + LEN) does not fit total_samples or whose
 * track range [START, START + LEN) does not fit track_len reads and writes nothing.
 * Block ownership, event order, no atomics and the same bits whatever else is in the launch: as ds_mix_notes. */
#define DS_MX_START 0
#define DS_MX_OFF 1
#define DS_MX_LEN 2
#define DS_MX_NI_PLAIN 3
#define DS_MX_NA 3
#define DS_MX_ND 4
#define DS_MX_NS 5
#define DS_MX_NR 6
#define DS_MX_GAIN 7
#define DS_MX_SUSTAIN 8
#define DS_MX_STEP_A 9
#define DS_MX_STEP_D 10
#define DS_MX_STEP_R 11
#define DS_MX_NI 12
int ds_mix_notes_shaped(const float* notes, long long total_samples, const int32_t* ev, int n_events, const int32_t* blk_ptr,
                        const int32_t* blk_ev, int n_blk_ev, float* track, int track_len, void* stream);

/* ---------------------------------------------------------------- pitch detection (csrc/pitch.hip): YIN (de Cheveigne & Kawahara 2002), fp32
 * ds_yin_frames: period and aperiodicity of every frame of a ragged batch.  A signal is row s of tab, a device array
 * [n_signals][DS_YIN_NI] int32: XOFF, LEN its samples in x; FOFF, NF its frames in period / aperiodicity, NF = max(0, (LEN - W - tau_max) / hop
 * + 1) computed by the host in integers (W = frame_length); frame i reads samples [i hop, i hop + W + tau_max).  A signal of zero frames is
 * legal; a row or a frame that does not fit its extents or the stated totals reads and writes nothing.  Per frame:
 *   d(tau) = sum_{j < W} (s[j] - s[j + tau])^2, tau = 0 .. tau_max, as differences (four interleaved accumulators j mod 4 walked in j
 *            order, summed as (a0 + a1) + (a2 + a3): a fixed order);
 *   c(0) = 1, c(tau) = d(tau) tau / sum_{k = 1 .. tau} d(k) (the sum running in k order), 1 where that sum is 0: silence is unvoiced, not NaN;
 *   pick = the smallest tau in [tau_min, tau_max) with c(tau) < threshold, then tau + 1 while tau + 1 < tau_max and c(tau + 1) < c(tau);
 *   with a, b, c = c(pick - 1), c(pick), c(pick + 1): offset = 0.5 (a - c) / (a - 2 b + c) if that denominator is > 0 and b <= a and b <= c,
 *   else 0;  period = pick + offset, aperiodicity = b.  No tau under the threshold: period = 0, aperiodicity = 1 (no global-minimum fallback).
 * 1 <= W <= DS_YIN_MAX_W, hop >= 1, 2 <= tau_min < tau_max <= DS_YIN_MAX_TAU, 0 < threshold < 1.  No atomics; a frame's outputs are the same
 * bits whatever shares the batch.
 * ds_pitch_median: per signal (rows FOFF, NF of the same table) the LOWER median of the periods > 0 — the element of rank (n_voiced - 1) / 2,
 * one of the input values bit for bit — and n_voiced; 0 and 0 when nothing is voiced.  NF <= DS_PITCH_MAX_FRAMES. */
#define DS_YIN_XOFF 0
#define DS_YIN_LEN 1
#define DS_YIN_FOFF 2
#define DS_YIN_NF 3
#define DS_YIN_NI 4
#define DS_YIN_MAX_W 2048
#define DS_YIN_MAX_TAU 1024
#define DS_PITCH_MAX_FRAMES 8192
int ds_yin_frames(const float* x, const int32_t* tab, int n_signals, int max_frames, long long total_samples, long long total_frames,
                  int frame_length, int hop, int tau_min, int tau_max, float threshold, float* period, float* aperiodicity, void* stream);
int ds_pitch_median(const float* period, const int32_t* tab, int n_signals, int max_frames, long long total_frames, float* median,
                    int32_t* voiced, void* stream);

/* ---------------------------------------------------------------- sample-rate conversion (csrc/resample_poly.hip), fp32
 * ds_resample_poly: scipy.signal.resample_poly(x, up, down) with its defaults (window ("kaiser", 5.0), padtype "constant") — which is
 * librosa.resample(res_type="polyphase") and what tools.adjust_audio_length (tools.py:126-151) means in this package — fused with its crop /
 * zero-pad (librosa.util.fix_length), for a ragged batch whose signals may each have their own rate pair.  With g = gcd(orig_sr, target_sr),
 * UP = target_sr / g, DOWN = orig_sr / g, HALF = 10 max(UP, DOWN), fc = 1 / max(UP, DOWN), the filter has 2 HALF + 1 taps
 *   h[k] = UP s[k] w[k] / sum_j s[j] w[j],  s[k] = fc sinc(fc (k - HALF)),  w[k] = I0(5 sqrt(1 - ((k - HALF) / HALF)^2)) / I0(5)
 * designed by the caller in float64 and rounded to fp32 once, and
 *   y[m] = sum_n x[n] h[HALF + m DOWN - n UP]  over 0 <= n < LEN with the tap index inside [0, 2 HALF],  0 <= m < NRES = ceil(LEN UP / DOWN).
 * A signal is row s of tab, a device array [n_signals][DS_RP_NI] int32 (offsets and counts in ELEMENTS):
 *   XOFF, LEN    its samples in x
 *   OOFF, OLEN   its output in out: out[m] = y[m] for m < min(OLEN, NRES), 0 for NRES <= m < OLEN (OLEN is the fix_length target)
 *   NRES         ceil(LEN UP / DOWN), computed by the caller in integers
 *   UP, DOWN, HALF   its rate pair; any HALF >= 1 with 2 HALF + 1 <= max_taps is legal (the taps are the caller's)
 *   HOFF         its 2 HALF + 1 taps in filt (rows of one rate pair share them)
 *   BLK          the outputs one block of the launch owns, 1 <= BLK <= DS_RP_MAX_BLK, chosen by the caller so that the inputs of BLK
 *                consecutive outputs — at most ((BLK - 1) DOWN + 2 HALF) / UP + 2 samples — number at most `span`
 * max_blocks = the largest ceil(OLEN / BLK) of the batch, max_taps >= every row's 2 HALF + 1 (<= DS_RP_MAX_TAPS), span <= DS_RP_MAX_SPAN;
 * the launch uses (max_taps + span) * 4 bytes of LDS per block.  Every element of a row's output is written and nothing outside it; a row that
 * does not fit the stated totals, max_taps or span reads and writes nothing.  The products m DOWN and n UP are formed in 64 bits.  Per output
 * the taps are walked in ascending tap index (descending n) as acc = fma(x[n], h[k], acc) from acc = 0: a fixed order, no atomics, so a
 * signal's output is the same bits whatever else is in the launch, and an impulse returns the fp32 taps themselves. */
#define DS_RP_XOFF 0
#define DS_RP_LEN 1
#define DS_RP_OOFF 2
#define DS_RP_OLEN 3
#define DS_RP_NRES 4
#define DS_RP_UP 5
#define DS_RP_DOWN 6
#define DS_RP_HALF 7
#define DS_RP_HOFF 8
#define DS_RP_BLK 9
#define DS_RP_NI 10
#define DS_RP_MAX_TAPS 16384
#define DS_RP_MAX_SPAN 20480
#define DS_RP_MAX_BLK 1024
int ds_resample_poly(const float* x, const int32_t* tab, const float* filt, int n_signals, int max_blocks, int max_taps, int span,
                     long long total_in, long long total_out, long long total_filt, float* out, void* stream);

/* ---------------------------------------------------------------- timbre encoder (timbre_encoder_pretrain.py:39,71,81-84), fp32
 * One nn.LSTM layer over a whole sequence, h0 = c0 = 0:  c' = sigmoid(f) c + sigmoid(i) tanh(g),  h' = sigmoid(o) tanh(c')  with
 * [i f g o][b][t] = pre[b][t] + h[b][t-1] w_hh^T.  pre [B][T][4H] = x W_ih^T + b_ih + b_hh comes from the caller (one ds_linear over all B T rows;
 * element (b, t, j) at pre[b * pre_batch_stride + t * pre_step_stride + j]), w_hh [4H][H] is nn.LSTM's weight_hh_l*.  Writes the hidden
 * sequence hs [B][T][H] (NULL: not wanted) and its last step h_last [B][H].  ws: ds_lstm_ws_floats(B, H) floats (c and two buffers of h), need
 * not be initialised.  H % 16 == 0, any B, T >= 1.  The call enqueues T launches on `stream` and returns: stream order is the only dependence
 * between steps, so no launch holds more than one step and no block waits for another.  The summation order over k of an output (b, unit) does
 * not depend on B: a sample's result is the same bits whatever shares its batch. */
size_t ds_lstm_ws_floats(int B, int H);
int ds_lstm_layer(const float* pre, long long pre_batch_stride, long long pre_step_stride, const float* w_hh, int B, int T, int H, float* hs,
                  float* h_last, float* ws, void* stream);
/* The four classifier heads on one stacked [B][y_stride] matrix of logits, in place: log-softmax over columns [0, n0), [n0, n0 + n1) and
 * [n0 + n1, n0 + n1 + n2), each by itself, and sigmoid over the n3 columns that follow. */
int ds_timbre_heads(float* y, int y_stride, int B, int n0, int n1, int n2, int n3, void* stream);

/* ---------------------------------------------------------------- CLAP text tower (RoBERTa-base encoder, pooler, projection), fp32
 * The dense layers and the post-LN residuals are ds_linear / ds_add_layernorm / ds_activation; these are the launches they do not cover
 * (csrc/clap_text.hip).  No result below depends on what else is in the batch.
 *
 * x[b * S + s][:] = LayerNorm(word[id] + pos[pid] + type0) * gamma + beta over H (biased variance, eps inside the sqrt), id = input_ids[b][s]
 * (device memory) and pid = pad_id + #{s' <= s : input_ids[b][s'] != pad_id} if id != pad_id, else pad_id: RoBERTa's position rule, a
 * function of input_ids alone.  word [V][H], pos [P][H], type0 [H].  The ids live on the device, so the call cannot see them: a row whose id
 * is outside [0, V) or whose position is outside [0, P) is filled with NaN, and no table is read out of bounds. */
int ds_text_embed(const int64_t* input_ids, int B, int S, int pad_id, const float* word, int V, const float* pos, int P, const float* type0,
                  const float* gamma, const float* beta, int H, float eps, float* x, void* stream);
/* ctx[b * S + q][h * d : (h + 1) * d] = softmax_k(q . k * d^-0.5 + mask_k) v per (sample, head, query), bidirectional, from the stacked rows
 * qkv [B * S][3H] = q | k | v with H = heads * d.  mask [B][S] of uint8 (mask_bytes 1) or int32 (mask_bytes 4), nonzero = attend, NULL = all
 * ones: a masked key has probability exactly 0 and takes no part in the maximum; a query with every key masked gives zeros.
 * 1 <= S <= 512, d a multiple of 4 up to 128.  The bits of a query's output do not depend on S or on the rest of the batch as long as the
 * extra keys are masked: a prompt alone and the same prompt padded inside a batch give equal rows. */
int ds_text_attention(const float* qkv, const void* mask, int mask_bytes, int B, int S, int heads, int d, float* ctx, void* stream);
/* The tower's tail, [B][D] rows, in place allowed: DS_TAIL_TANH (the pooler) and DS_TAIL_RELU (the projection) elementwise, eps unused;
 * DS_TAIL_L2NORM: out[b][:] = x[b][:] / max(||x[b]||_2, eps), so an all-zero row stays zero. */
#define DS_TAIL_TANH 0
#define DS_TAIL_RELU 1
#define DS_TAIL_L2NORM 2
int ds_text_tail(const float* x, int B, int D, int op, float eps, float* out, void* stream);

/* ---------------------------------------------------------------- the Inpaint tab's latent mask (csrc/inpaint_mask.hip)
 * What webUI/natural_language_guided_4/inpaint_with_text.py:204-233 does on the host with numpy and scipy.ndimage.zoom: the drawn layers to
 * the mask DiffSynthSampler.inpaint_sample takes, for a ragged batch of masks, one launch per stage.  A mask is row s of tab, a device array
 * [n_masks][DS_IM_NI] int32 (offsets and counts in ELEMENTS):
 *   LOFF, NL     its NL layers [H][W][4] uint8, back to back from PIXEL LOFF of layers (ds_mask_layers; NL = 0: the caller has put its
 *                plane in place and ds_mask_layers leaves it alone)
 *   POFF, H, W   its binary plane [H][W] uint8 in planes and its float64 coefficients in both halves of ws;  H, W >= 2
 *   OOFF, HO, WO its latent plane [HO][WO] in out (and pre);  HO = round(H / VAE_scale), WO = round(W / VAE_scale) with Python's round
 *                (half to even), computed by the caller;  HO, WO >= 2
 *   R0, R1, C0, C1   the rectangle set to 1, rows [R0, R1) and columns [C0, C1) of the UNFLIPPED plane: the caller resolves
 *                mask[int(fb):int(fe), int(tb tr / (4 VAE_scale)):int(te tr / (4 VAE_scale))] with slice(a, b).indices(n)
 *   INV          1: the area is "masked", the plane is 1 - mask
 * A row that does not fit the stated totals, or has H, W, HO or WO below 2, reads and writes nothing.
 *
 * ds_mask_layers (:205-206, :214): plane = any layer's alpha > 0 (for uint8 what mean(layers)[:, :, -1] > 0 is) as 0 / 1.  16-byte loads of
 * four pixels where LOFF, POFF and H W are multiples of 4, single pixels otherwise.  max_px = the largest H W of the batch.
 *
 * ds_mask_prefilter (:218, the first half of zoom): scipy.ndimage's cubic B-spline prefilter of the plane, float64, along axis 0 and then
 * along axis 1, whole-sample mirror boundary, pole z = sqrt(3) - 2, gain 6 per axis — spline_filter1d(x, 3, mode="mirror").  A line is
 * cut into independent segments of 16 samples: c+[j] = 6 e[j] + z c+[j-1] from zero over the mirror-extended line e, from DS_IM_RUN_IN
 * samples in front of the segment to DS_IM_RUN_IN behind it; c[s1] = -sum_k z^(k+1) c+[s1 + k] over the samples behind; downwards
 * c[j] = z (c[j+1] - c+[j]).  What the missing history contributes is below |z|^DS_IM_RUN_IN = 1.3e-23 of the data.
 * ws: ds_mask_ws_bytes(total_px) bytes = [2][total_px] float64; the coefficients are its second half.
 *
 * ds_mask_zoom (:218-233, the second half of zoom onwards): output (i, j) of the unflipped plane reads the coefficients at
 * x = i ((H - 1) / (HO - 1)), y = j ((W - 1) / (WO - 1)) (the ratio formed first, as scipy forms it): 4 x 4 taps at floor - 1 ... floor + 2,
 * cubic B-spline weights 2/3 - t^2 + |t|^3 / 2 (|t| < 1), (2 - |t|)^3 / 6 (1 <= |t| < 2), tap indices mirrored (-1 -> 1, n -> n - 2), all in
 * float64.  scipy's mode "constant": an output whose coordinate is outside the input, x < 0 or x > H - 1 (y likewise), is cval = 0 — for
 * about one size in ten (30, 63, 120, 252, 416 ...) the LAST output's product (HO - 1) ((H - 1) / (HO - 1)) rounds an ulp above H - 1, and
 * the whole last row (or column) of the zoomed mask is 0.  The reference zooms the INT64 mask, so scipy rounds the value half away from zero (v > 0 ? floor(v + 0.5) : ceil(v - 0.5)) to
 * -1 ... 2 and np.clip makes it 0 / 1: the mask is binary.  Then the rectangle, 1 - m if INV, and the flip:
 * out[OOFF + (HO - 1 - i) WO + j] as fp32 — one (1, 1, HO, WO) plane per mask, which the sampler broadcasts over batch and channels.
 * pre (NULL: not wanted) receives the float64 value before rounding at [OOFF + i WO + j].  max_out_px = the largest HO WO of the batch. */
#define DS_IM_LOFF 0
#define DS_IM_NL 1
#define DS_IM_POFF 2
#define DS_IM_H 3
#define DS_IM_W 4
#define DS_IM_OOFF 5
#define DS_IM_HO 6
#define DS_IM_WO 7
#define DS_IM_R0 8
#define DS_IM_R1 9
#define DS_IM_C0 10
#define DS_IM_C1 11
#define DS_IM_INV 12
#define DS_IM_NI 13
#define DS_IM_RUN_IN 40
int ds_mask_layers(const uint8_t* layers, const int32_t* tab, int n_masks, int max_px, long long total_layer_px, long long total_px,
                   uint8_t* planes, void* stream);
size_t ds_mask_ws_bytes(long long total_px);
int ds_mask_prefilter(const uint8_t* planes, const int32_t* tab, int n_masks, int max_h, int max_w, long long total_px, double* ws,
                      void* stream);
int ds_mask_zoom(const double* ws, const int32_t* tab, int n_masks, int max_out_px, long long total_px, long long total_out, float* out,
                 double* pre, void* stream);

/* ---------------------------------------------------------------- mastering: RMS gain and peak-hold limiter (csrc/master.hip), fp32
 * The stage behind the sum of the arranger's tracks, for a ragged batch: a signal is row s of tab, the arranger's [n_signals][DS_PV_NI]
 * int32 table, of which XOFF and LEN are read (its samples in x, and in out / pcm).  1 <= LEN <= DS_MS_MAX_LEN.  Per signal x[0..N), with
 * the scalars target_rms, max_gain and the ceiling c computed by the caller in float64 and rounded to fp32 once, A = lookahead and
 * R = hold in SAMPLES (floored by the caller), 0 <= A <= R:
 *   1 gain      rms = sqrt(sum x^2 / N), squares and sum in float64 (a square of an fp32 value is exact there);
 *               gL = fp32(min(target_rms / rms, max_gain)), 1.0 exactly for target_rms <= 0 (none); silence: rms = 0, gL = max_gain;
 *               peak = max |x|.
 *   2 required  u[n] = fl(gL x[n]);  r[n] = fl(c / |u[n]|) where |u[n]| > c, else 1 (IEEE fp32 division);  r = 1 outside [0, N).
 *   3 hold      m[j] = min r[k] over j - R <= k <= j + A, for -A <= j <= N - 1 + A.
 *   4 smooth    g[n] = fp32((sum of m[j], n - A <= j <= n + A, in float64) / (2 A + 1)), the division in float64.  Every window of step 3
 *               that the sum reads contains n (R >= A), so every m[j] <= r[n] and g[n] <= r[n].  With |u| <= 2^18 c and A <= 1024 every
 *               partial sum is exact in float64 (12 + 18 + 23 = 53 bits): the order of the sum changes no bit.  Where nothing within reach
 *               is over the ceiling the sum is 2 A + 1 ones and g = 1 exactly.
 *   5 apply     y[n] = fl(g[n] u[n]), then y > c -> c, y < -c -> -c (comparisons: a NaN stays a NaN).  fl(c / |u|) |u| can exceed c by
 *               one ulp; the clamp moves a sample by no more than that.  No product is contracted into an FMA.
 *   6 pcm       pcm[n] = int16(rint(fl(y[n] 32767))), half to even; c <= 1, so nothing overflows.
 *   7 stats     stats [n_signals][DS_MS_NS] fp32: GAIN = gL, RMS = fp32(rms), PEAK, MIN_GAIN = min g[n] (1 where nothing was limited);
 *               limited [n_signals] int32 = #{n : g[n] < 1}.  The last two go through integer atomics only (the bit pattern of a
 *               non-negative float, an int add): deterministic.
 * Non-finite samples are not checked (their effect on the values is unspecified); nothing is read or written out of bounds.
 *
 * ds_master_gain: steps 1 and the initial MIN_GAIN = 1, limited = 0.  Signal s is reduced by nb = clamp(ceil(N / DS_MS_CHUNK), 1,
 * DS_MS_MAX_PARTS) blocks of 256 threads (thread t of block b: samples b 256 + t, + nb 256, ... in that order), the partials (float64 sum,
 * fp32 max) go to ws and one block per signal adds them in a fixed order: the order depends on N alone, so gL is the same bits for a signal
 * alone and inside any batch.  ws: ds_master_ws_bytes(n_signals, max_len) bytes, 8-byte aligned, need not be initialised.
 *
 * ds_master_limit: steps 2-7 in one launch, grid (tiles of DS_MS_TILE output samples, signal); a block beyond its signal's last tile exits.
 * A block of tile [t0, t0 + T) stages r over [t0 - A - R, t0 + T - 1 + 2 A] in LDS (computed from x and GAIN as it loads), turns it in
 * place into minima over 2^k samples by doubling, stages m over [t0 - A, t0 + T - 1 + A] as the minimum of two of them, then forms g by
 * the direct 2 A + 1-term sum, applies it and stores.  LDS: 4 (T + R + 3 A) + 4 (T + 2 A) bytes, 86 016 at the caps.  pcm may be NULL.
 * out may not alias x (a tile reads its neighbours' inputs).  lookahead <= DS_MS_MAX_LOOKAHEAD, lookahead <= hold <= DS_MS_MAX_HOLD,
 * 0 < ceiling <= 1, else DS_EINVAL.
 * Both: every element of a fitting signal's output (and its stats row) is written and nothing outside it; a row that does not fit
 * total_samples or has LEN outside [1, DS_MS_MAX_LEN] reads and writes nothing. */
#define DS_MS_GAIN 0
#define DS_MS_RMS 1
#define DS_MS_PEAK 2
#define DS_MS_MIN_GAIN 3
#define DS_MS_NS 4
#define DS_MS_TILE 4096
#define DS_MS_MAX_LOOKAHEAD 1024
#define DS_MS_MAX_HOLD 8192
#define DS_MS_MAX_LEN 16777216
#define DS_MS_CHUNK 2048
#define DS_MS_MAX_PARTS 512
size_t ds_master_ws_bytes(int n_signals, int max_len);
int ds_master_gain(const float* x, const int32_t* tab, int n_signals, int max_len, long long total_samples, float target_rms, float max_gain,
                   void* ws, float* stats, int32_t* limited, void* stream);
int ds_master_limit(const float* x, const int32_t* tab, int n_signals, int max_len, long long total_samples, float ceiling, int lookahead,
                    int hold, float* stats, int32_t* limited, float* out, int16_t* pcm, void* stream);

/* ---------------------------------------------------------------- loudness: K-weighted gated loudness, BS.1770 (csrc/loudness.hip)
 * One mono signal x[0..N) in fp32 at an integer rate fs >= 8000, for the ragged batch of the mastering stage (row s of tab: XOFF, LEN,
 * 1 <= LEN <= DS_MS_MAX_LEN; and DS_LU_TAB_BOFF where the block energies are wanted).  Everything below is in float64.
 *   K-weighting  two biquads, re-derived for fs from the analogue prototypes in the form libebur128 and pyloudnorm use, computed by the
 *                host once:
 *                stage 1 (shelf)      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196,
 *                                     K = tan(pi f0 / fs), Vh = 10^(G / 20), Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2,
 *                                     b = [(Vh + Vb K / Q + K^2) / a0, 2 (K^2 - Vh) / a0, (Vh - Vb K / Q + K^2) / a0],
 *                                     a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0];
 *                stage 2 (high-pass)  f0 = 38.13547087602444, Q = 0.5003270373238773, K = tan(pi f0 / fs), d = 1 + K / Q + K^2,
 *                                     b = [1, -2, 1], a = [1, 2 (K^2 - 1) / d, (1 - K / Q + K^2) / d].
 *                At 48 kHz these are the standard's table to its 14 published digits.  y = x through stage 1, then stage 2, from zero
 *                state (transposed direct form II, as scipy.signal.lfilter).
 *   blocks       h = (fs + 5) / 10 samples (integer division: libebur128's 100 ms);  q_i = sum of y[n]^2 over [i h, (i + 1) h);
 *                block j covers 4 h samples from j h:  z_j = ((q_j + q_j+1) + (q_j+2 + q_j+3)) / (4 h);  nb = max(0, N / h - 3) blocks,
 *                only those that lie wholly inside the signal;  l_j = -0.691 + 10 log10 z_j.
 *   gates        both decided in the energy domain, no logarithm takes part in a decision:  z_abs = 10^((-70 + 0.691) / 10) (the host's);
 *                J1 = {j : z_j > z_abs};  z_rel = 0.1 mean(z_j, j in J1) (0 where J1 is empty);  J2 = {j in J1 : z_j > z_rel};
 *                Z = mean(z_j, j in J2);  integrated loudness L = -0.691 + 10 log10 Z;  the relative threshold in LUFS is
 *                -0.691 + 10 log10 z_rel;  the momentary maximum is max l_j over ALL blocks.  J2 empty (no block, or none above -70):
 *                Z = 0 and L = -inf;  every logarithm of 0 is -inf.
 *   sums         float64 in a fixed order that depends on N and fs alone; no float atomics: a signal has the same bits alone and inside
 *                any batch.
 *   gain         zt = 10^((target_lufs + 0.691) / 10) (the host's, float64);  gL = fp32(min(sqrt(zt / Z), max_gain)), IEEE division and
 *                square root, so gL is exact given Z;  Z = 0: gL = 1.0 exactly (nothing measurable, nothing changed).
 *
 * ds_loudness.  coef: DS_LU_NCOEF float64 values in HOST memory (they travel as a kernel argument):  stage 1's b at DS_LU_C_B1 (3) and
 * a[1], a[2] at DS_LU_C_A1, stage 2's at DS_LU_C_B2 / DS_LU_C_A2, then 4 x 4 row-major powers of the one-sample zero-input transition M of
 * the state (s1[0], s1[1], s2[0], s2[1]) of the transposed form,
 *     M = [[-a1[1], 1, 0, 0], [-a1[2], 0, 0, 0], [b2[1] - a2[1] b2[0], 0, -a2[1], 1], [b2[2] - a2[2] b2[0], 0, -a2[2], 0]]:
 * with Lc = ceil(h / DS_LU_THREADS) | 1 (odd), nc = ceil(h / Lc) and Lt = h - (nc - 1) Lc:  M^Lt at DS_LU_C_PTAIL, M^h at DS_LU_C_PHOP and
 * M^(Lc 2^k), k = 0 .. DS_LU_SCAN_STEPS - 1, at DS_LU_C_PSCAN + 16 k.  The recursion is linear, so it is cut exactly: a hop is a block, a
 * thread runs one chunk of Lc samples (the last one Lt) from zero state, a scan with the M^(Lc 2^k) carries the end states along the hop, one
 * wave per signal carries the hops' end states along the signal with M^h, and every chunk runs again from its true start state and adds its
 * squares.  This is the algebraic carry, not a warm-up: nothing is truncated.  Four launches (hops, carry, hops, gates); a batch in which no
 * signal has four hops takes the last one only.
 * ws: ds_loudness_ws_bytes(n_signals, max_len, h) bytes (0: bad arguments), 8-byte aligned, need not be initialised.
 * lu [n_signals][DS_LU_NS] float64: ENERGY = Z, INTEGRATED, MOMENTARY_MAX, THRESHOLD.  cnt [n_signals][3] int32: nb, |J1|, |J2|.
 * blocks (may be NULL): float64 [total_blocks], z_j of signal s at blocks[tab[s][DS_LU_TAB_BOFF] + j], j < nb.
 * DS_LU_MIN_HOP <= h <= DS_LU_MAX_HOP, z_abs >= 0 and finite, every coef finite, else DS_EINVAL.  Every lu / cnt entry of a fitting row and
 * exactly nb entries of its blocks are written, and nothing outside them; a row that does not fit total_samples (or, with blocks, whose
 * blocks do not fit total_blocks) or has LEN outside [1, max_len] reads and writes nothing.
 *
 * ds_loudness_gain: stats[s][DS_MS_GAIN] = gL from lu[s][DS_LU_ENERGY], behind a ds_master_gain call made with no RMS target; it touches
 * nothing else of stats.  zt and max_gain positive and finite, else DS_EINVAL. */
#define DS_LU_ENERGY 0
#define DS_LU_INTEGRATED 1
#define DS_LU_MOMENTARY_MAX 2
#define DS_LU_THRESHOLD 3
#define DS_LU_NS 4
#define DS_LU_TAB_BOFF 2
#define DS_LU_THREADS 256
#define DS_LU_MIN_HOP 800
#define DS_LU_MAX_HOP 19200
#define DS_LU_C_B1 0
#define DS_LU_C_A1 3
#define DS_LU_C_B2 5
#define DS_LU_C_A2 8
#define DS_LU_C_PTAIL 16
#define DS_LU_C_PHOP 32
#define DS_LU_C_PSCAN 48
#define DS_LU_SCAN_STEPS 8
#define DS_LU_NCOEF 176
size_t ds_loudness_ws_bytes(int n_signals, int max_len, int h);
int ds_loudness(const float* x, const int32_t* tab, int n_signals, int max_len, long long total_samples, const double* coef, int h, double z_abs,
                void* ws, double* lu, int32_t* cnt, double* blocks, long long total_blocks, void* stream);
int ds_loudness_gain(const double* lu, int n_signals, double zt, float max_gain, float* stats, void* stream);

/* ---------------------------------------------------------------- true peak: 4x meter and limiter detector, BS.1770 Annex 2 (csrc/true_peak.hip)
 * One mono signal x[0..N) in fp32, x = 0 outside [0, N), for the ragged batch of the mastering stage (row s of tab: XOFF, LEN).  The
 * oversampling factor is 4 at every rate.
 *   interpolator  libebur128's 49-tap, Hann-windowed sinc, restated without its delay:
 *                 c(d) = sinc(d / 4) (1 + cos(2 pi d / 48)) / 2 for integer |d| <= 24, sinc(t) = sin(pi t) / (pi t), c(0) = 1.
 *                 c(4 k) = 0 for k != 0: the phase at the sample instants is the identity and is never computed.
 *                 h[p][k] = fp32(c(4 (5 - k) + p)), p = 1, 2, 3, k = 0 .. 11, computed by the host in float64 and rounded once:
 *                 DS_TP_NCOEF = 36 fp32 values in HOST memory, row p - 1 at coef + (p - 1) DS_TP_TAPS (they travel as a kernel argument).
 *                 h[3][k] = h[1][11 - k], and h[2] is symmetric.
 *   inter-sample  v_p(n) = sum over k = 0 .. 11 of (double)h[p][k] (double)x[n - 5 + k], for n = -1 .. N - 1: the waveform at time
 *                 n + p / 4.  Every product is exact in float64; the sum runs in ascending k, one rounding per add, no product is
 *                 contracted into an FMA.  iv(n) = max over p of |v_p(n)|.
 *   envelope      e[n] = fp32(max(|x[n]|, iv(n - 1), iv(n))): the largest magnitude of the interpolated waveform on the open interval
 *                 (n - 1, n + 1).  The rounding is monotone, so it commutes with the maximum.
 *   true peak     TP = max e[n] over 0 <= n < N, fp32.  dBTP = 20 log10 TP is the caller's to compute.
 *   limiter       ds_master_limit_tp: step 2 of the mastering stage becomes r[n] = fl(c / d[n]) where d[n] = fl(gL e[n]) > c, else 1, with
 *                 e the envelope of the INPUT x; steps 3-7 are unchanged and on u = fl(gL x).  e[n] >= |x[n]|, so d[n] >= |u[n]|, and
 *                 g <= r still bounds the SAMPLE peak by c; the bits still have one right answer.  The detector gives no exact bound on the
 *                 output's true peak (a time-varying gain does not commute with the interpolator): that is measured, not promised
 *                 (DESIGN 7r).
 * Non-finite samples are not checked (their effect on the values is unspecified); nothing is read or written out of bounds.
 *
 * ds_true_peak: grid (tiles of DS_TP_TILE samples, signal).  A block of tile [t0, t0 + T) stages x over [t0 - 6, t0 + T + 6) in LDS, computes
 * iv(n), t0 - 1 <= n <= t0 + T - 1, into a second LDS tile, and after one barrier e[n]; the block's maximum goes to ws and one block per
 * signal takes the maximum of its tiles' (a maximum has no order: tp[s] is the same bits alone and inside any batch).  env may be NULL (the
 * meter alone); it may not alias x.  ws: ds_true_peak_ws_bytes(n_signals, max_len) bytes (0: bad arguments), 4-byte aligned, need not be
 * initialised.  Every coef finite, else DS_EINVAL.  tp[s] and, with env, every e[n] of a fitting row are written and nothing else; a row
 * that does not fit total_samples or has LEN outside [1, max_len] reads and writes nothing.
 * ds_master_limit_tp: ds_master_limit with env, the [total_samples] fp32 envelope that ds_true_peak wrote for the same x and tab, as the
 * detector; the same checks, LDS and grid; out may alias neither x nor env. */
#define DS_TP_TILE 2048
#define DS_TP_PHASES 3
#define DS_TP_TAPS 12
#define DS_TP_NCOEF 36
size_t ds_true_peak_ws_bytes(int n_signals, int max_len);
int ds_true_peak(const float* x, const int32_t* tab, int n_signals, int max_len, long long total_samples, const float* coef, float* env, void* ws,
                 float* tp, void* stream);
int ds_master_limit_tp(const float* x, const float* env, const int32_t* tab, int n_signals, int max_len, long long total_samples, float ceiling,
                       int lookahead, int hold, float* stats, int32_t* limited, float* out, int16_t* pcm, void* stream);

#ifdef __cplusplus
}
#endif
#endif
