// 3x3 stride-1 pad-1 convolution with 80 -> 80 channels (bf16 NHWC) of the VQGAN decoder's 256 x 128 stage, as a whole ResnetBlock body:
//     out = x + conv3x3(act(GroupNorm(G, 80)(x)))                (VQGAN.py:223-244 with temb = None and no nin_shortcut)
// reference: model/VAE VQGAN.py ResnetBlock / Decoder (tail row).  Sibling of convt4x4_c80.hip — the shared parts and the K
// decomposition are in conv_c80_parts.hpp: 9 taps x 5 groups = 45 pairs = 23 steps (the 46th pair has zero weights).  On the generic
// implicit GEMM this block was three launches: GroupNorm apply + swish (0.35 ms: read + write of the 335 MB tensor), the convolution with
// the residual (0.71 ms at 341 TF).
//   input   : GroupNorm affine + swish / ReLU applied to the loaded chunks on their way into LDS (optional), zero padding after it
//   block   : persistent, 4 waves, output tile 4 rows x 32 columns (wave = one row = 2 pixel tiles x 5 channel tiles); the 23 x 5 weight
//             fragments (115 KB) stay in LDS for the block's whole run of tiles, ONE halo image of 6 x 34 pixels x 176 bytes beside them;
//             the halo of tile t+1 and the residual pixels of tile t are requested before the MFMAs of tile t, a barrier releases the
//             image, the halo is written, the outputs leave, a second barrier publishes the image
//   MFMA    : the residual (the RAW x) comes back as 8-byte loads in the store pattern
#include <type_traits>

#include "conv_c80_parts.hpp"

namespace {

using C8 = C80Geom<5, 3, 4, false>;                             // 115 KB of weights + 35 KB: one block per CU
static_assert(C8::PIXB == 176 && C8::QPP == 10 && C8::LT == 250 && C8::PPI == 25 && C8::KS == 23 && C8::LDS == 153664, "the 3x3 geometry");

typedef unsigned c8_u32x2 __attribute__((ext_vector_type(2)));

struct C8Params : C80Params {       // x, out: [B][H][W][80] bf16; wpk: ds_pack_conv3x3_c80; 4 statistics slots per run (one per wave)
    int act;            // of the fused GroupNorm: DS_ACT_*
    int add_x;          // 1: out += x (the block's residual)
    const void* res;    // residual source when it is not the convolution's input (ds_conv3x3_c80_res: x is the activated copy), else null
};

__global__ __launch_bounds__(C80_NT, C8::BPC) void conv3x3_c80_kernel(const C8Params p) {
    extern __shared__ __attribute__((aligned(16))) char sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = lane & 15, kq = lane >> 4;
    C80Run run;
    if (!c80_run(p, blockIdx.x, 4, wave, m, kq, run)) return;
    c80_stage_weights<C8::WBYTES, 4>(sm, p.wpk, tid);
    f32x4 bv[C80_NJ];
    c80_bias(p.bias, kq, bv);

    // the block's sample: input, residual source, output
    const int sbytes = p.H * p.W * C80_CO * 2;
    const char* const base = reinterpret_cast<const char*>(p.x) + (size_t)run.b * sbytes;
    const char* const rbase = p.res ? reinterpret_cast<const char*>(p.res) + (size_t)run.b * sbytes : base;
    const c80_rsrc_t rs = c80_rsrc(base, sbytes), rs_r = c80_rsrc(rbase, sbytes);
    bf16* const outb = reinterpret_cast<bf16*>(p.out) + (size_t)run.b * p.H * p.W * C80_CO;
    const bool gn = p.gn_ab != nullptr;
    const auto act = [&](float v) {
        if (p.act == DS_ACT_RELU) return fmaxf(v, 0.f);
        if (p.act == DS_ACT_SILU) return silu_fast(v);
        return v;
    };

    C80Halo<C8> halo;
    halo.init(tid);
    char* const himg = sm + C8::OFF_H;
    int i0, j0;
    c80_locate<C8>(p, run.q0, i0, j0);
    halo.issue(p, base, rs, i0 - 1, j0 - 1);
    if (gn) halo.load_gn(p, run.b);
    halo.fill(himg, p, gn, i0 - 1, j0 - 1, act);
    __syncthreads();

    int xoff[C8::KS];
    c80_xoff<C8>(kq, xoff);
    const char* const hx = himg + (wave * C8::HC + m) * C8::PIXB;
    C80Stats stats;
    stats.init();
    const char* const wl = sm + lane * 16;
    auto tile_body = [&](const int u, auto more_t) {
        constexpr bool more = decltype(more_t)::value;
        int ni = i0, nj = j0;
        if constexpr (more) {
            c80_locate<C8>(p, run.q0 + u + 1, ni, nj);
            halo.issue(p, base, rs, ni - 1, nj - 1);
        }
        // residual pixels of THIS tile (raw x), in the store pattern: channels 16 j + 4 kq .. + 3 of pixel (row, 16 i + m)
        const int r = i0 + wave;
        c8_u32x2 rx[2][C80_NJ];
        if (p.add_x) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int c = j0 + 16 * i + m;
                const unsigned bad = (unsigned)(r >= p.H) | (unsigned)(c >= p.W);
                const unsigned o = ((unsigned)((r * p.W + c) * C80_CO + 4 * kq) * 2u) & 0x0fffffffu;
#pragma unroll
                for (int j = 0; j < C80_NJ; ++j) {
#if DS_BOUNDS
                    if (bad || !ds_bx_ok(rbase + o + 32u * j, p.res ? DS_BX_RES : DS_BX_SRC0, 8)) { rx[i][j] = c8_u32x2{0u, 0u}; continue; }
#endif
                    rx[i][j] = __builtin_bit_cast(c8_u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_r, (int)((o + 32u * j) | (bad << 31)), 0, 0));
                }
            }
        }
        f32x4 acc[2][C80_NJ];
        c80_mma<C8>(hx, wl, xoff, bv, acc);
        if constexpr (more) {
            __syncthreads();                                   // every wave is done reading the halo image
            halo.fill(himg, p, gn, ni - 1, nj - 1, act);
        }
        // ---- (+ residual) bf16, five 8-byte stores per pixel
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = j0 + 16 * i + m;
            if (r < p.H && c < p.W) {
                bf16* o = outb + ((size_t)r * p.W + c) * C80_CO + 4 * kq;
#pragma unroll
                for (int j = 0; j < C80_NJ; ++j) {
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc[i][j][e];
                    if (p.add_x) {
                        v[0] += __uint_as_float(rx[i][j][0] << 16);
                        v[1] += __uint_as_float(rx[i][j][0] & 0xffff0000u);
                        v[2] += __uint_as_float(rx[i][j][1] << 16);
                        v[3] += __uint_as_float(rx[i][j][1] & 0xffff0000u);
                    }
                    bf16x4 o4;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        o4[e] = (bf16)v[e];
                        stats.add(j, e, v[e]);
                    }
                    DS_ST(bf16x4, reinterpret_cast<bf16x4*>(o + 16 * j), DS_BX_OUT, o4);
                }
            }
        }
        if constexpr (more) __syncthreads();                   // the next halo image is complete
        i0 = ni;
        j0 = nj;
    };
    for (int u = 0; u + 1 < run.nt; ++u) tile_body(u, std::true_type{});
    tile_body(run.nt - 1, std::false_type{});
    if (run.sws) stats.finish(run.sws, m, kq);
}

// w [Cout = 80][Cin = 80][3][3] fp32 (Conv2d layout) -> [ks][j][lane = kg * 16 + row][8] bf16: row of tile j = output channel 16 j + row;
// k slot kg * 8 + e = pair 2 ks + (kg >> 1) = (tap = 3 dy + dx, group g), input channel 16 g + 8 (kg & 1) + e; pair 45: zeros
__global__ void pack_conv3x3_c80_kernel(const float* w, bf16* dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C8::KS * C80_NJ * 512) return;
    const int e = i & 7, lane = (i >> 3) & 63, j = (i >> 9) % C80_NJ, ks = i / (512 * C80_NJ);
    const int row = lane & 15, kg = lane >> 4;
    const int pidx = 2 * ks + (kg >> 1), tap = pidx / C8::NG, g = pidx - tap * C8::NG;
    const int ci = 16 * g + 8 * (kg & 1) + e, co = 16 * j + row;
    float v = 0.f;
    if (pidx < C8::NP) v = w[((size_t)co * C80_CO + ci) * 9 + tap];
    dst[i] = (bf16)v;
}

}  // namespace

#if DS_BOUNDS
extern "C" int ds_bounds_fetch_conv3x3_c80(ds_bounds_rec* out, int reset) { return ds_bounds_fetch_tu(out, reset); }
#endif

extern "C" size_t ds_conv3x3_c80_weight_elems(void) { return (size_t)C8::KS * C80_NJ * 512; }

extern "C" int ds_pack_conv3x3_c80(const float* w, int Cout, int Cin, void* dst, void* stream) {
    DS_REQUIRE(w && dst, "pack_conv3x3_c80: null pointer");
    DS_REQUIRE(Cin == C80_CO && Cout == C80_CO, "pack_conv3x3_c80: %d -> %d unsupported (80 -> 80)", Cin, Cout);
    const int n = C8::KS * C80_NJ * 512;
    hipLaunchKernelGGL(pack_conv3x3_c80_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), w, reinterpret_cast<bf16*>(dst));
    DS_CHECK_LAUNCH("pack_conv3x3_c80");
    return DS_OK;
}

// slots of per-channel statistics partials per sample that ds_conv3x3_c80 writes (stats_ws = [B][slots][80][2] floats)
extern "C" int ds_conv3x3_c80_stats_slots(int B, int H, int W) {
    int tw, th, rps, per;
    c80_partition(B > 0 ? B : 1, H, W, C8::TH, 256, tw, th, rps, per);
    return rps * 4;
}

static int c80_launch(const void* x, const void* res, int B, int H, int W, const void* wpk, const float* bias, void* out, const float* gn_ab, int G,
                      const float* gamma, const float* beta, int act, int add_x, float* stats_ws, void* stream) {
    DS_REQUIRE(x && wpk && out, "conv3x3_c80: null pointer");
    DS_REQUIRE(B > 0 && H > 0 && W > 0, "conv3x3_c80: bad sizes (B %d, %d x %d)", B, H, W);
    DS_REQUIRE(!gn_ab || (gamma && beta && G > 0 && C80_CO % G == 0), "conv3x3_c80: the fused GroupNorm needs gamma, beta and a group count dividing 80 (G = %d)", G);
    DS_REQUIRE(act == DS_ACT_NONE || act == DS_ACT_RELU || act == DS_ACT_SILU, "conv3x3_c80: activation %d", act);
    DS_REQUIRE(x != out, "conv3x3_c80: in-place is not supported (neighbouring tiles read the input halo)");
    DS_REQUIRE((long long)H * W * C80_CO * 2 < (1ll << 28), "conv3x3_c80: a sample must stay below 256 MB");
    if (!ds_aligned16(x) || !ds_aligned16(wpk) || !ds_aligned16(out)) DS_FAIL(DS_EALIGN, "conv3x3_c80: pointers must be 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    C8Params p;
    c80_fill<C8>(p, DS_K_CONV3X3_C80, x, res, B, H, W, wpk, C8::WBYTES, bias, out, (long long)B * H * W * C80_CO * 2, gn_ab, G, gamma, beta, stats_ws, 4,
                 256, st);                                     // 256 blocks: about one per CU
    p.act = gn_ab ? act : DS_ACT_NONE;
    p.add_x = (add_x || res) ? 1 : 0;
    p.res = res;
    DS_SET_MAX_LDS(conv3x3_c80_kernel, C8::LDS, "conv3x3_c80");
    hipLaunchKernelGGL(conv3x3_c80_kernel, dim3(B * p.rps), dim3(C80_NT), C8::LDS, st, p);
    DS_CHECK_LAUNCH("conv3x3_c80");
    return DS_OK;
}

extern "C" int ds_conv3x3_c80(const void* x, int B, int H, int W, const void* wpk, const float* bias, void* out, const float* gn_ab, int G,
                              const float* gamma, const float* beta, int act, int add_x, float* stats_ws, void* stream) {
    return c80_launch(x, nullptr, B, H, W, wpk, bias, out, gn_ab, G, gamma, beta, act, add_x, stats_ws, stream);
}

// out = res + conv3x3(h) + bias for an input h that already IS act(GroupNorm(res)) (written by ds_gn_apply): the block as two launches.  r04: with
// the norm + swish applied while the halo is staged the kernel is bound by that arithmetic on a 1.59 x redundant halo and one wave per SIMD
// (637 us at 64 x 256 x 128 x 80); the plain convolution takes 377 us and the apply pass ~110.
extern "C" int ds_conv3x3_c80_res(const void* h, const void* res, int B, int H, int W, const void* wpk, const float* bias, void* out, float* stats_ws,
                                  void* stream) {
    DS_REQUIRE(res && res != out && ds_aligned16(res), "conv3x3_c80_res: bad residual pointer");
    return c80_launch(h, res, B, H, W, wpk, bias, out, nullptr, 0, nullptr, nullptr, DS_ACT_NONE, 1, stats_ws, stream);
}
