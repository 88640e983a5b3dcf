// ConvTranspose2d(C, C, 4, 2, 1) with C = 80 channels (bf16 NHWC): the VQGAN decoder's last Upsample, 256 x 128 -> 512 x 256 per clip.
// reference: model/VAE VQGAN.py Decoder: the `up` layers = nn.ConvTranspose2d(cur, nxt, 4, 2, 1) (tail row).
//
// 80 channels fit none of the 32-channel-chunk kernels (the four-tap halo kernel wants chunks in sixes, the generic implicit GEMM pads
// K = 4 x 80 to 12 steps and gathers every operand per tap through registers: 1.38 ms = 311 TF for 0.27 ms worth of output bytes).
// Here a K step of 32 is TWO (tap, 16-channel group) pairs: 4 taps x 5 groups = 20 pairs = 10 steps exactly (conv_c80_parts.hpp has the
// K decomposition and every part shared with conv3x3_c80.hip).
//   phase   : output pixel (2i + py, 2j + px) = sum over a, b in {0, 1} of x[i + py - 1 + a][j + px - 1 + b] . w[.][.][3 - py - 2a][3 - px - 2b];
//             a block works on ONE phase (its 10 x 5 weight fragments, 50 KB, stay in LDS) and walks input tiles of 4 x 32 pixels; the four
//             phase blocks of a tile run are neighbours on one XCD (they read the same input through one L2)
//   input   : optionally relu(GroupNorm(G, 80)(x)) (the decoder's Normalize + ReLU in front of the layer): the per-(sample, group) affine is
//             applied to the loaded chunks on their way into LDS — the separate GroupNorm-apply pass (read + write of the input) disappears
//   LDS     : weights 50 KB (100 KB at 160 input channels) + ONE halo image of 5 x 33 pixels x 176 (336) bytes; a barrier releases the
//             image, the halo of the next tile is written, the output stores leave, a second barrier publishes it.  80 -> 80: two such
//             blocks per CU (79 KB each)
//   MFMA    : 5 x 8-byte stores per pixel; the four lanes of a pixel cover 32 contiguous bytes per store
#include <type_traits>

#include "conv_c80_parts.hpp"

namespace {

using U8A = C80Geom<5, 2, 4, false, 2>;   // 80 -> 80: 50 KB of weights + 29 KB, TWO blocks per CU — independent blocks overlap each other's MFMA,
                                          // staging and store phases (one 4-wave block per CU with 8-row tiles and two halo images: 0.78 ms against 0.55)
using U8B = C80Geom<10, 2, 4, false>;     // 160 -> 80: 100 KB of weights + 55 KB
static_assert(U8A::KS == 10 && U8A::HR == 5 && U8A::HC == 33 && U8B::KS == 20 && U8B::PIXB == 336, "the phase geometry");

struct U8Params : C80Params {       // x: [B][H][W][CI], out: [B][2H][2W][80] bf16; wpk: ds_pack_convt4x4_c80 ([4 phases] ...); the fused
    int runs;                       // activation is ReLU; 16 statistics slots per run (phase, wave); runs = B * rps
};

template <typename M>
__global__ __launch_bounds__(C80_NT, M::BPC) void convt4x4_c80_kernel(const U8Params p) {
    constexpr int RPW = M::RPW, NPT = M::NPT;
    extern __shared__ __attribute__((aligned(16))) char sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = lane & 15, kq = lane >> 4;
    // block -> (phase, tile run): hardware block L runs on XCD L % 8; the four phases of a run sit on one XCD
    const int L = blockIdx.x;
    const int phase = (L >> 3) & 3, rid = (L & 7) + 8 * (L >> 5);
    const int py = phase >> 1, px = phase & 1;
    if (rid >= p.runs) return;
    C80Run run;
    if (!c80_run(p, rid, 16, phase * 4 + wave, m, kq, run)) return;
    c80_stage_weights<M::WBYTES, 2>(sm, reinterpret_cast<const char*>(p.wpk) + (size_t)phase * M::WBYTES, tid);    // (this phase's)
    f32x4 bv[C80_NJ];
    c80_bias(p.bias, kq, bv);

    // the block's sample
    const char* const base = reinterpret_cast<const char*>(p.x) + (size_t)run.b * p.H * p.W * M::CI * 2;
    const c80_rsrc_t rs = c80_rsrc(base, p.H * p.W * M::CI * 2);
    bf16* const outb = reinterpret_cast<bf16*>(p.out) + (size_t)run.b * (2 * p.H) * (2 * p.W) * C80_CO;
    const bool gn = p.gn_ab != nullptr;
    const auto act = [](float v) { return fmaxf(v, 0.f); };

    C80Halo<M> halo;
    halo.init(tid);
    int i0, j0;
    c80_locate<M>(p, run.q0, i0, j0);
    halo.issue(p, base, rs, i0 + py - 1, j0 + px - 1);
    if (gn) halo.load_gn(p, run.b);
    halo.fill(sm + M::OFF_H, p, gn, i0 + py - 1, j0 + px - 1, act);
    __syncthreads();

    int xoff[M::KS];
    c80_xoff<M>(kq, xoff);
    const int xb = ((RPW * wave) * M::HC + m) * M::PIXB;
    C80Stats stats;
    stats.init();
    const char* const wl = sm + lane * 16;
    auto tile_body = [&](const int u, auto more_t) {
        constexpr bool more = decltype(more_t)::value;
        const char* const hcur = sm + M::OFF_H + (M::DB ? (u & 1) * M::HBYTES : 0);
        int ni = i0, nj = j0;
        if constexpr (more) {
            c80_locate<M>(p, run.q0 + u + 1, ni, nj);
            halo.issue(p, base, rs, ni + py - 1, nj + px - 1);
        }
        f32x4 acc[NPT][C80_NJ];
        c80_mma<M>(hcur + xb, wl, xoff, bv, acc);
        if constexpr (more) {
            if constexpr (!M::DB) __syncthreads();             // one halo image: every wave is done reading it
            halo.fill(sm + M::OFF_H + (M::DB ? ((u + 1) & 1) * M::HBYTES : 0), p, gn, ni + py - 1, nj + px - 1, act);   // (before the stores: see dwconv7_mfma2_kernel)
        }
        // ---- bf16, five 8-byte stores per pixel: lane = pixel m of each pixel tile, channels 16 j + 4 kq .. + 3
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int r = i0 + RPW * wave + (i >> 1), c = j0 + 16 * (i & 1) + m;
            if (r < p.H && c < p.W) {
                bf16* o = outb + ((size_t)(2 * r + py) * (2 * p.W) + (2 * c + px)) * C80_CO + 4 * kq;
#pragma unroll
                for (int j = 0; j < C80_NJ; ++j) {
                    bf16x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        v[e] = (bf16)acc[i][j][e];
                        stats.add(j, e, acc[i][j][e]);
                    }
                    DS_ST(bf16x4, reinterpret_cast<bf16x4*>(o + 16 * j), DS_BX_OUT, v);
                }
            }
        }
        if constexpr (M::DB || more) __syncthreads();          // next halo image complete (two images: and every wave is done with this one)
        i0 = ni;
        j0 = nj;
    };
    for (int u = 0; u + 1 < run.nt; ++u) tile_body(u, std::true_type{});
    tile_body(run.nt - 1, std::false_type{});
    if (run.sws) stats.finish(run.sws, m, kq);
}

// w [Cin][Cout = 80][4][4] fp32 (ConvTranspose2d layout) -> [phase][ks][j][lane = kg * 16 + row][8] bf16:
// row of tile j = output channel 16 j + row; k slot kg * 8 + e = pair 2 ks + (kg >> 1) = (tap, group g), input channel 16 g + 8 (kg & 1) + e,
// tap = 2 a + b -> kernel element (3 - py - 2 a, 3 - px - 2 b)
__global__ void pack_convt4x4_c80_kernel(const float* w, int Cin, bf16* dst) {
    const int NG = Cin / 16, KS = 4 * NG / 2;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 4 * KS * C80_NJ * 512) return;
    const int e = i & 7, lane = (i >> 3) & 63, j = (i >> 9) % C80_NJ, ks = (i / (512 * C80_NJ)) % KS, phase = i / (512 * C80_NJ * KS);
    const int row = lane & 15, kg = lane >> 4, py = phase >> 1, px = phase & 1;
    const int pidx = 2 * ks + (kg >> 1), tap = pidx / NG, g = pidx - tap * NG, a = tap >> 1, b = tap & 1;
    const int ci = 16 * g + 8 * (kg & 1) + e, co = 16 * j + row, kh = 3 - py - 2 * a, kw = 3 - px - 2 * b;
    dst[i] = (bf16)w[(((size_t)ci * C80_CO + co) * 4 + kh) * 4 + kw];
}

template <typename M>
static int u8_launch(const void* x, int B, int H, int W, const void* wpk, const float* bias, void* out, const float* gn_ab, int G,
                     const float* gamma, const float* beta, float* stats_ws, hipStream_t st) {
    U8Params p;
    c80_fill<M>(p, DS_K_CONVT4X4_C80, x, nullptr, B, H, W, wpk, (long long)4 * M::WBYTES, bias, out, (long long)B * 4 * H * W * C80_CO * 2, gn_ab, G, gamma,
                beta, stats_ws, 16, 64 * M::BPC, st);          // 64 runs x 4 phases = one block per CU (x BPC)
    p.runs = B * p.rps;
    // grid: block L = (run = (L & 7) + 8 (L >> 5), phase = (L >> 3) & 3); blocks beyond the last run return at once
    const int nb = 32 * ((p.runs + 7) / 8);
    DS_SET_MAX_LDS(convt4x4_c80_kernel<M>, M::LDS, "convt4x4_c80");
    hipLaunchKernelGGL(convt4x4_c80_kernel<M>, dim3(nb), dim3(C80_NT), M::LDS, st, p);
    DS_CHECK_LAUNCH("convt4x4_c80");
    return DS_OK;
}

}  // namespace

#if DS_BOUNDS
extern "C" int ds_bounds_fetch_convt4x4_c80(ds_bounds_rec* out, int reset) { return ds_bounds_fetch_tu(out, reset); }
#endif

extern "C" size_t ds_convt4x4_c80_weight_elems(int Cin) { return (size_t)4 * (4 * (Cin / 16) / 2) * C80_NJ * 512; }

extern "C" int ds_pack_convt4x4_c80(const float* w, int Cin, int Cout, void* dst, void* stream) {
    DS_REQUIRE(w && dst, "pack_convt4x4_c80: null pointer");
    DS_REQUIRE((Cin == 80 || Cin == 160) && Cout == C80_CO, "pack_convt4x4_c80: %d -> %d unsupported (80 or 160 -> 80)", Cin, Cout);
    const int n = (int)ds_convt4x4_c80_weight_elems(Cin);
    hipLaunchKernelGGL(pack_convt4x4_c80_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), w, Cin, reinterpret_cast<bf16*>(dst));
    DS_CHECK_LAUNCH("pack_convt4x4_c80");
    return DS_OK;
}

// slots of per-channel statistics partials per sample that ds_convt4x4_c80 writes (stats_ws = [B][slots][80][2] floats)
extern "C" int ds_convt4x4_c80_stats_slots(int B, int H, int W, int Cin) {
    int tw, th, rps, per;
    c80_partition(B > 0 ? B : 1, H, W, Cin == 160 ? U8B::TH : U8A::TH, 64 * (Cin == 160 ? U8B::BPC : U8A::BPC), tw, th, rps, per);
    return rps * 16;
}

extern "C" int ds_convt4x4_c80(const void* x, int B, int H, int W, int Cin, const void* wpk, const float* bias, void* out, const float* gn_ab, int G,
                               const float* gamma, const float* beta, float* stats_ws, void* stream) {
    DS_REQUIRE(x && wpk && out, "convt4x4_c80: null pointer");
    DS_REQUIRE(Cin == 80 || Cin == 160, "convt4x4_c80: %d input channels unsupported (80, 160)", Cin);
    DS_REQUIRE(!gn_ab || (gamma && beta && G > 0 && Cin % G == 0), "convt4x4_c80: the fused GroupNorm needs gamma, beta and a group count dividing %d (G = %d)", Cin, G);
    DS_REQUIRE(B > 0 && H > 0 && W > 0, "convt4x4_c80: bad sizes (B %d, %d x %d)", B, H, W);
    DS_REQUIRE((long long)H * W * Cin * 2 < (1ll << 28), "convt4x4_c80: a sample must stay below 256 MB");
    if (!ds_aligned16(x) || !ds_aligned16(wpk) || !ds_aligned16(out)) DS_FAIL(DS_EALIGN, "convt4x4_c80: pointers must be 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (Cin == 160) return u8_launch<U8B>(x, B, H, W, wpk, bias, out, gn_ab, G, gamma, beta, stats_ws, st);
    return u8_launch<U8A>(x, B, H, W, wpk, bias, out, gn_ab, G, gamma, beta, stats_ws, st);
}
